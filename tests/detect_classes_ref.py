"""Restatement of frcnn_detect_classes_batch (include/frcnn_hip.h) for the tests: no GPU, no library.

  lp: R x ncls fp32 log-probabilities of a frame's candidates; classes are 1-based, c = column + 1
  mode 0 (top)  c* = the FIRST maximum of the row, by cnet_decode_kernel's loop (best = 1; for c = 2 ...: lp[c] > lp[best] moves
                it -- a NaN never wins a comparison and is never displaced once it leads); the row (r, c*) is emitted iff
                c* != bgclass and exp((double)lp[c*]) > min_conf
  mode 1 (all)  a row (r, c) for EVERY c != bgclass with exp((double)lp[c]) > min_conf (a NaN emits nothing)
  order         candidate-major, c ascending
  a row j       cand[j] = r (0-based), cls[j] = c, conf[j] = lp[r, c - 1] (the fp32 value, bit for bit)
  total = the rows emitted; K = min(total, row_stride); the first K rows are stored

The decisions read exp() of the host libm where the device reads the HIP library's: both are within an ulp, so they agree on
every value whose exp does not lie within 1e-9 (relative) of the threshold -- threshold_margin() measures that distance, and
the host test asserts it for every generated problem.

The problems the GPU tests run are built here (problem()), so that their input conditions are asserted without a GPU."""
import math

import numpy as np

TOP, ALL = 0, 1


def first_max(lp):
    """0-based column of every row's first maximum, by cnet_decode_kernel's loop"""
    lp = np.asarray(lp, np.float32)
    rows = np.arange(len(lp))
    best = np.zeros(len(lp), np.int64)
    for j in range(1, lp.shape[1]):
        with np.errstate(invalid="ignore"):
            best = np.where(lp[:, j] > lp[rows, best], j, best)
    return best


def passes(lp, min_conf):
    """exp((double)lp) > min_conf, elementwise (a NaN does not pass)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(np.asarray(lp, np.float32).astype(np.float64)) > float(min_conf)


def detect_classes(lp, bgclass, min_conf, mode, row_stride=None):
    """-> dict(cand int32[K], cls int32[K], conf float32[K], total, K, per_candidate int[R] (rows every candidate emits))"""
    lp = np.asarray(lp, np.float32)
    R, ncls = lp.shape
    ok = passes(lp, min_conf)
    ok[:, bgclass - 1] = False
    if mode == TOP:
        top = np.zeros_like(ok)
        top[np.arange(R), first_max(lp)] = True
        ok &= top
    cand, col = np.nonzero(ok)          # (row-major: candidate-major, c ascending)
    total = len(cand)
    K = total if row_stride is None else min(total, row_stride)
    return dict(cand=cand[:K].astype(np.int32), cls=(col[:K] + 1).astype(np.int32), conf=lp[cand[:K], col[:K]], total=total, K=K,
                per_candidate=ok.sum(1))


def max_rows(ncls, min_conf):
    """m of Detector.scoring_rows under classes = "all": the rows a candidate can emit"""
    if min_conf <= 0:
        return ncls - 1
    return min(ncls - 1, int(math.floor(1.0 / min_conf)) + 1)


def threshold_margin(lp, min_conf):
    """the smallest |exp(lp) - min_conf| / min_conf over the finite entries (inf for min_conf = 0: exp(x) > 0 is decided by
    whether x is -inf, on which no two libraries differ for the values a test uses, all above -700)"""
    if min_conf <= 0:
        return math.inf
    v = np.asarray(lp, np.float32).astype(np.float64)
    v = v[np.isfinite(v)]
    return float(np.min(np.abs(np.exp(v) - min_conf)) / min_conf) if v.size else math.inf


def log_softmax32(z):
    """fp32 log-softmax of fp32 logits, one rounded operation per statement (what a net's last layer hands over)"""
    z = np.asarray(z, np.float32)
    z = z - z.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)


def problem(seed, R, ncls, spread=1.5, special=True, nan_row=False):
    """One frame: dict(lp R x ncls fp32 (a log-softmax; bgclass = ncls), bbox R x 4 fp32, rect n x 4 fp64 (n = R + 7 match rows),
    pick int64[R] (1-based rows of rect, a permutation's head)).  `spread` scales the logits: small -> the mass is shared by
    several classes.  special (R >= 4): row 0 has ALL its mass on the background (every foreground class -inf: fails at any
    threshold, also 0), row 1 a background arg-max of 0.56 beside a foreground class of 0.4 (the other foreground classes
    share 0.04; ncls = 2: 0.6 and 0.4), row 2 one foreground class at 1 (the others -inf), row 3 (nan_row) all NaN."""
    rng = np.random.RandomState(seed)
    lp = log_softmax32(rng.standard_normal((R, ncls)).astype(np.float32) * np.float32(spread))
    if special and R >= 4:
        lp[0] = -np.inf
        lp[0, ncls - 1] = 0.0
        f = seed % (ncls - 1)
        p = np.full(ncls, 0.04 / max(ncls - 2, 1), np.float64)
        p[ncls - 1], p[f] = (0.56, 0.4) if ncls > 2 else (0.6, 0.4)
        lp[1] = np.log(p).astype(np.float32)
        lp[2] = -np.inf
        lp[2, (seed + 1) % (ncls - 1)] = 0.0
        if nan_row:
            lp[3] = np.nan
    n = R + 7
    x0, y0 = rng.uniform(0, 150, n), rng.uniform(0, 100, n)
    rect = np.stack([x0, y0, x0 + rng.uniform(8, 60, n), y0 + rng.uniform(8, 60, n)], 1) + rng.uniform(-1, 1, (n, 4)) * 2.0 ** -20
    bbox = (rng.standard_normal((R, 4)) * 0.3).astype(np.float32)
    pick = (rng.permutation(n)[:R] + 1).astype(np.int64)
    return dict(lp=lp, bbox=bbox, rect=rect.astype(np.float64), pick=pick)


# the op-level cases of tests/test_gpu_detect_classes.py: R on both sides of a wave (64) and of a tile (1024), and more than two tiles
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2300)
NCLS = (2, 5, 17)
MIN_CONF = (0.0, 0.05, 0.2, 0.5)


def case_seed(R, ncls):
    return 1000 * ncls + R
