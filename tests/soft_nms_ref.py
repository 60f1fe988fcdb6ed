"""Restatement of frcnn_soft_nms_batch (include/frcnn_hip.h) for the tests: no GPU, no library.

  s[i] = score column; row i is alive iff s[i] >= min_score                       (a NaN is never alive)
  repeat: m = the alive, unpicked row of largest s (compared as values: -0 == +0); ties: the HIGHER row id; none -> stop
          pick m; score_out[m] = s[m]; for every alive unpicked j with cls[j] == cls[m] (all j without cls):
            hard:     if !(iou <= Nt): j dies
            linear:   if !(iou <= Nt): s[j] = s[j] * (1 - iou)               (log_domain: s[j] + log1p(-iou))
            gaussian: (every j)        s[j] = s[j] * exp(-(iou*iou)/sigma)   (log_domain: s[j] - (iou*iou)/sigma)
            then: if !(s[j] >= min_score): j dies
  area = (x2-x1+1)*(y2-y1+1), w = max(0, (xx2 + (-1)*xx1) + 1), iou = (w*h) / ((area_j + area_m) - w*h)

soft_nms_f32 does this in numpy fp32, one rounded operation per statement: for the EXACT combinations (hard; linear with
log_domain 0; gaussian with log_domain 1 -- no transcendental) the device must agree with it bit for bit.
soft_nms_f64 does it in float64 on the same fp32 inputs and parameters and reports the smallest DECISION MARGIN it met; for the
two INEXACT combinations (linear with log_domain 1: log1pf; gaussian with log_domain 0: expf) the device is compared with it on
inputs whose margin exceeds twice score_error_bound(), the worst case of the device's accumulated score error derived below.

THE IoU'S ERROR, |iou_dev - iou| <= K u with u = 2^-24, under one of two preconditions:
  K = IOU_ERR_INTEGER = 1 (asserted by inexact_cases): the coordinates are integers in [0, 2048).  Then x2 - x1, + 1, the two
      areas (<= 2^22), their sum (<= 2^23), w, h, w*h and the denominator are integers below 2^24: every fp32 operation in front
      of the division is exact, and the device's IoU carries ONE rounding, iou_dev = iou (1 + d0), |d0| <= u, with iou <= 1.
  K = IOU_ERR_GENERAL = 28: finite fp32 coordinates with x2 >= x1 and y2 >= y1 (the Detector's boxes).  a = xx2 - xx1 is rounded
      once; a + 1 <= 0 exactly when the device computes w = 0 (rounding is monotone and -1 is a number), so a disjoint pair has
      iou_dev = 0 = iou.  Otherwise a > -1 and |a| <= max(w, 1): w_dev = w (1 + 2u) up to an absolute 2u when w < 1, the same for
      h; inter = w h then carries 5u relative, or -- through the absolute part -- at most 2u h resp. 2u w, which the division by
      denom >= area >= h resp. w (every extent is >= 1 after the + 1) turns into at most 4u absolute.  Each area is three rounded
      operations on two exact differences: 5u relative; their sum S one more: 6u; denom = S - inter with S <= 2 denom (inter <=
      the smaller area <= S / 2): 12u + 5u iou + u <= 18u relative; the division u.  Together iou (5 + 18 + 1) u + 4u <= 28u.

gaussian, log_domain 0 (a RELATIVE bound).  One decay is s' = fl(s * E), E = expf(-t^), t^ = fl(fl(iou_dev * iou_dev) / sigma):
  |t^ - t| <= (2 iou / sigma) K u (the decay's sensitivity 2 iou / sigma to the IoU's error) + 2u t (the square, the division)
           <= ((2 K + 2) / sigma) u  with iou <= 1                                             [+ O(u^2)]
  exp(-t^) = exp(-t) exp(t - t^): a relative error of |t^ - t|
  expf: EXPF_ULP units in the last place of its result, i.e. at most 2 EXPF_ULP u relative
  the product: u
  e = ((2 K + 2) / sigma + 2 EXPF_ULP + 1) u per decay; a decay with iou = 0 has t^ = 0, expf(-0) = 1 and s * 1 = s: no error, and it is
  not counted.  After D counted decays the relative error is at most (1 + e)^D - 1.
linear, log_domain 1 (an ABSOLUTE bound).  One decay is s' = fl(s + L), L = log1pf(-iou_dev):
  log1p(-iou_dev) - log1p(-iou) = (iou - iou_dev) / (1 - x) for an x between iou and iou_dev (mean value theorem): at most
      K u / (1 - iou - K u) -- the sensitivity 1 / (1 - iou)
  log1pf: LOG1PF_ULP units in the last place of its result: at most 2 LOG1PF_ULP u |log1p(-iou)|
  the sum: u |s'|
  e = u (K / (1 - iou_max - K u) + 2 LOG1PF_ULP |log1p(-iou_max)| + s_abs_max) per decay, with iou_max the largest IoU
  below 1 of a counted decay (an IoU of exactly 1 gives -inf on both sides, exactly) and s_abs_max the largest finite |score| of
  the run; every term grows with iou, so iou_max covers every decay.  Absolute errors add: D e after D decays.
Both: the terms of second order are below 2^-10 of the first-order sum as long as D e < 2^-10 (asserted in
score_error_bound), so the bound is the first-order sum times (1 + 2^-10); the float64 restatement's own error, D * 16 * 2^-53
of the scale, is added; and the bound is never below K u, the IoU's own error, which covers the comparison of the IoU with Nt.
EXPF_ULP = LOG1PF_ULP = 1: the accuracy the HIP math API documents for expf and log1pf ("Maximum error: 1 ULP").

MARGINS (soft_nms_f64): the gap between the pick and every other alive row at every pick, the gap between every freshly decayed
score and min_score, and the gap between every IoU and Nt where Nt is compared -- relative (to the larger magnitude) with
log_domain 0, absolute with log_domain 1.  A score no counted decay has touched yet is the input's fp32 value on both sides,
exactly: a comparison between two such scores (ties included -- both sides break them by the row id) has no margin to keep, and
is left out.  A gap that is not a number (-inf against -inf) counts as 0."""
import functools
import math

import numpy as np

HARD, LINEAR, GAUSSIAN = 0, 1, 2
METHODS = ("hard", "linear", "gaussian")
U = 2.0 ** -24
EXPF_ULP = 1.0
LOG1PF_ULP = 1.0
IOU_ERR_INTEGER = 1.0
IOU_ERR_GENERAL = 28.0


def is_exact(method, log_domain):
    return method == HARD or (method == LINEAR and not log_domain) or (method == GAUSSIAN and bool(log_domain))


def _loop(rows, score_col, method, overlap, sigma, min_score, log_domain, cls, f, track):
    b = np.asarray(rows, np.float32).astype(f)
    n = b.shape[0] if b.ndim == 2 else 0
    pick, out = [], []
    stats = dict(margin=math.inf, decays=0, iou_max=0.0, s_abs_max=0.0)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, f), stats
    cls = None if cls is None else np.asarray(cls).astype(np.int64)
    # the parameters are the fp32 values the C entry point receives
    Nt, sg, ms = f(np.float32(overlap)), f(np.float32(sigma)), f(np.float32(min_score))
    one, zero = f(1), f(0)
    x1, y1, x2, y2 = b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy(), b[:, 3].copy()
    with np.errstate(all="ignore"):
        dx = x2 - x1
        dy = y2 - y1
        dx = dx + one
        dy = dy + one
        area = dx * dy
        s = b[:, score_col - 1].copy()
        alive = s >= ms
        nd = np.zeros(n, np.int64)            # counted (non-trivial) decays a row has received

        def gap(a, c):                        # relative / absolute distance, elementwise; not-a-number -> 0
            g = np.abs(a - c)
            if not log_domain:
                g = g / np.maximum(np.maximum(np.abs(a), np.abs(c)), np.finfo(np.float64).tiny)
            return np.where(np.isnan(g), 0.0, g)

        def note(g):
            if g.size:
                stats["margin"] = min(stats["margin"], float(np.min(g)))
        if track:
            fin = s[alive & np.isfinite(s)]
            if fin.size:
                stats["s_abs_max"] = float(np.max(np.abs(fin)))
        while True:
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                break
            v = s[idx]
            m = int(idx[np.nonzero(v == v.max())[0][-1]])
            if track:
                oth = idx[idx != m]
                if nd[m] == 0:
                    oth = oth[nd[oth] > 0]
                note(gap(s[oth], s[m]))
            pick.append(m + 1)
            out.append(s[m])
            alive[m] = False
            sel = alive if cls is None else (alive & (cls == cls[m]))
            j = np.nonzero(sel)[0]
            if j.size == 0:
                continue
            xx1 = np.where(x1[j] > x1[m], x1[j], x1[m])
            yy1 = np.where(y1[j] > y1[m], y1[j], y1[m])
            xx2 = np.where(x2[j] < x2[m], x2[j], x2[m])
            yy2 = np.where(y2[j] < y2[m], y2[j], y2[m])
            w = xx2 + f(-1) * xx1
            w = w + one
            w = np.where(w > zero, w, zero)
            h = yy2 + f(-1) * yy1
            h = h + one
            h = np.where(h > zero, h, zero)
            inter = w * h
            denom = area[j] + area[m]
            denom = denom - inter
            iou = inter / denom
            sj = s[j]
            dead = np.zeros(j.size, bool)
            if method == GAUSSIAN:
                t = iou * iou
                t = t / sg
                new = (sj - t) if log_domain else (sj * np.exp(-t))
                counted = ~(t == zero)
            else:
                hit = ~(iou <= Nt)
                if track:
                    note(gap(iou, np.full_like(iou, Nt)))
                if method == HARD:
                    dead = hit
                    new = sj
                    counted = np.zeros(j.size, bool)
                else:
                    if log_domain:
                        dec = sj + np.log1p(-iou)
                    else:
                        fct = one - iou
                        dec = sj * fct
                    new = np.where(hit, dec, sj)
                    counted = hit
            s[j] = new
            alive[j] = (new >= ms) & ~dead
            if track and counted.any():
                c = j[counted]
                nd[c] += 1
                note(gap(new[counted], np.full(c.size, ms)))
                stats["decays"] = max(stats["decays"], int(nd[c].max()))
                below = iou[counted][iou[counted] < one]
                if below.size:
                    stats["iou_max"] = max(stats["iou_max"], float(below.max()))
                fin = new[counted][np.isfinite(new[counted])]
                if fin.size:
                    stats["s_abs_max"] = max(stats["s_abs_max"], float(np.max(np.abs(fin))))
    return np.array(pick, np.int64), np.array(out, f), stats


def soft_nms_f32(rows, score_col, method, overlap, sigma, min_score, log_domain, cls=None):
    """-> (pick: 1-based int64 rows in pick order, scores at pick: fp32), every operation an fp32 operation of its own"""
    pick, out, _ = _loop(rows, score_col, method, overlap, sigma, min_score, log_domain, cls, np.float32, False)
    return pick, out


def soft_nms_f64(rows, score_col, method, overlap, sigma, min_score, log_domain, cls=None):
    """-> (pick, scores at pick: float64, stats): stats = dict(margin: the smallest decision margin of the run (see the module's
    docstring; inf when there was none to keep), decays: the largest number of counted decays a row received, iou_max: the
    largest IoU below 1 of a counted decay, s_abs_max: the largest finite |score|)"""
    return _loop(rows, score_col, method, overlap, sigma, min_score, log_domain, cls, np.float64, True)


def score_error_bound(method, log_domain, sigma, stats, iou_err=IOU_ERR_INTEGER):
    """The worst case of |device score - float64 score| for a run with these stats: relative with log_domain 0, absolute with
    log_domain 1 (derivation: the module's docstring; iou_err = K, the IoU's error in units of u under the precondition the
    caller has checked).  0 for the exact combinations."""
    if is_exact(method, log_domain):
        return 0.0
    D = stats["decays"]
    if method == GAUSSIAN:
        e = ((2.0 * iou_err + 2.0) / float(np.float32(sigma)) + 2.0 * EXPF_ULP + 1.0) * U
        first = math.expm1(D * math.log1p(e))
        own = D * 16 * 2.0 ** -53
    else:
        x = stats["iou_max"]
        if x > 1.0 - 2.0 ** -10:
            return math.inf
        e = U * (iou_err / (1.0 - x - iou_err * U) + 2.0 * LOG1PF_ULP * abs(math.log1p(-x)) + stats["s_abs_max"])
        first = D * e
        own = D * 16 * 2.0 ** -53 * max(stats["s_abs_max"], 1.0)
    assert D * e < 2.0 ** -10, "the second-order terms are not negligible"
    return max(first * (1.0 + 2.0 ** -10) + own, iou_err * U)


# ---------------------------------------------------------------------------------------------- generators (integer coordinates)
CELL = 40          # 51 x 51 disjoint cells of 40 x 40 in [0, 2048)


def _cells(rng, n):
    side = 2048 // CELL
    assert n <= side * side
    c = rng.permutation(side * side)[:n]
    return (c % side) * CELL, (c // side) * CELL


def disjoint_boxes(rng, n):
    """n pairwise disjoint boxes: one per cell, inside it"""
    cx, cy = _cells(rng, n)
    x1 = cx + rng.randint(0, 8, n)
    y1 = cy + rng.randint(0, 8, n)
    return np.stack([x1, y1, x1 + rng.randint(4, 30, n), y1 + rng.randint(4, 30, n)], 1).astype(np.float32)


def clustered_boxes(rng, n, per=12):
    """clusters of about `per` boxes around common centres: many overlaps per row, IoUs that repeat and hit simple fractions"""
    k = max(n // per, 1)
    g = np.arange(n) % k
    x1 = rng.randint(40, 1900, k)[g] + rng.randint(-10, 11, n) * 2
    y1 = rng.randint(40, 1900, k)[g] + rng.randint(-10, 11, n) * 2
    return np.stack([x1, y1, x1 + rng.randint(5, 20, n) * 2 - 1, y1 + rng.randint(5, 20, n) * 2 - 1], 1).astype(np.float32)


def same_box(rng, n):
    return np.tile(np.array([[100, 120, 139, 199]], np.float32), (n, 1))


def sparse_clusters(rng, n, groups=12):
    """disjoint boxes, except that `groups` cells (every cell for n <= 65) hold three boxes that overlap one another without
    coinciding: few rows receive a decay, and none more than two"""
    T = n // 3 if n <= 65 else min(groups, n // 3)
    rem = n - 3 * T
    counts = [3] * T + ([2] if (n <= 65 and rem == 2) else [1] * rem)
    cx, cy = _cells(rng, len(counts))
    b = np.zeros((n, 4), np.float32)
    r = 0
    for c, k in enumerate(counts):
        for q in range(k):
            x1 = cx[c] + 3 * q + rng.randint(0, 3)
            y1 = cy[c] + 2 * q + rng.randint(0, 3)
            b[r] = (x1, y1, x1 + rng.randint(14, 24), y1 + rng.randint(14, 24))
            r += 1
    assert r == n
    return b[rng.permutation(n)]


def grid_scores(rng, n, lo, hi):
    """n distinct fp32 scores, evenly spaced in (lo, hi), in random order"""
    return (lo + (rng.permutation(n) + 1.0) / (n + 1.0) * (hi - lo)).astype(np.float32)


def rows5(boxes, scores):
    return np.concatenate([boxes, np.asarray(scores, np.float32)[:, None]], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the inexact combinations' cases
INEXACT = ((LINEAR, 1), (GAUSSIAN, 0))
INEXACT_PARAMS = {(LINEAR, 1): dict(overlap=0.3, sigma=0.5, min_score=math.log(0.001)),
                  (GAUSSIAN, 0): dict(overlap=0.3, sigma=0.5, min_score=0.001)}
INEXACT_QUOTA = 2      # margin-filtered cases per (combination, n, classes)


@functools.lru_cache(maxsize=None)
def inexact_cases(method, log_domain, n, nclasses, quota=INEXACT_QUOTA):
    """`quota` cases (rows n x 5, cls or None, params, the float64 run, the bound) for one of the two inexact combinations whose
    float64 margin exceeds twice the derived bound.  Seeds are drawn in order; at most half of the seeds tried may be discarded
    (asserted): the generator (sparse_clusters, evenly spaced distinct scores) is chosen so that the restatement alone meets
    that cap.  nclasses 0: no classes."""
    P = INEXACT_PARAMS[(method, log_domain)]
    cases, tried = [], 0
    while len(cases) < quota:
        assert tried < 2 * quota, "more than half of the seeds discarded (%d tried, %d kept; n = %d)" % (tried, len(cases), n)
        rng = np.random.RandomState(7000 + 131 * tried + 17 * n + 3 * method + nclasses)
        tried += 1
        boxes = sparse_clusters(rng, n)
        assert np.all(boxes == np.floor(boxes)) and boxes.min() >= 0 and boxes.max() < 2048, "the bound's precondition"
        sc = grid_scores(rng, n, -1.6, -0.01) if log_domain else grid_scores(rng, n, 0.05, 1.0)
        rows = rows5(boxes, sc)
        cls = None if not nclasses else rng.randint(1, nclasses + 1, n).astype(np.int32)
        pick, out, st = soft_nms_f64(rows, 5, method, P["overlap"], P["sigma"], P["min_score"], log_domain, cls)
        bound = score_error_bound(method, log_domain, P["sigma"], st)
        if st["margin"] > 2.0 * bound:
            cases.append(dict(rows=rows, cls=cls, params=P, pick=pick, scores=out, stats=st, bound=bound, seed_index=tried - 1))
    return tuple(cases)
