"""Float64 restatements of the anchor-level and criterion entry points of include/frcnn_hip.h, for the tests: no GPU, no library.

  scan_ref         frcnn_rpn_scan[_batch]   Detector.lua:39-66, Anchors.lua:60-67 / 245-252, Rect.lua:30-32 / 90-93
  rpn_loss_ref     frcnn_rpn_loss           objective.lua:91-140 and 149-159, Anchors.lua:237-243
  cnet_losses_ref  frcnn_cnet_losses        objective.lua:170-177
  decode_ref       frcnn_cnet_decode        Detector.lua:110-113

Lua numbers are doubles; a value is rounded to fp32 exactly where the header or the reference holds it in a FloatTensor or a
CudaTensor: the log-probabilities of nn.LogSoftMax, the FloatTensor of Anchors.inputToAnchor, crtarget, the element-wise
difference and gradient of nn.SmoothL1Criterion, the criterion's output (the `(float)` of its sum), match_box.

THE VALUE RULE.  Host and device exp / log in fp64 may differ in the last bit.  That can move one fp32 rounding by one unit in
the last place (ulp), and one more fp32 rounding may follow (t - tgt).  An fp32 output that passes through exp or log must
therefore lie within 2 fp32 ulps of this module's value, the ulp taken at the magnitude of the larger operand of the output's
last operation when that is a sum or a difference (v - lse, exp(l) - onehot, t - tgt, x + w'; the result may have cancelled), and
at the magnitude of the result when it is a quotient or a log (crtarget; nothing cancels in them).  The x10 regression
gradients get ten times the bound of t - tgt, and reg * 10 ten times 2 ulps of the rounded sum.  Nothing else is added: no
tolerance is carried from an argument into a result.  The fp64 rects must lie within 4 * 2^-52 of the same magnitudes.  Every
function returns the tolerance next to the value; 0 means bit for bit, and a quantity without exp or log in its history has
tolerance 0.

The generators of the problems the GPU tests run are here as well, so that tests/test_anchor_ops_host.py can assert their input
conditions without a GPU."""
import functools
import math

import numpy as np

U32 = 2.0 ** -24
F32 = np.float32


def f32(x):
    return float(np.float32(x))


def ulp32(x):
    """the distance from fp32(|x|) to the next fp32 above it (elementwise)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------- geometry (scalars, Lua numbers)
def anchor_get(aw, ah, layer, aspect, y, x):
    """Anchors:get(layer, aspect, y, x), all 1-based, from the fp32 tables [4][3][200][2] -> (minX, minY, maxX, maxY)"""
    return (float(aw[layer - 1, aspect - 1, x - 1, 0]), float(ah[layer - 1, aspect - 1, y - 1, 0]),
            float(aw[layer - 1, aspect - 1, x - 1, 1]), float(ah[layer - 1, aspect - 1, y - 1, 1]))


def input_to_anchor(anchor, rect):
    """Anchors.inputToAnchor -> the four fp32 values of its FloatTensor"""
    w = anchor[2] - anchor[0]
    h = anchor[3] - anchor[1]
    return (f32((rect[0] - anchor[0]) / w), f32((rect[1] - anchor[1]) / h),
            f32(math.log((rect[2] - rect[0]) / w)), f32(math.log((rect[3] - rect[1]) / h)))


def anchor_to_input(anchor, t):
    """Anchors.anchorToInput(anchor, t) with Rect.fromXYWidthHeight -> (minX, minY, maxX, maxY) as doubles; t: four fp32 values"""
    w = anchor[2] - anchor[0]
    h = anchor[3] - anchor[1]
    x = float(t[0]) * w + anchor[0]
    y = float(t[1]) * h + anchor[1]
    return (x, y, x + math.exp(float(t[2])) * w, y + math.exp(float(t[3])) * h)


def overlaps_image(r, img_w, img_h):
    """Rect.overlaps(r, Rect(0, 0, img_w, img_h))"""
    return r[0] < img_w and r[2] > 0.0 and r[1] < img_h and r[3] > 0.0


def log_softmax2(v0, v1):
    """nn.LogSoftMax of two fp32 logits -> (l0, l1 as fp32 values, lse); max-shifted like the THNN module"""
    v0, v1 = float(v0), float(v1)
    m = max(v0, v1)
    lse = m + math.log(math.exp(v0 - m) + math.exp(v1 - m))
    return f32(v0 - lse), f32(v1 - lse), lse


# ---------------------------------------------------------------------------------------------- the scan
def scan_ref(maps, H, W, aw, ah, img_w, img_h, thr):
    """maps: four arrays [18][H_l][W_l] fp32; aw, ah: fp32 [4][3][200][2].  -> dict, matches in scan order (layer, y, x, aspect):
    p fp32, idx int32 {layer, aspect, y, x} 1-based, rect float64, box fp32, count (the full number of matches), the tolerances
    p_tol / rect_tol / box_tol of the value rule, and per ANCHOR of the scan (all 3 * sum(H W) of them): match (bool),
    thr_margin = |exp(c1) - thr| and ovl_margin[4] = the distances |minX - img_w|, |maxX|, |minY - img_h|, |maxY| of the overlap
    test divided by the image's size along that axis (inf where the threshold test already said no: no such decision is made)."""
    aw = np.asarray(aw, np.float32).astype(np.float64)
    ah = np.asarray(ah, np.float32).astype(np.float64)
    cols = dict(c1=[], e=[], pscale=[], rect=[], rscale=[], idx=[])
    for l in range(4):
        h, w = int(H[l]), int(W[l])
        m = np.asarray(maps[l], np.float32).reshape(3, 6, h, w).astype(np.float64).transpose(2, 3, 0, 1)   # [y][x][aspect][k]
        v0, v1 = m[..., 0], m[..., 1]
        mx = np.maximum(v0, v1)
        lse = mx + np.log(np.exp(v0 - mx) + np.exp(v1 - mx))
        c1 = (v0 - lse).astype(np.float32)
        cols["c1"].append(c1.ravel())
        cols["e"].append(np.exp(c1.astype(np.float64)).ravel())
        cols["pscale"].append(np.maximum(np.abs(v0), np.abs(lse)).ravel())
        ax0 = aw[l, :, :w, 0].T[None, :, :]
        ax1 = aw[l, :, :w, 1].T[None, :, :]
        ay0 = ah[l, :, :h, 0].T[:, None, :]
        ay1 = ah[l, :, :h, 1].T[:, None, :]
        awd, ahd = ax1 - ax0, ay1 - ay0
        tx, ty = m[..., 2] * awd, m[..., 3] * ahd
        rx, ry = tx + ax0, ty + ay0
        rw, rh = np.exp(m[..., 4]) * awd, np.exp(m[..., 5]) * ahd
        rx1, ry1 = rx + rw, ry + rh
        cols["rect"].append(np.stack([rx, ry, rx1, ry1], -1).reshape(-1, 4))
        sx = np.maximum(np.abs(tx), np.abs(ax0) + 0 * tx)
        sy = np.maximum(np.abs(ty), np.abs(ay0) + 0 * ty)
        cols["rscale"].append(np.stack([sx, sy, np.maximum(sx, np.abs(rw)), np.maximum(sy, np.abs(rh))], -1).reshape(-1, 4))
        yy, xx, aa = np.meshgrid(np.arange(1, h + 1), np.arange(1, w + 1), np.arange(1, 4), indexing="ij")
        cols["idx"].append(np.stack([np.full_like(yy, l + 1), aa, yy, xx], -1).reshape(-1, 4))
    c = {k: np.concatenate(v) for k, v in cols.items()}
    over = c["e"] > thr
    r = c["rect"]
    inside = (r[:, 0] < img_w) & (r[:, 2] > 0.0) & (r[:, 1] < img_h) & (r[:, 3] > 0.0)
    match = over & inside
    ovl = np.stack([np.abs(r[:, 0] - img_w) / img_w, np.abs(r[:, 2]) / img_w, np.abs(r[:, 1] - img_h) / img_h,
                    np.abs(r[:, 3]) / img_h], 1)
    ovl[~over] = np.inf
    s = np.nonzero(match)[0]
    return dict(p=c["c1"][s], idx=c["idx"][s].astype(np.int32), rect=r[s], box=r[s].astype(np.float32), count=int(s.size),
                p_tol=2.0 * ulp32(c["pscale"][s]), rect_tol=4.0 * 2.0 ** -52 * c["rscale"][s], box_tol=2.0 * ulp32(c["rscale"][s]),
                match=match, thr_margin=np.abs(c["e"] - thr), ovl_margin=ovl, total=int(match.size))


# ---------------------------------------------------------------------------------------------- the sparse RPN loss
EXACT_LOGIT_GAP = 40.0      # exp(-40) < 2^-53: 1 + exp(-gap) is 1 and its log 0 in fp64, whatever the last bit of exp says


def smooth_l1_terms(z):
    """nn.SmoothL1Criterion on the fp32 differences z -> (the float64 terms, the fp32 gradients of sizeAverage = false)"""
    terms, grads = [], []
    for v in z:
        v = f32(v)
        a = abs(v)
        terms.append(0.5 * v * v if a < 1.0 else a - 0.5)
        grads.append(v if a < 1.0 else (1.0 if v > 0.0 else -1.0))
    return terms, grads


def rpn_loss_ref(maps, deltas0, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, bgclass):
    """maps: four arrays [18][H][W] fp32; deltas0: the maps the gradients are added to (only their shapes are used: the caller
    forms the expected maps from `addends`).  -> dict: ex_loss float64 [E][2] = {cls, reg * 10} with ex_loss_tol, crtarget fp32
    [E][4] with crtarget_tol, cctarget fp32 [E], addends = [(layer 0-based, flat offset into [18][H][W], fp32 addend, tol)] in
    example order (a positive: 6, a negative: 2).

    Tolerances (the module's value rule), d(m) = 2 fp32 ulps at the magnitude m:
      log-prob l_k = fp32(v_k - lse): d(max(|v_k|, |lse|)); 0 when |v0 - v1| > 40 (lse is the larger logit, exactly)
      class gradient fp32(exp(l_k) - onehot): d(max(exp(l_k), onehot)); 0 when the log-prob's tolerance is 0 and either
        l_k == 0 (exp(0) = 1) or exp(l_k) < 2^-60 beside a onehot of 1 (the difference is -1 in fp64)
      tgt[0..1] = fp32 of a quotient of doubles: 0.  z = fp32(t - tgt): 0 for c < 2; for c >= 2 (tgt = fp32(log q))
        d(max(|t|, |tgt|)), and 0 when q == 1
      regression gradient fp32(g * 10): ten times the tolerance of z
      reg * 10 = fp32(sum of the four terms) * 10: 10 * d(sum); 0 when every z is exact.  The terms are added in index order in fp64
      crtarget = Anchors.inputToAnchor(proposal, roi), the proposal a Rect {x, y, x + w', y + h'} with w' = exp(t2) * w, so its
        width is (x + w') - x as in the reference: d(|value|) for all four"""
    E = npos + nneg
    out = dict(ex_loss=np.zeros((E, 2)), ex_loss_tol=np.zeros((E, 2)), crtarget=np.zeros((E, 4), np.float32),
               crtarget_tol=np.zeros((E, 4)), cctarget=np.zeros(E, np.float32), addends=[])
    for e in range(E):
        l, asp, y, x = (int(v) - 1 for v in ex_idx[e])
        m = np.asarray(maps[l], np.float32)
        hw = m.shape[1] * m.shape[2]
        v = [float(m[asp * 6 + k, y, x]) for k in range(6)]
        base = asp * 6 * hw + y * m.shape[2] + x
        pos = e < npos
        l0, l1, lse = log_softmax2(v[0], v[1])
        exact = abs(v[0] - v[1]) > EXACT_LOGIT_GAP
        if exact:
            assert lse == max(v[0], v[1])
        for k, (lk, hot) in enumerate(((l0, 1.0 if pos else 0.0), (l1, 0.0 if pos else 1.0))):
            ltol = 0.0 if exact else 2.0 * float(ulp32(max(abs(v[k]), abs(lse))))
            ek = math.exp(lk)
            if ltol == 0.0 and (lk == 0.0 or (hot == 1.0 and ek < 2.0 ** -60)):
                gtol = 0.0
            else:
                gtol = 2.0 * float(ulp32(max(ek, hot)))
            out["addends"].append((l, base + k * hw, f32(ek - hot), gtol))
            if hot == 1.0:
                out["ex_loss"][e, 0] = -lk
                out["ex_loss_tol"][e, 0] = ltol
        if not pos:
            out["cctarget"][e] = F32(bgclass)
            continue
        an = [float(a) for a in ex_anchor[e]]
        roi = [float(a) for a in ex_roi[e]]
        w, h = an[2] - an[0], an[3] - an[1]
        tgt = input_to_anchor(an, roi)
        q = ((roi[2] - roi[0]) / w, (roi[3] - roi[1]) / h)
        t = v[2:6]
        z = [f32(F32(t[c]) - F32(tgt[c])) for c in range(4)]
        ztol = [0.0, 0.0] + [0.0 if q[c - 2] == 1.0 else 2.0 * float(ulp32(max(abs(t[c]), abs(tgt[c])))) for c in (2, 3)]
        terms, grads = smooth_l1_terms(z)
        s = 0.0
        for c in range(4):
            s += terms[c]
            a = f32(F32(grads[c]) * F32(10.0))
            out["addends"].append((l, base + (2 + c) * hw, a, 10.0 * ztol[c]))
        out["ex_loss"][e, 1] = f32(s) * 10.0
        if any(ztol):
            out["ex_loss_tol"][e, 1] = 10.0 * 2.0 * float(ulp32(s))
        prop = anchor_to_input(an, t)               # reg_proposal, a Rect: its width is (x + w') - x
        crt = input_to_anchor(prop, roi)
        out["crtarget"][e] = crt
        out["crtarget_tol"][e] = [2.0 * float(ulp32(v)) for v in crt]
        out["cctarget"][e] = F32(int(ex_class[e]))
    return out


def expected_maps(deltas0, addends, mode):
    """The delta maps after the call.  mode "f32seq": the fp32 sum in example order (option deterministic) -> four fp32 arrays.
    mode "f64": -> (four float64 arrays of the exact sums, four arrays of bounds): the fp32 summation bound k * 2^-24 * sum|terms|
    (k terms, the initial value being one of them) plus the addends' own tolerances."""
    flat0 = [np.asarray(d, np.float32).ravel() for d in deltas0]
    if mode == "f32seq":
        out = [d.copy() for d in flat0]
        for l, off, a, _ in addends:
            out[l][off] = F32(out[l][off] + F32(a))
        return [o.reshape(np.shape(d)) for o, d in zip(out, deltas0)]
    per = {}
    for l, off, a, tol in addends:
        per.setdefault((l, off), []).append((a, tol))
    want = [d.astype(np.float64) for d in flat0]
    bound = [np.zeros(d.size) for d in flat0]
    for (l, off), items in per.items():
        terms = [float(flat0[l][off])] + [a for a, _ in items]
        want[l][off] = math.fsum(terms)
        bound[l][off] = len(terms) * U32 * math.fsum(abs(v) for v in terms) + sum(tol for _, tol in items)
    return ([w.reshape(np.shape(d)) for w, d in zip(want, deltas0)], [b.reshape(np.shape(d)) for b, d in zip(bound, deltas0)])


# ---------------------------------------------------------------------------------------------- the two criteria of the classification net
def cnet_losses_ref(crout, crtarget, ccout, cctarget, R, npos, ncls):
    """-> dict: crout (rows >= npos zeroed, the others as they were), crdelta fp32 [R][4] = SmoothL1 gradient * 10 (both fp32),
    ccdelta fp32 [R][ncls] = fp32(-1 / R) at the target and 0 elsewhere, reg_sum = the exact sum of the SmoothL1 terms and
    cls_mean = the exact sum of -ccout[r][target_r], divided by R (math.fsum, before any rounding to fp32).  The entry point adds
    (double)(float)reg_sum * 10 and (double)(float)cls_mean to loss2.  No exp and no log: everything but the two sums is exact."""
    cr = np.array(crout, np.float32).reshape(R, 4)
    cr[npos:] = 0.0
    z = (cr - np.asarray(crtarget, np.float32).reshape(R, 4)).astype(np.float32)
    terms, grads = smooth_l1_terms(z.ravel())
    crdelta = (np.array(grads, np.float32) * F32(10.0)).astype(np.float32).reshape(R, 4)
    cc = np.asarray(ccout, np.float32).reshape(R, ncls)
    tg = np.asarray(cctarget, np.float32).astype(np.int64) - 1
    ccdelta = np.zeros((R, ncls), np.float32)
    ccdelta[np.arange(R), tg] = F32(-1.0 / R)
    return dict(crout=cr, crdelta=crdelta, ccdelta=ccdelta, reg_sum=math.fsum(terms),
                cls_mean=math.fsum(-float(cc[r, tg[r]]) for r in range(R)) / R)


def decode_ref(lsm):
    """class = 1-based column of the FIRST maximum of the row (torch.sort(cprob, 1, true), Detector.lua:110), confidence = it"""
    lsm = np.asarray(lsm, np.float32)
    cls = np.zeros(lsm.shape[0], np.int32)
    conf = np.zeros(lsm.shape[0], np.float32)
    for r in range(lsm.shape[0]):
        best = 0
        for j in range(1, lsm.shape[1]):
            if lsm[r, j] > lsm[r, best]:
                best = j
        cls[r] = best + 1
        conf[r] = lsm[r, best]
    return cls, conf


# ============================================================================================== generators
# ---------------------------------------------------------------------------------------------- scan problems
IMG_W, IMG_H, THR = 300.0, 200.0, 0.95
BORDER = 0.01               # "just" inside / outside an image border, in pixels
BORDER_CENTRE = 8           # scan_case's `border` entry of an anchor whose rect is put around the image's centre
MARGIN = 1e-6               # the input conditions: no exp(c1) within MARGIN of thr, no overlap distance under MARGIN of the size
# head map sizes (H, W) per layer; 3 * sum(H W) anchors
SCAN_SIZES = {
    "n12": [(1, 1), (1, 1), (1, 1), (1, 1)],
    "n1023": [(13, 11), (9, 10), (7, 12), (4, 6)],       # one short of the compaction's 1024-anchor chunk
    "n1026": [(14, 11), (9, 10), (7, 12), (2, 7)],       # two anchors in the second chunk
    "n2490": [(23, 17), (15, 13), (11, 14), (9, 10)],    # three chunks, the last one partial
    "n1287": [(200, 1), (1, 200), (3, 5), (2, 7)],       # the last row of the 200-entry tables, in y and in x
}
SCAN_PATTERNS = ("none", "all", "first", "last", "a63_a64", "a1023_a1024", "wave1", "alternate", "random", "soft")
# every pattern but the last sets the foreground logit to +-30.  Its matches then have |p| < 0.007 beside operands of 30, whose ulp
# is the scale of p's bound.  "soft" is the random pattern with logits of order 1: p between -0.04 and -0.007, the bound about 1e-7.
SOFT_FG_GAP, SOFT_BG_GAP = (3.2, 5.0), (-3.0, 2.5)      # v0 - v1: exp(c1) in (0.960, 0.994), resp. below 0.925


def scan_total(name):
    return 3 * sum(h * w for h, w in SCAN_SIZES[name])


def scan_pattern(pattern, total, rng):
    """-> bool [total] (the anchors, 0-based in scan order, that are to match), or None where the problem is too small for it"""
    f = np.zeros(total, bool)
    if pattern == "none":
        pass
    elif pattern == "all":
        f[:] = True
    elif pattern == "first":
        f[0] = True
    elif pattern == "last":
        f[-1] = True
    elif pattern == "a63_a64":
        if total < 66:
            return None
        f[63:65] = True
    elif pattern == "a1023_a1024":
        if total < 1026:
            return None
        f[1023:1025] = True
    elif pattern == "wave1":      # lanes 0..63 of the second wave, both neighbours clear
        if total < 129:
            return None
        f[64:128] = True
    elif pattern == "alternate":
        f[::2] = True
    elif pattern in ("random", "soft"):
        f[:] = rng.rand(total) < 0.5
    else:
        raise KeyError(pattern)
    return f


def scan_patterns_for(name):
    return [p for p in SCAN_PATTERNS if scan_pattern(p, scan_total(name), np.random.RandomState(0)) is not None]


def anchor_tables(rng):
    """fp32 tables [4][3][200][2]: per (layer, aspect) random centres that increase along the row, one random extent"""
    t = np.zeros((2, 4, 3, 200, 2))
    for k in range(2):
        for l in range(4):
            for a in range(3):
                c = np.cumsum(rng.uniform(1.0, 3.0, 200))
                size = rng.uniform(8.0, 120.0)
                t[k, l, a, :, 0] = c - size / 2
                t[k, l, a, :, 1] = c + size / 2
    t = t.astype(np.float32)
    assert np.all(np.diff(t, axis=3) > 0) and np.all(t[..., 1] > t[..., 0])
    return t[0], t[1]


@functools.lru_cache(maxsize=None)
def scan_tables(name):
    return anchor_tables(np.random.RandomState(1000 + sorted(SCAN_SIZES).index(name)))


@functools.lru_cache(maxsize=None)
def scan_case(name, pattern):
    """-> dict(maps: four fp32 [18][H][W], H, W, aw, ah, want: scan_ref's result, flags: the pattern, border: per anchor the kind of
    border placement (-1: none; 2 * side + {0: just outside, 1: just inside}, sides minX/img_w, maxX/0, minY/img_h, maxY/0;
    BORDER_CENTRE: around the image's centre))"""
    sizes = SCAN_SIZES[name]
    H = [h for h, w in sizes]
    W = [w for h, w in sizes]
    aw, ah = scan_tables(name)
    total = scan_total(name)
    rng = np.random.RandomState(7 + 31 * SCAN_PATTERNS.index(pattern) + 1009 * sorted(SCAN_SIZES).index(name))
    flags = scan_pattern(pattern, total, rng)
    # per anchor in scan order: the six head values
    v = np.zeros((total, 6))
    v[:, 0] = np.where(flags, 30.0, -30.0)
    v[:, 1] = rng.uniform(-5.0, 25.0, total)
    if pattern == "soft":
        v[:, 0] = rng.uniform(-1.0, 1.0, total)
        v[:, 1] = v[:, 0] - np.where(flags, rng.uniform(*SOFT_FG_GAP, total), rng.uniform(*SOFT_BG_GAP, total))

    def draw(n):
        return np.concatenate([rng.randn(n, 2) * 0.5, rng.randn(n, 2) * 0.3], 1)
    v[:, 2:] = draw(total)
    # alternate / random / soft: 40 % of the anchors over the threshold are placed at a border, the kinds in rotation; the others keep
    # their random regression values, and some of those rects miss the image.  The other patterns are to reach the compaction as
    # they are: every anchor over the threshold gets a rect around the image's centre (BORDER_CENTRE).
    border = np.full(total, -1)
    on = np.nonzero(flags)[0]
    at_border = pattern in ("alternate", "random", "soft")
    chosen = on[rng.rand(on.size) < 0.4] if at_border else on
    aw64, ah64 = aw.astype(np.float64), ah.astype(np.float64)
    all_idx = _all_idx(H, W)
    for j, n in enumerate(chosen):
        l, a, y, x = all_idx[n]
        x0, x1 = aw64[l, a, x]
        y0, y1 = ah64[l, a, y]
        tx, ty = (IMG_W / 2 - x0) / (x1 - x0), (IMG_H / 2 - y0) / (y1 - y0)     # the other axis: well inside
        if not at_border:
            border[n] = BORDER_CENTRE
            v[n, 2:4] = (tx, ty)
            continue
        kind = j % 8
        side, inside = kind // 2, kind % 2
        border[n] = kind
        d = BORDER if inside else -BORDER
        if side == 0:
            tx = (IMG_W - d - x0) / (x1 - x0)
        elif side == 1:
            tx = (-(x1 - x0) + d - x0) / (x1 - x0)
        elif side == 2:
            ty = (IMG_H - d - y0) / (y1 - y0)
        else:
            ty = (-(y1 - y0) + d - y0) / (y1 - y0)
        v[n, 2:] = (tx, ty, 0.0, 0.0)
    # an anchor of the random share that came to lie within the margin of a border is drawn again
    for _ in range(20):
        maps = _to_maps(v, H, W)
        want = scan_ref(maps, H, W, aw, ah, IMG_W, IMG_H, THR)
        bad = np.nonzero((want["ovl_margin"].min(1) < 4 * MARGIN) & (border < 0))[0]
        if bad.size == 0:
            break
        v[bad, 2:] = draw(bad.size)
    return dict(name=name, pattern=pattern, maps=maps, H=H, W=W, aw=aw, ah=ah, want=want, flags=flags, border=border, total=total)


def _all_idx(H, W):
    """0-based (layer, aspect, y, x) per anchor in scan order"""
    out = []
    for l in range(4):
        for y in range(H[l]):
            for x in range(W[l]):
                for a in range(3):
                    out.append((l, a, y, x))
    return out


def _to_maps(v, H, W):
    """per-anchor values [total][6] in scan order -> four fp32 maps [18][H][W]"""
    maps, o = [], 0
    for l in range(4):
        n = 3 * H[l] * W[l]
        m = v[o:o + n].reshape(H[l], W[l], 3, 6).transpose(2, 3, 0, 1).reshape(18, H[l], W[l])
        maps.append(np.ascontiguousarray(m, np.float32))
        o += n
    return maps


def scan_caps(count, total):
    """the four caps of a problem with `count` matches: none, one short, exact, roomy"""
    return [0, max(count - 1, 0), count, total + 5]


# ---------------------------------------------------------------------------------------------- RPN loss problems
LOSS_SIZES = SCAN_SIZES["n2490"]
ONE_M = 1.0 - 2.0 ** -24                                   # the fp32 just below 1
Z_EDGES = (0.0, 1.0, -1.0, ONE_M, -ONE_M, 3.0, -3.0)      # t - tgt of the SmoothL1 switch cases
LOGIT_GAPS = (None, 0.0, 100.0, -100.0, 1.0e4, -1.0e4)    # v1 - v0; None: random
DYADIC_TGT = (0.0, -0.5, 0.25)
BGCLASS = 17


def _loss_anchors(rng, E, sizes):
    """E distinct 1-based (layer, aspect, y, x): first the (1, 1) and (H, W) corners of every layer and aspect, starting with the
    highest address, then random others; shuffled, so that corners fall among positives and negatives"""
    corners = []
    for l in range(3, -1, -1):
        for a in range(2, -1, -1):
            corners += [(l + 1, a + 1, sizes[l][0], sizes[l][1]), (l + 1, a + 1, 1, 1)]
    every = [(l + 1, a + 1, y + 1, x + 1) for l in range(4) for a in range(3) for y in range(sizes[l][0]) for x in range(sizes[l][1])]
    rest = [every[i] for i in rng.permutation(len(every)) if every[i] not in set(corners)]
    pick = (corners + rest)[:E]
    return [pick[i] for i in rng.permutation(len(pick))]


def _fill_example(rng, maps, k, key, pos, exact_only=False, first=True):
    """Writes the six head values of example number k at anchor `key` (only when `first`: a later example at the same anchor
    shares them) and returns (anchor rect, roi rect) of a positive.
    Kinds rotate with k: logit gaps through LOGIT_GAPS; a positive is `general` (arbitrary doubles) or an `edge` case: an anchor
    of 64 x 32 at a multiple of 1/4, a roi of the same extent at a dyadic offset -- tgt[0..1] exact, tgt[2..3] = log 1 = 0 -- and
    t = tgt + one of Z_EDGES per component.  exact_only: gaps beyond EXACT_LOGIT_GAP only, tgt[0..1] any multiple of 2^-10 in
    [-1/4, 1/4] and t = 1/4 + j 2^-23 with a random |j| < 2^21 (every |t - tgt| is below 1: the gradients are the differences
    themselves).  Every addend is then free of exp and log, and the fp32 sum of several of them depends on their order."""
    l, a, y, x = (v - 1 for v in key)
    m = maps[l]
    val = np.zeros(6, np.float32)
    gaps = LOGIT_GAPS[2:] if exact_only else LOGIT_GAPS
    gap = gaps[k % len(gaps)]
    val[0] = rng.randn() * 2.0
    val[1] = F32(rng.randn() * 2.0) if gap is None else F32(val[0] + F32(gap))
    val[2:] = rng.randn(4)
    r = None
    if pos and not exact_only and k % 3 == 0:       # general
        x0, y0 = rng.uniform(0, 200, 2)
        w, h = rng.uniform(10, 150, 2)
        rw, rh = w * math.exp(rng.uniform(-0.4, 0.4)), h * math.exp(rng.uniform(-0.4, 0.4))
        rx, ry = x0 + rng.uniform(-0.3, 0.3) * w, y0 + rng.uniform(-0.3, 0.3) * h
        val[2:] = rng.randn(4) * np.array([1.0, 1.0, 0.5, 0.5])
        r = (x0, y0, x0 + w, y0 + h), (rx, ry, rx + rw, ry + rh)
    elif pos:
        x0, y0 = rng.randint(0, 800, 2) * 0.25
        j = k if exact_only else (k // 3) * 2 + (k % 3 - 1)       # the edge cases' own counter
        t0, t1 = DYADIC_TGT[j % 3], DYADIC_TGT[(j // 3) % 3]
        if exact_only:      # any multiple of 2^-10 in [-1/4, 1/4]: examples that share an anchor differ in their targets
            t0, t1 = rng.randint(-256, 257, 2) * 2.0 ** -10
        r = ((x0, y0, x0 + 64.0, y0 + 32.0), (x0 + t0 * 64.0, y0 + t1 * 32.0, x0 + t0 * 64.0 + 64.0, y0 + t1 * 32.0 + 32.0))
        tgt = (t0, t1, 0.0, 0.0)
        for c in range(4):
            if exact_only:
                val[2 + c] = F32(0.25 + rng.randint(-2 ** 21 + 1, 2 ** 21) * 2.0 ** -23)
            else:
                val[2 + c] = F32(tgt[c] + Z_EDGES[(j + 2 * c) % len(Z_EDGES)])
    if first:
        m[a * 6:a * 6 + 6, y, x] = val
    return r


@functools.lru_cache(maxsize=None)
def loss_case(E, npos, dup=0):
    """One frcnn_rpn_loss problem on LOSS_SIZES.  dup = 0: E distinct anchors, kinds rotating (see _fill_example).  dup = k > 0:
    an exact_only problem in which DUP_ANCHORS anchors are named by k positives each, the first of them by two negatives
    as well, among distinct others.  -> dict(maps, deltas0, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, bgclass, want)"""
    sizes = LOSS_SIZES
    rng = np.random.RandomState(50000 + 1000 * dup + 7 * E + npos)
    maps = [rng.randn(18, h, w).astype(np.float32) for h, w in sizes]
    # (magnitudes over four decades: where an element is large, every addition to it rounds)
    deltas0 = [(rng.randn(18, h, w) * 10.0 ** rng.uniform(-2.0, 2.0, (18, h, w))).astype(np.float32) for h, w in sizes]
    for d in deltas0:
        d[d == 0] = 1.0
    nneg = E - npos
    if dup:
        nd = DUP_ANCHORS
        base = _loss_anchors(rng, E - nd * (dup - 1) - 2, sizes)
        singles = npos - nd * dup                      # positives that name an anchor of their own
        keys = [base[i] for i in range(nd) for _ in range(dup)] + list(base[nd:nd + singles])
        keys = [keys[i] for i in rng.permutation(len(keys))]
        negs = list(base[nd + singles:]) + [base[0], base[0]]
        keys = keys + [negs[i] for i in rng.permutation(len(negs))]
        assert singles >= 0 and len(keys) == E and len(negs) == nneg
    else:
        keys = _loss_anchors(rng, E, sizes)
    ex_idx = np.array(keys, np.int32).reshape(E, 4)
    ex_anchor = np.zeros((E, 4))
    ex_roi = np.zeros((max(npos, 1), 4))
    ex_class = np.zeros(max(npos, 1), np.int32)
    seen = set()
    for e, key in enumerate(keys):
        pos = e < npos
        r = _fill_example(rng, maps, e, key, pos, exact_only=bool(dup), first=key not in seen)
        seen.add(key)
        if pos:
            ex_anchor[e], ex_roi[e] = r
            ex_class[e] = 1 + (e * 5) % (BGCLASS - 1)
        else:
            x0, y0 = rng.uniform(0, 200, 2)
            ex_anchor[e] = (x0, y0, x0 + rng.uniform(10, 150), y0 + rng.uniform(10, 150))
    want = rpn_loss_ref(maps, deltas0, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, BGCLASS)
    return dict(maps=maps, deltas0=deltas0, ex_idx=ex_idx, ex_anchor=ex_anchor, ex_roi=ex_roi, ex_class=ex_class, npos=npos,
                nneg=nneg, bgclass=BGCLASS, want=want, sizes=sizes, dup=dup)


# (E, npos) of the distinct-anchor problems: the issue's E values, then all-negative and all-positive
LOSS_CASES = ((1, 1), (63, 20), (64, 33), (65, 64), (300, 128), (65, 0), (64, 64))
DUP_CASES = (2, 3, 7)
DUP_E, DUP_NPOS, DUP_ANCHORS = 64, 48, 6


# ---------------------------------------------------------------------------------------------- loss_accumulate problems
ACC_E = (1, 63, 64, 65, 300, 0)


@functools.lru_cache(maxsize=None)
def accumulate_case(E):
    """-> (ex_loss float64 [E][2] whose magnitudes span twelve decades, both signs; acc0 float64 [2], non-zero)"""
    rng = np.random.RandomState(900 + E)
    ex = 10.0 ** rng.uniform(-6.0, 6.0, (max(E, 1), 2)) * np.where(rng.rand(max(E, 1), 2) < 0.3, -1.0, 1.0)
    if E >= 2:
        ex[0, :] = (1.0e-6, 1.0e6)
        ex[1, :] = (1.0e6, 1.0e-6)
    return ex[:E].copy() if E else np.zeros((0, 2)), np.array([3.25e3, -7.5e-2])


# ---------------------------------------------------------------------------------------------- cnet_losses problems
CNET_R = (1, 63, 64, 65, 257, 600)
CNET_NCLS = (2, 17, 201)
CNET_Z = Z_EDGES + (ONE_M, -1.0)       # nine entries: the edge values, cycled over the first elements of the difference


def cnet_npos(R):
    return sorted({0, R // 2, R})


@functools.lru_cache(maxsize=None)
def cnet_losses_case(R, npos, ncls):
    """-> dict(crout, crtarget, ccout, cctarget, loss0, want).  The first 2 * len(CNET_Z) elements of crout - crtarget take the
    values of CNET_Z exactly (in a positive row through crout, in a negative row -- crout is zeroed there -- through crtarget);
    the targets include class 1 and class ncls."""
    rng = np.random.RandomState(77000 + 1000 * R + 10 * ncls + (npos * 3) // max(R, 1))
    crt = (rng.randint(-8, 9, (R, 4)) * 0.25).astype(np.float32)
    cro = (crt + rng.randn(R, 4) * 1.2).astype(np.float32)
    flat_t, flat_o = crt.reshape(-1), cro.reshape(-1)
    for i in range(min(R * 4, 2 * len(CNET_Z))):
        z = CNET_Z[i % len(CNET_Z)]
        if i // 4 < npos:
            flat_t[i] = 0.0
            flat_o[i] = F32(z)
        else:
            flat_t[i] = F32(-z)
    # log-probabilities: a LogSoftMax of random logits, as the net would hand over
    lg = rng.randn(R, ncls) * 2.0
    cco = (lg - np.log(np.exp(lg).sum(1, keepdims=True))).astype(np.float32)
    tgt = rng.randint(1, ncls + 1, R)
    tgt[0] = ncls
    tgt[-1] = 1 if R > 1 else tgt[-1]
    if R > 2:
        tgt[1] = 1
    cct = tgt.astype(np.float32)
    want = cnet_losses_ref(cro, crt, cco, cct, R, npos, ncls)
    return dict(crout=cro, crtarget=crt, ccout=cco, cctarget=cct, loss0=np.array([12.5, 0.375]), want=want, R=R, npos=npos, ncls=ncls)


# ---------------------------------------------------------------------------------------------- decode problems
DECODE_R = (1, 63, 64, 65, 300)
DECODE_NCLS = (1, 2, 17, 201)
DECODE_KINDS = ("quantised", "last_column", "all_equal")


@functools.lru_cache(maxsize=None)
def decode_case(R, ncls, kind):
    """-> fp32 [R][ncls] log-probabilities.  quantised: multiples of 1/4 in [-2, 0]: exact ties in most rows.  last_column: the same
    with the row's maximum raised in the last column alone.  all_equal: one value everywhere."""
    rng = np.random.RandomState(31000 + 100 * R + ncls)
    x = (-rng.randint(0, 9, (R, ncls)) * 0.25).astype(np.float32)
    if kind == "last_column":
        x[:, -1] = 0.25
    elif kind == "all_equal":
        x[:] = -1.5
    return x
