"""The numpy restatement of frcnn_detect_class_boxes_batch (include/frcnn_hip_classbox.h; csrc/class_boxes.hip) and the problems
its tests run.  Nothing here looks at the device's results.

  a row j < min(K[b], row_stride) of frame b:  r = keep_row[b][j] (0-based candidate), c = kc[b][j] (1-based class)
  the deltas   d = b[4 (c-1) .. 4 c) + W[4 (c-1) .. 4 c) @ feat[row0[b] + r], the product taken in float64 (box_head_ref.forward:
               the restatement the box head's own tests use); a class outside 1 ... C gives d = 0
  the box      Anchors.anchorToInput(rect[b][pick[b][r] - 1], d) in double, one rounding per operation (decode(), below: the
               statement of Anchors.lua:245-252 that csrc/anchor_decode.h makes on the device); bb[j][0..3] = float32 of it
  everything else -- bb[j][4], the rows at and behind K[b], other frames -- stays as it was.

decode() reads exp() of the host libm where the device reads the HIP library's: both are within an ulp of the true value
(detect_classes_ref.py's note), so x0 and y0 -- products and sums only -- are the device's bits, and x1 and y1 agree within
decode_bound().  The match rows of a problem come from detect_classes_ref.problem, the builder the class test's own tests use."""
import numpy as np

import box_head_ref as BH
import detect_classes_ref as D

SENT = -12345.0          # what the outputs hold before a launch
U64 = 2.0 ** -53         # unit roundoff of fp64


def decode(anchor, d):
    """anchor n x 4 float64 rects, d n x 4 deltas (any float type; taken to double as the device takes its fp32 deltas) ->
    n x 4 float64: x0 = d0 * aw + ax0, y0 = d1 * ah + ay0, x1 = x0 + exp(d2) * aw, y1 = y0 + exp(d3) * ah, every operation
    rounded on its own (numpy float64 arithmetic does not contract)."""
    a = np.asarray(anchor, np.float64).reshape(-1, 4)
    t = np.asarray(d).astype(np.float64).reshape(-1, 4)
    aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    x0 = t[:, 0] * aw
    x0 = x0 + a[:, 0]
    y0 = t[:, 1] * ah
    y0 = y0 + a[:, 1]
    ew, eh = np.exp(t[:, 2]) * aw, np.exp(t[:, 3]) * ah
    return np.stack([x0, y0, x0 + ew, y0 + eh], 1)


def decode_bound(anchor, d):
    """n x 4: how far the device's box may lie from decode()'s.  Columns 0 and 1: 0 (the same IEEE operations).  Columns 2 and 3:
    the two exp() are each within 1 ulp of the true value, so they differ by at most 2 ulp = 4 u |e|; the product with the
    extent rounds once more on each side (2 u on top, with the second-order terms 7 u |e w| covers it), and the final sum rounds
    once on each side (2 u |x1|): 7 u |e w| + 2 u |x1|."""
    a = np.asarray(anchor, np.float64).reshape(-1, 4)
    t = np.asarray(d).astype(np.float64).reshape(-1, 4)
    ref = decode(a, t)
    aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    out = np.zeros_like(ref)
    out[:, 2] = 7 * U64 * np.abs(np.exp(t[:, 2]) * aw) + 2 * U64 * np.abs(ref[:, 2])
    out[:, 3] = 7 * U64 * np.abs(np.exp(t[:, 3]) * ah) + 2 * U64 * np.abs(ref[:, 3])
    return out


def deltas(P):
    """-> per frame (d float64[k][4], mag float64[k][4], rows k) for the frame's k = min(K, row_stride) rows: the product in
    float64 and the magnitude box_head_ref.forward_bound scales with."""
    out = []
    Cn = P["W"].shape[0] // 4
    for b in range(P["B"]):
        k = min(int(P["K"][b]), P["row_stride"])
        r, c = P["keep_row"][b, :k].astype(np.int64), P["kc"][b, :k].astype(np.int64)
        sel = np.where((c >= 1) & (c <= Cn), c, 0)
        x = P["feat"][P["row0"][b] + r] if k else np.zeros((0, P["feat"].shape[1]), np.float32)
        d, mag = BH.forward(x, P["W"], P["b"], sel) if k else (np.zeros((0, 4)), np.zeros((0, 4)))
        out.append((d, mag, k))
    return out


def class_boxes(P, d32=None):
    """The whole launch on problem P -> dict(bb, r2): the arrays after it.  d32 (optional): per frame the fp32 deltas to decode
    (the device's own, for the bit-level checks of the decode); default: the float64 product rounded to fp32."""
    bb, r2 = P["bb"].copy(), P["r2"].copy()
    dl = deltas(P)
    for b in range(P["B"]):
        d, _, k = dl[b]
        if not k:
            continue
        t = np.asarray(d32[b], np.float32) if d32 is not None else d.astype(np.float32)
        anchor = P["rect"][b][P["pick"][b][P["keep_row"][b, :k]] - 1]
        q = decode(anchor, t)
        r2[b, :k] = q
        bb[b, :k, :4] = q.astype(np.float32)
    return dict(bb=bb, r2=r2)


def problem(seed, nf, Cn, B, cands, integer=False, Ks=None):
    """A chunk of B frames with `cands` candidates each (0: a frame without any).  feat: every frame's rows at a row0 that is not
    zero and not monotone in b; rect / pick: detect_classes_ref.problem's match rows (cands + 7 of them, pick a permutation's
    head, not the identity); the class rows: per candidate 1 ... min(3, C) + 1 rows, classes NOT sorted within a candidate,
    among them (where there is room) one class 0 and one class C + 1; K per frame from Ks ("zero", "mid", "full", "over": 0, about
    half the rows, exactly row_stride, above it), cycling.  Outputs sentinel-filled.  integer: small-integer features, weights and
    biases with zero rows for the two extent deltas (exp(0) = 1 on every library), integer match rects -- every result exact in
    fp32 and fp64."""
    rng = np.random.RandomState(seed)
    Ks = Ks or ("mid", "over", "zero", "full")
    order = rng.permutation(B)                   # frame b's features lie in slot order[b]: row0 not monotone (B > 1)
    if B > 1 and list(order) == sorted(order):
        order = order[::-1]
    slot = cands + 2
    row0 = [3 + int(order[b]) * slot for b in range(B)]
    N = 3 + B * slot + 1
    if integer:
        feat = rng.randint(-3, 4, (N, nf)).astype(np.float32)
        W = rng.randint(-2, 3, (4 * Cn, nf)).astype(np.float32)
        bias = rng.randint(-4, 5, 4 * Cn).astype(np.float32)
        W.reshape(Cn, 4, nf)[:, 2:] = 0
        bias.reshape(Cn, 4)[:, 2:] = 0
    else:
        feat = rng.standard_normal((N, nf)).astype(np.float32)
        W = (rng.standard_normal((4 * Cn, nf)) * (0.3 / np.sqrt(nf))).astype(np.float32)
        bias = (rng.standard_normal(4 * Cn) * 0.1).astype(np.float32)
    per = [[] for _ in range(B)]
    for b in range(B):
        for r in range(cands):
            n = 1 + int(rng.randint(0, min(3, Cn) + 1))
            cl = list(rng.permutation(Cn)[:min(n, Cn)] + 1)
            if n > len(cl) or r == 1:
                cl.append(0 if (r + b) % 2 else Cn + 1)        # no class: below and above the range
            if r == 0 and Cn >= 2:
                cl = sorted(cl, reverse=True)                 # (descending: not the order the class test emits)
            per[b].append([int(c) for c in cl])
    row_stride = max([sum(len(c) for c in f) for f in per] + [1])
    M = max(cands, 1) + 7
    rect = np.zeros((B, M, 4), np.float64)
    pick = np.ones((B, M), np.int64)
    kc = np.full((B, row_stride), 1, np.int32)
    keep_row = np.zeros((B, row_stride), np.int32)
    K = np.zeros(B, np.int32)
    for b in range(B):
        q = D.problem(seed * 31 + b, max(cands, 1), 3, special=False)
        rect[b] = np.rint(q["rect"]) if integer else q["rect"]
        if integer:
            rect[b][:, 2:] += 1.0                              # (a rounded extent may not vanish)
        pick[b, :max(cands, 1)] = q["pick"]
        rows = [(r, c) for r in range(cands) for c in per[b][r]]
        for j, (r, c) in enumerate(rows):
            keep_row[b, j], kc[b, j] = r, c
        # (the rows behind a frame's own keep valid candidates and classes: a K above the rows emitted must stay harmless)
        kind = Ks[b % len(Ks)] if cands else "zero"
        K[b] = dict(zero=0, mid=(len(rows) + 1) // 2, full=row_stride, over=row_stride + 5)[kind]
    bb = np.full((B, row_stride, 5), SENT, np.float32)
    r2 = np.full((B, row_stride, 4), SENT, np.float64)
    return dict(B=B, nf=nf, C=Cn, cands=cands, feat=feat, row0=row0, W=W, b=bias, rect=rect, pick=pick, kc=kc, keep_row=keep_row, K=K,
                bb=bb, r2=r2, row_stride=row_stride, per=per)


# the op-level cases of tests/test_gpu_class_boxes.py
NF = (1, 4, 7, 64, 260)      # fewer than 64 floats, a lane tail, the scalar path (7) and the vector path (4, 64, 260)
CLASSES = (1, 3, 17)
FRAMES = (1, 3)
CANDS = (0, 1, 5, 67)


def case_seed(nf, Cn, B, cands):
    return ((nf * 31 + Cn) * 7 + B) * 101 + cands
