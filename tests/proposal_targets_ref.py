"""A numpy restatement of frcnn_proposal_targets_batch (include/frcnn_hip.h) and the case tables of its tests.

targets_ref(case, b) is one segment: uint32 keys through masked uint64 arithmetic, the fp64 IoU of Rect.lua:126-141 in the stated
order of operations (numpy rounds every operation on its own), first-maximum matching, the quotas, the ordered output.  It also
reports which branches of the rule the segment reached (`reached`), so that the host test can show that the tables leave none
out.  The w / h targets go through numpy's fp64 log, the device's through its own: each within an ulp of the true value."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
BRANCHES = ("cut_fg", "cut_bg", "cut_both", "cut_none", "tie", "at_fg_iou", "at_bg_lo", "at_bg_hi", "nan_quotient", "non_finite",
            "zero_size", "G0", "R0", "G0_R0", "r_dev_over_cap", "no_include_gt", "quota_0", "quota_batch", "ignored_between", "G0_fg_iou_0")


def keys_ref(seed, n, b):
    """the keys of rows 0 ... n - 1 of segment b (uint32)"""
    i = np.arange(n, dtype=np.uint64)
    x = (np.uint64(seed & 0xFFFFFFFF) + np.uint64(0x9E3779B9) * (i + np.uint64(1)) + np.uint64(0x85EBCA6B) * np.uint64(b)) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def candidates_ref(case):
    """(c N x 4 float64, readable N bool): the ground truth in front (include_gt), then the first min(max(r_dev, 0), r_cap) picks"""
    rect = np.asarray(case["rect"], np.float64).reshape(-1, 4)
    pick = np.asarray(case["pick"], np.int64).reshape(-1)
    gt = np.asarray(case["gt_rect"], np.float64).reshape(-1, 4)
    R = min(max(int(case["r_dev"]), 0), int(case["r_cap"]))
    p = pick[:R]
    stride = int(case.get("match_stride", max(len(rect), int(case["r_cap"]))))
    ok = (p >= 1) & (p <= stride)
    rows = np.zeros((R, 4), np.float64)
    rows[ok] = rect[p[ok] - 1]
    if case["include_gt"]:
        return np.concatenate([gt, rows], 0), np.concatenate([np.ones(len(gt), bool), ok])
    return rows, ok


def iou_matrix(c, gt):
    """Rect.IoU(candidate, gt) for every pair, N x G; a quotient that is not a number is 0 (also returned: where that happened)"""
    with np.errstate(all="ignore"):
        c0, c1, c2, c3 = (c[:, k][:, None] for k in range(4))
        g0, g1, g2, g3 = (gt[:, k][None, :] for k in range(4))
        minx = np.where(g0 > c0, g0, c0); miny = np.where(g1 > c1, g1, c1)     # max(a, b): b when b > a, else a
        maxx = np.where(g2 < c2, g2, c2); maxy = np.where(g3 < c3, g3, c3)     # min(a, b): b when b < a, else a
        inter = np.where((maxx >= minx) & (maxy >= miny), (maxx - minx) * (maxy - miny), 0.0)
        ca = (c2 - c0) * (c3 - c1)
        ga = (g2 - g0) * (g3 - g1)
        den = (ca + ga) - inter
        q = inter / den
    nan = np.isnan(q)
    return np.where(nan, 0.0, q), nan


def targets_ref(case, b=0):
    gt = np.asarray(case["gt_rect"], np.float64).reshape(-1, 4)
    gcls = np.asarray(case["gt_class"], np.int32).reshape(-1)
    G = len(gt)
    fg_iou, bg_lo, bg_hi = float(case["fg_iou"]), float(case["bg_lo"]), float(case["bg_hi"])
    fg_quota, batch = int(case["fg_quota"]), int(case["batch"])
    c, readable = candidates_ref(case)
    N = len(c)
    reached = set()
    R = N - (G if case["include_gt"] else 0)
    if G == 0: reached.add("G0")
    if R == 0: reached.add("R0")
    if G == 0 and R == 0: reached.add("G0_R0")
    if int(case["r_dev"]) > int(case["r_cap"]): reached.add("r_dev_over_cap")
    if not case["include_gt"]: reached.add("no_include_gt")
    if fg_quota == 0: reached.add("quota_0")
    if fg_quota == batch: reached.add("quota_batch")
    if G == 0 and fg_iou == 0.0 and R > 0: reached.add("G0_fg_iou_0")
    empty = dict(counts=(0, 0, 0, 0), roi=np.zeros((0, 4)), crtarget=np.zeros((0, 4), np.float32), cctarget=np.zeros(0, np.float32),
                 src=np.zeros(0, np.int32), gt_idx=np.zeros(0, np.int32), iou=np.zeros(0), reached=reached)
    if N == 0:
        return empty
    with np.errstate(all="ignore"):
        w, h = c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
    finite = np.all(np.isfinite(c), 1)
    valid = readable & finite & (w > 0) & (h > 0)
    if np.any(readable & ~finite): reached.add("non_finite")
    if np.any(readable & finite & ~((w > 0) & (h > 0))): reached.add("zero_size")
    if G:
        q, nan = iou_matrix(c, gt)
        best_g = np.argmax(q, 1).astype(np.int32)          # the first maximum: the lowest g wins a tie
        best = q[np.arange(N), best_g]
        if np.any(nan[valid]): reached.add("nan_quotient")
        if np.any(valid & ((q == best[:, None]).sum(1) > 1) & (best > 0)): reached.add("tie")
    else:
        best_g = np.full(N, -1, np.int32)
        best = np.zeros(N)
    fg = valid & (best_g >= 0) & (best >= fg_iou)      # foreground needs a box: none with G = 0, whatever fg_iou is
    bg = valid & ~fg & (bg_lo <= best) & (best < bg_hi)
    if np.any(valid & (best == fg_iou)): reached.add("at_fg_iou")
    if np.any(valid & (best == bg_lo) & bg): reached.add("at_bg_lo")
    if np.any(valid & (best == bg_hi) & ~fg): reached.add("at_bg_hi")
    if np.any(valid & ~fg & ~bg): reached.add("ignored_between")
    nfg, nbg = int(fg.sum()), int(bg.sum())
    F = min(nfg, fg_quota)
    Bq = min(nbg, batch - F)
    reached.add({(True, True): "cut_both", (True, False): "cut_fg", (False, True): "cut_bg", (False, False): "cut_none"}[nfg > F, nbg > Bq])
    key = keys_ref(int(case["seed"]), N, b)

    def kept(mask, quota):
        rows = np.nonzero(mask)[0]
        if len(rows) > quota:
            rows = np.sort(rows[np.argsort(key[rows], kind="stable")[:quota]])   # the smallest keys, back in candidate order
        return rows
    rows = np.concatenate([kept(fg, F), kept(bg, Bq)]).astype(np.int64)
    S = F + Bq
    assert len(rows) == S
    crt = np.zeros((S, 4), np.float32)
    cct = np.full(S, float(case["bgclass"]), np.float32)
    if F:
        a = c[rows[:F]]; g = gt[best_g[rows[:F]]]
        with np.errstate(all="ignore"):
            aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
            t = np.stack([(g[:, 0] - a[:, 0]) / aw, (g[:, 1] - a[:, 1]) / ah, np.log((g[:, 2] - g[:, 0]) / aw),
                          np.log((g[:, 3] - g[:, 1]) / ah)], 1)
        crt[:F] = t.astype(np.float32)
        cct[:F] = gcls[best_g[rows[:F]]].astype(np.float32)
    return dict(counts=(nfg, nbg, F, Bq), roi=c[rows].copy(), crtarget=crt, cctarget=cct, src=rows.astype(np.int32),
                gt_idx=best_g[rows].copy(), iou=best[rows].copy(), reached=reached)


# ---- the case tables -------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(include_gt=True, fg_iou=0.5, bg_lo=0.1, bg_hi=0.5, fg_quota=8, batch=32, bgclass=21, seed=0)


def _case(name, rect, pick, gt_rect, gt_class, r_dev=None, r_cap=None, **kw):
    rect = np.asarray(rect, np.float64).reshape(-1, 4)
    pick = np.asarray(pick, np.int64).reshape(-1)
    c = dict(DEFAULTS)
    c.update(name=name, rect=rect, pick=pick, gt_rect=np.asarray(gt_rect, np.float64).reshape(-1, 4),
             gt_class=np.asarray(gt_class, np.int32).reshape(-1), r_dev=len(pick) if r_dev is None else r_dev,
             r_cap=len(pick) if r_cap is None else r_cap)
    c.update(kw)
    return c


def scene(seed, G, R, extra_rows=3, W=400.0, H=225.0):
    """G ground-truth boxes and R candidates around them: a third jittered a little (foreground), a third jittered a lot, a third
    anywhere; the rect table holds extra rows nobody picks, in shuffled order, and pick is a permutation into it"""
    rng = np.random.RandomState(seed)
    gw = rng.uniform(20, 120, G); gh = rng.uniform(20, 100, G)
    gx = rng.uniform(0, W - gw); gy = rng.uniform(0, H - gh)
    gt = np.stack([gx, gy, gx + gw, gy + gh], 1).reshape(-1, 4)
    n = R + extra_rows
    w = rng.uniform(10, 150, n); h = rng.uniform(10, 120, n)
    x = rng.uniform(0, W - 10, n); y = rng.uniform(0, H - 10, n)
    rect = np.stack([x, y, x + w, y + h], 1)
    if G:
        kind = rng.randint(0, 3, n)
        which = rng.randint(0, G, n)
        for i in range(n):
            if kind[i] < 2:
                j = 0.08 if kind[i] == 0 else 0.45
                d = rng.uniform(-j, j, 4) * np.array([gw[which[i]], gh[which[i]]] * 2)
                rect[i] = gt[which[i]] + d
    pick = rng.permutation(n)[:R] + 1
    return rect, pick, gt, rng.randint(1, 21, G)


def rule_cases():
    """every branch of the rule, each reached by at least two cases (test_proposal_targets_host checks it)"""
    out = []
    for k, seed in enumerate((3, 4)):
        rect, pick, gt, cls = scene(seed, 4, 90)
        out.append(_case("cut_both_%d" % k, rect, pick, gt, cls, fg_quota=4, batch=16, seed=seed))
        out.append(_case("cut_fg_only_%d" % k, rect, pick, gt, cls, fg_quota=2, batch=200, seed=seed + 10))
        out.append(_case("cut_bg_only_%d" % k, rect, pick, gt, cls, fg_quota=60, batch=60 + k, seed=seed + 20, bg_lo=0.0))
        out.append(_case("cut_none_%d" % k, rect, pick, gt, cls, fg_quota=100, batch=400, seed=seed + 30))
        out.append(_case("quota_0_%d" % k, rect, pick, gt, cls, fg_quota=0, batch=24, seed=seed + 40))
        out.append(_case("quota_batch_%d" % k, rect, pick, gt, cls, fg_quota=6 + k, batch=6 + k, seed=seed + 50))
        out.append(_case("no_include_gt_%d" % k, rect, pick, gt, cls, include_gt=False, seed=seed + 60))
        out.append(_case("r_dev_over_cap_%d" % k, rect, pick, gt, cls, r_dev=len(pick) + 7 + k, r_cap=40 + k, seed=seed + 70))
        out.append(_case("r_dev_negative_%d" % k, rect, pick, gt, cls, r_dev=-3 - k, seed=seed + 80))
        out.append(_case("G0_%d" % k, rect, pick, np.zeros((0, 4)), [], seed=seed + 90, bg_lo=0.0, batch=10 + k))
        out.append(_case("R0_%d" % k, rect, pick[:0], gt, cls, seed=seed + 100))
        out.append(_case("G0_R0_%d" % k, rect, pick[:0], np.zeros((0, 4)), [], seed=seed + 110, include_gt=bool(k)))
        out.append(_case("G0_bg_lo_positive_%d" % k, rect, pick, np.zeros((0, 4)), [], seed=seed + 120, bg_lo=0.05))
        # no box and fg_iou = 0: best_iou = 0 reaches fg_iou, but foreground needs a match, and bg_hi <= fg_iou leaves no
        # background below 0 either -- every candidate is ignored, nothing is stored
        out.append(_case("G0_fg_iou_0_%d" % k, rect, pick, np.zeros((0, 4)), [], seed=seed + 130, fg_iou=0.0, bg_lo=-0.5 * k,
                         bg_hi=0.0, include_gt=bool(k)))
    # equal IoU against two boxes: the candidate covers both halves alike (0.5 each) -- the lower g wins; also exactly at fg_iou
    halves = [[0, 0, 10, 5], [0, 5, 10, 10]]
    for k in range(2):
        gts = halves if k == 0 else [[50, 50, 60, 60]] + halves[::-1]
        out.append(_case("tie_%d" % k, [[0, 0, 10, 10], [100, 100, 130, 140]], [1, 2], gts, list(range(3, 3 + len(gts))), bg_lo=0.0))
    # IoU exactly at the thresholds: 10 x 10 against 10 x 5 is 0.5, against 5 x 5 is 0.25
    for k in range(2):
        o = 16.0 * k
        rect = [[o, 0, o + 10, 10], [o + 40, 0, o + 50, 10], [o + 80, 0, o + 90, 10]]
        gts = [[o, 0, o + 10, 5], [o + 40, 0, o + 45, 5], [o + 80, 0, o + 82, 2]]
        out.append(_case("at_fg_iou_%d" % k, rect, [3, 1, 2], gts, [1, 2, 3], fg_iou=0.5, bg_lo=0.25, bg_hi=0.5))
        out.append(_case("at_bg_hi_%d" % k, rect, [1, 2, 3], gts, [1, 2, 3], fg_iou=0.75, bg_lo=0.04, bg_hi=0.5))
        out.append(_case("at_bg_lo_%d" % k, rect, [2, 3, 1], gts, [1, 2, 3], fg_iou=0.5, bg_lo=0.25, bg_hi=0.25 + 0.125 * k))
    # a 0 / 0 quotient: a ground-truth "box" of negative height whose area cancels the candidate's, no intersection
    for k in range(2):
        out.append(_case("nan_quotient_%d" % k, [[0, 0, 2, 2], [20, 20, 40, 40]], [1, 2], [[10, 10, 12, 8]] + [[20, 20, 40, 38]] * k,
                         [5] + [6] * k, bg_lo=0.0, include_gt=False))
    # candidates that are ignored whatever they overlap: a coordinate that is not finite, a width or height <= 0
    for k, bad in enumerate((np.nan, np.inf)):
        rect, pick, gt, cls = scene(20 + k, 3, 30)
        rect[pick[0] - 1, k] = bad
        rect[pick[1] - 1, 2] = -bad if k else bad
        rect[pick[2] - 1, 2] = rect[pick[2] - 1, 0]             # width 0
        rect[pick[3] - 1, 3] = rect[pick[3] - 1, 1] - 1.0       # height < 0
        out.append(_case("bad_candidates_%d" % k, rect, pick, gt, cls, seed=5 + k, bg_lo=0.0))
    return out


SIZE_N = (1, 63, 64, 65, 255, 256, 257, 4096)
SIZE_G = (0, 1, 2, 64)


def size_cases():
    """N = G' + R candidates at every size where the kernel's tiles and waves change roles, G = 0, 1, 2, 64 (include_gt on and off)"""
    out = []
    for k, N in enumerate(SIZE_N):
        for G in SIZE_G:
            include_gt = (k + G) % 2 == 0 and G < N
            R = N - G if include_gt else N
            if R > 4096 - 64:
                R, include_gt = 4096 - 64, True
                if G != 64:
                    continue                                    # (N = 4096 needs the 64 boxes in front)
            rect, pick, gt, cls = scene(100 + 7 * k + G, G, R)
            out.append(_case("N%d_G%d" % (R + (G if include_gt else 0), G), rect, pick, gt, cls, include_gt=include_gt,
                             fg_quota=max(1, N // 8), batch=max(2, N // 3), seed=1000 + N + G, bg_lo=0.0))
    return out


def batch_cases():
    """B = 3 segments with different counts, one of them empty, on common strides"""
    a = scene(31, 5, 300); b = scene(32, 2, 70)
    common = dict(fg_quota=10, batch=40, seed=77, bg_lo=0.0)
    return [_case("seg0", a[0], a[1], a[2], a[3], **common),
            _case("seg1_empty", np.zeros((1, 4)), [], np.zeros((0, 4)), [], **common),
            _case("seg2", b[0], b[1], b[2], b[3], **common)]
