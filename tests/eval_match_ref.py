"""The numpy restatement of frcnn_eval_match_batch (include/frcnn_hip_eval.h) and the case tables of its tests.

match_frame() is written as the LITERAL greedy loop of evaluation.mean_average_precision -- per threshold, per class, the
detections by decreasing confidence (a stable sort), `used` flags per ground-truth box -- and not as the kernel's rule ("the first
detection, in that order, among those that reach the box"), so that the kernel's reformulation is tested against the original.
Two things are spelled out that the original leaves to its callers: the confidence is compared as an fp32 value, and a
ground-truth class < 1 is no class.  IoU is Rect.IoU on numpy float64 scalars: every operation rounded on its own, 0 / 0 = NaN."""
import numpy as np


def iou(a, b):
    """Rect.IoU(a, b) (Rect.py: intersect, area) for two rows {minX, minY, maxX, maxY} of float64"""
    a = [np.float64(v) for v in a]
    b = [np.float64(v) for v in b]
    minx = b[0] if b[0] > a[0] else a[0]; miny = b[1] if b[1] > a[1] else a[1]      # max(a, b) of Python: b when b > a
    maxx = b[2] if b[2] < a[2] else a[2]; maxy = b[3] if b[3] < a[3] else a[3]
    inter = np.float64(0.0)
    if maxx >= minx and maxy >= miny:
        inter = (maxx - minx) * (maxy - miny)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def match_frame(rects, classes, conf, gt_rects, gt_classes, thr):
    """-> dict(tp uint32[n], gt int32[n] (1-based in the frame's list, 0: none), iou float64[n] (-1: no box)), rows in the order
    given.  The greedy loop, once per threshold."""
    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    classes = np.asarray(classes).reshape(-1).astype(np.int64)
    conf = np.asarray(conf, np.float32).reshape(-1)
    gt_rects = np.asarray(gt_rects, np.float64).reshape(-1, 4)
    gt_classes = np.asarray(gt_classes).reshape(-1).astype(np.int64)
    n = len(rects)
    tp = np.zeros(n, np.uint32); gt = np.zeros(n, np.int32); best_of = np.full(n, -1.0, np.float64)
    memo = {}

    def pair_iou(a, b):           # (the loop below asks for every pair once per threshold: the value is computed once)
        key = (a.ctypes.data, b.ctypes.data)
        if key not in memo:
            memo[key] = iou(a, b)
        return memo[key]
    for t, th in enumerate(thr):
        for cls in sorted(set(int(c) for c in gt_classes if c >= 1)):
            boxes = [j for j in range(len(gt_classes)) if gt_classes[j] == cls]
            dets = [k for k in range(n) if classes[k] == cls]
            dets.sort(key=lambda k: -float(conf[k]))            # stable: equal confidences keep their detection order
            used = [False] * len(boxes)
            for k in dets:
                best, best_j = -1.0, -1
                for j, g in enumerate(boxes):
                    v = pair_iou(rects[k], gt_rects[g])
                    if v > best:
                        best, best_j = v, j
                if best_j >= 0 and best >= th and not used[best_j]:
                    tp[k] |= np.uint32(1 << t); used[best_j] = True
                gt[k] = boxes[best_j] + 1 if best_j >= 0 else 0
                best_of[k] = best
    return dict(tp=tp, gt=gt, iou=best_of)


def keep_best(conf, M):
    """Detector.keep_best: the rows (ascending) of the M highest fp32 values, ties to the earlier row"""
    c = np.asarray(conf).astype(np.float32)
    return np.sort(np.argsort(-c, kind="stable")[:M])


def table(frame, thr, sel=None):
    """The rows of the frame's table that frcnn_eval_match_batch writes -- int32[k + 2][4] -- and its k overlaps (float64).
    frame: dict(rects, classes, conf, gt_rects, gt_classes[, counts: the gather's header]); sel: the rows matched (ascending),
    None: all of them."""
    n_all = len(frame["classes"])
    rows = np.arange(n_all) if sel is None else np.asarray(sel, np.int64)
    k = len(rows)
    cls = np.asarray(frame["classes"], np.int32).reshape(-1)[rows]
    conf = np.asarray(frame["conf"], np.float32).reshape(-1)[rows]
    m = match_frame(np.asarray(frame["rects"], np.float64).reshape(-1, 4)[rows], cls, conf, frame["gt_rects"], frame["gt_classes"], thr)
    tab = np.zeros((k + 2, 4), np.int32)
    tab[0] = frame.get("counts", (n_all,) * 4)
    tab[1] = (k, len(frame["gt_classes"]), len(thr), n_all)
    tab[2:, 0] = cls
    tab[2:, 1] = conf.view(np.int32)
    tab[2:, 2] = m["tp"].view(np.int32)
    tab[2:, 3] = m["gt"]
    return tab, m["iou"]


# ---- the hand cases: each is built to reach one rule; tp / gt are worked out by hand ---------------------------------------------
A, B2 = [0, 0, 10, 10], [4, 0, 14, 10]
HAND = [
    # two detections of one box, the later row with the higher confidence: the later row claims it
    dict(name="later_row_higher_confidence", rects=[A, [0, 0, 10, 9]], classes=[1, 1], conf=[0.5, 0.9], gt_rects=[A], gt_classes=[1],
         thr=[0.5], tp=[0, 1], gt=[1, 1], iou=[1.0, 0.9]),
    # equal fp32 confidences (0.7 and the double next to it round to one float): the earlier row
    dict(name="equal_confidences", rects=[[0, 0, 10, 9], A], classes=[1, 1], conf=[0.7, np.nextafter(0.7, 1.0)], gt_rects=[A],
         gt_classes=[1], thr=[0.5], tp=[1, 0], gt=[1, 1], iou=[0.9, 1.0]),
    # best box taken, second-best free and over the threshold: a false positive (the VOC rule).  [1,0,11,10]: 90/110 with A, 70/130 with B2
    dict(name="best_box_taken", rects=[A, [1, 0, 11, 10]], classes=[1, 1], conf=[0.9, 0.8], gt_rects=[A, B2], gt_classes=[1, 1],
         thr=[0.5], tp=[1, 0], gt=[1, 1], iou=[1.0, 90.0 / 110.0]),
    # two boxes at equal IoU: the first
    dict(name="equal_iou_first_box", rects=[A], classes=[2], conf=[0.3], gt_rects=[[50, 50, 60, 60], A, A], gt_classes=[2, 2, 2],
         thr=[0.5], tp=[1], gt=[2], iou=[1.0]),
    # IoU exactly 0.5 at threshold 0.5: >= passes
    dict(name="exactly_one_half", rects=[[0, 0, 2, 1]], classes=[1], conf=[0.4], gt_rects=[[0, 0, 1, 1]], gt_classes=[1],
         thr=[0.5], tp=[1], gt=[1], iou=[0.5]),
    # a box of another class with the larger overlap is not looked at
    dict(name="other_class_overlaps_more", rects=[A], classes=[1], conf=[0.4], gt_rects=[A, [0, 0, 10, 6]], gt_classes=[2, 1],
         thr=[0.5, 0.75], tp=[1], gt=[2], iou=[0.6]),
    # the higher confidence reaches the box at 0.5 only, the lower one claims it at 0.75
    dict(name="lower_confidence_claims_at_075", rects=[[0, 0, 10, 6], [0, 0, 10, 8]], classes=[1, 1], conf=[0.9, 0.5], gt_rects=[A],
         gt_classes=[1], thr=[0.5, 0.75], tp=[1, 2], gt=[1, 1], iou=[0.6, 0.8]),
    # two empty rects: NaN never wins; the box behind it, at IoU 0, does
    dict(name="empty_rects", rects=[[0, 0, 0, 0], [0, 0, 0, 0]], classes=[1, 2], conf=[0.9, 0.9],
         gt_rects=[[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]], gt_classes=[1, 1, 2], thr=[0.0, 0.5], tp=[1, 0], gt=[2, 0], iou=[0.0, -1.0]),
    # disjoint rects at threshold 0: a true positive, as on the host
    dict(name="disjoint_at_threshold_0", rects=[[0, 0, 1, 1]], classes=[1], conf=[0.1], gt_rects=[[5, 5, 6, 6]], gt_classes=[1],
         thr=[0.0], tp=[1], gt=[1], iou=[0.0]),
    dict(name="no_ground_truth", rects=[A, B2], classes=[1, 2], conf=[0.9, 0.8], gt_rects=[], gt_classes=[], thr=[0.5], tp=[0, 0],
         gt=[0, 0], iou=[-1.0, -1.0]),
    dict(name="no_winners", rects=[], classes=[], conf=[], gt_rects=[A], gt_classes=[1], thr=[0.5], tp=[], gt=[], iou=[]),
    dict(name="class_without_ground_truth", rects=[A, A], classes=[3, 1], conf=[0.9, 0.8], gt_rects=[A], gt_classes=[1], thr=[0.5],
         tp=[0, 1], gt=[0, 1], iou=[-1.0, 1.0]),
    dict(name="box_nobody_detects", rects=[A], classes=[1], conf=[0.9], gt_rects=[[100, 100, 120, 120], A], gt_classes=[1, 1],
         thr=[0.5], tp=[1], gt=[2], iou=[1.0]),
    # a ground-truth class < 1 is no class: never matched, also by a detection that carries it
    dict(name="class_below_one", rects=[A, A], classes=[0, -1], conf=[0.9, 0.8], gt_rects=[A, A], gt_classes=[0, -1], thr=[0.5],
         tp=[0, 0], gt=[0, 0], iou=[-1.0, -1.0]),
]

CONF_LEVELS = np.array([0.05, 0.1, 0.25, 0.25, 0.5, 0.5, 0.5, 0.75, 0.9], np.float32)     # heavy ties


def frame(seed, n, G, ncls=4, size=400.0, ties=True):
    """A seeded frame: G ground-truth boxes, n detections -- most of them a box of the frame moved and resized by a few per cent
    to a few tens of per cent (so that the overlaps spread over 0.3 ... 1 and several detections want one box), some of the wrong
    class, the rest anywhere.  Confidences from CONF_LEVELS (ties=True) or uniform."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, size, G); y = rng.uniform(0, size, G)
    gt_rects = np.stack([x, y, x + rng.uniform(10, 80, G), y + rng.uniform(10, 80, G)], 1).reshape(-1, 4)
    gt_classes = rng.randint(1, ncls + 1, G).astype(np.int32)
    rects = np.zeros((n, 4)); classes = np.zeros(n, np.int32)
    for k in range(n):
        kind = rng.rand()
        if G and kind < 0.8:
            g = rng.randint(G)
            w, h = gt_rects[g, 2] - gt_rects[g, 0], gt_rects[g, 3] - gt_rects[g, 1]
            j = rng.choice([0.0, 0.03, 0.1, 0.25]) * rng.uniform(-1, 1, 4)
            rects[k] = gt_rects[g] + j * [w, h, w, h]
            classes[k] = gt_classes[g] if kind < 0.7 else rng.randint(1, ncls + 1)
        else:
            x0, y0 = rng.uniform(0, size, 2)
            rects[k] = [x0, y0, x0 + rng.uniform(10, 80), y0 + rng.uniform(10, 80)]
            classes[k] = rng.randint(1, ncls + 2)          # (ncls + 1: a class without ground truth)
    conf = CONF_LEVELS[rng.randint(len(CONF_LEVELS), size=n)] if ties else rng.uniform(0.01, 1, n).astype(np.float32)
    return dict(rects=rects, classes=classes, conf=conf.astype(np.float32), gt_rects=gt_rects, gt_classes=gt_classes)


IOU_RANGE = [round(0.5 + 0.05 * i, 2) for i in range(10)]
