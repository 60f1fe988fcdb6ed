"""Detections matched to ground truth on the device (Detector.match_batch, frcnn_eval_match_batch) measured, in the style of
tools/bench_class_boxes.py: everything is warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and
the spread (median, min, max) is reported.

  1. the kernels (default): frcnn_eval_match_batch (two launches) at B = 8, host launch included, with 490, 600 and 2 348 winners a
     frame (the README's counts: the defaults, "all" at 0.2, "all" at 0.05), 5 and 50 ground-truth boxes a frame, T = 1 and 10
     thresholds -- and beside it frcnn_detect_gather_batch on the same rows, whose tables the match reads.
  2. --detect: at 800x450, B = 8 (the model of tools/bench_detect_batch.py), Detector.match_batch against Detector.detect_batch per
     frame under the same three settings, and the bytes of read-back 2 of each (counted where the Detector reads them back).
  3. --evaluate: evaluate_detections over the same frames, match = "host" against "device", one threshold and the ten of
     0.5 ... 0.95: wall time per frame and, of it, the time inside the host's matching (mean_average_precision, or
     average_precision_from_matches).  --tree DIR imports the package from another checkout (the parent commit, which has the host
     path only: then only that is measured).
The untouched paths against the parent commit are bench.py's and tools/bench_detect_batch.py's own measurement on the two trees
in alternation; this tool does not run it.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="calls per measurement of a kernel")
ap.add_argument("--frames", type=int, default=64, help="frames per measurement of --detect and --evaluate")
ap.add_argument("--detect", action="store_true")
ap.add_argument("--evaluate", action="store_true")
ap.add_argument("--tree", default=None, help="root of the checkout to import the package from (default: this one)")
args = ap.parse_args()

ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import frcnn_amd as F  # noqa: E402

IOU_RANGE = [round(0.5 + 0.05 * i, 2) for i in range(10)]
SETTINGS = [("defaults", None), ("all@0.2", dict(classes="all", min_confidence=0.2)), ("all@0.05", dict(classes="all", min_confidence=0.05))]


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 3), min=round(v[0], 3), max=round(v[-1], 3))


def alternate(configs, per, warm=5):
    for _, fn in configs:
        fn(warm)
    torch.cuda.synchronize()
    t = dict((name, []) for name, _ in configs)
    for r in range(args.rounds):
        for name, fn in (configs if r % 2 == 0 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(per)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / per)
    return t


def kernels():
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    B, ncls = 8, 16
    dev = F.DeviceTensor.from_numpy
    configs, keep = [], []
    for W in (490, 600, 2348):
        # the gather's inputs: W survivors a frame that all win, in order; their boxes lie around 50 centres a frame
        cx, cy = rng.uniform(50, 750, (B, 50)), rng.uniform(50, 400, (B, 50))
        g = rng.randint(50, size=(B, W))
        x0 = np.take_along_axis(cx, g, 1) + rng.uniform(-8, 8, (B, W)); y0 = np.take_along_axis(cy, g, 1) + rng.uniform(-8, 8, (B, W))
        r2 = np.stack([x0, y0, x0 + rng.uniform(30, 60, (B, W)), y0 + rng.uniform(30, 60, (B, W))], 2)
        bb = np.concatenate([r2.astype(np.float32), np.log(rng.uniform(0.05, 1, (B, W, 1))).astype(np.float32)], 2)
        kc = (g % ncls + 1).astype(np.int32)
        ids = np.tile(np.arange(1, W + 1, dtype=np.int64), (B, 1))
        d = dict(wpick=dev(ids), counts=dev(np.full((4, B), W, np.int32)), keep_row=dev((ids - 1).astype(np.int32)), kc=dev(kc), bb=dev(bb),
                 r2=dev(r2), pick=dev(ids), mp=dev(rng.uniform(-0.05, 0, (B, W)).astype(np.float32)), rect=dev(r2),
                 midx=dev(rng.randint(0, 9, (B, W, 4)).astype(np.int32)), rec=F.DeviceTensor.zeros((B, W + 1, 16), np.float64),
                 match=F.DeviceTensor.zeros((B, W + 2, 4), np.int32))
        keep.append(d)

        def gather(n, d=d, W=W):
            for _ in range(n):
                F._lib.call("frcnn_detect_gather_batch", F.ptr(d["wpick"]), F.ptr(d["counts"]), B, W, F.ptr(d["keep_row"]), F.ptr(d["kc"]),
                            F.ptr(d["bb"]), F.ptr(d["r2"]), F.ptr(d["pick"]), W, F.ptr(d["mp"]), F.ptr(d["rect"]), F.ptr(d["midx"]),
                            F.ptr(d["rec"]), s)
        gather(1)
        configs.append(("winners%d/gather" % W, gather))
        for G in (5, 50):
            gt_rect = np.stack([cx[:, :G] - 4, cy[:, :G] - 4, cx[:, :G] + 41, cy[:, :G] + 41], 2).reshape(-1, 4)
            gt_class = np.tile(np.arange(G) % ncls + 1, B).astype(np.int32)
            d_gr, d_gc = dev(gt_rect), dev(gt_class)
            row0 = (C.c_longlong * (B + 1))(*[G * b for b in range(B + 1)])
            keep.append((d_gr, d_gc))
            for T in (1, 10):
                thr = (C.c_double * T)(*IOU_RANGE[:T])

                def match(n, d=d, W=W, d_gr=d_gr, d_gc=d_gc, row0=row0, thr=thr, T=T):
                    for _ in range(n):
                        F._lib.call("frcnn_eval_match_batch", F.ptr(d["rec"]), B, W, None, 0, None, F.ptr(d_gr), F.ptr(d_gc), row0, thr, T,
                                    F.ptr(d["match"]), None, s)
                configs.append(("winners%d/boxes%d/T%d/match" % (W, G, T), match))
    t = alternate(configs, args.calls)
    res = dict(metric="us per call, queued back to back, host launch included (B = 8 frames; winners a frame / ground-truth boxes a frame / "
                      "thresholds; match = frcnn_eval_match_batch, two launches; gather = frcnn_detect_gather_batch on the same rows)",
               calls=args.calls, rounds=args.rounds)
    for name, _ in configs:
        res[name] = dict(us=spread([v * 1e6 for v in t[name]]))
    return res


def ground_truth(winners, cap=50):
    """a frame's boxes from its detections, as the tests make them: copied, moved by 15 % of the width, of the next class, left out"""
    out = []
    for k, x in enumerate(list(winners)[:cap]):
        r, c = x["r2"], int(x["class"])
        if k % 4 == 0:
            out.append((c, F.Rect(r.minX, r.minY, r.maxX, r.maxY)))
        elif k % 4 == 1:
            dx = max(2.0, 0.15 * (r.maxX - r.minX))
            out.append((c, F.Rect(r.minX + dx, r.minY, r.maxX + dx, r.maxY)))
        elif k % 4 == 2:
            out.append((c % 16 + 1, F.Rect(r.minX, r.minY, r.maxX, r.maxY)))
    return out


def detectors():
    from detect_bench_model import amplified_vgg_small
    imgs = [F.to_device(F.synthetic_image(450, 800, i)) for i in range(4)]
    cfg, model, weights, gradient = amplified_vgg_small(F, 30.0)
    out = []
    for name, sc in SETTINGS:
        d = F.Detector(model, static_weights=True, scoring=sc) if sc else F.Detector(model, static_weights=True)
        d.BATCH = 8
        gts = [ground_truth(w) for w in d.detect_batch(imgs)]
        out.append((name, d, gts))
    return imgs, out, (model, weights, gradient)


def detect():
    imgs, dets, alive = detectors()
    read = {}

    def counted(d, key):       # the bytes of a chunk's read-backs, where the Detector reads them back
        inner = d._read

        def _read(dev_ptr, nbytes, dtype):
            read.setdefault(key, []).append(int(nbytes))
            return inner(dev_ptr, nbytes, dtype)
        d._read = _read
        return inner
    configs = []
    for name, d, gts in dets:
        def run_detect(n, d=d):
            for lo in range(0, n, 8):
                d.detect_batch([imgs[(lo + i) % 4] for i in range(min(8, n - lo))])

        def run_match(n, d=d, gts=gts):
            for lo in range(0, n, 8):
                k = [(lo + i) % 4 for i in range(min(8, n - lo))]
                d.match_batch([imgs[i] for i in k], [gts[i] for i in k], IOU_RANGE)
        configs += [(name + "/detect_batch", run_detect), (name + "/match_batch", run_match)]
    t = alternate(configs, args.frames, warm=32)
    res = dict(metric="ms per frame (vgg_small 800x450 inference, B = 8; match_batch at the ten thresholds 0.5 ... 0.95); readback2: the "
                      "bytes of a chunk's second read-back", frames=args.frames, rounds=args.rounds)
    for (name, d, gts), (cname, fn) in zip([x for x in dets for _ in (0, 1)], configs):
        inner = counted(d, cname)
        fn(8)
        d._read = inner
        res[cname] = dict(ms=spread([v * 1e3 for v in t[cname]]), readback2=read[cname][-1], boxes=[len(g) for g in gts],
                          detections=[len(w) for w in d.detect_batch(imgs)])
    return res


class Validation(object):
    def __init__(self, imgs, gts):
        self.items = [dict(img=f, rois=[F.Roi(r, c) for c, r in g]) for f, g in zip(imgs, gts)]
        self.at = 0

    def nextValidation(self, n):
        out = [self.items[(self.at + i) % len(self.items)] for i in range(n)]
        self.at += n
        return out


def evaluate():
    imgs, dets, alive = detectors()
    have = hasattr(F.Detector, "match_batch")
    spent = [0.0]

    def timed(fn):
        def inner(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                spent[0] += time.perf_counter() - t0
        return inner
    E = F.evaluation
    E.mean_average_precision = timed(E.mean_average_precision)       # (mean_average_precision_range calls it per threshold)
    if have:
        E.average_precision_from_matches = timed(E.average_precision_from_matches)
    configs, matching = [], {}
    for name, d, gts in dets:
        for tname, thr in (("T1", 0.5), ("T10", tuple(IOU_RANGE))):
            for how in (("host", "device") if have else ("host",)):
                key = "%s/%s/%s" % (name, tname, how)

                def run(n, d=d, gts=gts, thr=thr, how=how, key=key):
                    spent[0] = 0.0
                    kw = dict(match=how) if have else {}
                    E.evaluate_detections(d, Validation(imgs, gts), n, iou_threshold=thr, batch=8, **kw)
                    matching.setdefault(key, []).append(spent[0] / n)
                configs.append((key, run))
    t = alternate(configs, args.frames, warm=8)
    res = dict(metric="ms per frame of evaluate_detections (vgg_small 800x450, batch = 8; T1: IoU 0.5, T10: 0.5 ... 0.95); matching: the part "
                      "inside mean_average_precision (host) or average_precision_from_matches (device); the rest is the detector and the "
                      "lists' bookkeeping", frames=args.frames, rounds=args.rounds, tree=ROOT if args.tree else "this")
    for key, _ in configs:
        total = [v * 1e3 for v in t[key]]
        part = [v * 1e3 for v in matching[key][-len(total):]]
        res[key] = dict(ms=spread(total), matching_ms=spread(part), rest_ms=spread([a - b for a, b in zip(total, part)]))
    return res


print(json.dumps(evaluate() if args.evaluate else detect() if args.detect else kernels()))
