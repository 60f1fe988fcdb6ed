"""cfg.scoring (the class test of a chunk as ONE frcnn_detect_classes_batch launch; a row per class under classes = "all")
measured, in the style of tools/bench_box_vote.py: everything is warmed up, the configurations are ALTERNATED in this one process
`--rounds` times, and the spread (median, min, max) is reported, not the best.

  1. the kernel alone (default): frcnn_detect_classes_batch at B = 8 for R candidates a frame and ncls classes -- (300, 17) and
     (300, 201), (2000, 17) -- in mode 0 at 0.2 and in mode 1 at 0.2 and 0.05, beside the 2 B launches it replaces
     (frcnn_cnet_decode + frcnn_detect_post per frame) on the same rows in the same run.  Log-probabilities: an fp32
     log-softmax of normal logits, scale 3.  Reported per configuration: us per call and the rows a frame emits.
  2. --detector: detect_batch (B = 8) per frame on synthetic 3x450x800 frames (vgg_small, weights amplified as in
     tools/bench_proposals.py; --cls-gain scales the class head: the lower, the more classes share a candidate's mass): the key
     ABSENT, the EMPTY table ("top" at 0.2 from one launch: the launch saving, whatever its sign), "all" at 0.2 and "all" at
     0.05, alternated.  Per case: ms per frame, survivors and winners per frame, and the bytes of read-back 2 (the winner table
     is sized for Rmax * m rows a frame: it grows with m whether or not the rows are used).  With the key absent this Detector
     queues what the parent commit's queues; the parent's own figure comes from tools/bench_detect_batch.py run from both trees
     in alternation in the same session, and the spread of the alternating pairs printed here is what any difference has to be
     read against.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import frcnn_amd as F  # noqa: E402
from frcnn_amd.Detector import scoring_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="kernel calls per measurement")
ap.add_argument("--frames", type=int, default=104, help="frames per measurement of --detector (a multiple of 8)")
ap.add_argument("--gain", type=float, default=30.0)
ap.add_argument("--cls-gain", type=float, default=200.0)
ap.add_argument("--detector", action="store_true")
args = ap.parse_args()
B = 8


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 3), min=round(v[0], 3), max=round(v[-1], 3))


def kernels():
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    configs, info = [], {}
    for R, ncls in ((300, 17), (300, 201), (2000, 17)):
        z = (rng.standard_normal((B * R, ncls)) * 3.0).astype(np.float32)
        z -= z.max(1, keepdims=True)
        lp = F.DeviceTensor.from_numpy((z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32))
        bbox = F.DeviceTensor.from_numpy((rng.standard_normal((B * R, 4)) * 0.3).astype(np.float32))
        x0, y0 = rng.uniform(0, 700, B * R), rng.uniform(0, 380, B * R)
        rect = F.DeviceTensor.from_numpy(np.stack([x0, y0, x0 + rng.uniform(20, 80, B * R), y0 + rng.uniform(20, 80, B * R)], 1))
        pick = F.DeviceTensor.from_numpy(np.tile(np.arange(1, R + 1, dtype=np.int64), B))
        Rs, row0 = (C.c_int * B)(*([R] * B)), (C.c_longlong * B)(*[b * R for b in range(B)])
        dcls, dconf = F.DeviceTensor.empty((R,), np.int32), F.DeviceTensor.empty((R,), np.float32)
        for name, mode, c in (("top_0.2", 0, 0.2), ("all_0.2", 1, 0.2), ("all_0.05", 1, 0.05), ("decode+post_0.2", None, 0.2)):
            rows = R * (scoring_rows("all", c, ncls) if mode == 1 else 1)
            o = (F.DeviceTensor.empty((B, rows, 5), np.float32), F.DeviceTensor.empty((B, rows), np.int32),
                 F.DeviceTensor.empty((B, rows), np.int32), F.DeviceTensor.empty((B, rows, 4), np.float64),
                 F.DeviceTensor.empty((B,), np.int32))

            def one(n, o=o, mode=mode, c=c, rows=rows, a=(lp, bbox, rect, pick, Rs, row0, dcls, dconf), R=R, ncls=ncls):
                for _ in range(n):
                    F._lib.call("frcnn_detect_classes_batch", F.ptr(a[0]), F.ptr(a[1]), a[4], a[5], B, F.ptr(a[2]), F.ptr(a[3]), R, ncls,
                                ncls, c, mode, F.ptr(o[0]), F.ptr(o[1]), F.ptr(o[2]), F.ptr(o[3]), rows, F.ptr(o[4]), None, s)

            def pair(n, o=o, c=c, a=(lp, bbox, rect, pick, Rs, row0, dcls, dconf), R=R, ncls=ncls):
                for _ in range(n):
                    for b in range(B):
                        F._lib.call("frcnn_cnet_decode", C.c_void_p(a[0].ptr + 4 * ncls * b * R), R, ncls, F.ptr(a[6]), F.ptr(a[7]), s)
                        F._lib.call("frcnn_detect_post", F.ptr(a[6]), F.ptr(a[7]), C.c_void_p(a[1].ptr + 16 * b * R),
                                    C.c_void_p(a[2].ptr + 32 * b * R), C.c_void_p(a[3].ptr + 8 * b * R), R, ncls, c,
                                    F.ptr(o[0].segment(b)), F.ptr(o[1].segment(b)), F.ptr(o[2].segment(b)), F.ptr(o[3].segment(b)),
                                    C.c_void_p(o[4].ptr + 4 * b), s)
            configs.append(("R%d_ncls%d/%s" % (R, ncls, name), one if mode is not None else pair, o[4]))
    for name, fn, k in configs:
        fn(5)
        torch.cuda.synchronize()
        info[name] = dict(rows_per_frame=round(float(k.numpy().mean()), 1))
    us = dict((name, []) for name, _, _ in configs)
    for r in range(args.rounds):
        for name, fn, _ in (configs if r % 2 == 0 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.calls)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    res = dict(metric="us per call, B = 8 (R candidates a frame, ncls classes)", calls=args.calls, rounds=args.rounds)
    for name, _, _ in configs:
        res[name] = dict(us=spread(us[name]), **info[name])
    return res


def detector():
    cfg = dict(F.duplo_cfg)
    ncls = cfg["class_count"] + 1
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = weights.cpu().numpy().copy()
    for off, cnt, kind, aux in model["native"].param_table:
        if kind == 0 and aux == 18:
            v = w[off:off + cnt].reshape(18, -1)
            for a in range(3):
                v[a * 6:a * 6 + 2] *= args.gain
        if kind == 3 and cnt == 512 * ncls:
            w[off:off + cnt] *= args.cls_gain
    weights.copy_(torch.from_numpy(w))
    imgs = [F.to_device(F.synthetic_image(450, 800, i)) for i in range(4)]
    tables = [("absent", None), ("empty", {}), ("all_0.2", dict(classes="all", min_confidence=0.2)),
              ("all_0.05", dict(classes="all", min_confidence=0.05))]
    dets = dict((name, F.Detector(model, static_weights=True, scoring=t)) for name, t in tables)

    def run(d, n):
        for lo in range(0, n, B):
            d.detect_batch([imgs[(lo + i) % 4] for i in range(B)])
    refused = {}
    for name, _ in list(tables):
        try:
            run(dets[name], 2 * B)
        except F.FrcnnError as e:      # (Rmax * m over a limit of the per-class pass: reported, not measured)
            refused[name] = str(e)
            tables.remove((name, _))
    torch.cuda.synchronize()
    ms = dict((name, []) for name, _ in tables)
    for r in range(args.rounds):
        for name, _ in (tables if r % 2 == 0 else tables[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(dets[name], args.frames)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = dict(metric="ms per frame, detect_batch B = 8 (vgg_small 800x450 inference)", frames=args.frames, rounds=args.rounds,
               gain=args.gain, cls_gain=args.cls_gain)
    for name, _ in tables:
        d = dets[name]
        win = d.detect_batch([imgs[i % 4] for i in range(B)])
        rec = d.last_batch
        rows = max(len(r["pick"]) for r in rec) * (scoring_rows(d.scoring[0], d.scoring[1], ncls) if d.scoring else 1)
        res[name] = dict(ms=spread(ms[name]), candidates=round(float(np.mean([len(r["pick"]) for r in rec])), 1),
                         survivors=round(float(np.mean([r["kept"] for r in rec])), 1),
                         winners=round(float(np.mean([len(x) for x in win])), 1), readback2_bytes=B * (rows + 1) * 128)
    # the differences of the alternating pairs (per round): what "costs nothing" and "saves launches" are read against
    for name, _ in tables[1:]:
        res[name]["minus_absent_ms"] = spread([a - b for a, b in zip(ms[name], ms["absent"])])
    res.update(dict((name, dict(refused=why)) for name, why in refused.items()))
    return res


print(json.dumps(detector() if args.detector else kernels()))
