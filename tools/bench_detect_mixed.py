"""Detector.detect_batch(mixed_sizes=True) against the detect() loop on frames of DIFFERENT sizes: ms per frame (vgg_small).

The frames: 8 synthetic images at the sizes utilities.lua's find_target_size yields under the duplo settings (smaller side 450,
at most 1000) for common aspect ratios, landscape and portrait -- 4:3, 3:2, 16:9, 5:4, 1:1, 3:4, 2:3, 9:16 -- so every frame has
a size of its own, as almost every file of a real data set has.  Weights amplified and option static_weights on as in
tools/bench_detect_batch.py.  Three configurations, warmed up and then ALTERNATED in this one process, `--rounds` times; a
measurement is `--reps` passes over the 8 frames ending in a device synchronise:

  loop      (a) detect(frame) for every frame
  mixed8    (b) detect_batch(frames, mixed_sizes=True) with BATCH = 8: one chunk, one ragged scan, two host waits
  one_size  (c) detect(frame) on 8 frames of ONE size with the same total pixel count: what (a) would cost if a change of the
            frame size were free (the native model re-plans its shapes on every change)

  python tools/bench_detect_mixed.py            the three configurations; median and min-max of the rounds, ms per frame
  python tools/bench_detect_mixed.py --scan     the scan alone, device time per call (events): frcnn_rpn_scan_ragged beside
                                                frcnn_rpn_scan_batch on 8 frames of 450x800, and the ragged scan on the mixed set

The process ends itself after --time-limit seconds.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import frcnn_amd as F  # noqa: E402
from detect_bench_model import amplified_vgg_small  # noqa: E402
from frcnn_amd.BatchIterator import find_target_size  # noqa: E402
from frcnn_amd.Detector import _chunk_slots  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=6, help="passes over the 8 frames per measurement")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--gain", type=float, default=30.0)
ap.add_argument("--scan", action="store_true", help="time the scan entry points alone")
ap.add_argument("--calls", type=int, default=50, help="with --scan: calls per measurement")
ap.add_argument("--time-limit", type=int, default=600)
args = ap.parse_args()
signal.alarm(args.time_limit)

ORIGINALS = [(640, 480), (720, 480), (1280, 720), (1280, 1024), (500, 500), (480, 640), (480, 720), (720, 1280)]     # (w, h)
SIZES = [find_target_size(w, h, 450, 1000) for w, h in ORIGINALS]                                                    # (w, h)
assert len(set(SIZES)) == 8
pixels = sum(w * h for w, h in SIZES) // 8
ONE_W = int(round((pixels * 4.0 / 3.0) ** 0.5))
ONE_H = int(round(pixels / float(ONE_W)))

cfg, model, weights, gradient = amplified_vgg_small(F, args.gain)
det = F.Detector(model, static_weights=True)
res = dict(sizes=["%dx%d" % s for s in SIZES], one_size="%dx%d" % (ONE_W, ONE_H),
           library=os.path.basename(os.environ.get("FRCNN_LIB_PATH") or "libfrcnn_hip.so"))


def spread(values, digits=4):
    v = sorted(values)
    return dict(median=round(float(np.median(v)), digits), min=round(v[0], digits), max=round(v[-1], digits))


def scan_bench():
    """device time per call of the scan entry points on random head maps (about a third of the anchors pass)"""
    L = F._lib.load()
    rng = np.random.RandomState(0)

    def problem(sizes):     # sizes: (w, h) per frame -> the arguments of a ragged call and of a batch call (one size only)
        lay = [det._layout_of(h, w_) for w_, h in sizes]     # the Detector's own slot offsets, strides and anchor counts
        B = len(sizes)
        hw, hoffs = [t.hw for t in lay], [t.hoff for t in lay]
        slot, _, cap = _chunk_slots(lay)
        heads = np.zeros((B, slot), np.float32)
        for b, t in enumerate(hw):
            for i, (hh, ww) in enumerate(t):
                m = (rng.randn(18, hh, ww) * 0.02).astype(np.float32)
                for a in range(3):
                    m[a * 6] = rng.randn(hh, ww) * 3.0 + 2.0
                    m[a * 6 + 1] = rng.randn(hh, ww) * 3.0
                heads[b, hoffs[b][i]:hoffs[b][i] + m.size] = m.ravel()
        anchors = [t.anchors for t in lay]
        out = dict(heads=F.DeviceTensor.from_numpy(heads), B=B, slot=slot, cap=cap, anchors=anchors,
                   Hs=(C.c_int * (4 * B))(*[t[i][0] for t in hw for i in range(4)]),
                   Ws=(C.c_int * (4 * B))(*[t[i][1] for t in hw for i in range(4)]),
                   map_off=(C.c_longlong * (4 * B))(*[b * slot + hoffs[b][i] for b in range(B) for i in range(4)]),
                   img=(C.c_double * (2 * B))(*[float(v) for s in sizes for v in s]), hoff=hoffs[0], size=sizes[0],
                   p=F.DeviceTensor.empty((B, cap)), idx=F.DeviceTensor.empty((B, cap, 4), np.int32),
                   rect=F.DeviceTensor.empty((B, cap, 4), np.float64), box=F.DeviceTensor.empty((B, cap, 4)),
                   cnt=F.DeviceTensor.empty((B,), np.int32))
        out["wsb"] = L.frcnn_rpn_scan_ragged_workspace_bytes(out["Hs"], out["Ws"], B)
        out["ws"] = F.DeviceTensor.empty((out["wsb"],), np.uint8)
        return out

    def ragged(q):
        F._lib.call("frcnn_rpn_scan_ragged", F.ptr(q["heads"]), q["map_off"], q["Hs"], q["Ws"], q["img"], q["B"], F.ptr(det._aw),
                    F.ptr(det._ah), 0.95, q["cap"], F.ptr(q["p"]), F.ptr(q["idx"]), F.ptr(q["rect"]), F.ptr(q["box"]), F.ptr(q["cnt"]),
                    F.ptr(q["ws"]), q["wsb"], F.stream_ptr())

    def batch(q):
        maps = (C.c_void_p * 4)(*[q["heads"].ptr + 4 * q["hoff"][i] for i in range(4)])
        F._lib.call("frcnn_rpn_scan_batch", maps, q["Hs"], q["Ws"], q["B"], q["slot"], F.ptr(det._aw), F.ptr(det._ah),
                    float(q["size"][0]), float(q["size"][1]), 0.95, q["cap"], F.ptr(q["p"]), F.ptr(q["idx"]), F.ptr(q["rect"]),
                    F.ptr(q["box"]), F.ptr(q["cnt"]), F.ptr(q["ws"]), q["wsb"], F.stream_ptr())
    full, mixed = problem([(800, 450)] * 8), problem(SIZES)
    configs = [("batch_8x450x800", batch, full), ("ragged_8x450x800", ragged, full), ("ragged_mixed", ragged, mixed)]
    us = dict((name, []) for name, _, _ in configs)
    for name, fn, q in configs:
        fn(q)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, fn, q in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn(q)
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) / args.calls * 1e3)
    res.update(metric="us per scan call (device time between events, %d calls)" % args.calls, rounds=args.rounds,
               anchors_full=full["anchors"][0], anchors_mixed=mixed["anchors"], matches_mixed=mixed["cnt"].numpy().tolist())
    for name, _, _ in configs:
        res[name] = spread(us[name], 2)


if args.scan:
    scan_bench()
    print(json.dumps(res))
    sys.exit(0)

mixed = [F.to_device(F.synthetic_image(h, w_, i)) for i, (w_, h) in enumerate(SIZES)]
same = [F.to_device(F.synthetic_image(ONE_H, ONE_W, i)) for i in range(8)]


def run_loop(frames):
    for _ in range(args.reps):
        for f in frames:
            det.detect(f)


def run_mixed():
    det.BATCH = 8
    for _ in range(args.reps):
        det.detect_batch(mixed, mixed_sizes=True)


configs = [("loop", lambda: run_loop(mixed)), ("mixed8", run_mixed), ("one_size", lambda: run_loop(same))]
for name, fn in configs:      # warm-up: every shape, every buffer
    fn()
torch.cuda.synchronize()
ms = dict((name, []) for name, _ in configs)
for r in range(args.rounds):
    for name, fn in configs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) / (8 * args.reps) * 1e3)
res.update(metric="ms per frame (vgg_small inference, 8 frames of 8 sizes)", frames=8 * args.reps, rounds=args.rounds)
got = det.detect_batch(mixed, mixed_sizes=True)
res.update(matches=[int(r["n"]) for r in det.last_batch], winners=[len(g) for g in got])
for name, _ in configs:
    res[name] = spread(ms[name])
# pairwise, round by round: (b) against (a), and what the size changes cost the loop, (a) against (c)
res["mixed8_over_loop"] = spread([b / a for a, b in zip(ms["loop"], ms["mixed8"])])
res["loop_minus_one_size_ms"] = spread([a - c for a, c in zip(ms["loop"], ms["one_size"])])
print(json.dumps(res))
