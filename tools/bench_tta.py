"""cfg.tta (test-time augmentation: mirrored and rescaled views, merged behind the class test) measured, in the style of
tools/bench_box_vote.py: everything is warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and the
spread (median, min, max) is reported, not the best.

  1. the kernel alone (default): frcnn_detect_merge_views as the Detector calls it, F frames of V views at the row counts of the
     800x450 workload -- 300 rows a view of which 250 survive (the candidates of a frame under the reference's thresholds), a
     match stride of 26 544 (every anchor of the four maps) -- for (F, V) = (1, 2), (4, 2), (2, 4), (1, 8), and --big adds 1 404
     rows a view; beside frcnn_detect_gather_batch on the merged rows in the same run (a launch of the same kind that follows).
     Reported per configuration: us per call.
  2. --detector: detect_batch per FRAME on synthetic 3x450x800 frames (vgg_small, weights amplified as in
     tools/bench_detect_batch.py), as alternating rounds:
       absent / identity   Detector(model) against Detector(model, tta = {}): the key absent against a table that is off.  With
                           the key absent this Detector queues what the parent commit's queues; the parent's own figure comes
                           from tools/bench_detect_batch.py run from both trees in alternation in the same session, and the
                           spread of the alternating pairs printed here is what any difference has to be read against.
       hflip / two_frames  detect_batch of 4 frames under { hflip = true } (one chunk: 8 segments) against a plain detect_batch
                           over the 8 frames [x, mirror(x)] (one chunk of 8): the same proposal-net and classification-net
                           work, so the difference is the mirror launches, the merge and a per-class pass over segments
                           twice as long.  Both per ORIGINAL frame.

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
from detect_bench_model import amplified_vgg_small  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="kernel calls per measurement")
ap.add_argument("--frames", type=int, default=104, help="frames per measurement of --detector (a multiple of 8)")
ap.add_argument("--gain", type=float, default=30.0)
ap.add_argument("--detector", action="store_true")
ap.add_argument("--big", action="store_true")
args = ap.parse_args()


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 3), min=round(v[0], 3), max=round(v[-1], 3))


def kernels():
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    cap = 26544
    configs = []
    for rows in (300,) + ((1404,) if args.big else ()):
        for nF, nV in ((1, 2), (4, 2), (2, 4), (1, 8)):
            S = nF * nV
            K = rows * 5 // 6
            dev = F.DeviceTensor.from_numpy
            bb = dev(rng.standard_normal((S * rows, 5)).astype(np.float32)); kc = dev(rng.randint(1, 21, S * rows).astype(np.int32))
            keep = dev(rng.randint(0, rows, S * rows).astype(np.int32)); r2 = dev(rng.uniform(0, 800, (S * rows, 4)))
            counts = np.zeros((4, S), np.int32)
            counts[0], counts[1], counts[2] = 2000, rows, K
            cnt = dev(counts)
            pick = dev(rng.randint(1, 2001, (S, cap)).astype(np.int64))
            o = [F.DeviceTensor.empty((S * rows, 5)), F.DeviceTensor.empty((S * rows,), np.int32),
                 F.DeviceTensor.empty((S * rows,), np.int32), F.DeviceTensor.empty((S * rows, 4), np.float64),
                 F.DeviceTensor.empty((S, cap), np.int64),
                 dev(np.repeat(np.array([0, 0, 0, nV * K], np.int32), nF).reshape(4, nF))]    # (row 3: every survivor wins)
            flip = (C.c_int * S)(*[i % 2 for i in range(S)])
            wv = (C.c_double * S)(*[800.0 if i % nV < 2 else 1000.0 for i in range(S)])
            ax = (C.c_double * S)(*[1.0 if i % nV < 2 else 0.8 for i in range(S)])
            R = (C.c_int * S)(*([rows] * S))
            mp = F.DeviceTensor.zeros((S, cap)); mr = F.DeviceTensor.zeros((S, cap, 4), np.float64)
            mi = F.DeviceTensor.zeros((S, cap, 4), np.int32)
            wpick = dev(np.tile(np.arange(1, nV * rows + 1, dtype=np.int64), nF))
            rec = F.DeviceTensor.empty((nF, nV * rows + 1, 16), np.float64)
            keepalive = (bb, kc, keep, r2, cnt, pick, o, mp, mr, mi, wpick, rec)

            def merge(n, a=keepalive, nF=nF, nV=nV, rows=rows, flip=flip, wv=wv, ax=ax, R=R):
                for _ in range(n):
                    F._lib.call("frcnn_detect_merge_views", F.ptr(a[0]), F.ptr(a[1]), F.ptr(a[2]), F.ptr(a[3]), rows, F.ptr(a[4]),
                                F.ptr(a[5]), cap, nF, nV, flip, wv, ax, ax, R, *([F.ptr(t) for t in a[6]] + [s]))

            def gather(n, a=keepalive, nF=nF, nV=nV, rows=rows):
                o = a[6]
                for _ in range(n):
                    F._lib.call("frcnn_detect_gather_batch", F.ptr(a[10]), F.ptr(o[5]), nF, nV * rows, F.ptr(o[2]), F.ptr(o[1]),
                                F.ptr(o[0]), F.ptr(o[3]), F.ptr(o[4]), nV * cap, F.ptr(a[7]), F.ptr(a[8]), F.ptr(a[9]),
                                F.ptr(a[11]), s)
            tag = "F%d_V%d_rows%d" % (nF, nV, rows)
            configs.append((tag + "/merge_views", merge))
            configs.append((tag + "/gather", gather))
    for name, fn in configs:
        fn(5)
    torch.cuda.synchronize()
    us = dict((name, []) for name, _ in configs)
    for r in range(args.rounds):
        for name, fn in (configs if r % 2 == 0 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.calls)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    res = dict(metric="us per call (F frames of V views, rows a view; host launch included)", calls=args.calls, rounds=args.rounds)
    for name, _ in configs:
        res[name] = dict(us=spread(us[name]))
    return res


def detector():
    cfg, model, weights, gradient = amplified_vgg_small(F, args.gain)     # (`weights` keeps the amplified values alive)
    host = [F.synthetic_image(450, 800, i) for i in range(4)]
    imgs = [F.to_device(x) for x in host]
    both = [F.to_device(v) for x in host for v in (x, np.ascontiguousarray(x[:, :, ::-1]))]
    dets = dict(absent=F.Detector(model, static_weights=True), identity=F.Detector(model, static_weights=True, tta={}),
                hflip=F.Detector(model, static_weights=True, tta=dict(hflip=True)),
                two_frames=F.Detector(model, static_weights=True))

    def run(name, n):        # n ORIGINAL frames
        d = dets[name]
        if name == "two_frames":
            for lo in range(0, n, 4):
                d.detect_batch(both)
        elif name == "hflip":         # (one chunk a call, like two_frames: neither detaches records between chunks)
            for lo in range(0, n, 4):
                d.detect_batch(imgs)
        else:
            for lo in range(0, n, 8):
                d.detect_batch([imgs[(lo + i) % 4] for i in range(8)])
    names = ["absent", "identity", "hflip", "two_frames"]
    for name in names:
        run(name, 16)
    torch.cuda.synchronize()
    ms = dict((name, []) for name in names)
    for r in range(args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.frames)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = dict(metric="ms per original frame, detect_batch (vgg_small 800x450 inference)", frames=args.frames, rounds=args.rounds,
               gain=args.gain)
    for name in names:
        res[name] = dict(ms=spread(ms[name]))
    win = dets["hflip"].detect(imgs[0])
    rec = dets["hflip"]._last
    res["hflip"].update(candidates=np.diff(rec["roff"]).tolist(), survivors=int(rec["kept"]), winners=len(win),
                        winners_of_the_mirror=sum(x["view"] == 1 for x in win))
    # the differences of the alternating pairs, per round: what "costs nothing" / "one small launch" is read against
    res["identity"]["minus_absent_ms"] = spread([a - b for a, b in zip(ms["identity"], ms["absent"])])
    res["hflip"]["minus_two_frames_ms"] = spread([a - b for a, b in zip(ms["hflip"], ms["two_frames"])])
    return res


print(json.dumps(detector() if args.detector else kernels()))
