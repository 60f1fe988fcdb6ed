"""cfg.nms (Soft-NMS in the per-class pass) measured, in the style of tools/bench_proposals.py: everything is warmed up, the
configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min, max) is reported, not the best.

  1. the kernel alone (default): frcnn_soft_nms_batch (gaussian, log-scores, as the Detector calls it) at B = 8 for K = 64, 300
     and 1404 rows a segment -- one wave in registers / the same / the workgroup with LDS -- and --big adds 4096 (global
     memory), with 1 and with 20 classes, against frcnn_nms_device_batch on the same rows in the same run.  Boxes: clusters of
     about 12 around common centres, as a frame's class-test survivors come.  Reported per configuration: us per call, the picks
     of segment 0, and for the soft kernel ns per pick (the call's time over the picks of its longest segment: the segments run
     side by side, one workgroup each).
  2. --detector: detect_batch (B = 8) per frame on synthetic 3x450x800 frames (vgg_small, weights amplified as in
     tools/bench_proposals.py), "hard" (the setting absent) against "gaussian" and "linear", alternated.  The parent commit's
     figure for the setting off comes from tools/bench_detect_batch.py run from both trees in alternation in the same session:
     with the setting off this Detector queues what the parent's queues.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import frcnn_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="kernel calls per measurement")
ap.add_argument("--frames", type=int, default=104, help="frames per measurement of --detector (a multiple of 8)")
ap.add_argument("--gain", type=float, default=30.0)
ap.add_argument("--detector", action="store_true")
ap.add_argument("--big", action="store_true")
args = ap.parse_args()
L = F._lib.load()


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 3), min=round(v[0], 3), max=round(v[-1], 3))


def kernels():
    B = 8
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    configs, info = [], {}
    for K in (64, 300, 1404) + ((4096,) if args.big else ()):
        for ncls in (1, 20):
            k = max(K // 12, 1)
            g = np.arange(B * K) % k
            x1 = rng.randint(0, 700, k)[g] + rng.randint(-20, 21, B * K); y1 = rng.randint(0, 380, k)[g] + rng.randint(-20, 21, B * K)
            rows = np.stack([x1, y1, x1 + rng.randint(20, 80, B * K), y1 + rng.randint(20, 80, B * K),
                             np.log(rng.rand(B * K) * 0.8 + 0.2)], 1).astype(np.float32)
            d = F.DeviceTensor.from_numpy(rows)
            cls = F.DeviceTensor.from_numpy(rng.randint(1, ncls + 1, B * K).astype(np.int32))
            nd = F.DeviceTensor.from_numpy(np.full(B, K, np.int32))
            pick = F.DeviceTensor.empty((B * K,), np.int64); cnt = F.DeviceTensor.empty((B,), np.int32)
            out = F.DeviceTensor.empty((B * K,), np.float32)
            swsb = L.frcnn_soft_nms_workspace_bytes(B, K); sws = F.DeviceTensor.empty((swsb,), np.uint8)
            hwsb = L.frcnn_nms_batch_workspace_bytes(B, K); hws = F.DeviceTensor.empty((hwsb,), np.uint8)
            keep = (d, cls, nd, pick, cnt, out, sws, hws)

            def soft(n, method, a=keep, K=K, swsb=swsb):
                for _ in range(n):
                    F._lib.call("frcnn_soft_nms_batch", F.ptr(a[0]), B, K, K, F.ptr(a[2]), 5, 5, method, C.c_float(0.1), C.c_float(0.5),
                                C.c_float(math.log(0.001)), 1, F.ptr(a[1]), F.ptr(a[3]), F.ptr(a[4]), F.ptr(a[5]), 1, F.ptr(a[6]), swsb, s)

            def hard(n, a=keep, K=K, hwsb=hwsb):
                for _ in range(n):
                    F._lib.call("frcnn_nms_device_batch", F.ptr(a[0]), B, K, K, F.ptr(a[2]), 5, C.c_float(0.1), 2, 5, F.ptr(a[1]),
                                F.ptr(a[3]), F.ptr(a[4]), F.ptr(a[7]), hwsb, s)
            tag = "K%d_c%d" % (K, ncls)
            for name, fn in (("gaussian", lambda n, f=soft: f(n, 2)), ("linear", lambda n, f=soft: f(n, 1)), ("bitmatrix_hard", hard)):
                configs.append((tag + "/" + name, fn, cnt))
    for name, fn, cnt in configs:
        fn(5)
        torch.cuda.synchronize()
        info[name] = cnt.numpy().tolist()
    us = dict((name, []) for name, _, _ in configs)
    for r in range(args.rounds):
        for name, fn, _ in (configs if r % 2 == 0 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.calls)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    res = dict(metric="us per call, B = 8 segments", calls=args.calls, rounds=args.rounds)
    for name, _, _ in configs:
        res[name] = dict(us=spread(us[name]), picks_segment0=info[name][0], picks_longest=max(info[name]))
        if not name.endswith("bitmatrix_hard"):
            res[name]["ns_per_pick"] = round(float(np.median(us[name])) * 1e3 / max(max(info[name]), 1), 1)
    return res


def detector():
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = weights.cpu().numpy().copy()
    for off, cnt, kind, aux in model["native"].param_table:
        if kind == 0 and aux == 18:
            v = w[off:off + cnt].reshape(18, -1)
            for a in range(3):
                v[a * 6:a * 6 + 2] *= args.gain
        if kind == 3 and cnt == 512 * (cfg["class_count"] + 1):
            w[off:off + cnt] *= 200.0
    weights.copy_(torch.from_numpy(w))
    imgs = [F.to_device(F.synthetic_image(450, 800, i)) for i in range(4)]
    tables = [("hard", None), ("gaussian", dict(method="gaussian")), ("linear", dict(method="linear"))]
    dets = dict((name, F.Detector(model, static_weights=True, nms=t)) for name, t in tables)

    def run(d, n):
        for lo in range(0, n, 8):
            d.detect_batch([imgs[(lo + i) % 4] for i in range(8)])
    for name, _ in tables:
        run(dets[name], 16)
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
               gain=args.gain)
    for name, _ in tables:
        d = dets[name]
        win = d.detect(imgs[0])
        res[name] = dict(ms=spread(ms[name]), candidates=int(len(d.last_pick)), survivors=int(d._last["kept"]), winners=len(win))
    return res


print(json.dumps(detector() if args.detector else kernels()))
