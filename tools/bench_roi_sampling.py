"""cfg.roi_sampling (training the classification net on sampled RPN proposals) measured, in the style of tools/bench_box_vote.py:
everything is warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min,
max) is reported, not the best.

  1. the kernel alone (default): frcnn_proposal_targets_batch at B = 1 with R = 300 and 2000 picks and G = 4 ground-truth boxes
     (batch 128, fg_quota 32, the ground truth among the candidates), beside frcnn_nms_device_batch on the same rows in the same
     run (the launch it follows).  Candidates: a third close to a box, a third loosely around one, a third anywhere, so that both
     classes exceed their quotas and the rank walk runs.  Reported per configuration: us per call, and the sampler's counts.
  2. --step: the training step (vgg_small, synthetic 3x450x800 frames, rmsprop through begin_fold as bench.py runs it) with the key
     ABSENT against source = "proposals" at the defaults, as alternating pairs: ms per step and the per-round difference.  With
     the key absent this objective queues what the parent commit's queues; the parent's own figure comes from bench.py run from
     both trees in alternation.

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

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="kernel calls per measurement")
ap.add_argument("--steps", type=int, default=40, help="training steps per measurement of --step")
ap.add_argument("--step", action="store_true")
args = ap.parse_args()
L = F._lib.load()


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 3), min=round(v[0], 3), max=round(v[-1], 3))


def scene(rng, G, R, W=800.0, H=450.0):
    gw = rng.uniform(40, 240, G); gh = rng.uniform(40, 200, G)
    gx = rng.uniform(0, W - gw); gy = rng.uniform(0, H - gh)
    gt = np.stack([gx, gy, gx + gw, gy + gh], 1)
    w = rng.uniform(20, 300, R); h = rng.uniform(20, 240, R)
    x = rng.uniform(0, W - 20, R); y = rng.uniform(0, H - 20, R)
    rect = np.stack([x, y, x + w, y + h], 1)
    kind, which = rng.randint(0, 3, R), rng.randint(0, G, R)
    for i in range(R):
        if kind[i] < 2:
            j = 0.08 if kind[i] == 0 else 0.45
            rect[i] = gt[which[i]] + rng.uniform(-j, j, 4) * np.array([gw[which[i]], gh[which[i]]] * 2)
    return rect, gt


def kernels():
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    configs, info = [], {}
    G, batch, quota = 4, 128, 32
    for R in (300, 2000):
        rect, gt = scene(rng, G, R)
        box5 = np.concatenate([rect, np.log(rng.rand(R, 1) * 0.8 + 0.2)], 1).astype(np.float32)
        d_rect = F.DeviceTensor.from_numpy(rect); d_box5 = F.DeviceTensor.from_numpy(box5)
        d_pick = F.DeviceTensor.from_numpy(rng.permutation(R).astype(np.int64) + 1)
        d_gt = F.DeviceTensor.from_numpy(gt); d_gc = F.DeviceTensor.from_numpy(rng.randint(1, 17, G).astype(np.int32))
        ctl = F.DeviceTensor.from_numpy(np.array([0, 0, 0, 0, R, 0, 0, 0], np.int32))
        outs = [F.DeviceTensor.empty((batch, 4), np.float64), F.DeviceTensor.empty((batch, 4)), F.DeviceTensor.empty((batch,)),
                F.DeviceTensor.empty((batch,), np.int32), F.DeviceTensor.empty((batch,), np.int32),
                F.DeviceTensor.empty((batch,), np.float64)]
        npick = F.DeviceTensor.empty((R,), np.int64)
        wsb = L.frcnn_nms_batch_workspace_bytes(1, R); ws = F.DeviceTensor.empty((wsb,), np.uint8)
        keep = (d_rect, d_box5, d_pick, d_gt, d_gc, ctl, outs, npick, ws)
        G_host = (C.c_int * 1)(G)

        def targets(n, a=keep, R=R, G_host=G_host):
            for _ in range(n):
                F._lib.call("frcnn_proposal_targets_batch", F.ptr(a[0]), F.ptr(a[2]), R, C.c_void_p(a[5].ptr + 16), R, F.ptr(a[3]),
                            F.ptr(a[4]), G, G_host, 1, 1, 0.5, 0.0, 0.5, quota, batch, 17, C.c_uint(7), *([F.ptr(o) for o in a[6]] +
                                                                                                      [batch, F.ptr(a[5]), s]))

        def hard(n, a=keep, R=R, wsb=wsb):
            for _ in range(n):
                F._lib.call("frcnn_nms_device_batch", F.ptr(a[1]), 1, R, R, C.c_void_p(a[5].ptr + 16), 5, C.c_float(0.7), 2, 5, None,
                            F.ptr(a[7]), C.c_void_p(a[5].ptr + 20), F.ptr(a[8]), wsb, s)
        tag = "R%d_G%d" % (R, G)
        configs.append((tag + "/proposal_targets", targets, ctl))
        configs.append((tag + "/nms_device_batch", hard, None))
    for name, fn, ctl in configs:
        fn(5)
        torch.cuda.synchronize()
        if ctl is not None:
            info[name] = dict(counts=[int(v) for v in ctl.numpy()[:4]])
    us = dict((name, []) for name, _, _ in configs)
    for r in range(args.rounds):
        for name, fn, _ in (configs if r % 2 == 0 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.calls)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    res = dict(metric="us per call (B = 1, R picks, G ground-truth boxes, batch 128, fg_quota 32)", calls=args.calls, rounds=args.rounds)
    for name, _, _ in configs:
        res[name] = dict(us=spread(us[name]), **info.get(name, {}))
    return res


def step():
    tables = [("absent", None), ("proposals", dict(source="proposals"))]
    runs = {}
    for name, t in tables:
        cfg = dict(F.duplo_cfg)
        if t is not None:
            cfg["roi_sampling"] = t
        model = F.vgg_small(cfg)
        w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
        it = F.SyntheticBatchIterator(model, H=450, W=800, pool=4)
        stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
        f = F.create_objective(model, w, g, it, stats)
        runs[name] = (f, w, dict(learningRate=1e-5), stats, model)

    def run(name, n):
        f, w, state, _, _ = runs[name]
        for _ in range(n):
            F.rmsprop(f, w, state)
    for name, _ in tables:
        run(name, 10)
    torch.cuda.synchronize()
    ms = dict((name, []) for name, _ in tables)
    for r in range(args.rounds):
        for name, _ in (tables if r % 2 == 0 else tables[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    res = dict(metric="ms per training step (vgg_small 800x450, one image a step, rmsprop)", steps=args.steps, rounds=args.rounds)
    for name, _ in tables:
        res[name] = dict(ms=spread(ms[name]))
    rois = runs["proposals"][3]["rois"]
    res["proposals"].update(last_counts=list(rois[-1]), rows_mean=round(float(np.mean([c[2] + c[3] for c in rois])), 1),
                            fg_mean=round(float(np.mean([c[2] for c in rois])), 1))
    res["proposals"]["minus_absent_ms"] = spread([a - b for a, b in zip(ms["proposals"], ms["absent"])])
    return res


print(json.dumps(step() if args.step else kernels()))
