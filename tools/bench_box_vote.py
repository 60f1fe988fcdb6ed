"""cfg.box_voting (box voting behind the per-class pass) measured, in the style of tools/bench_soft_nms.py: everything is warmed
up, the configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min, max) is reported, not
the best.

  1. the kernel alone (default): frcnn_box_vote_batch as the Detector calls it (log-confidences, weight_mode 2, classes, fp64
     rects) at B = 1 and 8 for K survivors and W winners a segment -- (64, 16), (300, 60) and (1404, 300): what detect leaves
     behind the class test at 800x450 with the reference's thresholds up to no cap at all -- and --big adds (4096, 800), the
     global-memory tier; beside frcnn_nms_device_batch on the same rows in the same run (the launch it follows).  Boxes:
     clusters of about 12 around common centres, as a frame's class-test survivors come.  Reported per configuration: us per
     call, and for the voting kernel the voters of segment 0's winners.
  2. --detector: detect_batch (B = 8) per frame on synthetic 3x450x800 frames (vgg_small, weights amplified as in
     tools/bench_proposals.py): the key ABSENT against present ("score" and "uniform", overlap 0.1), as alternating pairs.  The
     first figure is the one claim this tool supports: with the key absent this Detector queues what the parent commit's
     queues.  The parent's own figure comes from tools/bench_detect_batch.py run from both trees in alternation in the same
     session; the spread of the alternating pairs printed here is what any difference has to be read against.

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
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    configs, info = [], {}
    for B in (1, 8):
        for K, W in ((64, 16), (300, 60), (1404, 300)) + (((4096, 800),) if args.big else ()):
            k = max(K // 12, 1)
            g = np.arange(B * K) % k
            x1 = rng.randint(0, 700, k)[g] + rng.randint(-20, 21, B * K); y1 = rng.randint(0, 380, k)[g] + rng.randint(-20, 21, B * K)
            rows = np.stack([x1, y1, x1 + rng.randint(20, 80, B * K), y1 + rng.randint(20, 80, B * K),
                             np.log(rng.rand(B * K) * 0.8 + 0.2)], 1).astype(np.float32)
            d = F.DeviceTensor.from_numpy(rows)
            cls = F.DeviceTensor.from_numpy(rng.randint(1, 21, B * K).astype(np.int32))
            rect = F.DeviceTensor.from_numpy(rows[:, :4].astype(np.float64))
            nd = F.DeviceTensor.from_numpy(np.full(B, K, np.int32))
            wins = F.DeviceTensor.from_numpy(np.full(B, W, np.int32))
            hp = np.zeros((B, K), np.int64)
            for b in range(B):
                hp[b, :W] = rng.permutation(K)[:W] + 1
            pick = F.DeviceTensor.from_numpy(hp)
            out = F.DeviceTensor.empty((B * K, 4), np.float64); votes = F.DeviceTensor.zeros((B * K,), np.int32)
            hpick = F.DeviceTensor.empty((B * K,), np.int64); hcnt = F.DeviceTensor.empty((B,), np.int32)
            hwsb = L.frcnn_nms_batch_workspace_bytes(B, K); hws = F.DeviceTensor.empty((hwsb,), np.uint8)
            keep = (d, cls, rect, nd, wins, pick, out, votes, hpick, hcnt, hws)

            def vote(n, a=keep, B=B, K=K):
                for _ in range(n):
                    F._lib.call("frcnn_box_vote_batch", F.ptr(a[0]), B, K, K, F.ptr(a[3]), 5, 5, 2, C.c_float(0.1), F.ptr(a[1]),
                                F.ptr(a[2]), F.ptr(a[5]), F.ptr(a[4]), F.ptr(a[6]), F.ptr(a[7]), s)

            def hard(n, a=keep, B=B, K=K, hwsb=hwsb):
                for _ in range(n):
                    F._lib.call("frcnn_nms_device_batch", F.ptr(a[0]), B, K, K, F.ptr(a[3]), 5, C.c_float(0.1), 2, 5, F.ptr(a[1]),
                                F.ptr(a[8]), F.ptr(a[9]), F.ptr(a[10]), hwsb, s)
            tag = "B%d_K%d_W%d" % (B, K, W)
            configs.append((tag + "/box_vote", vote, (votes, hp[0, :W] - 1)))
            configs.append((tag + "/bitmatrix_hard", hard, None))
    for name, fn, v in configs:
        fn(5)
        torch.cuda.synchronize()
        if v is not None:
            got = v[0].numpy()[v[1]]
            info[name] = dict(voters_mean=round(float(got.mean()), 2), voters_max=int(got.max()))
    us = dict((name, []) for name, _, _ in configs)
    for r in range(args.rounds):
        for name, fn, _ in (configs if r % 2 == 0 else configs[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.calls)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    res = dict(metric="us per call (K survivors, W winners a segment)", calls=args.calls, rounds=args.rounds)
    for name, _, _ in configs:
        res[name] = dict(us=spread(us[name]), **info.get(name, {}))
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
    tables = [("absent", None), ("score", dict(overlap=0.1)), ("uniform", dict(overlap=0.1, weight="uniform"))]
    dets = dict((name, F.Detector(model, static_weights=True, box_voting=t)) for name, t in tables)

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
        if "votes" in d._last:
            v = d._last["votes"]
            res[name].update(voters_max=int(v.max()) if v.size else 0, winners_voted=int((v > 1).sum()))
    # the differences of the alternating pairs (present - absent, per round): what "costs nothing" is read against
    for name in ("score", "uniform"):
        res[name]["minus_absent_ms"] = spread([a - b for a, b in zip(ms[name], ms["absent"])])
    return res


print(json.dumps(detector() if args.detector else kernels()))
