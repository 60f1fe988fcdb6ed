"""cfg.proposals (score order, pre_nms_top_n, post_nms_top_n) against the default Detector: ms per frame on synthetic 3x450x800
frames (vgg_small), in the style of tools/bench_detect_batch.py.

Weights amplified as there (class head x200), the anchor nets' class logits by --gain: the default 30 gives about 8 000 matches a
frame; the STRESS frames of the capped-against-uncapped comparison need at least twice the largest cap, so raise --gain until the
printed `matches` says so.  Option static_weights on, 4 resident frames cycled.  Every configuration is warmed up, then the
configurations are ALTERNATED in this one process, `--rounds` times; a measurement is `--frames` frames ending in a device
synchronise.  Reported per configuration: median and min-max of the rounds in ms per frame, for the detect() loop and for
detect_batch at B = 8, with the frame's counts (matches, rows of the first NMS, candidates, winners) and the bytes of the
first NMS's workspace per frame.

  python tools/bench_proposals.py --gain 120                 off, {order=score}, a no-op cap, K = 6000 / 2000 / 300
  python tools/bench_proposals.py --caps 300 --post 100      other caps; --post adds post_nms_top_n to the capped configurations
  python tools/bench_proposals.py --kernels                  no Detector: 20 launches each of frcnn_topk_select (K = n, then K = 6000) and
                                                             frcnn_rpn_gather_rows, and of the first NMS, at n = 26 544 and 45 015
                                                             keys -- for a kernel trace taken from outside

The A/B leg "settings off against the parent commit" is tools/bench_detect_batch.py run from both trees in alternation: with the
settings off this Detector queues what the parent's queues.

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
ap.add_argument("--frames", type=int, default=104, help="frames per measurement (a multiple of 8)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--gain", type=float, default=30.0)
ap.add_argument("--caps", default="6000,2000,300")
ap.add_argument("--post", type=int, default=0)
ap.add_argument("--kernels", action="store_true")
args = ap.parse_args()
L = F._lib.load()

if args.kernels:
    rng = np.random.RandomState(0)
    out = {}
    for n in (26544, 45015):
        K = 6000
        p = (-rng.rand(n) * 0.05).astype(np.float32)
        x1 = rng.uniform(0, 780, n); y1 = rng.uniform(0, 430, n)
        box = np.stack([x1, y1, x1 + rng.uniform(8, 150, n), y1 + rng.uniform(8, 150, n)], 1).astype(np.float32)
        dp, db = F.DeviceTensor.from_numpy(p), F.DeviceTensor.from_numpy(box)
        di = F.DeviceTensor.zeros((n, 4), np.int32); dr = F.DeviceTensor.zeros((n, 4), np.float64)
        nd = F.DeviceTensor.from_numpy(np.array([n], np.int32))
        sel = F.DeviceTensor.empty((K,), np.int32); kd = F.DeviceTensor.empty((1,), np.int32)
        sel_all = F.DeviceTensor.empty((n,), np.int32); kd_all = F.DeviceTensor.empty((1,), np.int32)   # (a cap that cuts nothing)
        wsb = L.frcnn_topk_select_workspace_bytes(1, n); ws = F.DeviceTensor.empty((wsb,), np.uint8)
        o = dict(p=F.DeviceTensor.empty((K,)), idx=F.DeviceTensor.empty((K, 4), np.int32), rect=F.DeviceTensor.empty((K, 4), np.float64),
                 box=F.DeviceTensor.empty((K, 4)), box5=F.DeviceTensor.empty((K, 5)), row=F.DeviceTensor.empty((K,), np.int32))
        nwsb = L.frcnn_nms_workspace_bytes(n); nws = F.DeviceTensor.empty((nwsb,), np.uint8)
        pick = F.DeviceTensor.empty((n,), np.int64); cnt = F.DeviceTensor.empty((1,), np.int32)
        s = F.stream_ptr()
        for _ in range(20):
            F._lib.call("frcnn_topk_select", F.ptr(dp), 1, n, n, F.ptr(nd), n, F.ptr(sel_all), n, F.ptr(kd_all), F.ptr(ws), wsb, s)
            F._lib.call("frcnn_topk_select", F.ptr(dp), 1, n, n, F.ptr(nd), K, F.ptr(sel), K, F.ptr(kd), F.ptr(ws), wsb, s)
            F._lib.call("frcnn_rpn_gather_rows", F.ptr(dp), F.ptr(di), F.ptr(dr), F.ptr(db), 1, n, n, F.ptr(sel), K, F.ptr(kd), K,
                        F.ptr(o["p"]), F.ptr(o["idx"]), F.ptr(o["rect"]), F.ptr(o["box"]), F.ptr(o["box5"]), F.ptr(o["row"]), K, s)
            F._lib.call("frcnn_nms_device", F.ptr(db), n, 4, C.c_float(0.25), 0, 0, F.ptr(pick), F.ptr(cnt), F.ptr(nws), nwsb, s)
        torch.cuda.synchronize()
        out["n%d" % n] = dict(selected=int(kd.numpy()[0]), picks=int(cnt.numpy()[0]))
    print(json.dumps(dict(traced="kernels", launches_each=20, **out)))
    sys.exit(0)

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
caps = [int(k) for k in args.caps.split(",") if k]
post = dict(post_nms_top_n=args.post) if args.post else {}
tables = [("off", None), ("score", dict(order="score")), ("score_noop_cap", dict(order="score", pre_nms_top_n=10 ** 6))]
tables += [("score_K%d" % k, dict(order="score", pre_nms_top_n=k, **post)) for k in caps]
tables += [("y2_K%d" % k, dict(order="y2", pre_nms_top_n=k)) for k in caps[:1]]
dets = dict((name, F.Detector(model, static_weights=True, proposals=t)) for name, t in tables)


def run_detect(d, n):
    for i in range(n):
        d.detect(imgs[i % 4])


def run_batch(d, n):
    for lo in range(0, n, 8):
        d.detect_batch([imgs[(lo + i) % 4] for i in range(8)])


configs = [(name + "/" + kind, (lambda n, d=dets[name], fn=fn: fn(d, n))) for name, _ in tables
           for kind, fn in (("detect", run_detect), ("batch8", run_batch))]
for name, fn in configs:      # warm-up: every shape, every buffer
    fn(16)
torch.cuda.synchronize()
ms = dict((name, []) for name, _ in configs)
for r in range(args.rounds):
    for name, fn in configs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(args.frames)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) / args.frames * 1e3)
res = dict(metric="ms per frame (vgg_small 800x450 inference)", frames=args.frames, rounds=args.rounds, gain=args.gain)
for name, t in tables:
    d = dets[name]
    win = d.detect(imgs[0])
    n = int(d.last_scan["n"])
    matches = int(d.last_scan.get("matches", n))
    anchors = 26544
    ncap = min(anchors, t["pre_nms_top_n"]) if t and "pre_nms_top_n" in t else max(min(anchors, d.NMS_FIRST_CAP), n)
    res[name] = dict(matches=matches, nms_rows=n, candidates=int(len(d.last_pick)), winners=len(win),
                     nms_workspace_bytes_per_frame=int(L.frcnn_nms_workspace_bytes(ncap)))
    for kind in ("detect", "batch8"):
        v = sorted(ms[name + "/" + kind])
        res[name][kind] = dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4))
print(json.dumps(res))
