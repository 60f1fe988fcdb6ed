"""cfg.roi_sampling.source = "hard" (online hard example mining) measured, in the style of tools/bench_roi_sampling.py: everything
is warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min, max) is reported.

  1. the parts alone (default), at N = 300 and N = 2064 labelled candidates (a quarter foreground, 21 classes, boxes clustered
     around a few centres so that the NMS has something to suppress): frcnn_roi_hard_keys_batch, frcnn_nms_device_batch keyed by
     the loss at 0.7, frcnn_roi_hard_gather_batch at batch 128 -- and the scoring pass on vgg_small's 800x450 feature map: ROI windows
     + ROI max pooling without the arg-max record + the classification net in evaluate mode on those N rows.
  2. --step: the training step (vgg_small, synthetic 3x450x800 frames, rmsprop as bench.py runs it) with the key ABSENT, with
     source = "proposals" and with source = "hard" at the defaults, alternating: ms per step, the differences per round, and the mean
     N (labelled candidates), survivors and selected rows under "hard".

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
ap.add_argument("--calls", type=int, default=50, help="calls per measurement of the parts")
ap.add_argument("--steps", type=int, default=40, help="training steps per measurement of --step")
ap.add_argument("--step", action="store_true")
args = ap.parse_args()
L = F._lib.load()


def spread(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 3), min=round(v[0], 3), max=round(v[-1], 3))


def alternate(configs, per):
    for _, fn in configs:
        fn(5)
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


def parts():
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    ncls, batch = 21, 128
    model = F.vgg_small(dict(F.duplo_cfg))
    F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    it = F.SyntheticBatchIterator(model, H=450, W=800, pool=1)
    fm = model["pnet"].forward(F.to_device(it.pool[0]["img"]))[-1]
    fmC, fmH, fmW = fm.shape
    kh, kw, _, _ = F.roi_pooling_settings(model["cfg"])
    loc = F.Localizer(model["pnet"].outnode.children[-1])
    layers = np.array([[l["kW"], l["kH"], l["dW"], l["dH"], l["padW"], l["padH"]] for l in loc.layers], np.int32).reshape(-1, 6)
    cnet_ncls = model["cfg"]["class_count"] + 1
    configs, info, keep = [], {}, []
    for N in (300, 2064):
        nfg = N // 4
        c = rng.rand(12, 2) * np.array([700.0, 350.0])
        k = rng.randint(0, 12, N)
        xy = c[k] + rng.randn(N, 2) * 25.0
        wh = 30.0 + rng.rand(N, 2) * 120.0
        roi = np.concatenate([xy, xy + wh], 1)
        logits = rng.randn(N, ncls) * 2.0
        d = dict(roi=roi, crout=rng.randn(N, 4).astype(np.float32), crtarget=(rng.randn(N, 4) * 0.5).astype(np.float32),
                 ccout=(logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32),
                 cctarget=np.where(np.arange(N) < nfg, 1 + rng.randint(0, ncls - 1, N), ncls).astype(np.float32),
                 src=np.arange(N, dtype=np.int32), gt_idx=np.zeros(N, np.int32), iou=rng.rand(N))
        d = dict((key, F.DeviceTensor.from_numpy(v)) for key, v in d.items())
        ctl = F.DeviceTensor.from_numpy(np.array([N, nfg, 0, 0, 0, 0, 0, 0], np.int32))
        c_n, c_f, c_s, c_o = (C.c_void_p(ctl.ptr + 4 * j) for j in (0, 1, 2, 4))
        box5 = F.DeviceTensor.empty((N, 5)); loss = F.DeviceTensor.empty((N,)); pick = F.DeviceTensor.empty((N,), np.int64)
        wsb = L.frcnn_nms_batch_workspace_bytes(1, N); ws = F.DeviceTensor.empty((wsb,), np.uint8)
        out = [F.DeviceTensor.empty((batch, 4), np.float64), F.DeviceTensor.empty((batch, 4)), F.DeviceTensor.empty((batch,)),
               F.DeviceTensor.empty((batch,), np.int32), F.DeviceTensor.empty((batch,), np.int32),
               F.DeviceTensor.empty((batch,), np.float64), F.DeviceTensor.empty((batch,))]
        wins = F.DeviceTensor.empty((N, 4), np.int32); cin = F.DeviceTensor.empty((N, fmC * kh * kw))
        sc = (F.DeviceTensor.empty((N, 4)), F.DeviceTensor.empty((N, cnet_ncls)))
        keep.append((d, ctl, box5, loss, pick, ws, out, wins, cin, sc))

        def keys(n, d=d, N=N, c_n=c_n, c_f=c_f, box5=box5, loss=loss):
            for _ in range(n):
                F._lib.call("frcnn_roi_hard_keys_batch", F.ptr(d["roi"]), F.ptr(d["crout"]), F.ptr(d["crtarget"]), F.ptr(d["ccout"]),
                            F.ptr(d["cctarget"]), 1, N, N, c_n, c_f, ncls, F.ptr(box5), F.ptr(loss), s)

        def nms(n, N=N, c_n=c_n, c_s=c_s, box5=box5, pick=pick, ws=ws, wsb=wsb):
            for _ in range(n):
                F._lib.call("frcnn_nms_device_batch", F.ptr(box5), 1, N, N, c_n, 5, C.c_float(0.7), 2, 5, None, F.ptr(pick), c_s, F.ptr(ws),
                            wsb, s)

        def gather(n, d=d, N=N, c_n=c_n, c_f=c_f, c_s=c_s, c_o=c_o, loss=loss, pick=pick, out=out):
            for _ in range(n):
                F._lib.call("frcnn_roi_hard_gather_batch", F.ptr(pick), c_s, batch, F.ptr(d["roi"]), F.ptr(d["crtarget"]),
                            F.ptr(d["cctarget"]), F.ptr(d["src"]), F.ptr(d["gt_idx"]), F.ptr(d["iou"]), F.ptr(loss), 1, N, N, c_n, c_f,
                            *([F.ptr(o) for o in out] + [batch, c_o, s]))

        def score(n, d=d, N=N, wins=wins, cin=cin, sc=sc):
            for _ in range(n):
                F._lib.call("frcnn_roi_windows", F.ptr(d["roi"]), None, N, layers.ctypes.data_as(C.c_void_p), len(layers), fmH, fmW,
                            F.ptr(wins), s)
                F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), fmC, fmH, fmW, F.ptr(wins), N, kh, kw, F.ptr(cin), None, s)
                model["cnet"].score(cin, sc)
        tag = "N%d" % N
        configs += [(tag + "/keys", keys), (tag + "/nms_device_batch", nms), (tag + "/gather", gather), (tag + "/scoring_pass", score)]
        keys(1); nms(1); gather(1)
        torch.cuda.synchronize()
        info[tag] = dict(counts=[int(v) for v in ctl.numpy()[4:8]])
    t = alternate(configs, args.calls)
    res = dict(metric="us per call (B = 1, N rows, 21 classes, batch 128, overlap 0.7; scoring pass: windows + pooling + evaluate-mode net)",
               calls=args.calls, rounds=args.rounds)
    for name, _ in configs:
        res[name] = dict(us=spread([v * 1e6 for v in t[name]]))
    res.update(info)
    return res


def step():
    tables = [("absent", None), ("proposals", dict(source="proposals")), ("hard", dict(source="hard"))]
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

    def runner(name):
        f, w, state, _, _ = runs[name]

        def run(n):
            for _ in range(n):
                F.rmsprop(f, w, state)
        return run
    configs = [(name, runner(name)) for name, _ in tables]
    for _, fn in configs:
        fn(5)
    t = alternate(configs, args.steps)
    res = dict(metric="ms per training step (vgg_small 800x450, one image a step, rmsprop)", steps=args.steps, rounds=args.rounds)
    for name, _ in tables:
        res[name] = dict(ms=spread([v * 1e3 for v in t[name]]))
    hard, rois = runs["hard"][3]["hard"], runs["hard"][3]["rois"]
    res["hard"].update(N_mean=round(float(np.mean([h[0] for h in hard])), 1), survivors_mean=round(float(np.mean([h[1] for h in hard])), 1),
                       rows_mean=round(float(np.mean([c[2] + c[3] for c in rois])), 1), fg_mean=round(float(np.mean([c[2] for c in rois])), 1))
    prois = runs["proposals"][3]["rois"]
    res["proposals"].update(rows_mean=round(float(np.mean([c[2] + c[3] for c in prois])), 1))
    res["hard"]["minus_proposals_ms"] = spread([(a - b) * 1e3 for a, b in zip(t["hard"], t["proposals"])])
    res["hard"]["minus_absent_ms"] = spread([(a - b) * 1e3 for a, b in zip(t["hard"], t["absent"])])
    return res


print(json.dumps(step() if args.step else parts()))
