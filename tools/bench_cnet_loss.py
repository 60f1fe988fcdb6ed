"""cfg.cnet_loss (the classification net's losses row by row) measured, in the style of tools/bench_roi_hard.py: everything is
warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min, max) is reported.

  1. the kernel (default): frcnn_cnet_loss_rows in the training mode plus its frcnn_loss_accumulate, beside frcnn_cnet_losses --
     the yardstick -- on the same rows, at R = 128 and 2 064 rows (a quarter foreground), 17 and 201 classes, under each setting
     of cls (nll, smoothed, focal) and box (smooth_l1, giou).
  2. --step: the training step (vgg_small, synthetic 3x450x800 frames, rmsprop as bench.py runs it) under roi_sampling
     "proposals" and "hard", each with the key ABSENT, with {} and with focal + GIoU, alternating: ms per step.
The 800x450 step with the key absent against the parent commit is bench.py's own measurement (--steps 100 --warmup 20) on the
two trees in alternation; this tool does not run it.

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
from frcnn_amd.objective import cnet_loss_desc, cnet_loss_settings  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="calls per measurement of the kernel")
ap.add_argument("--steps", type=int, default=40, help="training steps per measurement of --step")
ap.add_argument("--step", action="store_true")
args = ap.parse_args()

SETTINGS = [("default", {}), ("smoothed", dict(label_smoothing=0.1)), ("focal", dict(cls="focal")), ("giou", dict(box="giou")),
            ("focal_giou", dict(cls="focal", box="giou"))]


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


def kernel():
    rng = np.random.RandomState(0)
    s = F.stream_ptr()
    configs, keep = [], []
    for R in (128, 2064):
        for ncls in (17, 201):
            npos = R // 4
            logits = rng.randn(R, ncls) * 2.0
            crt = (rng.randn(R, 4) * 0.5).astype(np.float32); crt[npos:] = 0.0
            d = dict(crout=(crt + rng.randn(R, 4) * 0.3).astype(np.float32), crtarget=crt,
                     ccout=(logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32),
                     cctarget=np.where(np.arange(R) < npos, 1 + rng.randint(0, ncls - 1, R), ncls).astype(np.float32))
            d = dict((k, F.DeviceTensor.from_numpy(v)) for k, v in d.items())
            crdelta = F.DeviceTensor.empty((R, 4)); ccdelta = F.DeviceTensor.empty((R, ncls))
            row_loss = F.DeviceTensor.empty((R, 2), np.float64); acc = F.DeviceTensor.zeros((8,), np.float64)
            keep.append((d, crdelta, ccdelta, row_loss, acc))
            tag = "R%d/ncls%d/" % (R, ncls)

            def parent(n, d=d, R=R, npos=npos, ncls=ncls, crdelta=crdelta, ccdelta=ccdelta, acc=acc):
                for _ in range(n):
                    F._lib.call("frcnn_cnet_losses", F.ptr(d["crout"]), F.ptr(d["crtarget"]), F.ptr(d["ccout"]), F.ptr(d["cctarget"]), R, npos,
                                ncls, F.ptr(crdelta), F.ptr(ccdelta), C.c_void_p(acc.ptr + 32), s)
            configs.append((tag + "frcnn_cnet_losses", parent))
            for name, table in SETTINGS:
                desc = cnet_loss_desc(cnet_loss_settings(dict(cnet_loss=table)), ncls)
                keep.append(desc)

                def rows(n, d=d, R=R, npos=npos, ncls=ncls, crdelta=crdelta, ccdelta=ccdelta, row_loss=row_loss, acc=acc, desc=desc):
                    for _ in range(n):
                        F._lib.call("frcnn_cnet_loss_rows", F.ptr(d["crout"]), F.ptr(d["crtarget"]), F.ptr(d["ccout"]), F.ptr(d["cctarget"]),
                                    None, R, npos, ncls, C.byref(desc), F.ptr(crdelta), F.ptr(ccdelta), F.ptr(row_loss), None, None, s)
                        F._lib.call("frcnn_loss_accumulate", F.ptr(row_loss), R, C.c_void_p(acc.ptr + 32), s)
                configs.append((tag + "rows+accumulate/" + name, rows))
    t = alternate(configs, args.calls)
    res = dict(metric="us per call, queued back to back (training mode; a quarter of the rows foreground)", calls=args.calls,
               rounds=args.rounds)
    for name, _ in configs:
        res[name] = dict(us=spread([v * 1e6 for v in t[name]]))
    return res


def step():
    tables = [(src + "/" + name, dict(source=src), cl) for src in ("proposals", "hard")
              for name, cl in (("absent", None), ("empty", {}), ("focal_giou", dict(cls="focal", box="giou")))]
    runs = {}
    for name, rs, cl in tables:
        cfg = dict(F.duplo_cfg)
        cfg["roi_sampling"] = rs
        if cl is not None:
            cfg["cnet_loss"] = cl
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
    configs = [(name, runner(name)) for name, _, _ in tables]
    t = alternate(configs, args.steps)
    res = dict(metric="ms per training step (vgg_small 800x450, one image a step, rmsprop)", steps=args.steps, rounds=args.rounds)
    for name, _, _ in tables:
        rois = runs[name][3]["rois"]
        res[name] = dict(ms=spread([v * 1e3 for v in t[name]]), rows_mean=round(float(np.mean([c[2] + c[3] for c in rois])), 1))
    return res


print(json.dumps(step() if args.step else kernel()))
