"""cfg.box_head (per-class box regression in the classification net) measured, in the style of tools/bench_cnet_loss.py: everything
is warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min, max) is
reported.

  1. the kernels (default): frcnn_box_head_forward, and the two kernels of frcnn_box_head_backward each on its own (input
     gradient; weight and bias gradient), at R = 300 and 2 064 rows (a quarter foreground, the rest background), nf = 512,
     C = 16 and 200 classes -- and beside each, in the same run, the DENSE alternative the grouped kernels must justify
     themselves against: frcnn_linear_forward / frcnn_linear_backward to R x 4C (the full product, of which a row uses 4 columns).
  2. --step: the training step (vgg_small, synthetic 3x450x800 frames, rmsprop as bench.py runs it) with per_class against the key
     absent, under the example rows, roi_sampling "proposals" and "hard", alternating: ms per step.
  3. --detect: Detector.detect_batch at B = 8 (the model of tools/bench_detect_batch.py) with per_class against the key absent.
The 800x450 step and detect_batch with the key absent against the parent commit are bench.py's and tools/bench_detect_batch.py's
own measurements on the two trees in alternation; this tool does not run them.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import frcnn_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="calls per measurement of a kernel")
ap.add_argument("--steps", type=int, default=40, help="training steps per measurement of --step")
ap.add_argument("--frames", type=int, default=208, help="frames per measurement of --detect")
ap.add_argument("--step", action="store_true")
ap.add_argument("--detect", action="store_true")
args = ap.parse_args()


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
    nf = 512
    configs, keep = [], []
    for R in (300, 2064):
        for Cn in (16, 200):
            npos = R // 4
            dev = lambda a: F.DeviceTensor.from_numpy(a)
            x = dev(rng.standard_normal((R, nf)).astype(np.float32))
            W = dev((rng.standard_normal((4 * Cn, nf)) * 0.05).astype(np.float32))
            b = dev(rng.standard_normal(4 * Cn).astype(np.float32))
            cl = dev(np.where(np.arange(R) < npos, 1 + rng.randint(0, Cn, R), Cn + 1).astype(np.float32))
            g = dev(rng.standard_normal((R, 4)).astype(np.float32))
            out, sel = F.DeviceTensor.zeros((R, 4)), F.DeviceTensor.zeros((R,), np.int32)
            gfeat, gW, gb = F.DeviceTensor.zeros((R, nf)), F.DeviceTensor.zeros((4 * Cn, nf)), F.DeviceTensor.zeros((4 * Cn,))
            dense_out, dense_g = F.DeviceTensor.zeros((R, 4 * Cn)), F.DeviceTensor.zeros((R, 4 * Cn))
            keep.append((x, W, b, cl, g, out, sel, gfeat, gW, gb, dense_out, dense_g))
            F._lib.call("frcnn_box_head_forward", F.ptr(x), R, nf, F.ptr(W), F.ptr(b), Cn, F.ptr(cl), 2, 0, None, 0, F.ptr(out),
                        F.ptr(sel), s)
            tag = "R%d/C%d/" % (R, Cn)

            def fwd(n, x=x, W=W, b=b, cl=cl, out=out, sel=sel, R=R, Cn=Cn):
                for _ in range(n):
                    F._lib.call("frcnn_box_head_forward", F.ptr(x), R, nf, F.ptr(W), F.ptr(b), Cn, F.ptr(cl), 2, 0, None, 0,
                                F.ptr(out), F.ptr(sel), s)

            def dgrad(n, x=x, W=W, g=g, sel=sel, gfeat=gfeat, R=R, Cn=Cn):
                for _ in range(n):
                    F._lib.call("frcnn_box_head_backward", F.ptr(g), F.ptr(x), F.ptr(sel), R, nf, F.ptr(W), Cn, F.ptr(gfeat), None,
                                None, s)

            def wgrad(n, x=x, g=g, sel=sel, gW=gW, gb=gb, R=R, Cn=Cn):
                for _ in range(n):
                    F._lib.call("frcnn_box_head_backward", F.ptr(g), F.ptr(x), F.ptr(sel), R, nf, None, Cn, None, F.ptr(gW),
                                F.ptr(gb), s)

            def dense_fwd(n, x=x, W=W, b=b, y=dense_out, R=R, Cn=Cn):
                for _ in range(n):
                    F._lib.call("frcnn_linear_forward", F.ptr(x), R, nf, F.ptr(W), F.ptr(b), 4 * Cn, F.ptr(y), s)

            def dense_dgrad(n, x=x, W=W, gy=dense_g, gfeat=gfeat, R=R, Cn=Cn):
                for _ in range(n):
                    F._lib.call("frcnn_linear_backward", F.ptr(x), F.ptr(gy), R, nf, F.ptr(W), 4 * Cn, F.ptr(gfeat), None, None, s)

            def dense_wgrad(n, x=x, W=W, gy=dense_g, gW=gW, gb=gb, R=R, Cn=Cn):
                for _ in range(n):
                    F._lib.call("frcnn_linear_backward", F.ptr(x), F.ptr(gy), R, nf, F.ptr(W), 4 * Cn, None, F.ptr(gW), F.ptr(gb), s)
            configs += [(tag + "forward", fwd), (tag + "dense/forward", dense_fwd), (tag + "input_gradient", dgrad),
                        (tag + "dense/input_gradient", dense_dgrad), (tag + "weight_gradient", wgrad),
                        (tag + "dense/weight_gradient", dense_wgrad)]
    t = alternate(configs, args.calls)
    res = dict(metric="us per call, queued back to back (nf = 512; a quarter of the rows foreground, the rest background; dense = "
                      "frcnn_linear_* to R x 4C)", calls=args.calls, rounds=args.rounds)
    for name, _ in configs:
        res[name] = dict(us=spread([v * 1e6 for v in t[name]]))
    return res


def step():
    tables = [(src + "/" + name, src, bh) for src in ("examples", "proposals", "hard")
              for name, bh in (("absent", None), ("per_class", dict(per_class=True)))]
    runs = {}
    for name, src, bh in tables:
        cfg = dict(F.duplo_cfg)
        if src != "examples":
            cfg["roi_sampling"] = dict(source=src)
        if bh is not None:
            cfg["box_head"] = bh
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
        res[name] = dict(ms=spread([v * 1e3 for v in t[name]]))
    return res


def detect():
    from detect_bench_model import amplified_vgg_small
    imgs = [F.to_device(F.synthetic_image(450, 800, i)) for i in range(4)]
    dets, keep = {}, []
    for name, bh in (("absent", None), ("per_class", dict(per_class=True))):
        if bh is None:
            cfg, model, weights, gradient = amplified_vgg_small(F, 30.0)
        else:   # the same amplified weights on the longer vector: every class's rows are the shared head's four
            cfg0, base, w0, _ = amplified_vgg_small(F, 30.0)
            cfg = dict(cfg0, box_head=bh)
            model = F.vgg_small(cfg)
            nat, wb = model["native"], w0.cpu().numpy()
            (ow, nw, _, nf), (ob, nb, _, _) = (tuple(int(v) for v in r) for r in base["native"].param_table[-4:-2])
            Cn = cfg["class_count"]
            wp = np.concatenate([wb[:ow], np.tile(wb[ow:ob], Cn), np.tile(wb[ob:ob + nb], Cn), wb[ob + nb:]])
            weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], weights_host=wp)
        keep.append((model, weights, gradient))
        d = F.Detector(model, static_weights=True)
        d.BATCH = 8
        dets[name] = d

    def runner(d):
        def run(n):
            for lo in range(0, n, 8):
                d.detect_batch([imgs[(lo + i) % 4] for i in range(min(8, n - lo))])
        return run
    configs = [(name, runner(d)) for name, d in dets.items()]
    t = alternate(configs, args.frames, warm=32)
    res = dict(metric="ms per frame (vgg_small 800x450 inference, detect_batch at B = 8)", frames=args.frames, rounds=args.rounds)
    for name, d in dets.items():
        d.detect(imgs[0])
        res[name] = dict(ms=spread([v * 1e3 for v in t[name]]), candidates=int(len(d.last_pick)))
    return res


print(json.dumps(step() if args.step else detect() if args.detect else kernels()))
