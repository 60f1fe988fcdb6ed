"""The optimiser passes alone on vgg_small's flat vector (26 784 106 parameters): HIP-event time of each whole-vector form of
optim.rmsprop / optim.sgd / optim.nag (main.lua:122-124,133-135) and optim.adam, and the effective bytes/s of the fp32 streams it
moves (read x, g[, v]; write x[, g][, v]; adam reads and writes two state vectors); the gradient guard (frcnn_grad_clip: one more read of g, two small launches behind it)
alone and in front of each optimiser's pass, which then takes its divisor from the guard's record.
python tools/bench_optim.py [--n N] [--reps R] [--json FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import frcnn_amd as F


def forms(x, g, v, v2, gc, n, s):
    """(name, fp32 streams per element, launch) -- the streams as the kernels move them"""
    import torch
    P = F.ptr
    wsb = F._lib.load().frcnn_grad_clip_workspace_bytes(n)
    ws = torch.empty(wsb // 8, dtype=torch.float64, device="cuda")
    rec = torch.zeros(4, dtype=torch.float64, device="cuda")
    # a clip norm far above the gradient's: D' = D = 1 (the device-divisor forms always run the scaled pass; g keeps its values)
    clip = lambda: F._lib.call("frcnn_grad_clip", P(g), n, None, 0, 1.0, None, 1e30, P(rec), P(ws), wsb, s)
    dp = P(rec[2:])
    guarded = lambda fn: (lambda: (clip(), fn()))
    sc = 1.0 + 2.0 ** -23
    sgd = lambda gs, gcount, wd, mom, omd, nest, first: (
        lambda: F._lib.call("frcnn_sgd", P(x), P(g), P(v) if mom else None, n, gs, gcount, 1e-9, wd, mom, omd, nest, first, s))
    nag = lambda gs, wd, first: (lambda: F._lib.call("frcnn_nag", P(x), P(g), P(v), n, gs, None, 1e-9, wd, 0.9, first, s))
    # optim.adam: m travels in v, v in v2 (non-negative, and it stays so)
    adam = lambda gs, wd, decay: (lambda: F._lib.call("frcnn_adam", P(x), P(g), P(v), P(v2), n, gs, None, 1e-9, 0.9, 0.1, 0.999, 1e-3, 1e-8,
                                                      wd, decay, s))
    return [
        ("rmsprop, scaled (the default)", 6, lambda: F._lib.call("frcnn_scale_rmsprop", P(x), P(g), sc, P(v), n, 1e-9, 0.99, 1e-8, s)),
        ("sgd plain", 3, sgd(1.0, None, 0.0, 0.0, 1.0, 0, 0)),
        ("sgd sgd_state, scaled", 6, sgd(sc, None, 5e-4, 0.9, 0.1, 0, 0)),
        ("sgd sgd_state, scaled, first", 5, sgd(sc, None, 5e-4, 0.9, 0.1, 0, 1)),
        ("sgd sgd_state, device divisor", 6, sgd(1.0, P(gc), 5e-4, 0.9, 0.1, 0, 0)),
        ("sgd nesterov, scaled", 6, sgd(sc, None, 5e-4, 0.9, 1.0, 1, 0)),
        ("sgd momentum, unscaled", 5, sgd(1.0, None, 0.0, 0.9, 0.1, 0, 0)),
        ("nag nag_state, scaled", 6, nag(sc, 0.0, 0)),
        ("nag nag_state, unscaled", 5, nag(1.0, 0.0, 0)),
        ("nag look-ahead", 3, lambda: F._lib.call("frcnn_nag_lookahead", P(x), P(v), n, 1e-9, s)),
        ("grad_clip alone", 1, clip),
        ("rmsprop, device divisor", 6, lambda: F._lib.call("frcnn_scale_rmsprop_dev", P(x), P(g), P(gc), P(v), n, 1e-9, 0.99, 1e-8, s)),
        ("grad_clip + rmsprop", 7, guarded(lambda: F._lib.call("frcnn_scale_rmsprop_dev", P(x), P(g), dp, P(v), n, 1e-9, 0.99, 1e-8, s))),
        ("grad_clip + sgd sgd_state", 7, guarded(sgd(1.0, dp, 5e-4, 0.9, 0.1, 0, 0))),
        ("grad_clip + nag nag_state", 7, guarded(lambda: F._lib.call("frcnn_nag", P(x), P(g), P(v), n, 1.0, dp, 1e-9, 0.0, 0.9, 0, s))),
        ("adam, unscaled", 7, adam(1.0, 0.0, 0.0)),
        ("adam, scaled", 8, adam(sc, 0.0, 0.0)),
        ("adam, scaled, coupled decay", 8, adam(sc, 5e-4, 0.0)),
        ("adam, scaled, decoupled decay", 8, adam(sc, 0.0, 1e-9)),
        ("adam slice, scaled", 8, lambda: F._lib.call("frcnn_adam_slice", P(x), P(g), P(v), P(v2), 5, n - 2, sc, 1e-9, 0.9, 0.1, 0.999, 1e-3,
                                                      1e-8, 0.0, 0.0, s)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=26784106)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a HIP device")
    n = a.n
    # tiny steps and a scale factor of 1 + 2^-23 (1 itself selects the unscaled form) keep the vectors finite and normal
    x = torch.randn(n, device="cuda"); g = torch.randn(n, device="cuda") * 1e-3; v = torch.rand(n, device="cuda")
    v2 = torch.rand(n, device="cuda")
    gc = torch.tensor([1.0], dtype=torch.float64, device="cuda")
    s = F.stream_ptr()
    rows = []
    for name, streams, fn in forms(x, g, v, v2, gc, n, s):
        for _ in range(5):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        t1.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.reps
        gbs = streams * 4.0 * n / (us * 1e-6) / 1e9
        rows.append(dict(form=name, streams=streams, us=round(us, 2), GBps=round(gbs, 1)))
        print("%-32s %d streams  %8.1f us  %7.1f GB/s" % (name, streams, us, gbs), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(n=n, reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
