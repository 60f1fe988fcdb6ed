"""cfg.scoring.boxes = "class" (the box of its own class for every class row) measured, in the style of tools/bench_box_head.py:
everything is warmed up, the configurations are ALTERNATED in this one process `--rounds` times, and the spread (median, min,
max) is reported.

  1. the kernel (default): frcnn_detect_class_boxes_batch at B = 8 frames, nf = 512, C = 16, with 1 571 and 6 562 class rows a frame
     (the README's scoring paragraph: "all" at 0.2 and at 0.05), the rows of a candidate adjacent -- and beside it, in the same
     run, what it avoids and what it needs: the DENSE product frcnn_linear_forward to R x 4C over the frames' candidates (of which
     a row would use 4 columns, and which a gather + decode would still have to follow), and the B feature copies
     (frcnn_memcpy_d2d of a frame's R x nf floats each: the cost of cnet.features).
  2. --detect: Detector.detect_batch at B = 8 (the model of tools/bench_detect_batch.py, 800x450) under "all" at 0.2 and at 0.05:
     a per-class model with boxes = "class" against a shared-head model with the same settings.
The key absent against the parent commit is bench.py's and tools/bench_detect_batch.py's own measurement on the two trees in
alternation; this tool does not run it.

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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import frcnn_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=50, help="calls per measurement of a kernel")
ap.add_argument("--frames", type=int, default=208, help="frames per measurement of --detect")
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
    B, nf, Cn, cands = 8, 512, 16, 1403       # 1 403 candidates a frame: the Detector's count at 800x450 on the bench model
    dev = F.DeviceTensor.from_numpy
    feat = dev(rng.standard_normal((B * cands, nf)).astype(np.float32))
    W = dev((rng.standard_normal((4 * Cn, nf)) * 0.01).astype(np.float32))
    b = dev((rng.standard_normal(4 * Cn) * 0.1).astype(np.float32))
    x0, y0 = rng.uniform(0, 700, (B, cands)), rng.uniform(0, 400, (B, cands))
    rect = dev(np.stack([x0, y0, x0 + rng.uniform(8, 90, (B, cands)), y0 + rng.uniform(8, 90, (B, cands))], 2))
    pick = dev(np.stack([rng.permutation(cands) + 1 for _ in range(B)]).astype(np.int64))
    row0 = (C.c_longlong * B)(*[i * cands for i in range(B)])
    dense = F.DeviceTensor.zeros((B * cands, 4 * Cn))
    copy_dst = F.DeviceTensor.zeros((B * cands, nf))
    configs, keep = [], []
    for rows in (1571, 6562):
        per = np.full(cands, rows // cands)    # class rows a candidate (the first rows % cands have one more): candidate-major
        per[:rows % cands] += 1
        keep_row = np.repeat(np.arange(cands), per)
        kc = np.concatenate([np.sort(rng.permutation(Cn)[:n]) + 1 for n in per]).astype(np.int32)
        d_keep = dev(np.tile(keep_row.astype(np.int32), (B, 1)))
        d_kc = dev(np.tile(kc, (B, 1)))
        d_K = dev(np.full(B, rows, np.int32))
        bb, r2 = F.DeviceTensor.zeros((B, rows, 5)), F.DeviceTensor.zeros((B, rows, 4), np.float64)
        keep.append((d_keep, d_kc, d_K, bb, r2))

        def boxes(n, d_keep=d_keep, d_kc=d_kc, d_K=d_K, bb=bb, r2=r2, rows=rows):
            for _ in range(n):
                F._lib.call("frcnn_detect_class_boxes_batch", F.ptr(feat), nf, row0, B, F.ptr(W), F.ptr(b), Cn, F.ptr(rect), F.ptr(pick),
                            cands, F.ptr(d_kc), F.ptr(d_keep), F.ptr(d_K), rows, F.ptr(bb), F.ptr(r2), s)
        configs.append(("rows%d/class_boxes" % rows, boxes))

    def dense_fwd(n):
        for _ in range(n):
            F._lib.call("frcnn_linear_forward", F.ptr(feat), B * cands, nf, F.ptr(W), F.ptr(b), 4 * Cn, F.ptr(dense), s)

    def copies(n):
        for _ in range(n):
            for i in range(B):
                F._lib.call("frcnn_memcpy_d2d", C.c_void_p(copy_dst.ptr + 4 * i * cands * nf), C.c_void_p(feat.ptr + 4 * i * cands * nf),
                            4 * cands * nf, s)
    configs += [("dense/forward", dense_fwd), ("feature_copies", copies)]
    t = alternate(configs, args.calls)
    res = dict(metric="us per call, queued back to back (B = 8 frames of 1403 candidates, nf = 512, C = 16; rows: class rows a frame; dense "
                      "= frcnn_linear_forward to 11224 x 64; feature_copies = 8 device-to-device copies of 1403 x 512 floats)",
               calls=args.calls, rounds=args.rounds)
    for name, _ in configs:
        res[name] = dict(us=spread([v * 1e6 for v in t[name]]))
    return res


def detect():
    from detect_bench_model import amplified_vgg_small
    imgs = [F.to_device(F.synthetic_image(450, 800, i)) for i in range(4)]
    cfg0, base, w0, g0 = amplified_vgg_small(F, 30.0)
    # the same amplified weights on the longer vector: every class's rows are the shared head's four
    cfg = dict(cfg0, box_head=dict(per_class=True))
    per = F.vgg_small(cfg)
    wb = w0.cpu().numpy()
    (ow, nw, _, nf), (ob, nb, _, _) = (tuple(int(v) for v in r) for r in base["native"].param_table[-4:-2])
    Cn = cfg["class_count"]
    wp = np.concatenate([wb[:ow], np.tile(wb[ow:ob], Cn), np.tile(wb[ob:ob + nb], Cn), wb[ob + nb:]])
    weights, gradient = F.combine_and_flatten_parameters(per["pnet"], per["cnet"], weights_host=wp)
    dets = {}
    for c in (0.2, 0.05):
        for name, model, sc in (("shared/all@%g" % c, base, dict(classes="all", min_confidence=c)),
                                ("per_class/all@%g/boxes=class" % c, per, dict(classes="all", min_confidence=c, boxes="class"))):
            d = F.Detector(model, static_weights=True, scoring=sc)
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
        res[name] = dict(ms=spread([v * 1e3 for v in t[name]]), candidates=int(len(d.last_pick)), rows=int(d._last.get("kept", 0)))
    return res


print(json.dumps(detect() if args.detect else kernels()))
