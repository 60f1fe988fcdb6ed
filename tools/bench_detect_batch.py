"""Detector.detect_batch against the detect() loop: ms per frame on synthetic 3x450x800 frames (vgg_small, BASELINE config 2).

Weights amplified as bench.py's inference leg (head logits x30, class head x200), option static_weights on, 4 resident
frames cycled.  Every configuration is warmed up (every shape it launches), then the configurations are ALTERNATED in this
one process (the detect() loop, detect_batch at every B, the same with shared_cnet=True), `--rounds` times; a measurement is `--frames` frames ending in a device synchronise.  Reported per
configuration: median and min-max of the rounds, in ms per frame.

  python tools/bench_detect_batch.py                       all configurations
  python tools/bench_detect_batch.py --only detect         the detect() loop alone (e.g. with FRCNN_LIB_PATH pointing at another
                                                           build of the library: the A/B leg against a parent build)
  python tools/bench_detect_batch.py --trace-chunks 23     no timing: 23 chunks of 8 through detect_batch (after a warm-up of 2
                                                           chunks), for a kernel trace taken from outside;
                                                           with --only detect: 23 * 8 frames through detect() instead

Prints one JSON line."""
import argparse
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
ap.add_argument("--frames", type=int, default=208, help="frames per measurement (>= 200; a multiple of 16)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batches", default="1,2,4,8,16")
ap.add_argument("--only", default="", help="'detect': the detect() loop alone")
ap.add_argument("--trace-chunks", type=int, default=0)
ap.add_argument("--gain", type=float, default=30.0)
ap.add_argument("--shared", action="store_true", help="with --trace-chunks: shared_cnet=True")
args = ap.parse_args()

cfg, model, weights, gradient = amplified_vgg_small(F, args.gain)
imgs = [F.to_device(F.synthetic_image(450, 800, i)) for i in range(4)]
has_batch = hasattr(F.Detector, "detect_batch")
batches = [int(b) for b in args.batches.split(",")] if has_batch and args.only != "detect" else []
det = F.Detector(model, static_weights=True)


def run_detect(n):
    for i in range(n):
        det.detect(imgs[i % 4])


def run_batch(n, B, shared=False):
    det.BATCH = B
    for lo in range(0, n, B):
        det.detect_batch([imgs[(lo + i) % 4] for i in range(min(B, n - lo))], shared_cnet=shared)


configs = [("detect", run_detect)] + [("batch%d" % B, (lambda n, B=B: run_batch(n, B))) for B in batches]
configs += [("shared%d" % B, (lambda n, B=B: run_batch(n, B, True))) for B in batches]
if args.trace_chunks:
    if args.only == "detect":
        run_detect(16 + 8 * args.trace_chunks)
    else:
        run_batch(16 + 8 * args.trace_chunks, 8, args.shared)
    torch.cuda.synchronize()
    print(json.dumps(dict(traced="detect" if args.only == "detect" else "detect_batch", frames=16 + 8 * args.trace_chunks)))
    sys.exit(0)
for name, fn in configs:      # warm-up: every shape, every buffer
    fn(32)
torch.cuda.synchronize()
ms = dict((name, []) for name, _ in configs)
for r in range(args.rounds):
    for name, fn in configs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(args.frames)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) / args.frames * 1e3)
res = dict(metric="ms per frame (vgg_small 800x450 inference)", frames=args.frames, rounds=args.rounds,
           library=os.path.basename(os.environ.get("FRCNN_LIB_PATH") or "libfrcnn_hip.so"))
det.detect(imgs[0])
res.update(matches=int(det.last_scan["n"]), candidates=int(len(det.last_pick)))
for name, _ in configs:
    v = sorted(ms[name])
    res[name] = dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4))
print(json.dumps(res))
