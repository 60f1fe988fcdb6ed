"""bench.py's `other_legs` without the rest of `bench.py --full`: the `nms` leg (nms() at n = 300 / 2 000 / 6 000 / 26 544) and
the `inference` leg (Detector:detect), through bench.py's own functions, imported unmodified, with the model set up as its
main() does.  The CPU restatement is left out.  For A/B runs of two trees: one fresh process per tree and round.

  python tools/bench_other_legs.py                  both legs
  python tools/bench_other_legs.py --legs nms       the nms leg alone

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import frcnn_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="nms,inference")
legs = ap.parse_args().legs.split(",")
F._lib.load()
F._lib.call("frcnn_set_device", 0)
out = dict(library=os.path.relpath(F._lib.SO_PATH, ROOT))
if "nms" in legs:
    out["nms"] = bench.nms_leg(F, False)
if "inference" in legs:
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w0 = model["native"].init_parameters(42)
    bn0 = np.concatenate([np.zeros(1024, np.float32), np.ones(1024, np.float32)])
    out["inference"] = bench.inference_leg(F, cfg, model, weights, w0, bn0, False)
print(json.dumps(out))
