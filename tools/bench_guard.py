"""The cost of the gradient guard (state["clipNorm"] / state["skipNonFinite"]) in the default training step: ms/step of
F.rmsprop / F.sgd / F.nag on vgg_small at 450x800 with the guard off and on, the two alternated inside one process on one device
(windows of --steps steps each, --rounds of them per setting; medians and the spread of the windows are printed).
python tools/bench_guard.py [--opti rmsprop] [--steps 200] [--rounds 5] [--clip-norm 0] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import frcnn_amd as F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opti", default="rmsprop", choices=["rmsprop", "sgd", "nag"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height", type=int, default=450)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--clip-norm", type=float, default=0.0, help="0: skipNonFinite only (the norm is recorded, nothing clipped)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_guard.py needs a HIP device")
    F._lib.call("frcnn_set_device", 0)
    model = F.vgg_small(dict(F.duplo_cfg))
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    it = F.SyntheticBatchIterator(model, H=a.height, W=a.width, images_per_batch=1, pool=4)
    stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
    f = F.create_objective(model, weights, gradient, it, stats)
    base = dict(learningRate=1e-4, alpha=0.9) if a.opti == "rmsprop" else dict(learningRate=1e-4, momentum=0.9)
    guard = dict(clipNorm=a.clip_norm) if a.clip_norm > 0 else dict(skipNonFinite=True)
    state = dict(base)          # one optimiser state for both settings: only the guard's keys come and go
    opt = F.optimizer(a.opti)

    def window(on):
        for k in guard:
            state.pop(k, None)
        if on:
            state.update(guard)
        for _ in range(5):
            opt(f, weights, state)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            opt(f, weights, state)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for _ in range(2 * len(it.pool)):   # every pooled image once per setting: no workspace grows inside a window
        window(bool(_ % 2))
    off, on = [], []
    for r in range(a.rounds):
        off.append(window(False))
        on.append(window(True))
        print("round %d: guard off %.4f ms/step, on %.4f ms/step" % (r, off[-1], on[-1]), flush=True)
    out = dict(opti=a.opti, steps=a.steps, rounds=a.rounds, guard=guard, height=a.height, width=a.width,
               off_ms=[round(v, 4) for v in off], on_ms=[round(v, 4) for v in on],
               off_median_ms=round(statistics.median(off), 4), on_median_ms=round(statistics.median(on), 4),
               extra_us_per_step=round((statistics.median(on) - statistics.median(off)) * 1e3, 1),
               gnorm_last=stats.get("gnorm", [float("nan")])[-1], skipped=stats.get("skipped", 0),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
