"""Staged training: ms/step and launches/step of vgg_small at 800x450 for the default configuration and the four rows of
Faster R-CNN's 4-step alternating training (cfg.train).  RMSprop steps on one synthetic image per batch; the
launches are the library's own (frcnn_prof_collect over one extra step).
usage: python tools/bench_stages.py [--steps 20] [--warmup 5]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [
    ("default", None),
    ("1 train RPN", dict(proposal=True, classification=False, frozen_blocks=0)),
    ("2 train detector", dict(proposal=False, classification=True, frozen_blocks=0)),
    ("3 fixed trunk, RPN", dict(proposal=True, classification=False, frozen_blocks=-1)),
    ("4 fixed trunk, detector", dict(proposal=False, classification=True, frozen_blocks=-1)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import frcnn_amd as F
    F._lib.call("frcnn_set_device", 0)
    nk = len(F._lib.KC_NAMES)
    print("%-26s %10s %16s" % ("configuration", "ms/step", "launches/step"))
    for name, train in ROWS:
        model = F.vgg_small(dict(F.duplo_cfg))
        w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=1)
        it = F.SyntheticBatchIterator(model, H=450, W=800, pool=4)
        f = F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
        if train is not None:
            train = dict(train)
            if train["frozen_blocks"] < 0:
                train["frozen_blocks"] = len(model["layers"])
            model["cfg"]["train"] = train
        state = dict(learningRate=1e-5)
        for _ in range(a.warmup):
            F.rmsprop(f, w, state)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            F.rmsprop(f, w, state)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        la = (C.c_longlong * nk)(); t = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
        F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
        F.rmsprop(f, w, state)
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, t, fl, by)
        print("%-26s %10.3f %16d" % (name, ms, sum(la)), flush=True)


if __name__ == "__main__":
    main()
