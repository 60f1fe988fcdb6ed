"""ROI pooling alone on the benchmarked shapes (384 x 29 x 50 map, 560 / 1398 windows, 6 x 6 cells): HIP-event time of the
forward and backward launches, effective bytes/s of the output they write -- the max pool (frcnn_roi_pool_*) and, beside it in
the same run, RoIAlign (frcnn_roi_align_*, 2 x 2 samples per bin) on input rects whose snapped windows are the max rows' windows.
python tools/bench_roi.py [R ...]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import frcnn_amd as F


def rects_of_windows(wins, H, W):
    """Input-space rects that extract_roi_pooling_input snaps to the given windows on vgg_small's last map (stride 16): the
    Localizer is walked for every integer input coordinate once, a window's four sides are looked up, the result is checked."""
    conv, pool = (3, 3, 1, 1, 1, 1), (2, 2, 2, 2, 0, 0)                  # {kW, kH, dW, dH, padW, padH}
    loc = F.Localizer([conv, pool] + 3 * [conv, conv, pool])             # vgg_small's path to its last map
    v = np.arange(-64, 16 * max(H, W) + 65, dtype=np.float64)
    big = 1e6
    lo = loc.inputToFeatureRectBatch(np.stack([v, v, v + big, v + big], 1))      # floor of the mapped minimum, per coordinate
    hi = loc.inputToFeatureRectBatch(np.stack([v - big, v - big, v, v], 1))      # ceil of the mapped maximum
    rects = np.zeros((len(wins), 4), np.float64)
    for r, (r_lo, r_hi, c_lo, c_hi) in enumerate(wins):
        for k, (first, last, n, col) in enumerate(((c_lo, c_hi, W, 0), (r_lo, r_hi, H, 1))):
            a = v[np.clip(lo[:, col], 0, n) == first - 1]
            b = v[np.clip(hi[:, 2 + col], 0, n) == last]
            rects[r, k], rects[r, 2 + k] = a[len(a) // 2], b[len(b) // 2]
    assert np.array_equal(F.roi_windows(rects, loc, H, W), wins), "the rects do not snap to the max rows' windows"
    return rects


def run(R, Cn=384, H=29, W=50, kh=6, kw=6, reps=10, sampling=2):
    rng = np.random.RandomState(R)
    fm = F.DeviceTensor.from_numpy(rng.randn(Cn, H, W).astype(np.float32))
    wins = np.zeros((R, 4), np.int32)
    for r in range(R):   # windows like the training examples' : 6..29 rows, 6..50 columns
        h, w = rng.randint(6, H + 1), rng.randint(6, W + 1)
        y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        wins[r] = (y0 + 1, y0 + h, x0 + 1, x0 + w)
    dw = F.DeviceTensor.from_numpy(wins)
    dr = F.DeviceTensor.from_numpy(rects_of_windows(wins, H, W))
    out = F.DeviceTensor.empty((R, Cn * kh * kw)); idx = F.DeviceTensor.empty((R, Cn * kh * kw), np.int32)
    g = F.DeviceTensor.from_numpy(rng.randn(R, Cn * kh * kw).astype(np.float32)); gm = F.DeviceTensor.zeros((Cn, H, W))
    s = F.stream_ptr()
    k = F._lib.KC_NAMES.index("roi")
    nk = len(F._lib.KC_NAMES)
    for name, fn in (("forward", lambda: F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), Cn, H, W, F.ptr(dw), R, kh, kw, F.ptr(out), F.ptr(idx), s)),
                     ("forward (no indices)", lambda: F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), Cn, H, W, F.ptr(dw), R, kh, kw, F.ptr(out), None, s)),
                     ("backward", lambda: F._lib.call("frcnn_roi_pool_backward", F.ptr(gm), Cn, H, W, F.ptr(g), F.ptr(idx), R, kh, kw, s)),
                     ("align forward", lambda: F._lib.call("frcnn_roi_align_forward", F.ptr(fm), Cn, H, W, F.ptr(dr), None, R, 1 / 16.0,
                                                           1 / 16.0, kh, kw, sampling, F.ptr(out), s)),
                     ("align backward", lambda: F._lib.call("frcnn_roi_align_backward", F.ptr(gm), Cn, H, W, F.ptr(g), F.ptr(dr), None, R,
                                                            1 / 16.0, 1 / 16.0, kh, kw, sampling, s))):
        fn()
        la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
        F._lib.call("frcnn_prof_enable", 1 << k)
        for _ in range(reps):
            fn()
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
        t = ms[k] / reps
        print("R=%-5d %-22s %7.1f us   %6.2f TB/s of algorithmic bytes (%.1f MB)" % (R, name, t * 1e3, by[k] / reps / 1e12 / (t * 1e-3), by[k] / reps / 1e6), flush=True)


if __name__ == "__main__":
    for R in [int(a) for a in sys.argv[1:]] or [560, 1398]:
        run(R)
