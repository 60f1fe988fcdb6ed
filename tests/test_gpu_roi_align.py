"""RoIAlign on the device (frcnn_roi_align_forward / _backward, cfg["roi_pooling"]["method"] = "align").

Op level, against the float64 reference of tests/roi_align_ref.py, with the bars of the issue:
  forward    |out - ref| <= 1e-5 max|fmap| (an fp32 sum of at most 4 g^2 + 2 rounded terms: (4 g^2 + 2) 2^-24 max|x| < 4e-6 for
             g <= 4); two runs bit-equal
  backward   per element |gmap - ref| <= max(n, 1) 2^-23 A, n the reference's term count and A its sum of |term| at that element
             -- the worst-case bound of an fp32 sum in any order.  gmap starts from a non-zero map, which is one of the terms the
             device adds up (roi_align_ref.backward); elements no sample touches are exactly unchanged.  Deterministic mode: the
             same bar, two runs bit-equal
  adjoint    <forward(x), g> against <x, backward(g)>, both accumulated in float64 on the host, within the sum of the two bars
Every case asserts that none of its samples lies within 1e-6 of a discontinuity of the sampling rule (a condition on the inputs:
the rects are drawn from continuous distributions with fixed seeds).

Wiring: the objective, the Detector and validation_losses under "align", and "max" given explicitly against the key absent."""
import ctypes as C
import functools

import numpy as np
import pytest

import roi_align_ref as ref
from test_gpu_optim import _host, _masks, same_bits

pytestmark = pytest.mark.gpu

S = 16.0                      # the stride of both models' last map
INV = 1.0 / S
SHAPES = [(5, 3, 5), (3, 1, 1), (8, 29, 50), (2, 130, 130),     # 2 x 130 x 130: a plane larger than the 64 KB LDS path
          (257, 3, 5)]                                          # beside the issue's: enough channels for two planes per workgroup, odd
GRIDS = [(6, 6), (7, 7), (1, 1), (2, 3)]
RATIOS = [1, 2, 3]
# every shape with every grid, the sampling ratios cycling so that every shape and every grid sees each of them
EDGE_CASES = [("edges", si, gi, RATIOS[(si + gi) % 3]) for si in range(4) for gi in range(len(GRIDS))]
EXTRA_CASES = [("edges", 0, 3, 3), ("edges", 2, 0, 1), ("edges", 2, 1, 2), ("edges", 3, 3, 2),
               ("one", 2, 0, 2), ("one", 1, 2, 3), ("pick", 0, 0, 2), ("pick", 2, 3, 3), ("pick", 3, 1, 1),
               ("overlap", 2, 3, 2), ("overlap", 3, 2, 3), ("overlap", 0, 0, 1),
               ("edges", 4, 3, 2), ("overlap", 4, 2, 3)]
CASES = EDGE_CASES + EXTRA_CASES


def _feat(x0, y0, x1, y1):
    return np.array([x0 * S, y0 * S, x1 * S, y1 * S], np.float64)


def _edge_rects(rng, H, W):
    """inside the map, hanging over each side (samples between -1 and 0 clamp, samples beyond contribute 0), wholly outside,
    zero width, zero height, the whole map, smaller than one cell, and a few at random -- feature coordinates times the stride"""
    u = rng.uniform
    x0, y0 = u(0.1, 0.45) * W, u(0.1, 0.45) * H
    out = [_feat(x0, y0, x0 + u(0.2, 0.5) * W, y0 + u(0.2, 0.5) * H),                 # inside
           _feat(-u(1.6, 3.0), u(0, 0.3) * H, u(0.4, 0.9) * W, u(0.5, 1.0) * H),      # over the left side
           _feat(u(0.1, 0.5) * W, u(0, 0.3) * H, W + u(1.6, 3.0), u(0.5, 1.0) * H),   # right
           _feat(u(0, 0.3) * W, -u(1.6, 3.0), u(0.5, 1.0) * W, u(0.4, 0.9) * H),      # top
           _feat(u(0, 0.3) * W, u(0.1, 0.5) * H, u(0.5, 1.0) * W, H + u(1.6, 3.0)),   # bottom
           _feat(W + u(3, 4), H + u(3, 4), W + u(5, 7), H + u(5, 7)),                 # wholly outside
           _feat(-u(9, 12), -u(9, 12), -u(4, 6), -u(4, 6)),
           np.array([0.0, 0.0, W * S, H * S]),                                       # the whole map
           ]
    x0, y0 = u(0.2, 0.8) * W, u(0.2, 0.8) * H
    out.append(_feat(x0, y0, x0, y0 + u(0.1, 0.5) * H))                               # zero width
    out.append(_feat(x0, y0, x0 + u(0.1, 0.5) * W, y0))                               # zero height
    out.append(_feat(x0, y0, x0, y0))                                                 # both
    out.append(_feat(x0, y0, x0 + u(0.1, 0.6), y0 + u(0.1, 0.6)))                     # smaller than one cell
    out.append(_feat(x0 + 1.0, y0, x0, y0 + 1.0))                                     # maxX < minX: width clamps to zero
    for _ in range(3):
        xa, xb = np.sort(u(-2.0, W + 2.0, 2)); ya, yb = np.sort(u(-2.0, H + 2.0, 2))
        out.append(_feat(xa, ya, xb, yb))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _case(kind, si, gi, g):
    """inputs and float64 reference of one case, computed once and shared by the tests (never modified)"""
    Cn, H, W = SHAPES[si]
    kh, kw = GRIDS[gi]
    rng = np.random.RandomState(1000 * si + 100 * gi + 10 * g + len(kind))
    pick = None
    if kind == "edges":
        rects = _edge_rects(rng, H, W)
    elif kind == "one":
        rects = _edge_rects(rng, H, W)[:1]
    elif kind == "pick":
        rects = _edge_rects(rng, H, W)[:10]
        pick = np.array([7, 2, 10, 3], np.int64)        # 4 of 10 rows, out of order
    else:                                               # 300 heavily overlapping rects around the middle of the map
        u = rng.uniform
        cx, cy = u(0.46, 0.54, 300) * W, u(0.46, 0.54, 300) * H
        hw, hh = u(0.02, 0.1, 300) * W + 0.3, u(0.02, 0.1, 300) * H + 0.3
        rects = np.stack([(cx - hw) * S, (cy - hh) * S, (cx + hw) * S, (cy + hh) * S], 1)
    R = len(rects) if pick is None else len(pick)
    fmap = rng.randn(Cn, H, W).astype(np.float32)
    gout = rng.randn(R, Cn * kh * kw).astype(np.float32)
    gmap0 = rng.randn(Cn, H, W).astype(np.float32)
    gmap0[np.abs(gmap0) < 1e-3] = 1.0                                     # "starts from a non-zero map"
    near = ref.near_discontinuities(rects, H, W, kh, kw, g, S, S, pick)
    out = ref.forward(fmap, rects, kh, kw, g, S, S, pick)
    gm_zero, count_zero, abs_zero = ref.backward(gout, rects, (Cn, H, W), kh, kw, g, S, S, pick)
    # the same into the non-zero map (what roi_align_ref.backward(..., gmap0) returns, without walking the samples again)
    gm, count, abs_sum = gm_zero + gmap0.astype(np.float64), count_zero + 1, abs_zero + np.abs(gmap0.astype(np.float64))
    for a in (rects, fmap, gout, gmap0, out, gm, count, abs_sum, gm_zero, count_zero, abs_zero):
        a.setflags(write=False)
    return dict(C=Cn, H=H, W=W, kh=kh, kw=kw, g=g, rects=rects, pick=pick, R=R, fmap=fmap, gout=gout, gmap0=gmap0, near=near, out=out,
                gm=gm, count=count, abs_sum=abs_sum, gm_zero=gm_zero, count_zero=count_zero, abs_zero=abs_zero)


def _forward(F, c, fmap=None, guard=64):
    """-> the R x D rows; a guard tail behind them must stay untouched"""
    fm = F.DeviceTensor.from_numpy(c["fmap"] if fmap is None else fmap)
    rect = F.DeviceTensor.from_numpy(c["rects"])
    pick = F.DeviceTensor.from_numpy(c["pick"]) if c["pick"] is not None else None
    D = c["C"] * c["kh"] * c["kw"]
    out = F.DeviceTensor.from_numpy(np.full(c["R"] * D + guard, -77.0, np.float32))
    F._lib.call("frcnn_roi_align_forward", F.ptr(fm), c["C"], c["H"], c["W"], F.ptr(rect), F.ptr(pick), c["R"], INV, INV, c["kh"], c["kw"],
                c["g"], F.ptr(out), F.stream_ptr())
    got = out.numpy()
    assert np.all(got[c["R"] * D:] == -77.0), "stores behind the last row"
    return got[:c["R"] * D].reshape(c["R"], D)


def _backward(F, c, gmap0, det):
    gm = F.DeviceTensor.from_numpy(gmap0)
    g = F.DeviceTensor.from_numpy(c["gout"])
    rect = F.DeviceTensor.from_numpy(c["rects"])
    pick = F.DeviceTensor.from_numpy(c["pick"]) if c["pick"] is not None else None
    F._lib.call("frcnn_set_option", b"deterministic", int(det))
    try:
        F._lib.call("frcnn_roi_align_backward", F.ptr(gm), c["C"], c["H"], c["W"], F.ptr(g), F.ptr(rect), F.ptr(pick), c["R"], INV, INV,
                    c["kh"], c["kw"], c["g"], F.stream_ptr())
        return gm.numpy()
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)


def _ids(cases):
    return ["%s-%dx%dx%d-%dx%d-g%d" % ((k,) + SHAPES[si] + GRIDS[gi] + (g,)) for k, si, gi, g in cases]


def _forward_bar(c):
    return 1e-5 * float(np.abs(c["fmap"]).max())


def _backward_bar(count, abs_sum):
    return np.maximum(count, 1) * 2.0 ** -23 * abs_sum


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_forward(F, case):
    c = _case(*case)
    assert c["near"] == 0, "a sample within 1e-6 of a discontinuity: choose another seed"
    got = _forward(F, c)
    err = float(np.abs(got - c["out"]).max())
    print("forward %s: max error %.3g, bar %.3g" % (case, err, _forward_bar(c)))
    assert err <= _forward_bar(c)
    assert same_bits(got, _forward(F, c)), "two forward runs differ"
    if case[0] == "edges":
        assert not np.any(got[5]) and not np.any(got[6]), "a rect wholly outside the map must pool to zeros"


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_backward(F, case, det):
    c = _case(*case)
    assert c["near"] == 0, "a sample within 1e-6 of a discontinuity: choose another seed"
    got = _backward(F, c, c["gmap0"], det)
    err = np.abs(got - c["gm"])
    bar = _backward_bar(c["count"], c["abs_sum"])
    worst = float((err / bar).max())
    print("backward %s det=%d: worst error / bar %.3g, most terms %d" % (case, det, worst, int(c["count"].max())))
    assert np.all(err <= bar), "worst error / bar %.3g" % worst
    untouched = c["count"] == 1        # (the initial map is the element's only term)
    assert same_bits(got[untouched], c["gmap0"][untouched]), "an element no sample touches has changed"
    if case[0] == "overlap":
        assert int(c["count"].max()) > 50, "the rects do not pile up"
    if det:
        assert same_bits(got, _backward(F, c, c["gmap0"], 1)), "two deterministic backward runs differ"


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", EXTRA_CASES + EDGE_CASES[::3], ids=_ids(EXTRA_CASES + EDGE_CASES[::3]))
def test_adjoint_on_the_device(F, case, det):
    c = _case(*case)
    out = _forward(F, c).astype(np.float64)
    gm = _backward(F, c, np.zeros_like(c["gmap0"]), det).astype(np.float64)
    lhs = float(np.sum(out * c["gout"].astype(np.float64)))
    rhs = float(np.sum(c["fmap"].astype(np.float64) * gm))
    bar = (_forward_bar(c) * float(np.abs(c["gout"]).sum())
           + float(np.sum(np.abs(c["fmap"]).astype(np.float64) * _backward_bar(c["count_zero"], c["abs_zero"]))))
    print("adjoint %s det=%d: %.9g vs %.9g, bar %.3g" % (case, det, lhs, rhs, bar))
    assert abs(lhs - rhs) <= bar


def test_wholly_outside_gives_zero_gradient(F):
    c = dict(_case("edges", 2, 0, 1))
    far = np.array([[-900.0, -700.0, -500.0, -300.0], [50 * S + 80, 29 * S + 80, 50 * S + 300, 29 * S + 200]])
    c.update(rects=far, R=2, gout=np.ones((2, c["C"] * 36), np.float32), pick=None)
    for det in (0, 1):
        assert same_bits(_backward(F, c, c["gmap0"], det), c["gmap0"])
    assert not np.any(_forward(F, c))


def test_no_rois_no_launch(F):
    """R = 0: FRCNN_OK, nothing launched, nothing written"""
    nk = len(F._lib.KC_NAMES)
    k = F._lib.KC_NAMES.index("roi")
    out = F.DeviceTensor.from_numpy(np.full(64, 3.0, np.float32))
    gm = F.DeviceTensor.from_numpy(np.full(5 * 3 * 5, 2.0, np.float32))
    fm = F.DeviceTensor.zeros((5, 3, 5)); rect = F.DeviceTensor.zeros((1, 4), np.float64)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    F._lib.call("frcnn_prof_enable", 1 << k)
    try:
        for R in (0, -3):
            F._lib.call("frcnn_roi_align_forward", F.ptr(fm), 5, 3, 5, F.ptr(rect), None, R, INV, INV, 6, 6, 2, F.ptr(out), F.stream_ptr())
            F._lib.call("frcnn_roi_align_backward", F.ptr(gm), 5, 3, 5, F.ptr(out), F.ptr(rect), None, R, INV, INV, 6, 6, 2, F.stream_ptr())
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    assert la[k] == 0
    assert np.all(out.numpy() == 3.0) and np.all(gm.numpy() == 2.0)


def test_bad_arguments_are_refused(F):
    fm = F.DeviceTensor.zeros((5, 3, 5)); rect = F.DeviceTensor.zeros((1, 4), np.float64); out = F.DeviceTensor.zeros((5 * 36,))
    for g in (0, 5):
        with pytest.raises(F.FrcnnError):
            F._lib.call("frcnn_roi_align_forward", F.ptr(fm), 5, 3, 5, F.ptr(rect), None, 1, INV, INV, 6, 6, g, F.ptr(out), F.stream_ptr())
        with pytest.raises(F.FrcnnError):
            F._lib.call("frcnn_roi_align_backward", F.ptr(fm), 5, 3, 5, F.ptr(out), F.ptr(rect), None, 1, INV, INV, 6, 6, g, F.stream_ptr())
    with pytest.raises(F.FrcnnError):
        F._lib.call("frcnn_roi_align_forward", F.ptr(fm), 5, 3, 5, None, None, 1, INV, INV, 6, 6, 2, F.ptr(out), F.stream_ptr())


def test_grid_of_more_than_256_bins(F):
    """kh kw > 256: the generic forward kernel (the backward pass has one form for every grid)"""
    rng = np.random.RandomState(3)
    Cn, H, W, kh, kw, g = 2, 9, 11, 17, 16, 2
    rects = _edge_rects(rng, H, W)[:8]
    c = dict(C=Cn, H=H, W=W, kh=kh, kw=kw, g=g, rects=rects, pick=None, R=len(rects), fmap=rng.randn(Cn, H, W).astype(np.float32),
             gout=rng.randn(len(rects), Cn * kh * kw).astype(np.float32))
    assert ref.near_discontinuities(rects, H, W, kh, kw, g, S, S) == 0
    got = _forward(F, c)
    assert np.abs(got - ref.forward(c["fmap"], rects, kh, kw, g, S, S)).max() <= _forward_bar(c)
    assert same_bits(got, _forward(F, c))
    gm0 = rng.randn(Cn, H, W).astype(np.float32)
    want, count, abs_sum = ref.backward(c["gout"], rects, (Cn, H, W), kh, kw, g, S, S, None, gm0)
    for det in (0, 1):
        assert np.all(np.abs(_backward(F, c, gm0, det) - want) <= _backward_bar(count, abs_sum))


# ------------------------------------------------------------------------------------------------ wiring: the objective
HI, WI = 225, 400
ALIGN = dict(kw=6, kh=6, method="align", sampling_ratio=2)


def _objective(F, roi_pooling, train=None, seed=11):
    cfg = dict(F.duplo_cfg)
    if roi_pooling is not None:
        cfg["roi_pooling"] = dict(roi_pooling)
    if train is not None:
        cfg["train"] = dict(train)
    model = F.vgg_small(cfg)
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=seed)
    it = F.SyntheticBatchIterator(model, H=HI, W=WI, pool=2)
    stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
    return model, w, g, it, F.create_objective(model, w, g, it, stats), stats


def _one_step(F, roi_pooling, train=None, profile=False):
    """one deterministic step with explicit dropout masks (tests/test_gpu_stages.py) -> dict(g, model, f, w, it, launches)"""
    import torch
    model, w, g, it, f, stats = _objective(F, roi_pooling, train)
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    if profile:
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
        F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        _masks(F, model, it, 0, HI, WI, np.random.RandomState(5))
        loss, _ = f(w)
        torch.cuda.synchronize()
    finally:
        if profile:
            F._lib.call("frcnn_prof_enable", 0)
            F._lib.call("frcnn_prof_collect", la, ms, fl, by)
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    return dict(g=_host(g).copy(), model=model, f=f, w=w, gt=g, it=it, launches=list(la), loss=loss, stats=stats)


def _groups(model):
    pnet = model["pnet"]
    out = {"block%d" % (b + 1): pnet.block_param_range(b) for b in range(4)}
    out["heads"] = pnet.heads_param_range()
    out["cnet"] = (int(model["native"].pnet_params), int(model["native"].total_params))
    return out


def test_explicit_max_equals_the_key_absent(F):
    a = _one_step(F, None, profile=True)
    b = _one_step(F, dict(kw=6, kh=6, method="max"), profile=True)
    assert same_bits(a["g"], b["g"])
    assert a["launches"] == b["launches"], "launches per class differ: %r vs %r" % (a["launches"], b["launches"])
    assert a["loss"] == b["loss"]


def test_objective_forward_wiring_under_align(F):
    r = _one_step(F, ALIGN)
    model, f = r["model"], r["f"]
    E = f.debug["E"]
    rects = f.debug["rects"]
    assert E > 0 and rects.shape == (E, 4) and rects.dtype == np.float64
    # the proposal net's last output for that image: the same forward pass again (explicit dropout masks)
    _masks(F, model, r["it"], 0, HI, WI, np.random.RandomState(5))
    model["pnet"].training()
    fm = model["pnet"].forward(F.to_device(r["it"].pool[0]["img"]))[-1].numpy()
    model["pnet"].drop_masks = None; model["cnet"].drop_masks = None
    Cn, H, W = fm.shape
    cinput = f.debug["scratch"].get("cinput", (E, Cn * 36)).numpy()
    assert "pidx" not in f.debug["scratch"].bufs, "the index tensor of the max pool is allocated under align"
    # every row is compared, rows with a sample ON a discontinuity included (the examples' rects sit on round coordinates): the
    # device and the reference do the same double operations in the same order, and 1 / 16 is exact
    want = ref.forward(fm, rects, 6, 6, 2, S, S)
    assert np.abs(cinput - want).max() <= 1e-5 * np.abs(fm).max()
    assert np.all(np.isfinite(r["g"]))
    for name, (lo, hi) in _groups(model).items():
        assert np.any(r["g"][lo:hi]), "%s: no gradient" % name
    assert all(np.isfinite(v[-1]) for v in r["stats"].values())


def test_objective_backward_wiring_under_align(F):
    """proposal = false, classification = true, frozen_blocks = 0: the backbone's gradient comes through the ROI backward alone.
    The same pass composed by hand over the Python surface (pnet.forward, the align forward, cnet.forward / frcnn_cnet_losses /
    cnet.backward, the align backward into a zeroed map, pnet.backward, the objective's gradient:div) gives the backbone slices of
    the objective's gradient bit for bit in deterministic mode: both compositions queue the same launches on the same inputs
    (the regression targets are taken from the objective's own anchor-loss stage, which is not under test here)."""
    import torch
    train = dict(proposal=False, classification=True, frozen_blocks=0)
    r = _one_step(F, ALIGN, train)
    model, f, w, g, it = r["model"], r["f"], r["w"], r["gt"], r["it"]
    pnet, cnet, nat = model["pnet"], model["cnet"], model["native"]
    E = f.debug["E"]
    rects = f.debug["rects"].copy()
    x = it.pool[0]
    npos = len(F.clean_examples(x["positive"], F.output_map_sizes(model, HI, WI)))
    sc = f.debug["scratch"]
    crtarget = F.DeviceTensor.from_numpy(sc.get("crtarget", (E, 4)).numpy())
    cctarget = F.DeviceTensor.from_numpy(sc.get("cctarget", (E,)).numpy())
    s = F.stream_ptr()
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        _masks(F, model, it, 0, HI, WI, np.random.RandomState(5))
        F._lib.call("frcnn_model_set_trainable", nat.h, 0, 0, 1)
        F._lib.call("frcnn_zero", F.ptr(g), g.numel() * 4, s)
        pnet.training(); cnet.training()
        img = F.to_device(x["img"])
        outputs = pnet.forward(img)
        deltas = pnet.delta_outputs(zero=True)
        fm = outputs[-1]
        Cn, H, W = fm.shape
        drect = F.DeviceTensor.from_numpy(rects)
        cinput = F.DeviceTensor.empty((E, Cn * 36))
        F._lib.call("frcnn_roi_align_forward", F.ptr(fm), Cn, H, W, F.ptr(drect), None, E, INV, INV, 6, 6, 2, F.ptr(cinput), s)
        crout, ccout = cnet.forward(cinput)
        crdelta = F.DeviceTensor.empty((E, 4)); ccdelta = F.DeviceTensor.empty((E, 17))
        acc = torch.zeros(8, dtype=torch.float64, device="cuda")
        F._lib.call("frcnn_cnet_losses", F.ptr(crout), F.ptr(crtarget), F.ptr(ccout), F.ptr(cctarget), E, npos, 17, F.ptr(crdelta),
                    F.ptr(ccdelta), C.c_void_p(acc.data_ptr() + 32), s)
        gx = cnet.backward(cinput, [crdelta, ccdelta])
        F._lib.call("frcnn_roi_align_backward", F.ptr(deltas[4]), Cn, H, W, F.ptr(gx), F.ptr(drect), None, E, INV, INV, 6, 6, 2, s)
        for l in range(4):
            F._lib.call("frcnn_pnet_set_sparse_deltas", nat.h, l + 1, None, 0)
        pnet.backward(img, deltas)
        cnet.join_backward()
        F._lib.call("frcnn_scale", F.ptr(g), g.numel(), 1.0 / E, s)
        torch.cuda.synchronize()
        hand = _host(g).copy()
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        F._lib.call("frcnn_model_set_trainable", nat.h, 0, 1, 1)
        pnet.drop_masks = None; cnet.drop_masks = None
    for name, (lo, hi) in _groups(model).items():
        if name.startswith("block"):
            assert np.any(r["g"][lo:hi]), name
            assert same_bits(hand[lo:hi], r["g"][lo:hi]), "%s: rel. L2 difference %.3g" % (
                name, np.linalg.norm(hand[lo:hi] - r["g"][lo:hi]) / np.linalg.norm(r["g"][lo:hi]))
    lo, hi = _groups(model)["heads"]
    assert not np.any(r["g"][lo:hi])


def test_trunk_frozen_skips_the_align_backward(F):
    """frozen_blocks = all: no ROI backward is queued (one ROI-class launch, the forward), the backbone slices stay zero"""
    k = F._lib.KC_NAMES.index("roi")
    r = _one_step(F, ALIGN, dict(proposal=False, classification=True, frozen_blocks=4), profile=True)
    assert r["launches"][k] == 1
    for name, (lo, hi) in _groups(r["model"]).items():
        assert np.any(r["g"][lo:hi]) == (name == "cnet"), name
    full = _one_step(F, ALIGN, dict(proposal=False, classification=True, frozen_blocks=0), profile=True)
    assert full["launches"][k] == 2


def test_align_on_a_backbone_that_is_not_centred_is_refused(F, monkeypatch):
    monkeypatch.setattr(F.Localizer, "centred", lambda self: False)
    with pytest.raises(ValueError):
        _objective(F, ALIGN)
    cfg = dict(F.duplo_cfg); cfg["roi_pooling"] = dict(ALIGN)
    with pytest.raises(ValueError):
        F.Detector(F.vgg_small(cfg))


# ------------------------------------------------------------------------------------------------ wiring: the Detector
@pytest.fixture(scope="module")
def detect_setup(F):
    from test_gpu_detect_batch import _amplified_weights
    import torch
    out = {}
    for key, rp in (("max", None), ("align", ALIGN)):
        cfg = dict(F.duplo_cfg)
        if rp is not None:
            cfg["roi_pooling"] = dict(rp)
        model = F.vgg_small(cfg)
        weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
        wamp = _amplified_weights(model["native"], weights.cpu().numpy().copy(), 17, cls_gain=200.0)
        weights.copy_(torch.from_numpy(wamp))
        out[key] = dict(model=model, weights=weights, gradient=gradient)
    return out


def _roi_launches(F, fn):
    nk = len(F._lib.KC_NAMES)
    k = F._lib.KC_NAMES.index("roi")
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    F._lib.call("frcnn_prof_enable", 1 << k)
    try:
        res = fn()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return res, int(la[k])


def test_detector_under_align(F, detect_setup, monkeypatch):
    from test_gpu_detect_batch import _assert_same, _detect_reference, _frames
    model = detect_setup["align"]["model"]
    frames = _frames(F, range(5, 11))
    want = _detect_reference(F, model, frames)
    with_rows = [b for b, r in enumerate(want) if r["n"] > 0 and len(r["pick"]) > 0]
    assert with_rows, "no frame has candidates"
    # no window kernel: frcnn_roi_windows is never called, and a frame queues ONE launch of the ROI class (the align forward)
    real = F._lib.call
    called = []
    monkeypatch.setattr(F._lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    d = F.Detector(model)
    got, launches = _roi_launches(F, lambda: d.detect_batch(frames))
    assert "frcnn_roi_windows" not in called and "frcnn_roi_pool_forward" not in called
    assert called.count("frcnn_roi_align_forward") == launches == len(with_rows)
    _assert_same(d.last_batch, got, want, "detect_batch")          # bit for bit the detect() loop
    d1 = F.Detector(model)
    _, one = _roi_launches(F, lambda: d1.detect(frames[with_rows[0]]))
    assert one == 1
    # shared_cnet: the pooled rows are the reference applied to the frame's last feature map and rect[pick - 1]
    d2 = F.Detector(model)
    d2.detect_batch(frames, shared_cnet=True)
    pnet = model["pnet"]
    checked = 0
    for b in with_rows:
        rec = d2.last_batch[b]
        pooled = rec["pooled"]
        pick = rec["pick"]
        assert pooled is not None and pooled.shape[0] == len(pick)
        pnet.evaluate()
        fm = pnet.forward(F.to_device(frames[b]))[-1].numpy()
        Cn, H, W = fm.shape
        rows = pick[:12]                                   # (the reference is a plain loop: a dozen rows a frame, all compared)
        ref_rows = ref.forward(fm, rec["rect"], 6, 6, 2, S, S, rows)
        assert np.abs(pooled[:len(rows)] - ref_rows).max() <= 1e-5 * np.abs(fm).max(), "frame %d" % b
        checked += len(rows)
    assert checked > 0


def test_detector_under_max_is_unchanged(F, detect_setup):
    """the key absent and "max" given explicitly: the same frames give the same records bit for bit, through the window kernel and
    the max pool (two launches of the ROI class a frame with candidates)"""
    from test_gpu_detect_batch import _assert_same, _detect_reference, _frames
    model = detect_setup["max"]["model"]
    frames = _frames(F, range(5, 9))
    want = _detect_reference(F, model, frames)
    with_rows = [b for b, r in enumerate(want) if r["n"] > 0 and len(r["pick"]) > 0]
    assert with_rows
    model["cfg"]["roi_pooling"] = dict(kw=6, kh=6, method="max")
    try:
        d = F.Detector(model)
        got, launches = _roi_launches(F, lambda: d.detect_batch(frames))
    finally:
        model["cfg"]["roi_pooling"] = dict(kw=6, kh=6)
    assert launches == 2 * len(with_rows)
    _assert_same(d.last_batch, got, want, "explicit max")
    # ... and differ from the align features on the same weights (the switch is live)
    da = F.Detector(detect_setup["align"]["model"])
    da.detect_batch(frames, shared_cnet=True)
    dm = F.Detector(model)
    dm.detect_batch(frames, shared_cnet=True)
    b = with_rows[0]
    assert np.array_equal(da.last_batch[b]["pick"], dm.last_batch[b]["pick"])
    assert not np.array_equal(da.last_batch[b]["pooled"], dm.last_batch[b]["pooled"])


def test_validation_losses_under_align(F):
    cfg = dict(F.duplo_cfg); cfg["roi_pooling"] = dict(ALIGN)
    model = F.vgg_small(cfg)
    F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=3)
    from test_gpu_eval import _Val
    items = [dict(img=F.synthetic_image(128, 176, 40 + k), rois=F.synthetic_rois(cfg, 176, 128, 3, 7, 40 + k)) for k in range(2)]
    res = F.validation_losses(model, _Val(F.Anchors(model["pnet"], cfg["scales"]), items), 2)
    assert res["images"] == 2 and res["examples"] > 0
    for k in ("pcls", "preg", "dcls", "dreg"):
        assert np.isfinite(res[k]), (k, res[k])
