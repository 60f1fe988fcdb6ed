"""ROI max pooling on the device (frcnn_roi_pool_forward / _backward, csrc/roi.hip) op by op, against the numpy reference of
tests/roi_pool_ref.py on its case tables (tests/test_roi_pool_host.py: the reference equals the oracle bit for bit, the tables
reach every branch of roi.hip more than once, the "ties" maps tie, every window lies inside its map).

  forward    out and idx equal the reference exactly (a gather of existing values; the first maximum in row-major order wins, which
             the "ties", "constant" and ramp maps pin); two runs bit-equal; a guard tail of 64 elements behind out and behind idx
             untouched; idx = NULL (the Detector's call): the same out, nothing else written; R = 0: OK, nothing launched or written
  backward   default mode and option "deterministic", fed the REFERENCE's idx (the two ops are tested independently) with rows of
             idx = -1 and exact zeros in gout, into a non-zero map.  Per element |gmap - ref| <= max(n, 1) 2^-23 A, n the number
             of terms of that element's sum (the initial map is one of them) and A the sum of their magnitudes: the worst-case
             bound of an fp32 sum in any order.  Deterministic mode: n 2^-45 more (every term is rounded to a multiple of 2^-44,
             csrc/roi_fix.h), two runs bit-equal.  Elements no term touches are bit-identical to the initial map; a guard tail
             behind gmap is untouched
  wiring     one objective step of the narrow model with a 3 x 5 grid against the oracle: kh and kw swapped anywhere between
             roi_pooling_settings, the launches, D and the classification net's first Linear fail it"""
import ctypes as C

import numpy as np
import pytest

import roi_pool_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
IDS = [ref.case_id(c) for c in ref.CASES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _forward(F, c, with_idx=True):
    """-> (out, idx or None); the guard tails behind both must stay untouched, and so must the inputs"""
    wins = ref.check_windows(c["wins"], c["H"], c["W"])          # a window outside the map is an out-of-bounds read
    n = c["R"] * c["D"]
    fm = F.DeviceTensor.from_numpy(c["fmap"])
    dw = F.DeviceTensor.from_numpy(wins)
    out = F.DeviceTensor.from_numpy(np.full(n + GUARD, -77.0, np.float32))
    idx = F.DeviceTensor.from_numpy(np.full(n + GUARD, -7777, np.int32)) if with_idx else None
    F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), c["C"], c["H"], c["W"], F.ptr(dw), c["R"], c["kh"], c["kw"], F.ptr(out), F.ptr(idx),
                F.stream_ptr())
    got = out.numpy()
    assert np.all(got[n:] == -77.0), "stores behind the last row of out"
    assert np.array_equal(_bits(fm.numpy()), _bits(c["fmap"])) and np.array_equal(dw.numpy(), wins), "an input was written"
    gidx = None
    if with_idx:
        gidx = idx.numpy()
        assert np.all(gidx[n:] == -7777), "stores behind the last row of idx"
        gidx = gidx[:n].reshape(c["R"], c["D"])
    return got[:n].reshape(c["R"], c["D"]), gidx


def _backward(F, c, det):
    ref.check_windows(c["wins"], c["H"], c["W"])
    assert c["bidx"].max() < c["H"] * c["W"] and c["bidx"].min() >= -1              # every index lies inside its plane
    n = c["C"] * c["H"] * c["W"]
    gm = F.DeviceTensor.from_numpy(np.concatenate([c["gmap0"].reshape(-1), np.full(GUARD, -77.0, np.float32)]))
    g = F.DeviceTensor.from_numpy(c["gout"])
    idx = F.DeviceTensor.from_numpy(c["bidx"])
    F._lib.call("frcnn_set_option", b"deterministic", int(det))
    try:
        F._lib.call("frcnn_roi_pool_backward", F.ptr(gm), c["C"], c["H"], c["W"], F.ptr(g), F.ptr(idx), c["R"], c["kh"], c["kw"],
                    F.stream_ptr())
        got = gm.numpy()
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    assert np.all(got[n:] == -77.0), "stores behind the last plane of gmap"
    return got[:n].reshape(c["C"], c["H"], c["W"])


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_forward(F, case):
    c = ref.inputs(case)
    out, idx = _forward(F, c)
    wrong = np.argwhere(idx != c["idx"])
    assert len(wrong) == 0, "%d winners differ, the first at row %d, column %d: %d, reference %d (window %s)" % (
        len(wrong), wrong[0][0], wrong[0][1], idx[tuple(wrong[0])], c["idx"][tuple(wrong[0])], c["wins"][wrong[0][0]].tolist())
    assert np.array_equal(_bits(out), _bits(c["out"]))
    out2, idx2 = _forward(F, c)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(idx, idx2), "two forward runs differ"
    out3, _ = _forward(F, c, with_idx=False)
    assert np.array_equal(_bits(out), _bits(out3)), "idx = NULL changes out"


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_backward(F, case, det):
    c = ref.inputs(case)
    got = _backward(F, c, det)
    err = np.abs(got.astype(np.float64) - c["gmap"])
    bar = ref.backward_bar(c["count"], c["abs_sum"], det)
    worst = float((err / bar).max())
    print("backward %s det=%d: worst error / bar %.3g, most terms %d, labels %s" % (
        ref.case_id(case), det, worst, int(c["count"].max()), sorted(ref.backward_plan(c["H"], c["W"], det))))
    assert np.all(err <= bar), "worst error / bar %.3g" % worst
    untouched = c["count"] == 1          # (the initial map is the element's only term)
    assert untouched.any() or c["H"] * c["W"] < 29 * 50
    assert np.array_equal(_bits(got[untouched]), _bits(c["gmap0"][untouched])), "an element no term touches has changed"
    assert (c["count"] > 1).any()
    if case[3] == "overlap":
        assert int(c["count"].max()) > 50, "the windows do not pile up"
    if det:
        assert np.array_equal(_bits(got), _bits(_backward(F, c, 1))), "two deterministic backward runs differ"


def test_backward_of_nothing_leaves_the_map(F):
    """every idx = -1, and every gout = 0: no element changes, in either mode, on the LDS and on the global paths"""
    for case in ((ref.MAIN, (6, 6), "ties", "edges"), ((2, 127, 130), (7, 7), "ties", "edges")):
        c = dict(ref.inputs(case))
        for bidx, gout in ((np.full_like(c["bidx"], -1), c["gout"]), (c["idx"], np.zeros_like(c["gout"]))):
            c.update(bidx=bidx, gout=gout)
            for det in (0, 1):
                assert np.array_equal(_bits(_backward(F, c, det)), _bits(c["gmap0"])), (ref.case_id(case), det)


def test_no_rois_no_launch(F):
    """R = 0: FRCNN_OK, nothing launched, nothing written"""
    nk = len(F._lib.KC_NAMES)
    k = F._lib.KC_NAMES.index("roi")
    out = F.DeviceTensor.from_numpy(np.full(64, 3.0, np.float32))
    idx = F.DeviceTensor.from_numpy(np.full(64, -5, np.int32))
    gm = F.DeviceTensor.from_numpy(np.full(5 * 3 * 5, 2.0, np.float32))
    fm = F.DeviceTensor.zeros((5, 3, 5)); wins = F.DeviceTensor.from_numpy(np.array([[1, 3, 1, 5]], np.int32))
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    F._lib.call("frcnn_prof_enable", 1 << k)
    try:
        for det in (0, 1):
            F._lib.call("frcnn_set_option", b"deterministic", det)
            for R in (0, -3):
                F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), 5, 3, 5, F.ptr(wins), R, 3, 5, F.ptr(out), F.ptr(idx), F.stream_ptr())
                F._lib.call("frcnn_roi_pool_forward", F.ptr(fm), 5, 3, 5, F.ptr(wins), R, 3, 5, F.ptr(out), None, F.stream_ptr())
                F._lib.call("frcnn_roi_pool_backward", F.ptr(gm), 5, 3, 5, F.ptr(out), F.ptr(idx), R, 3, 5, F.stream_ptr())
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    assert la[k] == 0
    assert np.all(out.numpy() == 3.0) and np.all(idx.numpy() == -5) and np.all(gm.numpy() == 2.0)


# ------------------------------------------------------------------------------------------------ wiring: the objective
def test_objective_with_a_3x5_grid_against_the_oracle(F, O):
    """kh = 3, kw = 5 through roi_pooling_settings, the forward and backward launches, D = kh kw planes and the classification
    net's first Linear: losses and every gradient tensor against the oracle, which pools 3 rows by 5 columns.  The oracle takes the
    device's cell winners as given and counts those it would have chosen differently (tests/decisions.py): a grid of 5 rows by 3
    columns on either side has the same 15 cells a plane but other windows, and fails that count (the oracle built with kh = 5,
    kw = 3 differed in 11779 of this step's 15000 winners; none differ as it stands)"""
    import width_plan as WP
    from test_gpu_model import check_loss_and_gradient
    from test_gpu_widths import _examples
    from util import TINY_CLS, TINY_HEADS, TINY_LAYERS, oracle_model
    cfg = dict(F.duplo_cfg)
    cfg["roi_pooling"] = dict(kh=3, kw=5)
    assert F.roi_pooling_settings(cfg)[:3] == (3, 5, "max")
    model = F.create_model(cfg, TINY_LAYERS, TINY_HEADS, TINY_CLS)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=3)
    om = oracle_model(O, cfg, TINY_LAYERS, TINY_HEADS, TINY_CLS)
    assert O.param_count(om) == (model["native"].total_params, model["native"].pnet_params)
    s = dict(cfg=cfg, model=model, weights=weights, gradient=gradient, om=om, w=weights.cpu().numpy().copy())
    H, W = WP.SMALL
    ex = _examples(F, model, cfg, H, W, (16, 12, 8, 4), seed=2)
    r = check_loss_and_gradient(F, O, s, H, W, examples=[ex])
    assert r["examples"] > 0
