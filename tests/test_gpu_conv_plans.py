"""The fp32 matrix-core convolutions of csrc/conv.hip (conv_igemm, conv_wgrad, the first-layer weight gradient and their
split-K folds) across their launch plans, through frcnn_conv2d_forward / _backward_input / _backward_weight with option
split_bf16 off, so that EVERY shape runs conv.hip.  tests/conv_plan.py holds the case tables and says which plan each case
takes; tests/test_conv_plan.py checks that without a GPU.

Every result meets two things:
  the project's bar     |a - b| <= 1e-4 max(1, |b|) against the CPU oracle (fp64 accumulation), as tests/test_gpu_conv.py;
  the rounding bound    |a - b| <= (K + S + 2) 2^-24 mag against an fp64 reference, K = length of the dot product, S = slabs
                        folded, mag = the same operation on |x|, |w| (+ |b|, + |destination| where the call accumulates): the
                        standard bound of an fp32 sum taken in any order (conv_plan.rounding_bound).  It is far tighter than
                        the bar wherever an output cancels, and an operand rounded to 16 bits anywhere would break it.
Stores go to destinations filled with NaN: an element that the launch leaves out does not pass."""
import zlib

import numpy as np
import pytest

import conv_plan as CP
from util import assert_close

pytestmark = pytest.mark.gpu

FOUND = []    # the value of split_bf16 that the first test of the file found
WORST = {}    # role -> (largest error / rounding bound, case)


def _option(F, name, value=None):
    import ctypes as C
    if value is None:
        v = C.c_int(0)
        F._lib.call("frcnn_get_option", name.encode(), C.byref(v))
        return v.value
    F._lib.call("frcnn_set_option", name.encode(), int(value))


@pytest.fixture
def fp32_only(F):
    """option split_bf16 off for the test, then back to the value found"""
    before = _option(F, "split_bf16")
    if not FOUND:
        FOUND.append(before)
    _option(F, "split_bf16", 0)
    yield
    _option(F, "split_bf16", before)


def _dev(F, a):
    return F.DeviceTensor.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _nan(F, shape):
    return _dev(F, np.full(shape, np.nan, np.float32))


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _check(role, what, got, want_oracle, want64, mag, K, S, tol=1e-4):
    """the bar against the oracle's result, the rounding bound against the fp64 reference"""
    assert got.shape == want64.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), "%s %s: not finite (an element was left out?)" % (role, what)
    err = np.abs(got.astype(np.float64) - want64)
    bound = CP.rounding_bound(K, S, mag)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s %s: K %d S %d, max error / bound = %.3f" % (role, what, K, S, ratio))
    if ratio > WORST.get(role, (0.0, ""))[0]:
        WORST[role] = (ratio, what)
    assert_close(got, want_oracle, tol, "%s %s" % (role, what))
    assert ratio <= 1.0, "%s %s: error %.3f times the rounding bound (K = %d, S = %d)" % (role, what, ratio, K, S)


def _act_args(F, rng, mode, C_, two=False):
    """-> (slope, scale) host values and their device tensors for an activation mode of conv_plan.ACT_MODES, or Nones"""
    slope = np.float32(0.25) if mode in ("slope", "both") else None
    scale = None
    if mode in ("scale", "both"):
        scale = (rng.rand(C_) > 0.4).astype(np.float32)
        scale[0], scale[-1] = 1.0, 0.0 if C_ > 1 else 1.0
        if two:
            scale[C_ // 2] = 2.0
    return slope, scale, (_dev(F, [slope]) if slope is not None else None), (_dev(F, scale) if scale is not None else None)


# ---- forward ----------------------------------------------------------------------------------------------------------
def _forward_inputs(name, shape):
    C_, H, W, O_, k, pad = shape
    rng = _rng("fwd", name)
    x = rng.randn(C_, H, W).astype(np.float32)
    w = (rng.randn(O_, C_, k, k) / np.sqrt(C_ * k * k)).astype(np.float32)
    b = rng.randn(O_).astype(np.float32)
    return rng, x, w, b


def _run_forward(F, O, name, shape, bias=True, mode=None, two=False):
    C_, H, W, O_, k, pad = shape
    rng, x, w, b = _forward_inputs(name, shape)
    if not bias:
        b = None
    slope, scale, da, ds = _act_args(F, rng, mode, C_, two)
    act = CP.activate(x, slope, scale)
    plan = CP.forward_plan(shape, act=mode is not None)
    want64 = CP.ref_forward(act, w, b, pad)
    mag = CP.ref_forward(np.abs(act), np.abs(w), None if b is None else np.abs(b), pad)
    out = _nan(F, want64.shape)
    dx, dw = _dev(F, x), _dev(F, w)
    db = _dev(F, b) if bias else None
    F._lib.call("frcnn_conv2d_forward", F.ptr(dx), C_, H, W, F.ptr(da), F.ptr(ds), F.ptr(dw), F.ptr(db), O_, k, pad, F.ptr(out),
                F.stream_ptr())
    got = out.numpy()
    what = "%s%s%s" % (name, "" if bias else " no bias", "" if mode is None else " act " + mode + (" x2" if two else ""))
    _check("forward", what, got, O.conv2d_fwd(act, w, b, pad), want64, mag, plan["K"], plan["splitK"])
    return got


@pytest.mark.parametrize("c", CP.IGEMM_CASES + CP.SPLITK_CASES, ids=lambda c: c["name"])
def test_forward(F, O, fp32_only, c):
    _run_forward(F, O, c["name"], c["shape"])


@pytest.mark.parametrize("c", CP.SPLITK_CASES + [CP.find(n) for n in ("c3_k3", "c33_k1", "ragged_k3", "row_k7")], ids=lambda c: c["name"])
def test_forward_without_bias(F, O, fp32_only, c):
    """the fold adds the bias: a null bias is a path of its own there (and in the tile epilogue)"""
    _run_forward(F, O, c["name"], c["shape"], bias=False)


@pytest.mark.parametrize("mode", CP.ACT_MODES)
@pytest.mark.parametrize("k", sorted(CP.ACT_SHAPES))
def test_forward_fused_activation(F, O, fp32_only, k, mode):
    """the producing layer's PReLU slope and dropout scale, applied by the activating loader (every k: with split_bf16 on the
    entry point sends 3x3 launches with an activation to convx.hip, so this runs with the option off like the rest)"""
    for name in CP.ACT_SHAPES[k]:
        _run_forward(F, O, name, CP.find(name)["shape"], mode=mode)


@pytest.mark.parametrize("name,mode", CP.ACT_EXTRA)
def test_forward_fused_activation_other_instantiations(F, O, fp32_only, name, mode):
    _run_forward(F, O, name, CP.find(name)["shape"], mode=mode)


@pytest.mark.parametrize("name", CP.ACT_SCALE_TWO)
def test_forward_scale_entry_of_two(F, O, fp32_only, name):
    """the fp32 loader multiplies by the scale: an entry of 2.0 is accepted and doubles its channel"""
    _run_forward(F, O, name, CP.find(name)["shape"], mode="both", two=True)


def test_forward_activation_takes_conv_hip_at_default_options(F, O):
    """5x5 / 7x7 with an activation reach conv.hip whatever split_bf16 says (api.cpp): the same bits with the option on"""
    name = "split_k5"
    before = _option(F, "split_bf16")
    try:
        _option(F, "split_bf16", 1)
        a = _run_forward(F, O, name, CP.find(name)["shape"], mode="both")
        _option(F, "split_bf16", 0)
        b = _run_forward(F, O, name, CP.find(name)["shape"], mode="both")
    finally:
        _option(F, "split_bf16", before)
    assert np.array_equal(a, b)


# ---- input gradient ---------------------------------------------------------------------------------------------------
def _run_input_gradient(F, O, name, fshape):
    C_, H, W, O_, k, pad = CP.mirror(fshape)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    plan = CP.input_gradient_plan((C_, H, W, O_, k, pad))
    rng = _rng("dgrad", name)
    g = rng.randn(O_, Ho, Wo).astype(np.float32)
    w = (rng.randn(O_, C_, k, k) / np.sqrt(O_ * k * k)).astype(np.float32)
    gin0 = rng.randn(C_, H, W).astype(np.float32)
    want_o = O.conv2d_bwd_input(g, w, pad, H, W)
    want64 = CP.ref_input_gradient(g, w, pad, H, W)
    mag = CP.ref_input_gradient(np.abs(g), np.abs(w), pad, H, W)
    dg, dw = _dev(F, g), _dev(F, w)
    gin = _nan(F, (C_, H, W))
    F._lib.call("frcnn_conv2d_backward_input", F.ptr(dg), O_, Ho, Wo, F.ptr(dw), C_, k, pad, F.ptr(gin), 0, F.stream_ptr())
    stored = gin.numpy()
    _check("input_gradient", name, stored, want_o, want64, mag, plan["K"], plan["splitK"])
    # accumulate = 1 on a destination that is not zero
    acc = _dev(F, gin0)
    F._lib.call("frcnn_conv2d_backward_input", F.ptr(dg), O_, Ho, Wo, F.ptr(dw), C_, k, pad, F.ptr(acc), 1, F.stream_ptr())
    _check("input_gradient", name + " accumulate", acc.numpy(), gin0.astype(np.float64) + want_o, gin0.astype(np.float64) + want64,
           mag + np.abs(gin0), plan["K"], plan["splitK"])
    # ... and once more on top (tests/test_gpu_conv.py's second accumulating call)
    F._lib.call("frcnn_conv2d_backward_input", F.ptr(dg), O_, Ho, Wo, F.ptr(dw), C_, k, pad, F.ptr(gin), 1, F.stream_ptr())
    assert_close(gin.numpy(), 2.0 * want_o.astype(np.float64), 2e-4, "input gradient %s, second accumulating call" % name)
    return stored


@pytest.mark.parametrize("c", CP.IGEMM_CASES + CP.SPLITK_CASES, ids=lambda c: c["name"])
def test_input_gradient(F, O, fp32_only, c):
    """the forward case's plan on the mirrored shape (conv_plan.mirror): K channels = filters, M = input channels"""
    _run_input_gradient(F, O, c["name"], c["shape"])


# ---- weight gradient --------------------------------------------------------------------------------------------------
def _run_weight_gradient(F, O, name, shape, mode=None):
    C_, H, W, O_, k, pad = shape
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    rng = _rng("wgrad", name)
    x = rng.randn(C_, H, W).astype(np.float32)
    g = (rng.randn(O_, Ho, Wo) / np.sqrt(Ho * Wo)).astype(np.float32)
    gw0 = rng.randn(O_, C_, k, k).astype(np.float32)
    gb0 = rng.randn(O_).astype(np.float32)
    slope, scale, da, ds = _act_args(F, rng, mode, C_)
    act = CP.activate(x, slope, scale)
    plan = CP.weight_gradient_plan(shape, act=mode is not None)
    ogw, ogb = O.conv2d_bwd_weight(act, g, k, k, pad)
    gw64, gb64 = CP.ref_weight_gradient(act, g, k, pad)
    mw, mb = CP.ref_weight_gradient(np.abs(act), np.abs(g), k, pad)
    dx, dg, gw, gb = _dev(F, x), _dev(F, g), _dev(F, gw0), _dev(F, gb0)
    F._lib.call("frcnn_conv2d_backward_weight", F.ptr(dx), C_, H, W, F.ptr(da), F.ptr(ds), F.ptr(dg), O_, k, pad, F.ptr(gw), F.ptr(gb),
                F.stream_ptr())
    what = name if mode is None else name + " act " + mode
    got = gw.numpy()
    _check("weight_gradient", what, got, gw0.astype(np.float64) + ogw, gw0.astype(np.float64) + gw64, mw + np.abs(gw0), plan["K"],
           plan["nSplit"])
    _check("bias_gradient", what, gb.numpy(), gb0.astype(np.float64) + ogb, gb0.astype(np.float64) + gb64, mb + np.abs(gb0), plan["K"], 1)
    return got


@pytest.mark.parametrize("c", CP.WGRAD_CASES, ids=lambda c: c["name"])
def test_weight_gradient_accumulates(F, O, fp32_only, c):
    """accGradParameters ADDS to gradWeight and gradBias: both start from random values"""
    _run_weight_gradient(F, O, c["name"], c["shape"])


@pytest.mark.parametrize("mode", CP.ACT_MODES)
@pytest.mark.parametrize("name", CP.WGRAD_ACT_CASES)
def test_weight_gradient_fused_activation(F, O, fp32_only, name, mode):
    """the fused input activation of the fp32 weight gradient; a first-layer shape takes the generic kernel for it (the workspace
    the entry point sizes beforehand has to hold that plan's slabs, whatever call came before: the plain call runs first)"""
    shape = CP.find(name)["shape"]
    if CP.weight_gradient_plan(shape)["kernel"] == "first":
        _run_weight_gradient(F, O, name, shape)
    _run_weight_gradient(F, O, name, shape, mode=mode)


# ---- the answer of a call does not depend on the call before it -----------------------------------------------------------
def _run(F, O, role, name, mode):
    shape = CP.find(name)["shape"]
    if role == "forward":
        return _run_forward(F, O, name, shape, mode=mode)
    if role == "input_gradient":
        assert mode is None
        return _run_input_gradient(F, O, name, shape)
    return _run_weight_gradient(F, O, name, shape, mode=mode)


@pytest.mark.parametrize("pair", CP.ORDER_PAIRS, ids=lambda p: "%s-%s-%s_then_%s-%s-%s" % p)
def test_call_order_independence(F, O, fp32_only, pair):
    """A, B, A: the slabs are folded in a fixed order and nothing is accumulated with atomics, so the two results of A are the
    same bits whatever B left in the split-K workspace and the slab buffers -- and every call succeeds the first time it is made"""
    ra, a, acta, rb, b, actb = pair
    first = _run(F, O, ra, a, acta)
    _run(F, O, rb, b, actb)
    again = _run(F, O, ra, a, acta)
    assert np.array_equal(first, again)


def test_zz_option_restored_and_worst_ratios(F):
    """Runs last (file order): split_bf16 is what the file found, and the largest error / rounding bound of every role"""
    for role in sorted(WORST):
        print("largest error / ((K + S + 2) 2^-24 mag), %s: %.3f (%s)" % (role, WORST[role][0], WORST[role][1]))
    if FOUND:
        assert _option(F, "split_bf16") == FOUND[0]
