"""Two fused launches of the backbone's training step, op by op: the 2x2 max pool in conv_igemm's epilogue (csrc/conv.hip
IgemmPool / store_tile_pool, through frcnn_conv2d_forward_pool) and the first layer's weight, bias and slope gradients
straight from the pooled map's gradient (conv_wgrad_first_kernel<3, true>, through frcnn_conv2d_backward_weight_pooled).
tests/conv_plan.py holds the case tables and says which path each case takes; tests/test_conv_plan.py checks that without a
GPU.

Forward, every case on two kinds of data:
  exact data    small integers (bias, slopes, scales: multiples of 1/4) such that every partial sum is representable in fp32
                (asserted on the CPU): `out` equals the fp64 reference exactly, and the maps are full of exact ties;
  random data   `out` within conv_plan.rounding_bound(K, S, mag) of the fp64 reference.
In both, `pooled` and `pidx` get no tolerance: they are, bit for bit, what a numpy float32 restatement of
maxpool_act_forward_kernel (conv_plan.pool_act_fp32) and the pooling kernel itself make of the `out` the device returned;
*fused_out is what conv_plan.pool_plan says; nothing is written behind the ends of the three outputs; the record of the
pooled map, reduced as tests/test_gpu_amax.py reduces one, is max |pooled| exactly.

Backward: fp64 references by the definition (conv_plan.ref_pooled_weight_gradient); on exact data all three results are
exact, on random data within the rounding bounds, which the un-fused pair (pool backward, then the first-layer weight
gradient and the bias sum) has to meet on the same data as well."""
import ctypes as C
import zlib

import numpy as np
import pytest

import conv_plan as CP

pytestmark = pytest.mark.gpu

WORST = {}       # quantity -> (largest error / rounding bound, case)
TAIL = 64        # sentinel elements behind every output
SENT_F = np.float32(-7777.25)
SENT_B = 0xA5
MAX_BLOCKS = 16384


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _dev(F, a, dtype=np.float32):
    return F.DeviceTensor.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def _scalar(F, v):
    return None if v is None else _dev(F, [v])


def _guarded(F, n, body, tail, dtype=np.float32):
    """a device buffer of n elements filled with `body` and TAIL more filled with `tail`"""
    a = np.full(n + TAIL, body, dtype)
    a[n:] = tail
    return _dev(F, a, dtype)


def _split(t, n, tail, what):
    a = t.numpy()
    assert (a[n:] == tail).all(), "%s: written behind its end" % what
    return a[:n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ratio(quantity, what, got, want64, bound):
    err = np.abs(np.asarray(got, np.float64) - want64)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s %s: max error / bound = %.4f" % (quantity, what, ratio))
    if ratio > WORST.get(quantity, (-1.0, ""))[0]:
        WORST[quantity] = (ratio, what)
    return ratio


# ---- magnitude records (as tests/test_gpu_amax.py) -------------------------------------------------------------------------
def _new_rec(F):
    n = F._lib.load().frcnn_amax_record_floats()
    assert n >= MAX_BLOCKS + 1
    p = np.full(n, 1e30, np.float32)   # an entry or a count the launch leaves unwritten shows
    p[:1] = np.array([MAX_BLOCKS], np.int32).view(np.float32)
    return _dev(F, p)


def _rec_max(rec):
    rec = np.asarray(rec, np.float32)
    n = int(rec[:1].view(np.int32)[0])
    assert 1 <= n <= MAX_BLOCKS, "count word %d" % n
    e = rec[1:1 + n]
    assert np.isfinite(e).all() and (e >= 0).all()
    return e.max()


# ---- forward --------------------------------------------------------------------------------------------------------------
def _scale_vec(rng, n, other):
    """entries of {0, 1} and one `other`; a zero entry makes every window of its channel a four-way tie"""
    s = (rng.rand(n) > 0.4).astype(np.float32)
    s[0] = 1.0
    if n > 1:
        s[-1] = 0.0
    if n > 2:
        s[n // 2] = other
    return s


def _forward_data(name, shape, v, exact):
    C_, H, W, M = shape
    rng = _rng("pool", name, exact)
    if exact:
        x = rng.randint(-2, 3, (C_, H, W)).astype(np.float32)   # (a narrow range: many equal sums inside a window)
        w = rng.randint(-1, 2, (M, C_, 3, 3)).astype(np.float32)
        b = (rng.randint(-8, 9, M) * 0.25).astype(np.float32)
    else:
        x = rng.randn(C_, H, W).astype(np.float32)
        w = (rng.randn(M, C_, 3, 3) / np.sqrt(C_ * 9)).astype(np.float32)
        b = rng.randn(M).astype(np.float32)
    in_slope = in_scale = None
    quantum = 0.25
    if v["in_act"]:
        in_slope = np.float32(0.25)
        in_scale = _scale_vec(rng, C_, 0.5 if exact else 0.6)
        quantum = 0.125   # 1/4 (slope) * 1/2 (scale) * integers
    pool_scale = _scale_vec(rng, M, 0.75 if exact else 0.6) if v["scale"] else None
    return x, w, (b if v["bias"] else None), in_slope, in_scale, pool_scale, quantum


def _run_forward(F, name, shape, variant, exact):
    C_, H, W, M = shape
    pad = CP.POOL_PAD
    v = CP.pool_variant(variant)
    plan = CP.pool_plan(C_, H, W, M, pad)
    Ho, Wo, Hp, Wp = plan["Ho"], plan["Wo"], plan["Hp"], plan["Wp"]
    x, w, b, in_slope, in_scale, pool_scale, quantum = _forward_data(name, shape, v, exact)
    pool_slope = None if v["slope"] is None else np.float32(v["slope"])
    what = "%s%s %s" % (name, "" if variant is None else " " + variant, "exact" if exact else "random")
    act = CP.activate(x, in_slope, in_scale)
    want64 = CP.ref_forward(act, w, b, pad)
    mag = CP.ref_forward(np.abs(act), np.abs(w), None if b is None else np.abs(b), pad)
    if exact:
        CP.assert_exact_in_fp32(mag, quantum, what)

    n, npool = M * Ho * Wo, M * Hp * Wp
    out = _guarded(F, n, np.nan, SENT_F)
    pooled = _guarded(F, npool, np.nan, SENT_F)
    pidx = _guarded(F, npool, 0xEE, SENT_B, np.uint8)
    rec = _new_rec(F) if v["rec"] else None
    fused = C.c_int(-1)
    dx, dw, db = _dev(F, x), _dev(F, w), (None if b is None else _dev(F, b))
    dis, disc = _scalar(F, in_slope), (None if in_scale is None else _dev(F, in_scale))
    dps, dpsc = _scalar(F, pool_slope), (None if pool_scale is None else _dev(F, pool_scale))
    F._lib.call("frcnn_conv2d_forward_pool", F.ptr(dx), C_, H, W, F.ptr(dis), F.ptr(disc), F.ptr(dw), F.ptr(db), M, pad, F.ptr(dps),
                F.ptr(dpsc), F.ptr(out), F.ptr(pooled), F.ptr(pidx), F.ptr(rec), C.byref(fused), F.stream_ptr())
    got = _split(out, n, SENT_F, what + " out").reshape(M, Ho, Wo)
    gp = _split(pooled, npool, SENT_F, what + " pooled").reshape(M, Hp, Wp)
    gi = _split(pidx, npool, SENT_B, what + " pidx").reshape(M, Hp, Wp)
    assert fused.value == int(plan["fused"]), "%s: fused_out %d, the plan says %r" % (what, fused.value, plan["fused"])

    # out
    assert np.isfinite(got).all(), "%s: out not finite (an element was left out?)" % what
    if exact:
        assert np.array_equal(want64.astype(np.float32).astype(np.float64), want64)
        bad = got.astype(np.float64) != want64
        assert not bad.any(), "%s: %d elements of out differ from the exact result, first at %r" % (
            what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    else:
        ratio = _ratio("out", what, got, want64, CP.rounding_bound(plan["K"], plan["splitK"], mag))
        assert ratio <= 1.0, "%s: out error %.3f times the rounding bound (K = %d, S = %d)" % (what, ratio, plan["K"], plan["splitK"])

    # pooled, pidx: no tolerance
    wp, wi = CP.pool_act_fp32(got, pool_slope, pool_scale)
    assert np.isfinite(gp).all(), "%s: pooled not finite (an element was left out?)" % what
    bad = gi != wi
    assert not bad.any(), "%s: %d winner codes differ from the restatement, first at %r: %d, want %d" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), gi[bad][0], wi[bad][0])
    bad = _bits(gp) != _bits(wp)
    assert not bad.any(), "%s: %d pooled values differ from the restatement, first at %r: %r, want %r" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), gp[bad][0], wp[bad][0])
    if exact:   # the data are full of ties, and the ties are what "first maximum wins" is about
        a = CP.activate(got, pool_slope, pool_scale)
        if M * (Ho // 2) * (Wo // 2) >= 256:
            assert _tied_windows(a) > 0, "%s: no window with a tie" % what

    # ... and the pooling kernel on that same out
    kp = _guarded(F, npool, np.nan, SENT_F)
    ki = _guarded(F, npool, 0xEE, SENT_B, np.uint8)
    F._lib.call("frcnn_maxpool_act_forward", F.ptr(out), M, Ho, Wo, F.ptr(dps), F.ptr(dpsc), F.ptr(kp), F.ptr(ki), F.stream_ptr())
    assert np.array_equal(_bits(_split(kp, npool, SENT_F, what + " kernel pooled")), _bits(gp).ravel()), what
    assert np.array_equal(_split(ki, npool, SENT_B, what + " kernel pidx"), gi.ravel()), what

    if rec is not None:
        r, m = _rec_max(rec.numpy()), np.abs(gp).max()
        assert r.dtype == np.float32 and r == m, "%s: record %r, max |pooled| %r" % (what, r, m)
    return plan


def _tied_windows(a):
    """how many full 2x2 windows of a hold their maximum more than once"""
    C_, H, W = a.shape
    h, w = H // 2 * 2, W // 2 * 2
    if h == 0 or w == 0:
        return 0
    win = a[:, :h, :w].reshape(C_, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 2, 4).reshape(C_, h // 2, w // 2, 4)
    return int(((win == win.max(-1, keepdims=True)).sum(-1) > 1).sum())


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "random"))
@pytest.mark.parametrize("c", CP.POOL_CASES, ids=lambda c: c["name"])
def test_forward_pool(F, c, exact):
    """the base call: pool slope 0.25, no pool scale, a bias, a record"""
    _run_forward(F, c["name"], c["shape"], None, exact)


@pytest.mark.parametrize("exact", (True, False), ids=("exact", "random"))
@pytest.mark.parametrize("variant", CP.POOL_VARIANTS)
@pytest.mark.parametrize("base", CP.POOL_VARIANT_BASES)
def test_forward_pool_variants(F, base, variant, exact):
    """one fused case of the first-layer kernel and one of the generic kernel with a pool scale, slopes <= 0 and > 1, no slope,
    an activation on the input, no bias, no record"""
    plan = _run_forward(F, base, CP.find_pool(base)["shape"], variant, exact)
    assert plan["fused"]


def test_forward_pool_does_not_depend_on_the_call_before_it(F):
    """fused, fallback (whose launch leaves slabs in the split-K workspace), fused again: the same bits"""
    def run(name):
        c = CP.find_pool(name)
        C_, H, W, M = c["shape"]
        plan = CP.pool_plan(C_, H, W, M, CP.POOL_PAD)
        x, w, b, _, _, _, _ = _forward_data(name, c["shape"], CP.pool_variant(None), False)
        n, npool = M * plan["Ho"] * plan["Wo"], M * plan["Hp"] * plan["Wp"]
        out, pooled, pidx = _guarded(F, n, np.nan, SENT_F), _guarded(F, npool, np.nan, SENT_F), _guarded(F, npool, 0xEE, SENT_B, np.uint8)
        ds = _scalar(F, np.float32(0.25))
        fused = C.c_int(-1)
        dx, dw, db = _dev(F, x), _dev(F, w), _dev(F, b)
        F._lib.call("frcnn_conv2d_forward_pool", F.ptr(dx), C_, H, W, None, None, F.ptr(dw), F.ptr(db), M,
                    CP.POOL_PAD, F.ptr(ds), None, F.ptr(out), F.ptr(pooled), F.ptr(pidx), None, C.byref(fused), F.stream_ptr())
        assert fused.value == int(plan["fused"])
        return out.numpy(), pooled.numpy(), pidx.numpy()
    first = run("p_generic_m70")
    run("p_two_splits")
    again = run("p_generic_m70")
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- backward -------------------------------------------------------------------------------------------------------------
def _inside_codes(rng, O_, Ho, Wo, Hp, Wp):
    """a random winner code per window, restricted to positions inside the map"""
    dy = rng.randint(0, 2, (O_, Hp, Wp))
    dx = rng.randint(0, 2, (O_, Hp, Wp))
    dy[(2 * np.arange(Hp)[None, :, None] + dy) >= Ho] = 0
    dx[(2 * np.arange(Wp)[None, None, :] + dx) >= Wo] = 0
    return (2 * dy + dx).astype(np.uint8)


def _backward_data(name, shape, exact, codes, slope):
    C_, H, W, O_, pad = shape
    p = CP.first_pooled_plan(*shape)
    Ho, Wo, Hp, Wp = p["Ho"], p["Wo"], p["Hp"], p["Wp"]
    rng = _rng("pooled wgrad", name, exact, codes)
    if exact:
        inp = rng.randint(-3, 4, (C_, H, W)).astype(np.float32)
        x = rng.randint(-3, 4, (O_, Ho, Wo)).astype(np.float32)
        gpool = rng.randint(-3, 4, (O_, Hp, Wp)).astype(np.float32)
        gw0 = (rng.randint(-8, 9, (O_, C_, 3, 3)) * 0.25).astype(np.float32)
        gb0 = (rng.randint(-8, 9, O_) * 0.25).astype(np.float32)
        gs0 = np.float32(-1.75)
    else:
        inp = rng.randn(C_, H, W).astype(np.float32)
        x = rng.randn(O_, Ho, Wo).astype(np.float32)
        gpool = (rng.randn(O_, Hp, Wp) / np.sqrt(Hp * Wp)).astype(np.float32)
        gw0 = rng.randn(O_, C_, 3, 3).astype(np.float32)
        gb0 = rng.randn(O_).astype(np.float32)
        gs0 = np.float32(rng.randn())
    code = CP.pool_act_fp32(x, slope, None)[1] if codes == "pooled" else _inside_codes(rng, O_, Ho, Wo, Hp, Wp)
    return p, inp, x, gpool, code, gw0, gb0, gs0


def _check_backward(what, tag, exact, p, N, got, want, mags, start):
    """got = (gw, gb, gslope) of the device, want / mags the fp64 sums and their magnitude sums, start the values the
    destinations held"""
    gw0, gb0, gs0 = start
    (gw64, gb64, gs64), (mw, mb, ms) = want, mags
    gw, gb, gs = got
    wants = (gw0.astype(np.float64) + gw64, gb0.astype(np.float64) + gb64, np.float64(gs0) + gs64)
    mags = (mw + np.abs(gw0), mb + np.abs(gb0), ms + abs(float(gs0)))
    if exact:
        for q, g_, w_, m_ in zip(("gweight", "gbias", "gslope"), got, wants, mags):
            CP.assert_exact_in_fp32(m_, 0.25, what + " " + q)
            assert np.array_equal(np.asarray(g_, np.float64), w_), "%s %s%s: not the exact result" % (what, q, tag)
        return
    bounds = (CP.rounding_bound(p["K"], p["nSplit"], mags[0]), CP.rounding_bound(p["K"], p["nSplit"], mags[1]),
              CP.rounding_bound(N, p["nSplit"], mags[2]))
    for q, g_, w_, b_ in zip(("gweight", "gbias", "gslope"), got, wants, bounds):
        assert np.isfinite(g_).all()
        ratio = _ratio(q + tag, what, g_, w_, b_)
        assert ratio <= 1.0, "%s %s%s: error %.3f times the rounding bound" % (what, q, tag, ratio)


def _run_backward(F, name, shape, exact, codes, slope=0.25):
    C_, H, W, O_, pad = shape
    slope = np.float32(slope)
    p, inp, x, gpool, code, gw0, gb0, gs0 = _backward_data(name, shape, exact, codes, slope)
    Ho, Wo = p["Ho"], p["Wo"]
    what = "%s %s codes %s slope %g" % (name, "exact" if exact else "random", codes, slope)
    want, mags = CP.ref_pooled_weight_gradient(inp, gpool, code, x, slope, pad)
    N = CP.first_pooled_slope_terms(p)
    din, dgp, dcode, dx, dsl = _dev(F, inp), _dev(F, gpool), _dev(F, code, np.uint8), _dev(F, x), _scalar(F, slope)

    gw, gb, gs = (_dev(F, np.concatenate([np.ravel(a).astype(np.float32), np.full(TAIL, SENT_F, np.float32)])) for a in (gw0, gb0, [gs0]))
    F._lib.call("frcnn_conv2d_backward_weight_pooled", F.ptr(din), C_, H, W, F.ptr(dgp), F.ptr(dcode), F.ptr(dx), F.ptr(dsl), O_, pad,
                F.ptr(gw), F.ptr(gb), F.ptr(gs), F.stream_ptr())
    got = (_split(gw, gw0.size, SENT_F, what + " gweight").reshape(gw0.shape), _split(gb, O_, SENT_F, what + " gbias"),
           _split(gs, 1, SENT_F, what + " gslope")[0])
    _check_backward(what, "", exact, p, N, got, want, mags, (gw0, gb0, gs0))

    # the un-fused pair on the same data: pool + PReLU backward to the full-resolution gradient, then the first-layer weight
    # gradient and the bias sum
    g = F.DeviceTensor.zeros((O_, Ho, Wo))
    ugw, ugb, ugs = _dev(F, gw0), _dev(F, gb0), _dev(F, [gs0])
    F._lib.call("frcnn_maxpool_act_backward", F.ptr(dgp), F.ptr(dcode), F.ptr(dx), O_, Ho, Wo, F.ptr(dsl), None, F.ptr(g), None, F.ptr(ugs),
                F.stream_ptr())
    F._lib.call("frcnn_conv2d_backward_weight", F.ptr(din), C_, H, W, None, None, F.ptr(g), O_, 3, pad, F.ptr(ugw), F.ptr(ugb),
                F.stream_ptr())
    _check_backward(what, " (un-fused)", exact, p, N, (ugw.numpy(), ugb.numpy(), ugs.numpy()[0]), want, mags, (gw0, gb0, gs0))


@pytest.mark.parametrize("codes", ("pooled", "random"))
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "random"))
@pytest.mark.parametrize("c", CP.FIRST_POOLED_CASES, ids=lambda c: c["name"])
def test_backward_weight_pooled(F, c, exact, codes):
    """the destinations start non-zero: the entry point accumulates.  codes: the winners of the numpy pooling of x, or a random
    draw among the positions inside the map"""
    _run_backward(F, c["name"], c["shape"], exact, codes)
    if exact:
        _run_backward(F, c["name"], c["shape"], exact, codes, slope=-0.5)


@pytest.mark.parametrize("name", sorted(CP.FIRST_POOLED_ERRORS))
def test_backward_weight_pooled_refuses(F, name):
    """C = 4, O = 65, Wo = 1, no slope: an error, and the three destinations untouched"""
    (C_, H, W, O_, pad), with_slope = CP.FIRST_POOLED_ERRORS[name]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    rng = _rng("refuse", name)
    gw0, gb0, gs0 = rng.randn(O_ * C_ * 9).astype(np.float32), rng.randn(O_).astype(np.float32), rng.randn(1).astype(np.float32)
    gw, gb, gs = _dev(F, gw0), _dev(F, gb0), _dev(F, gs0)
    din, dx = _dev(F, rng.randn(C_, H, W)), _dev(F, rng.randn(O_, Ho, Wo))
    dgp, dcode = _dev(F, rng.randn(O_, Hp, Wp)), _dev(F, np.zeros((O_, Hp, Wp)), np.uint8)
    dsl = _scalar(F, np.float32(0.25)) if with_slope else None
    with pytest.raises(F._lib.FrcnnError):
        F._lib.call("frcnn_conv2d_backward_weight_pooled", F.ptr(din), C_, H, W, F.ptr(dgp), F.ptr(dcode), F.ptr(dx), F.ptr(dsl), O_, pad,
                    F.ptr(gw), F.ptr(gb), F.ptr(gs), F.stream_ptr())
    for t, a in ((gw, gw0), (gb, gb0), (gs, gs0)):
        assert np.array_equal(_bits(t.numpy()), _bits(a))


def test_zz_worst_ratios_of_the_file(F):
    """Runs last (file order): the largest error / rounding bound of every quantity.  No bar is taken from these numbers.
    On an MI355X: out 0.18, gweight 0.18 and gbias 0.08 (both on the one-row map; below 1e-4 on the maps of 127 slabs and more,
    where three of four routed gradients are zero and K = Ho Wo counts them all), gslope 0.004 (un-fused 0.012).  The slope
    bound is a worst case over 72 to 136 roundings of a sum whose errors mostly cancel: it would not see one lost term, nor would
    the weight bounds on the large maps.  The exact-data runs are what guards those: there a lost or doubled term changes bits."""
    for q in sorted(WORST):
        print("largest error / rounding bound, %s: %.4f (%s)" % (q, WORST[q][0], WORST[q][1]))
