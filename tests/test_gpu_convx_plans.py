"""The split-operand convolutions of csrc/convx.hip (conv_x3 and its split-K fold) and csrc/wgradx.hip (conv_wgradx)
across their launch plans, through frcnn_conv2d_forward / _backward_input / _backward_weight / _backward_input_rec with the
default option split_bf16 = 1.  tests/convx_plan.py holds the case tables, says which plan each case takes and derives the
error bound; tests/test_convx_plan.py checks the tables without a GPU.  Every case runs in both operand forms (option x3_f16:
two fp16 planes / three bf16 planes; the _rec entry point exists in the fp16 form only).

Every result meets three things:
  the project's bar     |a - b| <= 1e-4 max(1, |b|) against the fp64 reference (by the definition: conv_plan.ref_*);
  the worst-case bound  |a - b| <= (n + S + 2) 2^-24 mag + the operands' representation error, n = the kept plane products
                        of the dot product, S = slabs folded (convx_plan.split_bound, derived there), all values finite;
  the precision gate    its RMS error against the fp64 reference is at most RMS_GATE times that of the fp32 matrix-core
                        kernel of conv.hip on the same inputs (the same call with split_bf16 = 0; that kernel is held to
                        its own rounding bound by tests/test_gpu_conv_plans.py), and over the file the geometric mean of
                        the ratios is at most MEAN_GATE -- the gates of tests/test_gpu_convx.py.  A case with fewer than
                        8192 outputs is repeated with further seeds and the ratio taken over the pooled outputs.
The slope gradient and the bias gradient are single sums per tensor / per filter: they meet the bar and the same bound,
relative to the sum of the magnitudes of their terms.  Stores go to destinations filled with NaN: an element that the
launch leaves out does not pass; a misaligned destination lies 4 bytes into a larger NaN-filled buffer whose other elements
must stay NaN.

Measured on an MI355X, 2026-10-20 (every ratio is printed; the last test of the file prints the worst per role and form):
  largest error / bound      forward 0.0060 bf16x6, 0.0092 f16x3 (fill_256 without a bias); input gradient 0.0057 (fill_128,
                             accumulating) / 0.0084 (fill_256); activation backward 0.0033 f16x3 (two_tiles_bm128, x misaligned);
                             slope gradient < 0.0001; weight gradient 0.0134 / 0.0154 (tile_pad0); bias gradient 0.0105 (tile,
                             scale).  The bound is a worst case over n roundings and lies a hundred times above what random
                             data does: it is the gate that notices a lost partial product.
  largest gate ratio         forward 1.525 bf16x6, 1.178 f16x3 (short_last, scale); input gradient 1.527 / 1.139 (recomputed_k3,
                             accumulating); activation backward 1.117 f16x3 (short_last_vec2_bm128, scale); weight gradient
                             1.218 bf16x6 (nt3_nt2_exact), 1.236 f16x3 (small_odd); geometric mean over the file's 303 ratios
                             0.941.
What this file found: nine_slabs_k5 = (144, 9, 12, 128, 5, 0) in the three-plane form missed RMS_GATE = 1.75 in the forward
(1.915) and in both input-gradient runs (2.033 storing, 2.020 accumulating) while conv_x3 kept at least two 16-channel chunks
of a 5x5 per split (min_chunks = cdiv(36, 25), against the comment beside it): 9 chunks -> 3 slabs of 1200 products where
conv_igemm of conv.hip folds 18 slabs of 200.  No partial product was lost.  The RMS rounding error of an fp32 accumulation
grows with the square root of the roundings PER SLAB: one v_mfma 32x32x16 rounds once per 16 products and the three-plane
form issues six of them (0.375 roundings per product; the two-plane form three: 0.1875), the fp32 32x32x2 instruction rounds
once per 2 products (0.5) -- 450 / 225 / 100 roundings per slab, expected ratios sqrt(4.5) = 2.12 and sqrt(2.25) = 1.50,
measured 1.92 to 2.03 and 1.38 to 1.49.  The same count gives the other ratios of the file to within 15 % (cap24 0.87 / 0.61
against 0.93 / 0.69 measured, recomputed_k3 1.58 / 1.12 against 1.25 to 1.53 / 0.96 to 1.14, cap16 1.02 / 0.72 against 0.98
to 1.04 / 0.75 to 0.78).  conv_x3 now lets a 5x5 split down to one chunk, as a 7x7 always could: the 5x5 cases (two_slabs_k5,
nine_slabs_k5, cut_k5) went from 1.62 to 2.03 / 1.21 to 1.49 to 1.13 to 1.19 / 0.88 to 0.91 (expected 1.22 / 0.87); the
model's 384-channel 5x5 launch on the 29 x 50 map keeps its 12 splits of two chunks."""
import ctypes as C
import zlib

import numpy as np
import pytest

import conv_plan as CP
import convx_plan as XP
from test_gpu_convx import MEAN_GATE, RMS_GATE
from util import assert_close

pytestmark = pytest.mark.gpu

POOL = 8192       # outputs a gate ratio is taken over, at least
FORMS = {0: "bf16x6", 1: "f16x3"}
RATIOS = []       # every gate ratio of the file
WORST = {}        # (role, form) -> (largest error / bound, case)
GATE_WORST = {}   # (role, form) -> (largest gate ratio, case)
SLOPE = np.float32(0.25)


def _option(F, name, value=None):
    if value is None:
        v = C.c_int(0)
        F._lib.call("frcnn_get_option", name.encode(), C.byref(v))
        return v.value
    F._lib.call("frcnn_set_option", name.encode(), int(value))


@pytest.fixture
def options(F):
    """-> set(name, value); split_bf16 and x3_f16 are put back after the test"""
    before = {n: _option(F, n) for n in ("split_bf16", "x3_f16")}
    yield lambda name, value: _option(F, name, value)
    for n, v in before.items():
        _option(F, n, v)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _dev(F, a):
    return F.DeviceTensor.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _alloc_range(F, t):
    """(base, size) of the allocation a tensor lies in, asked of the runtime the library itself uses"""
    fn = F._lib.load().hipMemGetAddressRange
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    base, size = C.c_void_p(), C.c_size_t()
    assert fn(C.byref(base), C.byref(size), C.c_void_p(t.ptr)) == 0
    return base.value, size.value


class Placed(object):
    """a tensor at a chosen place of a NaN-filled allocation of its own (convx_plan.WG_PLACES; "offset" also for destinations)"""

    def __init__(self, F, a, place="slack"):
        a = np.ascontiguousarray(a, np.float32)
        n = a.size
        self.buf = F.DeviceTensor.empty((n + 8,))
        base, size = _alloc_range(F, self.buf)
        assert base == self.buf.ptr and base % 16 == 0 and size % 4 == 0
        total = size // 4                                    # floats the allocation really has
        self.first = {"slack": 0, "offset": 1, "exact": total - n}[place]
        self.n, self.total = n, total
        host = np.full(total, np.nan, np.float32)
        host[self.first:self.first + n] = a.ravel()
        whole = F.DeviceTensor(self.buf.ptr, (total,), owner=self.buf)
        whole.copy_from_numpy(host)
        self.whole = whole
        self.t = self.buf.offset_view(self.first, a.shape)
        past = base + size - (self.t.ptr + 4 * n)            # bytes of the allocation behind the tensor
        if place == "exact":
            assert past == 0 and self.t.ptr % 16 == 0
        else:
            assert past >= 16 and (self.t.ptr % 16 == 0) == (place == "slack")

    def read(self):
        """the tensor; everything around it must still be NaN"""
        host = self.whole.numpy()
        rest = np.concatenate([host[:self.first], host[self.first + self.n:]])
        assert np.isnan(rest).all(), "the launch wrote outside its destination"
        return host[self.first:self.first + self.n].reshape(self.t.shape)


def _dest(F, start, aligned=True):
    """a destination that starts at the values `start` (NaN for a storing call)"""
    return Placed(F, start, "slack" if aligned else "offset")


def _act(rng, mode, C_):
    """-> (slope, scale): PReLU slope and a dropout scale with kept (1), dropped (0) and halved channels; all entries <= 1,
    as the fp16 form wants them"""
    slope = SLOPE if mode in ("slope", "both") else None
    scale = None
    if mode in ("scale", "both"):
        scale = rng.choice(np.array([0.0, 0.5, 1.0, 1.0], np.float32), C_).astype(np.float32)
        scale[0], scale[-1] = 1.0, 0.0
    return slope, scale


def _amax_of_activated(x, slope):
    """the magnitude the fp16 form scales an activated operand by: the raw tensor's, times max(1, |slope|)"""
    return float(np.abs(x).max()) * max(1.0, abs(float(slope)) if slope is not None else 1.0)


class Gate(object):
    """squared errors of the split form and of the fp32 kernel, pooled over the repetitions of one case.  ratios / worst: the
    lists the ratio is recorded in (this file's; another file that uses the class passes its own)"""

    def __init__(self, ratios=None, worst=None):
        self.s = self.d = 0.0
        self.n = 0
        self.differ = False
        self.ratios = RATIOS if ratios is None else ratios
        self.worst = GATE_WORST if worst is None else worst

    def add(self, split, direct, want):
        self.s += float(((split.astype(np.float64) - want) ** 2).sum())
        self.d += float(((direct.astype(np.float64) - want) ** 2).sum())
        self.n += want.size
        self.differ |= not np.array_equal(split, direct)

    def ratio(self, role, form, what):
        """-> (ratio, passes); printed and recorded"""
        assert self.n >= POOL and self.differ, "%s %s: the option did not switch the kernel" % (role, what)
        es, ed = np.sqrt(self.s / self.n), np.sqrt(self.d / self.n)
        r = es / max(ed, 1e-30)
        self.ratios.append(r)
        key = (role, FORMS[form])
        if r > self.worst.get(key, (0.0, ""))[0]:
            self.worst[key] = (r, what)
        print("%s %s %s: rms error split / fp32 kernel = %.3f over %d outputs" % (role, FORMS[form], what, r, self.n))
        return r, es <= RMS_GATE * ed + 1e-9


def _gates(role, what, gates):
    """every form's ratio is printed before any is asserted"""
    got = {FORMS[form]: g.ratio(role, form, what) for form, g in sorted(gates.items())}
    bad = {f: round(r, 3) for f, (r, ok) in got.items() if not ok}
    assert not bad, "%s %s: rms error above %.2f times the fp32 kernel's: %r" % (role, what, RMS_GATE, bad)


def _check(role, form, what, got, want64, bound, worst=WORST):
    """all finite, the bar, the worst-case bound; worst: where the largest ratio per role and form is recorded"""
    assert got.shape == want64.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), "%s %s: not finite (an element was left out?)" % (role, what)
    err = np.abs(got.astype(np.float64) - want64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    key = (role, FORMS[form])
    if ratio > worst.get(key, (0.0, ""))[0]:
        worst[key] = (ratio, what)
    print("%s %s %s: max error / bound = %.4f" % (role, FORMS[form], what, ratio))
    assert_close(got, want64, 1e-4, "%s %s %s" % (role, FORMS[form], what))
    assert ratio <= 1.0, "%s %s %s: error %.3f times the bound" % (role, FORMS[form], what, ratio)


def _reps(outputs):
    return XP.cdiv(POOL, outputs)


def _run_id(r):
    extra = [k + ("" if v is True else "=%s" % v) for k, v in sorted(r.items()) if k not in ("role", "name", "shape")]
    return "-".join([r["role"], r["name"]] + extra)


# ---- forward ------------------------------------------------------------------------------------------------------------
def _forward(F, options, r):
    C_, H, W, O_, k, pad = r["shape"]
    plan = XP.x3_plan_of_run(r)
    mode, aligned = r.get("act"), r.get("out_aligned", True)
    what = _run_id(r)
    op = lambda a, b: CP.ref_forward(a, b, None, pad)   # noqa: E731
    gates = {form: Gate() for form in FORMS}
    for rep in range(_reps(O_ * plan["Ho"] * plan["Wo"])):
        rng = _rng("fwd", what, rep)
        x = rng.randn(C_, H, W).astype(np.float32)
        w = (rng.randn(O_, C_, k, k) / np.sqrt(C_ * k * k)).astype(np.float32)
        b = rng.randn(O_).astype(np.float32) if r["bias"] else None
        slope, scale = _act(rng, mode, C_)
        act = CP.activate(x, slope, scale)
        want = CP.ref_forward(act, w, b, pad)
        mag = CP.ref_forward(np.abs(act), np.abs(w), None if b is None else np.abs(b), pad)
        dx, dw = _dev(F, x), _dev(F, w)
        db = _dev(F, b) if b is not None else None
        da = _dev(F, [slope]) if slope is not None else None
        ds = _dev(F, scale) if scale is not None else None

        def call():
            out = _dest(F, np.full(want.shape, np.nan, np.float32), aligned)
            F._lib.call("frcnn_conv2d_forward", F.ptr(dx), C_, H, W, F.ptr(da), F.ptr(ds), F.ptr(dw), F.ptr(db), O_, k, pad,
                        F.ptr(out.t), F.stream_ptr())
            return out.read()
        options("split_bf16", 0)
        direct = call()
        assert_close(direct, want, 1e-4, "fp32 matrix-core forward %s (the gate's denominator)" % what)
        options("split_bf16", 1)
        for form in FORMS:
            options("x3_f16", form)
            got = call()
            rep_b = XP.representation_bound(op, act, w, form, amax_a=_amax_of_activated(x, slope) if mode else None)
            _check("forward", form, what, got, want, XP.split_bound(XP.PRODUCTS[form] * plan["K"], plan["splitK"], mag, rep_b))
            gates[form].add(got, direct, want)
    _gates("forward", what, gates)


X3_RUNS = XP.x3_runs()


@pytest.mark.parametrize("r", [r for r in X3_RUNS if r["role"] == "forward"], ids=_run_id)
def test_forward(F, options, r):
    _forward(F, options, r)


# ---- input gradient -------------------------------------------------------------------------------------------------------
def _gradient_inputs(rng, shape):
    """the launch of forward shape (C, H, W, O, k, pad) as an input gradient: the gradient map has C channels on H x W, the
    operator's weights are [C filters][O channels], its padding k - 1 - pad, and the result has O channels on Ho x Wo"""
    C_, H, W, O_, k, pad = shape
    g = rng.randn(C_, H, W).astype(np.float32)
    w = (rng.randn(C_, O_, k, k) / np.sqrt(C_ * k * k)).astype(np.float32)
    return g, w


def _input_gradient(F, options, r):
    C_, H, W, O_, k, pad = r["shape"]
    plan = XP.x3_plan_of_run(r)
    Ho, Wo, opad = plan["Ho"], plan["Wo"], k - 1 - pad
    add, aligned = r.get("add", False), r.get("out_aligned", True)
    what = _run_id(r)
    op = lambda a, b: CP.ref_input_gradient(a, b, opad, Ho, Wo)   # noqa: E731
    gates = {form: Gate() for form in FORMS}
    for rep in range(_reps(O_ * Ho * Wo)):
        rng = _rng("dgrad", what, rep)
        g, w = _gradient_inputs(rng, r["shape"])
        start = rng.randn(O_, Ho, Wo).astype(np.float32) if add else np.full((O_, Ho, Wo), np.nan, np.float32)
        want, mag = op(g, w), op(np.abs(g), np.abs(w))
        if add:
            want, mag = want + start, mag + np.abs(start)
        dg, dw = _dev(F, g), _dev(F, w)

        def call():
            gin = _dest(F, start, aligned)
            F._lib.call("frcnn_conv2d_backward_input", F.ptr(dg), C_, H, W, F.ptr(dw), O_, k, opad, F.ptr(gin.t), 1 if add else 0,
                        F.stream_ptr())
            return gin.read()
        options("split_bf16", 0)
        direct = call()
        assert_close(direct, want, 1e-4, "fp32 matrix-core input gradient %s (the gate's denominator)" % what)
        options("split_bf16", 1)
        for form in FORMS:
            options("x3_f16", form)
            got = call()
            rep_b = XP.representation_bound(op, g, w, form)
            _check("input_gradient", form, what, got, want, XP.split_bound(XP.PRODUCTS[form] * plan["K"], plan["splitK"], mag, rep_b))
            gates[form].add(got, direct, want)
    _gates("input_gradient", what, gates)


@pytest.mark.parametrize("r", [r for r in X3_RUNS if r["role"] == "input_gradient"], ids=_run_id)
def test_input_gradient(F, options, r):
    """accumulate = 1 adds to a destination that starts at random values"""
    _input_gradient(F, options, r)


# ---- input gradient through the fused activation backward ---------------------------------------------------------------------
@pytest.mark.parametrize("r", [r for r in X3_RUNS if r["role"] == "post"], ids=_run_id)
def test_input_gradient_fused_activation_backward(F, options, r):
    """frcnn_conv2d_backward_input_rec with post_x: gin = prelu'(x) scale[m] conv, gslope += sum over x <= 0 of x scale[m] conv
    (written out in fp64 below); gslope starts at a value that is not zero.  The entry point exists in the fp16 form only; the
    gate's denominator is the fp32 kernel's convolution put through the same two fp32 multiplications on the host."""
    C_, H, W, O_, k, pad = r["shape"]
    plan = XP.x3_plan_of_run(r)
    Ho, Wo, opad = plan["Ho"], plan["Wo"], k - 1 - pad
    what, form = _run_id(r), 1
    op = lambda a, b: CP.ref_input_gradient(a, b, opad, Ho, Wo)   # noqa: E731
    n, S = XP.PRODUCTS[form] * plan["K"], plan["splitK"]
    gate = Gate()
    options("x3_f16", 1)
    for rep in range(_reps(O_ * Ho * Wo)):
        rng = _rng("post", what, rep)
        g, w = _gradient_inputs(rng, r["shape"])
        px = rng.randn(O_, Ho, Wo).astype(np.float32)
        px[0, 0, 0] = 0.0                                   # x = 0 takes the slope's branch
        scale = rng.choice(np.array([0.0, 0.5, 1.0, 1.0], np.float32), O_).astype(np.float32) if r["post_scale"] else None
        gslope0 = np.float32(rng.randn() * 50.0)
        conv, mag = op(g, w), op(np.abs(g), np.abs(w))
        s64 = np.ones(O_) if scale is None else scale.astype(np.float64)
        fs = np.where(px > 0, 1.0, float(SLOPE)) * s64[:, None, None]
        want = fs * conv
        neg = px <= 0
        xs = np.abs(px.astype(np.float64)) * s64[:, None, None] * neg
        want_slope = float(gslope0) + float((px.astype(np.float64) * s64[:, None, None] * conv)[neg].sum())
        # the convolution's bound with two more roundings (x scale, x slope), scaled by the same factors
        conv_bound = XP.split_bound(n, S, mag, XP.representation_bound(op, g, w, form), extra=4)
        terms = int(neg.sum())
        slope_bound = float((xs * conv_bound).sum()) + (terms + 2) * CP.U * XP.MAG_SLACK * (float((xs * mag).sum()) + abs(float(gslope0)))
        dg, dw, dsl = _dev(F, g), _dev(F, w), _dev(F, [SLOPE])
        dsc = _dev(F, scale) if scale is not None else None
        dpx = Placed(F, px, "slack" if r["post_aligned"] else "offset")
        options("split_bf16", 0)
        plain = _dest(F, np.full(want.shape, np.nan, np.float32))
        F._lib.call("frcnn_conv2d_backward_input", F.ptr(dg), C_, H, W, F.ptr(dw), O_, k, opad, F.ptr(plain.t), 0, F.stream_ptr())
        gd = plain.read() if scale is None else (plain.read() * scale[:, None, None]).astype(np.float32)
        direct = np.where(px > 0, gd, SLOPE * gd).astype(np.float32)
        assert_close(direct, want, 1e-4, "fp32 matrix-core input gradient + activation backward %s (the gate's denominator)" % what)
        options("split_bf16", 1)
        gin = _dest(F, np.full(want.shape, np.nan, np.float32))
        gsl = _dev(F, [gslope0])
        F._lib.call("frcnn_conv2d_backward_input_rec", F.ptr(dg), C_, H, W, F.ptr(dw), O_, k, opad, F.ptr(gin.t), 0, None, None,
                    F.ptr(dpx.t), F.ptr(dsl), F.ptr(dsc), F.ptr(gsl), F.stream_ptr())
        got = gin.read()
        np.testing.assert_array_equal(dpx.read(), px)      # the launch only reads x
        _check("post_activation", form, what, got, want, np.abs(fs) * conv_bound)
        _check("slope_gradient", form, what, gsl.numpy(), np.array([want_slope]), np.array([slope_bound]))
        gate.add(got, direct, want)
    _gates("post_activation", what, {form: gate})


# ---- weight gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", XP.wg_runs(), ids=lambda r: "%s-%s" % (r["name"], r["act"]))
def test_weight_gradient_accumulates(F, options, r):
    """accGradParameters ADDS to gradWeight and gradBias: both start from random values.  The two tensors lie where the case's
    `place` says (convx_plan.WG_PLACES), which decides the loader."""
    C_, H, W, O_, k, pad = r["shape"]
    plan = XP.wgradx_plan(r["shape"])
    Ho, Wo = plan["Ho"], plan["Wo"]
    what = "%s act %s" % (r["name"], r["act"])
    rng = _rng("wgrad", what)
    x = rng.randn(C_, H, W).astype(np.float32)
    g = (rng.randn(O_, Ho, Wo) / np.sqrt(Ho * Wo)).astype(np.float32)
    gw0 = rng.randn(O_, C_, 3, 3).astype(np.float32)
    gb0 = rng.randn(O_).astype(np.float32)
    slope, scale = _act(rng, r["act"], C_)
    act = CP.activate(x, slope, scale)
    op = lambda a, b: CP.ref_weight_gradient(a, b, 3, pad)[0]   # noqa: E731
    gw64, gb64 = CP.ref_weight_gradient(act, g, 3, pad)
    mw, mb = CP.ref_weight_gradient(np.abs(act), np.abs(g), 3, pad)
    want, want_b = gw0 + gw64, gb0 + gb64
    dx, dg = Placed(F, x, r["place"]), Placed(F, g, r["place"])
    da = _dev(F, [slope]) if slope is not None else None
    ds = _dev(F, scale) if scale is not None else None

    def call():
        gw, gb = _dev(F, gw0), _dev(F, gb0)
        F._lib.call("frcnn_conv2d_backward_weight", F.ptr(dx.t), C_, H, W, F.ptr(da), F.ptr(ds), F.ptr(dg.t), O_, 3, pad, F.ptr(gw),
                    F.ptr(gb), F.stream_ptr())
        return gw.numpy(), gb.numpy()
    options("split_bf16", 0)
    direct, direct_b = call()
    assert_close(direct, want, 1e-4, "fp32 matrix-core weight gradient %s (the gate's denominator)" % what)
    assert_close(direct_b, want_b, 1e-4, "fp32 bias gradient %s" % what)
    options("split_bf16", 1)
    gates = {form: Gate() for form in FORMS}
    for form in FORMS:
        options("x3_f16", form)
        got, got_b = call()
        rep_b = XP.representation_bound(op, act, g, form, amax_a=_amax_of_activated(x, slope) if r["act"] else None)
        _check("weight_gradient", form, what, got, want,
               XP.split_bound(XP.PRODUCTS[form] * plan["K"], plan["nSplit"], mw + np.abs(gw0), rep_b))
        # the bias gradient is summed from the fp32 values of the staged gradient tiles: no representation error
        _check("bias_gradient", form, what, got_b, want_b, CP.rounding_bound(plan["K"], 1, mb + np.abs(gb0)))
        gates[form].add(got, direct, want)
    _gates("weight_gradient", what, gates)
    assert np.array_equal(dx.read(), x) and np.array_equal(dg.read(), g)


# ---- a caller-made record ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["short_last", "ragged_y_bm64"])
def test_forward_with_a_caller_made_record(F, options, name):
    """frcnn_conv2d_forward_rec with the input's magnitude record made by frcnn_tensor_absmax: the same bits as the entry point
    that takes the record itself"""
    C_, H, W, O_, k, pad = XP.find_x3(name)["shape"]
    rng = _rng("rec", name)
    x = rng.randn(C_, H, W).astype(np.float32)
    w = (rng.randn(O_, C_, k, k) / np.sqrt(C_ * k * k)).astype(np.float32)
    b = rng.randn(O_).astype(np.float32)
    options("split_bf16", 1)
    options("x3_f16", 1)
    dx, dw, db = _dev(F, x), _dev(F, w), _dev(F, b)
    rec = F.DeviceTensor.empty((F._lib.load().frcnn_amax_record_floats(),))
    F._lib.call("frcnn_tensor_absmax", F.ptr(dx), x.size, F.ptr(rec), F.stream_ptr())
    shape = (O_, H + 2 * pad - k + 1, W + 2 * pad - k + 1)
    a, c = _dest(F, np.full(shape, np.nan, np.float32)), _dest(F, np.full(shape, np.nan, np.float32))
    F._lib.call("frcnn_conv2d_forward_rec", F.ptr(dx), C_, H, W, None, None, F.ptr(dw), F.ptr(db), O_, k, pad, F.ptr(a.t), F.ptr(rec),
                None, F.stream_ptr())
    F._lib.call("frcnn_conv2d_forward", F.ptr(dx), C_, H, W, None, None, F.ptr(dw), F.ptr(db), O_, k, pad, F.ptr(c.t), F.stream_ptr())
    assert np.array_equal(a.read().view(np.uint32), c.read().view(np.uint32))


def test_zz_error_ratio_over_the_file(F):
    """Runs last (file order): the worst ratios per role and form, and over every comparison of the file the split forms' RMS
    error is, on the geometric mean, no larger than the fp32 matrix-core kernel's (MEAN_GATE of tests/test_gpu_convx.py)"""
    for key in sorted(WORST):
        print("largest error / bound, %s %s: %.4f (%s)" % (key + WORST[key]))
    for key in sorted(GATE_WORST):
        print("largest rms ratio split / fp32 kernel, %s %s: %.3f (%s)" % (key + GATE_WORST[key]))
    if len(RATIOS) >= 20:     # (a filtered session has too few comparisons for a mean to say anything)
        gm = float(np.exp(np.mean(np.log(np.maximum(RATIOS, 1e-12)))))
        print("split / fp32 kernel RMS error over %d comparisons: geometric mean %.3f, min %.3f, max %.3f" % (
            len(RATIOS), gm, min(RATIOS), max(RATIOS)))
        assert gm <= MEAN_GATE, (gm, len(RATIOS))
