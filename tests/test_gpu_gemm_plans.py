"""The two products behind every nn.Linear of the classification net across their launch plans, through
frcnn_linear_forward / frcnn_linear_backward: csrc/gemm.hip (gemm_f32, option gemm_x_roles = 0) and csrc/gemmx.hip
(gemm_planes_kernel with split_planes_kernel and the slab fold, gemm_x_roles = 7, in both operand forms of option x3_f16:
three bf16 planes / two fp16 planes; the weight gradient with magnitude records of gY and X).  The entry points and the
classification net both run csrc/linear.h: what is tested here is what a training step executes
(tests/test_gpu_linear_shared.py compares the two bit for bit, tests/test_linear_host.py checks the launch sequences).
tests/gemm_plan.py holds the case tables and says which plan each case takes; tests/test_gemm_plan.py checks the tables
without a GPU.

Every stored result goes to a destination filled with NaN; the weight gradient and the bias gradient ADD to random contents.
Operands and destinations lie where the case's placing says (gemm_plan.PLACINGS; test_gpu_convx_plans.py::Placed): 16-byte
aligned, 4 bytes into a NaN-filled buffer whose other elements must stay NaN, or ending exactly where their allocation ends.

Every gemm_f32 result meets
  the project's bar     |a - b| <= 1e-4 max(1, |b|) against the fp64 reference;
  the rounding bound    |a - b| <= (K + S + 2) 2^-24 mag (conv_plan.rounding_bound: K products, S slabs, a bias or an
                        accumulating destination), mag = the same product on magnitudes (+ |bias|, + |destination|).
Every gemmx result meets
  the bar;
  the worst-case bound  convx_plan.split_bound with PRODUCTS[form] K kept plane products, S slabs and
                        convx_plan.representation_bound of its two operands (the records are the tensors' true maxima);
  the precision gate    its RMS error against fp64 is at most RMS_GATE = 2.0 times that of gemm_f32 on the same inputs
                        (the gate of tests/test_gpu_elem.py::test_linear_fc1_split_bf16_form), and the two results differ.
Inputs are drawn as the existing Linear tests draw them (x with a few decades of range downwards, gY / R); one case also runs
with activation operands that span twelve binades (every element of x and gY scaled by 2^-0 .. 2^-11), where the low fp16
plane loses bits: the representation term of the bound covers that.

Measured on an MI355X, 2026-10-20 (every ratio is printed; the last test of the file prints the worst per role and form):
  largest error / bound      gemm_f32: forward 0.052 (tile_plus_one), input gradient 0.362 (bbox_head: K = 4, a bound of seven
                             roundings), weight gradient 0.443 (tn128: K = 5), bias gradient 0.446 (one_row: two roundings).
                             gemmx, bf16x6 / f16x3: forward 0.0036 (dgrad_n_240) / 0.0051 (few_blocks), input gradient 0.0138 /
                             0.0187 (n_64), weight gradient 0.0234 (rp_32) / 0.0494 (rp_48), bias gradient 0.441.  The twelve
                             binades of short_last-wide stay at 0.0073 / 0.0113 (weight gradient) and below.  As in test_gpu_convx_plans.py the
                             bound is a worst case over n roundings: it notices a lost plane product or an element left out,
                             the gate notices lost precision.
  largest gate ratio         forward 0.935 bf16x6 (tile_heights, 64 rows), 0.808 f16x3 (short_last, wide); input gradient 1.878 /
                             1.287 (few_blocks: 4 slabs of 5088 against gemm_f32's 16 of 1280, expected sqrt(1908 / 640) = 1.73
                             and sqrt(954 / 640) = 1.22); weight gradient 1.573 / 1.161 (n_tail_240, 2 slabs of 1008 against 7 of
                             288: expected 1.62 / 1.15).
What this file found, both in the planner of gemmx.hip and neither a lost product (every case met its bound throughout):
  The weight gradient never split K.  n_tail_240 = (2000, 1040, 496) in the three-plane form missed the gate with 2.237 (f16x3:
  1.609): one slab of 2000 rows where gemm_f32, with few tiles, folds 7 slabs of 288.  By the count of test_gpu_convx_plans.py
  -- the RMS rounding error grows with the square root of the roundings per slab; 0.375 per product with six plane products,
  0.1875 with three, 0.5 in gemm_f32 -- that is sqrt(750 / 144) = 2.28 and sqrt(375 / 144) = 1.61.  n_64 (1136 rows) and n_lt_256
  (1104) measured 1.69 and 1.68.  linear_x_wgrad now asks for one slab per 1024 rows of k: at most 384 roundings against
  gemm_f32's 128 at its 256-value floor, sqrt(3) = 1.73; a training step (a few hundred rows) keeps its single slab.
  A forced tile height that the operand form does not have (FRCNN_GX_TM = 256 with fp32 weights) left gx_plan without a
  candidate, and forward and input gradient ran gx_run's defaults, 128 rows and ONE slab of any K, where
  tests/test_gpu_elem.py says they keep their own choice: rp_32 with 256 forced measured 3.522 bf16x6 / 2.497 f16x3 in the
  forward (one slab of 13824 against 16 of 864: sqrt(12) = 3.46, sqrt(6) = 2.45) and 2.524 in the input gradient; tile_heights
  2.04 in both.  Such a height now forces nothing.  The same run showed that (33, 13824, 1024) of that file, its "less than
  one tile" case, is below the split form's size floor and runs gemm_f32: rp_32 / rp_48 / few_rows here are the split
  kernels' first runs with fewer rows than a tile."""
import numpy as np
import pytest

import conv_plan as CP
import convx_plan as XP
import gemm_plan as GP
from test_gpu_convx_plans import Placed, _option, _rng
from util import assert_close

pytestmark = pytest.mark.gpu

RMS_GATE = 2.0    # tests/test_gpu_elem.py::test_linear_fc1_split_bf16_form
WORST = {}        # (kernel, role) -> (largest error / bound, case)
GATE_WORST = {}   # (role, form) -> (largest gate ratio, case)
ROLE_OF = {"y": "forward", "gx": "input_gradient", "gw": "weight_gradient"}


@pytest.fixture
def options(F):
    """-> set(name, value); x3_f16 is put back after the test, gemm_x_roles goes back to the built-in rule"""
    before = _option(F, "x3_f16")
    yield lambda name, value: _option(F, name, value)
    _option(F, "x3_f16", before)
    _option(F, "gemm_x_roles", -1)


# ---- inputs and fp64 references, made once per case ----------------------------------------------------------------------------
_REFS = {}   # the references of the case that ran last (the runs of a case follow each other)


def _refs(kind, name, shape, wide=False):
    """inputs, fp64 references and the same products on magnitudes of one case; read-only, shared by the case's runs"""
    key = (kind, name, wide)
    if key in _REFS:
        return _REFS[key]
    _REFS.clear()
    x, w, b, gy, gw0, gb0 = GP.linear_inputs(_rng("linear", kind, name, wide), shape, wide)
    x64, w64, g64 = x.astype(np.float64), w.astype(np.float64), gy.astype(np.float64)
    ax, aw, ag = np.abs(x64), np.abs(w64), np.abs(g64)
    want = dict(y=x64 @ w64.T + b, gx=g64 @ w64, gw=gw0 + g64.T @ x64, gb=gb0 + g64.sum(0))
    mag = dict(y=ax @ aw.T + np.abs(b), gx=ag @ aw, gw=np.abs(gw0) + ag.T @ ax, gb=np.abs(gb0) + ag.sum(0))
    ref = dict(shape=shape, x=x, w=w, b=b, gy=gy, gw0=gw0, gb0=gb0, want=want, mag=mag, rep={})
    for a in (x, w, b, gy, gw0, gb0):
        a.setflags(write=False)
    _REFS[key] = ref
    return ref


OPS = {"y": lambda a, b: a @ b.T, "gx": lambda a, b: a @ b, "gw": lambda a, b: a.T @ b}
OPERANDS = {"y": ("x", "w"), "gx": ("gy", "w"), "gw": ("gy", "x")}


def _representation(ref, out, form):
    key = (out, form)
    if key not in ref["rep"]:
        a, b = OPERANDS[out]
        ref["rep"][key] = XP.representation_bound(OPS[out], ref[a], ref[b], form)
    return ref["rep"][key]


# ---- one forward + backward -----------------------------------------------------------------------------------------------------
class Operands(object):
    """x, w, b and gy on the device where the placing says; checked unchanged at the end"""

    def __init__(self, F, ref, placing):
        self.ref, self.placing = ref, placing
        self.where = GP.PLACINGS[placing]
        self.t = {n: Placed(F, ref[n], self.where.get(n, "slack")) for n in ("x", "w", "b", "gy")}
        for n, p in self.t.items():   # the tensors lie as gemm_plan.starts_aligned assumes
            assert (p.t.ptr % 16 == 0) == GP.starts_aligned(placing, n, ref["shape"]), (n, placing)

    def run(self, F, roles=GP.ROLES):
        """-> dict(y, gx, gw, gb) of the roles asked for: frcnn_linear_forward, then frcnn_linear_backward"""
        ref = self.ref
        R, I, O = ref["shape"]
        t, out = self.t, {}
        place = lambda n, a: Placed(F, a, self.where.get(n, "slack"))   # noqa: E731
        if "forward" in roles:
            y = place("y", np.full((R, O), np.nan, np.float32))
            F._lib.call("frcnn_linear_forward", F.ptr(t["x"].t), R, I, F.ptr(t["w"].t), F.ptr(t["b"].t), O, F.ptr(y.t), F.stream_ptr())
            out["y"] = y.read()
        gx = place("gx", np.full((R, I), np.nan, np.float32)) if "input_gradient" in roles else None
        gw = place("gw", ref["gw0"]) if "weight_gradient" in roles else None
        gb = place("gb", ref["gb0"])
        if gx is not None or gw is not None:
            F._lib.call("frcnn_linear_backward", F.ptr(t["x"].t), F.ptr(t["gy"].t), R, I, F.ptr(t["w"].t), O,
                        F.ptr(gx.t) if gx is not None else None, F.ptr(gw.t) if gw is not None else None, F.ptr(gb.t), F.stream_ptr())
            out["gb"] = gb.read()
            if gx is not None:
                out["gx"] = gx.read()
            if gw is not None:
                out["gw"] = gw.read()
        return out

    def unchanged(self):
        for n, p in self.t.items():
            assert np.array_equal(p.read(), self.ref[n]), "the launch wrote to its operand %s" % n


def _check(kernel, out, what, got, want64, bound):
    """all finite, the bar, the worst-case bound; the ratio is printed before anything is asserted"""
    assert got.shape == want64.shape and got.dtype == np.float32
    role = ROLE_OF.get(out, "bias_gradient")
    finite = bool(np.isfinite(got).all())
    err = np.abs(got.astype(np.float64) - want64)
    ratio = float(np.nanmax(err / np.maximum(bound, 1e-300))) if finite else float("inf")
    key = (kernel, role)
    if ratio > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (ratio, what)
    print("%s %s %s: max error / bound = %.4f" % (kernel, role, what, ratio))
    assert finite, "%s %s %s: not finite (an element was left out?)" % (kernel, role, what)
    assert_close(got, want64, 1e-4, "%s %s %s" % (kernel, role, what))
    assert ratio <= 1.0, "%s %s %s: error %.3f times the bound" % (kernel, role, what, ratio)


def _rms(got, want64):
    return float(np.sqrt(np.mean((got.astype(np.float64) - want64) ** 2)))


# ---- gemm_f32 -------------------------------------------------------------------------------------------------------------------
def _f32_id(r):
    return "%s-%s" % (r["name"], r["placing"])


@pytest.mark.parametrize("r", GP.f32_runs(), ids=_f32_id)
def test_gemm_f32(F, options, r):
    """the three products of Linear(R, I, O) on the fp32 matrix-core kernels of gemm.hip (gemm_plan.f32_plan says which)"""
    what = _f32_id(r)
    ref = _refs("f32", r["name"], r["shape"])
    plans = {p["role"]: p for p in GP.f32_plans_of_run(r)}
    options("gemm_x_roles", 0)
    ops = Operands(F, ref, r["placing"])
    got = ops.run(F, r["roles"])
    ops.unchanged()
    for out in ("y", "gx", "gw"):
        p = plans.get(ROLE_OF[out])
        if p is not None:
            _check("gemm_f32", out, what, got[out], ref["want"][out], CP.rounding_bound(p["K"], p["splitK"], ref["mag"][out]))
    if "gb" in got:   # fp64 column sums, rounded once into the fp32 destination
        _check("gemm_f32", "gb", what, got["gb"], ref["want"]["gb"], CP.rounding_bound(0, 0, ref["mag"]["gb"]))


# ---- gemmx ------------------------------------------------------------------------------------------------------------------------
def _gx_id(r):
    return "%s-%s%s" % (r["name"], "tm%d" % r["tm"] if r["tm"] else "planned", "-wide" if r["wide"] else "")


@pytest.mark.parametrize("r", GP.gx_runs(), ids=_gx_id)
def test_gemmx(F, options, monkeypatch, r):
    """the three products in the split form, both operand forms, against fp64, their bound and gemm_f32 on the same inputs"""
    what = _gx_id(r)
    if r["tm"] is not None:
        monkeypatch.setenv("FRCNN_GX_TM", str(r["tm"]))
    ref = _refs("gx", r["name"], r["shape"], r["wide"])
    R = r["shape"][0]
    ops = Operands(F, ref, r["placing"])
    options("gemm_x_roles", 0)
    direct = ops.run(F)
    for out in ("y", "gx", "gw"):
        assert_close(direct[out], ref["want"][out], 1e-4, "gemm_f32 %s %s (the gate's denominator)" % (ROLE_OF[out], what))
    options("gemm_x_roles", 7)
    gates = {}
    for form, fname in sorted(GP.FORMS.items()):
        options("x3_f16", form)
        got = ops.run(F)
        for out in ("y", "gx", "gw"):
            role = ROLE_OF[out]
            p = GP.gx_launch(role, r["shape"], form, r["tm"])
            k = R if out == "gw" else p["K"]     # (the padded rows of k are exact zeros)
            bound = XP.split_bound(XP.PRODUCTS[form] * k, p["splitK"], ref["mag"][out], _representation(ref, out, form))
            _check("gemmx " + fname, out, what, got[out], ref["want"][out], bound)
            es, ed = _rms(got[out], ref["want"][out]), _rms(direct[out], ref["want"][out])
            ratio = es / max(ed, 1e-30)
            if ratio > GATE_WORST.get((role, fname), (0.0, ""))[0]:
                GATE_WORST[(role, fname)] = (ratio, what)
            print("%s %s %s: rms error split %.3e / gemm_f32 %.3e = %.3f (TM %d, %d slabs of %d)" % (
                role, fname, what, es, ed, ratio, p["TM"], p["splitK"], p["kPerSplit"]))
            gates[(role, fname)] = (ratio, es <= RMS_GATE * ed + 1e-12, not np.array_equal(got[out], direct[out]))
        _check("gemmx " + fname, "gb", what, got["gb"], ref["want"]["gb"], CP.rounding_bound(0, 0, ref["mag"]["gb"]))
    ops.unchanged()
    same = sorted(k for k, g in gates.items() if not g[2])
    assert not same, "%s: the split form was not taken: %r" % (what, same)
    bad = {k: round(g[0], 3) for k, g in gates.items() if not g[1]}
    assert not bad, "%s: rms error above %.1f times gemm_f32's: %r" % (what, RMS_GATE, bad)


def test_zz_worst_ratios_of_the_file(F):
    """Runs last (file order): the worst ratios per kernel and role"""
    for key in sorted(WORST):
        print("largest error / bound, %s %s: %.4f (%s)" % (key + WORST[key]))
    for key in sorted(GATE_WORST):
        print("largest rms ratio split / gemm_f32, %s %s: %.3f (%s)" % (key + GATE_WORST[key]))
    _REFS.clear()
