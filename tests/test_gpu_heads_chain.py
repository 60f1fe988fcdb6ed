"""The anchor nets' sparse training chain op by op: the six kernels of csrc/heads.hip, the grouped product of csrc/gemm.hip
(gemm_f32_group / gemm_group_kernel) in every orientation, the K-split planner, and the per-net position helpers of
csrc/elem.hip, through the test-facing entry points of include/frcnn_hip_heads.h.  Those run the functions a training step
runs (heads_add_job, heads_chain_forward, heads_chain_backward_input, heads_chain_backward_params): there is no second copy of
the chain.  tests/heads_plan.py holds the case tables, says which path each case takes and computes the fp64 references;
tests/test_heads_plan.py checks tables and references without a GPU.

Every stored result goes to a destination filled with NaN inside a NaN-filled allocation (test_gpu_convx_plans.py::Placed: the
elements around a tensor must still be NaN afterwards); every accumulated one is added to random contents.

Stage by stage.  The caller owns the scratch, so COL, the slabs, HX, HY, OUT, D, GH and DX are read back and each stage is
compared with the fp64 reference computed FROM THE DEVICE'S OWN PREVIOUS STAGE: a PReLU branch is decided once, by the device's
HX.  Pure moves are bit-exact (COL, D, the scatter's addressing and its one addition, HY where HX > 0).  Products and sums meet
the project bar (util.assert_close, 1e-4) and conv_plan.rounding_bound = (K + S + 2) 2^-24 mag, with the roundings counted from
the code:
  slab s            K_s products of its run of K                                   rounding_bound(K_s, 0)
  HX                the bias plus S slabs in split order: S additions                rounding_bound(0, S)
  HY (HX <= 0)      one multiplication by the slope                                  rounding_bound(0, 0)
  OUT               n products                                                       rounding_bound(n, 0)
  gbias1, gbias3    P - 1 additions in the block (strided partials, the wave's shuffle tree, four wave sums), one atomic
                    onto the old contents                                            rounding_bound(0, P)
  GH                18 products, one multiplication by the slope                     rounding_bound(18, 1)
  gslope            the incoming gradient's 18 products each, a double sum rounded to fp32 per filter, n atomics
                                                                                     rounding_bound(18, n)
  DX                n products                                                       rounding_bound(n, 0)
  input gradient    one atomic per patch that covers the element (at most k k)       rounding_bound(0, patches)
  gw1, gw3          P products onto the old contents                                 rounding_bound(P, 0)
Exact-data runs: every tensor holds small integers (the slope is 1/4), test_heads_plan.py asserts on the reference that no sum
of magnitudes reaches 2^24 quarter units, so every output -- the atomically accumulated input gradient, gbias1, gbias3, gslope,
gw1 and gw3 included -- equals the fp64 reference bit for bit in any summation order: a lost, doubled or misplaced term shows.
Untouched memory: the output map off the positions stays NaN, the input gradient outside the patches keeps its bits, a net
without a gin keeps DX NaN, and nothing of a skipped net (P = 0) changes.

Not reached (heads_plan.CHAIN_NOT_REACHED): the 4096-block cap of the [n][P] and [18][P] kernels.

Measured on an MI355X, 2026-10-21 (every ratio is printed; the last test of the file prints the worst per stage), largest
error / bound:
  chain      slab 0.059 (forward_only net 0), HX 0.432 (mixed_p1_first net 3), HY 0.475 (no_gin net 3), OUT 0.105 (tiny_all net 0),
             gbias1 0.297 (gin_null net 2), GH 0.173 (mixed_p1_first net 1), gbias3 0.324 (mixed net 1), gslope 0.0036
             (mixed_p1_first net 0), DX 0.139 (tiny_all net 0), input gradient 0.510 (stride net 0), gw1 0.468 and gw3 0.569
             (mixed_p1_first net 0)
  product    store 0.317 (sizes_a job 0, 1 x 129 x 1), add 0.072 (sizes_b job 1), slab 0.322 (role_HX job 1 split 1)
  helpers    col2im_positions_add atomic 0.337 (mixed net 3), gathering 0.386 (mixed_p1_first net 1)
The two above 0.5 are bounds of three roundings that really hold two: gw3 and gw1 at P = 1 are one product added to the old
contents, and the input gradient's worst element lies under one patch (one atomic onto the old contents); half an ulp each of
two roundings against (K + S + 2) = 3 is 1/3 on average and up to 2/3.  The slab's 0.059 and gslope's 0.0036 are bounds over
hundreds of roundings (K_s up to 320 products; 18 + n with the sum carried in double) that a random walk stays far inside; none is
far below 1e-3.  Every exact-data comparison held bit for bit.
What this file found: no defect.  All 39 cases passed on their first run; the claim of gemm.hip that a job whose unit stride is
an accident of a dimension of 1 is computed correctly under job 0's flags holds in both directions (p1_first, p1_first_gh,
p1_later, role_OUT), and p1_first_gh shows that the <false, true> instantiation IS launched by a training step: the GH product
when the first net has one position."""
import ctypes as C

import numpy as np
import pytest

import conv_plan as CP
import gemm_plan as GP
import heads_plan as HP
from test_gpu_convx_plans import Placed, _option
from util import assert_close

pytestmark = pytest.mark.gpu

WORST = {}   # stage -> (largest error / bound, what)
NAN = np.float32(np.nan)


def _check(stage, what, got, want64, bound):
    """all finite, the bar, the worst-case bound; the ratio is printed before anything is asserted"""
    got = np.asarray(got)
    want64 = np.asarray(want64, np.float64)
    assert got.shape == want64.shape and got.dtype == np.float32, (stage, what, got.shape, want64.shape)
    if got.size == 0:
        return
    finite = bool(np.isfinite(got).all())
    err = np.abs(got.astype(np.float64) - want64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    # (err == 0 where the bound is 0 -- an all-zero sum -- is a ratio of 0, not 0 / 0)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if finite else float("inf")
    if ratio > WORST.get(stage, (-1.0, ""))[0]:
        WORST[stage] = (ratio, what)
    print("%s %s: max error / bound = %.4f" % (stage, what, ratio))
    assert finite, "%s %s: not finite (an element was left out?)" % (stage, what)
    assert_close(got, want64, 1e-4, "%s %s" % (stage, what))
    assert ratio <= 1.0, "%s %s: error %.3f times the bound" % (stage, what, ratio)


def _same(stage, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (stage, what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), "%s %s: %d of %d elements differ, first at %r" % (stage, what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))


def _launches(F, fn):
    """-> (return code of fn(), launches by kernel class name)"""
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        rc = fn()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return rc, {F._lib.KC_NAMES[i]: int(la[i]) for i in range(nk) if la[i]}


# ---- the grouped product ---------------------------------------------------------------------------------------------------------
def _gemm_table(F, jobs, data, where):
    """-> (ctypes table, the Placed operands per job)"""
    tab = (F._lib.GemmJob * max(1, len(jobs)))()
    held = []
    for i, (j, d) in enumerate(zip(jobs, data)):
        a, b = HP.gemm_layout(j, d["A"], d["B"])
        live = j["M"] > 0 and j["N"] > 0
        pa = Placed(F, a if a.size else np.full(8, NAN), where.get("x", "slack") if a.size else "slack")
        pb = Placed(F, b if b.size else np.full(8, NAN), where.get("w", "slack") if b.size else "slack")
        pc = Placed(F, d["C0"] if live else np.full(8, NAN), where.get("y", "slack") if live else "slack")
        sAm, sAk, sBk, sBn, ldc = HP.strides(j)
        q = tab[i]
        q.A, q.sAm, q.sAk, q.B, q.sBk, q.sBn, q.C, q.ldc = pa.t.ptr, sAm, sAk, pb.t.ptr, sBk, sBn, pc.t.ptr, ldc
        q.M, q.N, q.K, q.out_mode, q.splits = j["M"], j["N"], j["K"], 1 if j["add"] else 0, j["splits"]
        held.append((pa, pb, pc, a, b))
    return tab, held


@pytest.mark.parametrize("c", HP.GEMM_CASES, ids=lambda c: c["name"])
def test_gemm_group(F, c):
    """1 to 4 products in one launch of gemm_group_kernel, every orientation, sizes at the tile edges, K splits, ldc > N, jobs
    without blocks anywhere in the group, and a unit stride that is an accident of a dimension of 1"""
    jobs, data = c["jobs"], HP.gemm_inputs(c)
    tab, held = _gemm_table(F, jobs, data, GP.PLACINGS[c["placing"]])
    rc, la = _launches(F, lambda: F._lib.load().frcnn_gemm_group(tab, len(jobs), F.stream_ptr()))
    assert rc == 0, F._lib.load().frcnn_last_error()
    assert la == {"gemm": 1}, la
    for i, (j, d, (pa, pb, pc, a, b)) in enumerate(zip(jobs, data, held)):
        what = "%s job %d (%d x %d x %d %s)" % (c["name"], i, j["M"], j["N"], j["K"], j["orient"])
        got = pc.read()                       # (asserts that everything around the destination is still NaN)
        _same("operand", what, pa.read().ravel(), a.ravel() if a.size else np.full(8, NAN))
        _same("operand", what, pb.read().ravel(), b.ravel() if b.size else np.full(8, NAN))
        if not (j["M"] > 0 and j["N"] > 0):
            assert np.isnan(got).all(), "%s: a job without blocks wrote" % what
            continue
        want, mag, ks = HP.gemm_reference(j, d)
        if j["splits"] > 1:
            for s, k in enumerate(ks):        # K_s products per slab
                _check("gemm_group slab", "%s split %d" % (what, s), got[s], want[s], CP.rounding_bound(k, 0, mag[s]))
        else:                                  # K products (+ the old contents)
            _check("gemm_group add" if j["add"] else "gemm_group store", what, got[:, :j["N"]], want, CP.rounding_bound(j["K"], 0, mag))
            assert np.isnan(got[:, j["N"]:]).all(), "%s: the padding behind N was written" % what


def test_gemm_group_argument_errors(F):
    """0 or 5 jobs and splits that leave a run empty return an error before any launch"""
    for jobs, why in HP.GEMM_ERRORS:
        c = dict(name="error " + why, jobs=jobs)
        tab, held = _gemm_table(F, jobs, HP.gemm_inputs(c), {})
        rc, la = _launches(F, lambda: F._lib.load().frcnn_gemm_group(tab, len(jobs), F.stream_ptr()))
        assert rc != 0 and not la, (why, rc, la)
        for pa, pb, pc, a, b in held:
            got = pc.read()
            assert np.isnan(got).all(), why
    tab, _ = _gemm_table(F, [HP.gjob(8, 8, 32, "kn")], HP.gemm_inputs(dict(name="null", jobs=[HP.gjob(8, 8, 32, "kn")])), {})
    tab[0].C = None
    assert F._lib.load().frcnn_gemm_group(tab, 1, F.stream_ptr()) != 0


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
GRADS = ("gw3", "gbias3", "gslope", "gw1", "gbias1")


class DevNet(object):
    """one net's tensors on the device, each in a NaN-filled allocation of its own; a skipped net (P = 0) gets scratch for three
    positions, so that there is something that must not change"""

    def __init__(self, F, t, d, forward_only=False, tight_slab=0, splits=None):
        self.t, self.d = t, d
        P, n, ckk, hw = max(t["P"], 3) if t["P"] == 0 else t["P"], t["n"], t["ckk"], t["Ho"] * t["Wo"]
        self.S = S = splits or (HP.planned_splits(t) if t["P"] else 1)
        nan = lambda *shape: np.full(shape, NAN, np.float32)   # noqa: E731
        p = self.p = {}
        for name in ("inp", "w3", "bias3", "w1", "bias1", "delta"):
            p[name] = Placed(F, d[name])
        p["slope"] = Placed(F, np.array([d["slope"]], np.float32))
        self.pos = F.DeviceTensor.from_numpy(d["pos"] if len(d["pos"]) else np.zeros(4, np.int32))
        p["out"] = Placed(F, nan(HP.HEAD_OUT, hw))
        for name, shape in (("COL", (P, ckk)), ("HX", (n, P)), ("HY", (n, P)), ("OUT", (HP.HEAD_OUT, P)), ("D", (HP.HEAD_OUT, P)),
                            ("GH", (n, P)), ("DX", (P, ckk)), ("slab", (S, n, P))):
            p[name] = Placed(F, nan(*shape))
        self.start = dict(gin=d["gin0"], gw3=d["gw3_0"], gbias3=d["gbias3_0"], gslope=np.array([d["gslope0"]], np.float32),
                          gw1=d["gw1_0"], gbias1=d["gbias1_0"])
        for name, a in self.start.items():
            p[name] = Placed(F, a)
        self.forward_only = forward_only
        self.slab_floats = S * n * P - tight_slab

    def fill(self, q):
        t, p = self.t, self.p
        q.Cin, q.H, q.W, q.k, q.n, q.P, q.force_splits = t["Cin"], t["H"], t["W"], t["k"], t["n"], t["P"], t["force"]
        q.pos, q.in_ = self.pos.ptr, p["inp"].t.ptr
        for name in ("w3", "bias3", "slope", "w1", "bias1", "out", "COL", "HX", "HY", "OUT", "slab"):
            setattr(q, name, p[name].t.ptr)
        q.slab_floats = self.slab_floats
        if not self.forward_only:
            for name in GRADS + ("delta", "D", "GH"):
                setattr(q, name, p[name].t.ptr)
            if t["gin"]:
                q.gin, q.DX = p["gin"].t.ptr, p["DX"].t.ptr

    def read(self):
        return {name: pl.read() for name, pl in self.p.items()}

    def untouched(self, what):
        """a skipped net: every buffer as it was"""
        got = self.read()
        for name in ("out", "COL", "HX", "HY", "OUT", "D", "GH", "DX", "slab"):
            assert np.isnan(got[name]).all(), "%s: %s of a skipped net was written" % (what, name)
        for name, a in self.start.items():
            _same("skipped " + name, what, got[name].ravel(), a.ravel())


def _run_chain(F, nets, forward_only=False):
    """forward, then backward -> (split counts, launches of the forward, launches of the backward)"""
    L = F._lib.load()
    tab = (F._lib.HeadNet * len(nets))()
    for q, dn in zip(tab, nets):
        dn.fill(q)
    splits = (C.c_int * len(nets))()
    rc, fwd = _launches(F, lambda: L.frcnn_heads_chain_forward(tab, len(nets), splits, F.stream_ptr()))
    assert rc == 0, L.frcnn_last_error()
    bwd = None
    if not forward_only:
        rc, bwd = _launches(F, lambda: L.frcnn_heads_chain_backward(tab, len(nets), F.stream_ptr()))
        assert rc == 0, L.frcnn_last_error()
    return list(splits), fwd, bwd


def _expect_launches(c, fwd, bwd):
    live = [t for t in c["nets"] if t["P"] > 0]
    assert fwd == ({"elemwise": 3, "gemm": 2} if live else {}), fwd          # 5 launches
    if bwd is not None:
        gin = any(t["gin"] for t in live)
        assert bwd == ({"elemwise": 3, "gemm": 4} if gin else {"elemwise": 2, "gemm": 3}), bwd   # 7, or 5 when no net has a gin


def _check_forward_stages(what, dn, g):
    t, d, S = dn.t, dn.d, dn.S
    pos, n, hw = d["pos"], t["n"], t["Ho"] * t["Wo"]
    _same("COL", what, g["COL"], HP.ref_col(t, d["inp"], pos))
    sl, mg, runs = HP.ref_slabs(d["w3"], g["COL"], S)
    for s, k in enumerate(runs):
        _check("slab", "%s split %d of %d" % (what, s, S), g["slab"][s], sl[s], CP.rounding_bound(k, 0, mg[s]))
    hx, mag = HP.ref_hx(d["bias3"], g["slab"])
    _check("HX", what, g["HX"], hx, CP.rounding_bound(0, S, mag))
    hy = HP.ref_hy(g["HX"], d["slope"])
    _check("HY", what, g["HY"], hy, CP.rounding_bound(0, 0, np.abs(hy)))
    up = g["HX"] > 0
    _same("HY where HX > 0", what, g["HY"][up], g["HX"][up])
    assert up.any() and (~up).any(), "%s: one PReLU branch only" % what
    o, mag = HP.ref_out(d["w1"], g["HY"])
    _check("OUT", what, g["OUT"], o, CP.rounding_bound(n, 0, mag))
    want = np.full((HP.HEAD_OUT, hw), NAN, np.float32)
    want[:, pos] = g["OUT"] + d["bias1"][:, None]          # one fp32 addition: the scatter is bit-exact, and NaN off the positions
    _same("out map", what, g["out"], want)


def _check_backward_stages(what, dn, g):
    t, d = dn.t, dn.d
    pos, n, P, slope = d["pos"], t["n"], t["P"], d["slope"]
    a64 = lambda x: np.abs(np.asarray(x, np.float64))   # noqa: E731
    _same("D", what, g["D"], d["delta"][:, pos])
    D = g["D"].astype(np.float64)
    _check("gbias1", what, g["gbias1"], d["gbias1_0"] + D.sum(1), CP.rounding_bound(0, P, a64(d["gbias1_0"]) + np.abs(D).sum(1)))
    gh, mag, g0, mag0 = HP.ref_gh(d["w1"], g["D"], g["HX"], slope)
    _check("GH", what, g["GH"], gh, CP.rounding_bound(HP.HEAD_OUT, 1, mag))
    G = g["GH"].astype(np.float64)
    _check("gbias3", what, g["gbias3"], d["gbias3_0"] + G.sum(1), CP.rounding_bound(0, P, a64(d["gbias3_0"]) + np.abs(G).sum(1)))
    gs, gsm = HP.ref_gslope(g["HX"], g0, mag0)
    _check("gslope", what, g["gslope"], np.array([float(d["gslope0"]) + gs]), CP.rounding_bound(HP.HEAD_OUT, n, abs(float(d["gslope0"])) + gsm))
    if t["gin"]:
        _check("DX", what, g["DX"], G.T @ d["w3"].astype(np.float64), CP.rounding_bound(n, 0, np.abs(G).T @ a64(d["w3"])))
        gin, mag, cnt = HP.ref_col2im(t, g["DX"], pos, d["gin0"])
        assert cnt.max() <= t["k"] ** 2
        _check("input gradient", what, g["gin"], gin, CP.rounding_bound(0, cnt, mag))
        _same("input gradient outside the patches", what, g["gin"][cnt == 0], d["gin0"][cnt == 0])
    else:
        assert np.isnan(g["DX"]).all(), "%s: DX of a net without a gin was written" % what
        _same("input gradient of a net without one", what, g["gin"], d["gin0"])
    Y, X = g["HY"].astype(np.float64), g["COL"].astype(np.float64)
    _check("gw1", what, g["gw1"], d["gw1_0"] + D @ Y.T, CP.rounding_bound(P, 0, a64(d["gw1_0"]) + np.abs(D) @ np.abs(Y).T))
    _check("gw3", what, g["gw3"], d["gw3_0"] + G @ X, CP.rounding_bound(P, 0, a64(d["gw3_0"]) + np.abs(G) @ np.abs(X)))


@pytest.mark.parametrize("c", HP.CHAIN_CASES, ids=lambda c: c["name"])
def test_chain_stage_by_stage(F, c):
    """forward and backward of up to four nets in one chain, every stage against fp64 from the device's previous stage"""
    nets = [DevNet(F, t, HP.net_data(c, i), c["forward_only"], splits=t["force"] or None) for i, t in enumerate(c["nets"])]
    splits, fwd, bwd = _run_chain(F, nets, c["forward_only"])
    _expect_launches(c, fwd, bwd)
    assert splits == [HP.planned_splits(t) if t["P"] else 0 for t in c["nets"]], splits
    for i, dn in enumerate(nets):
        what = "%s net %d" % (c["name"], i)
        if dn.t["P"] == 0:
            dn.untouched(what)
            continue
        g = dn.read()
        _check_forward_stages(what, dn, g)
        if c["forward_only"]:
            for name in ("D", "GH", "DX"):
                assert np.isnan(g[name]).all(), (what, name)
            for name, a in dn.start.items():
                _same("forward only: " + name, what, g[name].ravel(), a.ravel())
        else:
            _check_backward_stages(what, dn, g)
        for name in ("inp", "w3", "bias3", "w1", "bias1", "delta"):
            _same("operand " + name, what, g[name], dn.d[name])


@pytest.mark.parametrize("c", [c for c in HP.CHAIN_CASES if c["exact"]], ids=lambda c: c["name"])
def test_chain_exact_data(F, c):
    """small integers throughout: every output equals the fp64 reference bit for bit, whatever the order of the atomics"""
    data = [HP.net_data(c, i, exact=True) for i in range(len(c["nets"]))]
    nets = [DevNet(F, t, d) for t, d in zip(c["nets"], data)]
    _, fwd, bwd = _run_chain(F, nets)
    _expect_launches(c, fwd, bwd)
    for i, dn in enumerate(nets):
        what = "%s net %d (exact)" % (c["name"], i)
        t, d = dn.t, dn.d
        if t["P"] == 0:
            dn.untouched(what)
            continue
        g, r = dn.read(), HP.reference(t, d)
        hw = t["Ho"] * t["Wo"]
        for name in ("COL", "HX", "HY", "OUT", "D", "GH", "gbias1", "gbias3", "gw1", "gw3"):
            _same(name, what, g[name], r[name].astype(np.float32))
        _same("gslope", what, g["gslope"], np.array([r["gslope"]], np.float32))
        want = np.full((HP.HEAD_OUT, hw), NAN, np.float32)
        want[:, d["pos"]] = r["out_at_pos"]
        _same("out map", what, g["out"], want)
        if t["gin"]:
            _same("DX", what, g["DX"], r["DX"].astype(np.float32))
            _same("input gradient", what, g["gin"], r["gin"].astype(np.float32))
        else:
            assert np.isnan(g["DX"]).all()
            _same("input gradient of a net without one", what, g["gin"], d["gin0"])


def test_chain_argument_errors(F):
    """a forced split count that leaves a run empty, a slab that is too small and a wrong number of nets are refused when the
    table is built: nothing is launched, nothing is written"""
    L = F._lib.load()
    c = HP.find("fold")
    for t, why in HP.CHAIN_ERRORS:
        dn = DevNet(F, t, HP.net_data(dict(name="error", nets=[t]), 0), splits=t["force"])
        tab = (F._lib.HeadNet * 1)()
        dn.fill(tab[0])
        rc, la = _launches(F, lambda: L.frcnn_heads_chain_forward(tab, 1, None, F.stream_ptr()))
        assert rc != 0 and not la, (why, rc, la)
        assert all(np.isnan(dn.p[name].read()).all() for name in ("COL", "slab", "HX", "out")), why
    t = c["nets"][0]
    for forced in (0, 11):    # the planner's 9 and a forced 11, each with a slab one float short
        tt = dict(t, force=forced)
        dn = DevNet(F, tt, HP.net_data(c, 0), tight_slab=1, splits=forced or None)
        tab = (F._lib.HeadNet * 1)()
        dn.fill(tab[0])
        rc, la = _launches(F, lambda: L.frcnn_heads_chain_forward(tab, 1, None, F.stream_ptr()))
        assert rc != 0 and not la and np.isnan(dn.p["slab"].read()).all(), (forced, rc, la)
    tab = (F._lib.HeadNet * 5)()
    assert L.frcnn_heads_chain_forward(tab, 0, None, F.stream_ptr()) != 0
    assert L.frcnn_heads_chain_forward(tab, 5, None, F.stream_ptr()) != 0 and L.frcnn_heads_chain_backward(tab, 5, F.stream_ptr()) != 0
    # every net skipped: no launch at all
    rc, la = _launches(F, lambda: L.frcnn_heads_chain_forward(tab, 4, None, F.stream_ptr()))
    assert rc == 0 and not la, (rc, la)
    rc, la = _launches(F, lambda: L.frcnn_heads_chain_backward(tab, 4, F.stream_ptr()))
    assert rc == 0 and not la, (rc, la)


# ---- the per-net helpers of elem.hip -----------------------------------------------------------------------------------------------
HELPER_NETS = [("mixed_p1_first", 1), ("mixed", 3), ("tiny_all", 0), ("mixed", 1)]


@pytest.fixture
def deterministic(F):
    before = _option(F, "deterministic")
    yield lambda v: _option(F, "deterministic", v)
    _option(F, "deterministic", before)


@pytest.mark.parametrize("name,i", HELPER_NETS, ids=lambda v: str(v))
def test_position_helpers(F, deterministic, name, i):
    """gather_positions and im2col_positions are pure moves (the gathered PReLU: one multiplication); col2im_positions_add in
    its atomic and its gathering form against the same reference, the gathering form bit-identical run to run, and on exact
    data both bit-identical to the reference"""
    c = HP.find(name)
    t = c["nets"][i]
    what = "%s net %d" % (name, i)
    d, dx = HP.net_data(c, i), HP.net_data(c, i, exact=True)
    pos, P, hw = d["pos"], t["P"], t["Ho"] * t["Wo"]
    dpos = F.DeviceTensor.from_numpy(pos)
    L = F._lib.load()
    # gather_positions, plain and with the activation
    src = Placed(F, d["delta"])
    dst, act = Placed(F, np.full((HP.HEAD_OUT, P), NAN)), Placed(F, np.full((HP.HEAD_OUT, P), NAN))
    slope = Placed(F, np.array([d["slope"]], np.float32))
    assert L.frcnn_gather_positions(src.t.ptr, HP.HEAD_OUT, hw, dpos.ptr, P, dst.t.ptr, None, None, F.stream_ptr()) == 0
    _same("gather_positions", what, dst.read(), d["delta"][:, pos])
    hxmap = HP.rng_of("helpers", name, i).randn(t["n"], hw).astype(np.float32)
    src2, dst2, act2 = Placed(F, hxmap), Placed(F, np.full((t["n"], P), NAN)), Placed(F, np.full((t["n"], P), NAN))
    assert L.frcnn_gather_positions(src2.t.ptr, t["n"], hw, dpos.ptr, P, dst2.t.ptr, slope.t.ptr, act2.t.ptr, F.stream_ptr()) == 0
    v = hxmap[:, pos]
    _same("gather_positions with slope", what, dst2.read(), v)
    _same("gather_positions activation", what, act2.read(), np.where(v > 0, v, d["slope"] * v).astype(np.float32))   # one fp32 product
    assert np.isnan(act.read()).all()
    # im2col_positions
    X, col = Placed(F, d["inp"]), Placed(F, np.full((P, t["ckk"]), NAN))
    assert L.frcnn_im2col_positions(X.t.ptr, t["Cin"], t["H"], t["W"], t["k"], t["Wo"], dpos.ptr, P, col.t.ptr, F.stream_ptr()) == 0
    _same("im2col_positions", what, col.read(), HP.ref_col(t, d["inp"], pos))
    # col2im_positions_add, both forms
    rng = HP.rng_of("col2im", name, i)
    for exact, dd in ((False, d), (True, dx)):
        DX = (rng.randint(-3, 4, size=(P, t["ckk"])) if exact else rng.randn(P, t["ckk"])).astype(np.float32)
        want, mag, cnt = HP.ref_col2im(t, DX, pos, dd["gin0"])
        assert not exact or mag.max() < 2 ** 24      # integers: every partial sum is exact in fp32
        dcol = Placed(F, DX)
        got = {}
        for form in (0, 1, 1):
            deterministic(form)
            gx = Placed(F, dd["gin0"])
            assert L.frcnn_col2im_positions_add(dcol.t.ptr, t["Cin"], t["H"], t["W"], t["k"], t["Wo"], dpos.ptr, P, gx.t.ptr,
                                                F.stream_ptr()) == 0
            g = gx.read()
            stage = "col2im_positions_add " + ("gathering" if form else "atomic")
            # atomic: one rounding per patch on the element; gathering: the patches summed in a register, then one addition
            _check(stage, "%s%s" % (what, " (exact)" if exact else ""), g, want, CP.rounding_bound(0, cnt, mag))
            _same(stage + " outside the patches", what, g[cnt == 0], dd["gin0"][cnt == 0])
            if form and form in got:
                _same("gathering form, run to run", what, g, got[form])
            got[form] = g
            if exact:
                _same(stage + " on exact data", what, g, want.astype(np.float32))
        _same("operand", what, dcol.read(), DX)


def test_zz_worst_ratios_of_the_file(F):
    """Runs last (file order): the worst ratio per stage"""
    for stage in sorted(WORST):
        print("largest error / bound, %s: %.4f (%s)" % ((stage,) + WORST[stage]))
