"""optim.sgd and optim.nag (main.lua:122-124 sgd_state / nag_state, main.lua:134-135) on the device: frcnn_sgd / frcnn_nag and
their slice forms, the look-ahead, the folded gradient:div (objective.lua:200) and the Python optimisers F.sgd / F.nag; and
optim.rmsprop's kernel (main.lua:133), which runs through the same range kernel as those two.

The reference is a numpy fp32 restatement of Torch's optim functions: one separately rounded numpy operation per Lua statement
(numpy never contracts to FMA), host scalars in double as Lua computes them, passed as fp32.  Comparisons are bit for bit,
signed zeros included."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32

MAIN_SGD = dict(learningRate=1e-3, weightDecay=0.0005, momentum=0.9)     # main.lua:122-123
MAIN_NAG = dict(learningRate=1e-3, weightDecay=0, momentum=0.9)          # main.lua:124 (momentum = opt.rms_decay, 0.9)
SGD_CFGS = {
    "plain": dict(learningRate=1e-2),
    "main_lua": MAIN_SGD,
    "nesterov": dict(learningRate=1e-2, momentum=0.9, dampening=0, nesterov=True, weightDecay=1e-4),
    "dampening": dict(learningRate=1e-2, momentum=0.9, dampening=0.5),
    "lrd": dict(learningRate=1e-2, learningRateDecay=0.25, momentum=0.5, weightDecay=1e-3),
}
NAG_CFGS = {"main_lua": MAIN_NAG, "wd": dict(MAIN_NAG, weightDecay=5e-4)}


# ---------------------------------------------------------------- the restatement
def sgd_scalars(cfg, nevals):
    lr = cfg.get("learningRate", 1e-3); lrd = cfg.get("learningRateDecay", 0)
    mom = cfg.get("momentum", 0); damp = cfg.get("dampening", mom)
    return dict(clr=lr / (1 + nevals * lrd), wd=cfg.get("weightDecay", 0), mom=mom, omd=1 - damp,
                nesterov=bool(cfg.get("nesterov", False)))


def nag_scalars(cfg, nevals):
    lr = cfg.get("learningRate", 1e-3); lrd = cfg.get("learningRateDecay", 0)
    return dict(clr=lr / (1 + nevals * lrd), wd=cfg.get("weightDecay", 0), mom=cfg.get("momentum", 0.9))


def ref_sgd(x, g, v, gscale, s, first):
    """optim.sgd after opfunc: -> x, g, v as Torch leaves them"""
    if gscale is not None:
        g = g * f32(gscale)                          # gradient:div(n)
    if s["wd"] != 0:
        g = g + f32(s["wd"]) * x                     # dfdx:add(wd, x)
    d = g
    if s["mom"] != 0:
        if first:
            v = g.copy()                             # state.dfdx = ...:copy(dfdx)
        else:
            v = v * f32(s["mom"]) + f32(s["omd"]) * g   # state.dfdx:mul(mom):add(1-damp, dfdx)
        if s["nesterov"]:
            g = g + f32(s["mom"]) * v                # dfdx:add(mom, state.dfdx)
            d = g
        else:
            d = v
    x = x + f32(-s["clr"]) * d                       # x:add(-clr, dfdx)
    return x, g, v


def ref_lookahead(x, v, mom):
    return x + f32(mom) * v                          # x:add(mom, state.dfdx)


def ref_nag(x, g, v, gscale, s, first):
    """optim.nag after its look-ahead and opfunc: -> x, g, v"""
    if gscale is not None:
        g = g * f32(gscale)
    if s["wd"] != 0:
        g = g + f32(s["wd"]) * x
    v = np.zeros_like(g) if first else v * f32(s["mom"])   # fill(0) | mul(mom)
    v = v + f32(-s["clr"]) * g                       # add(-clr, dfdx)
    x = x + v                                        # x:add(state.dfdx)
    return x, g, v


RMS = dict(lr=1e-3, alpha=0.9, eps=1e-8)


def ref_rmsprop(x, g, m, gscale, s, first=None):
    """optim.rmsprop after opfunc: -> x, g, m (fp32 divide and square root are correctly rounded, here and on the device)"""
    if gscale is not None:
        g = g * f32(gscale)                          # gradient:div(n)
    m = f32(s["alpha"]) * m + (f32(1) - f32(s["alpha"])) * (g * g)
    x = x - f32(s["lr"]) * g / (np.sqrt(m) + f32(s["eps"]))
    return x, g, m


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _gradient(rng, n):
    g = (rng.randn(n) * 3.0).astype(np.float32)
    g[::7] = 0.0                                     # signed zeros: 0 * anything, 0 + -0
    g[3::11] = -0.0
    return g


# ---------------------------------------------------------------- device calls
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _sgd_call(F, x, g, v, gscale, s, first, gcount=None, lo=None, hi=None):
    args = (s["wd"], s["mom"], s["omd"], int(s["nesterov"]), int(first))
    if lo is None:
        F._lib.call("frcnn_sgd", F.ptr(x), F.ptr(g), F.ptr(v), x.numel(), gscale, F.ptr(gcount), s["clr"], *args, F.stream_ptr())
    else:
        F._lib.call("frcnn_sgd_slice", F.ptr(x), F.ptr(g), F.ptr(v), lo, hi, gscale, s["clr"], *args, F.stream_ptr())


def _nag_call(F, x, g, v, gscale, s, first, gcount=None, lo=None, hi=None):
    args = (s["wd"], s["mom"], int(first))
    if lo is None:
        F._lib.call("frcnn_nag", F.ptr(x), F.ptr(g), F.ptr(v), x.numel(), gscale, F.ptr(gcount), s["clr"], *args, F.stream_ptr())
    else:
        F._lib.call("frcnn_nag_slice", F.ptr(x), F.ptr(g), F.ptr(v), lo, hi, gscale, s["clr"], *args, F.stream_ptr())


def _rmsprop_call(F, x, g, m, gscale, s, first=None, gcount=None, lo=None, hi=None, unscaled_entry=False):
    args = (s["lr"], s["alpha"], s["eps"], F.stream_ptr())
    if unscaled_entry:
        F._lib.call("frcnn_rmsprop", F.ptr(x), F.ptr(g), F.ptr(m), x.numel(), *args)
    elif lo is None and gcount is None:
        F._lib.call("frcnn_scale_rmsprop", F.ptr(x), F.ptr(g), gscale, F.ptr(m), x.numel(), *args)
    elif lo is None:
        F._lib.call("frcnn_scale_rmsprop_dev", F.ptr(x), F.ptr(g), F.ptr(gcount), F.ptr(m), x.numel(), *args)
    elif gcount is None:
        F._lib.call("frcnn_scale_rmsprop_slice", F.ptr(x), F.ptr(g), gscale, F.ptr(m), lo, hi, *args)
    else:
        F._lib.call("frcnn_scale_rmsprop_slice_dev", F.ptr(x), F.ptr(g), F.ptr(gcount), F.ptr(m), lo, hi, *args)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1_000_003])
@pytest.mark.parametrize("gscale", [1.0 / 41.0, 1.0])
@pytest.mark.parametrize("name", sorted(SGD_CFGS))
def test_sgd_kernel_matches_the_restatement(F, name, gscale, n):
    """three consecutive steps (the first creates state.dfdx): x, g and v bit for bit"""
    import torch
    cfg = SGD_CFGS[name]
    rng = np.random.RandomState(n % 1000 + 7)
    x_ref = rng.randn(n).astype(np.float32)
    x = _dev(x_ref)
    mom = cfg.get("momentum", 0)
    v = torch.empty_like(x) if mom != 0 else None
    v_ref = None
    for k in range(3):
        s = sgd_scalars(cfg, k)
        g_in = _gradient(rng, n)
        g = _dev(g_in)
        _sgd_call(F, x, g, v, gscale, s, k == 0)
        x_ref, g_ref, v_ref = ref_sgd(x_ref, g_in, v_ref, gscale if gscale != 1.0 else None, s, k == 0)
        assert same_bits(_host(x), x_ref), "x after step %d" % k
        assert same_bits(_host(g), g_ref), "g after step %d" % k
        if mom != 0:
            assert same_bits(_host(v), v_ref), "v after step %d" % k


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1_000_003])
@pytest.mark.parametrize("gscale", [1.0 / 41.0, 1.0])
@pytest.mark.parametrize("name", sorted(NAG_CFGS))
def test_nag_kernel_matches_the_restatement(F, name, gscale, n):
    """three steps with the look-ahead in front of every step after the first: x, g and v bit for bit"""
    import torch
    cfg = NAG_CFGS[name]
    rng = np.random.RandomState(n % 1000 + 11)
    x_ref = rng.randn(n).astype(np.float32)
    x = _dev(x_ref)
    v = torch.empty_like(x)
    v_ref = None
    for k in range(3):
        s = nag_scalars(cfg, k)
        if k > 0:
            F._lib.call("frcnn_nag_lookahead", F.ptr(x), F.ptr(v), n, s["mom"], F.stream_ptr())
            x_ref = ref_lookahead(x_ref, v_ref, s["mom"])
            assert same_bits(_host(x), x_ref), "x after the look-ahead of step %d" % k
        g_in = _gradient(rng, n)
        g = _dev(g_in)
        _nag_call(F, x, g, v, gscale, s, k == 0)
        x_ref, g_ref, v_ref = ref_nag(x_ref, g_in, v_ref, gscale if gscale != 1.0 else None, s, k == 0)
        assert same_bits(_host(x), x_ref), "x after step %d" % k
        assert same_bits(_host(g), g_ref), "g after step %d" % k
        assert same_bits(_host(v), v_ref), "v after step %d" % k


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1_000_003])
@pytest.mark.parametrize("gscale", [1.0 / 41.0, 1.0])
def test_rmsprop_kernel_matches_the_restatement(F, gscale, n):
    """three consecutive steps from m = 0 (as optim.rmsprop creates it): x, g and m bit for bit from frcnn_scale_rmsprop, and
    from frcnn_rmsprop where the gradient is unscaled; a scale of exactly 1 leaves g's bits alone"""
    entries = (False,) if gscale != 1.0 else (False, True)      # frcnn_scale_rmsprop | frcnn_rmsprop
    rng = np.random.RandomState(n % 1000 + 13)
    x_ref = rng.randn(n).astype(np.float32)
    m_ref = np.zeros(n, np.float32)
    xs = [_dev(x_ref) for _ in entries]
    ms = [_dev(m_ref) for _ in entries]
    for k in range(3):
        g_in = _gradient(rng, n)
        x_ref, g_ref, m_ref = ref_rmsprop(x_ref, g_in, m_ref, gscale if gscale != 1.0 else None, RMS)
        for x, m, unscaled_entry in zip(xs, ms, entries):
            g = _dev(g_in)
            _rmsprop_call(F, x, g, m, gscale, RMS, unscaled_entry=unscaled_entry)
            what = "frcnn_rmsprop" if unscaled_entry else "frcnn_scale_rmsprop"
            assert same_bits(_host(x), x_ref), "x after step %d of %s" % (k, what)
            assert same_bits(_host(g), g_ref), "g after step %d of %s" % (k, what)
            assert same_bits(_host(m), m_ref), "m after step %d of %s" % (k, what)
            if gscale == 1.0:
                assert same_bits(_host(g), g_in), "g changed by step %d of %s" % (k, what)


@pytest.mark.parametrize("form", ["whole", "slice"])
@pytest.mark.parametrize("opt", ["rmsprop", "sgd_main_lua"])
def test_a_grid_that_wraps_matches_the_restatement(F, opt, form):
    """the grid-stride loop takes a second turn: one block's worth of 16-byte groups above the grid's cap (2048 blocks for the
    whole vector, 1024 for a slice), a three-element tail on the whole vector, ragged ends on both sides of the slice.
    x, g and v bit for bit against the restatement inside the range, untouched outside it"""
    n = 4 * (2048 * 256 + 256) + 3
    lo, hi = (0, n) if form == "whole" else (5, 5 + 3 + 4 * (1024 * 256 + 256) + 2)
    rng = np.random.RandomState(17)
    x0 = rng.randn(n).astype(np.float32); g0 = _gradient(rng, n); v0 = rng.rand(n).astype(np.float32)
    gscale = 1.0 / 41.0
    if opt == "rmsprop":
        s, call, ref = RMS, _rmsprop_call, ref_rmsprop
    else:
        s, call, ref = sgd_scalars(MAIN_SGD, 4), _sgd_call, ref_sgd
    x, g, v = _dev(x0), _dev(g0), _dev(v0)
    if form == "whole":
        call(F, x, g, v, gscale, s, False)
    else:
        call(F, x, g, v, gscale, s, False, lo=lo, hi=hi)
    want = [a.copy() for a in (x0, g0, v0)]
    for w, r in zip(want, ref(x0[lo:hi], g0[lo:hi], v0[lo:hi], gscale, s, False)):
        w[lo:hi] = r
    for t, w, a0, what in zip((x, g, v), want, (x0, g0, v0), ("x", "g", "v")):
        got = _host(t)
        assert same_bits(got[lo:hi], w[lo:hi]), "%s differs from the restatement" % what
        assert same_bits(got[:lo], a0[:lo]) and same_bits(got[hi:], a0[hi:]), "%s changed outside [%d, %d)" % (what, lo, hi)
    assert not same_bits(_host(x)[lo:hi], x0[lo:hi])


def test_nag_first_step_adds_to_a_literal_zero(F):
    """fill(0):add(-clr, dfdx): a zero gradient leaves +0 in v (0 + -0), never -0"""
    import torch
    x = _dev(np.ones(8, np.float32))
    g = _dev(np.zeros(8, np.float32))
    v = torch.full_like(x, -1.0)
    _nag_call(F, x, g, v, 1.0, nag_scalars(MAIN_NAG, 0), True)
    assert same_bits(_host(v), np.zeros(8, np.float32)) and same_bits(_host(x), np.ones(8, np.float32))


@pytest.mark.parametrize("opt", ["sgd_main_lua", "sgd_nesterov", "nag_main_lua", "nag_wd", "rmsprop"])
def test_slices_tile_the_whole_vector_bit_for_bit(F, opt):
    """the slice form over a partition with ragged bounds (inside 16-byte groups, empty, shorter than a group) == the whole-vector
    form: x, g and v bit for bit, on the first step and on a later one, with and without the folded scale"""
    import torch
    kind, _, name = opt.partition("_")
    n = 1_000_003
    rng = np.random.RandomState(5)
    x0 = _dev(rng.randn(n)); v0 = _dev(rng.rand(n))
    cuts = [0, 1, 2, 2, 7, 9, 10, 12, 4099, 4100, 300001, 300006, 999999, n]
    for first in (True, False):
        for gscale in (1.0 / 41.0, 1.0):
            g0 = _dev(_gradient(rng, n))
            if kind == "sgd":
                s, call = sgd_scalars(SGD_CFGS[name], 0 if first else 4), _sgd_call
            elif kind == "nag":
                s, call = nag_scalars(NAG_CFGS[name], 0 if first else 4), _nag_call
            else:
                s, call = RMS, _rmsprop_call         # (no first step of its own: both rounds are later steps)
            a = [t.clone() for t in (x0, g0, v0)]
            b = [t.clone() for t in (x0, g0, v0)]
            call(F, a[0], a[1], a[2], gscale, s, first)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                call(F, b[0], b[1], b[2], gscale, s, first, lo=lo, hi=hi)
            torch.cuda.synchronize()
            for u, w, what in zip(a, b, ("x", "g", "v")):
                assert torch.equal(u.view(torch.int32), w.view(torch.int32)), "%s differs (first %r, gscale %r)" % (what, first, gscale)
            assert not torch.equal(a[0], x0)


def test_slice_and_whole_reject_bad_arguments(F):
    import torch
    x = torch.zeros(64, device="cuda"); g = torch.zeros_like(x); v = torch.zeros_like(x)
    s = sgd_scalars(MAIN_SGD, 0)
    with pytest.raises(F.FrcnnError):
        _sgd_call(F, x, g, v, 1.0, s, False, lo=5, hi=4)
    with pytest.raises(F.FrcnnError):
        _nag_call(F, x, g, v, 1.0, nag_scalars(MAIN_NAG, 0), False, lo=-1, hi=4)
    with pytest.raises(F.FrcnnError):   # a misaligned vector
        F._lib.call("frcnn_sgd", C.c_void_p(x.data_ptr() + 4), F.ptr(g), F.ptr(v), 8, 1.0, None, 0.1, 0.0, 0.9, 0.1, 0, 0,
                    F.stream_ptr())
    with pytest.raises(F.FrcnnError):   # momentum without a momentum vector
        F._lib.call("frcnn_sgd", F.ptr(x), F.ptr(g), None, 8, 1.0, None, 0.1, 0.0, 0.9, 0.1, 0, 0, F.stream_ptr())
    with pytest.raises(F.FrcnnError):   # nesterov with dampening
        F._lib.call("frcnn_sgd", F.ptr(x), F.ptr(g), F.ptr(v), 8, 1.0, None, 0.1, 0.0, 0.9, 0.1, 1, 0, F.stream_ptr())
    with pytest.raises(F.FrcnnError):
        F._lib.call("frcnn_nag", F.ptr(x), F.ptr(g), F.ptr(v), 8, 1.0, None, 0.1, 0.0, 0.0, 0, F.stream_ptr())
    # mom = 0: no momentum vector needed
    F._lib.call("frcnn_sgd", F.ptr(x), F.ptr(g), None, 8, 1.0, None, 0.1, 0.0, 0.0, 1.0, 0, 0, F.stream_ptr())
    torch.cuda.synchronize()
    # optim.rmsprop: every form refuses the same malformed calls, and refuses them before anything is written
    rng = np.random.RandomState(2)
    kept = [rng.randn(64).astype(np.float32), _gradient(rng, 64), rng.rand(64).astype(np.float32)]
    x, g, m = (_dev(a) for a in kept)
    cnt = torch.tensor([41.0], dtype=torch.float64, device="cuda")
    off = C.c_void_p(x.data_ptr() + 4)
    tail = (RMS["lr"], RMS["alpha"], RMS["eps"], F.stream_ptr())
    whole = {"frcnn_rmsprop": lambda x_, m_, n: (x_, F.ptr(g), m_, n),
             "frcnn_scale_rmsprop": lambda x_, m_, n: (x_, F.ptr(g), 1.0 / 41.0, m_, n),
             "frcnn_scale_rmsprop_dev": lambda x_, m_, n: (x_, F.ptr(g), F.ptr(cnt), m_, n)}
    sliced = {"frcnn_scale_rmsprop_slice": lambda x_, m_, lo, hi: (x_, F.ptr(g), 1.0 / 41.0, m_, lo, hi),
              "frcnn_scale_rmsprop_slice_dev": lambda x_, m_, lo, hi: (x_, F.ptr(g), F.ptr(cnt), m_, lo, hi)}
    bad = [(fn, args(off, F.ptr(m), 8)) for fn, args in whole.items()]                 # a misaligned x
    bad += [(fn, args(F.ptr(x), None, 8)) for fn, args in whole.items()]              # a NULL m
    bad += [(fn, args(F.ptr(x), F.ptr(m), -1)) for fn, args in whole.items()]         # n = -1
    for fn, args in sliced.items():
        bad += [(fn, args(off, F.ptr(m), 5, 9)), (fn, args(F.ptr(x), None, 5, 9)),    # a misaligned x, a NULL m
                (fn, args(F.ptr(x), F.ptr(m), 5, 4)), (fn, args(F.ptr(x), F.ptr(m), -1, 4))]   # lo > hi, lo = -1
    for fn, args in bad:
        with pytest.raises(F.FrcnnError):
            F._lib.call(fn, *args, *tail)
    for fn, args in whole.items():                                                     # empty ranges: OK, nothing written
        F._lib.call(fn, *args(F.ptr(x), F.ptr(m), 0), *tail)
    for fn, args in sliced.items():
        F._lib.call(fn, *args(F.ptr(x), F.ptr(m), 7, 7), *tail)
    for t, a, what in zip((x, g, m), kept, ("x", "g", "m")):
        assert same_bits(_host(t), a), "%s changed by a refused or an empty rmsprop call" % what


@pytest.mark.parametrize("kind", ["sgd", "nag"])
def test_device_divisor_matches_the_host_scale(F, kind):
    """gscale = 1 / *gcount_dev (the data-parallel count) == the host's 1/41 bit for bit; a count of 0 leaves g unscaled"""
    import torch
    n = 100_003
    rng = np.random.RandomState(3)
    x0 = _dev(rng.randn(n)); g0 = _dev(_gradient(rng, n)); v0 = _dev(rng.rand(n))
    if kind == "sgd":
        s, call, ref = sgd_scalars(MAIN_SGD, 1), _sgd_call, ref_sgd
    else:
        s, call, ref = nag_scalars(dict(MAIN_NAG, weightDecay=5e-4), 1), _nag_call, ref_nag
    for count, host_gscale in ((41.0, 1.0 / 41.0), (0.0, 1.0)):
        cnt = torch.tensor([count], dtype=torch.float64, device="cuda")
        a = [t.clone() for t in (x0, g0, v0)]
        b = [t.clone() for t in (x0, g0, v0)]
        call(F, a[0], a[1], a[2], host_gscale, s, False)
        call(F, b[0], b[1], b[2], 1.0, s, False, gcount=cnt)
        torch.cuda.synchronize()
        for u, w, what in zip(a, b, ("x", "g", "v")):
            assert torch.equal(u.view(torch.int32), w.view(torch.int32)), "%s differs (count %r)" % (what, count)
        want = ref(_host(x0), _host(g0), _host(v0), host_gscale if count else None, s, False)
        for u, w, what in zip(b, want, ("x", "g", "v")):
            assert same_bits(_host(u), w), "%s differs from the restatement (count %r)" % (what, count)


# ---------------------------------------------------------------- F.sgd / F.nag with a plain opfunc
class _Quadratic(object):
    """opfunc(x) -> (f, g) with g depending on x (so the look-ahead's order shows), a fresh device gradient per call"""

    def __init__(self, n, seed):
        rng = np.random.RandomState(seed)
        self.a = (rng.rand(n) + 0.5).astype(np.float32)
        self.b = [(rng.randn(n)).astype(np.float32) for _ in range(8)]
        self.calls = 0
        self.last = None

    def host(self, x, k):
        return float(np.dot(x.astype(np.float64), x)), self.a * x + self.b[k]

    def __call__(self, x):
        fx, g = self.host(x.cpu().numpy(), self.calls)
        self.calls += 1
        self.last = _dev(g)
        return fx, self.last


@pytest.mark.parametrize("name", sorted(SGD_CFGS))
def test_F_sgd_with_a_plain_opfunc_matches_the_restatement(F, name):
    cfg = dict(SGD_CFGS[name])
    n = 4099
    x_ref = np.random.RandomState(1).randn(n).astype(np.float32)
    x = _dev(x_ref)
    f = _Quadratic(n, 2)
    v_ref = None
    for k in range(3):
        _, fx = F.sgd(f, x, cfg)
        fx_ref, g = f.host(x_ref, k)
        x_ref, g_ref, v_ref = ref_sgd(x_ref, g, v_ref, None, sgd_scalars(cfg, k), k == 0)
        assert fx[0] == fx_ref
        assert same_bits(_host(x), x_ref) and same_bits(_host(f.last), g_ref), "step %d" % k
        if cfg.get("momentum", 0):
            assert same_bits(_host(cfg["dfdx"]), v_ref)
        else:
            assert "dfdx" not in cfg
        assert cfg["evalCounter"] == k + 1


@pytest.mark.parametrize("name", sorted(NAG_CFGS))
def test_F_nag_with_a_plain_opfunc_matches_the_restatement(F, name):
    cfg = dict(NAG_CFGS[name], learningRateDecay=0.1)
    state = {}
    n = 4099
    x_ref = np.random.RandomState(1).randn(n).astype(np.float32)
    x = _dev(x_ref)
    f = _Quadratic(n, 3)
    v_ref = None
    for k in range(3):
        _, fx = F.nag(f, x, cfg, state)        # optim's (opfunc, x, config, state) form
        s = nag_scalars(cfg, k)
        if k > 0:
            x_ref = ref_lookahead(x_ref, v_ref, s["mom"])
        fx_ref, g = f.host(x_ref, k)           # opfunc sees the looked-ahead weights
        x_ref, g_ref, v_ref = ref_nag(x_ref, g, v_ref, None, s, k == 0)
        assert fx[0] == fx_ref
        assert same_bits(_host(x), x_ref) and same_bits(_host(f.last), g_ref) and same_bits(_host(state["dfdx"]), v_ref), k
        assert state["evalCounter"] == k + 1 and "evalCounter" not in cfg


@pytest.mark.parametrize("fn,cfg", [
    ("sgd", dict(momentum=0.9, nesterov=True)),                   # dampening defaults to momentum
    ("sgd", dict(momentum=0, dampening=0, nesterov=True)),
    ("sgd", dict(momentum=0.9, learningRates=[1.0])),
    ("sgd", dict(weightDecay=1e-4, weightDecays=[1.0])),
    ("nag", dict(momentum=0)),
    ("nag", dict(momentum=-0.5)),
    ("nag", dict(learningRates=[1.0])),
])
def test_bad_configurations_raise_without_touching_x(F, fn, cfg):
    x0 = np.arange(16, dtype=np.float32)
    x = _dev(x0)
    calls = []
    with pytest.raises((ValueError, F.FrcnnError)):
        getattr(F, fn)(lambda w: calls.append(1), x, cfg)
    assert not calls and same_bits(_host(x), x0)
    assert "dfdx" not in cfg and "evalCounter" not in cfg


# ---------------------------------------------------------------- training steps of the real objective
def _masks(F, model, it, k, H, W, rng):
    model["pnet"].drop_masks = [None] + [(rng.rand(c) > 0.4).astype(np.float32) for c in (128, 256, 384)]
    E = len(F.clean_examples(it.pool[k % 2]["positive"], F.output_map_sizes(model, H, W))) + \
        len(F.clean_examples(it.pool[k % 2]["negative"], F.output_map_sizes(model, H, W)))
    model["cnet"].drop_masks = [(rng.rand(E, 1024) > 0.5).astype(np.float32), (rng.rand(E, 512) > 0.5).astype(np.float32)]


def _train(F, kind, mode, steps, H=225, W=400):
    """mode 'fused' / 'eager': F.sgd / F.nag on the objective (the update folded into the pass after it, or beside it);
    'unfused': f(w), then the numpy restatement on the returned gradient, the weights uploaded again.
    -> per step (loss, weights, gradient, v)"""
    import torch
    model = F.vgg_small(dict(F.duplo_cfg))
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=11)
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
    f = F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
    cfg = dict(MAIN_SGD) if kind == "sgd" else dict(MAIN_NAG, weightDecay=5e-4)
    if mode != "unfused":
        cfg["eager"] = mode == "eager"
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    out = []
    x_ref = v_ref = None
    try:
        for k in range(steps):
            _masks(F, model, it, k, H, W, rng)
            if mode != "unfused":
                _, fx = getattr(F, kind)(f, w, cfg)
                torch.cuda.synchronize()
                out.append((fx[0], w.cpu().numpy().copy(), g.cpu().numpy().copy(), cfg["dfdx"].cpu().numpy().copy()))
                continue
            if x_ref is None:
                x_ref = w.cpu().numpy().copy()
            if kind == "nag" and k > 0:
                x_ref = ref_lookahead(x_ref, v_ref, cfg["momentum"])
                w.copy_(torch.from_numpy(x_ref))
            loss, grad = f(w)
            gh = _host(grad)
            if kind == "sgd":
                x_ref, g_ref, v_ref = ref_sgd(x_ref, gh, v_ref, None, sgd_scalars(cfg, k), k == 0)
            else:
                x_ref, g_ref, v_ref = ref_nag(x_ref, gh, v_ref, None, nag_scalars(cfg, k), k == 0)
            w.copy_(torch.from_numpy(x_ref))
            torch.cuda.synchronize()
            out.append((loss, x_ref.copy(), g_ref.copy(), v_ref.copy()))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
    return out


def _assert_same_runs(a, b):
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0], "loss of step %d: %r vs %r" % (k, ra[0], rb[0])
        for name, u, v in zip(("weights", "gradient", "momentum vector"), ra[1:], rb[1:]):
            assert same_bits(u, v), "%s differ after step %d (%d elements)" % (name, k, int((u != v).sum()))
    assert not np.array_equal(a[0][1], a[-1][1])


@pytest.mark.parametrize("kind", ["sgd", "nag"])
def test_three_training_steps_equal_the_unfused_restatement(F, kind):
    """F.sgd(f, w, sgd_state) / F.nag(f, w, nag_state) on the objective (gradient:div folded into the update's pass) == f(w)
    followed by the numpy restatement applied to the gradient it returned, bit for bit over three steps (deterministic mode)"""
    _assert_same_runs(_train(F, kind, "fused", 3), _train(F, kind, "unfused", 3))


@pytest.mark.parametrize("kind", ["sgd", "nag"])
def test_eager_update_equals_the_update_after_the_pass(F, kind):
    """the update beside the backward pass (state["eager"]) == the update after it: weights, gradient and v bit for bit over
    three steps.  For NAG the look-ahead writes the weights after the previous step renewed the packs beside its pass: the
    next forward must not run on those packs."""
    _assert_same_runs(_train(F, kind, "eager", 3), _train(F, kind, "fused", 3))
