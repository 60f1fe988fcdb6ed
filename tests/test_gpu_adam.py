"""optim.adam (Torch's optim/adam.lua) with coupled and decoupled (AdamW) weight decay on the device: frcnn_adam and its slice
forms on the range kernel of the other optimisers, carrying two state vectors; the folded gradient:div (objective.lua:200), the
device divisor, the gradient guard, staged training, the eager update, and the Python optimiser F.adam.

The reference is tests/adam_ref.py: a numpy fp32 restatement, one separately rounded operation per Lua statement.  Comparisons
are bit for bit, signed zeros included.  (_Quadratic, _masks and the training loop follow test_gpu_optim.py, the guard's host
arithmetic test_gpu_gradclip.py, copied so that this file stands alone.)"""
import ctypes as C
import math

import numpy as np
import pytest

from adam_ref import adam_args, adam_scalars, gradient, ref_adam, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32

ADAM_CFGS = {
    "defaults": dict(),
    "coupled": dict(weightDecay=5e-4),
    "decoupled": dict(weightDecay=5e-4, decoupled=True),
    "lrd": dict(learningRateDecay=0.25),
    "beta1_0": dict(beta1=0),
    "beta2_eps": dict(beta2=0.9, epsilon=1e-3),
}
DECAY_MODES = ["defaults", "coupled", "decoupled"]
NAMES = ("x", "g", "m", "v")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _adam_call(F, x, g, m, v, gscale, s, gcount=None, lo=None, hi=None):
    p = [F.ptr(t) for t in (x, g, m, v)]
    if lo is None:
        F._lib.call("frcnn_adam", *p, x.numel(), gscale, F.ptr(gcount), *adam_args(s), F.stream_ptr())
    elif gcount is None:
        F._lib.call("frcnn_adam_slice", *p, lo, hi, gscale, *adam_args(s), F.stream_ptr())
    else:
        F._lib.call("frcnn_adam_slice_dev", *p, lo, hi, F.ptr(gcount), *adam_args(s), F.stream_ptr())


# ---------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1_000_003])
@pytest.mark.parametrize("gscale", [1.0 / 41.0, 1.0])
@pytest.mark.parametrize("name", sorted(ADAM_CFGS))
def test_adam_kernel_matches_the_restatement(F, name, gscale, n):
    """three consecutive steps from m = v = 0 (as optim.adam creates them): x, g, m and v bit for bit after each; an unscaled
    gradient without coupled decay keeps its input bits"""
    cfg = ADAM_CFGS[name]
    rng = np.random.RandomState(n % 1000 + 19)
    ref = [rng.randn(n).astype(np.float32), None, np.zeros(n, np.float32), np.zeros(n, np.float32)]
    x, m, v = _dev(ref[0]), _dev(ref[2]), _dev(ref[3])
    for k in range(3):
        s = adam_scalars(cfg, k)
        g_in = gradient(rng, n)
        g = _dev(g_in)
        _adam_call(F, x, g, m, v, gscale, s)
        ref = ref_adam(ref[0], g_in, ref[2], ref[3], gscale if gscale != 1.0 else None, s)
        for t, w, what in zip((x, g, m, v), ref, NAMES):
            assert same_bits(_host(t), w), "%s after step %d" % (what, k)
        if gscale == 1.0 and s["wd"] == 0:
            assert same_bits(_host(g), g_in), "g changed by step %d" % k


@pytest.mark.parametrize("form", ["whole", "slice"])
def test_a_grid_that_wraps_matches_the_restatement(F, form):
    """the grid-stride loop takes a second turn: one block's worth of 16-byte groups above the grid's cap (2048 blocks for the
    whole vector, 1024 for a slice), a three-element tail on the whole vector, ragged ends on both sides of the slice"""
    n = 4 * (2048 * 256 + 256) + 3
    lo, hi = (0, n) if form == "whole" else (5, 5 + 3 + 4 * (1024 * 256 + 256) + 2)
    rng = np.random.RandomState(17)
    h0 = [rng.randn(n).astype(np.float32), gradient(rng, n), rng.randn(n).astype(np.float32), rng.rand(n).astype(np.float32)]
    gscale = 1.0 / 41.0
    s = adam_scalars(ADAM_CFGS["coupled"], 4)
    d = [_dev(a) for a in h0]
    if form == "whole":
        _adam_call(F, *d, gscale, s)
    else:
        _adam_call(F, *d, gscale, s, lo=lo, hi=hi)
    want = ref_adam(*[a[lo:hi] for a in h0[:2]], *[a[lo:hi] for a in h0[2:]], gscale, s)
    for t, w, a0, what in zip(d, want, h0, NAMES):
        got = _host(t)
        assert same_bits(got[lo:hi], w), "%s differs from the restatement" % what
        assert same_bits(got[:lo], a0[:lo]) and same_bits(got[hi:], a0[hi:]), "%s changed outside [%d, %d)" % (what, lo, hi)
    assert not same_bits(_host(d[0])[lo:hi], h0[0][lo:hi])


@pytest.mark.parametrize("name", DECAY_MODES)
def test_slices_tile_the_whole_vector_bit_for_bit(F, name):
    """the slice form over a partition with ragged bounds (inside 16-byte groups, empty, shorter than a group) == the whole-vector
    form: x, g, m and v bit for bit, with and without the folded scale"""
    import torch
    n = 1_000_003
    rng = np.random.RandomState(5)
    x0 = _dev(rng.randn(n)); m0 = _dev(rng.randn(n)); v0 = _dev(rng.rand(n))
    cuts = [0, 1, 2, 2, 7, 9, 10, 12, 4099, 4100, 300001, 300006, 999999, n]
    s = adam_scalars(ADAM_CFGS[name], 4)
    for gscale in (1.0 / 41.0, 1.0):
        g0 = _dev(gradient(rng, n))
        a = [t.clone() for t in (x0, g0, m0, v0)]
        b = [t.clone() for t in (x0, g0, m0, v0)]
        _adam_call(F, *a, gscale, s)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            _adam_call(F, *b, gscale, s, lo=lo, hi=hi)
        torch.cuda.synchronize()
        for u, w, what in zip(a, b, NAMES):
            assert torch.equal(u.view(torch.int32), w.view(torch.int32)), "%s differs (gscale %r)" % (what, gscale)
        assert not torch.equal(a[0], x0)


@pytest.mark.parametrize("form", ["whole", "slice"])
def test_device_divisor_matches_the_host_scale(F, form):
    """gscale = 1 / *gcount_dev (the data-parallel count) == the host's 1/41 bit for bit; a count of 0 leaves g unscaled"""
    import torch
    n = 100_003
    lo, hi = (None, None) if form == "whole" else (3, 100_001)
    rng = np.random.RandomState(3)
    h0 = [rng.randn(n).astype(np.float32), gradient(rng, n), rng.randn(n).astype(np.float32), rng.rand(n).astype(np.float32)]
    s = adam_scalars(ADAM_CFGS["coupled"], 1)
    for count, host_gscale in ((41.0, 1.0 / 41.0), (0.0, 1.0)):
        cnt = torch.tensor([count], dtype=torch.float64, device="cuda")
        a = [_dev(t) for t in h0]
        b = [_dev(t) for t in h0]
        _adam_call(F, *a, host_gscale, s, lo=lo, hi=hi)
        _adam_call(F, *b, 1.0, s, gcount=cnt, lo=lo, hi=hi)
        torch.cuda.synchronize()
        for u, w, what in zip(a, b, NAMES):
            assert torch.equal(u.view(torch.int32), w.view(torch.int32)), "%s differs (count %r)" % (what, count)
        r = slice(lo, hi)
        want = ref_adam(h0[0][r], h0[1][r], h0[2][r], h0[3][r], host_gscale if count else None, s)
        for u, w, a0, what in zip(b, want, h0, NAMES):
            got = _host(u)
            assert same_bits(got[r], w), "%s differs from the restatement (count %r)" % (what, count)
            if lo is not None:
                assert same_bits(got[:lo], a0[:lo]) and same_bits(got[hi:], a0[hi:]), "%s changed outside the slice" % what


def test_bad_arguments_are_refused_before_anything_is_written(F):
    import torch
    rng = np.random.RandomState(2)
    kept = [rng.randn(64).astype(np.float32), gradient(rng, 64), rng.randn(64).astype(np.float32), rng.rand(64).astype(np.float32)]
    x, g, m, v = (_dev(a) for a in kept)
    cnt = torch.tensor([41.0], dtype=torch.float64, device="cuda")
    s = adam_scalars(ADAM_CFGS["coupled"], 0)
    tail = adam_args(s) + (F.stream_ptr(),)
    both = adam_args(dict(s, decay=1e-6)) + (F.stream_ptr(),)           # wd != 0 and decay != 0
    P = [F.ptr(t) for t in (x, g, m, v)]
    forms = {"frcnn_adam": lambda p, a, b: (*p, b, 1.0 / 41.0, None),                     # (b = n)
             "frcnn_adam_dev": lambda p, a, b: (*p, b, 1.0, F.ptr(cnt)),
             "frcnn_adam_slice": lambda p, a, b: (*p, a, b, 1.0 / 41.0),
             "frcnn_adam_slice_dev": lambda p, a, b: (*p, a, b, F.ptr(cnt))}
    bad = []
    for fn, args in forms.items():
        entry = "frcnn_adam" if fn == "frcnn_adam_dev" else fn
        for i in range(4):                                                                 # each vector NULL, then misaligned
            bad.append((entry, args(P[:i] + [None] + P[i + 1:], 5, 9), tail))
            bad.append((entry, args(P[:i] + [C.c_void_p(P[i].value + 4)] + P[i + 1:], 5, 9), tail))
        bad.append((entry, args(P, 5, 9), both))
        if "slice" in fn:
            bad += [(entry, args(P, 5, 4), tail), (entry, args(P, -1, 4), tail)]           # lo > hi, lo < 0
        else:
            bad.append((entry, args(P, 0, -1), tail))                                      # n < 0
    bad.append(("frcnn_adam_slice_dev", (*P, 5, 9, None), tail))                           # a NULL divisor
    for fn, args, t in bad:
        with pytest.raises(F.FrcnnError):
            F._lib.call(fn, *args, *t)
    for fn, args in forms.items():                                                         # empty ranges: OK, nothing written
        entry = "frcnn_adam" if fn == "frcnn_adam_dev" else fn
        F._lib.call(entry, *(args(P, 7, 7) if "slice" in fn else args(P, 0, 0)), *tail)
    for t, a, what in zip((x, g, m, v), kept, NAMES):
        assert same_bits(_host(t), a), "%s changed by a refused or an empty call" % what


# ---------------------------------------------------------------- F.adam with a plain opfunc
class _Quadratic(object):
    """opfunc(x) -> (f, g) with g depending on x, a fresh device gradient per call"""

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


@pytest.mark.parametrize("separate_state", [False, True])
@pytest.mark.parametrize("name", sorted(ADAM_CFGS))
def test_F_adam_with_a_plain_opfunc_matches_the_restatement(F, name, separate_state):
    cfg = dict(ADAM_CFGS[name])
    state = {} if separate_state else cfg
    n = 4099
    x_ref = np.random.RandomState(1).randn(n).astype(np.float32)
    m_ref = np.zeros(n, np.float32); v_ref = np.zeros(n, np.float32)
    x = _dev(x_ref)
    f = _Quadratic(n, 2)
    for k in range(3):
        _, fx = F.adam(f, x, cfg, state) if separate_state else F.adam(f, x, cfg)
        fx_ref, g = f.host(x_ref, k)
        x_ref, g_ref, m_ref, v_ref = ref_adam(x_ref, g, m_ref, v_ref, None, adam_scalars(cfg, k))
        assert fx[0] == fx_ref
        assert same_bits(_host(x), x_ref) and same_bits(_host(f.last), g_ref), "step %d" % k
        assert same_bits(_host(state["m"]), m_ref) and same_bits(_host(state["v"]), v_ref), "step %d" % k
        assert state["t"] == k + 1
        if separate_state:
            assert "t" not in cfg and "m" not in cfg and "v" not in cfg


def test_a_step_that_raises_leaves_the_state_as_it_was(F):
    x0 = np.arange(16, dtype=np.float32)
    x = _dev(x0)

    def boom(w):
        raise RuntimeError("opfunc failed")
    cfg = dict()
    with pytest.raises(RuntimeError):
        F.adam(boom, x, cfg)
    assert cfg == {} and same_bits(_host(x), x0)
    f = _Quadratic(16, 1)
    F.adam(f, x, cfg)
    m1, v1 = cfg["m"], cfg["v"]
    with pytest.raises(RuntimeError):
        F.adam(boom, x, cfg)
    assert cfg["t"] == 1 and cfg["m"] is m1 and cfg["v"] is v1


# ---------------------------------------------------------------- the guard (plain opfunc: D = 1)
def _d_prime(S, D, clip):
    """include/frcnn_hip.h's formula in double, one correctly rounded operation per step"""
    norm = math.sqrt(S) / D
    if clip > 0 and math.isfinite(S):
        ratio = norm / clip
        if ratio > 1.0:
            return D * ratio
    return D


@pytest.mark.parametrize("name", DECAY_MODES)
def test_clipped_step_is_frcnn_adam_with_the_recorded_divisor(F, name):
    import torch
    n, clip = 10_007, 0.25
    rng = np.random.RandomState(6)
    xh = rng.randn(n).astype(np.float32); gh = gradient(rng, n)
    x, gd = _dev(xh), _dev(gh)
    cfg = dict(ADAM_CFGS[name], clipNorm=clip)
    F.adam(lambda w: (0.0, gd), x, cfg)
    rec = _host(cfg["_guard"]["record"])
    S = rec[0]
    exact = math.fsum((gh.astype(np.float64) ** 2).tolist())
    assert abs(S - exact) <= 2.0 ** -27 * exact and rec[3] == 0.0
    dp = _d_prime(S, 1.0, clip)                       # sqrt, divide, multiply: the three fp64 operations on the recorded S
    assert rec[2] == dp and dp > 1.0, "the step was not clipped"
    x2, g2, m2, v2 = _dev(xh), _dev(gh), _dev(np.zeros(n, np.float32)), _dev(np.zeros(n, np.float32))
    up = torch.tensor([dp], dtype=torch.float64, device="cuda")
    _adam_call(F, x2, g2, m2, v2, 1.0, adam_scalars(cfg, 0), gcount=up)
    for a, b, what in zip((x, gd, cfg["m"], cfg["v"]), (x2, g2, m2, v2), NAMES):
        assert same_bits(_host(a), _host(b)), what
    want = ref_adam(xh, gh, np.zeros(n, np.float32), np.zeros(n, np.float32), f32(1.0 / dp), adam_scalars(cfg, 0))
    for a, w, what in zip((x2, g2, m2, v2), want, NAMES):
        assert same_bits(_host(a), w), "%s differs from the restatement" % what
    assert cfg["t"] == 1


@pytest.mark.parametrize("bad", [np.inf, np.nan])
@pytest.mark.parametrize("name", DECAY_MODES)
def test_non_finite_gradient_is_treated_as_zero(F, name, bad):
    """a skipped step: g counts as zero, and Adam goes on with its moments (and its weight decay, if any) alone"""
    n = 10_007
    rng = np.random.RandomState(8)
    xh = rng.randn(n).astype(np.float32)
    x = _dev(xh)
    cfg = dict(ADAM_CFGS[name], skipNonFinite=True)
    f = _Quadratic(n, 4)
    F.adam(f, x, cfg)                                  # an ordinary first step: m and v are not zero afterwards
    assert _host(cfg["_guard"]["record"])[3] == 0.0
    xh1, mh1, vh1 = _host(x).copy(), _host(cfg["m"]).copy(), _host(cfg["v"]).copy()
    assert np.any(mh1) and np.any(vh1)
    gh = gradient(rng, n)
    gh[7_777] = bad
    gd = _dev(gh)
    F.adam(lambda w: (0.0, gd), x, cfg)
    rec = _host(cfg["_guard"]["record"])
    assert rec[3] == 1.0 and rec[2] == 1.0 and not math.isfinite(rec[0])
    zero = np.zeros(n, np.float32)
    xw, gw, mw, vw = ref_adam(xh1, zero, mh1, vh1, None, adam_scalars(cfg, 1))
    ga = _host(gd)
    if name != "coupled":
        assert not np.any(ga) and not np.any(np.signbit(ga)), "g is not all +0"
    assert same_bits(ga, gw), "g"
    assert same_bits(_host(x), xw) and same_bits(_host(cfg["m"]), mw) and same_bits(_host(cfg["v"]), vw)
    assert not same_bits(xw, xh1), "Adam goes on with its moments on a skipped step"
    assert cfg["t"] == 2


# ---------------------------------------------------------------- training steps of the real objective
H, W = 225, 400
TRAIN_CFGS = {"coupled": dict(learningRate=1e-3, weightDecay=5e-4), "decoupled": dict(learningRate=1e-3, weightDecay=5e-4, decoupled=True)}


def _masks(F, model, it, k, rng):
    model["pnet"].drop_masks = [None] + [(rng.rand(c) > 0.4).astype(np.float32) for c in (128, 256, 384)]
    E = len(F.clean_examples(it.pool[k % 2]["positive"], F.output_map_sizes(model, H, W))) + \
        len(F.clean_examples(it.pool[k % 2]["negative"], F.output_map_sizes(model, H, W)))
    model["cnet"].drop_masks = [(rng.rand(E, 1024) > 0.5).astype(np.float32), (rng.rand(E, 512) > 0.5).astype(np.float32)]


_RUNS = {}


def _train(F, name, mode, steps, train=None):
    """mode 'fused' / 'eager': F.adam on the objective (the update folded into the pass after it, or beside it); 'unfused': f(w),
    then the numpy restatement on the returned gradient (on the trainable slices, with staged training), the weights uploaded
    again.  -> (per step (loss, weights, gradient, m, v), the blocks' ranges, the initial weights); computed once per (name, mode, steps, train) and shared, read-only"""
    import torch
    key = (name, mode, steps, None if train is None else tuple(sorted(train.items())))
    if key in _RUNS:
        return _RUNS[key]
    model = F.vgg_small(dict(F.duplo_cfg))
    if train is not None:
        model["cfg"]["train"] = dict(train)
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=11)
    w0 = w.cpu().numpy().copy()
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
    f = F.create_objective(model, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
    cfg = dict(TRAIN_CFGS[name])
    if mode != "unfused":
        cfg["eager"] = mode == "eager"
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    out = []
    ref = None
    try:
        for k in range(steps):
            _masks(F, model, it, k, rng)
            if mode != "unfused":
                _, fx = F.adam(f, w, cfg)
                torch.cuda.synchronize()
                assert cfg["t"] == k + 1
                out.append((fx[0],) + tuple(t.cpu().numpy().copy() for t in (w, g, cfg["m"], cfg["v"])))
                continue
            if ref is None:
                ref = [w.cpu().numpy().copy(), None, np.zeros(w.numel(), np.float32), np.zeros(w.numel(), np.float32)]
            ranges = f.trainable_ranges() or [(0, w.numel())]
            loss, grad = f(w)
            ref[1] = _host(grad).copy()
            s = adam_scalars(cfg, k)
            for lo, hi in ranges:
                for a, r in zip(ref, ref_adam(ref[0][lo:hi], ref[1][lo:hi], ref[2][lo:hi], ref[3][lo:hi], None, s)):
                    a[lo:hi] = r
            w.copy_(torch.from_numpy(ref[0]))
            torch.cuda.synchronize()
            out.append((loss,) + tuple(a.copy() for a in ref))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
    groups = {"block%d" % (b + 1): model["pnet"].block_param_range(b) for b in range(4)}
    for r in out:
        for a in r[1:]:
            a.flags.writeable = False
    _RUNS[key] = out, groups, w0
    return _RUNS[key]


def _assert_same_runs(a, b):
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0] == rb[0], "loss of step %d: %r vs %r" % (k, ra[0], rb[0])
        for name, u, v in zip(("weights", "gradient", "m", "v"), ra[1:], rb[1:]):
            assert same_bits(u, v), "%s differ after step %d (%d elements)" % (name, k, int((u != v).sum()))
    assert not np.array_equal(a[0][1], a[-1][1])


@pytest.mark.parametrize("name", sorted(TRAIN_CFGS))
def test_three_training_steps_equal_the_unfused_restatement(F, name):
    """F.adam(f, w, cfg) on the objective (gradient:div folded into the update's pass) == f(w) followed by the numpy restatement
    applied to the gradient it returned, bit for bit over three steps (deterministic mode)"""
    _assert_same_runs(_train(F, name, "fused", 3)[0], _train(F, name, "unfused", 3)[0])


@pytest.mark.parametrize("name", sorted(TRAIN_CFGS))
def test_eager_update_equals_the_update_after_the_pass(F, name):
    """the update beside the backward pass (state["eager"]) == the update after it: weights, gradient, m and v bit for bit"""
    _assert_same_runs(_train(F, name, "eager", 3)[0], _train(F, name, "fused", 3)[0])


def test_staged_training_leaves_frozen_weights_and_moments_alone(F):
    """cfg["train"] = {frozen_blocks = 2}, two F.adam steps: the frozen slices of the weights, m and v keep their bits (m and v
    stay zero there); the trainable slices equal the restatement applied to those slices of the same gradient"""
    train = dict(proposal=True, classification=True, frozen_blocks=2)
    fused, groups, w0 = _train(F, "coupled", "fused", 2, train=train)
    ref = _train(F, "coupled", "unfused", 2, train=train)[0]
    lo, cut = 0, groups["block3"][0]                  # blocks 1 and 2 are frozen: everything below block 3
    assert groups["block2"][1] <= cut and cut > 0
    for k, (a, b) in enumerate(zip(fused, ref)):
        assert same_bits(a[1][lo:cut], w0[lo:cut]), "step %d changed frozen weights" % k
        assert not np.any(a[3][lo:cut]) and not np.any(a[4][lo:cut]), "step %d touched the moments of a frozen slice" % k
        assert not np.any(np.signbit(a[3][lo:cut])) and not np.any(np.signbit(a[4][lo:cut]))
        assert a[0] == b[0]
        for i, what in ((1, "weights"), (2, "gradient"), (3, "m"), (4, "v")):
            assert same_bits(a[i], b[i]), "%s differ from the restatement after step %d" % (what, k)
    assert not same_bits(fused[1][1][cut:], w0[cut:]) and np.any(fused[1][3][cut:]) and np.any(fused[1][4][cut:])
