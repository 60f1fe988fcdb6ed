"""Gradient-norm clipping and the non-finite-step guard (frcnn_grad_clip, state["clipNorm"] / state["skipNonFinite"]) on the device.

The semantics of include/frcnn_hip.h, restated.  g = the flat gradient after the pass, T = the trainable slices (the whole vector
without staged training), D = the divisor of gradient:div (objective.lua:200; 1: nothing to scale):
    S     = sum over T of (double)g[i] * (double)g[i], in fp64, in a fixed order (two calls: the same bits)
    norm  = sqrt(S) / D
    D'    = D * max(1, norm / clipNorm)   (fp64, each operation correctly rounded; clipNorm <= 0: D' = D)
    a clipped step IS the optimiser's existing update with the device divisor D' (frcnn_scale_rmsprop_dev, frcnn_sgd, frcnn_nag)
    S not finite: g is overwritten with zeros on T, D' = D, skipped = 1
    record = double[4] {S, norm, D', skipped}
Comparisons between the guarded path and the existing entry points are bit for bit.  (ref_sgd / ref_nag, _masks and the training
loop follow test_gpu_optim.py, copied so that this file stands alone.)"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
VGG_SMALL_PARAMS = 26_784_106


# ---------------------------------------------------------------- helpers
def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _flat(ranges):
    if ranges is None:
        return None, 0
    return (C.c_longlong * max(1, 2 * len(ranges)))(*[int(b) for r in ranges for b in r]), len(ranges)


def _grad_clip(F, g, ranges=None, divisor=1.0, divisor_dev=None, clip=0.0, record=None):
    """queues frcnn_grad_clip on g (a device tensor) -> the record as a device tensor of 4 doubles"""
    import torch
    n = g.numel()
    nbytes = F._lib.load().frcnn_grad_clip_workspace_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    if record is None:
        record = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    flat, nr = _flat(ranges)
    F._lib.call("frcnn_grad_clip", F.ptr(g), n, flat, nr, divisor, F.ptr(divisor_dev), clip, F.ptr(record), F.ptr(ws), nbytes,
                F.stream_ptr())
    torch.cuda.synchronize()
    return record


def _covered(n, ranges):
    return [(0, n)] if ranges is None else [(lo, hi) for lo, hi in ranges if hi > lo]


def _exact_S(g, ranges):
    """math.fsum of the fp64 squares: the correctly rounded sum of the exact products (taken over blocks of 2^20 terms and
    then over the blocks' sums, to bound the host's memory: at most 2^-52 relative from the true sum)"""
    parts = []
    for lo, hi in _covered(len(g), ranges):
        for c in range(lo, hi, 1 << 20):
            d = g[c:min(hi, c + (1 << 20))].astype(np.float64)
            parts.append(math.fsum((d * d).tolist()))
    return math.fsum(parts)


def _d_prime(S, D, clip):
    """the header's formula in double, one correctly rounded operation per step"""
    norm = math.sqrt(S) / D
    if clip > 0 and math.isfinite(S):
        ratio = norm / clip
        if ratio > 1.0:
            return D * ratio
    return D


def _slice_sets(n):
    sets = [None, [(0, n)]]
    if n >= 3:
        sets.append([(1, n - 1)])                                   # unaligned at both ends
    if n >= 5:
        sets.append([(0, 0), (1, 2), (2, 2), (3, n)])               # empty slices, touching slices, a ragged head
    if n >= 1023:
        sets.append([(5, 6), (7, 401), (402, 402), (515, n - 3)])   # ragged ends inside 16-byte groups, one empty
    return sets


# ---------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1 << 20, VGG_SMALL_PARAMS])
def test_sum_of_squares_matches_fsum_and_repeats_bit_for_bit(F, n):
    """S against math.fsum of the fp64 squares: relative error at most 2^-27.  Derived, not measured: every product of two fp32
    values is exact in fp64, and an fp64 sum of n <= 2^26 non-negative terms in any order is within n * 2^-53 of the true sum."""
    rng = np.random.RandomState(n % 997 + 1)
    gh = (rng.randn(n) * 3.0).astype(np.float32)
    gh[::7] = 0.0
    g = _dev(gh)
    sets = _slice_sets(n)
    if n == VGG_SMALL_PARAMS:
        sets = [None, [(12_089_683, n)], [(3, 1_000_001), (12_089_681, n - 2)]]    # the classification net's slice; ragged bounds
    for ranges in sets:
        r1 = _host(_grad_clip(F, g, ranges)).copy()
        r2 = _host(_grad_clip(F, g, ranges)).copy()
        assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64)), "two calls differ (%r)" % (ranges,)
        want = _exact_S(gh, ranges)
        err = abs(r1[0] - want) / want if want else abs(r1[0])
        print("n=%d ranges=%r S=%r fsum=%r rel err %.3g" % (n, ranges, r1[0], want, err))
        assert err <= 2.0 ** -27, (ranges, r1[0], want, err)
        assert r1[1] == math.sqrt(r1[0]) and r1[2] == 1.0 and r1[3] == 0.0     # D = 1, nothing clipped
        assert same_bits(_host(g), gh), "frcnn_grad_clip changed a finite gradient"


# ---------------------------------------------------------------- the optimisers' entry points
RMS = dict(lr=1e-2, alpha=0.99, eps=1e-8)
SGD = dict(clr=1e-3, wd=0.0005, mom=0.9, omd=1.0 - 0.9, nesterov=False)        # main.lua:122-123
NAG = dict(clr=1e-3, wd=5e-4, mom=0.9)


def _update(F, kind, x, g, s, gcount=None, gscale=1.0, ranges=None, cfg=None):
    """one update (not the first step: the state vector exists) on the whole vector or on `ranges`, the divisor on the device
    (gcount) or as the host factor gscale"""
    ptr, sp = F.ptr, F.stream_ptr
    call = F._lib.call
    if kind == "rmsprop":
        c = cfg or RMS
        if ranges is None:
            if gcount is not None:
                call("frcnn_scale_rmsprop_dev", ptr(x), ptr(g), ptr(gcount), ptr(s), x.numel(), c["lr"], c["alpha"], c["eps"], sp())
            else:
                call("frcnn_scale_rmsprop", ptr(x), ptr(g), gscale, ptr(s), x.numel(), c["lr"], c["alpha"], c["eps"], sp())
        else:
            for lo, hi in ranges:
                if gcount is not None:
                    call("frcnn_scale_rmsprop_slice_dev", ptr(x), ptr(g), ptr(gcount), ptr(s), lo, hi, c["lr"], c["alpha"], c["eps"], sp())
                else:
                    call("frcnn_scale_rmsprop_slice", ptr(x), ptr(g), gscale, ptr(s), lo, hi, c["lr"], c["alpha"], c["eps"], sp())
    elif kind == "sgd":
        c = cfg or SGD
        args = (c["clr"], c["wd"], c["mom"], c["omd"], int(c["nesterov"]), int(c.get("first", 0)))
        if ranges is None:
            call("frcnn_sgd", ptr(x), ptr(g), ptr(s), x.numel(), gscale, ptr(gcount), *args, sp())
        else:
            for lo, hi in ranges:
                if gcount is not None:
                    call("frcnn_sgd_slice_dev", ptr(x), ptr(g), ptr(s), lo, hi, ptr(gcount), *args, sp())
                else:
                    call("frcnn_sgd_slice", ptr(x), ptr(g), ptr(s), lo, hi, gscale, *args, sp())
    else:
        c = cfg or NAG
        args = (c["clr"], c["wd"], c["mom"], int(c.get("first", 0)))
        if ranges is None:
            call("frcnn_nag", ptr(x), ptr(g), ptr(s), x.numel(), gscale, ptr(gcount), *args, sp())
        else:
            for lo, hi in ranges:
                if gcount is not None:
                    call("frcnn_nag_slice_dev", ptr(x), ptr(g), ptr(s), lo, hi, ptr(gcount), *args, sp())
                else:
                    call("frcnn_nag_slice", ptr(x), ptr(g), ptr(s), lo, hi, gscale, *args, sp())


def _vectors(n, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(n).astype(np.float32)
    g = (rng.randn(n) * 3.0).astype(np.float32)
    g[::7] = 0.0
    g[3::11] = -0.0
    s = rng.rand(n).astype(np.float32)
    return x, g, s


SLICES = [(3, 1001), (1001, 40_002), (50_005, 100_001)]     # of n = 100_003: ragged bounds, two touching slices, a gap, a tail left out


# ---------------------------------------------------------------- 2. a clipped step is the existing step with D'
@pytest.mark.parametrize("divisor", ["host", "device"])
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_clipped_step_is_the_existing_step_with_the_recorded_divisor(F, kind, sliced, divisor):
    import torch
    n, D = 100_003, 41.0
    xh, gh, sh = _vectors(n, 3)
    ranges = SLICES if sliced else None
    norm = math.sqrt(_exact_S(gh, ranges)) / D
    ddev = torch.tensor([D], dtype=torch.float64, device="cuda") if divisor == "device" else None
    for clip, clipped in ((0.5 * norm, True), (2.0 * norm, False)):
        x, g, s = _dev(xh), _dev(gh), _dev(sh)
        rec = _grad_clip(F, g, ranges, divisor=1.0 if ddev is not None else D, divisor_dev=ddev, clip=clip)
        assert same_bits(_host(g), gh)
        r = _host(rec).copy()
        S = r[0]
        assert r[3] == 0.0 and r[1] == math.sqrt(S) / D
        want_dp = _d_prime(S, D, clip)
        assert r[2] == want_dp, "D' recorded %r, recomputed %r" % (r[2], want_dp)
        assert (r[2] > D) == clipped
        _update(F, kind, x, g, s, gcount=rec[2:], ranges=ranges)              # the guarded path: the record's D' as the divisor
        got = [_host(t).copy() for t in (x, g, s)]
        # the existing whole-vector entry point with the host's D' on copies
        x2, g2, s2 = _dev(xh), _dev(gh), _dev(sh)
        up = torch.tensor([want_dp], dtype=torch.float64, device="cuda")
        _update(F, kind, x2, g2, s2, gcount=up)
        want = [_host(t).copy() for t in (x2, g2, s2)]
        inside = np.zeros(n, bool)
        for lo, hi in _covered(n, ranges):
            inside[lo:hi] = True
        for a, b, orig, what in zip(got, want, (xh, gh, sh), ("x", "g", "state")):
            assert same_bits(a[inside], b[inside]), "%s differs on T (clip %r)" % (what, clip)
            assert same_bits(a[~inside], orig[~inside]), "%s changed outside T" % what
        if not clipped:   # norm <= clipNorm: the unguarded step with D
            x3, g3, s3 = _dev(xh), _dev(gh), _dev(sh)
            _update(F, kind, x3, g3, s3, gscale=1.0 / D, ranges=ranges)
            for a, t, what in zip(got, (x3, g3, s3), ("x", "g", "state")):
                assert same_bits(a, _host(t)), "%s differs from the unguarded step" % what


# ---------------------------------------------------------------- 3. the effect
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_clipped_gradient_has_the_clip_norm(F, kind, sliced):
    """||g|| over T after a clipped step (fp64 sum of the fp32 values g is left holding; wd = 0, SGD/NAG add wd*x into g) is
    clipNorm within 2^-22 relative.  Derived: one fp32 rounding of 1/D' and one per element bound the error by 2^-23."""
    n, D, clip = 100_003, 41.0, 0.37
    xh, gh, sh = _vectors(n, 4)
    ranges = SLICES if sliced else None
    x, g, s = _dev(xh), _dev(gh), _dev(sh)
    rec = _grad_clip(F, g, ranges, divisor=D, clip=clip)
    assert _host(rec)[2] > D
    cfg = {"rmsprop": RMS, "sgd": dict(SGD, wd=0.0), "nag": dict(NAG, wd=0.0)}[kind]
    _update(F, kind, x, g, s, gcount=rec[2:], ranges=ranges, cfg=cfg)
    after = math.sqrt(_exact_S(_host(g), ranges))
    print("%s sliced=%s: norm after %r, clipNorm %r, rel %.3g" % (kind, sliced, after, clip, abs(after - clip) / clip))
    assert abs(after - clip) <= 2.0 ** -22 * clip


# ---------------------------------------------------------------- 4. non-finite gradients
def ref_sgd(x, g, v, gscale, s):
    """optim.sgd after opfunc, a later step (test_gpu_optim.py's restatement): -> x, g, v as Torch leaves them"""
    if gscale is not None:
        g = g * f32(gscale)
    if s["wd"] != 0:
        g = g + f32(s["wd"]) * x
    d = g
    if s["mom"] != 0:
        v = v * f32(s["mom"]) + f32(s["omd"]) * g
        if s["nesterov"]:
            g = g + f32(s["mom"]) * v
            d = g
        else:
            d = v
    x = x + f32(-s["clr"]) * d
    return x, g, v


def ref_nag(x, g, v, gscale, s):
    if gscale is not None:
        g = g * f32(gscale)
    if s["wd"] != 0:
        g = g + f32(s["wd"]) * x
    v = v * f32(s["mom"])
    v = v + f32(-s["clr"]) * g
    x = x + v
    return x, g, v


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_non_finite_gradient_is_treated_as_zero(F, kind, sliced, bad):
    n, D = 100_003, 41.0
    xh, gh, sh = _vectors(n, 5)
    gh[77_777] = bad                                       # inside T of both forms
    ranges = SLICES if sliced else None
    inside = np.zeros(n, bool)
    for lo, hi in _covered(n, ranges):
        inside[lo:hi] = True
    x, g, s = _dev(xh), _dev(gh), _dev(sh)
    rec = _grad_clip(F, g, ranges, divisor=D, clip=0.5)
    r = _host(rec)
    assert r[3] == 1.0 and r[2] == D and not math.isfinite(r[0])
    gz = _host(g).copy()
    assert not np.any(gz[inside]) and not np.any(np.signbit(gz[inside])), "g is not all +0 on T"
    assert same_bits(gz[~inside], gh[~inside]), "g touched outside T"
    _update(F, kind, x, g, s, gcount=rec[2:], ranges=ranges)
    xa, ga, sa = _host(x), _host(g), _host(s)
    for a, orig in ((xa, xh), (ga, gz), (sa, sh)):
        assert same_bits(a[~inside], orig[~inside])
    zero = np.zeros(n, np.float32)
    if kind == "rmsprop":
        assert same_bits(xa, xh), "RMSprop moved x on a skipped step"
        assert same_bits(sa[inside], (f32(RMS["alpha"]) * sh)[inside]), "m != alpha*m"
    else:
        ref = ref_sgd if kind == "sgd" else ref_nag
        xw, gw, vw = ref(xh, zero, sh, 1.0 / D, SGD if kind == "sgd" else NAG)
        assert same_bits(xa[inside], xw[inside]) and same_bits(ga[inside], gw[inside]) and same_bits(sa[inside], vw[inside])


def test_huge_finite_gradient_is_not_skipped(F):
    """3e38 is finite in fp32 and its square (9e76) in fp64: the step is clipped, not skipped"""
    n, D, clip = 1000, 41.0, 1.0
    gh = np.full(n, 3e38, np.float32)
    gh[1::2] = -3e38
    g = _dev(gh)
    r = _host(_grad_clip(F, g, None, divisor=D, clip=clip))
    assert r[3] == 0.0 and math.isfinite(r[0]) and abs(r[0] - _exact_S(gh, None)) <= 2.0 ** -27 * r[0]
    assert r[2] == _d_prime(r[0], D, clip) and r[2] > 1e38
    assert same_bits(_host(g), gh)


# ---------------------------------------------------------------- the real objective
MAIN_SGD = dict(learningRate=1e-3, weightDecay=0.0005, momentum=0.9)     # main.lua:122-123
MAIN_NAG = dict(learningRate=1e-3, weightDecay=5e-4, momentum=0.9)       # main.lua:124, with a weight decay
MAIN_RMS = dict(learningRate=1e-3, alpha=0.9)                            # main.lua:122 rms_state
CFGS = dict(rmsprop=MAIN_RMS, sgd=MAIN_SGD, nag=MAIN_NAG)
STATE_KEY = dict(rmsprop="m", sgd="dfdx", nag="dfdx")


def _masks(F, model, it, k, H, W, rng):
    model["pnet"].drop_masks = [None] + [(rng.rand(c) > 0.4).astype(np.float32) for c in (128, 256, 384)]
    E = len(F.clean_examples(it.pool[k % 2]["positive"], F.output_map_sizes(model, H, W))) + \
        len(F.clean_examples(it.pool[k % 2]["negative"], F.output_map_sizes(model, H, W)))
    model["cnet"].drop_masks = [(rng.rand(E, 1024) > 0.5).astype(np.float32), (rng.rand(E, 512) > 0.5).astype(np.float32)]
    return E


def _train(F, kind, steps, extra=None, manual_clip=None, train=None, H=225, W=400, profile=False):
    """`steps` training steps of the small loop of test_gpu_optim.py (deterministic mode, explicit dropout masks).
    extra: keys added to the optimiser's state (clipNorm / skipNonFinite).  manual_clip: the test itself is the guard -- it takes
    the pass from begin_fold, has frcnn_grad_clip compute S into a record of its own, recomputes D' on the host from S, uploads it
    and calls the EXISTING whole-vector entry point with that device divisor.
    -> (per step (loss, weights, gradient, state vector), stats, launches per kernel class, model)"""
    import torch
    model = F.vgg_small(dict(F.duplo_cfg))
    if train is not None:
        model["cfg"]["train"] = dict(train)
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=11)
    it = F.SyntheticBatchIterator(model, H=H, W=W, pool=2)
    stats = dict(pcls=[], preg=[], dcls=[], dreg=[])
    f = F.create_objective(model, w, g, it, stats)
    cfg = dict(CFGS[kind])
    if extra:
        cfg.update(extra)
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    if profile:
        F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    out = []
    state = None
    try:
        for k in range(steps):
            E = _masks(F, model, it, k, H, W, rng)
            if manual_clip is None:
                _, fx = getattr(F, kind)(f, w, cfg)
                torch.cuda.synchronize()
                out.append((fx[0], _host(w).copy(), _host(g).copy(), _host(cfg[STATE_KEY[kind]]).copy()))
                continue
            first = state is None
            if first:
                state = torch.zeros_like(w)
            elif kind == "nag":
                F._lib.call("frcnn_nag_lookahead", F.ptr(w), F.ptr(state), w.numel(), cfg["momentum"], F.stream_ptr())
                torch.autograd.graph.increment_version(w)
            finish, dfdx, gscale = f.begin_fold(w)
            assert gscale == 1.0 / E
            S = _host(_grad_clip(F, dfdx, None))[0]
            dp = torch.tensor([_d_prime(S, float(E), manual_clip)], dtype=torch.float64, device="cuda")
            if kind == "rmsprop":
                c = dict(lr=cfg["learningRate"], alpha=cfg["alpha"], eps=1e-8)
            elif kind == "sgd":
                c = dict(clr=cfg["learningRate"], wd=cfg["weightDecay"], mom=cfg["momentum"], omd=1 - cfg["momentum"], nesterov=False,
                         first=first)
            else:
                c = dict(clr=cfg["learningRate"], wd=cfg["weightDecay"], mom=cfg["momentum"], first=first)
            _update(F, kind, w, dfdx, state, gcount=dp, cfg=c)
            fx, _ = finish()
            torch.cuda.synchronize()
            out.append((fx, _host(w).copy(), _host(g).copy(), _host(state).copy()))
    finally:
        if profile:
            F._lib.call("frcnn_prof_enable", 0)
            F._lib.call("frcnn_prof_collect", la, ms, fl, by)
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        model["pnet"].drop_masks = None
        model["cnet"].drop_masks = None
    return out, stats, list(la), model


# ---------------------------------------------------------------- 6. end to end
@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_three_guarded_training_steps_equal_steps_with_a_host_made_divisor(F, kind):
    probe, pstats, _, _ = _train(F, kind, 1, extra=dict(skipNonFinite=True))
    norm0 = pstats["gnorm"][0]
    assert math.isfinite(norm0) and norm0 > 0 and pstats["skipped"] == 0
    clip = 0.5 * norm0
    guarded, stats, _, _ = _train(F, kind, 3, extra=dict(clipNorm=clip))
    manual, mstats, _, _ = _train(F, kind, 3, manual_clip=clip)
    assert len(stats["gnorm"]) == 3 and all(math.isfinite(v) and v > 0 for v in stats["gnorm"]) and stats["skipped"] == 0
    assert stats["gnorm"][0] == norm0 and "gnorm" not in mstats
    for k in ("pcls", "preg", "dcls", "dreg"):
        assert stats[k] == mstats[k], k
    for k, (a, b) in enumerate(zip(guarded, manual)):
        assert a[0] == b[0], "loss of step %d" % k
        for i, what in ((1, "weights"), (2, "gradient"), (3, "state")):
            assert same_bits(a[i], b[i]), "%s differ after step %d" % (what, k)
    # the first step was clipped: it differs from the unclipped probe step
    assert not same_bits(guarded[0][1], probe[0][1])


@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_guard_off_queues_what_a_state_without_the_keys_queues(F, kind):
    plain, pstats, pl, _ = _train(F, kind, 2, profile=True)
    off, ostats, ol, _ = _train(F, kind, 2, extra=dict(clipNorm=0, skipNonFinite=False), profile=True)
    none, nstats, nl, _ = _train(F, kind, 2, extra=dict(clipNorm=None, skipNonFinite=None), profile=True)
    on, sstats, sl, _ = _train(F, kind, 2, extra=dict(skipNonFinite=True), profile=True)
    for st in (pstats, ostats, nstats):
        assert "gnorm" not in st and "skipped" not in st
    assert pl == ol == nl, "launches per class differ with the guard off: %r / %r / %r" % (pl, ol, nl)
    i = F._lib.KC_NAMES.index("optim")
    assert [b - a for a, b in zip(pl, sl)] == [6 if j == i else 0 for j in range(len(pl))], "the guard is three launches per step"
    for a, b, c, d in zip(plain, off, none, on):
        for j in (1, 2, 3):
            assert same_bits(a[j], b[j]) and same_bits(a[j], c[j])
            assert same_bits(a[j], d[j]), "a guard that neither clips nor skips changed the step"
    assert len(sstats["gnorm"]) == 2


# ---------------------------------------------------------------- 5. frozen slices
STAGES = {
    "frozen_2": dict(proposal=True, classification=True, frozen_blocks=2),
    "cnet_only": dict(proposal=False, classification=True, frozen_blocks=4),
    "pnet_only": dict(proposal=True, classification=False, frozen_blocks=0),
}


@pytest.mark.parametrize("row", sorted(STAGES))
@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_staged_step_clips_over_the_trainable_slices_only(F, kind, row):
    """weights and optimiser state outside T stay bit-unchanged, T's are clipped (the _slice_dev forms: a staged step with a
    device divisor used to raise); S over T equals S over the whole vector (frozen slices of the gradient are exact zeros)"""
    import torch
    train = STAGES[row]
    probe, pstats, _, model = _train(F, kind, 1, extra=dict(skipNonFinite=True), train=train)
    clip = 0.5 * pstats["gnorm"][0]
    w0 = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=11)[0].cpu().numpy()
    (loss, w1, g1, s1), = _train(F, kind, 1, extra=dict(clipNorm=clip), train=train)[0]
    # T as the objective publishes it
    m2 = F.vgg_small(dict(F.duplo_cfg)); m2["cfg"]["train"] = dict(train)
    w, g = F.combine_and_flatten_parameters(m2["pnet"], m2["cnet"], seed=11)
    it = F.SyntheticBatchIterator(m2, H=225, W=400, pool=2)
    f = F.create_objective(m2, w, g, it, dict(pcls=[], preg=[], dcls=[], dreg=[]))
    ranges = f.trainable_ranges()
    assert ranges is not None
    inside = np.zeros(w0.size, bool)
    for lo, hi in ranges:
        inside[lo:hi] = True
    assert same_bits(w1[~inside], w0[~inside]), "frozen weights moved"
    assert not np.any(s1[~inside]) and not np.any(g1[~inside]), "frozen state / gradient touched"
    assert not same_bits(w1[inside], w0[inside])
    assert not same_bits(w1[inside], probe[0][1][inside]), "the step was not clipped"
    # the norm g is left holding over T is the clip norm (rmsprop leaves the scaled gradient; sgd / nag add wd*x: looser)
    if kind == "rmsprop":
        after = math.sqrt(_exact_S(g1, ranges))
        assert abs(after - clip) <= 2.0 ** -22 * clip
    # S over T == S over the whole vector, on the gradient of a pass (unscaled: begin_fold leaves gradient:div to the caller)
    rng = np.random.RandomState(5)
    F._lib.call("frcnn_set_option", b"deterministic", 1)
    try:
        _masks(F, m2, it, 0, 225, 400, rng)
        finish, dfdx, gscale = f.begin_fold(w)
        a = _host(_grad_clip(F, dfdx, ranges))[0]
        b = _host(_grad_clip(F, dfdx, None))[0]
        finish()
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
        m2["pnet"].drop_masks = None
        m2["cnet"].drop_masks = None
    assert a == b and a > 0
    assert math.sqrt(a) * gscale == pytest.approx(pstats["gnorm"][0], rel=1e-12)


# ---------------------------------------------------------------- with a plain opfunc: D = 1
@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
def test_plain_opfunc_is_clipped_with_divisor_one(F, kind):
    import torch
    n = 10_007
    xh, gh, _ = _vectors(n, 6)
    x = _dev(xh)
    cfg = dict(CFGS[kind], clipNorm=0.25)
    gd = _dev(gh)
    getattr(F, kind)(lambda w: (0.0, gd), x, cfg)
    rec = _host(cfg["_guard"]["record"])
    S = _exact_S(gh, None)
    assert abs(rec[0] - S) <= 2.0 ** -27 * S and rec[2] == _d_prime(rec[0], 1.0, 0.25) and rec[3] == 0.0
    x2, g2 = _dev(xh), _dev(gh)
    cfg2 = dict(CFGS[kind])
    up = torch.tensor([rec[2]], dtype=torch.float64, device="cuda")

    class Divisor(object):
        ptr = up.data_ptr()
    # the same optimiser on an opfunc that speaks begin_fold and hands out D' as its device divisor
    op = lambda w: (0.0, g2)
    op.begin_fold = lambda w: ((lambda: (0.0, g2)), g2, Divisor)
    getattr(F, kind)(op, x2, cfg2)
    assert same_bits(_host(x), _host(x2)) and same_bits(_host(gd), _host(g2))
    assert same_bits(_host(cfg[STATE_KEY[kind]]), _host(cfg2[STATE_KEY[kind]]))


# ---------------------------------------------------------------- 7. errors
def test_grad_clip_rejects_bad_arguments_before_queueing(F):
    import torch
    n = 1000
    gh = np.arange(n, dtype=np.float32)
    g = _dev(gh)
    nbytes = F._lib.load().frcnn_grad_clip_workspace_bytes(n)
    assert nbytes >= 8 and F._lib.load().frcnn_grad_clip_workspace_bytes(VGG_SMALL_PARAMS) <= 1 << 20
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    rec = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    ok = dict(g=F.ptr(g), n=n, ranges=None, divisor=1.0, ddev=None, clip=1.0, rec=F.ptr(rec), ws=F.ptr(ws), wsb=nbytes)

    def call(**kw):
        a = dict(ok); a.update(kw)
        flat, nr = _flat(a["ranges"])
        if "nranges" in a:
            nr = a["nranges"]
        F._lib.call("frcnn_grad_clip", a["g"], a["n"], flat, nr, a["divisor"], a["ddev"], a["clip"], a["rec"], a["ws"], a["wsb"],
                    F.stream_ptr())
    bad = [
        dict(g=None), dict(rec=None), dict(ws=None), dict(n=-1),
        dict(g=C.c_void_p(g.data_ptr() + 4)),                        # misaligned gradient
        dict(rec=C.c_void_p(rec.data_ptr() + 4)),                    # misaligned record
        dict(ranges=[(10, 5)]),                                      # lo > hi
        dict(ranges=[(0, 10), (5, 20)]),                             # overlapping
        dict(ranges=[(20, 30), (0, 10)]),                            # unsorted
        dict(ranges=[(0, n + 1)]), dict(ranges=[(-1, 4)]),           # out of the vector
        dict(ranges=[(i, i + 1) for i in range(17)]),                # more slices than the launch carries
        dict(ranges=None, nranges=2),                                # a count without a list
        dict(wsb=nbytes - 8),                                        # short workspace
        dict(divisor=0.0), dict(divisor=-2.0), dict(divisor=float("nan")),
        dict(clip=float("nan")), dict(clip=float("inf")),
    ]
    for kw in bad:
        with pytest.raises(F.FrcnnError):
            call(**kw)
    torch.cuda.synchronize()
    assert same_bits(_host(g), gh) and np.all(_host(rec) == -7.0), "something was queued by a rejected call"
    call()   # and the good call works
    assert _host(rec)[0] == _exact_S(gh, None)
    for name in ("frcnn_scale_rmsprop_slice_dev", "frcnn_sgd_slice_dev", "frcnn_nag_slice_dev"):
        x = _dev(gh); s = _dev(gh)
        with pytest.raises(F.FrcnnError):    # NULL divisor
            if name == "frcnn_scale_rmsprop_slice_dev":
                F._lib.call(name, F.ptr(x), F.ptr(g), None, F.ptr(s), 0, n, 1e-2, 0.9, 1e-8, F.stream_ptr())
            elif name == "frcnn_sgd_slice_dev":
                F._lib.call(name, F.ptr(x), F.ptr(g), F.ptr(s), 0, n, None, 1e-3, 0.0, 0.9, 1.0, 0, 0, F.stream_ptr())
            else:
                F._lib.call(name, F.ptr(x), F.ptr(g), F.ptr(s), 0, n, None, 1e-3, 0.0, 0.9, 0, F.stream_ptr())
        assert same_bits(_host(x), gh)


@pytest.mark.parametrize("kind", ["rmsprop", "sgd", "nag"])
@pytest.mark.parametrize("extra,exc", [
    (dict(clipNorm=float("nan")), ValueError),
    (dict(clipNorm=-1.0), ValueError),
    (dict(clipNorm=float("inf")), ValueError),
    (dict(clipNorm="0.5"), ValueError),
    (dict(clipNorm=True), ValueError),
    (dict(skipNonFinite="yes"), ValueError),
    (dict(clipNorm=1.0, eager=True), None),
    (dict(skipNonFinite=True, eager=True), None),
])
def test_bad_guard_settings_raise_without_touching_x(F, kind, extra, exc):
    x0 = np.arange(16, dtype=np.float32)
    x = _dev(x0)
    calls = []
    cfg = dict(CFGS[kind]); cfg.update(extra)
    with pytest.raises(exc or F.FrcnnError):
        getattr(F, kind)(lambda w: calls.append(1), x, cfg)
    assert not calls and same_bits(_host(x), x0)
    assert "dfdx" not in cfg and "evalCounter" not in cfg and "_guard" not in cfg
