"""The launches of a channel-compact dropout block (option drop_compact, on by default) op by op, through the test-facing entry
points of include/frcnn_hip_compact.h: the gathered weight packs of csrc/convx.hip (pack_x_job with PackXJob::oidx / cidx / Cs /
bias_dst, through the multi-job pack launch a training step uses) feeding conv_x3 forward and backward, and the weight
gradient of csrc/wgradx.hip folded through a WgradMap (csrc/conv.hip wgrad_reduce_map_kernel; the bias gradient follows the
filter map inside the kernel).  tests/compact_plan.py holds the case tables and the numpy restatement of the gather and the
scatter, tests/test_compact_plan.py checks them without a GPU.  Every case runs in both operand forms (option x3_f16).

Each of the six launches of a block (compact_plan.ROLES) meets, per case:
  the fp64 reference    the dense operation by its definition (conv_plan.ref_*) on the HOST-gathered operands: the project's bar
                        |a - b| <= 1e-4 max(1, |b|), the worst-case bound convx_plan.split_bound with n = P 9 K of the launch
                        (in the fp16 form the representation share takes the FULL weight tensor's largest magnitude, which is
                        what the gathered pack scales by), all values finite, stores into NaN-filled destinations (every other
                        case 4 bytes into a larger NaN-filled buffer that must stay NaN);
  the plain entry point the same bits as frcnn_conv2d_forward / _backward_input / _backward_input_rec on the host-gathered
                        weights: always in the three-plane form (behind the fused activation backward, which has a plain
                        entry point in the fp16 form only: the plain input gradient put through the epilogue's one fp32
                        multiplication on the host), in the fp16 form where the tensor's largest magnitude lies in the kept
                        part; the mapped weight gradient the same bits as frcnn_conv2d_backward_weight on the compact tensors
                        scatter-added on the host into the (non-zero) initial gradient; the bias gradient, whose partial
                        sums meet in atomics, the bound only;
  zeros and sentinels   rows of a negative table entry are exactly +0, also behind the fused activation backward, and do not move
                        the slope gradient (their pre-activations are set to -1e30); filters / channels of the weight and bias
                        gradients that the map does not name keep the bits of distinct finite sentinels; channels of the compact
                        input beyond the nkK the launch reads are NaN and must not show;
  the precision gate    RMS_GATE of tests/test_gpu_convx.py against the fp32 matrix-core kernel (the plain entry point with
                        split_bf16 = 0 on the gathered operands), over the rows a table entry names, for the forward and
                        input-gradient cases that reach POOL such outputs within four seeds.
Further tests: two NULL tables over a larger tensor read it at its own row pitch; the fp16 scale is the full tensor's (bit for
bit against a plain launch whose weights carry the full tensor's largest magnitude in a padding row / channel -- a pack scaled by
the gathered part's magnitude gives other low planes);
independence of the result from where the kept filters lie and from which entry is padding; refusals launch and store nothing;
the six launches of one block in the model's order on the device's own intermediate tensors (the structural facts the op tests
assume of each other: padding rows exactly zero, dropped rows untouched).

Measured on an MI355X, 2026-10-21 (every ratio is printed; the last test of the file prints the worst per role and form),
bf16x6 / f16x3:
  largest error / bound      fwd0 0.0012 (c128_k15) / 0.0014 (c128_k112); fwd1 0.0049 / 0.0101 (c128_k1); dgrad1 0.0014 (c128_k64) /
                             0.0016 (c192_k176), behind the activation backward 0.0010 / 0.0017 (c128_k15), slope gradient
                             < 0.0001; dgrad0 0.0039 / 0.0073 (c128_k1, accumulating); wgrad1 0.0104 / 0.0142 and wgrad0 0.0075 /
                             0.0140 (wg_one_tile, wg_one_tile_first); bias gradient 0.0066 (wgrad1, c128_k16) and 0.0062 (wgrad0,
                             c192_k65_last) in both forms.  As in tests/test_gpu_convx_plans.py the bound is a worst case over n
                             roundings, a hundred times above what random data does: it notices a lost or misplaced product.
  largest gate ratio         fwd0 1.202 (c128_k65) / 0.908; fwd1 1.608 / 1.184 (c128_k112); dgrad1 1.215 (c128_k63) / 0.920, behind
                             the activation backward 1.215 / 0.921; dgrad0 1.626 (c128_k112) / 1.189 (c128_k112_first); RMS_GATE
                             is 1.75.  Geometric mean over the file's 128 ratios 1.0497 against MEAN_GATE = 1.05: close, and
                             stable (fixed seeds, no atomics in these launches).  It is the mean of this file's mix, not a
                             property of the gather -- every gated result equals the plain entry point's bit for bit: half the
                             ratios are three-plane launches of K = 64 channels on a 9 x 12 to 12 x 16 map, which sit at 1.17 to
                             1.21 (the two-plane form at 0.88 to 0.92), and the seven-chunk launches of nk = 112 at 1.6 / 1.19,
                             the one-slab-against-many-slabs effect tests/test_gpu_convx_plans.py derives from the rounding count.
What this file found: nothing wrong in the kernels or in net.cpp.  (The pack reads PackXJob::Cs only in its gathered branch; the
model never builds a job with Cs and no table, the entry points add an identity table where a caller does.)  Each of these,
tried on a scratch copy of the sources, makes tests of this file fail: the source row pitch Cs replaced by the launch's channel
count in the gathered tile fill (every fwd1 and
dgrad1 case of test_gathered_convolution, test_f16_scale_is_the_full_tensors, test_result_does_not_depend_on_where_the_kept_
filters_lie); bias_dst without its `o >= 0 ? ... : 0` (the fwd0 cases with padding rows: a padding row is not exactly +0; the
swap and the contract tests); omap ignored for gbias (every wgrad0 case of test_mapped_weight_gradient, the swap, independence
and contract tests); `cd >= 0` dropped in wgrad_reduce_map_kernel, for the filters where that stays inside the tensor (every
wgrad1 case with a padding channel, the independence and contract tests); the gathered pack scaled by the gathered part's
magnitude instead of the full tensor's (the six cases of test_f16_scale_is_the_full_tensors, and nothing else: that result is
as accurate, only not what a training step computes)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import compact_plan as KP
import conv_plan as CP
import convx_plan as XP
import test_gpu_convx_plans as TP
from test_gpu_convx import MEAN_GATE, RMS_GATE
from test_gpu_convx_plans import FORMS, POOL, Placed, _dest, _dev, options   # noqa: F401  (options: the fixture)
from util import assert_close

pytestmark = pytest.mark.gpu

PAD = KP.PAD
SLOPE = KP.SLOPE
MAX_REPS = 4
WORST = {}        # (role, form) -> (largest error / bound, run)
GATE_WORST = {}   # (role, form) -> (largest gate ratio, run)
RATIOS = []


def Gate():
    """convx_plans' pooled squared errors, recorded in this file's own lists"""
    return TP.Gate(RATIOS, GATE_WORST)


_check = functools.partial(TP._check, worst=WORST)   # all finite, the bar, the worst-case bound; the ratio is printed


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape
    n = int((a != b).sum())
    assert n == 0, "%s: %d of %d elements differ in their bits" % (what, n, a.size)


def _itab(F, t):
    return None if t is None else F.DeviceTensor.from_numpy(np.ascontiguousarray(t, np.int32))


def _misaligned(what):
    return bool(zlib.crc32(what.encode()) & 1)


def _read_tensor(F, d):
    """the tensor the launch reads, with the rows its producer gives it: those beyond the launch's K are NaN"""
    rows = d["L"].get("rows", d["K"])
    a = np.full((rows, d["H"], d["W"]), np.nan, np.float32)
    a[:d["K"]] = d["x"]
    return _dev(F, a)


# ---- the two entry points and their plain counterparts ----------------------------------------------------------------------
def _fwd_gathered(F, d, dx, dw, db, dsl, out, oidx=None, cidx=None):
    O_full, C_full = d["L"]["full"]
    F._lib.call("frcnn_conv2d_forward_gathered", F.ptr(dx), d["H"], d["W"], F.ptr(dsl), None, F.ptr(dw), F.ptr(db), O_full, C_full,
                F.ptr(oidx), d["nO"], F.ptr(cidx), d["nC"], PAD, F.ptr(out.t), None, None, F.stream_ptr())
    return out.read()


def _fwd_plain(F, d, dxg, dwg, dbg, dsl, out):
    F._lib.call("frcnn_conv2d_forward", F.ptr(dxg), d["nC"], d["H"], d["W"], F.ptr(dsl), None, F.ptr(dwg), F.ptr(dbg), d["nO"], 3, PAD,
                F.ptr(out.t), F.stream_ptr())
    return out.read()


def _dgrad_gathered(F, d, dg, dw, gin, acc, oidx=None, cidx=None, post=None):
    O_full, C_full = d["L"]["full"]
    px, psl, gsl = post if post else (None, None, None)
    F._lib.call("frcnn_conv2d_backward_input_gathered", F.ptr(dg), d["H"], d["W"], F.ptr(dw), O_full, C_full, F.ptr(oidx), d["nO"],
                F.ptr(cidx), d["nC"], PAD, F.ptr(gin.t), int(acc), None, None, F.ptr(px), F.ptr(psl), None, F.ptr(gsl), F.stream_ptr())
    return gin.read()


def _dgrad_plain(F, d, dgg, dwg, gin, acc, post=None):
    if post:
        px, psl, gsl = post
        F._lib.call("frcnn_conv2d_backward_input_rec", F.ptr(dgg), d["nO"], d["H"], d["W"], F.ptr(dwg), d["nC"], 3, PAD, F.ptr(gin.t), 0,
                    None, None, F.ptr(px), F.ptr(psl), None, F.ptr(gsl), F.stream_ptr())
    else:
        F._lib.call("frcnn_conv2d_backward_input", F.ptr(dgg), d["nO"], d["H"], d["W"], F.ptr(dwg), d["nC"], 3, PAD, F.ptr(gin.t),
                    int(acc), F.stream_ptr())
    return gin.read()


def _rep_bound(d, form):
    """the representation share: the weights' magnitude is the FULL tensor's, the input's the raw tensor's (|slope| < 1)"""
    return XP.representation_bound(d["op"], d["act"], d["wg"], form, amax_a=float(np.abs(d["x"]).max()),
                                   amax_b=float(np.abs(d["w"]).max()))


# ---- the four convolution roles ------------------------------------------------------------------------------------------------
CONV_RUNS = [r for r in KP.runs() if r["role"] in KP.CONV_ROLES]


@pytest.mark.parametrize("r", CONV_RUNS, ids=KP.run_id)
def test_gathered_convolution(F, options, r):
    role, what = r["role"], KP.run_id(r)
    fwd, acc = role in ("fwd0", "fwd1"), role == "dgrad0"
    L = KP.launch_of_run(r)
    plan = XP.x3_plan(L["shape"], post=r["post"])
    live_out = L["live"] * L["H"] * L["W"]
    reps = min(MAX_REPS, XP.cdiv(POOL, live_out))
    gated = reps * live_out >= POOL
    gates = {form: Gate() for form in FORMS}
    aligned = not _misaligned(what)
    for rep in range(reps):
        d = KP.conv_inputs(r, rep)
        rng = d["rng"]
        live = KP.live_rows(d)
        shape = d["want"].shape
        start = rng.randn(*shape).astype(np.float32) if acc else np.full(shape, np.nan, np.float32)
        want, mag = (d["want"] + start, d["mag"] + np.abs(start)) if acc else (d["want"], d["mag"])
        dx, dxg = _read_tensor(F, d), _dev(F, d["x"])
        dw, dwg = _dev(F, d["w"]), _dev(F, d["wg"])
        db, dbg = (_dev(F, d["b"]), _dev(F, d["bg"])) if fwd else (None, None)
        dsl = _dev(F, [d["slope"]]) if d["slope"] is not None else None
        oidx, cidx = _itab(F, d["oidx"]), _itab(F, d["cidx"])
        px = gslope0 = None
        if r["post"]:
            px = rng.randn(*shape).astype(np.float32)
            px[0, 0, 0] = 0.0                               # x = 0 takes the slope's branch
            px[~live] = np.float32(-1e30)                   # a padding row times anything but an exact zero would show
            gslope0 = np.float32(rng.randn() * 50.0)
            dpx, dpsl = _dev(F, px), _dev(F, [SLOPE])
            fs = np.where(px > 0, 1.0, float(SLOPE))
            neg = px <= 0
            conv = d["want"]
            want = fs * conv
            want_slope = float(gslope0) + float((px.astype(np.float64) * conv)[neg].sum())

        def gathered():
            out = _dest(F, start, aligned)
            if fwd:
                return _fwd_gathered(F, d, dx, dw, db, dsl, out, oidx, cidx), None
            if r["post"]:
                gsl = _dev(F, [gslope0])
                return _dgrad_gathered(F, d, dx, dw, out, 0, oidx, cidx, (dpx, dpsl, gsl)), gsl.numpy()
            return _dgrad_gathered(F, d, dx, dw, out, acc, oidx, cidx), None

        def plain(post_ok=True):
            out = _dest(F, start, aligned)
            if fwd:
                return _fwd_plain(F, d, dxg, dwg, dbg, dsl, out)
            if r["post"] and post_ok:
                return _dgrad_plain(F, d, dxg, dwg, out, 0, (dpx, dpsl, _dev(F, [gslope0])))
            return _dgrad_plain(F, d, dxg, dwg, out, acc)
        options("split_bf16", 0)
        direct = plain(post_ok=False)
        if r["post"]:   # the fp32 kernel's convolution through the same fp32 multiplication on the host
            direct = np.where(px > 0, direct, SLOPE * direct).astype(np.float32)
        assert_close(direct, want, 1e-4, "fp32 matrix-core kernel on the gathered operands, %s (the gate's denominator)" % what)
        options("split_bf16", 1)
        for form in FORMS:
            options("x3_f16", form)
            got, got_slope = gathered()
            n, S = XP.PRODUCTS[form] * plan["K"], plan["splitK"]
            rep_b = _rep_bound(d, form)
            if r["post"]:
                conv_bound = XP.split_bound(n, S, d["mag"], rep_b, extra=4)
                _check(role + "_post", form, what, got, want, np.abs(fs) * conv_bound)
                xs = np.where(neg & live[:, None, None], np.abs(px.astype(np.float64)), 0.0)
                slope_bound = float((xs * conv_bound).sum()) + (int(neg.sum()) + 2) * CP.U * XP.MAG_SLACK * (
                    float((xs * d["mag"]).sum()) + abs(float(gslope0)))
                _check(role + "_slope_gradient", form, what, got_slope, np.array([want_slope]), np.array([slope_bound]))
            else:
                _check(role, form, what, got, want, XP.split_bound(n, S, mag, rep_b))
            # rows of a negative entry: exactly +0
            if not acc:
                assert not _bits(got[~live]).any(), "%s %s: a padding row is not exactly +0" % (what, FORMS[form])
            # the plain entry point on the host-gathered operands: the same bits
            if form == 0 or KP.amax_lies_in_kept(d["w"], d["kept"], L["gather"]):
                if r["post"] and form == 0:
                    # frcnn_conv2d_backward_input_rec exists in the fp16 form only: the plain input gradient, put through the
                    # epilogue's one fp32 multiplication on the host (convx.hip: g = acc * 1, stored as x > 0 ? g : slope * g)
                    v = plain(post_ok=False)
                    _same_bits(got, np.where(px > 0, v, SLOPE * v).astype(np.float32),
                               "%s %s against the plain input gradient and the activation backward on the host" % (what, FORMS[form]))
                else:
                    _same_bits(got, plain(), "%s %s against the plain entry point" % (what, FORMS[form]))
            gates[form].add(got[live], direct[live], want[live])
    if gated:
        got = {FORMS[form]: g.ratio(role + ("_post" if r["post"] else ""), form, what) for form, g in sorted(gates.items())}
        bad = {f: round(x, 3) for f, (x, ok) in got.items() if not ok}
        assert not bad, "%s: rms error above %.2f times the fp32 kernel's: %r" % (what, RMS_GATE, bad)


# ---- two NULL tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORMS[f] for f in sorted(FORMS)])
def test_two_null_tables_read_the_full_tensor_at_its_own_pitch(F, options, form):
    """oidx = cidx = NULL over a tensor with more filters and channels than the launch: the first nO filters by the first nC
    channels, read at the row pitch C_full (the pack honours PackXJob::Cs in its gathered branch only: the entry point hands it an
    identity channel table).  The same bits as the plain entry points on the host-sliced weights, forward and input gradient."""
    options("split_bf16", 1)
    options("x3_f16", form)
    O_full, C_full, nO, nC, H, W = 128, 192, 64, 80, 9, 12
    rng = KP.rng_of("two null tables")
    w = (rng.randn(O_full, C_full, 3, 3) / np.sqrt(nC * 9)).astype(np.float32)
    b = rng.randn(O_full).astype(np.float32)
    w[3, 5, 1, 1] = np.float32(2.0 * np.abs(w).max())        # the tensor's largest magnitude lies inside both slices
    nan = lambda *s: np.full(s, np.nan, np.float32)   # noqa: E731
    dw = _dev(F, w)
    for mode, (n_o, n_c) in (("fwd", (nO, nC)), ("dgrad", (nC, nO))):      # (the input gradient: K = n_o % 16, M = n_c % 64)
        wg = np.ascontiguousarray(w[:n_o, :n_c])
        d = dict(L=dict(full=(O_full, C_full)), H=H, W=W, nO=n_o, nC=n_c)
        K, M = (n_c, n_o) if mode == "fwd" else (n_o, n_c)
        x = rng.randn(K, H, W).astype(np.float32)
        dx, dwg = _dev(F, x), _dev(F, wg)
        if mode == "fwd":
            got = _fwd_gathered(F, d, dx, dw, _dev(F, b), None, _dest(F, nan(M, H, W)))
            ref = _fwd_plain(F, d, dx, dwg, _dev(F, b[:n_o]), None, _dest(F, nan(M, H, W)))
            want = CP.ref_forward(x, wg, b[:n_o], PAD)
        else:
            got = _dgrad_gathered(F, d, dx, dw, _dest(F, nan(M, H, W)), 0)
            ref = _dgrad_plain(F, d, dx, dwg, _dest(F, nan(M, H, W)), 0)
            want = CP.ref_input_gradient(x, wg, PAD, H, W)
        assert_close(got, want, 1e-4, "two NULL tables, %s %s" % (mode, FORMS[form]))
        _same_bits(got, ref, "two NULL tables, %s %s" % (mode, FORMS[form]))


# ---- the fp16 scale ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,role", [("c128_k63", "fwd0"), ("c192_k65", "fwd0"), ("c128_k63", "fwd1"), ("c192_k65", "fwd1"),
                                        ("c128_k65", "dgrad1"), ("c192_k65", "dgrad0")])
def test_f16_scale_is_the_full_tensors(F, options, name, role):
    """amax_in_dropped: a dropped filter / channel carries weights 2^10 times the kept ones.  The gathered pack scales by the FULL
    tensor's largest magnitude (net.cpp pack_compact: g.amax = j.amax), so its planes are those of a plain pack whose tensor has the
    same largest magnitude: the plain entry point on the host-gathered weights with that magnitude planted in a padding row /
    channel (whose own output is set aside; a padding channel of the input is zero, as its producer leaves it) gives the same
    bits.  A pack scaled by the gathered part's own magnitude would fill the low planes differently."""
    r = dict(name=name, role=role, post=False)
    d = KP.conv_inputs(r)
    L, fwd = d["L"], role in ("fwd0", "fwd1")
    assert d["case"]["amax"] == "dropped" and not KP.amax_lies_in_kept(d["w"], d["kept"], L["gather"])
    nk = L["nk"]
    top = np.float32(np.abs(d["w"]).max())
    wg, x = d["wg"].copy(), d["x"].copy()
    out_rows = np.ones(d["M"], bool)
    if role in ("fwd0", "dgrad0"):      # oidx: filter nk of the launch is padding
        assert d["nO"] > nk and not wg[nk].any()
        wg[nk, 0, 1, 1] = top
        if role == "fwd0":
            out_rows[nk] = False          # its output row is not zero in the plain launch
        else:
            x[nk] = 0.0                   # K channel nk of the compact gradient: zero, as the launch before leaves it
    else:                                # cidx: channel nk of the launch is padding
        assert d["nC"] > nk and not wg[:, nk].any()
        wg[0, nk, 1, 1] = top
        if role == "fwd1":
            x[nk] = 0.0
        else:
            out_rows[nk] = False
    d["x"] = x
    options("split_bf16", 1)
    options("x3_f16", 1)
    dx, dxg, dw, dwg = _read_tensor(F, d), _dev(F, x), _dev(F, d["w"]), _dev(F, wg)
    oidx, cidx = _itab(F, d["oidx"]), _itab(F, d["cidx"])
    shape = d["want"].shape
    nan = np.full(shape, np.nan, np.float32)
    if fwd:
        dsl = _dev(F, [d["slope"]]) if d["slope"] is not None else None
        got = _fwd_gathered(F, d, dx, dw, _dev(F, d["b"]), dsl, _dest(F, nan), oidx, cidx)
        ref = _fwd_plain(F, d, dxg, dwg, _dev(F, d["bg"]), dsl, _dest(F, nan))
    else:
        got = _dgrad_gathered(F, d, dx, dw, _dest(F, nan), 0, oidx, cidx)
        ref = _dgrad_plain(F, d, dxg, dwg, _dest(F, nan), 0)
    _same_bits(got[out_rows], ref[out_rows], "%s %s: planes scaled by the full tensor's magnitude" % (role, name))
    # the control: the plain launch on the gathered weights alone scales by THEIR magnitude and gives other bits
    if fwd:
        own = _fwd_plain(F, d, dxg, _dev(F, d["wg"]), _dev(F, d["bg"]), dsl, _dest(F, nan))
    else:
        own = _dgrad_plain(F, d, dxg, _dev(F, d["wg"]), _dest(F, nan), 0)
    assert (_bits(own[out_rows]) != _bits(got[out_rows])).any(), "the two scales give the same bits: the test cannot tell them apart"


# ---- the mapped weight gradient ----------------------------------------------------------------------------------------------------
def _sentinels(shape):
    """distinct finite values in [1, 1.5): an initial gradient of the size of what is added to it"""
    n = int(np.prod(shape))
    assert n <= 1 << 19
    return (1.0 + np.arange(n, dtype=np.float64) / (1 << 20)).astype(np.float32).reshape(shape)


def _wgrad_inputs(r, seed=0):
    c, L = KP.find(r["name"]), KP.launch_of_run(r)
    rng = KP.rng_of("compact wgrad", r["name"], r["role"], seed)
    Cin, H, W, O = L["shape"][:4]
    kept = KP.kept_set(c["C"], c["nk"], c["kind"])
    idx = KP.table(c["C"], kept)
    O_full, C_full = L["full"]
    # every row of the compact tensors carries data, the padding rows too: the map, not a zero, must keep them out
    x = rng.randn(Cin, H, W).astype(np.float32)
    g = (rng.randn(O, H, W) / np.sqrt(H * W)).astype(np.float32)
    gw0 = _sentinels((O_full, C_full, 3, 3)) * rng.choice(np.array([-1.0, 1.0], np.float32), (O_full, C_full, 3, 3))
    gb0 = -2 * _sentinels((O_full,))
    slope = SLOPE if r["role"] == "wgrad1" else None       # (b, 1) reads (b, 0)'s pre-activations through their PReLU
    omap, cmap = (None, idx) if L["gather"] == "c" else (idx, None)
    return dict(L=L, Cin=Cin, H=H, W=W, O=O, O_full=O_full, C_full=C_full, x=x, g=g, gw0=gw0, gb0=gb0, slope=slope, omap=omap, cmap=cmap,
                kept=kept, idx=idx)


def _wgrad_mapped(F, q, dx, dg, dsl, gw0, gb0, omap, cmap):
    gw, gb = _dev(F, gw0), _dev(F, gb0)
    F._lib.call("frcnn_conv2d_backward_weight_mapped", F.ptr(dx), q["Cin"], q["H"], q["W"], F.ptr(dsl), None, F.ptr(dg), q["O"], PAD,
                F.ptr(gw), F.ptr(gb), q["O_full"], q["C_full"], F.ptr(omap), F.ptr(cmap), F.stream_ptr())
    return gw.numpy(), gb.numpy()


def _wgrad_plain(F, q, dx, dg, dsl):
    gw, gb = F.DeviceTensor.zeros((q["O"], q["Cin"], 3, 3)), F.DeviceTensor.zeros((q["O"],))
    F._lib.call("frcnn_conv2d_backward_weight", F.ptr(dx), q["Cin"], q["H"], q["W"], F.ptr(dsl), None, F.ptr(dg), q["O"], 3, PAD,
                F.ptr(gw), F.ptr(gb), F.stream_ptr())
    return gw.numpy(), gb.numpy()


def _named(q):
    """-> (o', c', o, c): the launch's filters / channels with a non-negative entry and where they land"""
    o = np.arange(q["O"]) if q["omap"] is None else q["omap"][:q["O"]]
    c = np.arange(q["Cin"]) if q["cmap"] is None else q["cmap"][:q["Cin"]]
    oo, cc = np.nonzero(o >= 0)[0], np.nonzero(c >= 0)[0]
    return oo, cc, o[oo], c[cc]


WG_RUNS = [r for r in KP.runs() if r["role"] in ("wgrad1", "wgrad0")]


@pytest.mark.parametrize("r", WG_RUNS, ids=KP.run_id)
def test_mapped_weight_gradient(F, options, r):
    what = KP.run_id(r)
    q = _wgrad_inputs(r)
    plan = XP.wgradx_plan(q["L"]["shape"])
    act = CP.activate(q["x"], q["slope"], None)
    op = lambda a, b: CP.ref_weight_gradient(a, b, 3, PAD)[0]   # noqa: E731
    part, part_b = CP.ref_weight_gradient(act, q["g"], 3, PAD)
    mw, mb = CP.ref_weight_gradient(np.abs(act), np.abs(q["g"]), 3, PAD)
    oo, cc, o, c = _named(q)
    sel, land = np.ix_(oo, cc), np.ix_(o, c)
    want = q["gw0"][land].astype(np.float64) + part[sel]
    want_b = q["gb0"][o].astype(np.float64) + part_b[oo]
    dx, dg = Placed(F, q["x"], "slack"), Placed(F, q["g"], "slack")
    dsl = _dev(F, [q["slope"]]) if q["slope"] is not None else None
    omap, cmap = _itab(F, q["omap"]), _itab(F, q["cmap"])
    options("split_bf16", 1)
    for form in FORMS:
        options("x3_f16", form)
        got, got_b = _wgrad_mapped(F, q, dx.t, dg.t, dsl, q["gw0"], q["gb0"], omap, cmap)
        rep_b = XP.representation_bound(op, act, q["g"], form, amax_a=float(np.abs(q["x"]).max()))
        bound = XP.split_bound(XP.PRODUCTS[form] * plan["K"], plan["nSplit"], mw + 0.0, rep_b)[sel] + (
            plan["nSplit"] + 2) * CP.U * np.abs(q["gw0"][land])
        _check(r["role"], form, what, np.ascontiguousarray(got[land]), want, bound)
        _check(r["role"] + "_bias", form, what, got_b[o], want_b, CP.rounding_bound(plan["K"], 1, mb[oo] + np.abs(q["gb0"][o])))
        # what the map does not name keeps its bits
        rest = np.ones(got.shape, bool)
        rest[land] = False
        assert rest.any() and np.array_equal(_bits(got)[rest], _bits(q["gw0"])[rest]), "%s: an unnamed filter / channel was written" % what
        rest_b = np.ones(q["O_full"], bool)
        rest_b[o] = False
        assert np.array_equal(_bits(got_b)[rest_b], _bits(q["gb0"])[rest_b]), "%s: the bias gradient of an unnamed filter was written" % what
        assert (q["omap"] is None) == (not rest_b.any())
        # the unmapped fold on the compact tensors, scatter-added on the host in fp32: the same bits
        pw, _ = _wgrad_plain(F, q, dx.t, dg.t, dsl)
        expect = KP.scatter_add(q["gw0"].copy(), pw, q["omap"], q["cmap"])
        _same_bits(got, expect, "%s %s against frcnn_conv2d_backward_weight + a host scatter-add" % (what, FORMS[form]))
    assert np.array_equal(dx.read(), q["x"]) and np.array_equal(dg.read(), q["g"])


# ---- independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORMS[f] for f in sorted(FORMS)])
def test_result_does_not_depend_on_where_the_kept_filters_lie(F, options, form):
    """two kept sets with the same nk whose gathered operands are the same numbers (and, for the fp16 form, the same largest
    magnitude, planted in the kept part): the same bits, for a filter table, a channel table and both maps"""
    options("split_bf16", 1)
    options("x3_f16", form)
    C_, nk, H, W = 128, 17, 10, 13
    ka, kb = KP.kept_set(C_, nk, "ends"), KP.kept_set(C_, nk, "random", seed=5)
    assert ka != kb
    ta, tb = KP.table(C_, ka), KP.table(C_, kb)
    nan = lambda *s: np.full(s, np.nan, np.float32)   # noqa: E731
    for role in ("fwd0", "fwd1", "wgrad1", "wgrad0"):
        L = KP.launch(role, C_, nk, 64, (H, W))
        rng = KP.rng_of("independent", role)
        outs = []
        if role in ("fwd0", "fwd1"):
            wa, ba = KP.weights(rng, L["full"], ka, L["gather"], "kept")
            wb, bb = KP.weights(rng, L["full"], kb, L["gather"], None)
            wb *= np.float32(0.5)                    # (nothing of the second tensor's own exceeds the planted magnitude)
            if L["gather"] == "o":
                wb[kb], bb[kb] = wa[ka], ba[ka]
            else:
                wb[:, kb] = wa[:, ka]
                bb = ba
            assert float(np.abs(wa).max()) == float(np.abs(wb).max())
            K = L["shape"][0]
            x = _dev(F, rng.randn(K, H, W).astype(np.float32))
            for w, b, t in ((wa, ba, ta), (wb, bb, tb)):
                d = dict(L=L, H=H, W=W, nO=L["n"][0], nC=L["n"][1])
                it = _itab(F, t)
                oidx, cidx = (it, None) if L["gather"] == "o" else (None, it)
                outs.append(_fwd_gathered(F, d, x, _dev(F, w), _dev(F, b), None, _dest(F, nan(L["n"][0], H, W)), oidx, cidx))
            _same_bits(outs[0], outs[1], role)
        else:
            r = dict(name="c128_k17", role=role, post=False)
            q = _wgrad_inputs(r)
            assert q["kept"] == ka
            dx, dg = _dev(F, q["x"]), _dev(F, q["g"])
            dsl = _dev(F, [q["slope"]]) if q["slope"] is not None else None
            ga, gba = _wgrad_mapped(F, q, dx, dg, dsl, q["gw0"], q["gb0"], _itab(F, q["omap"]), _itab(F, q["cmap"]))
            gw0b, gb0b = q["gw0"][::-1].copy(), q["gb0"].copy()         # other sentinels, the named ones carried over
            if L["gather"] == "c":
                gw0b[:, kb] = q["gw0"][:, ka]
                gb, gbb = _wgrad_mapped(F, q, dx, dg, dsl, gw0b, gb0b, None, _itab(F, tb))
                _same_bits(ga[:, ka], gb[:, kb], role)
                assert np.allclose(gba, gbb, rtol=1e-5, atol=1e-5)      # (the bias sums meet in atomics)
                rest = sorted(set(range(C_)) - set(kb))
                _same_bits(gb[:, rest], gw0b[:, rest], role + ": unnamed channels")
            else:
                gw0b[kb], gb0b[kb] = q["gw0"][ka], q["gb0"][ka]
                gb, gbb = _wgrad_mapped(F, q, dx, dg, dsl, gw0b, gb0b, _itab(F, tb), None)
                _same_bits(ga[ka], gb[kb], role)
                rest = sorted(set(range(C_)) - set(kb))
                _same_bits(gb[rest], gw0b[rest], role + ": unnamed filters")
                _same_bits(gbb[rest], gb0b[rest], role + ": unnamed bias entries")
                # the bias sums meet in atomics: the same numbers to a rounding of their few partial sums
                assert np.allclose(gba[ka], gbb[kb], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORMS[f] for f in sorted(FORMS)])
def test_swapping_the_padding_entry_changes_only_the_rows_it_names(F, options, form):
    """a table with -1 in the MIDDLE: entry i or entry j of the same table made padding.  The forward, the input gradient behind
    its activation backward and the filter-mapped weight gradient differ only in rows i and j, which are +0 / untouched where
    their entry is negative"""
    options("split_bf16", 1)
    options("x3_f16", form)
    C_, nk, H, W = 128, 63, 9, 12
    kept = KP.kept_set(C_, nk, "random", seed=9)
    i, j = 5, 40
    tabs = []
    for hole in (i, j):
        t = KP.table(C_, kept)
        t[hole] = -1
        tabs.append(t)
    others = np.ones(64, bool)
    others[[i, j]] = False
    nan = lambda *s: np.full(s, np.nan, np.float32)   # noqa: E731
    # forward, filters gathered; the largest weight lies in kept filter 0 of both tables
    L = KP.launch("fwd0", C_, nk, 64, (H, W))
    rng = KP.rng_of("swap")
    w, b = KP.weights(rng, L["full"], kept, "o", "kept")
    d = dict(L=L, H=H, W=W, nO=64, nC=64)
    x = _dev(F, rng.randn(64, H, W).astype(np.float32))
    ya, yb = [_fwd_gathered(F, d, x, _dev(F, w), _dev(F, b), None, _dest(F, nan(64, H, W)), _itab(F, t), None) for t in tabs]
    _same_bits(ya[others], yb[others], "forward")
    assert not _bits(ya[i]).any() and not _bits(yb[j]).any() and _bits(ya[j]).any() and _bits(yb[i]).any()
    assert not _bits(ya[nk:]).any()
    # input gradient, channels gathered, through the activation backward
    L = KP.launch("dgrad1", C_, nk, 64, (H, W))
    w, _ = KP.weights(rng, L["full"], kept, "c", "kept")
    d = dict(L=L, H=H, W=W, nO=64, nC=64)
    g = _dev(F, rng.randn(64, H, W).astype(np.float32))
    px, psl = _dev(F, rng.randn(64, H, W).astype(np.float32)), _dev(F, [SLOPE])
    res = []
    for t in tabs:
        gsl = _dev(F, [np.float32(3.0)])
        res.append(_dgrad_gathered(F, d, g, _dev(F, w), _dest(F, nan(64, H, W)), 0, None, _itab(F, t), (px, psl, gsl)))
    _same_bits(res[0][others], res[1][others], "input gradient")
    assert not _bits(res[0][i]).any() and not _bits(res[1][j]).any() and _bits(res[0][j]).any() and _bits(res[1][i]).any()
    # weight gradient, filters mapped
    q = _wgrad_inputs(dict(name="c128_k63", role="wgrad0", post=False))
    dx, dg = _dev(F, q["x"]), _dev(F, q["g"])
    ga, gb = [_wgrad_mapped(F, q, dx, dg, None, q["gw0"], q["gb0"], _itab(F, t), None) for t in tabs]
    rows = np.ones(C_, bool)
    rows[[kept[i], kept[j]]] = False
    _same_bits(ga[0][rows], gb[0][rows], "weight gradient")
    _same_bits(ga[0][kept[i]], q["gw0"][kept[i]], "weight gradient, the row made padding")
    _same_bits(gb[0][kept[j]], q["gw0"][kept[j]], "weight gradient, the row made padding")
    assert ga[1][kept[i]] == q["gb0"][kept[i]] and gb[1][kept[j]] == q["gb0"][kept[j]]
    assert (ga[0][kept[j]] != q["gw0"][kept[j]]).mean() > 0.99 and (gb[0][kept[i]] != q["gw0"][kept[i]]).mean() > 0.99


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _launches(F, fn):
    nk = len(F._lib.KC_NAMES)
    la = (C.c_longlong * nk)(); ms = (C.c_double * nk)(); fl = (C.c_double * nk)(); by = (C.c_double * nk)()
    F._lib.call("frcnn_prof_enable", (1 << nk) - 1)
    try:
        fn()
    finally:
        F._lib.call("frcnn_prof_enable", 0)
        F._lib.call("frcnn_prof_collect", la, ms, fl, by)
    return sum(la)


def test_refused_calls_launch_nothing_and_store_nothing(F, options):
    options("split_bf16", 1)
    options("x3_f16", 1)
    lib = F._lib.load()
    H, W, SENT = 6, 8, np.float32(-77.25)
    x = _dev(F, np.ones((128, H, W), np.float32))
    w = _dev(F, np.ones((128, 128, 3, 3), np.float32))
    b = _dev(F, np.ones(128, np.float32))
    out = _dev(F, np.full((128, H, W), SENT, np.float32))
    gw = _dev(F, np.full((128, 128, 3, 3), SENT, np.float32))
    gb = _dev(F, np.full(128, SENT, np.float32))
    gsl = _dev(F, [SENT])
    rec = _dev(F, np.full(lib.frcnn_amax_record_floats(), SENT, np.float32))
    good = KP.table(128, list(range(40)))
    t_ok, t_big, t_far = _itab(F, good), _itab(F, np.where(good == 3, 128, good)), _itab(F, np.where(good == 7, 1 << 20, good))
    p, s = F.ptr, F.stream_ptr()

    def fwd(in_=x, weight=w, out_=out, oidx=t_ok, nO=64, cidx=None, nC=64, O_full=128, C_full=128, H_=H, rec_out=None):
        return lib.frcnn_conv2d_forward_gathered(p(in_), H_, W, None, None, p(weight), p(b), O_full, C_full, p(oidx), nO, p(cidx), nC,
                                                 PAD, p(out_), None, p(rec_out), s)

    def dgr(gout=x, weight=w, gin=out, oidx=None, nO=64, cidx=t_ok, nC=64, acc=0, px=None, psl=None, gs=None, pad=PAD):
        return lib.frcnn_conv2d_backward_input_gathered(p(gout), H, W, p(weight), 128, 128, p(oidx), nO, p(cidx), nC, pad, p(gin), acc,
                                                        None, None, p(px), p(psl), None, p(gs), s)

    def wgr(in_=x, gout=x, gweight=gw, Cin=64, O=64, omap=t_ok, cmap=None, O_full=128, Cfull=128):
        return lib.frcnn_conv2d_backward_weight_mapped(p(in_), Cin, H, W, None, None, p(gout), O, PAD, p(gweight), p(gb), O_full, Cfull,
                                                       p(omap), p(cmap), s)
    bad = [
        lambda: fwd(in_=None), lambda: fwd(weight=None), lambda: fwd(out_=None),
        lambda: fwd(nC=24), lambda: fwd(nC=0), lambda: fwd(nO=32), lambda: fwd(nO=0), lambda: fwd(H_=0),
        lambda: fwd(oidx=t_big), lambda: fwd(oidx=t_far), lambda: fwd(cidx=t_big), lambda: fwd(O_full=39),
        lambda: fwd(oidx=None, nO=128, O_full=64), lambda: fwd(cidx=None, nC=128, C_full=64), lambda: fwd(O_full=0),
        lambda: dgr(gout=None), lambda: dgr(gin=None), lambda: dgr(nO=24), lambda: dgr(nC=32), lambda: dgr(cidx=t_big),
        lambda: dgr(oidx=t_far), lambda: dgr(pad=3), lambda: dgr(psl=b), lambda: dgr(gs=gsl), lambda: dgr(px=x, psl=None),
        lambda: dgr(px=x, psl=b, acc=1),
        lambda: wgr(in_=None), lambda: wgr(gout=None), lambda: wgr(gweight=None), lambda: wgr(Cin=32), lambda: wgr(O=96),
        lambda: wgr(omap=t_big), lambda: wgr(cmap=t_far), lambda: wgr(omap=None, cmap=None, Cfull=128), lambda: wgr(Cfull=0),
        lambda: wgr(omap=None, cmap=t_ok, O=128, O_full=64), lambda: wgr(O_full=39),
    ]

    def run(calls):
        for k, f in enumerate(calls):
            assert f() != 0, "refusal %d was accepted" % k
            assert lib.frcnn_last_error()
    assert _launches(F, lambda: run(bad)) == 0, "a refused call launched something"
    # without the split form no gathered launch exists; records belong to the fp16 form
    options("split_bf16", 0)
    assert _launches(F, lambda: run([fwd, dgr, wgr])) == 0
    options("split_bf16", 1)
    options("x3_f16", 0)
    assert _launches(F, lambda: run([lambda: fwd(rec_out=rec)])) == 0
    for t in (out, gw, gb, gsl, rec):
        assert (t.numpy() == SENT).all(), "a refused call stored something"
    # the same calls with nothing wrong go through (the refusals above are not refusals of the fixture itself)
    options("x3_f16", 1)
    assert _launches(F, lambda: [F._lib.check(f()) for f in (fwd, dgr, wgr)]) > 0
    assert not (out.numpy()[:64] == SENT).any() and (out.numpy()[64:] == SENT).all()
    assert (gw.numpy()[40:] == SENT).all() and not (gw.numpy()[:40, :64] == SENT).any()
    assert (gw.numpy()[:, 64:] == SENT).all() and (gb.numpy()[40:] == SENT).all() and not (gb.numpy()[:40] == SENT).any()


# ---- the producer-consumer contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORMS[f] for f in sorted(FORMS)])
def test_one_block_in_the_models_order_on_the_devices_own_tensors(F, options, form):
    """C = 128, nk = 65 (nkM = 128, nkK = 80), cin = 64, nb = C, a 12 x 16 map: forward of (b, 0) and (b, 1), then weight gradient
    and input gradient of (b, 1), weight gradient and input gradient of (b, 0), each reading what the launch before it stored.
    Only the structural facts the op tests assume of each other: the padding rows nk .. nkM - 1 of the compact output and of the
    compact gradient are exact zeros, the dropped rows of both full weight gradients and of the bias gradient are their initial
    values.  Numbers are compared in the op tests, where every input is given."""
    options("split_bf16", 1)
    options("x3_f16", form)
    C_, nk, cin, H, W = 128, 65, KP.CIN, 12, 16
    nkM, nkK = KP.sizes(C_, nk)
    assert (nkM, nkK) == (128, 80)
    rng = KP.rng_of("contract")
    kept = KP.kept_set(C_, nk, "ends")
    dropped = sorted(set(range(C_)) - set(kept))
    idx = _itab(F, KP.table(C_, kept))
    w0, b0 = KP.weights(rng, (C_, cin), kept, "o")
    w1, b1 = KP.weights(rng, (C_, C_), kept, "c")
    dw0, db0, dw1, db1 = _dev(F, w0), _dev(F, b0), _dev(F, w1), _dev(F, b1)
    x0 = _dev(F, rng.randn(cin, H, W).astype(np.float32))
    g1 = _dev(F, rng.randn(C_, H, W).astype(np.float32))
    dsl = _dev(F, [SLOPE])
    nan = lambda *s: np.full(s, np.nan, np.float32)   # noqa: E731
    L0, L1 = KP.launch("fwd0", C_, nk, C_, (H, W)), KP.launch("fwd1", C_, nk, C_, (H, W))
    # forward
    y0 = _dest(F, nan(nkM, H, W))
    a = _fwd_gathered(F, dict(L=L0, H=H, W=W, nO=nkM, nC=cin), x0, dw0, db0, None, y0, idx, None)
    assert np.isfinite(a).all() and not _bits(a[nk:]).any() and (np.abs(a[:nk]).max(axis=(1, 2)) > 0).all()
    y1 = _dest(F, nan(C_, H, W))
    c = _fwd_gathered(F, dict(L=L1, H=H, W=W, nO=C_, nC=nkK), y0.t, dw1, db1, dsl, y1, None, idx)
    assert np.isfinite(c).all()
    # (b, 1): weight gradient for the kept input channels, then the input gradient through (b, 0)'s PReLU, stored compact
    sent1, sentb = _sentinels((C_, C_, 3, 3)), -2 * _sentinels((C_,))
    q1 = dict(Cin=nkM, H=H, W=W, O=C_, O_full=C_, C_full=C_)
    gw1, gb1 = _wgrad_mapped(F, q1, y0.t, g1, dsl, sent1, sentb, None, idx)
    _same_bits(gw1[:, dropped], sent1[:, dropped], "dropped channels of the second convolution's weight gradient")
    assert np.isfinite(gw1).all() and (gw1[:, kept] != sent1[:, kept]).mean() > 0.99 and (gb1 != sentb).all()
    g0 = _dest(F, nan(nkM, H, W))
    gsl = _dev(F, [np.float32(0.0)])
    e = _dgrad_gathered(F, dict(L=L1, H=H, W=W, nO=C_, nC=nkM), g1, dw1, g0, 0, None, idx, (y0.t, dsl, gsl))
    assert np.isfinite(e).all() and not _bits(e[nk:]).any() and (np.abs(e[:nk]).max(axis=(1, 2)) > 0).all()
    assert np.isfinite(gsl.numpy()).all()
    # (b, 0): weight gradient for the kept filters, then the input gradient from the nkK rows of the compact gradient, accumulating
    sent0 = -_sentinels((C_, cin, 3, 3))
    q0 = dict(Cin=cin, H=H, W=W, O=nkM, O_full=C_, C_full=cin)
    gw0, gb0 = _wgrad_mapped(F, q0, x0, g0.t, None, sent0, sentb, idx, None)
    _same_bits(gw0[dropped], sent0[dropped], "dropped filters of the first convolution's weight gradient")
    _same_bits(gb0[dropped], sentb[dropped], "dropped filters of the first convolution's bias gradient")
    assert np.isfinite(gw0).all() and (gw0[kept] != sent0[kept]).mean() > 0.99 and (gb0[kept] != sentb[kept]).all()
    start = rng.randn(cin, H, W).astype(np.float32)
    gx = _dgrad_gathered(F, dict(L=L0, H=H, W=W, nO=nkK, nC=cin), g0.t, dw0, _dest(F, start), 1, idx, None)
    assert np.isfinite(gx).all() and (gx != start).mean() > 0.99
    y0.read(); g0.read()      # the consumers only read


def test_zz_error_ratio_over_the_file(F):
    """Runs last (file order): the worst ratios per role and form; over the file's gate ratios the split forms' RMS error is, on the
    geometric mean, no larger than the fp32 matrix-core kernel's (MEAN_GATE of tests/test_gpu_convx.py)"""
    for key in sorted(WORST):
        print("largest error / bound, %s %s: %.4f (%s)" % (key + WORST[key]))
    for key in sorted(GATE_WORST):
        print("largest rms ratio split / fp32 kernel, %s %s: %.3f (%s)" % (key + GATE_WORST[key]))
    if len(RATIOS) >= 20:     # (a filtered session has too few comparisons for a mean to say anything)
        gm = float(np.exp(np.mean(np.log(np.maximum(RATIOS, 1e-12)))))
        print("split / fp32 kernel RMS error over %d comparisons: geometric mean %.3f, min %.3f, max %.3f" % (
            len(RATIOS), gm, min(RATIOS), max(RATIOS)))
        assert gm <= MEAN_GATE, (gm, len(RATIOS))
