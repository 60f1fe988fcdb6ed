"""The anchor-level and criterion kernels, one entry point at a time, against the float64 restatements of tests/anchor_ops_ref.py:
frcnn_rpn_scan / frcnn_rpn_scan_batch (csrc/rpn.hip: threshold test + ordered compaction), frcnn_rpn_loss, frcnn_loss_accumulate,
frcnn_cnet_losses and frcnn_cnet_decode (csrc/cnet.hip).  The problems, their input conditions (asserted without a GPU in
tests/test_anchor_ops_host.py) and the tolerances -- 0 (bit for bit) for everything that does not pass through exp or log, the
value rule of anchor_ops_ref's docstring for the rest -- come from that module.  Every output buffer carries a guard tail and
is pre-filled; what the entry point must not write is compared bit for bit with what was there.  Each test prints the largest
deviation it saw per quantity (absolute, and as a fraction of the bound where there is one)."""
import ctypes as C
import math

import numpy as np
import pytest

import anchor_ops_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = -7
GUARD = 64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Guarded(object):
    """a device buffer of body.size + guard elements: the body, then a tail that nothing may touch"""

    def __init__(self, F, body, tail=SENTINEL, guard=GUARD):
        body = np.ascontiguousarray(body)
        self.shape, self.n = body.shape, body.size
        self.host = np.concatenate([body.ravel(), np.full(guard, tail, body.dtype)])
        self.dev = F.DeviceTensor.from_numpy(self.host)
        self.ptr = C.c_void_p(self.dev.ptr)

    def read(self, what):
        got = self.dev.numpy()
        assert same_bits(got[self.n:], self.host[self.n:]), "%s: stores behind the end of the buffer" % what
        return got[:self.n].reshape(self.shape)


class Deviations(object):
    def __init__(self):
        self.worst = {}

    def check(self, name, got, want, tol):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
        assert got.shape == want.shape, name
        dev = np.abs(got - want)
        ratio = np.where(tol > 0, dev / np.where(tol > 0, tol, 1.0), 0.0)
        w = self.worst.setdefault(name, [0.0, 0.0, 0])
        if dev.size:
            w[0] = max(w[0], float(np.nanmax(dev)))
            w[1] = max(w[1], float(np.nanmax(ratio)))
            w[2] += dev.size
        bad = ~(dev <= tol)
        assert not bad.any(), "%s: %d of %d outside the bound; worst |got - want| = %.3e against %.3e (got %r, want %r)" % (
            name, int(bad.sum()), bad.size, float(dev[bad].max()), float(tol[bad][np.argmax(dev[bad])]),
            got[bad][np.argmax(dev[bad])], want[bad][np.argmax(dev[bad])])

    def report(self, title):
        for name in sorted(self.worst):
            a, r, n = self.worst[name]
            print("%s: %-12s largest |got - want| = %.3e = %.3f of its bound (%d values)" % (title, name, a, r, n))


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


# ================================================================================================ the scan
def _scan_call(F, frames, cap, batch):
    """One frcnn_rpn_scan (one frame) or frcnn_rpn_scan_batch (B frames, the frames slot_stride floats apart in one buffer, NaNs
    between the maps) -> (outputs read back, counts [B]); guard tails of the outputs, of count and of the workspace checked."""
    c0 = frames[0]
    H, W, B = c0["H"], c0["W"], len(frames)
    hoff = [0]
    for l in range(4):
        hoff.append(hoff[-1] + 18 * H[l] * W[l] + 5)
    slot = hoff[4] + 37
    heads = np.full((B, slot), np.nan, np.float32)
    for b, c in enumerate(frames):
        for l in range(4):
            heads[b, hoff[l]:hoff[l] + c["maps"][l].size] = c["maps"][l].ravel()
    dheads = F.DeviceTensor.from_numpy(heads)
    aw, ah = F.DeviceTensor.from_numpy(c0["aw"]), F.DeviceTensor.from_numpy(c0["ah"])
    # (the guard tails hold every match of a frame: a compaction that ignored the cap would be seen, not left to write elsewhere)
    rows, g = B * cap, c0["total"] + 16
    o = dict(p=Guarded(F, np.full(rows, SENTINEL, np.float32), guard=g),
             idx=Guarded(F, np.full((rows, 4), SENTINEL, np.int32), guard=4 * g),
             rect=Guarded(F, np.full((rows, 4), SENTINEL, np.float64), guard=4 * g),
             box=Guarded(F, np.full((rows, 4), SENTINEL, np.float32), guard=4 * g))
    cnt = Guarded(F, np.full(B, SENTINEL, np.int32))
    L = F._lib.load()
    Hs, Ws = _ints(H), _ints(W)
    maps = (C.c_void_p * 4)(*[dheads.ptr + 4 * hoff[l] for l in range(4)])
    if batch:
        wsb = L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B)
    else:
        assert B == 1
        wsb = L.frcnn_rpn_scan_workspace_bytes(Hs, Ws)
    ws = F.DeviceTensor.from_numpy(np.full(wsb + 256, 0xA5, np.uint8))
    if batch:
        F._lib.call("frcnn_rpn_scan_batch", maps, Hs, Ws, B, slot, F.ptr(aw), F.ptr(ah), ref.IMG_W, ref.IMG_H, ref.THR, cap,
                    o["p"].ptr, o["idx"].ptr, o["rect"].ptr, o["box"].ptr, cnt.ptr, F.ptr(ws), wsb, F.stream_ptr())
    else:
        F._lib.call("frcnn_rpn_scan", maps, Hs, Ws, F.ptr(aw), F.ptr(ah), ref.IMG_W, ref.IMG_H, ref.THR, cap, o["p"].ptr,
                    o["idx"].ptr, o["rect"].ptr, o["box"].ptr, cnt.ptr, F.ptr(ws), wsb, F.stream_ptr())
    got = {k: v.read("match_" + k) for k, v in o.items()}
    counts = cnt.read("count")
    assert np.all(ws.numpy()[wsb:] == 0xA5), "stores behind the workspace"
    assert same_bits(dheads.numpy(), heads), "the head maps were written"
    return got, counts


def _check_frame(D, got, count, b, cap, c, what):
    w = c["want"]
    n = w["count"]
    k = min(cap, n)
    assert int(count) == n, "%s: count %d, the full number of matches is %d (cap %d)" % (what, count, n, cap)
    seg = {key: v[b * cap:(b + 1) * cap] for key, v in got.items()}
    for key, v in seg.items():
        assert np.all(v[k:] == SENTINEL), "%s: rows behind the first min(cap, count) = %d of match_%s were written" % (what, k, key)
    assert same_bits(seg["idx"][:k], w["idx"][:k]), "%s: match_idx is not the first %d matches in scan order" % (what, k)
    D.check("p", seg["p"][:k], w["p"][:k], w["p_tol"][:k])
    D.check("rect", seg["rect"][:k], w["rect"][:k], w["rect_tol"][:k])
    D.check("box", seg["box"][:k], w["box"][:k], w["box_tol"][:k])


@pytest.mark.parametrize("name", sorted(ref.SCAN_SIZES))
def test_rpn_scan_against_reference(F, name):
    """frcnn_rpn_scan on every pattern of the problem, under the four caps"""
    D = Deviations()
    for pattern in ref.scan_patterns_for(name):
        c = ref.scan_case(name, pattern)
        for cap in ref.scan_caps(c["want"]["count"], c["total"]):
            got, counts = _scan_call(F, [c], cap, batch=False)
            _check_frame(D, got, counts[0], 0, cap, c, "%s/%s cap %d" % (name, pattern, cap))
    D.report("rpn_scan %s" % name)


@pytest.mark.parametrize("name", sorted(ref.SCAN_SIZES))
def test_rpn_scan_batch_against_reference(F, name):
    """frcnn_rpn_scan_batch with B = 3 and a slot stride: three patterns per call (every pattern leads one call), the caps taken
    from the middle frame's count -- frames with fewer and with more matches than the cap meet in one call"""
    D = Deviations()
    pats = ref.scan_patterns_for(name)
    for i in range(len(pats)):
        frames = [ref.scan_case(name, pats[(i + j) % len(pats)]) for j in range(3)]
        for cap in ref.scan_caps(frames[1]["want"]["count"], frames[1]["total"]):
            got, counts = _scan_call(F, frames, cap, batch=True)
            for b, c in enumerate(frames):
                _check_frame(D, got, counts[b], b, cap, c, "%s/%s frame %d cap %d" % (name, c["pattern"], b, cap))
    D.report("rpn_scan_batch %s" % name)


def test_rpn_scan_rejects_a_map_beyond_the_tables(F):
    """H = 201: the anchor tables hold 200 entries; an error code, and nothing is written"""
    H, W = [201, 2, 2, 2], [2, 3, 3, 3]
    rng = np.random.RandomState(3)
    aw, ah = ref.anchor_tables(rng)
    daw, dah = F.DeviceTensor.from_numpy(aw), F.DeviceTensor.from_numpy(ah)
    ms = []
    for h, w in zip(H, W):
        m = rng.randn(18, h, w).astype(np.float32)
        m[0::6] = 30.0
        ms.append(F.DeviceTensor.from_numpy(m))
    maps = (C.c_void_p * 4)(*[m.ptr for m in ms])
    L = F._lib.load()
    Hs, Ws = _ints(H), _ints(W)
    cap = 3 * sum(h * w for h, w in zip(H, W))
    for batch in (False, True):
        o = [Guarded(F, np.full(cap, SENTINEL, np.float32)), Guarded(F, np.full((cap, 4), SENTINEL, np.int32)),
             Guarded(F, np.full((cap, 4), SENTINEL, np.float64)), Guarded(F, np.full((cap, 4), SENTINEL, np.float32)),
             Guarded(F, np.full(1, SENTINEL, np.int32))]
        wsb = L.frcnn_rpn_scan_workspace_bytes(Hs, Ws)
        ws = F.DeviceTensor.from_numpy(np.full(wsb + 256, 0xA5, np.uint8))
        if batch:
            rc = L.frcnn_rpn_scan_batch(maps, Hs, Ws, 1, 0, F.ptr(daw), F.ptr(dah), ref.IMG_W, ref.IMG_H, ref.THR, cap, o[0].ptr, o[1].ptr,
                                        o[2].ptr, o[3].ptr, o[4].ptr, F.ptr(ws), wsb, F.stream_ptr())
        else:
            rc = L.frcnn_rpn_scan(maps, Hs, Ws, F.ptr(daw), F.ptr(dah), ref.IMG_W, ref.IMG_H, ref.THR, cap, o[0].ptr, o[1].ptr, o[2].ptr,
                                  o[3].ptr, o[4].ptr, F.ptr(ws), wsb, F.stream_ptr())
        assert rc != 0, "a 201-row head map was accepted"
        assert b"200" in L.frcnn_last_error()
        for g in o:
            assert np.all(g.read("output") == SENTINEL), "an output was written by the rejected call"
        assert np.all(ws.numpy() == 0xA5)


# ================================================================================================ the sparse RPN loss
def _option(F, name, value=None):
    if value is None:
        v = C.c_int(0)
        F._lib.call("frcnn_get_option", name.encode(), C.byref(v))
        return v.value
    F._lib.call("frcnn_set_option", name.encode(), int(value))


def _loss_call(F, c, npos=None, nneg=None, deltas0=None):
    """frcnn_rpn_loss on the problem (deltas0: other initial delta maps than the problem's) -> dict(deltas: four maps, ex_loss,
    crtarget, cctarget), guard tails checked"""
    npos = c["npos"] if npos is None else npos
    nneg = c["nneg"] if nneg is None else nneg
    E = c["npos"] + c["nneg"]
    sizes = c["sizes"]
    dm = [Guarded(F, m, tail=np.nan) for m in c["maps"]]
    dd = [Guarded(F, d, tail=123.0) for d in (c["deltas0"] if deltas0 is None else deltas0)]
    maps = (C.c_void_p * 4)(*[m.dev.ptr for m in dm])
    deltas = (C.c_void_p * 4)(*[d.dev.ptr for d in dd])
    ins = [F.DeviceTensor.from_numpy(a) for a in (c["ex_idx"].astype(np.int32), c["ex_anchor"].astype(np.float64),
                                                  c["ex_roi"].astype(np.float64), c["ex_class"].astype(np.int32))]
    out = dict(ex_loss=Guarded(F, np.full((E, 2), SENTINEL, np.float64)), crtarget=Guarded(F, np.full((E, 4), SENTINEL, np.float32)),
               cctarget=Guarded(F, np.full(E, SENTINEL, np.float32)))
    F._lib.call("frcnn_rpn_loss", maps, deltas, _ints([h for h, w in sizes]), _ints([w for h, w in sizes]), F.ptr(ins[0]),
                F.ptr(ins[1]), F.ptr(ins[2]), F.ptr(ins[3]), npos, nneg, c["bgclass"], out["ex_loss"].ptr, out["crtarget"].ptr,
                out["cctarget"].ptr, F.stream_ptr())
    got = {k: v.read(k) for k, v in out.items()}
    got["deltas"] = [d.read("delta map %d" % (l + 1)) for l, d in enumerate(dd)]
    for l in range(4):
        assert same_bits(dm[l].read("head map %d" % (l + 1)), c["maps"][l]), "head map %d was written" % (l + 1)
    return got


def _check_loss_outputs(D, c, got):
    w = c["want"]
    npos = c["npos"]
    D.check("ex_loss cls", got["ex_loss"][:, 0], w["ex_loss"][:, 0], w["ex_loss_tol"][:, 0])
    D.check("ex_loss reg", got["ex_loss"][:, 1], w["ex_loss"][:, 1], w["ex_loss_tol"][:, 1])
    assert same_bits(got["cctarget"], w["cctarget"]), "cctarget"
    assert not got["crtarget"][npos:].view(np.uint32).any(), "crtarget rows of the negatives are not +0"
    D.check("crtarget", got["crtarget"][:npos], w["crtarget"][:npos], w["crtarget_tol"][:npos])
    # the non-transcendental part, bit for bit: every value whose tolerance is 0
    for key in ("ex_loss", "crtarget"):
        exact = w[key + "_tol"] == 0
        assert same_bits(got[key][exact], w[key][exact]), "%s: an exact value differs in its bits" % key


def _check_maps_f64(D, c, got):
    """the maps against the float64 sums under the fp32 summation bound; elements no example names: bit for bit as they were;
    elements with ONE addend free of exp and log: bit for bit the fp32 sum"""
    w = c["want"]
    want, bound = ref.expected_maps(c["deltas0"], w["addends"], "f64")
    seq = ref.expected_maps(c["deltas0"], w["addends"], "f32seq")
    n_add, tol_sum = [np.zeros(d.size, np.int64) for d in c["deltas0"]], [np.zeros(d.size) for d in c["deltas0"]]
    for l, off, a, tol in w["addends"]:
        n_add[l][off] += 1
        tol_sum[l][off] += tol
    for l in range(4):
        g = got["deltas"][l]
        named = (n_add[l] > 0).reshape(g.shape)
        assert same_bits(g[~named], c["deltas0"][l][~named]), "delta map %d: an element no example names has changed" % (l + 1)
        D.check("delta maps", g[named], want[l][named], bound[l][named])
        one_exact = ((n_add[l] == 1) & (tol_sum[l] == 0)).reshape(g.shape)
        assert same_bits(g[one_exact], seq[l][one_exact]), "delta map %d: an exact gradient was not added exactly" % (l + 1)


def _check_gradients(D, c, got):
    """the problem run on delta maps of zeros, its anchors distinct: every named element IS the gradient the kernel formed (0 + g
    is g), so the class and the regression gradients are compared on their own, each under its own tolerance (0: equal)"""
    w = c["want"]
    flat = [g.ravel() for g in got["deltas"]]
    assert len({(l, off) for l, off, _, _ in w["addends"]}) == len(w["addends"]), "an anchor is named twice"
    for name, planes in (("class grad", (0, 1)), ("reg grad", (2, 3, 4, 5))):
        sel = [(l, off, a, tol) for l, off, a, tol in w["addends"] if (off // (c["sizes"][l][0] * c["sizes"][l][1])) % 6 in planes]
        if sel:
            D.check(name, [flat[l][off] for l, off, _, _ in sel], [a for _, _, a, _ in sel], [tol for _, _, _, tol in sel])
    named = [np.zeros(f.size, bool) for f in flat]
    for l, off, _, _ in w["addends"]:
        named[l][off] = True
    for l in range(4):
        assert not flat[l][~named[l]].view(np.uint32).any(), "delta map %d: an element no example names has changed" % (l + 1)


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("E,npos", ref.LOSS_CASES)
def test_rpn_loss_against_reference(F, E, npos, det):
    """distinct anchors: the corners of every layer and aspect, every logit gap, the SmoothL1 switch values.  Run on the problem's
    random delta maps (gradients are added, nothing else changes) and on maps of zeros (the gradients themselves)"""
    c = ref.loss_case(E, npos)
    D = Deviations()
    before = _option(F, "deterministic")
    _option(F, "deterministic", det)
    try:
        got = _loss_call(F, c)
        zero = _loss_call(F, c, deltas0=[np.zeros_like(d) for d in c["deltas0"]])
    finally:
        _option(F, "deterministic", before)
    title = "rpn_loss E=%d npos=%d" % (E, npos)
    _check_loss_outputs(D, c, got)
    _check_maps_f64(D, c, got)
    _check_gradients(D, c, zero)
    for key in ("ex_loss", "crtarget", "cctarget"):
        assert same_bits(zero[key], got[key]), key
    D.report(title + (" det" if det else ""))


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
def test_rpn_loss_without_examples_touches_nothing(F, det):
    c = ref.loss_case(63, 20)
    before = _option(F, "deterministic")
    _option(F, "deterministic", det)
    try:
        got = _loss_call(F, c, npos=0, nneg=0)
    finally:
        _option(F, "deterministic", before)
    for l in range(4):
        assert same_bits(got["deltas"][l], c["deltas0"][l])
    for key in ("ex_loss", "crtarget", "cctarget"):
        assert np.all(got[key] == SENTINEL), key


@pytest.mark.parametrize("k", ref.DUP_CASES)
def test_rpn_loss_duplicate_anchors(F, k):
    """anchors named k times (one of them k + 2 times), every addend free of exp and log.  Option deterministic: the maps are the
    fp32 sum in example order, bit for bit, twice.  Default: within the fp32 summation bound of the float64 sum."""
    c = ref.loss_case(ref.DUP_E, ref.DUP_NPOS, k)
    w = c["want"]
    D = Deviations()
    title = "rpn_loss dup=%d" % k
    before = _option(F, "deterministic")
    try:
        _option(F, "deterministic", 1)
        a = _loss_call(F, c)
        b = _loss_call(F, c)
        _option(F, "deterministic", 0)
        d = _loss_call(F, c)
    finally:
        _option(F, "deterministic", before)
    seq = ref.expected_maps(c["deltas0"], w["addends"], "f32seq")
    for l in range(4):
        assert same_bits(a["deltas"][l], seq[l]), "deterministic: delta map %d is not the fp32 sum in example order" % (l + 1)
        assert same_bits(a["deltas"][l], b["deltas"][l]), "deterministic: two runs differ"
    for key in ("ex_loss", "crtarget", "cctarget"):
        assert same_bits(a[key], b[key]), key
    for got in (a, d):
        _check_loss_outputs(D, c, got)
    _check_maps_f64(D, c, d)
    D.report(title)


# ================================================================================================ frcnn_loss_accumulate
@pytest.mark.parametrize("E", ref.ACC_E)
def test_loss_accumulate_against_fsum(F, E):
    """acc += the column sums: within E * 2^-53 * sum|terms| of math.fsum (acc's initial value is a term), and the same bits twice"""
    ex, acc0 = ref.accumulate_case(E)
    dex = F.DeviceTensor.from_numpy(ex if E else np.zeros((1, 2)))
    runs = []
    for _ in range(2):
        acc = Guarded(F, acc0.copy(), tail=SENTINEL)
        F._lib.call("frcnn_loss_accumulate", F.ptr(dex), E, acc.ptr, F.stream_ptr())
        runs.append(acc.read("acc"))
    assert same_bits(runs[0], runs[1]), "two runs differ"
    if E == 0:
        assert same_bits(runs[0], acc0)
        return
    assert same_bits(dex.numpy(), ex)
    D = Deviations()
    for j in range(2):
        terms = [float(acc0[j])] + [float(v) for v in ex[:, j]]
        D.check("acc", runs[0][j], math.fsum(terms), E * 2.0 ** -53 * math.fsum(abs(v) for v in terms))
    D.report("loss_accumulate E=%d" % E)


# ================================================================================================ frcnn_cnet_losses
@pytest.mark.parametrize("R", ref.CNET_R)
def test_cnet_losses_against_reference(F, R):
    """crout (zeroed in place behind the positives), both gradients and ccdelta bit for bit -- no exp, no log; each of the two
    loss terms within one fp32 ulp of the reference's rounded sum (the order of the fp64 sum in front of the rounding), the
    regression term's ulp times the 10 it is multiplied by afterwards, plus the rounding of the fp64 addition to loss2"""
    D = Deviations()
    rng = np.random.RandomState(R)
    for npos in ref.cnet_npos(R):
        for ncls in ref.CNET_NCLS:
            c = ref.cnet_losses_case(R, npos, ncls)
            w = c["want"]
            what = "R=%d npos=%d ncls=%d" % (R, npos, ncls)
            crout = Guarded(F, c["crout"])
            crdelta = Guarded(F, (rng.randn(R, 4) * 1e3).astype(np.float32))
            ccdelta = Guarded(F, (rng.randn(R, ncls) * 1e3).astype(np.float32))
            loss2 = Guarded(F, c["loss0"].copy())
            dcrt, dcco, dcct = (F.DeviceTensor.from_numpy(c[k]) for k in ("crtarget", "ccout", "cctarget"))
            F._lib.call("frcnn_cnet_losses", crout.ptr, F.ptr(dcrt), F.ptr(dcco), F.ptr(dcct), R, npos, ncls, crdelta.ptr, ccdelta.ptr,
                        loss2.ptr, F.stream_ptr())
            got = crout.read("crout")
            assert same_bits(got[:npos], c["crout"][:npos]), what + ": a positive row of crout has changed"
            assert not got[npos:].view(np.uint32).any(), what + ": a negative row of crout is not +0"
            assert same_bits(crdelta.read("crdelta"), w["crdelta"]), what + ": crdelta"
            gcc = ccdelta.read("ccdelta")
            hit = w["ccdelta"] != 0
            assert hit.sum() == R and not gcc[~hit].view(np.uint32).any(), what + ": ccdelta is not +0 off the targets"
            assert same_bits(gcc, w["ccdelta"]), what + ": ccdelta"
            for k in ("crtarget", "ccout", "cctarget"):
                assert same_bits({"crtarget": dcrt, "ccout": dcco, "cctarget": dcct}[k].numpy(), c[k]), k
            gl = loss2.read("loss2")
            reg, cls = ref.f32(w["reg_sum"]), ref.f32(w["cls_mean"])
            for j, (term, ulp) in enumerate(((reg * 10.0, 10.0 * float(ref.ulp32(reg))), (cls, float(ref.ulp32(cls))))):
                want = c["loss0"][j] + term
                D.check("loss2[%d]" % j, gl[j], want, (ulp if term != 0.0 else 0.0) + 2.0 ** -52 * abs(want))
    D.report("cnet_losses R=%d" % R)


# ================================================================================================ frcnn_cnet_decode
@pytest.mark.parametrize("R", ref.DECODE_R)
def test_cnet_decode_against_reference(F, R):
    """the first maximum of every row and its value, bit for bit"""
    for ncls in ref.DECODE_NCLS:
        for kind in ref.DECODE_KINDS:
            x = ref.decode_case(R, ncls, kind)
            wc, wf = ref.decode_ref(x)
            dx = F.DeviceTensor.from_numpy(x)
            cls, conf = Guarded(F, np.full(R, SENTINEL, np.int32)), Guarded(F, np.full(R, SENTINEL, np.float32))
            F._lib.call("frcnn_cnet_decode", F.ptr(dx), R, ncls, cls.ptr, conf.ptr, F.stream_ptr())
            what = "R=%d ncls=%d %s" % (R, ncls, kind)
            assert same_bits(cls.read("cls"), wc), what + ": class"
            assert same_bits(conf.read("conf"), wf), what + ": confidence"
            assert same_bits(dx.numpy(), x)
