"""The three kernels of the per-class box head (csrc/box_head.hip) through frcnn_box_head_forward / frcnn_box_head_backward,
against the float64 restatement of tests/box_head_ref.py: every class source and class pattern, shapes from one row and one
feature to 2100 rows, 1025 features and 200 classes, arrays at 4-byte-misaligned offsets inside their allocations (the scalar
paths), integer-valued data (exact: the indexing), random data (bounds derived from the operation counts), sentinel-filled
buffers (nothing is written behind an output; the gradient rows of a class without a row stay byte for byte), and
bit-reproducibility in and out of deterministic mode."""
import ctypes as C

import numpy as np
import pytest

import box_head_ref as B

pytestmark = pytest.mark.gpu

SENT = np.uint32(0x7FA5A5A5)    # a signalling NaN: any arithmetic on it changes its bits
GUARD = 8                       # sentinel words behind (and `off` words in front of) every array


class Placed(object):
    """a host array of 4-byte elements inside a sentinel-filled device allocation, `off` elements from its 256-byte aligned start"""

    def __init__(self, F, a, off):
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize == 4
        self.shape, self.dtype, self.n, self.off = a.shape, a.dtype, a.size, off
        host = np.full(off + a.size + GUARD, SENT, np.uint32)
        host[off:off + a.size] = a.view(np.uint32).ravel()
        self.buf = F.DeviceTensor.from_numpy(host)
        self.ptr = C.c_void_p(self.buf.ptr + 4 * off)

    def read(self):
        """-> (the array, the raw words); the words around it must still be the sentinel"""
        h = self.buf.numpy()
        assert (h[:self.off] == SENT).all() and (h[self.off + self.n:] == SENT).all(), "written outside the array"
        raw = h[self.off:self.off + self.n].copy()
        return raw.view(self.dtype).reshape(self.shape), raw


def sentinel(shape, dtype=np.float32):
    return np.full(shape, SENT, np.uint32).view(dtype)


# ---- class patterns: -> (kind, classes, n_fg, lsm) ---------------------------------------------------------------------------------
def pattern(name, R, C, rng):
    ncls = C + 1
    if name == "one_class":
        return "int", np.full(R, min(2, C), np.int32), R, None
    if name == "all_background":
        return "float", np.full(R, C + 1, np.float32), 0, None
    if name == "last_class_only":
        t = np.full(R, C + 1, np.float32)
        t[::3] = C
        return "float", t, 0, None
    if name == "alternating":
        return "float", (1 + np.arange(R) % C).astype(np.float32), 0, None
    if name == "nfg0":
        return "int", rng.randint(1, C + 1, R).astype(np.int32), 0, None
    if name == "nfgR":
        return "int", rng.randint(1, C + 1, R).astype(np.int32), R, None
    if name == "nfg_half":
        return "int", rng.randint(1, C + 1, R).astype(np.int32), R // 2, None
    if name == "garbage_int":
        t = rng.randint(1, C + 1, R).astype(np.int32)
        bad = np.array([0, C + 1, -3, 10 ** 9], np.int32)
        idx = rng.rand(R) < 0.4
        t[idx] = bad[rng.randint(0, 4, int(idx.sum()))]
        return "int", t, R, None
    if name == "garbage_float":
        t = rng.randint(1, C + 1, R).astype(np.float32)
        bad = np.array([0, C + 1, -3, 1e9, np.nan, 0.5, C + 0.5, -np.inf, np.inf], np.float32)
        idx = rng.rand(R) < 0.5
        t[idx] = bad[rng.randint(0, len(bad), int(idx.sum()))]
        return "float", t, 0, None
    if name == "argmax":
        return "argmax", None, 0, np.log(rng.dirichlet(np.ones(ncls), R)).astype(np.float32)
    if name == "argmax_ties":   # few distinct values: ties everywhere; the background as the maximum; NaN in column 0 and elsewhere
        lsm = rng.randint(-3, 0, (R, ncls)).astype(np.float32)
        lsm[1::4, C] = 0.0
        lsm[2::5, 0] = np.nan
        lsm[3::7, rng.randint(0, ncls)] = np.nan
        lsm[4::9, :] = -np.inf
        return "argmax", None, 0, lsm
    raise ValueError(name)


# ---- data --------------------------------------------------------------------------------------------------------------------------
def data(mode, R, nf, C, rng, sel):
    """mode "int": small integers, every sum exact in fp32 in any order (|.| <= 2: 4 * 1025 and 4 * 2100 are far below 2^24);
    "random": normal rows, uniform weights.  gW0 / gb0: a non-zero prior gradient on the rows of the classes with a row, the
    sentinel on the others."""
    if mode == "int":
        draw = lambda *s: rng.randint(-2, 3, s).astype(np.float32)
    else:
        draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    x, W, b, g = draw(R, nf), draw(4 * C, nf), draw(4 * C), draw(R, 4)
    if mode == "random":
        W *= np.float32(0.1)
    touched = np.repeat(np.bincount(sel, minlength=C + 1)[1:] > 0, 4)
    gW0, gb0 = draw(4 * C, nf) + np.float32(3), draw(4 * C) + np.float32(3)
    gW0.view(np.uint32)[~touched] = SENT
    gb0.view(np.uint32)[~touched] = SENT
    return x, W, b, g, gW0, gb0, touched


KIND = {"argmax": 0, "int": 1, "float": 2}


def device(F, x, W, b, kind, classes, n_fg, lsm, g, gW0, gb0, offs):
    """the two entry points on placed arrays -> dict(out, sel, gfeat, gW, gb) and their raw words"""
    R, nf = x.shape
    Cn = W.shape[0] // 4
    ox, oW, oo, of, og = offs
    px, pW, pb = Placed(F, x, ox), Placed(F, W, oW), Placed(F, b, 0)
    pcls = Placed(F, classes, 0) if classes is not None else None
    plsm = Placed(F, lsm, 0) if lsm is not None else None
    out, sel = Placed(F, sentinel((R, 4)), oo), Placed(F, sentinel((R,), np.int32), 0)
    s = F.stream_ptr()
    F._lib.call("frcnn_box_head_forward", px.ptr, R, nf, pW.ptr, pb.ptr, Cn, pcls.ptr if pcls else None, KIND[kind], n_fg,
                plsm.ptr if plsm else None, lsm.shape[1] if lsm is not None else 0, out.ptr, sel.ptr, s)
    pg, gfeat, gW, gb = Placed(F, g, 0), Placed(F, sentinel((R, nf)), of), Placed(F, gW0, og), Placed(F, gb0, 0)
    F._lib.call("frcnn_box_head_backward", pg.ptr, px.ptr, sel.ptr, R, nf, pW.ptr, Cn, gfeat.ptr, gW.ptr, gb.ptr, s)
    res = {}
    for k, p in (("out", out), ("sel", sel), ("gfeat", gfeat), ("gW", gW), ("gb", gb)):
        res[k], res[k + "_raw"] = p.read()
    for p, a in ((px, x), (pW, W), (pb, b), (pg, g)):      # the inputs are only read
        assert p.read()[1].tobytes() == np.ascontiguousarray(a).tobytes()
    return res


# (R, nf, C, pattern, offsets of x, W, out, gfeat, gW in floats): every R, nf and C of the issue appears; the extremes pair up;
# nf % 4 == 0 runs aligned (16-byte moves) AND misaligned (the scalar path); every pattern appears
A, M = (0, 0, 0, 0, 0), (1, 3, 1, 2, 3)
CASES = [
    (1, 1, 1, "one_class", A),
    (1, 1025, 200, "argmax", M),
    (4, 7, 2, "alternating", A),
    (5, 64, 16, "garbage_float", A),
    (5, 64, 16, "garbage_int", M),
    (63, 100, 200, "last_class_only", M),
    (64, 512, 16, "argmax_ties", A),
    (64, 512, 2, "nfg_half", (1, 0, 0, 0, 0)),      # only x misaligned
    (65, 1025, 2, "nfgR", A),
    (65, 100, 1, "all_background", A),
    (65, 512, 16, "nfg0", (0, 0, 3, 1, 0)),          # W and x aligned, the outputs not
    (300, 512, 200, "garbage_float", A),
    (300, 100, 16, "argmax_ties", (0, 2, 0, 0, 1)),
    (2100, 1025, 200, "alternating", A),
    (2100, 1, 1, "one_class", M),
    (2100, 512, 16, "one_class", A),                 # 2100 rows of one class: every wave of the weight gradient, three pieces
    (2100, 64, 2, "argmax", M),
]
IDS = ["R%d-nf%d-C%d-%s-%s" % (c[0], c[1], c[2], c[3], "aligned" if c[4] == A else "off" + "".join(map(str, c[4]))) for c in CASES]


def test_the_cases_cover_the_issue():
    assert {c[0] for c in CASES} == {1, 4, 5, 63, 64, 65, 300, 2100}
    assert {c[1] for c in CASES} == {1, 7, 64, 100, 512, 1025}
    assert {c[2] for c in CASES} == {1, 2, 16, 200}
    assert {c[3] for c in CASES} >= {"one_class", "all_background", "last_class_only", "alternating", "nfg0", "nfgR", "garbage_int",
                                    "garbage_float", "argmax_ties"}


def check(F, case, mode):
    R, nf, Cn, pat, offs = case
    rng = np.random.RandomState(1000 * R + nf + Cn)
    kind, classes, n_fg, lsm = pattern(pat, R, Cn, rng)
    sel = B.select(R, Cn, kind, classes, n_fg, lsm)
    x, W, b, g, gW0, gb0, touched = data(mode, R, nf, Cn, rng, sel)
    got = device(F, x, W, b, kind, classes, n_fg, lsm, g, gW0, gb0, offs)
    assert np.array_equal(got["sel"], sel), "sel differs in %d rows" % int((got["sel"] != sel).sum())
    out, omag = B.forward(x, W, b, sel)
    gfeat, fmag = B.input_gradient(g, W, sel)
    prior_W, prior_b = np.where(touched[:, None], gW0, 0), np.where(touched, gb0, 0)
    wg = B.weight_gradient(g, x, sel, Cn, prior_W, prior_b)
    assert np.array_equal(wg["touched"], touched[::4])
    # rows without a class: exact zeros, whatever g holds; classes without a row: the sentinel, byte for byte
    assert not got["out"][sel == 0].any() and not got["gfeat"][sel == 0].any()
    assert got["out_raw"].reshape(R, 4)[sel == 0].tobytes() == np.zeros((int((sel == 0).sum()), 4), np.float32).tobytes()
    assert (got["gW_raw"].reshape(4 * Cn, nf)[~touched] == SENT).all() and (got["gb_raw"][~touched] == SENT).all()
    gotW, gotb = got["gW"][touched].astype(np.float64), got["gb"][touched].astype(np.float64)
    if mode == "int":
        assert np.array_equal(got["out"].astype(np.float64), out)
        assert np.array_equal(got["gfeat"].astype(np.float64), gfeat)
        assert np.array_equal(gotW, wg["gW"][touched]) and np.array_equal(gotb, wg["gb"][touched])
        return
    nrow = np.repeat(wg["n"], 4)[touched]
    e_out = np.abs(got["out"] - out) - B.forward_bound(nf, omag)
    e_gf = np.abs(got["gfeat"] - gfeat) - B.input_gradient_bound(fmag)
    e_W = np.abs(gotW - wg["gW"][touched]) - B.weight_gradient_bound(nrow[:, None], wg["magW"][touched])
    e_b = np.abs(gotb - wg["gb"][touched]) - B.weight_gradient_bound(nrow, wg["magb"][touched])
    for name, e in (("forward", e_out), ("input gradient", e_gf), ("weight gradient", e_W), ("bias gradient", e_b)):
        print("%s: largest excess over the bound %.3g (<= 0 passes)" % (name, e.max() if e.size else 0.0))
        assert not e.size or e.max() <= 0, name
    if (sel > 0).any():
        assert got["out"][sel > 0].any() and got["gfeat"][sel > 0].any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integer_data_is_exact(F, case):
    """(a) every sum is exact in fp32 in any order: each output equals the float64 restatement -- the indexing"""
    check(F, case, "int")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_data_within_the_derived_bounds(F, case):
    """(b) forward within (nf + 2) u (|b| + sum |x w|), input gradient within 5 u sum |g w|, weight and bias gradient within
    (n_c + 2) u (|G0| + sum |g x|) on a non-zero prior gradient (box_head_ref.py derives them)"""
    check(F, case, "random")


@pytest.mark.parametrize("case", [CASES[6], CASES[11], CASES[15], CASES[16]], ids=[IDS[6], IDS[11], IDS[15], IDS[16]])
def test_two_runs_are_bit_equal_in_and_out_of_deterministic_mode(F, case):
    R, nf, Cn, pat, offs = case
    rng = np.random.RandomState(7)
    kind, classes, n_fg, lsm = pattern(pat, R, Cn, rng)
    sel = B.select(R, Cn, kind, classes, n_fg, lsm)
    x, W, b, g, gW0, gb0, touched = data("random", R, nf, Cn, rng, sel)
    runs = []
    try:
        for det in (0, 0, 1, 1):
            F._lib.call("frcnn_set_option", b"deterministic", det)
            runs.append(device(F, x, W, b, kind, classes, n_fg, lsm, g, gW0, gb0, offs))
    finally:
        F._lib.call("frcnn_set_option", b"deterministic", 0)
    for r in runs[1:]:
        for k in ("out_raw", "sel_raw", "gfeat_raw", "gW_raw", "gb_raw"):
            assert r[k].tobytes() == runs[0][k].tobytes(), k


def test_the_host_array_wrapper(F):
    """nms.box_head: the op on host arrays, the three class sources"""
    rng = np.random.RandomState(3)
    R, nf, Cn = 37, 20, 5
    x, W, b, g = (rng.randint(-2, 3, s).astype(np.float32) for s in ((R, nf), (4 * Cn, nf), (4 * Cn,), (R, 4)))
    cl = rng.randint(1, Cn + 1, R).astype(np.int32)
    lsm = np.log(rng.dirichlet(np.ones(Cn + 1), R)).astype(np.float32)
    for kw, sel in ((dict(classes=cl, n_fg=11), B.select(R, Cn, "int", cl, 11)),
                    (dict(classes=cl.astype(np.float32)), B.select(R, Cn, "float", cl.astype(np.float32))),
                    (dict(lsm=lsm), B.select(R, Cn, "argmax", lsm=lsm))):
        got = F.box_head(x, W, b, g=g, **kw)
        assert np.array_equal(got["sel"], sel)
        assert np.array_equal(got["out"], B.forward(x, W, b, sel)[0])
        assert np.array_equal(got["gfeat"], B.input_gradient(g, W, sel)[0])
        wg = B.weight_gradient(g, x, sel, Cn, np.zeros_like(W), np.zeros_like(b))
        assert np.array_equal(got["gW"], wg["gW"]) and np.array_equal(got["gb"], wg["gb"])
