"""Magnitude records of the two-plane fp16 form (csrc/amax.h, option "x3_f16"), checked at their producers.

Every eligible convolution scales its operands by a power of two taken from a record: one max|x| per block of the launch that
wrote the tensor.  The consumers hide a wrong record (a spare binade, 1e-4 bars further up), so each producer is checked here on
its own: the record is poisoned, the launch runs, and the largest entry must EQUAL np.abs(stored).max() of the tensor read back
from the device -- float32 `==`, no tolerance (fmaxf over stored values is exact).  Inputs are randn plus one planted value of 64x
the largest magnitude, moved over the places where a mask, a tail or a chunk boundary decides whether a thread sees it; for the
pooling and activation kernels a numpy restatement first proves that the planted value is the unique maximum of the output, and
where it sits is then read from the output itself.  The model-level tests read the records the nets keep through
frcnn_model_debug_buffer and derive WHICH records must exist from the layer table."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANT = 64.0
MAX_BLOCKS = 16384


# ------------------------------------------------------------------------------------------------ helpers
def _dev(F, a, dtype=np.float32):
    return F.DeviceTensor.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def _option(F, name, value=None):
    if value is None:
        v = C.c_int(0)
        F._lib.call("frcnn_get_option", name.encode(), C.byref(v))
        return v.value
    F._lib.call("frcnn_set_option", name.encode(), int(value))


def _rec_floats(F):
    n = F._lib.load().frcnn_amax_record_floats()
    assert n >= MAX_BLOCKS + 1
    return n


def _poison_host(F):
    p = np.full(_rec_floats(F), 1e30, np.float32)
    p[:1] = np.array([MAX_BLOCKS], np.int32).view(np.float32)
    return p


_POISON = {}


def _poison(F, rec):
    """Fill a device record with 1e30 and the count word with 16384: an entry or a count the launch leaves unwritten shows."""
    if "t" not in _POISON:
        _POISON["t"] = _dev(F, _poison_host(F))
    rec.copy_(_POISON["t"])
    return rec


def _new_rec(F):
    return _poison(F, F.DeviceTensor.empty((_rec_floats(F),)))


def rec_max(rec):
    rec = np.asarray(rec, np.float32)
    n = int(rec[:1].view(np.int32)[0])
    assert 1 <= n <= MAX_BLOCKS, "count word %d" % n
    e = rec[1:1 + n]
    assert np.isfinite(e).all() and (e >= 0).all(), "entries %r" % e[~(np.isfinite(e) & (e >= 0))][:8]
    return e.max()


def _same(rec, stored, what=""):
    got, want = rec_max(rec.numpy()), np.abs(stored).max()
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert got == want, "%s: record %r, tensor %r" % (what, got, want)


def _unique_max_at(ref, pos, what=""):
    m = np.abs(ref)
    assert m[pos] == m.max() and int((m == m.max()).sum()) == 1, "%s: the planted value is not the unique maximum" % (what,)


def _argmax(stored):
    return tuple(int(i) for i in np.unravel_index(np.abs(stored).argmax(), stored.shape))


@pytest.fixture
def f16_on(F):
    before = _option(F, "x3_f16")
    _option(F, "x3_f16", 1)
    yield
    _option(F, "x3_f16", before)


@pytest.fixture(params=[0, 1], ids=["atomics", "deterministic"])
def det_mode(F, request):
    before = _option(F, "deterministic")
    _option(F, "deterministic", request.param)
    yield request.param
    _option(F, "deterministic", before)


# ------------------------------------------------------------------------------------------------ tensor_absmax
THREADS = 1024 * 256   # threads of the largest launch: one 16-byte group each per grid stride


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, 4200003])
def test_tensor_absmax(F, n):
    rng = np.random.RandomState(n % 1000)
    x = rng.randn(n).astype(np.float32)
    big = np.float32(PLANT * np.abs(x).max())
    buf = F.DeviceTensor.empty((n + 8,))
    assert buf.ptr % 16 == 0
    rec = F.DeviceTensor.empty((_rec_floats(F),))
    one = np.empty(1, np.float32)
    launches = 0
    for off in range(4):
        t = buf.offset_view(off, (n,))
        t.copy_from_numpy(x)

        def run(want, what):
            _poison(F, rec)
            F._lib.call("frcnn_tensor_absmax", F.ptr(t), n, F.ptr(rec), F.stream_ptr())
            got = rec_max(rec.numpy())
            assert got == want, "n %d, offset %d, %s: record %r, tensor %r" % (n, off, what, got, want)

        run(np.abs(x).max(), "randn")
        head = min((4 - off) % 4, n)
        n4 = (n - head) // 4
        tail = head + 4 * n4
        spots = {0: "first", n - 1: "last"}
        if head:
            spots[head - 1] = "last head element"
        if n4:
            spots[head] = "first body element"
            spots[tail - 1] = "last body element"
        if tail < n:
            spots[tail] = "first tail element"
        for k in range(1, 5):   # the four loads in flight of the unrolled loop, and the first group behind it
            if n4 > k * THREADS:
                spots[head + 4 * k * THREADS + 1] = "group %d strides on" % k
        for j, (i, what) in enumerate(sorted(spots.items())):
            one[0] = big if (j + off) % 2 else -big   # (a negative value as the maximum, every other launch)
            t.offset_view(i, (1,)).copy_from_numpy(one)
            run(big, "planted at %d (%s)" % (i, what))
            t.offset_view(i, (1,)).copy_from_numpy(x[i:i + 1])
            launches += 1
    assert launches >= 4 * (1 if n == 1 else 2)


def test_tensor_absmax_of_zeros_and_of_negative_values(F):
    rec = F.DeviceTensor.empty((_rec_floats(F),))
    for n in (5, 4097):
        for x in (np.zeros(n, np.float32), -np.arange(1, n + 1, dtype=np.float32), np.full(n, -0.0, np.float32)):
            t = _dev(F, x)
            _poison(F, rec)
            F._lib.call("frcnn_tensor_absmax", F.ptr(t), n, F.ptr(rec), F.stream_ptr())
            got = rec_max(rec.numpy())
            assert got == np.abs(x).max() and not np.signbit(got)


# ------------------------------------------------------------------------------------------------ pooling forward
def _act(x, slope, scale):
    v = x
    if slope is not None:
        v = np.where(v > 0, v, np.float32(slope) * v).astype(np.float32)
    if scale is not None:
        v = (v * scale[:, None, None]).astype(np.float32)
    return v


def pool_ref(x, slope, scale):
    """2x2 stride-2 ceil-mode max pool of act(x): (best, code dy*2+dx of the first maximum)."""
    C_, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    v = np.full((C_, 2 * Ho, 2 * Wo), -np.inf, np.float32)
    v[:, :H, :W] = _act(x, slope, scale)
    win = v.reshape(C_, Ho, 2, Wo, 2).transpose(0, 1, 3, 2, 4).reshape(C_, Ho, Wo, 4)
    return win.max(-1), win.argmax(-1).astype(np.uint8)


def _scale_vec(kind, C_, rng):
    if kind is None:
        return None
    if kind == "half":
        return np.full(C_, 0.5, np.float32)
    s = (rng.rand(C_) > 0.4).astype(np.float32)
    s[0] = 1.0
    s[C_ - 1] = 1.0
    s[C_ // 2] = 0.0
    return s


POOL_SHAPES = [(5, 9, 13), (4, 2, 2), (2, 3, 2), (8, 57, 100)]


def _pool_case(F, x, slope, scale, plants, what):
    C_, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ds = _dev(F, [slope]) if slope is not None else None
    dsc = _dev(F, scale) if scale is not None else None
    out, idx = F.DeviceTensor.empty((C_, Ho, Wo)), F.DeviceTensor.empty((C_, Ho, Wo), np.uint8)
    rec = F.DeviceTensor.empty((_rec_floats(F),))
    dx = F.DeviceTensor.empty(x.shape)
    for name, edit, want_pos in plants:
        xp = x.copy()
        edit(xp)
        if want_pos is not None:
            _unique_max_at(pool_ref(xp, slope, scale)[0], want_pos, what + name)
        dx.copy_from_numpy(xp)
        _poison(F, rec)
        F._lib.call("frcnn_maxpool_act_forward_rec", F.ptr(dx), C_, H, W, F.ptr(ds), F.ptr(dsc), F.ptr(out), F.ptr(idx), F.stream_ptr(),
                    F.ptr(rec))
        stored = out.numpy()
        if want_pos is not None:
            assert _argmax(stored) == want_pos, (what, name)
        _same(rec, stored, what + name)


def _pool_plants(x, scale):
    C_, H, W = x.shape
    big = np.float32(PLANT * np.abs(x).max())
    live = [c for c in range(C_) if scale is None or scale[c] != 0]
    c0, c1 = live[0], live[-1]
    dead = [c for c in range(C_) if scale is not None and scale[c] == 0]

    def put(c, y, xx, v):
        def edit(a):
            a[c, y, xx] = v
        return edit

    def negative_window(c, oy, ox):   # every member of the window large and negative: the stored value is the LEAST negative one
        def edit(a):
            ys, xs = slice(2 * oy, min(2 * oy + 2, H)), slice(2 * ox, min(2 * ox + 2, W))
            n = a[c, ys, xs].size
            a[c, ys, xs] = (-big * (1 + 0.125 * np.arange(n, dtype=np.float32))).reshape(a[c, ys, xs].shape)
        return edit
    plants = [("randn", lambda a: None, None),
              ("first pixel", put(c0, 0, 0, big), (c0, 0, 0)),
              ("last row, last column", put(c1, H - 1, W - 1, big), (c1, (H - 1) // 2, (W - 1) // 2)),
              ("last row", put(c0, H - 1, 0, big), (c0, (H - 1) // 2, 0)),
              ("last column", put(c1, 0, W - 1, big), (c1, 0, (W - 1) // 2)),
              ("negative window, last cell", negative_window(c1, (H - 1) // 2, (W - 1) // 2), (c1, (H - 1) // 2, (W - 1) // 2)),
              ("negative window, first cell", negative_window(c0, 0, 0), (c0, 0, 0))]
    if dead:   # a value the dropout scale multiplies by zero is stored as zero: it must not reach the record
        plants.append(("dropped channel", put(dead[0], H - 1, W - 1, big), None))
    return plants


@pytest.mark.parametrize("scale_kind", [None, "keep", "half"])
@pytest.mark.parametrize("slope", [None, 0.25, 1.5])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_act_forward_record(F, shape, slope, scale_kind):
    rng = np.random.RandomState(shape[1] * 7 + shape[2])
    x = rng.randn(*shape).astype(np.float32)
    scale = _scale_vec(scale_kind, shape[0], rng)
    _pool_case(F, x, slope, scale, _pool_plants(x, scale), "%r slope %r scale %r: " % (shape, slope, scale_kind))


def test_maxpool_act_forward_record_grid_stride(F):
    """32 x 200 x 200 outputs: more than the 4096 x 256 threads of the launch, so every thread visits a second element."""
    rng = np.random.RandomState(5)
    x = rng.randn(32, 400, 400).astype(np.float32)
    scale = _scale_vec("keep", 32, rng)
    plants = [p for p in _pool_plants(x, scale) if p[0] in ("first pixel", "last row, last column", "negative window, last cell")]
    assert plants[1][2][0] * 200 * 200 > 4096 * 256
    _pool_case(F, x, 0.25, scale, plants, "grid stride: ")


# ------------------------------------------------------------------------------------------------ activation backward
def _chunks(C_, hw):
    """Blocks per channel of the two backward launches (elem.hip act_bwd_chunks): only used to aim the planted values."""
    return max(1, min(-(-512 // C_), -(-hw // 4096)))


def act_bwd_ref(g, x, slope, scale):
    r = g
    if scale is not None:
        r = (r * scale[:, None]).astype(np.float32)
    if slope is not None:
        r = np.where(x > 0, r, np.float32(slope) * r).astype(np.float32)
    return r


def _bwd_spots(C_, hw, vec):
    ch = _chunks(C_, hw)
    per = -(-hw // ch)
    if vec:
        per = (per + 3) & ~3
    spots = {0: "first", hw - 1: "hw - 1"}
    for k in range(1, ch):
        spots[k * per - 1] = "last element of chunk %d" % (k - 1)
        spots[k * per] = "first element of chunk %d" % k
    return ch, sorted(spots.items())


ACT_SHAPES = [(5, 9, 13), (8, 57, 100), (8, 56, 100), (3, 59, 101), (4, 2, 2)]


@pytest.mark.parametrize("variant", ["plain", "slope", "slope+scale", "in place"])
@pytest.mark.parametrize("shape", ACT_SHAPES)
def test_act_backward_record(F, det_mode, shape, variant):
    C_, H, W = shape
    hw = H * W
    rng = np.random.RandomState(hw % 997)
    g = rng.randn(C_, hw).astype(np.float32)
    x = rng.randn(C_, hw).astype(np.float32)
    slope = None if variant == "plain" else 0.25
    scale = _scale_vec("keep", C_, rng) if variant in ("slope+scale", "in place") else None
    big = np.float32(PLANT * np.abs(g).max())
    ch, spots = _bwd_spots(C_, hw, hw % 4 == 0)
    assert ch == (2 if hw > 4096 else 1)
    dx, ds, dsc = _dev(F, x), (_dev(F, [slope]) if slope else None), (_dev(F, scale) if scale is not None else None)
    dg, dout = F.DeviceTensor.empty(g.shape), F.DeviceTensor.empty(g.shape)
    gb, gs = F.DeviceTensor.zeros((C_,)), F.DeviceTensor.zeros((1,))
    rec = F.DeviceTensor.empty((_rec_floats(F),))
    cases = [(None, None, "randn")]
    for j, (i, what) in enumerate(spots):
        for c in sorted({0, C_ - 1}):
            if scale is None or scale[c] != 0:
                cases.append((c, i, what))
    if scale is not None:
        cases.append((C_ // 2, hw - 1, "dropped channel"))
    for j, (c, i, what) in enumerate(cases):
        gp, xp = g.copy(), x.copy()
        if c is not None:
            gp[c, i] = big if j % 2 else -big
            xp[c, i] = -1.0 if j % 3 else 1.0   # (both PReLU branches under the planted value)
            if what != "dropped channel":
                _unique_max_at(act_bwd_ref(gp, xp, slope, scale), (c, i), what)
        dg.copy_from_numpy(gp)
        dx.copy_from_numpy(xp)
        dst = dg if variant == "in place" else dout
        _poison(F, rec)
        F._lib.call("frcnn_act_backward_rec", F.ptr(dg), F.ptr(dx), C_, hw, F.ptr(ds), F.ptr(dsc), F.ptr(dst), F.ptr(gb), F.ptr(gs),
                    F.stream_ptr(), F.ptr(rec))
        stored = dst.numpy()
        if c is not None and what != "dropped channel":
            assert _argmax(stored) == (c, i), (shape, variant, what)
        _same(rec, stored, "%r %s, %s" % (shape, variant, what))


@pytest.mark.parametrize("variant", ["plain", "slope", "slope+scale"])
@pytest.mark.parametrize("shape", ACT_SHAPES)
def test_maxpool_act_backward_record(F, det_mode, shape, variant):
    C_, H, W = shape
    hw = H * W
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rng = np.random.RandomState(hw % 991)
    x = rng.randn(C_, H, W).astype(np.float32)
    slope = None if variant == "plain" else 0.25
    scale = _scale_vec("keep", C_, rng) if variant == "slope+scale" else None
    idx = pool_ref(x, slope, scale)[1]
    gp = rng.randn(C_, Ho, Wo).astype(np.float32)
    big = np.float32(PLANT * np.abs(gp).max())
    ch, spots = _bwd_spots(C_, hw, W % 4 == 0 and Wo % 2 == 0)
    assert ch == (2 if hw > 4096 else 1)

    def ref(gpool, code, xx):
        yy, xs = np.arange(H)[:, None], np.arange(W)[None, :]
        hit = code[:, yy >> 1, xs >> 1] == ((yy & 1) * 2 + (xs & 1)).astype(np.uint8)[None]
        g = np.where(hit, gpool[:, yy >> 1, xs >> 1], np.float32(0)).astype(np.float32)
        return act_bwd_ref(g.reshape(C_, hw), xx.reshape(C_, hw), slope, scale).reshape(C_, H, W)

    ds, dsc = (_dev(F, [slope]) if slope else None), (_dev(F, scale) if scale is not None else None)
    dx, dgp, didx = F.DeviceTensor.empty(x.shape), F.DeviceTensor.empty(gp.shape), F.DeviceTensor.empty(idx.shape, np.uint8)
    dout = F.DeviceTensor.empty(x.shape)
    gb, gs = F.DeviceTensor.zeros((C_,)), F.DeviceTensor.zeros((1,))
    rec = F.DeviceTensor.empty((_rec_floats(F),))
    cases = [(None, None, "randn")]
    for i, what in spots:
        for c in sorted({0, C_ - 1}):
            if scale is None or scale[c] != 0:
                cases.append((c, i, what))
    for j, (c, i, what) in enumerate(cases):
        g2, i2, x2 = gp.copy(), idx.copy(), x.copy()
        if c is not None:   # the window's winner is made the aimed-at element, the planted gradient is routed there
            y, xx = divmod(i, W)
            i2[c, y >> 1, xx >> 1] = (y & 1) * 2 + (xx & 1)
            g2[c, y >> 1, xx >> 1] = big if j % 2 else -big
            x2[c, y, xx] = -1.0 if j % 3 else 1.0
            _unique_max_at(ref(g2, i2, x2), (c, y, xx), what)
        dx.copy_from_numpy(x2)
        dgp.copy_from_numpy(g2)
        didx.copy_from_numpy(i2)
        _poison(F, rec)
        F._lib.call("frcnn_maxpool_act_backward_rec", F.ptr(dgp), F.ptr(didx), F.ptr(dx), C_, H, W, F.ptr(ds), F.ptr(dsc), F.ptr(dout),
                    F.ptr(gb), F.ptr(gs), F.stream_ptr(), F.ptr(rec))
        stored = dout.numpy()
        if c is not None:
            assert _argmax(stored) == (c, y, xx), (shape, variant, what)
        _same(rec, stored, "%r %s, %s" % (shape, variant, what))


@pytest.mark.parametrize("pooled", [False, True], ids=["act_backward", "maxpool_act_backward"])
def test_backward_records_beyond_the_block_limit(F, det_mode, pooled):
    """16 400 channels = 16 400 blocks, more than a record has entries: the launchers take the magnitude in a pass of its own."""
    C_ = MAX_BLOCKS + 16
    rng = np.random.RandomState(8)
    x = rng.randn(C_, 2, 2).astype(np.float32)
    g = rng.randn(C_, 1 if pooled else 4).astype(np.float32)
    slope = np.float32(0.25)
    ds, dx, dout = _dev(F, [slope]), _dev(F, x), F.DeviceTensor.empty(x.shape)
    gb, gs = F.DeviceTensor.zeros((C_,)), F.DeviceTensor.zeros((1,))
    idx = pool_ref(x, slope, None)[1]
    rec = F.DeviceTensor.empty((_rec_floats(F),))
    dg, didx = F.DeviceTensor.empty(g.shape), _dev(F, idx, np.uint8)
    for c in (None, 0, C_ - 1):
        g2 = g.copy()
        if c is not None:
            g2[c, -1] = -PLANT * np.abs(g).max()
        dg.copy_from_numpy(g2)
        _poison(F, rec)
        if pooled:
            F._lib.call("frcnn_maxpool_act_backward_rec", F.ptr(dg), F.ptr(didx), F.ptr(dx), C_, 2, 2, F.ptr(ds), None,
                        F.ptr(dout), F.ptr(gb), F.ptr(gs), F.stream_ptr(), F.ptr(rec))
        else:
            F._lib.call("frcnn_act_backward_rec", F.ptr(dg), F.ptr(dx), C_, 4, F.ptr(ds), None, F.ptr(dout), F.ptr(gb), F.ptr(gs),
                        F.stream_ptr(), F.ptr(rec))
        stored = dout.numpy()
        if c is not None:
            assert _argmax(stored)[0] == c
        _same(rec, stored, "channel %r" % (c,))


# ------------------------------------------------------------------------------------------------ convolutions
def _conv_fwd(F, x, w, b, slope, scale, pad, rec_in=None, want_rec=True):
    C_, H, W = x.shape
    O_ = w.shape[0]
    out = F.DeviceTensor.empty((O_, H + 2 * pad - 2, W + 2 * pad - 2))
    rec = _new_rec(F) if want_rec else None
    keep = [_dev(F, x), _dev(F, w), _dev(F, b) if b is not None else None, _dev(F, [slope]) if slope is not None else None,
            _dev(F, scale) if scale is not None else None]
    F._lib.call("frcnn_conv2d_forward_rec", F.ptr(keep[0]), C_, H, W, F.ptr(keep[3]), F.ptr(keep[4]), F.ptr(keep[1]), F.ptr(keep[2]), O_, 3,
                pad, F.ptr(out), F.ptr(rec_in), F.ptr(rec), F.stream_ptr())
    return out.numpy(), rec


def _conv_bwd(F, g, w, C_, pad, old=None, rec_g=None, post=None):
    """-> (gin read back, its record, slope gradient); post = (post_x, slope, scale or None)."""
    O_, Ho, Wo = g.shape
    H, W = Ho + 2 - 2 * pad, Wo + 2 - 2 * pad
    gin = _dev(F, old) if old is not None else F.DeviceTensor.empty((C_, H, W))
    rec = _new_rec(F)
    keep = [_dev(F, g), _dev(F, w)]
    pa = [None, None, None, None]
    if post is not None:
        pa = [_dev(F, post[0]), _dev(F, [post[1]]), _dev(F, post[2]) if post[2] is not None else None, F.DeviceTensor.zeros((1,))]
    F._lib.call("frcnn_conv2d_backward_input_rec", F.ptr(keep[0]), O_, Ho, Wo, F.ptr(keep[1]), C_, 3, pad, F.ptr(gin), 1 if old is not None else 0,
                F.ptr(rec_g), F.ptr(rec), F.ptr(pa[0]), F.ptr(pa[1]), F.ptr(pa[2]), F.ptr(pa[3]), F.stream_ptr())
    return gin.numpy(), rec, (pa[3].numpy()[0] if post is not None else None)


def _targets(M, Ho, Wo):
    """(filter, y, x) of the output the planted pair is aimed at: corners of the map (the last pixels of the ragged tiles on both
    edges), first / last filter, and the two filters where one wave's rows end and the next one's begin."""
    t = [(0, 0, 0), (M - 1, Ho - 1, Wo - 1), (0, Ho - 1, Wo - 1), (M - 1, 0, 0), (M - 1, Ho - 1, 0), (0, 0, Wo - 1), (M // 2, Ho // 2, Wo // 2)]
    if M > 64:
        t += [(63, Ho - 1, Wo - 1), (64, Ho - 1, Wo - 1)]
    return t


FWD_SHAPES = [
    # C, H, W, O          pad 1
    (16, 12, 16, 64),     # wide epilogue, 64-filter blocks
    (16, 12, 16, 128),    # wide epilogue, 128-filter blocks
    (16, 12, 16, 192),    # 3 x 64 filters
    (16, 9, 11, 128),     # scalar epilogue, the map is one tile
    (64, 57, 100, 128),   # wide epilogue, tiles ragged at the bottom, one K split
    (64, 23, 37, 128),    # scalar epilogue (odd width), tiles ragged on both edges, one K split
    (64, 57, 99, 128),    # ... several tiles each way
    (128, 28, 50, 256),   # K splits: the fold, four pixels per thread
    (128, 29, 50, 256),   # ... two
    (128, 29, 51, 256),   # ... one
]


@pytest.mark.parametrize("variant", ["plain", "bias", "slope+scale"])
@pytest.mark.parametrize("C_,H,W,O_", FWD_SHAPES)
def test_conv2d_forward_record(F, f16_on, C_, H, W, O_, variant):
    rng = np.random.RandomState(C_ + H + W + O_)
    x = rng.randn(C_, H, W).astype(np.float32)
    w = (rng.randn(O_, C_, 3, 3) * np.sqrt(2.0 / (9 * O_))).astype(np.float32)
    b = rng.randn(O_).astype(np.float32) if variant != "plain" else None
    slope = 0.25 if variant == "slope+scale" else None
    scale = _scale_vec("keep", C_, rng) if variant == "slope+scale" else None
    c0 = C_ - 1   # (a kept channel)
    bx, bw = np.float32(PLANT * np.abs(x).max()), np.float32(PLANT * np.abs(w).max())
    stored, rec = _conv_fwd(F, x, w, b, slope, scale, 1)
    _same(rec, stored, "randn")
    for j, (o, y, xx) in enumerate(_targets(O_, H, W)):
        xp, wp = x.copy(), w.copy()
        xp[c0, y, xx] = bx
        wp[o, c0, 1, 1] = bw if j % 2 else -bw
        stored, rec = _conv_fwd(F, xp, wp, b, slope, scale, 1)
        assert _argmax(stored) == (o, y, xx)
        _same(rec, stored, "aimed at %r" % ((o, y, xx),))
    # The planted pair meets only OUTSIDE the map: below its last row (tap 0,1 over the last input row) / right of its last column
    # (tap 1,0).  A thread of a ragged tile computes that product in a masked lane; nothing of it is stored, so none of it belongs
    # in the record.
    for name, (y, xx), tap in (("below the last row", (H - 1, W // 2), (0, 1)), ("right of the last column", (H // 2, W - 1), (1, 0)),
                               ("below the last pixel", (H - 1, W - 1), (0, 1))):
        xp, wp = x.copy(), w.copy()
        xp[c0, y, xx] = bx
        wp[O_ - 1, c0, tap[0], tap[1]] = bw
        stored, rec = _conv_fwd(F, xp, wp, b, slope, scale, 1)
        _same(rec, stored, name)


BWD_SHAPES = [
    # O (K channels), Ho, Wo, C (filters of the launch)
    (16, 12, 16, 64), (16, 12, 16, 128), (16, 9, 11, 128), (64, 57, 100, 128),
    (64, 23, 37, 128), (64, 57, 99, 128),   # the scalar epilogue on tiles ragged on both edges
    (128, 28, 50, 256), (128, 29, 50, 256), (128, 29, 51, 256),
]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("O_,Ho,Wo,C_", BWD_SHAPES)
def test_conv2d_backward_input_record(F, f16_on, O_, Ho, Wo, C_, accumulate):
    rng = np.random.RandomState(C_ + Ho + Wo + O_ + 1)
    g = rng.randn(O_, Ho, Wo).astype(np.float32)
    w = (rng.randn(O_, C_, 3, 3) * np.sqrt(2.0 / (9 * O_))).astype(np.float32)
    o0 = O_ - 1
    bg, bw = np.float32(PLANT * np.abs(g).max()), np.float32(PLANT * np.abs(w).max())
    # accumulate: what is there before is larger than the convolution's own values, so a record of the summand alone is wrong
    old = (rng.randn(C_, Ho, Wo) * 8).astype(np.float32) if accumulate else None
    stored, rec, _ = _conv_bwd(F, g, w, C_, 1, old)
    _same(rec, stored, "randn")
    for j, (c, y, xx) in enumerate(_targets(C_, Ho, Wo)):
        gp, wp = g.copy(), w.copy()
        gp[o0, y, xx] = bg
        wp[o0, c, 1, 1] = bw if j % 2 else -bw
        stored, rec, _ = _conv_bwd(F, gp, wp, C_, 1, old)
        assert _argmax(stored) == (c, y, xx)
        _same(rec, stored, "aimed at %r" % ((c, y, xx),))
    if accumulate:   # the maximum of the sum comes from what was there
        o2 = old.copy()
        o2[C_ - 1, Ho - 1, Wo - 1] = -PLANT * PLANT * np.abs(old).max()
        stored, rec, _ = _conv_bwd(F, g, w, C_, 1, o2)
        assert _argmax(stored) == (C_ - 1, Ho - 1, Wo - 1)
        _same(rec, stored, "maximum in the old values")
    # the planted pair meets outside the map only (gin[y] takes gout[y + 1 - ky]: the last row reaches y = H through ky = 2)
    for name, (y, xx), tap in (("below the last row", (Ho - 1, Wo // 2), (2, 1)), ("right of the last column", (Ho // 2, Wo - 1), (1, 2)),
                               ("below the last pixel", (Ho - 1, Wo - 1), (2, 1))):
        gp, wp = g.copy(), w.copy()
        gp[o0, y, xx] = bg
        wp[o0, C_ - 1, tap[0], tap[1]] = bw
        stored, rec, _ = _conv_bwd(F, gp, wp, C_, 1, old)
        _same(rec, stored, name)


POST_SHAPES = [
    (64, 28, 52, 128),    # one K split: the fused epilogue, four pixels per thread
    (64, 29, 50, 128),    # ... one pixel per thread
    (64, 29, 50, 64),     # ... 64-filter blocks
    (64, 23, 37, 128),    # ... tiles ragged on both edges
    (128, 29, 50, 256),   # K splits: the activation backward runs in the fold
    (128, 28, 50, 256),
]


@pytest.mark.parametrize("O_,Ho,Wo,C_", POST_SHAPES)
def test_conv2d_backward_input_record_through_the_fused_activation_backward(F, f16_on, O_, Ho, Wo, C_):
    rng = np.random.RandomState(C_ + Ho + Wo + O_ + 2)
    g = rng.randn(O_, Ho, Wo).astype(np.float32)
    w = (rng.randn(O_, C_, 3, 3) * np.sqrt(2.0 / (9 * O_))).astype(np.float32)
    px = rng.randn(C_, Ho, Wo).astype(np.float32)
    scale = _scale_vec("keep", C_, rng)
    scale[[c for c, _, _ in _targets(C_, Ho, Wo)]] = 1.0   # the channels aimed at are kept ones; one beside them is dropped
    dropped = C_ // 2 + 1
    scale[dropped] = 0.0
    slope = np.float32(0.25)
    o0 = O_ - 1
    bg, bw = np.float32(PLANT * np.abs(g).max()), np.float32(PLANT * np.abs(w).max())
    plain, _, _ = _conv_bwd(F, g, w, C_, 1)
    stored, rec, gs = _conv_bwd(F, g, w, C_, 1, post=(px, slope, scale))
    _same(rec, stored, "randn")
    # the epilogue did apply the activation backward: dropped channels are zero, the others prelu'(x) times the plain result
    want = plain * scale[:, None, None] * np.where(px > 0, np.float32(1), slope)
    assert not stored[scale == 0].any() and np.allclose(stored, want, rtol=1e-4, atol=1e-5)
    assert np.isfinite(gs) and gs != 0
    for scale_v in (scale, None):
        for j, (c, y, xx) in enumerate(_targets(C_, Ho, Wo)):
            gp, wp, xp = g.copy(), w.copy(), px.copy()
            gp[o0, y, xx] = bg
            wp[o0, c, 1, 1] = bw if j % 2 else -bw
            xp[c, y, xx] = -1.0 if j % 3 else 1.0   # (the planted value lands on both PReLU branches)
            stored, rec, _ = _conv_bwd(F, gp, wp, C_, 1, post=(xp, slope, scale_v))
            assert _argmax(stored) == (c, y, xx)
            _same(rec, stored, "aimed at %r" % ((c, y, xx),))
    # aimed at a dropped channel: its stored values are zeros, the record is of the others
    gp, wp = g.copy(), w.copy()
    gp[o0, Ho - 1, Wo - 1] = bg
    wp[o0, dropped, 1, 1] = bw
    stored, rec, _ = _conv_bwd(F, gp, wp, C_, 1, post=(px, slope, scale))
    assert not stored[dropped].any()
    _same(rec, stored, "dropped channel")
    # the planted pair meets outside the map only: a masked lane's product, which the epilogue must leave out of the record
    for name, (y, xx), tap in (("below the last row", (Ho - 1, Wo // 2), (2, 1)), ("right of the last column", (Ho // 2, Wo - 1), (1, 2)),
                               ("below the last pixel", (Ho - 1, Wo - 1), (2, 1))):
        gp, wp = g.copy(), w.copy()
        gp[o0, y, xx] = bg
        wp[o0, C_ - 1, tap[0], tap[1]] = bw
        stored, rec, _ = _conv_bwd(F, gp, wp, C_, 1, post=(px, slope, None))
        _same(rec, stored, name)


def test_conv_rec_entry_points_refuse_what_is_not_the_fp16_form(F, f16_on):
    x, w = np.zeros((16, 8, 8), np.float32), np.zeros((64, 16, 3, 3), np.float32)
    with pytest.raises(F.FrcnnError):   # 3 input channels: not a split shape
        _conv_fwd(F, np.zeros((3, 8, 8), np.float32), np.zeros((64, 3, 3, 3), np.float32), None, None, None, 1)
    with pytest.raises(F.FrcnnError):   # a scale entry beyond 1 leaves the fp16 form
        _conv_fwd(F, x, w, None, None, np.full(16, 2.0, np.float32), 1)
    with pytest.raises(F.FrcnnError):   # 48 filters: not a split shape
        _conv_bwd(F, np.zeros((16, 8, 8), np.float32), np.zeros((16, 48, 3, 3), np.float32), 48, 1)
    _option(F, "x3_f16", 0)
    try:
        with pytest.raises(F.FrcnnError):
            _conv_fwd(F, x, w, None, None, None, 1)
        with pytest.raises(F.FrcnnError):
            _conv_bwd(F, np.zeros((16, 8, 8), np.float32), np.zeros((16, 64, 3, 3), np.float32), 64, 1)
    finally:
        _option(F, "x3_f16", 1)
    out, rec = _conv_fwd(F, x, w, None, None, None, 1)   # (and the same call goes through with the option back on)
    assert rec_max(rec.numpy()) == 0 and not out.any()


# ------------------------------------------------------------------------------------------------ a record the consumer is handed
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_consumer_reduces_any_record_of_the_same_maximum(F, f16_on):
    """The consumer takes the exponent of the largest entry: however the producer's blocks split the tensor, and whatever lies
    behind the n entries, the result is bit-identical to the one with a record taken by the entry point itself."""
    rng = np.random.RandomState(23)
    C_, H, W, O_ = 64, 23, 37, 128
    x = rng.randn(C_, H, W).astype(np.float32)
    w = (rng.randn(O_, C_, 3, 3) * 0.05).astype(np.float32)
    b = rng.randn(O_).astype(np.float32)
    base, _ = _conv_fwd(F, x, w, b, None, None, 1)
    m = np.abs(x).max()
    lo = np.float32(2.0 ** np.floor(np.log2(m)))

    def record(n, entries):
        r = _poison_host(F)
        r[:1] = np.array([n], np.int32).view(np.float32)
        r[1:1 + n] = 0
        for i, v in entries.items():
            assert 1 <= i <= n
            r[i] = v
        return r
    cases = {"the maximum alone": record(1, {1: m}),
             "16384 entries, the last one": record(MAX_BLOCKS, {MAX_BLOCKS: m}),
             "300 entries, entry 256": record(300, {256: m}),
             "300 entries, entry 300": record(300, {300: m}),
             "lowest value of the binade": record(1, {1: lo}),
             "highest value of the binade": record(7, {3: np.nextafter(np.float32(2) * lo, np.float32(0)), 5: m})}
    for name, r in cases.items():
        got, rec_out = _conv_fwd(F, x, w, b, None, None, 1, rec_in=_dev(F, r))
        assert np.array_equal(_bits(got), _bits(base)), name
        _same(rec_out, got, name)
    # ... and a record of another binade does change the planes (the argument is read at all)
    got, _ = _conv_fwd(F, x, w, b, None, None, 1, rec_in=_dev(F, record(1, {1: m * np.float32(2.0 ** 12)})))
    assert not np.array_equal(_bits(got), _bits(base))


def test_records_chain_from_producer_to_consumer(F, f16_on):
    rng = np.random.RandomState(29)
    # forward: the pooling launch keeps the record the convolution reads
    x = rng.randn(64, 45, 73).astype(np.float32)
    scale = _scale_vec("keep", 64, rng)
    w = (rng.randn(128, 64, 3, 3) * 0.05).astype(np.float32)
    pooled, idx, rec = F.DeviceTensor.empty((64, 23, 37)), F.DeviceTensor.empty((64, 23, 37), np.uint8), _new_rec(F)
    keep = [_dev(F, x), _dev(F, [0.25]), _dev(F, scale)]
    F._lib.call("frcnn_maxpool_act_forward_rec", F.ptr(keep[0]), 64, 45, 73, F.ptr(keep[1]), F.ptr(keep[2]), F.ptr(pooled), F.ptr(idx),
                F.stream_ptr(), F.ptr(rec))
    p = pooled.numpy()
    _same(rec, p)
    a, _ = _conv_fwd(F, p, w, None, None, None, 1, rec_in=rec)
    b, _ = _conv_fwd(F, p, w, None, None, None, 1)
    assert np.array_equal(_bits(a), _bits(b))
    # backward: the activation backward keeps the record the input-gradient launch reads
    gy = rng.randn(128, 23 * 37).astype(np.float32)
    xx = rng.randn(128, 23 * 37).astype(np.float32)
    gx, rec2 = F.DeviceTensor.empty(gy.shape), _new_rec(F)
    keep = [_dev(F, gy), _dev(F, xx), _dev(F, [0.25]), F.DeviceTensor.zeros((128,)), F.DeviceTensor.zeros((1,))]
    F._lib.call("frcnn_act_backward_rec", F.ptr(keep[0]), F.ptr(keep[1]), 128, 23 * 37, F.ptr(keep[2]), None, F.ptr(gx), F.ptr(keep[3]),
                F.ptr(keep[4]), F.stream_ptr(), F.ptr(rec2))
    g = gx.numpy().reshape(128, 23, 37)
    _same(rec2, g)
    a, ra, _ = _conv_bwd(F, g, w, 64, 1, rec_g=rec2)
    b, rb, _ = _conv_bwd(F, g, w, 64, 1)
    assert np.array_equal(_bits(a), _bits(b))
    _same(ra, a)


# ------------------------------------------------------------------------------------------------ the nets' own records
K_REC_X, K_REC_POOL, K_X, K_REC_GX, K_POOL, K_REC_W, K_GX = 5, 6, 7, 8, 9, 10, 11


def _dbg(F, nat, kind, index):
    p, n = C.c_void_p(), C.c_longlong()
    F._lib.call("frcnn_model_debug_buffer", nat.h, kind, index, C.byref(p), C.byref(n))
    return p.value, n.value


def _split_shape(cin, m, k):
    """kernels.h conv_x3_eligible: the shapes the split launches (hence the fp16 form and its records) take."""
    return k in (3, 5, 7) and cin >= 16 and cin % 16 == 0 and m % (64 if k == 3 else 128) == 0


def _expected_records(model, training):
    """Which records a pass must keep, from the layer table alone: {(kind, index)}."""
    want = set()
    ci, cin = 0, 3
    convs = []
    for b, l in enumerate(model["layers"]):
        for st in range(l["conv_steps"]):
            convs.append((b, st, cin, l["filters"], l["kW"], st == l["conv_steps"] - 1))
            cin = l["filters"]
    for ci, (b, st, cin, cout, k, last) in enumerate(convs):
        x_f = k == 3 and _split_shape(cin, cout, k)
        x_d = ci > 0 and _split_shape(cout, cin, k)
        # its output's record: kept for the next convolution of the block, when that one takes the split form
        if not last and _split_shape(cout, convs[ci + 1][3], convs[ci + 1][4]) and convs[ci + 1][4] == 3:
            want.add((K_REC_X, ci))
        # its output gradient's: kept for its own input-gradient launch (none for the very first convolution, an fp32 kernel)
        if training and x_d:
            want.add((K_REC_GX, ci))
        if x_f or x_d:
            want.add((K_REC_W, ci))
    for b in range(len(model["layers"])):
        want.add((K_REC_POOL, b))
    for h, a in enumerate(model["anchor_nets"]):
        if _split_shape(model["layers"][a["input"] - 1]["filters"], a["n"], a["kW"]):
            want.add((K_REC_W, len(convs) + h))
    return want, convs


def _run_model(F, model, H, W, training, masks, rng):
    import torch
    pnet = model["pnet"]
    pnet.training() if training else pnet.evaluate()
    pnet.drop_masks = masks if training else None
    img = rng.randn(3, H, W).astype(np.float32)

    def one_pass():
        outs = pnet.forward(img)
        if training:
            deltas = pnet.delta_outputs()
            r2 = np.random.RandomState(11)
            for d in deltas:   # dense deltas on every output: every anchor net takes the dense backward path
                d.copy_from_numpy(r2.randn(*d.shape).astype(np.float32))
            pnet.backward(img, deltas)
        torch.cuda.synchronize()
    return one_pass


def _check_model(F, model_fn, cfg_name, H, W, training, compact, runs_compact=None):
    runs_compact = bool(training and compact) if runs_compact is None else runs_compact
    cfg = dict(getattr(F, cfg_name))
    model = getattr(F, model_fn)(cfg)
    w, g = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=5)
    nat = model["native"]
    rng = np.random.RandomState(H + W)
    masks = [None if l["dropout"] <= 0 else (rng.rand(l["filters"]) > l["dropout"]).astype(np.float32) for l in model["layers"]]
    before = _option(F, "drop_compact")
    _option(F, "drop_compact", compact)
    try:
        one_pass = _run_model(F, model, H, W, training, masks, rng)
        want, convs = _expected_records(model, training)
        nrec = len(convs) + len(model["anchor_nets"])
        universe = [(K_REC_X, i) for i in range(len(convs))] + [(K_REC_GX, i) for i in range(len(convs))] + \
                   [(K_REC_POOL, b) for b in range(len(model["layers"]))] + [(K_REC_W, i) for i in range(nrec)]

        def live():
            got = {}
            for key in universe:
                try:
                    got[key] = _dbg(F, nat, *key)
                except F.FrcnnError:
                    pass
            return got
        one_pass()
        first = live()
        assert set(first) == want, (sorted(set(first) - want), sorted(want - set(first)))
        for p, n in first.values():   # poison what the pass keeps, run the same pass again: every record must be rewritten
            assert n == _rec_floats(F) * 4
            _poison(F, F.DeviceTensor(p, (_rec_floats(F),)))
        one_pass()
        got = live()
        assert got == first
        wh = w.cpu().numpy()
        table = nat.param_table
        smaller = 0
        for (kind, i), (p, n) in sorted(got.items()):
            rec = F.DeviceTensor(p, (_rec_floats(F),))
            if kind == K_REC_W:
                off, cnt = (table[3 * i] if i < len(convs) else table[3 * len(convs) + 5 * (i - len(convs))])[:2]
                assert table[3 * i if i < len(convs) else 3 * len(convs) + 5 * (i - len(convs))][2] == 0
                _same(rec, wh[off:off + cnt], "weights %d" % i)
                continue
            tp, tn = _dbg(F, nat, {K_REC_X: K_X, K_REC_GX: K_GX, K_REC_POOL: K_POOL}[kind], i)
            stored = F.DeviceTensor(tp, (tn // 4,)).numpy()
            if kind != K_REC_POOL:
                b, st, cin, cout, k, last = convs[i]
                _, dn = _dbg(F, nat, 0, i)
                assert tn <= dn
                if tn < dn:   # stored compact: the kept channels, padded to a multiple of 64 filters
                    nk = int(masks[b].sum())
                    assert st == 0 and runs_compact and tn * cout == dn * (-(-nk // 64) * 64)
                    smaller += 1
            assert stored.any()
            _same(rec, stored, "kind %d index %d" % (kind, i))
        if runs_compact:
            assert smaller >= 2, "no block ran compact: the compact records are not covered"
        else:
            assert smaller == 0
        # option x3_f16 off: no record is kept, every record kind refuses
        _option(F, "x3_f16", 0)
        try:
            one_pass()
            assert live() == {}
        finally:
            _option(F, "x3_f16", 1)
    finally:
        _option(F, "drop_compact", before)
        model["pnet"].drop_masks = None


@pytest.mark.parametrize("compact", [1, 0], ids=["compact", "dense"])
@pytest.mark.parametrize("size", [(128, 176), (131, 173)])
def test_model_records_training(F, f16_on, size, compact):
    _check_model(F, "vgg_small", "duplo_cfg", size[0], size[1], True, compact)


def test_model_records_training_deterministic(F, f16_on):
    """Deterministic mode fuses no activation backward into the input-gradient launches (and runs no block compact): every
    gradient record comes from act_backward / maxpool_act_backward in a pass of its own."""
    before = _option(F, "deterministic")
    _option(F, "deterministic", 1)
    try:
        _check_model(F, "vgg_small", "duplo_cfg", 131, 173, True, 1, runs_compact=False)
    finally:
        _option(F, "deterministic", before)


@pytest.mark.parametrize("size", [(128, 176), (131, 173)])
def test_model_records_evaluate(F, f16_on, size):
    _check_model(F, "vgg_small", "duplo_cfg", size[0], size[1], False, 1)


def test_model_records_vgg_large_three_convolution_blocks(F, f16_on):
    _check_model(F, "vgg_large", "imgnet_cfg", 99, 131, True, 1)
