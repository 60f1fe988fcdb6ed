"""Frames of different sizes in one detect_batch call (mixed_sizes=True).  Kernel level: frcnn_rpn_scan_ragged on the frames of
tests/scan_ragged_cases.py -- per frame BIT FOR BIT frcnn_rpn_scan on that frame alone, against scan_ref under the value rule
of tests/anchor_ops_ref.py, nothing stored behind a frame's matches, behind B * cap rows, behind count[B - 1] or behind the
workspace size the library asked for; truncation; frames of one size against frcnn_rpn_scan_batch; every refusal.  Detector
level: detect_batch(frames, mixed_sizes=True) against [detect(f)] bit for bit under the Detector's settings, the number of host
waits, chunks of one size inside a mixed call, the default call's refusal, evaluate_detections(mixed_sizes=True).  The one
front: its copies and its scan for a chunk of one size and for a mixed one, the layout cache, the shape check."""
import ctypes as C

import numpy as np
import pytest

import scan_ragged_cases as cases
from test_gpu_detect_batch import _Val, _amplified_weights, _assert_same, _detect_reference, _winner_rows

pytestmark = pytest.mark.gpu
SENTINEL = -7
KEYS = ("p", "idx", "rect", "box")
DTYPES = dict(p=np.float32, idx=np.int32, rect=np.float64, box=np.float32)


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Deviations(object):
    """|got - want| <= tol elementwise (tol 0: bit for bit), keeping the largest deviation per quantity for the report"""

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
            w[0], w[1], w[2] = max(w[0], float(np.nanmax(dev))), max(w[1], float(np.nanmax(ratio))), w[2] + dev.size
        bad = ~(dev <= tol)
        assert not bad.any(), "%s: %d of %d outside the bound; worst |got - want| = %.3e" % (name, int(bad.sum()), bad.size,
                                                                                              float(dev[bad].max()))

    def report(self, title):
        for name in sorted(self.worst):
            a, r, n = self.worst[name]
            print("%s: %-5s largest |got - want| = %.3e = %.3f of its bound (%d values)" % (title, name, a, r, n))


# ================================================================================================ kernel level
@pytest.fixture(scope="module")
def tables(F):
    aw, ah = cases.tables()
    return F.DeviceTensor.from_numpy(aw), F.DeviceTensor.from_numpy(ah)


def _outputs(F, rows, tail):
    """the four match arrays of rows + tail rows, all SENTINEL"""
    return {k: F.DeviceTensor.from_numpy(np.full((rows + tail,) + ((4,) if k != "p" else ()), SENTINEL, DTYPES[k])) for k in KEYS}


_SINGLE = {}


def _single(F, tables, c, cap):
    """frcnn_rpn_scan on the frame alone -> (count, the cap rows of the four match arrays); computed once per (frame, cap)"""
    key = (c["name"], c["pattern"], c["img_w"], c["img_h"], cap)
    if key not in _SINGLE:
        L = F._lib.load()
        Hs, Ws = _ints(c["H"]), _ints(c["W"])
        dm = [F.DeviceTensor.from_numpy(m) for m in c["maps"]]
        maps = (C.c_void_p * 4)(*[m.ptr for m in dm])
        o = _outputs(F, cap, 0)
        cnt = F.DeviceTensor.from_numpy(np.full(1, SENTINEL, np.int32))
        wsb = L.frcnn_rpn_scan_workspace_bytes(Hs, Ws)
        ws = F.DeviceTensor.empty((wsb,), np.uint8)
        F._lib.call("frcnn_rpn_scan", maps, Hs, Ws, F.ptr(tables[0]), F.ptr(tables[1]), c["img_w"], c["img_h"], cases.THR, cap,
                    F.ptr(o["p"]), F.ptr(o["idx"]), F.ptr(o["rect"]), F.ptr(o["box"]), F.ptr(cnt), F.ptr(ws), wsb, F.stream_ptr())
        _SINGLE[key] = (int(cnt.numpy()[0]), {k: v.numpy() for k, v in o.items()})
    return _SINGLE[key]


class _Problem(object):
    """B frames packed into one `heads` buffer (NaNs between the maps and between the frames), with the host arrays of a
    frcnn_rpn_scan_ragged call, SENTINEL-filled outputs (a tail that holds every match of the largest frame behind B * cap
    rows, one more count entry) and a 0xA5 guard behind the workspace size the library asks for"""

    def __init__(self, F, tables, frames, cap):
        self.F, self.frames, self.cap, self.B = F, frames, cap, len(frames)
        B = self.B
        off, o = [], 3
        for c in frames:
            for m in c["maps"]:
                off.append(o)
                o += m.size + 5
            o += 37
        self.heads_host = np.full(max(o, 1), np.nan, np.float32)
        for b, c in enumerate(frames):
            for l, m in enumerate(c["maps"]):
                self.heads_host[off[4 * b + l]:off[4 * b + l] + m.size] = m.ravel()
        self.heads = F.DeviceTensor.from_numpy(self.heads_host)
        self.map_off = (C.c_longlong * max(4 * B, 1))(*off)
        self.Hs = _ints([h for c in frames for h in c["H"]] or [0])
        self.Ws = _ints([w for c in frames for w in c["W"]] or [0])
        self.img = (C.c_double * max(2 * B, 1))(*[v for c in frames for v in (c["img_w"], c["img_h"])])
        self.tail = max([c["total"] for c in frames] + [0]) + 16
        self.out = _outputs(F, B * cap, self.tail)
        self.cnt = F.DeviceTensor.from_numpy(np.full(B + 1, SENTINEL, np.int32))
        self.wsb = F._lib.load().frcnn_rpn_scan_ragged_workspace_bytes(self.Hs, self.Ws, B)
        self.ws = F.DeviceTensor.from_numpy(np.full(self.wsb + 256, 0xA5, np.uint8))
        self.aw, self.ah = tables

    def args(self, **kw):
        F = self.F
        a = dict(heads=F.ptr(self.heads), map_off=self.map_off, Hs=self.Hs, Ws=self.Ws, img=self.img, B=self.B, aw=F.ptr(self.aw),
                 ah=F.ptr(self.ah), thr=cases.THR, cap=self.cap, p=F.ptr(self.out["p"]), idx=F.ptr(self.out["idx"]),
                 rect=F.ptr(self.out["rect"]), box=F.ptr(self.out["box"]), cnt=F.ptr(self.cnt), ws=F.ptr(self.ws), wsb=self.wsb)
        a.update(kw)
        return [a[k] for k in ("heads", "map_off", "Hs", "Ws", "img", "B", "aw", "ah", "thr", "cap", "p", "idx", "rect", "box", "cnt",
                               "ws", "wsb")] + [F.stream_ptr()]

    def run(self):
        self.F._lib.call("frcnn_rpn_scan_ragged", *self.args())
        return self.read()

    def read(self):
        got = {k: v.numpy() for k, v in self.out.items()}
        counts = self.cnt.numpy()
        rows = self.B * self.cap
        for k in KEYS:
            assert np.all(got[k][rows:] == SENTINEL), "match_%s: stores behind B * cap rows" % k
        assert counts[self.B] == SENTINEL, "count[B] was written"
        assert np.all(self.ws.numpy()[self.wsb:] == 0xA5), "stores behind the workspace"
        assert same_bits(self.heads.numpy(), self.heads_host), "the head maps were written"
        return got, counts

    def untouched(self):
        """nothing at all was written (a refused call, B = 0)"""
        for k in KEYS:
            assert np.all(self.out[k].numpy() == SENTINEL), k
        assert np.all(self.cnt.numpy() == SENTINEL) and np.all(self.ws.numpy() == 0xA5)


def _check(F, tables, D, frames, cap, got, counts, what):
    for b, c in enumerate(frames):
        tag = "%s frame %d (%s/%s)" % (what, b, c["name"], c["pattern"])
        n1, one = _single(F, tables, c, cap)
        w = c["want"]
        assert int(counts[b]) == n1 == w["count"], "%s: count %d, frcnn_rpn_scan %d, reference %d" % (tag, counts[b], n1, w["count"])
        k = min(n1, cap)
        for key in KEYS:
            seg = got[key][b * cap:(b + 1) * cap]
            assert same_bits(seg[:k], one[key][:k]), "%s: match_%s differs from frcnn_rpn_scan on the frame alone" % (tag, key)
            assert np.all(seg[k:] == SENTINEL), "%s: rows behind the frame's %d matches of match_%s were written" % (tag, k, key)
        assert same_bits(got["idx"][b * cap:b * cap + k], w["idx"][:k]), "%s: match_idx against the reference" % tag
        D.check("p", got["p"][b * cap:b * cap + k], w["p"][:k], w["p_tol"][:k])
        D.check("rect", got["rect"][b * cap:b * cap + k], w["rect"][:k], w["rect_tol"][:k])
        D.check("box", got["box"][b * cap:b * cap + k], w["box"][:k], w["box_tol"][:k])


@pytest.mark.parametrize("which", ["B1", "B3", "B17"])
def test_ragged_scan_equals_the_single_frame_scan_and_the_reference(F, tables, which):
    D = Deviations()
    calls = dict(B1=[(i,) for i in range(len(cases.FRAMES))], B3=[cases.CALL_B3], B17=[cases.CALL_B17])[which]
    for idx in calls:
        frames = cases.frames(idx)
        cap = max(c["total"] for c in frames)       # what the Detector passes: the largest frame's anchors
        got, counts = _Problem(F, tables, frames, cap).run()
        _check(F, tables, D, frames, cap, got, counts, which)
    D.report("rpn_scan_ragged %s" % which)


def test_ragged_scan_truncates_per_frame(F, tables):
    """cap = 5 below both counts: count reports the full numbers, five rows a frame are written, nothing behind them"""
    frames = cases.frames(cases.CALL_TRUNCATED)
    D = Deviations()
    got, counts = _Problem(F, tables, frames, 5).run()
    assert [int(v) for v in counts[:2]] == [c["want"]["count"] for c in frames] and counts[1] == frames[1]["total"] > 5
    _check(F, tables, D, frames, 5, got, counts, "cap 5")
    for k in KEYS:
        assert np.all(got[k][:10] != SENTINEL), k


def test_ragged_scan_of_one_size_equals_the_batch_scan(F, tables):
    frames = cases.one_size_frames()
    c0, B = frames[0], len(frames)
    cap = c0["total"]
    pr = _Problem(F, tables, frames, cap)
    got, counts = pr.run()
    L = F._lib.load()
    Hs, Ws = _ints(c0["H"]), _ints(c0["W"])
    assert L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B) == pr.wsb
    slot = pr.map_off[4] - pr.map_off[0]
    assert all(pr.map_off[4 * b + l] - pr.map_off[l] == b * slot for b in range(B) for l in range(4))
    maps = (C.c_void_p * 4)(*[pr.heads.ptr + 4 * pr.map_off[l] for l in range(4)])
    o = _outputs(F, B * cap, 0)
    cnt = F.DeviceTensor.from_numpy(np.full(B, SENTINEL, np.int32))
    ws = F.DeviceTensor.empty((pr.wsb,), np.uint8)
    F._lib.call("frcnn_rpn_scan_batch", maps, Hs, Ws, B, slot, F.ptr(pr.aw), F.ptr(pr.ah), c0["img_w"], c0["img_h"], cases.THR, cap,
                F.ptr(o["p"]), F.ptr(o["idx"]), F.ptr(o["rect"]), F.ptr(o["box"]), F.ptr(cnt), F.ptr(ws), pr.wsb, F.stream_ptr())
    assert np.array_equal(cnt.numpy(), counts[:B])
    assert sorted(int(v) for v in counts[:B]) [::B - 1] == [0, cap]
    for k in KEYS:
        assert same_bits(o[k].numpy(), got[k][:B * cap]), k


def test_ragged_scan_refusals_write_nothing(F, tables):
    L = F._lib.load()
    frames = cases.frames(cases.CALL_B3)
    cap = max(c["total"] for c in frames)

    def refused(what, needle=None, **kw):
        pr = _Problem(F, tables, frames, cap)
        if "patch" in kw:
            kw.pop("patch")(pr)
        rc = L.frcnn_rpn_scan_ragged(*pr.args(**kw))
        assert rc != 0, "%s was accepted" % what
        assert L.frcnn_last_error(), what
        if needle:
            assert needle in L.frcnn_last_error(), (what, L.frcnn_last_error())
        with pytest.raises(F.FrcnnError):
            F._lib.call("frcnn_rpn_scan_ragged", *pr.args(**kw))
        pr.untouched()
    refused("B = -1", B=-1)
    refused("B = 65536", B=65536)
    refused("cap = -1", cap=-1)
    refused("a workspace one byte short", wsb=_Problem(F, tables, frames, cap).wsb - 1)

    def size(arr, i, v):
        def patch(pr):
            getattr(pr, arr)[i] = v
            # (the workspace is sized for the frames as they are: the refusal must come from the size, not from the workspace)
        return patch
    refused("H = 201", b"200", patch=size("Hs", 5, 201))
    refused("W = 201", b"200", patch=size("Ws", 10, 201))
    refused("H = 0", patch=size("Hs", 0, 0))
    refused("W = -3", patch=size("Ws", 11, -3))
    refused("a negative offset", patch=size("map_off", 6, -1))
    for name in ("heads", "map_off", "Hs", "Ws", "img", "aw", "ah", "p", "idx", "rect", "box", "cnt", "ws"):
        refused("%s = NULL" % name, **{name: None})
    # B = 0: no error, nothing written -- with or without arrays
    pr = _Problem(F, tables, frames, cap)
    F._lib.call("frcnn_rpn_scan_ragged", *pr.args(B=0))
    F._lib.call("frcnn_rpn_scan_ragged", *pr.args(B=0, heads=None, map_off=None, Hs=None, Ws=None, img=None))
    pr.untouched()


# ================================================================================================ Detector level
SIZES = [(128, 176), (128, 192), (144, 176), (176, 128), (128, 176)]      # (H, W)
SEEDS = [5, 6, 7, 8, 9]
ALIGN = dict(kw=6, kh=6, method="align", sampling_ratio=2)


@pytest.fixture(scope="module")
def setup(F):
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w_host = weights.cpu().numpy().copy()
    return dict(cfg=cfg, model=model, weights=weights, gradient=gradient, w=w_host,
                wamp=_amplified_weights(model["native"], w_host, 17, cls_gain=200.0))


@pytest.fixture
def amplified(setup):
    import torch
    setup["weights"].copy_(torch.from_numpy(setup["wamp"]))
    try:
        yield setup
    finally:
        setup["weights"].copy_(torch.from_numpy(setup["w"]))


def _blank(F, h, w):
    """a frame without a match (asserted where it is used): a constant image"""
    return np.zeros((3, h, w), np.float32)


def _mixed_frames(F):
    fr = [F.synthetic_image(h, w, k) for (h, w), k in zip(SIZES, SEEDS)]
    return fr[:3] + [_blank(F, 160, 144)] + fr[3:]


def _run_mixed(F, s, what, batch=None, **kw):
    """detect_batch(mixed_sizes=True) against the detect() loop under the Detector attributes kw -> (detector, want)"""
    frames = _mixed_frames(F)
    want = _detect_reference(F, s["model"], frames, **kw)
    assert want[3]["n"] == 0 and want[3]["empty_list"], "the blank frame has matches"
    assert sum(r["nwin"] > 0 for r in want) >= 3, "%s: too few frames with winners: %s" % (what, [r["nwin"] for r in want])
    d = F.Detector(s["model"])
    for k, v in kw.items():
        setattr(d, k, v)
    if batch:
        d.BATCH = batch
    got = d.detect_batch(frames, mixed_sizes=True)
    _assert_same(d.last_batch, got, want, what)
    print("%s: matches %s, candidates %s, winners %s" % (what, [r["n"] for r in want], [len(r["pick"]) for r in want],
                                                         [r["nwin"] for r in want]))
    return d, want


def test_mixed_detect_batch_equals_detect_bit_for_bit(F, amplified, monkeypatch):
    """default settings; one ragged scan for the chunk, two host waits, one proposal-net pass per frame"""
    s = amplified
    pnet = s["model"]["pnet"]
    fwd, calls = [], []
    orig_fwd, orig_call = pnet.forward, F._lib.call
    frames = _mixed_frames(F)
    want = _detect_reference(F, s["model"], frames)
    assert want[3]["n"] == 0 and sum(r["nwin"] > 0 for r in want) >= 3, [r["nwin"] for r in want]
    monkeypatch.setattr(pnet, "forward", lambda img, **kw: fwd.append(1) or orig_fwd(img, **kw))
    monkeypatch.setattr(F._lib, "call", lambda name, *a, **kw: calls.append(name) or orig_call(name, *a, **kw))
    d = F.Detector(s["model"])
    reads = []
    orig_read = d._read
    d._read = lambda *a, **kw: reads.append(a[1]) or orig_read(*a, **kw)
    got = d.detect_batch(frames, mixed_sizes=True)
    seen = list(calls)
    assert all(r["n"] <= d.NMS_FIRST_CAP for r in d.last_batch)
    assert len(reads) == 2 and len(fwd) == len(frames), (reads, len(fwd))
    assert seen.count("frcnn_rpn_scan_ragged") == 1 and seen.count("frcnn_rpn_scan_batch") == 0
    assert seen.count("frcnn_nms_device_batch") == 2 and seen.count("frcnn_detect_gather_batch") == 1
    _assert_same(d.last_batch, got, want, "mixed sizes")
    # detect() afterwards is untouched by what the mixed call left behind
    assert _winner_rows(d.detect(frames[1])) == want[1]["winners"]


def test_mixed_detect_batch_under_score_order_and_caps(F, amplified):
    d, want = _run_mixed(F, amplified, "order = score, caps", proposal_order="score", pre_nms_top_n=300, post_nms_top_n=40)
    assert any(r["matches"] > 300 for r in d.last_batch) and any(len(r["pick"]) == 40 for r in want)


def test_mixed_detect_batch_under_soft_nms(F, amplified):
    _run_mixed(F, amplified, "nms gaussian", nms_method="gaussian")


def test_mixed_detect_batch_under_box_voting(F, amplified):
    _run_mixed(F, amplified, "box voting", box_voting=F.Detector.box_voting_settings({}))


def test_mixed_detect_batch_under_roi_align(F, amplified):
    cfg = amplified["model"]["cfg"]
    before = cfg.get("roi_pooling")
    cfg["roi_pooling"] = dict(ALIGN)
    try:
        _run_mixed(F, amplified, "roi align")
    finally:
        cfg["roi_pooling"] = before


def test_mixed_detect_batch_in_chunks_of_two(F, amplified):
    """BATCH = 2: three chunks, each of two sizes; the records of the earlier chunks are detached"""
    _run_mixed(F, amplified, "BATCH = 2", batch=2)


def test_mixed_detect_batch_frames_over_the_first_nms_bound(F, amplified):
    """NMS_FIRST_CAP = 8: every frame with matches repeats its first NMS alone -- one more wait each"""
    s = amplified
    frames = _mixed_frames(F)
    want = _detect_reference(F, s["model"], frames, NMS_FIRST_CAP=8)
    d = F.Detector(s["model"])
    d.NMS_FIRST_CAP = 8
    reads = []
    orig_read = d._read
    d._read = lambda *a, **kw: reads.append(a[1]) or orig_read(*a, **kw)
    got = d.detect_batch(frames, mixed_sizes=True)
    over = sum(1 for r in want if r["n"] > 8)
    assert over >= 3 and len(reads) == 2 + over
    _assert_same(d.last_batch, got, want, "NMS_FIRST_CAP = 8")


def test_mixed_detect_batch_shared_cnet(F, amplified):
    """shared_cnet=True: everything up to the pooled rows bit-identical to detect(), the net's outputs within 1e-3"""
    from util import assert_close
    s = amplified
    frames = _mixed_frames(F)
    want = _detect_reference(F, s["model"], frames, pooled=True)
    d = F.Detector(s["model"])
    got = d.detect_batch(frames, shared_cnet=True, mixed_sizes=True)
    assert len(got) == len(frames)
    for b, (rec, w) in enumerate(zip(d.last_batch, want)):
        assert rec["n"] == w["n"]
        for k in ("idx", "p", "rect", "box", "pick"):
            assert np.array_equal(rec[k], w[k]), "frame %d: %s" % (b, k)
        if w["n"] == 0:
            assert rec["cnet"] is None and rec["pooled"] is None
            continue
        assert rec["pooled"].shape == w["pooled"].shape and np.array_equal(rec["pooled"], w["pooled"]), "frame %d: pooled rows" % b
        for name in ("bbox", "cls"):
            assert_close(rec["cnet"][name], w["cnet"][name], 1e-3, "frame %d: cnet %s of the shared pass" % (b, name))


def test_mixed_call_with_chunks_of_one_size_is_the_default_call(F, amplified, monkeypatch):
    """BATCH = 2 over frames a a b b: no chunk mixes sizes -> no ragged call, each chunk is the default call on it"""
    s = amplified
    a = [F.synthetic_image(128, 176, k) for k in (5, 6)]
    b = [F.synthetic_image(144, 176, k) for k in (7, 8)]
    calls = []
    orig_call = F._lib.call
    monkeypatch.setattr(F._lib, "call", lambda name, *args, **kw: calls.append(name) or orig_call(name, *args, **kw))
    d = F.Detector(s["model"])
    d.BATCH = 2
    got = d.detect_batch(a + b, mixed_sizes=True)
    seen = list(calls)
    assert seen.count("frcnn_rpn_scan_ragged") == 0 and seen.count("frcnn_rpn_scan_batch") == 2
    recs = d.last_batch
    d2 = F.Detector(s["model"])
    d2.BATCH = 2
    for lo, chunk in ((0, a), (2, b)):
        want = d2.detect_batch(chunk)
        for j in range(2):
            assert _winner_rows(got[lo + j]) == _winner_rows(want[j])
            for k in ("idx", "p", "rect", "box", "pick"):
                assert np.array_equal(recs[lo + j][k], d2.last_batch[j][k]), (lo + j, k)
    assert any(len(g) > 0 for g in got)


def test_mixed_sizes_without_the_keyword_are_refused(F, amplified, monkeypatch):
    s = amplified
    pnet = s["model"]["pnet"]
    fwd = []
    orig_fwd = pnet.forward
    monkeypatch.setattr(pnet, "forward", lambda img, **kw: fwd.append(1) or orig_fwd(img, **kw))
    d = F.Detector(s["model"])
    reads = []
    orig_read = d._read
    d._read = lambda *a, **kw: reads.append(a[1]) or orig_read(*a, **kw)
    with pytest.raises(ValueError):
        d.detect_batch(_mixed_frames(F))
    with pytest.raises(ValueError):      # a frame that is not 3 x H x W: refused under the keyword as well, before any device call
        d.detect_batch([_mixed_frames(F)[0], np.zeros((128, 176), np.float32)], mixed_sizes=True)
    assert not reads and not fwd


def test_evaluate_detections_mixed_sizes(F, amplified):
    from frcnn_amd.Rect import Rect
    from frcnn_amd.evaluation import evaluate_detections
    s = amplified
    frames = _mixed_frames(F)
    d = F.Detector(s["model"])
    items = []
    for img in frames:     # ground truth: every third detection's box, some of them shifted, and an undetected class
        rois = []
        for j, x in enumerate(list(d.detect(img))[::3]):
            r = x["r2"]
            rois.append(F.Roi(Rect(r.minX, r.minY, r.maxX, r.maxY) if j % 2 == 0 else r.offset(r.width() * 0.8, 0), x["class"]))
        rois.append(F.Roi(Rect(5, 5, 40, 40), 16))
        items.append(dict(img=img, rois=rois))
    one = evaluate_detections(F.Detector(s["model"]), _Val(items), len(items))
    assert one["detections"] > 0 and one["tp"] > 0
    got = evaluate_detections(F.Detector(s["model"]), _Val(items), len(items), batch=4, mixed_sizes=True)
    assert got == one


# ================================================================================================ the one front
SCANS = ("frcnn_rpn_scan_batch", "frcnn_rpn_scan_ragged")


def _counted(F, monkeypatch):
    """the names of the library calls made through _lib.call from here on"""
    calls = []
    orig_call = F._lib.call
    monkeypatch.setattr(F._lib, "call", lambda name, *a, **kw: calls.append(name) or orig_call(name, *a, **kw))
    return calls


@pytest.mark.parametrize("sizes,scan", [([(128, 176)] * 3, SCANS[0]), ([(128, 176), (144, 176), (176, 128)], SCANS[1])])
def test_front_copies_and_scan(F, amplified, monkeypatch, sizes, scan):
    """a chunk of 3 frames: five copies a frame in front of ONE scan -- the batch scan for one size, the ragged scan for three"""
    frames = [F.synthetic_image(h, w, k) for (h, w), k in zip(sizes, SEEDS)]
    d = F.Detector(amplified["model"])
    calls = _counted(F, monkeypatch)
    got = d.detect_batch(frames, mixed_sizes=len(set(sizes)) > 1)
    seen = list(calls)
    assert len(got) == 3 and [n for n in seen if n in SCANS] == [scan]
    assert seen[:seen.index(scan)].count("frcnn_memcpy_d2d") == 15


def _snapshot(d, win):
    """what detect() returned and left behind, as _detect_reference keeps it"""
    m = d.last_scan
    return dict(n=m["n"], idx=m["idx"].numpy(), p=m["p"].numpy(), rect=m["rect"].numpy(), box=m["box"].numpy(),
                pick=d.last_pick.copy(), cnet=d.last_cnet if m["n"] else None, kept=d._last.get("kept", 0),
                winners=_winner_rows(win), nwin=len(win), empty_list=(win == []))


def test_layout_is_worked_out_once_per_size(F, amplified, monkeypatch):
    """detect(a), detect(b) of another size, detect(a): the layer lists are walked once per size, and the third call is the first"""
    import sys
    mod = sys.modules[F.Detector.__module__]
    walks = []
    orig = mod._map_hw
    monkeypatch.setattr(mod, "_map_hw", lambda layers, H, W: walks.append((H, W)) or orig(layers, H, W))
    a, b = F.synthetic_image(128, 176, 5), F.synthetic_image(144, 176, 7)
    d = F.Detector(amplified["model"])
    outputs = len(amplified["model"]["pnet"].outnode.children)
    first = _snapshot(d, d.detect(a))
    assert first["n"] > 0 and walks == [(128, 176)] * outputs
    other = _snapshot(d, d.detect(b))
    assert other["n"] > 0 and walks == [(128, 176)] * outputs + [(144, 176)] * outputs
    win = d.detect(a)
    assert len(walks) == 2 * outputs
    _assert_same([d._last], [win], [first], "the first size again")
    for k in ("idx", "p", "rect", "box"):
        assert same_bits(d.last_scan[k].numpy(), first[k]), k


def test_shape_check_guards_the_one_size_chunk(F, amplified, monkeypatch):
    """a layout that reports a head map one row too tall: detect() and a one-size detect_batch raise on the host, in front of
    the scan"""
    d = F.Detector(amplified["model"])
    orig = d._layout_of

    def too_tall(H, W):
        t = orig(H, W)
        hw = list(t.hw)
        hw[1] = (hw[1][0] + 1, hw[1][1])
        return t._replace(hw=hw)
    d._layout_of = too_tall
    frames = [F.synthetic_image(128, 176, k) for k in (5, 6)]
    calls = _counted(F, monkeypatch)
    with pytest.raises(F._lib.FrcnnError, match="gives maps"):
        d.detect(frames[0])
    with pytest.raises(F._lib.FrcnnError, match="gives maps"):
        d.detect_batch(frames)
    assert not [n for n in calls if n.startswith("frcnn_rpn_scan")] and "frcnn_memcpy_d2d" not in calls
    d._layout_of = orig      # the Detector is none the worse for it
    d.detect(frames[0])
    assert d.last_scan["n"] > 0
