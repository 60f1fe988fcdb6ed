"""Detector.detect_batch: many frames per call.  Kernel level (no model): the segmented NMS against the single-problem
entry point and the oracle, the batched anchor scan against the single-frame scan.  Detector level: detect_batch against
detect() on the same frames, BIT FOR BIT (every stage of a frame sees the inputs detect() gives it, through the same
kernels or kernels that share their code), against the oracle under the rules of test_gpu_model.check_detect, the number
of host waits, and evaluate_detections(batch=...)."""
import ctypes as C

import numpy as np
import pytest

from util import assert_close, oracle_model, random_boxes

pytestmark = pytest.mark.gpu
H, W = 128, 176
SENTINEL = -7


# ------------------------------------------------------------------------------------------------ kernel level: NMS
def _nms_single(F, boxes, n_cap, n, ncols, thr, cls):
    """frcnn_nms_device_n on one segment (host arrays in, pick list out)."""
    db = F.DeviceTensor.from_numpy(boxes)
    dc = F.DeviceTensor.from_numpy(cls) if cls is not None else None
    ndev = F.DeviceTensor.from_numpy(np.array([n], np.int32))
    wsb = F._lib.load().frcnn_nms_workspace_bytes(n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    pick = F.DeviceTensor.empty((n_cap,), np.int64); cnt = F.DeviceTensor.zeros((1,), np.int32)
    F._lib.call("frcnn_nms_device_n", F.ptr(db), n_cap, F.ptr(ndev), ncols, C.c_float(thr), 0, 0, F.ptr(dc), F.ptr(pick), F.ptr(cnt),
                F.ptr(ws), wsb, F.stream_ptr())
    return pick.numpy()[:int(cnt.numpy()[0])].tolist()


def _nms_batch(F, boxes, B, row_stride, n_cap, counts, ncols, thr, cls):
    """frcnn_nms_device_batch; returns (pick [B][row_stride] + a guard tail, count [B] + a guard entry, boxes read back)."""
    db = F.DeviceTensor.from_numpy(boxes)
    dc = F.DeviceTensor.from_numpy(cls) if cls is not None else None
    ndev = F.DeviceTensor.from_numpy(np.asarray(counts, np.int32))
    L = F._lib.load()
    wsb = L.frcnn_nms_batch_workspace_bytes(B, n_cap)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    pick = F.DeviceTensor.from_numpy(np.full(B * row_stride + 64, SENTINEL, np.int64))
    cnt = F.DeviceTensor.from_numpy(np.full(B + 1, SENTINEL, np.int32))
    F._lib.call("frcnn_nms_device_batch", F.ptr(db), B, row_stride, n_cap, F.ptr(ndev), ncols, C.c_float(thr), 0, 0, F.ptr(dc),
                F.ptr(pick), F.ptr(cnt), F.ptr(ws), wsb, F.stream_ptr())
    return pick.numpy(), cnt.numpy(), db.numpy()


def _oracle_nms(O, b, thr, cls):
    """Pick list of the reference: plain nms, or one nms per class with the lists merged back into global pick order
    (descending key = max-y; random_boxes keys are unique)."""
    if len(b) == 0:
        return []
    if cls is None:
        return O.nms(b, thr).tolist()
    ids = []
    for c in np.unique(cls):
        rows = np.nonzero(cls == c)[0]
        ids += [int(rows[i - 1]) + 1 for i in O.nms(b[rows], thr).tolist()]
    return sorted(ids, key=lambda i: -b[i - 1, 3])


# per-segment device counts (the issue's set; a count above n_cap is clipped to it by the kernels)
_COUNTS = {
    (1, "empty"): [0], (1, "full"): ["cap"], (1, "part"): [63],
    (3, "mix"): [0, "cap", 65],
    (8, "mix"): [1, 0, 63, "cap", 64, 65, 700, 0],
}


@pytest.mark.parametrize("with_cls", [False, True])
@pytest.mark.parametrize("n_cap", [64, 2000])
@pytest.mark.parametrize("B,which", sorted(_COUNTS.keys()))
def test_nms_batch_equals_single_problem_nms_and_oracle(F, O, B, which, n_cap, with_cls):
    counts = [n_cap if c == "cap" else c for c in _COUNTS[(B, which)]]
    if B > 1:
        assert 0 in counts and n_cap in counts          # one empty and one full segment in the same call
    row_stride = n_cap + 37
    ncols = 5 if with_cls else 4
    rng = np.random.RandomState(1000 * B + n_cap + int(with_cls))
    boxes = np.zeros((B * row_stride, ncols), np.float32)
    for b in range(B):
        boxes[b * row_stride:(b + 1) * row_stride, :4] = random_boxes(rng, row_stride)
    if with_cls:
        boxes[:, 4] = rng.rand(len(boxes))
    cls = rng.randint(1, 5, B * row_stride).astype(np.int32) if with_cls else None
    thr = 0.1 if with_cls else 0.25
    pick, cnt, boxes_after = _nms_batch(F, boxes, B, row_stride, n_cap, counts, ncols, thr, cls)
    assert np.array_equal(boxes_after, boxes)
    assert cnt[B] == SENTINEL and np.all(pick[B * row_stride:] == SENTINEL)
    for b in range(B):
        n = min(counts[b], n_cap)
        seg = boxes[b * row_stride:(b + 1) * row_stride]
        scl = cls[b * row_stride:(b + 1) * row_stride] if with_cls else None
        k = int(cnt[b])
        got = pick[b * row_stride:b * row_stride + k].tolist()
        assert np.all(pick[b * row_stride + k:(b + 1) * row_stride] == SENTINEL), "segment %d: stray stores behind its picks" % b
        want = _nms_single(F, seg[:n_cap].copy(), n_cap, counts[b], ncols, thr, scl[:n_cap].copy() if with_cls else None)
        assert got == want, "segment %d (count %d) differs from frcnn_nms_device_n" % (b, counts[b])
        assert got == _oracle_nms(O, seg[:n], thr, scl[:n] if with_cls else None), "segment %d differs from the oracle" % b
        if n == 0:
            assert k == 0


def test_nms_batch_tie_rule_does_not_leak_across_segments(F, O):
    """The same boxes, equal keys included, in every segment: identical pick lists in every segment, and the oracle's."""
    B, n = 8, 500
    rng = np.random.RandomState(3)
    b = random_boxes(rng, n, unique_y2=False)
    b[:, 3] = np.round(b[:, 3] / 8) * 8     # many equal keys
    row_stride = n + 12
    boxes = np.zeros((B * row_stride, 4), np.float32)
    for s in range(B):
        boxes[s * row_stride:s * row_stride + n] = b
    pick, cnt, _ = _nms_batch(F, boxes, B, row_stride, n, [n] * B, 4, 0.25, None)
    want = O.nms(b, 0.25).tolist()
    for s in range(B):
        assert pick[s * row_stride:s * row_stride + int(cnt[s])].tolist() == want, "segment %d" % s


# ------------------------------------------------------------------------------------------------ kernel level: scan
def test_rpn_scan_batch_equals_rpn_scan_per_slot(F, small_cfg):
    sizes = [(55, 98), (27, 48), (25, 46), (23, 44)]     # vgg_small head maps of an 800x450 frame
    model = F.vgg_small(dict(small_cfg))
    anchors = F.Anchors(model["pnet"], small_cfg["scales"])
    aw, ah = F.DeviceTensor.from_numpy(anchors.w), F.DeviceTensor.from_numpy(anchors.h)
    cap = 3 * sum(h * w for h, w in sizes)
    assert cap == 26544
    rng = np.random.RandomState(17)
    # class-logit gain and shift per slot: none passes / all pass / in between
    slots = [(1.0, -30.0), (1.0, 30.0), (1.0, 0.0), (3.0, 2.0), (10.0, 0.0)]
    B = len(slots)
    hoff = [0]
    for h, w in sizes:
        hoff.append(hoff[-1] + (18 * h * w + 63) // 64 * 64)
    slot = hoff[4] + 128
    heads = np.zeros((B, slot), np.float32)
    for b, (gain, shift) in enumerate(slots):
        for l, (h, w) in enumerate(sizes):
            m = (rng.randn(18, h, w) * 0.02).astype(np.float32)
            for a in range(3):
                m[a * 6] = rng.randn(h, w) * gain + shift      # foreground logit
                m[a * 6 + 1] = rng.randn(h, w) * gain
            heads[b, hoff[l]:hoff[l] + m.size] = m.ravel()
    dheads = F.DeviceTensor.from_numpy(heads)
    Hs = (C.c_int * 4)(*[h for h, w in sizes]); Ws = (C.c_int * 4)(*[w for h, w in sizes])
    L = F._lib.load()

    def outputs(rows):
        return dict(p=F.DeviceTensor.from_numpy(np.full(rows, SENTINEL, np.float32)),
                    idx=F.DeviceTensor.from_numpy(np.full((rows, 4), SENTINEL, np.int32)),
                    rect=F.DeviceTensor.from_numpy(np.full((rows, 4), SENTINEL, np.float64)),
                    box=F.DeviceTensor.from_numpy(np.full((rows, 4), SENTINEL, np.float32)))
    o = outputs(B * cap + 16)
    cnt = F.DeviceTensor.from_numpy(np.full(B + 1, SENTINEL, np.int32))
    wsb = L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B)
    ws = F.DeviceTensor.empty((wsb,), np.uint8)
    maps = (C.c_void_p * 4)(*[dheads.ptr + 4 * hoff[l] for l in range(4)])
    F._lib.call("frcnn_rpn_scan_batch", maps, Hs, Ws, B, slot, F.ptr(aw), F.ptr(ah), 800.0, 450.0, 0.95, cap, F.ptr(o["p"]),
                F.ptr(o["idx"]), F.ptr(o["rect"]), F.ptr(o["box"]), F.ptr(cnt), F.ptr(ws), wsb, F.stream_ptr())
    got = {k: v.numpy() for k, v in o.items()}
    counts = cnt.numpy()
    assert counts[B] == SENTINEL
    for k in got:
        assert np.all(got[k][B * cap:] == SENTINEL), k
    wsb1 = L.frcnn_rpn_scan_workspace_bytes(Hs, Ws)
    # (the single call runs on one slice of the batch layout, rounded up to 256 bytes -- 26 544 x 40 is no multiple: nothing may be
    # stored behind the size the library asked for)
    assert wsb1 == L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, 1) and (cap * 40) % 256 != 0
    guard = np.full(wsb1 + 256, 0xA5, np.uint8)
    ws1 = F.DeviceTensor.from_numpy(guard)
    for b in range(B):
        s = outputs(cap)
        c1 = F.DeviceTensor.zeros((1,), np.int32)
        maps1 = (C.c_void_p * 4)(*[dheads.ptr + 4 * (b * slot + hoff[l]) for l in range(4)])
        F._lib.call("frcnn_rpn_scan", maps1, Hs, Ws, F.ptr(aw), F.ptr(ah), 800.0, 450.0, 0.95, cap, F.ptr(s["p"]), F.ptr(s["idx"]),
                    F.ptr(s["rect"]), F.ptr(s["box"]), F.ptr(c1), F.ptr(ws1), wsb1, F.stream_ptr())
        n = int(c1.numpy()[0])
        assert int(counts[b]) == n, "slot %d" % b
        for k in got:
            seg = got[k][b * cap:(b + 1) * cap]
            assert np.array_equal(seg[:n], s[k].numpy()[:n]), "slot %d: %s" % (b, k)
            assert np.all(seg[n:] == SENTINEL), "slot %d: stray stores behind the matches of %s" % (b, k)
    assert np.all(ws1.numpy()[wsb1:] == 0xA5), "frcnn_rpn_scan stored behind its workspace"
    print("scan batch: matches per slot", counts[:B].tolist())
    assert counts[0] == 0 and counts[1] == cap
    assert all(0 < c < cap for c in counts[2:B])


# ------------------------------------------------------------------------------------------------ Detector level
def _amplified_weights(nat, w, ncls, cls_gain=30.0, hidden=512):
    """Head logits amplified so that the p > 0.95 test fires, class head sharpened so that p > 0.2 does
    (test_gpu_model._amplified_weights; `hidden`: width of the layer in front of the class head)."""
    w = w.copy()
    for off, cnt, kind, aux in nat.param_table:
        if kind == 0 and aux == 18:  # the 1x1 head convs (kW*kH*nOutputPlane = 18): amplify the 2 class logits
            v = w[off:off + cnt].reshape(18, -1)
            for a in range(3):
                v[a * 6:a * 6 + 2] *= 60.0
        if kind == 3 and cnt == hidden * ncls:  # class head of cnet: make the arg-max confident (p > 0.2)
            w[off:off + cnt] *= cls_gain
    return w


@pytest.fixture(scope="module")
def setup(F, O):
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w_host = weights.cpu().numpy().copy()
    return dict(cfg=cfg, model=model, weights=weights, gradient=gradient, om=oracle_model(O, cfg), w=w_host,
                wamp=_amplified_weights(model["native"], w_host, 17, cls_gain=200.0))


@pytest.fixture
def amplified(setup):
    import torch
    setup["weights"].copy_(torch.from_numpy(setup["wamp"]))
    try:
        yield setup
    finally:
        setup["weights"].copy_(torch.from_numpy(setup["w"]))


_FIELDS = ("class", "confidence", "p", "l", "candidate")


def _winner_rows(winners):
    rows = []
    for x in winners:
        rows.append(tuple(x[k] for k in _FIELDS) + tuple(getattr(x[r], c) for r in ("r", "r2") for c in ("minX", "minY", "maxX", "maxY"))
                    + (x["a"].layer, x["a"].aspect, repr(x["a"].index), x["a"].minX, x["a"].minY, x["a"].maxX, x["a"].maxY))
    return rows


def _detect_reference(F, model, frames, pooled=False, **kw):
    """[detect(f) for f in frames] from a fresh Detector, with everything detect() leaves behind per frame
    (pooled=True: the classification net's input rows too, from the Detector's own buffer)."""
    d = F.Detector(model)
    for k, v in kw.items():
        setattr(d, k, v)
    out = []
    for f in frames:
        win = d.detect(f)
        m = d.last_scan
        if pooled and m["n"]:
            cfg = model["cfg"]
            D = cfg["roi_pooling"]["kh"] * cfg["roi_pooling"]["kw"] * model["layers"][-1]["filters"]
            rows = d._buf("cinput", (len(d.last_pick), D)).numpy()
        out.append(dict(n=m["n"], idx=m["idx"].numpy(), p=m["p"].numpy(), rect=m["rect"].numpy(), box=m["box"].numpy(),
                        pick=d.last_pick.copy(), cnet=d.last_cnet if m["n"] else None, kept=d._last.get("kept", 0),
                        winners=_winner_rows(win), nwin=len(win), empty_list=(win == [])))
        if pooled:
            out[-1]["pooled"] = rows if m["n"] else None
    return out


def _assert_same(records, results, want, what=""):
    assert len(records) == len(results) == len(want)
    for b, (rec, win, ref) in enumerate(zip(records, results, want)):
        tag = "%s frame %d" % (what, b)
        assert rec["n"] == ref["n"], tag
        for k in ("idx", "p", "rect", "box", "pick"):
            got = rec[k]
            assert got.dtype == ref[k].dtype and got.shape == ref[k].shape and np.array_equal(got, ref[k]), "%s: %s" % (tag, k)
        if ref["cnet"] is None:
            assert rec["cnet"] is None, tag
        else:
            for k in ("bbox", "cls"):
                assert rec["cnet"][k].shape == ref["cnet"][k].shape and np.array_equal(rec["cnet"][k], ref["cnet"][k]), "%s: cnet %s" % (tag, k)
        assert rec["kept"] == ref["kept"], tag
        assert len(win) == ref["nwin"] and _winner_rows(win) == ref["winners"], tag
        if ref["empty_list"]:
            assert win == [], tag


def _frames(F, seeds, h=H, w=W):
    return [F.synthetic_image(h, w, k) for k in seeds]


def test_detect_batch_equals_detect_bit_for_bit(F, amplified):
    s = amplified
    frames = _frames(F, range(5, 13))
    want = _detect_reference(F, s["model"], frames)
    assert any(r["nwin"] > 0 for r in want), "no frame has winners: the back half of the batch path is not exercised"
    d = F.Detector(s["model"])
    got = d.detect_batch(frames)
    _assert_same(d.last_batch, got, want)
    print("detect_batch: matches %s, candidates %s, winners %s" % ([r["n"] for r in want], [len(r["pick"]) for r in want],
                                                                   [r["nwin"] for r in want]))


def test_detect_batch_of_one_frame(F, amplified):
    s = amplified
    frames = _frames(F, [5])
    d = F.Detector(s["model"])
    got = d.detect_batch(frames)
    _assert_same(d.last_batch, got, _detect_reference(F, s["model"], frames), "B = 1")
    assert d.detect_batch([]) == [] and d.last_batch == []


def test_detect_batch_chunks_keep_the_order(F, amplified):
    s = amplified
    frames = _frames(F, range(5, 24))                  # 19 frames: chunks of 8 + 8 + 3
    d = F.Detector(s["model"])
    assert d.BATCH == 8
    got = d.detect_batch(frames)
    _assert_same(d.last_batch, got, _detect_reference(F, s["model"], frames), "19 frames")


def test_detect_batch_with_one_frame_repeated(F, amplified):
    s = amplified
    f = F.synthetic_image(H, W, 5)
    other = F.synthetic_image(H, W, 6)
    frames = [f, f, other, f]
    d = F.Detector(s["model"])
    got = d.detect_batch(frames)
    want = _detect_reference(F, s["model"], frames)
    _assert_same(d.last_batch, got, want, "repeated frame")
    assert _winner_rows(got[0]) == _winner_rows(got[1]) == _winner_rows(got[3])


def test_detect_batch_frames_over_the_first_nms_bound(F, amplified):
    s = amplified
    frames = _frames(F, range(5, 9))
    d = F.Detector(s["model"])
    d.NMS_FIRST_CAP = 8
    got = d.detect_batch(frames)
    assert all(r["n"] > 8 for r in d.last_batch)        # every frame takes the repeat path
    _assert_same(d.last_batch, got, _detect_reference(F, s["model"], frames), "NMS_FIRST_CAP = 8")


def test_detect_between_two_detect_batch_calls(F, amplified):
    s = amplified
    frames = _frames(F, range(5, 10))
    want = _detect_reference(F, s["model"], frames)
    single = _detect_reference(F, s["model"], [frames[2]])[0]
    d = F.Detector(s["model"])
    got1 = d.detect_batch(frames[:3])
    rec1 = d.last_batch
    win = d.detect(frames[2])
    _assert_same(rec1, got1, want[:3], "first call, looked at after detect()")
    assert _winner_rows(win) == single["winners"] and d.last_pick.tolist() == single["pick"].tolist()
    assert np.array_equal(d.last_scan["p"].numpy(), single["p"])
    got2 = d.detect_batch(frames[3:])
    _assert_same(d.last_batch, got2, want[3:], "second call")
    assert [_winner_rows(g) for g in got1] == [r["winners"] for r in want[:3]]
    # detect() still works unchanged afterwards
    win = d.detect(frames[0])
    assert _winner_rows(win) == want[0]["winners"]


def test_detect_batch_with_static_weights(F, amplified):
    s = amplified
    frames = _frames(F, range(5, 9))
    want = _detect_reference(F, s["model"], frames)
    try:
        d = F.Detector(s["model"], static_weights=True)
        for _ in range(2):       # (second round: the packs of the first are re-used)
            got = d.detect_batch(frames)
            _assert_same(d.last_batch, got, want, "static_weights")
    finally:
        F._lib.call("frcnn_set_option", b"static_weights", 0)


def test_detect_batch_without_matches_skips_the_classification_net(F, setup, monkeypatch):
    """Un-amplified random weights: no anchor passes 0.95."""
    s = setup
    d = F.Detector(s["model"])
    calls = []
    cnet = s["model"]["cnet"]
    orig = cnet.forward
    monkeypatch.setattr(cnet, "forward", lambda x, **kw: calls.append(1) or orig(x, **kw))
    got = d.detect_batch(_frames(F, range(5, 9)))
    assert got == [[], [], [], []] and not calls
    assert [r["n"] for r in d.last_batch] == [0, 0, 0, 0]
    assert all(r["pick"].shape == (0,) and r["cnet"] is None and r["kept"] == 0 for r in d.last_batch)


def test_detect_batch_host_waits(F, amplified, monkeypatch):
    s = amplified
    frames = _frames(F, range(5, 13))
    pnet = s["model"]["pnet"]
    fwd = []
    orig_fwd = pnet.forward
    monkeypatch.setattr(pnet, "forward", lambda img, **kw: fwd.append(1) or orig_fwd(img, **kw))

    def counting(d):
        reads = []
        orig = d._read
        d._read = lambda *a, **kw: reads.append(a[1]) or orig(*a, **kw)
        return reads
    d = F.Detector(s["model"])
    reads = counting(d)
    d.detect_batch(frames)
    assert all(r["n"] <= d.NMS_FIRST_CAP for r in d.last_batch) and any(r["n"] > 0 for r in d.last_batch)
    assert len(reads) == 2 and len(fwd) == 8, reads
    # frames over the first-NMS bound: one more wait each
    ns = [r["n"] for r in d.last_batch]
    bound = sorted(ns)[len(ns) // 2]                     # some frames above it, some not
    over = sum(1 for n in ns if n > bound)
    assert 0 < over < 8
    d2 = F.Detector(s["model"])
    d2.NMS_FIRST_CAP = bound
    reads2 = counting(d2)
    d2.detect_batch(frames)
    assert len(reads2) == 2 + over, (reads2, ns, bound)
    # frames of different sizes: refused before anything is queued
    del fwd[:]
    d3 = F.Detector(s["model"])
    reads3 = counting(d3)
    with pytest.raises(ValueError):
        d3.detect_batch([frames[0], F.synthetic_image(H, W + 16, 1), frames[1]])
    assert not reads3 and not fwd


def test_detect_host_waits_and_copies(F, amplified, monkeypatch):
    """detect() is the one-frame chunk of the detect_batch pipeline on the model's own output buffers: two waits, one
    proposal-net pass, no device-to-device copy; the batched scan and gather once each, the batched NMS twice."""
    import torch
    s = amplified
    f = F.synthetic_image(H, W, 5)
    pnet, cnet = s["model"]["pnet"], s["model"]["cnet"]
    fwd, cfwd, calls, reads = [], [], [], []
    orig_fwd, orig_cfwd, orig_call = pnet.forward, cnet.forward, F._lib.call
    monkeypatch.setattr(pnet, "forward", lambda img, **kw: fwd.append(1) or orig_fwd(img, **kw))
    monkeypatch.setattr(cnet, "forward", lambda x, **kw: cfwd.append(1) or orig_cfwd(x, **kw))
    monkeypatch.setattr(F._lib, "call", lambda name, *a, **kw: calls.append(name) or orig_call(name, *a, **kw))
    d = F.Detector(s["model"])
    orig_read = d._read
    d._read = lambda *a, **kw: reads.append(a[1]) or orig_read(*a, **kw)
    win = d.detect(f)
    seen = list(calls)                                   # (looking at last_pick below copies from the device too)
    R = len(d.last_pick)
    assert d.last_scan["n"] > 0 and R > 0 and type(win).__name__ == "_Detections"
    assert reads == [8, (R + 1) * 128], reads
    assert len(fwd) == 1 and len(cfwd) == 1
    assert seen.count("frcnn_memcpy_d2d") == 0
    assert seen.count("frcnn_rpn_scan_batch") == 1 and seen.count("frcnn_detect_gather_batch") == 1
    assert seen.count("frcnn_nms_device_batch") == 2
    # un-amplified weights, no anchor passes 0.95: the frame stops after the first wait, in front of the classification net
    s["weights"].copy_(torch.from_numpy(s["w"]))
    del fwd[:], cfwd[:], reads[:]
    win = d.detect(f)
    assert win == [] and isinstance(win, list)
    assert reads == [8] and len(fwd) == 1 and not cfwd


def _iou_border_pairs(boxes, thr, eps=1e-5):
    """number of box pairs whose nms.lua IoU (the +1 convention of nms.lua:35,88-94) lies within eps of thr"""
    b = boxes.astype(np.float64)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    n = 0
    for lo in range(0, len(b), 512):
        c = b[lo:lo + 512]
        w = np.maximum(0, np.minimum(c[:, None, 2], b[None, :, 2]) - np.maximum(c[:, None, 0], b[None, :, 0]) + 1)
        h = np.maximum(0, np.minimum(c[:, None, 3], b[None, :, 3]) - np.maximum(c[:, None, 1], b[None, :, 1]) + 1)
        inter = w * h
        iou = inter / (area[lo:lo + 512, None] + area[None, :] - inter)
        n += int((np.abs(iou - thr) < eps).sum())
    return n


def _compare_with_oracle(O, rec, winners, ref, tag):
    """One frame of a batch against orc_detect under the rules and tolerances of test_gpu_model.check_detect: lists may
    differ only where a border case is shown to exist (an anchor within 1e-4 of the 0.95 threshold, a box pair within 1e-5
    of an NMS threshold, a class decision within 1e-4); values at 1e-4 / 1e-3.  True: the frame was compared through every
    stage."""
    gp, gidx, grect = rec["p"], rec["idx"], rec["rect"]

    def key(a):
        return set(map(tuple, a.tolist()))
    border_ref = np.abs(np.exp(ref["match_p"].astype(np.float64)) - 0.95) < 1e-4
    border_got = np.abs(np.exp(gp.astype(np.float64)) - 0.95) < 1e-4
    assert key(gidx[~border_got]) - key(ref["match_idx"]) == set()
    assert key(ref["match_idx"][~border_ref]) - key(gidx) == set()
    assert len(gidx) > 10, "test image produced too few matches to be meaningful"
    same_matches = len(gidx) == len(ref["match_idx"]) and np.array_equal(gidx, ref["match_idx"])
    if not (border_ref.any() or border_got.any()):
        assert same_matches, "%s: match lists differ although no anchor is near the threshold" % tag
    boxes = rec["box"]
    assert rec["pick"].tolist() == O.nms(boxes, 0.25).tolist()
    if not same_matches:
        return False
    assert_close(gp, ref["match_p"], 1e-4, "match log-prob")
    assert_close(grect, ref["match_rect"], 1e-3, "decoded rects")
    if rec["pick"].tolist() != ref["cand_ids"].tolist():
        assert _iou_border_pairs(boxes, 0.25) > 0, "%s: NMS candidates differ although no box pair is near the overlap threshold" % tag
        return False
    assert len(ref["cand_ids"]) > 0
    assert_close(rec["cnet"]["bbox"], ref["cand_bbox"], 1e-3, "cnet bbox (eval)")
    assert_close(rec["cnet"]["cls"], ref["cand_cls"], 1e-3, "cnet log-probs (eval)")
    cls_sorted = np.sort(ref["cand_cls"].astype(np.float64), axis=1)
    cls_border = int(((cls_sorted[:, -1] - cls_sorted[:, -2]) < 1e-4).sum() + (np.abs(np.exp(cls_sorted[:, -1]) - 0.2) < 1e-4).sum())
    got_cls = [x["class"] for x in winners]; want_cls = [int(r[0]) for r in ref["winners"]]
    if got_cls != want_cls:
        wb = np.array([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in winners], dtype=np.float32)
        assert cls_border > 0 or _iou_border_pairs(wb, 0.1) > 0, "%s: winners differ without a border case" % tag
        return False
    if len(winners):
        assert_close([x["confidence"] for x in winners], ref["winners"][:, 1], 1e-3, "winner confidence")
        assert_close([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in winners], ref["winners"][:, 2:6],
                     1e-3, "winner rects (Detector.lua:107)")
    return True


def test_detect_batch_against_the_oracle(F, O, amplified):
    s = amplified
    seeds = list(range(5, 10))
    frames = _frames(F, seeds)
    d = F.Detector(s["model"])
    got = d.detect_batch(frames)
    bn = s["model"]["native"].bn_running.cpu().numpy()
    deep = []
    for b, seed in enumerate(seeds):
        ref = O.detect(s["om"], s["wamp"], bn, frames[b])
        if _compare_with_oracle(O, d.last_batch[b], got[b], ref, "frame %d" % seed):
            deep.append((seed, len(got[b])))
    print("detect_batch vs oracle: frames compared through every stage (seed, winners):", deep)
    assert deep, "no frame of the batch went through every stage"
    assert max(nw for _, nw in deep) > 0, "no winner among the frames compared through every stage"


def test_detect_batch_full_size_vgg_small(F):
    """450x800, B = 4: the launch shapes of a real frame (26 544 anchors, the 16 384-row first NMS), once."""
    import torch
    cfg = dict(F.duplo_cfg)
    model = F.vgg_small(cfg)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=42)
    w = _amplified_weights(model["native"], weights.cpu().numpy().copy(), cfg["class_count"] + 1, cls_gain=200.0)
    for off, cnt, kind, aux in model["native"].param_table:     # x30 on the class logits: about 8 000 matches a frame
        if kind == 0 and aux == 18:
            v = w[off:off + cnt].reshape(18, -1)
            for a in range(3):
                v[a * 6:a * 6 + 2] *= 0.5
    weights.copy_(torch.from_numpy(w))
    frames = _frames(F, range(4), 450, 800)
    want = _detect_reference(F, model, frames)
    d = F.Detector(model)
    got = d.detect_batch(frames)
    _assert_same(d.last_batch, got, want, "450x800")
    print("full-size detect_batch: matches %s, candidates %s, winners %s" % ([r["n"] for r in want], [len(r["pick"]) for r in want],
                                                                             [r["nwin"] for r in want]))
    assert max(r["n"] for r in want) > 1000 and any(r["nwin"] > 0 for r in want)


def test_detect_batch_vgg_large_topology(F):
    """vgg_large topology (2-2-3-3 conv steps, 7x7 pooling, 200 classes) at the narrow widths and the 120x168 frames of
    test_gpu_large.py, B = 2."""
    import torch
    layers = [
        dict(filters=8, kW=3, kH=3, padW=1, padH=1, dropout=0.0, conv_steps=2),
        dict(filters=16, kW=3, kH=3, padW=1, padH=1, dropout=0.4, conv_steps=2),
        dict(filters=24, kW=3, kH=3, padW=1, padH=1, dropout=0.4, conv_steps=3),
        dict(filters=40, kW=3, kH=3, padW=1, padH=1, dropout=0.4, conv_steps=3),
    ]
    heads = [dict(kW=3, n=24, input=3), dict(kW=3, n=24, input=4), dict(kW=5, n=24, input=4), dict(kW=7, n=24, input=4)]
    cls = [dict(n=48, dropout=0.5, batch_norm=True), dict(n=32, dropout=0.5)]
    cfg = dict(F.imgnet_cfg)
    cfg["roi_pooling"] = dict(kw=7, kh=7)
    model = F.create_model(cfg, layers, heads, cls)
    weights, gradient = F.combine_and_flatten_parameters(model["pnet"], model["cnet"], seed=3)
    w = _amplified_weights(model["native"], weights.cpu().numpy().copy(), cfg["class_count"] + 1, cls_gain=400.0, hidden=32)
    weights.copy_(torch.from_numpy(w))
    frames = _frames(F, [2, 3], 120, 168)
    want = _detect_reference(F, model, frames)
    d = F.Detector(model)
    got = d.detect_batch(frames)
    _assert_same(d.last_batch, got, want, "vgg_large topology")
    print("vgg_large-topology detect_batch: matches %s, candidates %s, winners %s"
          % ([r["n"] for r in want], [len(r["pick"]) for r in want], [r["nwin"] for r in want]))
    assert all(r["n"] > 0 for r in want), "no matches: only the scan was exercised"


class _Val(object):
    """nextValidation(count) -> [{img, rois}] over a fixed list (the synthetic iterator of test_gpu_eval.py)."""

    def __init__(self, items):
        self.items, self.i = items, 0

    def nextValidation(self, count=1):
        out = []
        for _ in range(count):
            out.append(self.items[self.i % len(self.items)])
            self.i += 1
        return out


def test_evaluate_detections_in_batches(F, amplified):
    from frcnn_amd.Rect import Rect
    from frcnn_amd.evaluation import evaluate_detections
    s = amplified
    frames = _frames(F, [60 + k for k in range(6)])
    d = F.Detector(s["model"])
    items = []
    for img in frames:     # ground truth: every third detection's box (true positives), shifted copies, an undetected class
        rois = []
        for j, x in enumerate(list(d.detect(img))[::3]):
            r = x["r2"]
            rois.append(F.Roi(Rect(r.minX, r.minY, r.maxX, r.maxY) if j % 2 == 0 else r.offset(r.width() * 0.8, 0), x["class"]))
        rois.append(F.Roi(Rect(5, 5, 40, 40), 16))
        items.append(dict(img=img, rois=rois))
    one = evaluate_detections(F.Detector(s["model"]), _Val(items), len(items))
    assert one["detections"] > 0 and one["tp"] > 0
    for batch in (4, 2, 16):
        got = evaluate_detections(F.Detector(s["model"]), _Val(items), len(items), batch=batch)
        assert got == one, batch


# ------------------------------------------------------------------------------------------------ shared_cnet=True
def _rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


RMS_GATE = 1.75     # what tests/test_gpu_convx.py grants an alternative arithmetic form, per case


def test_shared_cnet_pass_against_the_oracle(F, O, amplified):
    """One classification-net pass for the candidates of all frames: everything up to the pooled rows is bit-identical to
    detect() per frame; the net's outputs are compared with the ORACLE on the device's own pooled rows at 1e-3 (the bar of
    check_detect for this stage), and their RMS error may exceed the per-frame pass's error against the same oracle by at
    most RMS_GATE per case (frame x output) -- never one device path against the other."""
    s = amplified
    frames = _frames(F, range(5, 13))
    want = _detect_reference(F, s["model"], frames, pooled=True)
    d = F.Detector(s["model"])
    got = d.detect_batch(frames, shared_cnet=True)
    bn = s["model"]["native"].bn_running.cpu().numpy()
    assert len(got) == 8 and sum(r["n"] > 0 for r in want) > 1
    for b, (rec, ref) in enumerate(zip(d.last_batch, want)):
        assert rec["n"] == ref["n"]
        for k in ("idx", "p", "rect", "box", "pick"):
            assert np.array_equal(rec[k], ref[k]), "frame %d: %s" % (b, k)
        if ref["n"] == 0:
            assert rec["cnet"] is None and rec["pooled"] is None
            continue
        assert rec["pooled"].shape == ref["pooled"].shape and np.array_equal(rec["pooled"], ref["pooled"]), "frame %d: pooled rows" % b
        ob, oc, _ = O.cnet_forward(s["om"], s["wamp"], rec["pooled"], False, None, bn)
        for name, o in (("bbox", ob), ("cls", oc)):
            shared, own = rec["cnet"][name], ref["cnet"][name]
            assert shared.shape == o.shape
            es, eo = _rms(shared, o), _rms(own, o)
            print("frame %d %-4s: RMS error against the oracle, shared pass %.3e, per-frame pass %.3e, ratio %.2f" % (b, name, es, eo, es / max(eo, 1e-30)))
            assert_close(shared, o, 1e-3, "frame %d: cnet %s of the shared pass" % (b, name))
            assert es <= RMS_GATE * eo, "frame %d %s: %.3e > %.2f x %.3e" % (b, name, es, RMS_GATE, eo)


def test_shared_cnet_winners_follow_from_its_own_outputs(F, O, amplified):
    """The winners of each frame equal what the host mirror of Detector.lua:106-136 derives from the shared pass's OWN
    classification-net outputs: arg-max, exp(conf) > 0.2, Anchors.anchorToInput in double, nms per class at 0.1 on the fp32
    boxes -- classes, candidate rows and order exact, r2 to 2e-15 relative (device exp against libm)."""
    import math
    s = amplified
    frames = _frames(F, range(5, 13))
    d = F.Detector(s["model"])
    got = d.detect_batch(frames, shared_cnet=True)
    bg = s["cfg"]["class_count"] + 1
    assert any(len(g) > 0 for g in got)
    for b, (rec, win) in enumerate(zip(d.last_batch, got)):
        if rec["n"] == 0:
            assert win == []
            continue
        bbox, logp = rec["cnet"]["bbox"], rec["cnet"]["cls"]
        cls = np.argmax(logp, axis=1) + 1                                   # Detector.lua:110-113
        conf = logp[np.arange(len(cls)), cls - 1]
        keep = np.nonzero((cls != bg) & (np.exp(conf.astype(np.float64)) > 0.2))[0]     # :115
        assert rec["kept"] == len(keep)
        ra = rec["rect"][rec["pick"][keep] - 1]
        aw, ah = ra[:, 2] - ra[:, 0], ra[:, 3] - ra[:, 1]
        t = bbox[keep].astype(np.float64)
        x0 = t[:, 0] * aw + ra[:, 0]; y0 = t[:, 1] * ah + ra[:, 1]
        ew = np.array([math.exp(v) for v in t[:, 2].tolist()]) * aw; eh = np.array([math.exp(v) for v in t[:, 3].tolist()]) * ah
        r2 = np.stack([x0, y0, x0 + ew, y0 + eh], 1).reshape(-1, 4)
        bb = r2.astype(np.float32)
        want = []                                                           # (class, candidate row 1-based, row of keep)
        for c in sorted(set(cls[keep].tolist())):                           # :125-136, classes ascending
            rows = np.nonzero(cls[keep] == c)[0]
            for i in O.nms(bb[rows], 0.1).tolist():
                want.append((c, int(keep[rows[i - 1]]) + 1, int(rows[i - 1])))
        assert [(x["class"], x["candidate"]) for x in win] == [(c, r) for c, r, _ in want], "frame %d" % b
        if want:
            j = [k for _, _, k in want]
            got_r2 = np.array([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in win])
            assert np.allclose(got_r2, r2[j], rtol=2e-15, atol=0), "frame %d: r2" % b
            assert [x["confidence"] for x in win] == [float(conf[keep[k]]) for k in j]
