"""cfg["scoring"]["boxes"] = "class" through the Detector, on the tiny per-class model of tests/test_gpu_box_head_model.py (its
fixture, imported) with a box head whose weights are NOT zero: a row's box depends on its class AND on its candidate's features.
  (a) "all" at one half with boxes = "class" is "top" at one half, bit for bit: over one half only the arg-max passes, and its
      box is the one the net's own pass computes with the same arithmetic (fails without the feature: the combination is refused)
  (b) at 0.05 every detection's r2 is recomputed from cnet.features, its candidate, class and anchor rect: the deltas by
      frcnn_box_head_forward, their decode by frcnn_detect_post bit for bit and by the numpy restatement (x0 / y0 bit for bit,
      x1 / y1 within the two exp()'s ulp); one candidate at least yields two classes with different boxes
  (c) detect_batch equals the detect() loop bit for bit: plain, mixed sizes, a mirrored view, box voting; under shared_cnet every
      frame is judged against the shared pass's own features and outputs
  (d) "top" with boxes = "class" is "top": results and launches
  (e) the key absent: no buffer, no launch; the setting costs one launch per chunk."""
import numpy as np
import pytest

import class_boxes_ref as R
from test_gpu_box_head_model import CLASSES, detector_setup, head       # noqa: F401  (detector_setup: a fixture)
from test_gpu_detect_batch import _winner_rows
from test_gpu_proposals import _launches

pytestmark = pytest.mark.gpu

ALL05 = dict(classes="all", min_confidence=0.05, boxes="class")
SPREAD = 1.5      # standard deviation the class head's logits are scaled to: several classes over 0.05, some over one half


def _features(F, model, rows):
    t = F.DeviceTensor.empty((rows, model["cnet"].feature_count))
    model["cnet"].features(t)
    return t.numpy().copy()


@pytest.fixture(scope="module")
def setup(F, detector_setup):
    """detector_setup's model with (1) box-head weights drawn from a seeded normal, scaled so that no delta of any candidate of
    the frames exceeds 0.4 in front of the bias, (2) the class head's weight and bias scaled so that the logits of the frames'
    candidates have standard deviation SPREAD: the mass is shared by several classes."""
    import torch
    s = dict(detector_setup)
    model, nat = s["model"], s["model"]["native"]
    ow, ob, end, nf, rows = head(nat)
    (cw, cn, _, _), (cb, cbn, _, _) = (tuple(int(v) for v in r) for r in nat.param_table[-2:])
    d = F.Detector(model)
    feats = []
    for f in s["frames"]:
        d.detect(f)
        if d.last_scan["n"]:
            feats.append(_features(F, model, len(d.last_pick)))
    X = np.concatenate(feats).astype(np.float64)
    w = s["w"].copy()
    W0 = np.random.RandomState(3).standard_normal((rows, nf)).astype(np.float32)
    w[ow:ob] = (W0 * np.float32(0.4 / np.abs(X @ W0.T.astype(np.float64)).max())).ravel()
    Z = X @ w[cw:cw + cn].reshape(-1, nf).T.astype(np.float64) + w[cb:cb + cbn]
    gain = np.float32(SPREAD / (Z - Z.mean(1, keepdims=True)).std())
    w[cw:cb + cbn] *= gain
    s["weights"].copy_(torch.from_numpy(w))
    s.update(w=w, W=w[ow:ob].reshape(rows, nf).copy(), b=w[ob:end].copy(), nf=nf)
    print("class boxes: %d candidates, class-head gain %.3g" % (len(X), float(gain)))
    return s


def _loop(F, s, scoring, frames=None, **kw):
    d = F.Detector(s["model"], scoring=scoring, **kw)
    return [_winner_rows(d.detect(f)) for f in (frames if frames is not None else s["frames"])]


def _recompute(F, s, feat, winners):
    """(r2 from frcnn_box_head_forward + frcnn_detect_post, deltas) for winners (dicts of a detection list) whose candidates index
    the rows of feat"""
    k = len(winners)
    cand = np.array([x["candidate"] - 1 for x in winners])
    cls = np.array([x["class"] for x in winners], np.int32)
    rect = np.array([[x["r"].minX, x["r"].minY, x["r"].maxX, x["r"].maxY] for x in winners], np.float64)
    # (the entry point on the MODEL'S weight tensors, where they lie in the flat vector: their alignment picks the 16-byte or the
    # one-float path of the row product, and with it the order of the sum)
    W_box, b_box = s["model"]["native"].box_head_parameters()
    x, c = F.DeviceTensor.from_numpy(np.ascontiguousarray(feat[cand])), F.DeviceTensor.from_numpy(cls)
    o, sel = F.DeviceTensor.empty((k, 4)), F.DeviceTensor.empty((k,), np.int32)
    F._lib.call("frcnn_box_head_forward", F.ptr(x), k, s["nf"], F.ptr(W_box), F.ptr(b_box), CLASSES, F.ptr(c), 1, k, None, 0, F.ptr(o),
                F.ptr(sel), F.stream_ptr())
    dl = o.numpy().copy()
    dev = [F.DeviceTensor.from_numpy(a) for a in (np.ones(k, np.int32), np.zeros(k, np.float32), dl, rect, np.arange(1, k + 1, dtype=np.int64))]
    out = [F.DeviceTensor.empty((k, 5)), F.DeviceTensor.empty((k,), np.int32), F.DeviceTensor.empty((k,), np.int32),
           F.DeviceTensor.empty((k, 4), np.float64), F.DeviceTensor.empty((1,), np.int32)]
    F._lib.call("frcnn_detect_post", *([F.ptr(t) for t in dev] + [k, 2, 0.5] + [F.ptr(t) for t in out] + [F.stream_ptr()]))
    return out[3].numpy().copy(), dl, rect


def _r2(winners):
    return np.array([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in winners], np.float64).reshape(-1, 4)


def test_all_at_one_half_is_top_at_one_half(F, setup):
    s = setup
    top = _loop(F, s, dict(classes="top", min_confidence=0.5))
    every = _loop(F, s, dict(classes="all", min_confidence=0.5, boxes="class"))
    assert every == top
    assert sum(len(w) for w in top) > 0, "no winner at one half: nothing is compared"
    d = F.Detector(s["model"], scoring=dict(classes="all", min_confidence=0.5, boxes="class"))
    assert [_winner_rows(w) for w in d.detect_batch(s["frames"])] == top


def test_every_detection_carries_the_box_of_its_class(F, setup):
    s = setup
    d = F.Detector(s["model"], scoring=ALL05)
    checked, shared_candidates = 0, 0
    for f in s["frames"]:
        win = list(d.detect(f))
        if not d.last_scan["n"]:
            assert win == []
            continue
        feat = _features(F, s["model"], len(d.last_pick))
        if not win:
            continue
        want, dl, rect = _recompute(F, s, feat, win)
        got = _r2(win)
        assert got.tobytes() == want.tobytes(), "r2 against box_head_forward + detect_post on the detection's own candidate"
        ref, bound = R.decode(rect, dl), R.decode_bound(rect, dl)
        assert got[:, :2].tobytes() == ref[:, :2].tobytes() and (np.abs(got - ref) <= bound).all(), "r2 against the restated decode"
        lp = np.asarray(d.last_cnet["cls"])
        for x in win:
            assert np.float32(x["confidence"]) == lp[x["candidate"] - 1, x["class"] - 1]
        checked += len(win)
        by_cand = {}
        for x, q in zip(win, got):
            by_cand.setdefault(x["candidate"], []).append((x["class"], q.tobytes()))
        shared_candidates += sum(len({c for c, _ in v}) >= 2 and len({q for _, q in v}) == len(v) for v in by_cand.values())
    print("class boxes: %d detections recomputed, %d candidates with two classes and different boxes" % (checked, shared_candidates))
    assert checked > 0 and shared_candidates >= 1


@pytest.mark.parametrize("case", ["plain", "mixed_sizes", "hflip", "box_voting"])
def test_detect_batch_equals_the_detect_loop(F, setup, case):
    s = setup
    frames, kw, bkw = s["frames"], {}, {}
    if case == "mixed_sizes":
        from test_gpu_box_head_model import H, W
        from test_gpu_soft_nms import SEEDS
        frames = [F.synthetic_image(h, w, k) for k, (h, w) in zip(SEEDS, [(H, W), (128, 192), (144, 176), (176, 128)] * 2)]
        bkw = dict(mixed_sizes=True)
    if case == "hflip":
        kw = dict(tta=dict(hflip=True))
    if case == "box_voting":
        kw = dict(box_voting=dict(overlap=0.5))
    want = _loop(F, s, ALL05, frames=frames, **kw)
    got = [_winner_rows(w) for w in F.Detector(s["model"], scoring=ALL05, **kw).detect_batch(frames, **bkw)]
    assert got == want
    assert sum(len(w) for w in want) > 0
    if case == "hflip":      # the mirrored view's per-class boxes are transformed like any others: they are not the plain run's
        assert want != _loop(F, s, ALL05, frames=frames)


def test_shared_cnet_rows_follow_from_the_shared_pass(F, setup):
    """the shared pass's features differ from detect()'s within the net's error, so every frame is judged against the shared
    pass's OWN features and outputs: the box of each detection recomputed from them, bit for bit"""
    s = setup
    d = F.Detector(s["model"], scoring=ALL05)
    res = d.detect_batch(s["frames"], shared_cnet=True)
    Rs = [len(rec["pick"]) if rec["n"] else 0 for rec in d.last_batch]
    feat = _features(F, s["model"], sum(Rs))          # (one pass over the chunk's candidates, frame after frame)
    off = np.concatenate([[0], np.cumsum(Rs)])
    checked = 0
    for b, (rec, win) in enumerate(zip(d.last_batch, res)):
        win = list(win)
        if not win:
            continue
        want, _, _ = _recompute(F, s, feat[off[b]:off[b + 1]], win)
        assert _r2(win).tobytes() == want.tobytes(), "frame %d" % b
        lp = np.asarray(rec["cnet"]["cls"])
        for x in win:
            assert np.float32(x["confidence"]) == lp[x["candidate"] - 1, x["class"] - 1]
        checked += len(win)
    assert checked > 0
    # and the loop's detections are the same up to that error: the same (frame, class, candidate) almost everywhere
    loop = _loop(F, s, ALL05)
    a = {(b, r[0], r[4]) for b, w in enumerate(loop) for r in w}
    print("shared_cnet: %d detections, %d of the loop's %d among them" % (checked, len(a & {(b, x["class"], x["candidate"])
                                                                                          for b, w in enumerate(res) for x in w}), len(a)))


def test_top_with_class_boxes_is_top(F, setup):
    s = setup
    got, want = {}, {}
    la1 = _launches(F, lambda: got.update(w=_loop(F, s, dict(classes="top", min_confidence=0.05, boxes="class"))))
    la0 = _launches(F, lambda: want.update(w=_loop(F, s, dict(classes="top", min_confidence=0.05))))
    assert got["w"] == want["w"] and sum(len(w) for w in want["w"]) > 0
    assert la1 == la0, "the same launches per kernel class"


def test_key_absent_allocates_and_launches_nothing_new(F, setup):
    s = setup
    frames = s["frames"]
    runs = {}

    def run(name, scoring):
        d = F.Detector(s["model"], scoring=scoring) if scoring is not None else F.Detector(s["model"])
        la = _launches(F, lambda: runs.update({name: [_winner_rows(w) for w in d.detect_batch(frames)]}))
        return d, la
    d0, la0 = run("absent", None)
    d1, la1 = run("candidate", dict(boxes="candidate"))
    d2, la2 = run("top", dict(classes="top", min_confidence=0.05))
    d3, la3 = run("all", ALL05)
    assert d0.boxes == "candidate" and d0.scoring is None
    for d in (d0, d1, d2):
        assert not any("feat" in k for k in d._bufs), "a feature buffer without the setting"
    assert any(k.endswith("feat") for k in d3._bufs)
    # the table {boxes = "candidate"} is the table {}: the key absent's results, from the one-launch class test
    assert runs["candidate"] == runs["absent"]
    # "all" with boxes = "class" runs the launches of the one-launch class test plus ONE per chunk (the feature copies are copies)
    chunks = -(-len(frames) // d3.BATCH)
    assert la3["elemwise"] - la2["elemwise"] == chunks, (la2, la3)
    assert dict(la3, elemwise=0) == dict(la2, elemwise=0)
    assert dict(la1, elemwise=0) == dict(la2, elemwise=0) and la1["elemwise"] == la2["elemwise"]
