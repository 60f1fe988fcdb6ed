"""What the ragged anchor scan and its callers need that runs without a GPU: the input conditions of the problems in
tests/scan_ragged_cases.py (which tests/test_gpu_detect_mixed.py runs on the device), the host-only workspace size of
frcnn_rpn_scan_ragged, and the mixed_sizes keyword of evaluate_detections with a fake detector."""
import ctypes as C

import numpy as np

import anchor_ops_ref as ref
import scan_ragged_cases as cases


def test_every_frame_decides_far_from_its_thresholds():
    """no anchor of any frame within MARGIN of the p threshold or of an image border: every correct fp64 evaluation agrees on
    the matches, nothing is left out of a comparison"""
    for c in cases.frames() + cases.one_size_frames():
        w = c["want"]
        what = "%s/%s %gx%g" % (c["name"], c["pattern"], c["img_w"], c["img_h"])
        assert w["total"] == c["total"] == cases.total(c["name"]), what
        assert w["thr_margin"].min() >= ref.MARGIN, what
        assert w["ovl_margin"].min() >= ref.MARGIN, what


def test_the_set_covers_the_sizes_and_the_outcomes():
    fr = cases.frames()
    assert sorted(set(c["total"] for c in fr)) == [12, 72, 1026, 1287, 2490]
    assert any(c["want"]["count"] == 0 for c in fr), "no empty frame"
    assert any(c["want"]["count"] == c["total"] for c in fr), "no full frame"
    both = 0
    for c in fr:
        w = c["want"]
        over = np.isfinite(w["ovl_margin"][:, 0])          # the anchors that passed the threshold test
        if (over & w["match"]).any() and (over & ~w["match"]).any():
            both += 1
    assert both > 0, "no frame with both outcomes of the overlap test"
    # every frame has its own image size beside its own map sizes; the tables' last row is read (H = 200 and W = 200)
    assert len(set((c["img_w"], c["img_h"]) for c in fr)) >= 4
    assert any(200 in c["H"] and 200 in c["W"] for c in fr)
    # the calls of the GPU test
    b3 = cases.frames(cases.CALL_B3)
    assert b3[1]["total"] == max(c["total"] for c in fr) and len(set(c["total"] for c in b3)) == 3
    assert len(cases.CALL_B17) == 17 and max(c["total"] for c in cases.frames(cases.CALL_B17)) <= 1026
    tr = cases.frames(cases.CALL_TRUNCATED)
    assert tr[1]["pattern"] == "all" and tr[1]["want"]["count"] == tr[1]["total"] > 5 and tr[0]["want"]["count"] > 5
    one = cases.one_size_frames()
    assert len(set((tuple(c["H"]), tuple(c["W"]), c["img_w"], c["img_h"]) for c in one)) == 1


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def test_ragged_workspace_bytes(F):
    """one slice per frame, sized by the frame's own anchors: B frames of one size -> the batch form's bytes, B = 1 -> the
    single frame's; mixed frames -> the sum of their single-frame slices behind one 256-byte head"""
    L = F._lib.load()
    fr = cases.frames()
    single = []
    for c in fr:
        Hs, Ws = _ints(c["H"]), _ints(c["W"])
        one = L.frcnn_rpn_scan_workspace_bytes(Hs, Ws)
        assert L.frcnn_rpn_scan_ragged_workspace_bytes(Hs, Ws, 1) == one
        for B in (2, 3, 8, 17):
            assert L.frcnn_rpn_scan_ragged_workspace_bytes(_ints(c["H"] * B), _ints(c["W"] * B), B) \
                == L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B), (c["name"], B)
        single.append(one)
    Hs = _ints([h for c in fr for h in c["H"]])
    Ws = _ints([w for c in fr for w in c["W"]])
    assert L.frcnn_rpn_scan_ragged_workspace_bytes(Hs, Ws, len(fr)) == 256 + sum(s - 256 for s in single)
    assert L.frcnn_rpn_scan_ragged_workspace_bytes(Hs, Ws, 0) == 256


# ------------------------------------------------------------------------------------------------ evaluate_detections
class _Img(object):
    def __init__(self, shape):
        self.shape = shape


class _Iter(object):
    def __init__(self, shapes):
        self.shapes, self.i = shapes, 0

    def nextValidation(self, count=1):
        out = []
        for _ in range(count):
            out.append(dict(img=_Img(self.shapes[self.i % len(self.shapes)]), rois=[]))
            self.i += 1
        return out


class _FakeDetector(object):
    def __init__(self):
        self.calls = []

    def detect_batch(self, frames, **kw):
        frames = list(frames)
        self.calls.append(([f.shape for f in frames], kw))
        return [[] for _ in frames]

    def detect(self, frame):
        raise AssertionError("batch > 1 goes through detect_batch")


def test_evaluate_detections_mixed_sizes():
    from frcnn_amd.evaluation import evaluate_detections
    a, b, c = (3, 128, 176), (3, 128, 192), (3, 176, 128)
    shapes = [a, b, c, c, a, a, b]
    d = _FakeDetector()
    res = evaluate_detections(d, _Iter(shapes), 7, batch=3, mixed_sizes=True)
    assert res["images"] == 7
    assert [s for s, _ in d.calls] == [[a, b, c], [c, a, a], [b]]
    assert all(kw == dict(mixed_sizes=True) for _, kw in d.calls)
    # the default: a chunk ends where the size changes, and detect_batch is called as it always was
    d = _FakeDetector()
    evaluate_detections(d, _Iter(shapes), 7, batch=3)
    assert [s for s, _ in d.calls] == [[a], [b], [c, c], [a, a], [b]]
    assert all(kw == {} for _, kw in d.calls)
