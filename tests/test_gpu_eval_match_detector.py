"""Detector.match_batch and evaluate_detections(match="device") on the tiny per-class model and frames of
tests/test_gpu_box_head_model.py (its fixture, imported).  Ground truth is made from the detector's own winners -- some boxes copied,
some moved by 15 % of their width (at least two pixels), some given the wrong class, some left out -- so that there are true and
false positives at 0.5 and fewer true positives at 0.9.
  (a) row k of match_batch carries the class and confidence of detect_batch's detection k, and its mask, box and overlap are the
      restatement's (tests/eval_match_ref.py: the greedy loop) fed with detect_batch's own lists -- under the defaults, "all" at
      0.05 with max_detections, Soft-NMS, box voting, a mirrored view, mixed sizes, a shared classification-net pass, per-class boxes, and candidate
      boxes on the shared-head model
  (b) evaluate_detections(match="device") == match="host", one threshold and the range, batch 1 and 8
  (c) a plain detect_batch before and after launches and returns what it did; the path costs two launches a chunk
Without the feature every test here fails on the missing method."""
import numpy as np
import pytest

import eval_match_ref as R
from test_gpu_box_head_model import CLASSES, H, W, detector_setup, head      # noqa: F401  (detector_setup: a fixture)
from test_gpu_detect_batch import _winner_rows
from test_gpu_proposals import _launches

pytestmark = pytest.mark.gpu

ALL05 = dict(classes="all", min_confidence=0.05, boxes="class")
SETTINGS = {
    "defaults": (dict(), dict()),
    "all_005_max_detections": (dict(scoring=dict(ALL05, max_detections=12)), dict()),
    "soft_nms": (dict(scoring=ALL05, nms=dict(method="linear")), dict()),
    "box_voting": (dict(scoring=ALL05, box_voting=dict(overlap=0.5)), dict()),
    "hflip": (dict(scoring=ALL05, tta=dict(hflip=True)), dict()),
    "mixed_sizes": (dict(scoring=ALL05), dict(mixed_sizes=True)),
    "shared_cnet": (dict(scoring=ALL05), dict(shared_cnet=True)),
    "class_boxes": (dict(scoring=ALL05), dict()),
    "candidate_boxes": (dict(scoring=dict(classes="all", min_confidence=0.05)), dict()),      # on the shared-head model
}
THR = [0.5, 0.75, 0.9]


def _ground_truth(F, winners):
    """a frame's boxes from its detections: detection k is copied (k % 4 == 0), moved (1), given the next class (2) or left out (3)"""
    out = []
    for k, x in enumerate(winners):
        r, c = x["r2"], int(x["class"])
        if k % 4 == 0:
            out.append((c, F.Rect(r.minX, r.minY, r.maxX, r.maxY)))
        elif k % 4 == 1:
            d = max(2.0, 0.15 * (r.maxX - r.minX))
            out.append((c, F.Rect(r.minX + d, r.minY, r.maxX + d, r.maxY)))
        elif k % 4 == 2:
            out.append((c % CLASSES + 1, F.Rect(r.minX, r.minY, r.maxX, r.maxY)))
    return out


def _frames_of(F, s, name):
    if name != "mixed_sizes":
        return s["frames"]
    from test_gpu_soft_nms import SEEDS
    return [F.synthetic_image(h, w, k) for k, (h, w) in zip(SEEDS, [(H, W), (128, 192), (144, 176), (176, 128)] * 2)]


def _shared_model(F, s):
    """detector_setup's shared-head model with the per-class model's weights: the shared box head gets class 1's four rows"""
    import torch
    ow, ob, end, nf, rows = head(s["model"]["native"])
    w = s["w"]
    s["sw"].copy_(torch.from_numpy(np.concatenate([w[:ow], w[ow:ow + 4 * nf], w[ob:ob + 4], w[end:]])))
    return s["shared"]


def _arrays(winners, boxes):
    return dict(rects=np.array([[x["r2"].minX, x["r2"].minY, x["r2"].maxX, x["r2"].maxY] for x in winners], np.float64).reshape(-1, 4),
                classes=np.array([x["class"] for x in winners], np.int32), conf=np.array([x["confidence"] for x in winners], np.float32),
                gt_rects=np.array([[r.minX, r.minY, r.maxX, r.maxY] for _, r in boxes], np.float64).reshape(-1, 4),
                gt_classes=np.array([c for c, _ in boxes], np.int32))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_match_batch_is_the_restatement_on_detect_batchs_lists(F, detector_setup, name):
    s = detector_setup
    kw, bkw = SETTINGS[name]
    frames = _frames_of(F, s, name)
    d = F.Detector(_shared_model(F, s) if name == "candidate_boxes" else s["model"], **kw)
    lists = [list(w) for w in d.detect_batch(frames, **bkw)]
    rows_before = [_winner_rows(w) for w in lists]
    gts = [_ground_truth(F, w) for w in lists]
    got = d.match_batch(frames, gts, THR, with_iou=True, **bkw)
    assert len(got) == len(frames) == len(d.last_batch)
    tp5 = fp5 = tp9 = 0
    for f, (w, m, boxes) in enumerate(zip(lists, got, gts)):
        tag = "%s frame %d" % (name, f)
        assert m["cls"].tolist() == [x["class"] for x in w], tag
        assert m["confidence"].dtype == np.float32 and m["tp"].dtype == np.uint32
        assert m["confidence"].tobytes() == np.array([x["confidence"] for x in w], np.float32).tobytes(), tag
        a = _arrays(w, boxes)
        want = R.match_frame(a["rects"], a["classes"], a["conf"], a["gt_rects"], a["gt_classes"], THR)
        assert m["tp"].tolist() == want["tp"].tolist() and m["gt"].tolist() == want["gt"].tolist(), tag
        assert m["iou"].tobytes() == want["iou"].tobytes(), tag
        tp5 += int((want["tp"] & 1).sum()); fp5 += int(len(w) - (want["tp"] & 1).sum()); tp9 += int((want["tp"] >> 2 & 1).sum())
    print("%s: %d detections, %d boxes; at 0.5 %d true and %d false positives, at 0.9 %d true" %
          (name, sum(len(w) for w in lists), sum(len(g) for g in gts), tp5, fp5, tp9))
    assert tp5 > 0 and fp5 > 0 and 0 < tp9 < tp5
    # without the overlaps: the same arrays, and no iou; the Detector's lists did not change under the match
    plain = d.match_batch(frames, gts, THR, **bkw)
    for m, p in zip(got, plain):
        assert "iou" not in p and all(m[k].tobytes() == p[k].tobytes() for k in ("cls", "confidence", "tp", "gt"))
    assert [_winner_rows(w) for w in d.detect_batch(frames, **bkw)] == rows_before


def test_max_detections_changes_who_claims_a_box(F, detector_setup):
    """the selection happens before the match, as on the host: with the cap the rows are keep_best's, and a box whose best
    detection was cut goes to the next one"""
    s = detector_setup
    free = F.Detector(s["model"], scoring=ALL05)
    lists = [list(w) for w in free.detect_batch(s["frames"])]
    gts = [_ground_truth(F, w) for w in lists]
    M = max(2, min(len(w) for w in lists if len(w)) // 2)
    capped = F.Detector(s["model"], scoring=dict(ALL05, max_detections=M))
    got = capped.match_batch(s["frames"], gts, [0.5])
    cut = 0
    for w, m, boxes in zip(lists, got, gts):
        a = _arrays(w, boxes)
        keep = R.keep_best(a["conf"], M)
        keep = keep[np.argsort(a["classes"][keep], kind="stable")]
        assert m["cls"].tolist() == a["classes"][keep].tolist() and m["confidence"].tobytes() == a["conf"][keep].tobytes()
        want = R.match_frame(a["rects"][keep], a["classes"][keep], a["conf"][keep], a["gt_rects"], a["gt_classes"], [0.5])
        assert m["tp"].tolist() == want["tp"].tolist() and m["gt"].tolist() == want["gt"].tolist()
        cut += len(w) - len(keep)
    assert cut > 0


class _Validation(object):
    """nextValidation(n) over given frames and boxes, round and round"""

    def __init__(self, F, frames, gts):
        self.items = [dict(img=f, rois=[F.Roi(r, c) for c, r in g]) for f, g in zip(frames, gts)]
        self.at = 0

    def nextValidation(self, n):
        out = [self.items[(self.at + i) % len(self.items)] for i in range(n)]
        self.at += n
        return out


@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("thr", [0.5, tuple(R.IOU_RANGE)], ids=["one", "range"])
def test_evaluate_detections_on_the_device_equals_the_host(F, detector_setup, batch, thr):
    s = detector_setup
    d = F.Detector(s["model"], scoring=ALL05)
    gts = [_ground_truth(F, list(w)) for w in d.detect_batch(s["frames"])]
    n = len(s["frames"])
    host = F.evaluate_detections(d, _Validation(F, s["frames"], gts), n, iou_threshold=thr, batch=batch)
    dev = F.evaluate_detections(d, _Validation(F, s["frames"], gts), n, iou_threshold=thr, batch=batch, match="device")
    assert dev == host
    first = host["by_iou"][0.5] if isinstance(thr, tuple) else host
    assert first["tp"] > 0 and first["fp"] > 0 and host["detections"] > 0 and 0.0 < host["mAP"] < 1.0


def test_mixed_sizes_through_evaluate_detections(F, detector_setup):
    s = detector_setup
    frames = _frames_of(F, s, "mixed_sizes")
    d = F.Detector(s["model"], scoring=ALL05)
    gts = [_ground_truth(F, list(w)) for w in d.detect_batch(frames, mixed_sizes=True)]
    for kw in (dict(batch=8, mixed_sizes=True), dict(batch=8), dict(batch=1)):
        host = F.evaluate_detections(d, _Validation(F, frames, gts), len(frames), iou_threshold=0.5, **kw)
        dev = F.evaluate_detections(d, _Validation(F, frames, gts), len(frames), iou_threshold=0.5, match="device", **kw)
        assert dev == host and host["tp"] > 0, kw


def test_frames_without_detections_or_ground_truth(F, detector_setup):
    s = detector_setup
    d = F.Detector(s["model"])
    blank = np.zeros((3, H, W), np.float32)
    frames = [blank, s["frames"][0], blank]
    lists = d.detect_batch(frames)
    got = d.match_batch(frames, [[(CLASSES + 5, F.Rect(0, 0, 10, 10))], [], []], [0.5], with_iou=True)     # (a class nobody detects)
    for w, m in zip(lists, got):
        assert len(m["cls"]) == len(w) and not m["tp"].any() and not m["gt"].any() and (m["iou"] == -1.0).all()
    assert len(lists[1]) > 0
    only = d.match_batch([blank], [[]])
    assert sorted(only[0]) == ["cls", "confidence", "gt", "tp"] and [len(v) for v in only[0].values()] == [len(lists[0])] * 4


def test_detect_batch_before_and_after_is_untouched(F, detector_setup):
    s = detector_setup
    frames = s["frames"]
    d = F.Detector(s["model"], scoring=ALL05)
    runs = {}
    la0 = _launches(F, lambda: runs.update(before=[_winner_rows(w) for w in d.detect_batch(frames)]))
    bufs0 = set(d._bufs)
    gts = [_ground_truth(F, list(w)) for w in d.detect_batch(frames)]
    lam = _launches(F, lambda: runs.update(match=d.match_batch(frames, gts, THR)))
    la1 = _launches(F, lambda: runs.update(after=[_winner_rows(w) for w in d.detect_batch(frames)]))
    assert runs["after"] == runs["before"] and sum(len(w) for w in runs["before"]) > 0
    assert la1 == la0, "the same launches per kernel class"
    assert not any("eval_" in k or "gt_" in k for k in bufs0), "a match buffer without the call"
    assert any("eval_match" in k for k in d._bufs)
    chunks = -(-len(frames) // d.BATCH)
    # the path costs two launches a chunk, counted with the NMS kernels; everything else is detect_batch's
    assert lam["nms"] - la0["nms"] == 2 * chunks and dict(lam, nms=0) == dict(la0, nms=0), (la0, lam)
    capped = F.Detector(s["model"], scoring=dict(ALL05, max_detections=5))
    lac = _launches(F, lambda: capped.match_batch(frames, gts, THR))
    assert lac["nms"] - la0["nms"] == 3 * chunks and lac["topk"] - la0["topk"] == chunks, (la0, lac)
