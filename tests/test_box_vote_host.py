"""Box voting without a GPU: hand-worked cases of the restatement (tests/box_vote_ref.py), the derived error bound's shape, the
setting's validation (box_voting_settings, Detector.set_box_voting, Detector(model, box_voting=...)), evaluation at several IoU
thresholds (mean_average_precision_range), and static checks of the surfaces (ctypes row, export, Lua drop-in)."""
import os

import numpy as np
import pytest

import box_vote_ref as V
from test_abi import ROOT, _lua_code


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def _rows(boxes, scores):
    return np.concatenate([np.asarray(boxes, np.float32), np.asarray(scores, np.float32)[:, None]], 1)


def test_two_coincident_boxes_stay_where_they_are():
    rows = _rows([[0, 0, 9, 9], [0, 0, 9, 9]], [0.5, 0.25])
    for mode in (V.UNIFORM, V.SCORE, V.LOG_SCORE):
        out, votes, A = V.box_vote(rows, [1, 2], 0.5, 5, mode)
        assert votes.tolist() == [2, 2]
        assert out.tolist() == [[0, 0, 9, 9], [0, 0, 9, 9]]
        assert A[0].tolist() == [0, 0, 9, 9]


def test_weights_one_to_three_give_the_mean_one_can_write_down():
    """IoU = 80 / (100 + 100 - 80) = 2/3; weights 0.25 : 0.75 -> x1 = (0 * 1 + 2 * 3) / 4, x2 = (9 * 1 + 11 * 3) / 4"""
    rows = _rows([[0, 0, 9, 9], [2, 0, 11, 9]], [0.25, 0.75])
    out, votes, _ = V.box_vote(rows, [1], 0.5, 5, V.SCORE)
    assert votes.tolist() == [2] and out.tolist() == [[1.5, 0.0, 10.5, 9.0]]
    out, votes, _ = V.box_vote(rows, [2, 1], 0.5, 5, V.UNIFORM)
    assert votes.tolist() == [2, 2] and out.tolist() == [[1.0, 0.0, 10.0, 9.0]] * 2
    # log-scores: the weights are their exps -- log(0.25) and log(0.75) give 1 : 3 again, within exp's rounding
    logs = _rows(rows[:, :4], np.log(np.array([0.25, 0.75])))
    out, votes, A = V.box_vote(logs, [1], 0.5, 5, V.LOG_SCORE)
    assert votes.tolist() == [2]
    assert np.all(np.abs(out[0] - [1.5, 0.0, 10.5, 9.0]) <= 1e-6)      # (the fp32 logs, not exp's rounding, set this distance)
    # at a threshold above 2/3 nothing but the winner votes, and it keeps its box
    out, votes, A = V.box_vote(rows, [1, 2], 0.7, 5, V.SCORE)
    assert votes.tolist() == [1, 1] and out.tolist() == rows[:, :4].tolist() and not A.any()


def test_disjoint_boxes_are_unchanged():
    rows = _rows([[0, 0, 9, 9], [20, 20, 29, 29], [40, 0, 49, 9]], [0.9, 0.8, 0.7])
    rect = rows[:, :4].astype(np.float64) + 2.0 ** -30         # fp64 rects that are not the fp32 boxes
    out, votes, _ = V.box_vote(rows, [3, 1, 2], 0.5, 5, V.SCORE, rect=rect)
    assert votes.tolist() == [1, 1, 1]
    assert out.tobytes() == rect[[2, 0, 1]].tobytes()


def test_two_classes_never_mix():
    rows = _rows([[0, 0, 9, 9], [0, 0, 9, 9], [2, 0, 11, 9], [2, 0, 11, 9]], [0.5, 0.5, 0.5, 0.5])
    out, votes, _ = V.box_vote(rows, [1, 2], 0.5, 5, V.SCORE, cls=[1, 2, 2, 1])
    assert votes.tolist() == [2, 2]
    assert out.tolist() == [[1.0, 0.0, 10.0, 9.0], [1.0, 0.0, 10.0, 9.0]]
    out, votes, _ = V.box_vote(rows, [1, 2, 3, 4], 0.5, 5, V.SCORE, cls=[1, 2, 3, 4])
    assert votes.tolist() == [1, 1, 1, 1] and out.tolist() == rows[:, :4].tolist()
    out, votes, _ = V.box_vote(rows, [1], 0.5, 5, V.SCORE)
    assert votes.tolist() == [4]


def test_a_pair_at_exactly_the_threshold_votes():
    """[0,0,9,9] and [0,0,9,4]: intersection 50, union 100 + 50 - 50 -> IoU = 0.5 exactly, and >= includes it"""
    rows = _rows([[0, 0, 9, 9], [0, 0, 9, 4]], [0.5, 0.5])
    out, votes, _ = V.box_vote(rows, [1, 2], 0.5, 5, V.SCORE)
    assert votes.tolist() == [2, 2] and out.tolist() == [[0.0, 0.0, 9.0, 6.5]] * 2
    out, votes, _ = V.box_vote(rows, [1, 2], np.nextafter(np.float32(0.5), np.float32(1)), 5, V.SCORE)
    assert votes.tolist() == [1, 1] and out.tolist() == rows[:, :4].tolist()


def test_rows_without_a_positive_finite_weight_do_not_vote():
    boxes = [[0, 0, 9, 9]] * 6
    rows = _rows(boxes, [0.5, 0.0, -1.0, np.inf, np.nan, 0.25])
    rect = np.array([[0, 0, 9, 9], [100, 0, 0, 0], [200, 0, 0, 0], [300, 0, 0, 0], [400, 0, 0, 0], [4, 0, 9, 9]], np.float64)
    out, votes, _ = V.box_vote(rows, [1, 2], 0.5, 5, V.SCORE, rect=rect)
    assert votes.tolist() == [2, 2]                           # rows 1 and 6, also for the winner that does not vote itself
    assert out[0].tolist() == [(0 * 0.5 + 4 * 0.25) / 0.75, 0.0, 9.0, 9.0] and out[1].tolist() == out[0].tolist()
    out, votes, _ = V.box_vote(_rows(boxes, [0.0] * 6), [1, 4], 0.5, 5, V.SCORE, rect=rect)
    assert votes.tolist() == [0, 0] and out.tolist() == rect[[0, 3]].tolist()
    # a lone voter that is not the winner does not move it
    out, votes, _ = V.box_vote(_rows(boxes[:2], [0.0, 0.5]), [1], 0.5, 5, V.SCORE, rect=rect[:2])
    assert votes.tolist() == [1] and out.tolist() == rect[[0]].tolist()
    # uniform weights never look at the score column; log-scores: exp(-inf) = 0 does not vote, exp(nan) neither
    out, votes, _ = V.box_vote(rows, [1], 0.5, 5, V.UNIFORM)
    assert votes.tolist() == [6]
    out, votes, _ = V.box_vote(_rows(boxes[:4], [-1.0, -np.inf, np.nan, 800.0]), [1], 0.5, 5, V.LOG_SCORE)
    assert votes.tolist() == [1]


def test_error_bound_is_linear_in_the_voters_and_scales_with_the_coordinates():
    u = 2.0 ** -53
    assert V.rect_error_bound(0, 5.0, V.SCORE) == V.rect_error_bound(1, 5.0, V.LOG_SCORE) == 0.0
    for mode, extra in ((V.UNIFORM, 0), (V.SCORE, 0), (V.LOG_SCORE, 8)):
        for k in (2, 12, 2048):
            assert V.rect_error_bound(k, 3.0, mode) == (2 * k + 1 + extra) * u * 3.0 * (1 + 2.0 ** -10)
        assert V.rect_error_bound(7, 2000.0, mode) == 2000.0 * V.rect_error_bound(7, 1.0, mode)
    # far below anything a wrong vote would cause: half a pixel over a dozen voters is 13 orders of magnitude away
    assert V.rect_error_bound(12, 2048.0, V.LOG_SCORE) < 1e-11


def test_restatement_is_permutation_invariant_and_picks_keep_their_order():
    from soft_nms_ref import clustered_boxes, grid_scores, rows5
    rng = np.random.RandomState(3)
    n = 150
    rows = rows5(clustered_boxes(rng, n), grid_scores(rng, n, 0.05, 1.0))
    cls = rng.randint(1, 4, n).astype(np.int32)
    picks = rng.permutation(n)[:40] + 1
    out, votes, A = V.box_vote(rows, picks, 0.2, 5, V.SCORE, cls)      # (0.2: clusters of several voters)
    assert votes.max() > 2 and votes.min() >= 1
    perm = rng.permutation(n)
    inv = np.argsort(perm)
    out2, votes2, _ = V.box_vote(rows[perm], inv[picks - 1] + 1, 0.2, 5, V.SCORE, cls[perm])
    assert np.array_equal(votes, votes2) and out.tobytes() == out2.tobytes()      # (the means are exact, then rounded once)
    lo = np.minimum.reduce([rows[:, t].min() for t in range(4)])
    many = votes > 1
    assert np.all(out >= lo) and np.all(A[many] >= np.abs(out[many]) * (1 - 1e-15)) and not A[~many].any()


# ------------------------------------------------------------------------------------------------ the setting
def _settings():
    from frcnn_amd.Detector import box_voting_settings
    return box_voting_settings


def test_box_voting_settings_defaults_and_accepted_tables():
    bs = _settings()
    assert bs(None) is None and bs(dict(class_count=16)) is None and bs(dict(class_count=16, box_voting=None)) is None
    assert bs({}) == (0.5, "score") == bs(dict(class_count=16, box_voting={}))
    assert bs(dict(overlap=0.7)) == (0.7, "score")
    assert bs(dict(weight="uniform")) == (0.5, "uniform")
    assert bs(dict(box_voting=dict(overlap=1, weight="score"), class_count=16)) == (1.0, "score")
    assert bs(dict(overlap=np.float32(0.25))) == (0.25, "score")


@pytest.mark.parametrize("table", [
    dict(overlaps=0.5), dict(overlap=0.5, sigma=0.5), dict(weight="log_score"), dict(weight="scores"), dict(weight=1), dict(weight=None),
    dict(weight=True), dict(overlap=True), dict(overlap="0.5"), dict(overlap=None), dict(overlap=[0.5]),
    dict(overlap=0), dict(overlap=0.0), dict(overlap=-0.5), dict(overlap=1.01), dict(overlap=float("nan")), dict(overlap=float("inf")),
    "score", 0.5, ["score"], True,
])
def test_box_voting_settings_rejects(table):
    with pytest.raises(ValueError):
        _settings()(table)
    if isinstance(table, dict):
        with pytest.raises(ValueError):
            _settings()(dict(class_count=16, box_voting=table))


def test_detector_takes_the_setting_from_the_argument_or_the_cfg():
    """set_box_voting is host code, validated before any device call; the class call takes the keyword beside an unchanged
    __init__"""
    import inspect
    from frcnn_amd.Detector import Detector
    d = Detector.__new__(Detector)
    d.set_box_voting(dict(class_count=16))
    assert d.box_voting is None
    d.set_box_voting(dict(class_count=16, box_voting=dict(overlap=0.6)))
    assert d.box_voting == (0.6, "score")
    with pytest.raises(ValueError):
        d.set_box_voting(dict(weight="best"))
    assert d.box_voting == (0.6, "score")
    d.set_box_voting(None)
    assert d.box_voting is None
    assert Detector.box_voting_settings(dict(weight="uniform")) == (0.5, "uniform")
    for bad in (dict(weight="best"), dict(overlap=0), "score"):
        with pytest.raises(ValueError):
            Detector(None, box_voting=bad)          # refused before the model is looked at
    assert list(inspect.signature(Detector.__init__).parameters)[1:] == ["model", "static_weights", "proposals", "nms"]


def test_surfaces_name_the_entry_point():
    import frcnn_amd as F
    assert callable(F.box_vote) and "box_vote" in F.__all__ and "mean_average_precision_range" in F.__all__
    assert "frcnn_box_vote_batch" in F._lib.exported_symbols()
    assert "box_vote" not in F._lib.KC_NAMES, "counted under nms: no new kernel class"
    with pytest.raises(ValueError):
        F.box_vote(np.zeros((2, 5), np.float32), [1], weights="best")
    r, v = F.box_vote(np.zeros((0, 5), np.float32), [])
    assert r.shape == (0, 4) and r.dtype == np.float64 and v.shape == (0,) and v.dtype == np.int32
    src = open(os.path.join(ROOT, "build_lib.sh")).read()
    assert src.count("box_vote") == 2, "box_vote.hip belongs to both source lists of build_lib.sh"
    det = _lua_code(open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read())
    assert "C.frcnn_box_vote_batch(" in det and "function Detector.box_voting_settings" in det and "cfg.box_voting" in det
    # the drop-in votes between the per-class pass and the gather, and the gather reads the voted rects
    a, b, c = det.index("C.frcnn_nms_device_batch(dbb"), det.index("C.frcnn_box_vote_batch("), det.index("C.frcnn_detect_gather_batch(")
    assert a < b < c
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    assert "function M.box_vote(" in shim and "box_vote = M.box_vote" in shim


# ------------------------------------------------------------------------------------------------ evaluation
def _scene():
    """one class, two images; ground truth 10 x 10 boxes; detections at IoU 1, 0.6 (exactly: 6 of 10 columns), and a miss"""
    from frcnn_amd.Rect import Rect
    gt = [(0, 1, Rect(0, 0, 10, 10)), (1, 1, Rect(0, 0, 10, 10)), (1, 1, Rect(50, 50, 60, 60))]
    det = [(0, 1, 0.9, Rect(0, 0, 10, 10)),          # IoU 1
           (1, 1, 0.8, Rect(2.5, 0, 12.5, 10)),      # IoU 75 / 125 = 0.6
           (1, 1, 0.7, Rect(80, 80, 90, 90))]        # IoU 0
    return det, gt


def test_mean_average_precision_range():
    from frcnn_amd.Rect import Rect
    from frcnn_amd.evaluation import IOU_RANGE, mean_average_precision, mean_average_precision_range
    det, gt = _scene()
    assert Rect.IoU(det[1][3], gt[1][2]) == 0.6
    assert IOU_RANGE == (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)
    res = mean_average_precision_range(det, gt)
    assert sorted(res) == ["by_iou", "mAP"] and tuple(res["by_iou"]) == IOU_RANGE
    for t in IOU_RANGE:
        assert res["by_iou"][t] == mean_average_precision(det, gt, t)
    # the detection at IoU 0.6 counts at 0.5, 0.55 and 0.6 and not above: 2 of 3 recalled at full precision, then 1 of 3
    for t in (0.5, 0.55, 0.6):
        assert res["by_iou"][t]["tp"] == 2 and res["by_iou"][t]["fp"] == 1 and res["by_iou"][t]["mAP"] == pytest.approx(2 / 3.0)
    for t in IOU_RANGE[3:]:
        assert res["by_iou"][t]["tp"] == 1 and res["by_iou"][t]["fp"] == 2 and res["by_iou"][t]["mAP"] == pytest.approx(1 / 3.0)
    assert res["mAP"] == pytest.approx((3 * (2 / 3.0) + 7 * (1 / 3.0)) / 10)
    two = mean_average_precision_range(det, gt, (0.5, 0.75), use_07_metric=True)
    assert tuple(two["by_iou"]) == (0.5, 0.75)
    assert two["by_iou"][0.75] == mean_average_precision(det, gt, 0.75, use_07_metric=True)
    assert two["mAP"] == pytest.approx((two["by_iou"][0.5]["mAP"] + two["by_iou"][0.75]["mAP"]) / 2)
    with pytest.raises(ValueError):
        mean_average_precision_range(det, gt, ())


class _FakeDetector(object):
    def __init__(self, per_image):
        self.per_image, self.i = per_image, 0

    def detect(self, img):
        out = self.per_image[self.i]
        self.i += 1
        return out

    def detect_batch(self, imgs):
        return [self.detect(i) for i in imgs]


class _FakeIterator(object):
    def __init__(self, items):
        self.items, self.i = items, 0

    def nextValidation(self, n):
        x = self.items[self.i % len(self.items)]
        self.i += 1
        return [x]


class _Roi(object):
    def __init__(self, rect, class_index):
        self.rect, self.class_index = rect, class_index


def test_evaluate_detections_routes_a_sequence_and_leaves_a_scalar_alone():
    from frcnn_amd.evaluation import evaluate_detections, mean_average_precision, mean_average_precision_range
    det, gt = _scene()
    img = np.zeros((3, 8, 8), np.float32)
    items = [dict(img=img, rois=[_Roi(g[2], g[1]) for g in gt if g[0] == i]) for i in (0, 1)]
    per_image = [[{"class": d[1], "confidence": d[2], "r2": d[3]} for d in det if d[0] == i] for i in (0, 1)]

    def run(**kw):
        return evaluate_detections(_FakeDetector(per_image), _FakeIterator(items), 2, **kw)
    counts = dict(images=2, detections=3, ground_truth=3)
    assert run() == dict(mean_average_precision(det, gt, 0.5), **counts)                       # the scalar form, as it was
    assert run(iou_threshold=0.75) == dict(mean_average_precision(det, gt, 0.75), **counts)
    for seq in ((0.5, 0.75), [0.5, 0.75], np.array([0.5, 0.75])):
        assert run(iou_threshold=seq) == dict(mean_average_precision_range(det, gt, (0.5, 0.75)), **counts)
    assert run(iou_threshold=(0.5, 0.75), batch=2) == run(iou_threshold=(0.5, 0.75))
