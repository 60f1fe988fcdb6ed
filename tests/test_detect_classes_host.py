"""The class test under cfg.scoring without a GPU: the setting's validation (scoring_settings, Detector.set_scoring,
Detector(model, scoring=...)), the restatement's properties (tests/detect_classes_ref.py), the input conditions of the problems
tests/test_gpu_detect_classes.py runs, max_detections' rule and static checks of the surfaces."""
import os

import numpy as np
import pytest

import detect_classes_ref as D
from test_abi import ROOT, _lua_code


# ------------------------------------------------------------------------------------------------ the setting
def _settings():
    from frcnn_amd.Detector import scoring_settings
    return scoring_settings


def test_scoring_settings_defaults_and_accepted_tables():
    ss = _settings()
    assert ss(None) is None and ss(dict(class_count=16)) is None and ss(dict(class_count=16, scoring=None)) is None
    assert ss({}) == ("top", 0.2, None) == ss(dict(class_count=16, scoring={}))
    assert ss(dict(classes="all")) == ("all", 0.2, None)
    assert ss(dict(classes="all", min_confidence=0.05, max_detections=100)) == ("all", 0.05, 100)
    assert ss(dict(min_confidence=0)) == ("top", 0.0, None)
    assert ss(dict(min_confidence=np.float32(0.5), max_detections=np.int64(1))) == ("top", 0.5, 1)
    assert ss(dict(max_detections=None)) == ("top", 0.2, None)
    assert ss(dict(scoring=dict(classes="top", min_confidence=0.99), class_count=16)) == ("top", 0.99, None)


@pytest.mark.parametrize("table", [
    dict(class_="all"), dict(classes="all", overlap=0.5), dict(classes="every"), dict(classes="ALL"), dict(classes=1), dict(classes=None),
    dict(classes=True), dict(min_confidence=True), dict(min_confidence="0.2"), dict(min_confidence=None), dict(min_confidence=[0.2]),
    dict(min_confidence=-0.1), dict(min_confidence=1), dict(min_confidence=1.0), dict(min_confidence=1.5),
    dict(min_confidence=float("nan")), dict(min_confidence=float("inf")),
    dict(max_detections=0), dict(max_detections=-3), dict(max_detections=2.0), dict(max_detections=2.5), dict(max_detections=True),
    dict(max_detections="10"), dict(max_detections=[10]),
    "all", 0.2, ["all"], True,
])
def test_scoring_settings_rejects(table):
    with pytest.raises(ValueError):
        _settings()(table)
    if isinstance(table, dict):
        with pytest.raises(ValueError):
            _settings()(dict(class_count=16, scoring=table))


def test_detector_takes_the_setting_from_the_argument_or_the_cfg():
    """set_scoring is host code, validated before any device call; the class call takes the keyword beside an unchanged __init__"""
    import inspect
    from frcnn_amd.Detector import Detector
    d = Detector.__new__(Detector)
    d.set_scoring(dict(class_count=16))
    assert d.scoring is None
    d.set_scoring(dict(class_count=16, scoring=dict(classes="all")))
    assert d.scoring == ("all", 0.2, None)
    with pytest.raises(ValueError):
        d.set_scoring(dict(classes="best"))
    assert d.scoring == ("all", 0.2, None)
    d.set_scoring(None)
    assert d.scoring is None
    assert Detector.scoring_settings(dict(min_confidence=0.05)) == ("top", 0.05, None)
    for bad in (dict(classes="best"), dict(min_confidence=1), dict(max_detections=0), "all"):
        with pytest.raises(ValueError):
            Detector(None, scoring=bad)          # refused before the model is looked at
        with pytest.raises(ValueError):
            Detector(None, box_voting={}, scoring=bad)
    assert list(inspect.signature(Detector.__init__).parameters)[1:] == ["model", "static_weights", "proposals", "nms"]


def test_rows_per_candidate():
    from frcnn_amd.Detector import scoring_rows
    assert scoring_rows("top", 0.0, 17) == 1 and scoring_rows("top", 0.05, 201) == 1
    assert scoring_rows("all", 0.0, 17) == 16 and scoring_rows("all", 0.0, 2) == 1
    assert scoring_rows("all", 0.05, 201) == 21 and scoring_rows("all", 0.05, 17) == 16
    assert scoring_rows("all", 0.2, 17) == 6 and scoring_rows("all", 0.5, 17) == 3 and scoring_rows("all", 0.3, 17) == 4
    assert scoring_rows("all", 0.99, 17) == 2 and scoring_rows("all", 0.5, 2) == 1
    for ncls in D.NCLS:
        for c in D.MIN_CONF:
            assert scoring_rows("all", c, ncls) == D.max_rows(ncls, c)


def test_max_detections_keeps_the_best_with_ties_to_the_earlier_pick():
    from frcnn_amd.Detector import keep_best
    conf = np.array([-0.5, -0.1, -0.5, -0.05, -0.1, -2.0])
    assert keep_best(conf, 1).tolist() == [3]
    assert keep_best(conf, 2).tolist() == [1, 3]            # -0.1 twice: the earlier pick
    assert keep_best(conf, 3).tolist() == [1, 3, 4]
    assert keep_best(conf, 4).tolist() == [0, 1, 3, 4]      # -0.5 twice: the earlier pick
    assert keep_best(conf, 6).tolist() == [0, 1, 2, 3, 4, 5] == keep_best(conf, 60).tolist()
    # compared as fp32 values: two doubles that round to one fp32 tie
    a = float(np.float32(-0.3))
    assert keep_best(np.array([a - 1e-12, a + 1e-12, -1.0]), 1).tolist() == [0]
    assert keep_best(np.array([-0.0, 0.0]), 1).tolist() == [0]


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_by_hand():
    lp = np.log(np.array([[0.5, 0.32, 0.18], [0.1, 0.3, 0.6], [0.25, 0.25, 0.5], [0.45, 0.45, 0.1]])).astype(np.float32)
    top = D.detect_classes(lp, 3, 0.2, D.TOP)
    assert top["cand"].tolist() == [0, 3] and top["cls"].tolist() == [1, 1] and top["total"] == 2      # (row 3: the FIRST maximum)
    assert top["conf"].tobytes() == lp[[0, 3], [0, 0]].tobytes()
    every = D.detect_classes(lp, 3, 0.2, D.ALL)
    assert list(zip(every["cand"].tolist(), every["cls"].tolist())) == [(0, 1), (0, 2), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)]
    assert every["per_candidate"].tolist() == [2, 1, 2, 2]
    assert D.detect_classes(lp, 1, 0.2, D.ALL)["cand"].tolist() == [0, 1, 1, 2, 2, 3]                   # another background
    cut = D.detect_classes(lp, 3, 0.2, D.ALL, row_stride=3)
    assert cut["K"] == 3 and cut["total"] == 7 and cut["cand"].tolist() == [0, 0, 1]
    assert D.detect_classes(lp, 3, 0.5, D.ALL)["total"] == 0        # (0.5 is not > 0.5 -- and the fp32 log of 0.5 lies below it)
    nan = np.array([[np.nan, -0.1, -3.0], [-0.1, np.nan, -3.0]], np.float32)
    assert D.first_max(nan).tolist() == [0, 0]                       # cnet_decode_kernel's loop: a leading NaN stays, a later one never wins
    assert D.detect_classes(nan, 3, 0.2, D.TOP)["cand"].tolist() == [1]
    assert D.detect_classes(nan, 3, 0.2, D.ALL)["cand"].tolist() == [0, 1]


def _problems():
    for ncls in D.NCLS:
        for R in D.SIZES:
            yield R, ncls, D.problem(D.case_seed(R, ncls), R, ncls, nan_row=True)


def test_properties_and_input_conditions_of_the_gpu_problems():
    multi = 0
    for R, ncls, P in _problems():
        lp, bg = P["lp"], ncls
        for c in D.MIN_CONF:
            tag = "R %d ncls %d min_conf %g" % (R, ncls, c)
            # no exp(lp) within 1e-9 (relative) of the threshold: the device's exp and libm cannot disagree on a decision
            assert D.threshold_margin(lp, c) > 1e-9, tag
            top, every = D.detect_classes(lp, bg, c, D.TOP), D.detect_classes(lp, bg, c, D.ALL)
            # mode 1 holds mode 0's rows
            rows = set(zip(every["cand"].tolist(), every["cls"].tolist()))
            assert set(zip(top["cand"].tolist(), top["cls"].tolist())) <= rows, tag
            assert np.all(every["cls"] != bg) and every["total"] == every["per_candidate"].sum(), tag
            assert every["per_candidate"].max() <= D.max_rows(ncls, c), tag
            if R >= 4:
                assert every["per_candidate"][0] == 0 and top["per_candidate"][0] == 0, "%s: a row whose classes all fail" % tag
                assert every["per_candidate"][3] == 0, "%s: the NaN row" % tag
                if c < 0.4:    # the background arg-max (0.56) beside a class of 0.4: nothing under "top", a row under "all"
                    assert D.first_max(lp)[1] == bg - 1 and top["per_candidate"][1] == 0 and every["per_candidate"][1] >= 1, tag
                if c == 0:     # every foreground class of an ordinary row passes
                    assert np.all(every["per_candidate"][4:] == ncls - 1), tag
            if ncls > 2 and R >= 63 and c <= 0.2:
                assert every["per_candidate"].max() >= 2, "%s: no candidate with several rows" % tag
                multi += 1
    assert multi > 0


def test_all_at_one_half_is_top_at_one_half():
    """at most one class exceeds 1/2, and it is the arg-max"""
    for R, ncls, P in _problems():
        a, b = D.detect_classes(P["lp"], ncls, 0.5, D.ALL), D.detect_classes(P["lp"], ncls, 0.5, D.TOP)
        assert a["cand"].tolist() == b["cand"].tolist() and a["cls"].tolist() == b["cls"].tolist()


# ------------------------------------------------------------------------------------------------ the surfaces
def test_surfaces_name_the_entry_point():
    import frcnn_amd as F
    assert "frcnn_detect_classes_batch" in F._lib.exported_symbols()
    det = _lua_code(open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read())
    assert "C.frcnn_detect_classes_batch(" in det and "function Detector.scoring_settings" in det and "cfg.scoring" in det
    assert "opts.scoring" in det and "function Detector:set_scoring" in det
    # the drop-in's one launch lies between the classification net and the per-class pass; the per-frame pair stays for the key absent
    a, b = det.index("C.frcnn_detect_classes_batch("), det.index("C.frcnn_nms_device_batch(dbb")
    assert det.index("C.frcnn_detect_post(") < a < b
    from frcnn_amd.evaluation import evaluate_detections
    assert "scoring" in evaluate_detections.__doc__
