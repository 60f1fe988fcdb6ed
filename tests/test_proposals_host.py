"""cfg.proposals without a device: Detector.proposal_settings (defaults, every error, errors before anything touches the model
or the device), evaluation.proposal_recall on a stub detector, and the texts that carry the feature through the C ABI and the
Lua drop-in (static checks: no Lua runtime here)."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ------------------------------------------------------------------------------------------------ settings
def test_defaults_are_the_reference(F):
    ps = F.Detector.proposal_settings
    assert ps(None) == ("y2", None, None)
    assert ps({}) == ("y2", None, None)
    assert ps(dict(order="y2")) == ("y2", None, None)
    assert ps(dict(F.duplo_cfg)) == ("y2", None, None)                      # a model's cfg without the table
    assert ps(dict(F.duplo_cfg, proposals=None)) == ("y2", None, None)
    cfg = dict(F.imgnet_cfg, proposals=dict(order="score", pre_nms_top_n=6000, post_nms_top_n=300))
    assert ps(cfg) == ("score", 6000, 300)
    assert ps(cfg["proposals"]) == ("score", 6000, 300)
    assert ps(dict(pre_nms_top_n=np.int64(12))) == ("y2", 12, None)         # pre_nms_top_n goes with either order
    assert type(ps(dict(pre_nms_top_n=np.int64(12)))[1]) is int
    assert ps(dict(order="score", post_nms_top_n=1)) == ("score", None, 1)


BAD = [
    dict(top_n=5),                                        # an unknown key
    dict(order="score", pre_nms_topn=5),
    dict(order="area"),                                   # an unknown order
    dict(order=2),
    dict(order=None),
    dict(pre_nms_top_n=True),                             # a bool
    dict(order="score", post_nms_top_n=False),
    dict(pre_nms_top_n=300.0),                            # not an integer
    dict(pre_nms_top_n="300"),
    dict(order="score", post_nms_top_n=2.5),
    dict(pre_nms_top_n=0),                                # N < 1
    dict(pre_nms_top_n=-4),
    dict(order="score", post_nms_top_n=0),
    dict(post_nms_top_n=300),                             # post_nms_top_n without order = "score"
    dict(order="y2", post_nms_top_n=300),
    dict(order="y2", pre_nms_top_n=6000, post_nms_top_n=300),
    [("order", "score")],                                 # not a table
]


@pytest.mark.parametrize("table", BAD, ids=[repr(t) for t in BAD])
def test_errors(F, table):
    with pytest.raises(ValueError):
        F.Detector.proposal_settings(table)
    with pytest.raises(ValueError):
        F.Detector.proposal_settings(dict(F.duplo_cfg, proposals=table))


class _Untouchable(object):
    """stands for the model: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the model was touched (%s) before the settings were checked" % name)

    def __getitem__(self, key):
        raise AssertionError("the model was touched ([%r]) before the settings were checked" % (key,))


class _CfgOnly(dict):
    """a model of which only the cfg may be read"""

    def __getitem__(self, key):
        if key != "cfg":
            raise AssertionError("the model was touched ([%r]) before the settings were checked" % (key,))
        return dict.__getitem__(self, key)


@pytest.mark.parametrize("table", BAD[:16], ids=[repr(t) for t in BAD[:16]])
def test_errors_come_before_any_device_call(F, table, monkeypatch):
    def no_call(name, *a):
        raise AssertionError("device call %s before the settings were checked" % name)
    monkeypatch.setattr(F._lib, "call", no_call)
    with pytest.raises(ValueError):
        F.Detector(_Untouchable(), proposals=table)
    with pytest.raises(ValueError):
        F.Detector(_Untouchable(), static_weights=True, proposals=table)
    with pytest.raises(ValueError):
        F.Detector(_CfgOnly(cfg=dict(F.duplo_cfg, proposals=table)))       # main.lua's Detector(model): the cfg carries it


# ------------------------------------------------------------------------------------------------ proposal_recall
class _StubDetector(object):
    def __init__(self, F, boxes_per_image):
        self.F, self.boxes, self.i = F, boxes_per_image, 0

    def proposals(self, img):
        out = [dict(p=0.0, r=self.F.Rect(*b), l=1, a=None) for b in self.boxes[self.i % len(self.boxes)]]
        self.i += 1
        return out


class _Val(object):
    def __init__(self, items):
        self.items, self.i = items, 0

    def nextValidation(self, count=1):
        out = []
        for _ in range(count):
            out.append(self.items[self.i % len(self.items)])
            self.i += 1
        return out


def test_proposal_recall_on_hand_made_boxes(F):
    R, Roi = F.Rect, F.Roi
    items = [
        dict(img=None, rois=[Roi(R(0, 0, 10, 10), 1), Roi(R(50, 50, 70, 70), 2)]),
        dict(img=None, rois=[Roi(R(0, 0, 10, 10), 3)]),
        dict(img=None, rois=[]),
    ]
    props = [
        [(0, 0, 10, 5), (0, 0, 10, 10.5), (200, 200, 210, 210)],      # IoU 0.5 (exactly the threshold) and 0.952 with roi 1; roi 2 missed
        [(0, 0, 10, 4.9)],                                            # IoU 0.49: missed
        [(1, 1, 2, 2), (3, 3, 4, 4)],
    ]
    got = F.proposal_recall(_StubDetector(F, props), _Val(items), 3)
    assert got == dict(recall=1.0 / 3.0, ground_truth=3, proposals_per_image=2.0)
    # a stricter threshold loses nothing here (0.952 still covers roi 1); at 0.96 it is lost
    assert F.evaluation.proposal_recall(_StubDetector(F, props), _Val(items), 3, iou_threshold=0.9)["recall"] == 1.0 / 3.0
    assert F.evaluation.proposal_recall(_StubDetector(F, props), _Val(items), 3, iou_threshold=0.96)["recall"] == 0.0
    # a looser one recalls the second image's box too
    assert F.proposal_recall(_StubDetector(F, props), _Val(items), 3, iou_threshold=0.45)["recall"] == 2.0 / 3.0
    # the iterator is cycled like nextValidation does; no ground truth at all: recall is nan
    assert F.proposal_recall(_StubDetector(F, props), _Val(items), 6)["ground_truth"] == 6
    none = F.proposal_recall(_StubDetector(F, props), _Val(items[2:]), 2)
    assert math.isnan(none["recall"]) and none["ground_truth"] == 0 and none["proposals_per_image"] == 2.0    # (3 + 1 boxes on 2 images)
    assert "proposal_recall" in F.__all__


# ------------------------------------------------------------------------------------------------ texts
def test_header_declares_the_entry_points():
    hdr = _text("include", "frcnn_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bsize_t frcnn_topk_select_workspace_bytes\(int B, int n_cap\);", code)
    m = re.search(r"\bint frcnn_topk_select\((.*?)\);", code, re.S)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "score", "B", "stride", "n_cap", "n_dev", "K", "sel_row", "sel_stride", "k_dev", "workspace", "workspace_bytes", "stream"]
    m = re.search(r"\bint frcnn_rpn_gather_rows\((.*?)\);", code, re.S)
    assert m
    args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    for name in ("match_p", "match_idx", "match_rect", "match_box", "sel_row", "k_dev", "box5", "row", "stream"):
        assert name in args, name
    assert re.search(r"const double \*match_rect", m.group(1))
    consts = dict((k, int(v)) for k, v in re.findall(r"#define FRCNN_KC_(\w+) (\d+)", hdr))
    assert consts["TOPK"] == consts["COUNT"] - 1


def _plain(txt):
    """comment decoration and line breaks out of the way, lower case"""
    return re.sub(r"\s+", " ", re.sub(r"^\s*(\*|--|#|//)\s?", " ", txt, flags=re.M)).lower()


def test_the_semantics_are_stated_alike_everywhere():
    """rank, tie rule and order of the selected set: the same words in the header, INTEGRATION.md, both hosts and the kernel"""
    for parts in (("include", "frcnn_hip.h"), ("INTEGRATION.md",), ("faster-rcnn.torch_amd", "Detector.py"),
                  ("bindings", "Detector_hip.lua")):
        txt = _plain(_text(*parts))
        for phrase in ("-0 equals +0", "a nan ranks below everything", "ties are broken by the lower scan row",
                       "keep their scan order"):
            assert phrase in txt, (parts[-1], phrase)
    kern = _plain(_text("faster-rcnn.torch_amd", "csrc", "topk.hip"))
    for phrase in ("-0 equals +0, a nan ranks below everything", "ties are broken by the lower scan row", "keep their scan order"):
        assert phrase in kern, phrase


def test_lua_binding_declares_and_the_drop_in_calls_them():
    lua = _text("bindings", "frcnn_hip.lua")
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for name in ("frcnn_topk_select", "frcnn_rpn_gather_rows"):
        assert re.search(r"\bint %s\(" % name, cdef), name
    assert re.search(r"\bsize_t frcnn_topk_select_workspace_bytes\(", cdef)
    assert "static const int FRCNN_KC_TOPK" in cdef
    det = _text("bindings", "Detector_hip.lua")
    # main.lua calls Detector(model) unchanged: the settings come from the model's cfg
    assert "Detector.proposal_settings(self.model.cfg.proposals)" in det
    assert re.search(r"^function Detector\.proposal_settings\(t\)", det, re.M)
    assert re.search(r"^function Detector:proposals\(input\)", det, re.M)
    assert re.search(r"^function Detector:first_stage\(frames, prefix\)", det, re.M)
    for call in ("C.frcnn_topk_select_workspace_bytes(", "C.frcnn_topk_select(", "C.frcnn_rpn_gather_rows("):
        assert call in det, call
    # both hosts refuse the same things
    for needle in ("unknown key", "is not an integer", "at least 1", "needs order = \"score\""):
        assert needle in det, needle
    # every NMS call of the one pipeline (first pass, its repeat over the bound, per-class pass) takes the key from the setting
    assert det.count("key_mode, key_col = 2, 5") >= 1
    calls = re.findall(r"C\.frcnn_nms_device\w*\([^;]*?\)\)", det)
    assert len(calls) >= 3 and len(calls) == len(re.findall(r"C\.frcnn_nms_device\w*\(", det))
    for call in calls:
        assert "key_mode, key_col" in " ".join(call.split()), call
    assert "'pre_nms_top_n'" in det and "'post_nms_top_n'" in det and "self:clamp_candidates(" in det


def test_python_detector_surface(F):
    import inspect
    sig = inspect.signature(F.Detector.__init__)
    assert list(sig.parameters)[1:] == ["model", "static_weights", "proposals", "nms"]
    assert sig.parameters["static_weights"].default is False and sig.parameters["proposals"].default is None
    assert sig.parameters["nms"].default is None
    assert callable(F.Detector.proposals) and callable(F.Detector.set_proposals)
    assert "topk" == F._lib.KC_NAMES[-1]
    for name in ("frcnn_topk_select", "frcnn_topk_select_workspace_bytes", "frcnn_rpn_gather_rows"):
        assert name in F._lib.exported_symbols()
    assert F._lib.load().frcnn_topk_select_workspace_bytes(8, 45015) >= 8 * 45015 * 4
    src = _text("build_lib.sh")
    assert src.count("topk") == 2, "topk.hip belongs to both source lists of build_lib.sh"
