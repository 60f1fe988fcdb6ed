"""cfg["scoring"]["boxes"] without a device: the setting's validation (scoring_boxes), the three refusals, the return values of
scoring_settings and box_head_settings (unchanged), the numpy restatement (tests/class_boxes_ref.py) against hand-computed
cases, the entry points' argument errors (returned before any launch), and the declarations for both hosts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import class_boxes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the setting
def test_scoring_boxes_accepted(F):
    sb = F.scoring_boxes
    from frcnn_amd.Detector import Detector
    assert Detector.scoring_boxes is sb
    for t in (None, {}, dict(class_count=16), dict(class_count=16, scoring=None), dict(class_count=16, scoring={}),
              dict(classes="all"), dict(boxes="candidate"), dict(class_count=16, scoring=dict(boxes="candidate", classes="all"))):
        assert sb(t) == "candidate", t
    for t in (dict(boxes="class"), dict(boxes="class", classes="all", min_confidence=0.05, max_detections=3),
              dict(class_count=16, scoring=dict(boxes="class")), dict(boxes="class", classes="top")):
        assert sb(t) == "class", t


@pytest.mark.parametrize("table", [
    dict(boxes="row"), dict(boxes="CLASS"), dict(boxes="classes"), dict(boxes=""), dict(boxes=True), dict(boxes=False), dict(boxes=1),
    dict(boxes=0), dict(boxes=None), dict(boxes=["class"]), dict(boxes=dict(per="class")), dict(boxes=b"class"), dict(boxes=1.0),
    dict(box="class"), dict(boxes="class", per_class=True), "class", ["class"], True,
])
def test_scoring_boxes_rejects(F, table):
    with pytest.raises(ValueError):
        F.scoring_boxes(table)
    if isinstance(table, dict):
        with pytest.raises(ValueError):
            F.scoring_boxes(dict(class_count=16, scoring=table))
        from frcnn_amd.Detector import Detector
        with pytest.raises(ValueError):
            Detector(None, scoring=table)                  # refused before the model is looked at


def test_the_other_validators_return_what_they_returned(F):
    from frcnn_amd.Detector import scoring_settings
    assert scoring_settings(dict(boxes="class")) == ("top", 0.2, None)
    assert scoring_settings(dict(classes="all", min_confidence=0.05, max_detections=7, boxes="class")) == ("all", 0.05, 7)
    assert scoring_settings(dict(class_count=16, scoring=dict(boxes="candidate"))) == ("top", 0.2, None)
    assert scoring_settings(None) is None and scoring_settings(dict(class_count=16)) is None
    st = F.box_head_settings
    assert st(dict(box_head=dict(per_class=True), scoring=dict(classes="all", boxes="class"))) == dict(per_class=True)
    assert st(dict(box_head=dict(per_class=True), scoring=dict(classes="top", boxes="class"))) == dict(per_class=True)
    assert st(dict(box_head=dict(per_class=True), scoring=dict(boxes="candidate"))) == dict(per_class=True)
    assert st(dict(scoring=dict(classes="all", boxes="candidate"))) == dict(per_class=False)
    assert st(dict()) == dict(per_class=False)


def test_the_three_refusals(F):
    from frcnn_amd.Detector import Detector
    per = dict(F.duplo_cfg, box_head=dict(per_class=True))
    # 1. a shared head with boxes = "class": box_head_settings, create_model, set_scoring, each naming both keys
    for sc in (dict(boxes="class"), dict(boxes="class", classes="all"), dict(boxes="class", classes="top")):
        for cfg in (dict(F.duplo_cfg, scoring=sc), dict(F.duplo_cfg, scoring=sc, box_head=dict(per_class=False)),
                    dict(F.duplo_cfg, scoring=sc, box_head={})):
            with pytest.raises(F.FrcnnError) as e:
                F.box_head_settings(cfg)
            assert "scoring.boxes" in str(e.value) and "box_head.per_class" in str(e.value)
            with pytest.raises(F.FrcnnError):
                F.vgg_small(cfg)
        d = Detector.__new__(Detector)
        d.model = F.vgg_small(dict(F.duplo_cfg))
        d.set_scoring(dict(classes="all"))
        with pytest.raises(F.FrcnnError) as e:
            d.set_scoring(sc)
        assert "scoring.boxes" in str(e.value) and "box_head.per_class" in str(e.value)
        assert d.scoring == ("all", 0.2, None) and d.boxes == "candidate"          # (a refused table changes nothing)
    # 2. a bad value: ValueError from the validator, before the model is looked at
    d = Detector.__new__(Detector)
    d.model = F.vgg_small(per)
    d.set_scoring(dict(classes="top"))
    with pytest.raises(ValueError, match="boxes"):
        d.set_scoring(dict(classes="all", boxes="per_class"))
    assert d.scoring == ("top", 0.2, None) and d.boxes == "candidate"
    # 3. the present refusal, still raised without the key and with "candidate" -- and its message names the way out
    for sc in (dict(classes="all"), dict(classes="all", boxes="candidate")):
        with pytest.raises(F.FrcnnError) as e:
            F.box_head_settings(dict(per, scoring=sc))
        assert all(w in str(e.value) for w in ("box_head.per_class", "scoring.classes", "scoring.boxes = \"class\""))
        with pytest.raises(F.FrcnnError) as e:
            d.set_scoring(sc)
        assert all(w in str(e.value) for w in ("box_head.per_class", "scoring.classes", "scoring.boxes = \"class\""))
    # the opt-in is accepted, by the validators and by a Detector -- under "all" and, as a no-op, under "top"
    for sc, want in ((dict(classes="all", boxes="class"), ("all", 0.2, None)), (dict(boxes="class"), ("top", 0.2, None))):
        F.vgg_small(dict(per, scoring=sc))
        d.set_scoring(sc)
        assert d.scoring == want and d.boxes == "class"
    d.set_scoring(None)
    assert d.scoring is None and d.boxes == "candidate"


def test_feature_count_and_the_features_entry_point(F):
    m = F.vgg_small(dict(F.duplo_cfg))
    assert m["cnet"].feature_count == 512 == m["class_layers"][-1]["n"]
    p = C.c_void_p(0x1000)
    with pytest.raises(F.FrcnnError, match="cnet_features.*forward"):
        F._lib.call("frcnn_cnet_features", m["native"].h, p, None)                # before any forward pass
    with pytest.raises(F.FrcnnError, match="cnet_features"):
        F._lib.call("frcnn_cnet_features", m["native"].h, None, None)
    with pytest.raises(F.FrcnnError, match="cnet_features"):
        F._lib.call("frcnn_cnet_features", None, p, None)
    with pytest.raises(F.FrcnnError, match="combine_and_flatten"):
        m["native"].box_head_parameters()


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_decode_by_hand():
    a = np.array([[10.0, 20.0, 30.0, 60.0], [0.0, 0.0, 8.0, 4.0]])
    d = np.array([[0.5, -0.25, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    assert R.decode(a, d).tolist() == [[20.0, 10.0, 40.0, 50.0], [0.0, 0.0, 8.0, 4.0]]
    q = R.decode(a[:1], np.array([[0, 0, 1, -1]], np.float32))[0]
    e = np.exp(np.array([1.0, -1.0]))
    assert q[2] == 10.0 + e[0] * 20.0 and q[3] == 20.0 + e[1] * 40.0
    b = R.decode_bound(a, d)
    assert not b[:, :2].any() and (b[:, 2:] > 0).all() and (b[:, 2:] < 1e-13).all()


def test_restatement_by_hand():
    """two classes, two features, two frames whose features lie in reverse order; frame 1 is cut at K = 1"""
    feat = np.array([[9, 9], [1, 2], [3, -1], [0, 0], [2, 2]], np.float32)
    W = np.array([[1, 0], [0, 1], [0, 0], [0, 0], [2, 0], [0, 2], [0, 0], [0, 0]], np.float32)
    b = np.array([0, 0, 0, 0, 1, 1, 0, 0], np.float32)
    rect = np.array([[[0, 0, 10, 10], [100, 100, 102, 104]], [[0, 0, 1, 1], [5, 5, 7, 7]]], np.float64)
    P = dict(B=2, feat=feat, row0=[4, 1], W=W, b=b, rect=rect, pick=np.array([[2, 1], [1, 2]], np.int64),
             kc=np.array([[2, 1, 3], [1, 2, 2]], np.int32), keep_row=np.array([[0, 0, 0], [1, 0, 1]], np.int32),
             K=np.array([7, 1], np.int32), row_stride=3, bb=np.full((2, 3, 5), R.SENT, np.float32), r2=np.full((2, 3, 4), R.SENT))
    dl = R.deltas(P)
    assert dl[0][0].tolist() == [[5, 5, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0]] and dl[0][2] == 3       # (K above row_stride: clipped)
    assert dl[1][0].tolist() == [[3, -1, 0, 0]] and dl[1][2] == 1
    w = R.class_boxes(P)
    assert w["r2"][0].tolist() == [[110, 120, 112, 124], [104, 108, 106, 112], [100, 100, 102, 104]]   # (class 3 of 2: d = 0)
    assert w["r2"][1].tolist() == [[11, 3, 13, 5], [R.SENT] * 4, [R.SENT] * 4]
    assert w["bb"][0, :, :4].tolist() == w["r2"][0].tolist() and (w["bb"][:, :, 4] == np.float32(R.SENT)).all()
    assert (w["bb"][1, 1:] == np.float32(R.SENT)).all()


def test_the_problems_are_what_the_gpu_tests_promise():
    for nf, Cn, B, cands in ((7, 3, 3, 67), (64, 17, 3, 5), (4, 1, 1, 67), (260, 17, 1, 1), (1, 3, 3, 0)):
        for integer in (False, True):
            P = R.problem(R.case_seed(nf, Cn, B, cands), nf, Cn, B, cands, integer=integer)
            assert min(P["row0"]) > 0 and (B == 1 or list(P["row0"]) != sorted(P["row0"]))
            assert max(P["row0"]) + max(cands, 1) <= len(P["feat"])
            assert P["pick"].min() >= 1 and P["pick"].max() <= P["rect"].shape[1]
            assert P["keep_row"].min() >= 0 and P["keep_row"].max() < max(cands, 1)
            if cands >= 5:
                rows = [c for f in P["per"] for cl in f for c in cl]
                assert (0 in rows or Cn + 1 in rows) and any(len(cl) > 1 for f in P["per"] for cl in f)
                assert any(cl != sorted(cl) for f in P["per"] for cl in f) or Cn == 1
            if B == 3:
                k = [min(int(v), P["row_stride"]) for v in P["K"]]
                assert k[2] == 0 and (cands == 0 or (0 < k[0] < k[1] == P["row_stride"] < int(P["K"][1])))
            if integer:
                w = R.class_boxes(P)
                assert np.array_equal(w["r2"], np.rint(w["r2"])) and np.abs(w["r2"]).max() < 2 ** 24


# ------------------------------------------------------------------------------------------------------ the entry point's errors
def test_argument_errors_are_returned_before_any_launch(F):
    """every refused call returns an error code with a message; the pointers are never dereferenced (they are not device memory
    here)"""
    lib = F._lib.load()
    p = C.c_void_p(0x1000)
    row0 = (C.c_longlong * 3)(0, 5, 2)

    def call(feat=p, nf=8, row0=row0, B=3, W=p, b=p, Cn=3, rect=p, pick=p, ms=12, kc=p, keep=p, K=p, rs=16, bb=p, r2=p):
        return lib.frcnn_detect_class_boxes_batch(feat, nf, row0, B, W, b, Cn, rect, pick, ms, kc, keep, K, rs, bb, r2, None)

    bad = [dict(B=-1), dict(B=65536), dict(nf=0), dict(nf=-4), dict(Cn=0), dict(Cn=1 << 20, nf=1 << 10), dict(rs=-1), dict(ms=-1),
           dict(feat=None), dict(row0=None), dict(W=None), dict(b=None), dict(rect=None), dict(pick=None), dict(kc=None),
           dict(keep=None), dict(K=None), dict(bb=None), dict(r2=None), dict(row0=(C.c_longlong * 3)(0, -1, 2)),
           dict(feat=C.c_void_p(0x1002)), dict(r2=C.c_void_p(0x1004))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.frcnn_last_error().decode().startswith("detect_class_boxes_batch"), kw
    # nothing to do: no launch, no error -- also with every array NULL
    for kw in (dict(B=0), dict(rs=0)):
        assert call(**kw) == 0, kw
        assert call(feat=None, row0=None, W=None, b=None, rect=None, pick=None, kc=None, keep=None, K=None, bb=None, r2=None, **kw) == 0
    with pytest.raises(F.FrcnnError, match="frames"):
        F._lib.call("frcnn_detect_class_boxes_batch", p, 8, row0, 70000, p, p, 3, p, p, 12, p, p, p, 16, p, p, None)


# ------------------------------------------------------------------------------------------------------------ the declarations
def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_points_are_declared_for_both_hosts(F):
    """the two entry points live in include/frcnn_hip_classbox.h, which frcnn_hip.h includes: the library exports them, the host
    mirror's fifth ctypes table and the Lua binding's fifth generated cdef declare exactly them with the header's argument
    counts, and the Lua files call them through the CX handle only"""
    names = {"frcnn_detect_class_boxes_batch", "frcnn_cnet_features"}
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_classbox.h")).read()
    assert '#include "frcnn_hip_classbox.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names == set(F._lib.CLASSBOX_SIGS)
    others = set(F._lib.exported_symbols()) | set(F._lib.HARD_SIGS) | set(F._lib.LOSS_SIGS) | set(F._lib.BOX_SIGS)
    assert not names & others
    for name, nargs in (("frcnn_detect_class_boxes_batch", 17), ("frcnn_cnet_features", 3)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m and len(m.group(1).split(",")) == len(F._lib.CLASSBOX_SIGS[name][0]) == nargs, name
    lib = C.CDLL(F._lib.SO_PATH)
    assert all(hasattr(lib, n) for n in names) and all(getattr(F._lib.load(), n).argtypes for n in names)
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    fifth = re.findall(r"ffi\.cdef \[\[(.*?)\]\]", lua, re.S)
    assert len(fifth) == 1 and _symbols(fifth[0]) == names
    first = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert not names & _symbols(first)
    hcdef = re.sub(r"\s+", " ", re.search(r"int frcnn_detect_class_boxes_batch\([^;]*\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(0))
    assert hcdef in re.sub(r"\s+", " ", fifth[0])
    used = set()
    for fn in ("frcnn_hip.lua", "objective_hip.lua", "Detector_hip.lua", "frcnn_shims.lua.in"):
        txt = open(os.path.join(ROOT, "bindings", fn)).read()
        used |= set(re.findall(r"\bCX\.(frcnn_[a-z0-9_]+)", txt))
        for n in names:
            assert not re.search(r"\bC[HLB]?\.%s\b" % n, txt), (fn, n)
    assert used == names
    assert "class_boxes.hip" in open(os.path.join(ROOT, "build_lib.sh")).read()
    for name in ("class_boxes", "scoring_boxes"):
        assert name in F.__all__ and callable(getattr(F, name))
    # counted with the element-wise kernels, like the class test and the box head
    src = open(os.path.join(ROOT, "faster-rcnn.torch_amd", "csrc", "class_boxes.hip")).read()
    assert src.count("FR_LAUNCH(KC_ELEMWISE") == 2 and "atomic" not in src.replace("No atomics", "")


def test_the_lua_drop_in_carries_the_path():
    det = open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read()
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    assert "function Detector.scoring_boxes(t)" in det and "self.scoring_box = boxes" in det
    assert "hip.CX.frcnn_detect_class_boxes_batch(all_feat, nf, row0_arg, B, W_box, b_box, ncls - 1, mr, dpick, cap, dkc, dkeep," in det
    assert det.index("frcnn_detect_class_boxes_batch(all_feat") < det.index("C.frcnn_detect_merge_views(")    # in front of the merge
    assert det.index("C.frcnn_detect_classes_batch(all_cls") < det.index("frcnn_detect_class_boxes_batch(all_feat")
    assert det.count("cnet:features(") == 2 and "k ~= 'boxes'" in det
    assert 'cfg.scoring.boxes = "class" needs cfg.box_head.per_class = true' in det
    assert "function cnet:features(dst)" in shim and "CX.frcnn_cnet_features(native, dst, nil)" in shim
    assert "function M.box_head_parameters(model)" in shim and "cnet.feature_count =" in shim
    assert 'cfg.scoring.boxes = "class" needs cfg.box_head.per_class = true' in shim and "boxes ~= 'class'" in shim


def test_the_documents_name_the_setting(F):
    for fn in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, fn)).read()
        assert "frcnn_detect_class_boxes_batch" in txt and "boxes" in txt, fn
    assert "boxes" in F.evaluate_detections.__doc__
