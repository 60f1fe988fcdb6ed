"""The proposal-target layer (cfg.roi_sampling, frcnn_proposal_targets_batch) without a GPU: the numpy restatement the device test
compares against equals a plain Python loop over the host mirror's own Rect.IoU / Rect.intersect / Anchors.inputToAnchor, on every
case of the tables; the tables reach every branch of the rule at least twice; the settings are accepted and refused as
documented; the entry point is declared for the Lua host."""
import math
import os
import re

import numpy as np
import pytest

import proposal_targets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = R.rule_cases() + R.size_cases() + R.batch_cases()


def _key(seed, i, b):
    x = (seed + 0x9E3779B9 * (i + 1) + 0x85EBCA6B * b) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _iou(F, a, b):
    """Rect.IoU with C's division: Python raises where IEEE gives an infinity or a NaN"""
    try:
        return F.Rect.IoU(a, b)
    except ZeroDivisionError:
        i = F.Rect.intersect(a, b).area()
        return float("nan") if i == 0 or i != i else math.copysign(float("inf"), i)


def loop_ref(F, case, b=0):
    """frcnn_proposal_targets_batch as the header states it, row by row, on the host mirror's classes"""
    gts = [F.Rect(*[float(v) for v in g]) for g in case["gt_rect"]]
    R_ = min(max(int(case["r_dev"]), 0), int(case["r_cap"]))
    cands = list(gts) if case["include_gt"] else []
    for p in case["pick"][:R_]:
        cands.append(F.Rect(*[float(v) for v in case["rect"][int(p) - 1]]))
    label, best, best_g = [], [], []
    for c in cands:
        ok = all(math.isfinite(v) for v in c.unpack()) and c.width() > 0 and c.height() > 0
        bi, bg = 0.0, -1
        for g, r in enumerate(gts if ok else []):
            q = _iou(F, c, r)
            q = 0.0 if q != q else q
            if g == 0 or q > bi:
                bi, bg = q, g
        best.append(bi); best_g.append(bg)
        label.append(0 if not ok else 1 if bg >= 0 and bi >= case["fg_iou"] else 2 if case["bg_lo"] <= bi < case["bg_hi"] else 0)
    fg = [i for i, l in enumerate(label) if l == 1]
    bgr = [i for i, l in enumerate(label) if l == 2]
    Fq = min(len(fg), case["fg_quota"])
    Bq = min(len(bgr), case["batch"] - Fq)
    keep = lambda rows, q: sorted(sorted(rows, key=lambda i: _key(case["seed"], i, b))[:q])
    rows = keep(fg, Fq) + keep(bgr, Bq)
    out = dict(counts=(len(fg), len(bgr), Fq, Bq), src=rows, gt_idx=[best_g[i] for i in rows], iou=[best[i] for i in rows],
               roi=[list(cands[i].unpack()) for i in rows], crtarget=[], cctarget=[])
    for k, i in enumerate(rows):
        if k < Fq:
            g = gts[best_g[i]]
            c = cands[i]
            try:
                t = F.Anchors.inputToAnchor(c, g)
            except ValueError:     # math.log of a ratio that is not positive: IEEE gives NaN or -inf
                t = None
            out["crtarget"].append(t)
            out["cctarget"].append(float(case["gt_class"][best_g[i]]))
        else:
            out["crtarget"].append(np.zeros(4, np.float32))
            out["cctarget"].append(float(case["bgclass"]))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_restatement_equals_the_plain_loop(F, case):
    for b in (0, 2):
        got, want = R.targets_ref(case, b), loop_ref(F, case, b)
        assert got["counts"] == want["counts"]
        S = want["counts"][2] + want["counts"][3]
        assert got["src"].tolist() == want["src"] and got["gt_idx"].tolist() == want["gt_idx"]
        assert _bits(got["iou"]) == _bits(np.array(want["iou"], np.float64).reshape(S))
        assert _bits(got["roi"]) == _bits(np.array(want["roi"], np.float64).reshape(S, 4))
        assert got["cctarget"].tolist() == want["cctarget"]
        for k in range(S):
            if want["crtarget"][k] is not None:
                assert _bits(got["crtarget"][k]) == _bits(np.asarray(want["crtarget"][k], np.float32)), (k, got["crtarget"][k])


def test_tables_reach_every_branch_twice():
    count = dict((b, 0) for b in R.BRANCHES)
    for case in R.rule_cases():
        for b in R.targets_ref(case)["reached"]:
            count[b] += 1
    assert all(v >= 2 for v in count.values()), count
    names = [c["name"] for c in ALL_CASES]
    assert len(set(names)) == len(names)
    sizes = set(len(R.candidates_ref(c)[0]) for c in R.size_cases())
    assert sizes >= set(R.SIZE_N), sizes
    assert set(len(c["gt_rect"]) for c in R.size_cases()) == set(R.SIZE_G)


def test_the_lower_box_wins_a_tie_and_thresholds_are_closed_below():
    tie = dict((c["name"], c) for c in R.rule_cases())
    r = R.targets_ref(tie["tie_0"])
    k = r["src"].tolist().index(2)                      # the candidate that covers both halves (rows 0, 1 are the boxes themselves)
    assert r["gt_idx"][k] == 0 and r["iou"][k] == 0.5 and r["cctarget"][k] == 3.0
    r = R.targets_ref(tie["tie_1"])
    k = r["src"].tolist().index(3)
    assert r["gt_idx"][k] == 1 and r["cctarget"][k] == 4.0
    r = R.targets_ref(tie["at_bg_hi_0"])                # 0.5 is neither background (< 0.5) nor foreground (>= 0.75): ignored
    assert 3 not in r["src"].tolist() and r["iou"][r["src"].tolist().index(4)] == 0.25


def test_keys_never_tie_within_a_segment():
    for seed in (0, 1, 0xFFFFFFFF, 123456789):
        for b in (0, 1, 65534):
            k = R.keys_ref(seed, 4096, b)
            assert len(np.unique(k)) == 4096
            assert [int(v) for v in k[:3]] == [_key(seed, i, b) for i in range(3)]


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_settings_defaults_and_quota(F):
    assert F.roi_sampling_settings({}) is None
    s = F.roi_sampling_settings(dict(roi_sampling={}))
    assert s == dict(source="examples", batch=128, fg_fraction=0.25, fg_iou=0.5, bg_iou=(0.0, 0.5), include_gt=True, threshold=0.5,
                     nms_overlap=0.7, pre_nms_top_n=6000, post_nms_top_n=2000, seed=0, fg_quota=32)
    q = lambda batch, frac: F.roi_sampling_settings(dict(roi_sampling=dict(batch=batch, fg_fraction=frac)))["fg_quota"]
    assert [q(128, 0.25), q(10, 0.25), q(10, 0.35), q(7, 0.5), q(5, 0.0), q(5, 1.0), q(1, 0.5)] == [32, 3, 4, 4, 0, 5, 1]
    s = F.roi_sampling_settings(dict(roi_sampling=dict(source="proposals", bg_iou=[0.1, 0.3], fg_iou=0.6, post_nms_top_n=4032,
                                                       pre_nms_top_n=F.Detector.NMS_FIRST_CAP, seed=2 ** 32 - 1)))
    assert s["source"] == "proposals" and s["bg_iou"] == (0.1, 0.3) and s["post_nms_top_n"] == 4032
    assert F.roi_sampling_settings(dict(roi_sampling=dict(bg_iou={1: 0.0, 2: 0.25})))["bg_iou"] == (0.0, 0.25)   # a Lua array


BAD = [("not a table", 3), ("unknown key", dict(sources="proposals")), ("source", dict(source="rpn")), ("source type", dict(source=1)),
       ("batch 0", dict(batch=0)), ("batch bool", dict(batch=True)), ("batch float", dict(batch=64.0)), ("batch big", dict(batch=4097)),
       ("fraction", dict(fg_fraction=1.25)), ("fraction neg", dict(fg_fraction=-0.1)), ("fraction str", dict(fg_fraction="1")),
       ("fg_iou", dict(fg_iou=1.5)), ("fg_iou nan", dict(fg_iou=float("nan"))), ("bg pair", dict(bg_iou=0.5)),
       ("bg three", dict(bg_iou=(0, 0.1, 0.2))), ("bg order", dict(bg_iou=(0.4, 0.3))), ("bg above fg", dict(bg_iou=(0.0, 0.6))),
       ("bg negative", dict(bg_iou=(-0.1, 0.3))), ("bg bool", dict(bg_iou=(False, 0.3))), ("include_gt", dict(include_gt=1)),
       ("threshold", dict(threshold=1.5)), ("overlap 0", dict(nms_overlap=0.0)), ("overlap big", dict(nms_overlap=1.5)),
       ("pre 0", dict(pre_nms_top_n=0)), ("pre big", dict(pre_nms_top_n=16385)), ("post 0", dict(post_nms_top_n=0)),
       ("post + 64 > 4096", dict(post_nms_top_n=4033)), ("seed neg", dict(seed=-1)), ("seed big", dict(seed=2 ** 32)),
       ("seed float", dict(seed=1.0))]


@pytest.mark.parametrize("what,table", BAD, ids=[b[0] for b in BAD])
def test_settings_refused(F, what, table):
    with pytest.raises(F.FrcnnError):
        F.roi_sampling_settings(dict(roi_sampling=table))
    if isinstance(table, dict) and "source" not in table:     # a bad value is refused under either source
        with pytest.raises(F.FrcnnError):
            F.roi_sampling_settings(dict(roi_sampling=dict(table, source="proposals")))


def test_ground_truth_table(F):
    from frcnn_amd.objective import ground_truth_table
    roi = lambda *r, c=1: F.Roi(F.Rect(*r), c)
    gt, cls = ground_truth_table(dict(rois=[roi(1, 2, 3, 4, c=7), roi(0, 0, 10, 10, c=2)]), 20)
    assert gt.tolist() == [[1, 2, 3, 4], [0, 0, 10, 10]] and cls.tolist() == [7, 2] and gt.dtype == np.float64 and cls.dtype == np.int32
    gt, cls = ground_truth_table(dict(rois=[]))
    assert gt.shape == (0, 4) and cls.shape == (0,)
    with pytest.raises(F.FrcnnError, match="rois"):
        ground_truth_table(dict(img=None, positive=[], negative=[]))
    with pytest.raises(F.FrcnnError, match="65"):
        ground_truth_table(dict(rois=[roi(0, 0, 5, 5)] * 65))
    assert len(ground_truth_table(dict(rois=[roi(0, 0, 5, 5)] * 64))[1]) == 64
    for bad in ((0, 0, 0, 5), (0, 0, 5, -1), (0, 0, float("inf"), 5)):
        with pytest.raises(F.FrcnnError):
            ground_truth_table(dict(rois=[roi(*bad)]))
    with pytest.raises(F.FrcnnError, match="class_index"):
        ground_truth_table(dict(rois=[roi(0, 0, 5, 5, c=21)]), 20)


def test_training_batches_carry_their_ground_truth():
    src = open(os.path.join(ROOT, "faster-rcnn.torch_amd", "BatchIterator.py")).read()
    body = src[src.index("def nextTraining"):src.index("def nextValidation")] if "def nextValidation" in src else src[src.index("def nextTraining"):]
    appends = re.findall(r"batch\.append\(dict\(([^)]*)\)\)", body)
    assert appends and all("rois=" in a for a in appends if "positive" in a), appends


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_everywhere(F):
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    cdef = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    for txt in (re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), cdef):
        m = re.search(r"int frcnn_proposal_targets_batch\(([^;]*)\);", txt)
        assert m, "frcnn_proposal_targets_batch is not declared"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert len(args) == 27 and args[17] == "unsigned int seed" and args[-1] == "void *stream"
    assert "frcnn_proposal_targets_batch" in F._lib.exported_symbols()
    assert len(F._lib._SIGS["frcnn_proposal_targets_batch"][0]) == 27
    assert hasattr(F._lib.load(), "frcnn_proposal_targets_batch")
    assert len(set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))) == 143
    for fn in ("objective_hip.lua", "frcnn_shims.lua.in"):
        assert "frcnn_proposal_targets_batch" in open(os.path.join(ROOT, "bindings", fn)).read(), fn
    assert callable(F.proposal_targets) and callable(F.roi_sampling_settings)
