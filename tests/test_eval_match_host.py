"""Detections matched to ground truth for mean average precision (Detector.match_batch, frcnn_eval_match_batch): everything that
needs no GPU.
  * the numpy restatement (tests/eval_match_ref.py, the literal greedy loop) against evaluation.mean_average_precision and
    mean_average_precision_range on seeded sets with heavy confidence ties: AP dicts and tp / fp totals equal with ==
  * evaluation.average_precision_from_matches against the same, whole dicts with ==
  * the hand cases by their hand-computed masks, boxes and overlaps
  * every argument error of the two entry points, returned without a device; the host mirror's refusals
  * the header, _lib.EVAL_SIGS and the Lua binding's sixth cdef declare the same functions; the Lua drop-in carries the path"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = 12
FRAMES = 3


def _rect(F, row):
    return F.Rect(*[np.float64(v) for v in row])      # (numpy scalars: an empty pair gives NaN, as a winner's r2 does)


def _dataset(F, seed, ties=True):
    """FRAMES seeded frames -> (frames, detections and ground truth as evaluation.mean_average_precision takes them, the
    ground truth per frame as match_batch takes it)"""
    frames = [R.frame(1000 * seed + f, n=40 + 7 * f, G=6 + f, ties=ties) for f in range(FRAMES)]
    dets, gt, per_frame = [], [], []
    for f, fr in enumerate(frames):
        for k in range(len(fr["classes"])):
            dets.append((f, int(fr["classes"][k]), float(fr["conf"][k]), _rect(F, fr["rects"][k])))
        boxes = [(int(c), _rect(F, r)) for c, r in zip(fr["gt_classes"], fr["gt_rects"])]
        per_frame.append(boxes)
        gt += [(f, c, r) for c, r in boxes]
    return frames, dets, gt, per_frame


def _matches(frames, thr):
    out = []
    for fr in frames:
        m = R.match_frame(fr["rects"], fr["classes"], fr["conf"], fr["gt_rects"], fr["gt_classes"], thr)
        out.append(dict(cls=fr["classes"], confidence=fr["conf"], tp=m["tp"], gt=m["gt"], iou=m["iou"]))
    return out


def _ap_by_hand(F, matches, per_frame, bit, use_07=False):
    """AP per class and the totals from the masks, in plain loops: the curve code of mean_average_precision on given flags"""
    npos = {}
    for boxes in per_frame:
        for c, _ in boxes:
            npos[c] = npos.get(c, 0) + 1
    ap, tps, fps = {}, 0, 0
    for c in sorted(npos):
        dets = [(float(m["confidence"][k]), int(m["tp"][k]) >> bit & 1) for m in matches for k in range(len(m["cls"])) if m["cls"][k] == c]
        dets.sort(key=lambda d: -d[0])
        tp = np.array([d[1] for d in dets], np.float64); fp = 1.0 - tp
        ctp, cfp = np.cumsum(tp), np.cumsum(fp)
        ap[c] = F.evaluation.voc_ap(ctp / float(npos[c]), ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps), use_07) if dets else 0.0
        tps += int(tp.sum()); fps += int(fp.sum())
    return ap, tps, fps


@pytest.mark.parametrize("seed", range(SETS))
def test_the_restatement_is_the_greedy_loop_of_mean_average_precision(F, seed):
    frames, dets, gt, per_frame = _dataset(F, seed)
    thr = R.IOU_RANGE
    matches = _matches(frames, thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = F.mean_average_precision_range(dets, gt, thr)
    for bit, t in enumerate(thr):
        w = want["by_iou"][t]
        ap, tps, fps = _ap_by_hand(F, matches, per_frame, bit)
        assert ap == w["ap"] and (tps, fps) == (w["tp"], w["fp"]), t
        if bit == 0:
            assert tps > 0 and fps > 0, "a set without true or without false positives shows little"
    # a confidence tie decided an outcome somewhere: the sets do exercise the order
    assert len({float(c) for fr in frames for c in fr["conf"]}) < 10


@pytest.mark.parametrize("seed", range(SETS))
@pytest.mark.parametrize("use_07", [False, True])
def test_average_precision_from_matches_equals_the_host_functions(F, seed, use_07):
    frames, dets, gt, per_frame = _dataset(F, seed, ties=seed % 2 == 0)
    thr = R.IOU_RANGE
    with np.errstate(divide="ignore", invalid="ignore"):
        want_range = F.mean_average_precision_range(dets, gt, thr, use_07)
        want_one = F.mean_average_precision(dets, gt, 0.5, use_07)
    assert F.average_precision_from_matches(_matches(frames, thr), per_frame, thr, use_07) == want_range
    assert F.average_precision_from_matches(_matches(frames, [0.5]), per_frame, 0.5, use_07) == want_one
    assert want_one["tp"] > 0 and want_one["fp"] > 0
    # objects with .class_index and .rect, what nextValidation hands out, are ground truth too
    rois = [[F.Roi(r, c) for c, r in boxes] for boxes in per_frame]
    assert F.average_precision_from_matches(_matches(frames, [0.5]), rois, 0.5, use_07) == want_one


def test_average_precision_from_matches_edges(F):
    none = dict(cls=np.zeros(0, np.int32), confidence=np.zeros(0, np.float32), tp=np.zeros(0, np.uint32))
    gt = [[(2, F.Rect(0, 0, 1, 1))], []]
    assert F.average_precision_from_matches([none, none], gt, 0.5) == F.mean_average_precision([], [(0, 2, gt[0][0][1])], 0.5)
    with pytest.raises(ValueError):
        F.average_precision_from_matches([none], gt, 0.5)
    with pytest.raises(ValueError):
        F.average_precision_from_matches([none, none], gt, [])


@pytest.mark.parametrize("case", R.HAND, ids=[c["name"] for c in R.HAND])
def test_hand_cases(case):
    m = R.match_frame(case["rects"], case["classes"], case["conf"], case["gt_rects"], case["gt_classes"], case["thr"])
    assert m["tp"].tolist() == case["tp"] and m["gt"].tolist() == case["gt"]
    assert m["iou"].tolist() == case["iou"]


def test_the_two_identities_of_rect_iou(F):
    assert R.iou([0, 0, 2, 1], [0, 0, 1, 1]) == 0.5 == F.Rect.IoU(F.Rect(0, 0, 2, 1), F.Rect(0, 0, 1, 1))
    assert np.isnan(R.iou([0, 0, 0, 0], [3, 3, 3, 3]))
    rng = np.random.RandomState(4)
    for _ in range(200):
        (ax, ay, bx, by) = np.sort(rng.uniform(0, 50, (4, 2)), axis=1)
        a, b = [ax[0], ay[0], ax[1], ay[1]], [bx[0], by[0], bx[1], by[1]]
        assert R.iou(a, b) == F.Rect.IoU(_rect(F, a), _rect(F, b))


def test_keep_best_is_the_detectors(F):
    from frcnn_amd.Detector import keep_best
    conf = R.frame(3, 200, 5)["conf"]
    for M in (1, 17, 199, 200, 500):
        assert R.keep_best(conf, M).tolist() == keep_best(conf, M).tolist()


# ------------------------------------------------------------------------------------------------------ the entry points' errors
def test_argument_errors_are_returned_before_any_launch(F):
    """every refused call returns an error code with a message; the pointers are never dereferenced (they are not device memory
    here)"""
    lib = F._lib.load()
    p = C.c_void_p(0x1000)
    row0 = (C.c_longlong * 4)(0, 5, 5, 9)
    thr = (C.c_double * 16)(*([0.5] * 16))

    def call(rec=p, B=3, rs=64, sel=None, ss=0, kd=None, gr=p, gc=p, row0=row0, thr=thr, T=2, match=p, iou=p):
        return lib.frcnn_eval_match_batch(rec, B, rs, sel, ss, kd, gr, gc, row0, thr, T, match, iou, None)

    nan = (C.c_double * 16)(*([0.5] * 16)); nan[1] = float("nan")
    bad = [dict(B=-1), dict(B=65536), dict(rs=-1), dict(rs=(1 << 27) + 1), dict(T=0), dict(T=17), dict(T=-3), dict(thr=None), dict(thr=nan),
           dict(ss=-1), dict(rec=None), dict(match=None), dict(row0=None), dict(sel=p), dict(kd=p), dict(sel=p, kd=C.c_void_p(0x1002), ss=8),
           dict(row0=(C.c_longlong * 4)(0, 5, 4, 9)), dict(row0=(C.c_longlong * 4)(-1, 5, 5, 9)), dict(row0=(C.c_longlong * 4)(0, 5, 5, 1031)),
           dict(gr=None), dict(gc=None), dict(rec=C.c_void_p(0x1004)), dict(match=C.c_void_p(0x1008)), dict(iou=C.c_void_p(0x1004)),
           dict(gr=C.c_void_p(0x1004)), dict(gc=C.c_void_p(0x1002))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.frcnn_last_error().decode().startswith("eval_match_batch"), kw
    # nothing to do: no launch, no error -- also with every array NULL; no ground truth at all needs no arrays
    assert call(B=0) == 0 and call(B=0, rec=None, match=None, row0=None, gr=None, gc=None, iou=None) == 0
    with pytest.raises(F.FrcnnError, match="thresholds"):
        F._lib.call("frcnn_eval_match_batch", p, 3, 64, None, 0, None, p, p, row0, thr, 17, p, p, None)

    def conf(rec=p, B=3, rs=64, out=p, cnt=p):
        return lib.frcnn_eval_conf_rows(rec, B, rs, out, cnt, None)
    for kw in (dict(B=-1), dict(B=65536), dict(rs=-1), dict(rs=(1 << 27) + 1), dict(rec=None), dict(out=None), dict(cnt=None),
               dict(rec=C.c_void_p(0x1004)), dict(out=C.c_void_p(0x1002)), dict(cnt=C.c_void_p(0x1001))):
        assert conf(**kw) != 0, kw
        assert lib.frcnn_last_error().decode().startswith("eval_conf_rows"), kw
    assert conf(B=0) == 0 and conf(B=0, rec=None, out=None, cnt=None) == 0


def test_the_host_mirror_refuses_before_the_device_is_touched(F):
    with pytest.raises(ValueError, match="bogus"):
        F.evaluate_detections(None, None, 4, match="bogus")
    with pytest.raises(ValueError):
        F.evaluate_detections(None, None, 4, match=None)
    frame = np.zeros((3, 8, 8), np.float32)
    nobody = object()      # (no Detector: every refusal below comes before the first use of one)
    box = (1, F.Rect(0, 0, 1, 1))
    for args, kw in ((([frame], []), {}), (([frame], [[box]]), dict(iou_thresholds=())), (([frame], [[box]]), dict(iou_thresholds=[0.5] * 17)),
                     (([frame], [[box]]), dict(iou_thresholds=[0.5, float("nan")])), (([frame], [[box] * 1025]), {})):
        with pytest.raises(ValueError, match="match_batch"):
            F.Detector.match_batch(nobody, *args, **kw)
    with pytest.raises(ValueError):
        F.eval_match(np.zeros((2, 4)), [1], [0.5, 0.5], np.zeros((0, 4)), [], [0.5])
    with pytest.raises(ValueError):
        F.eval_match(np.zeros((1, 4)), [1], [0.5], np.zeros((1, 4)), [], [0.5])


def test_table_helpers_round_trip(F):
    from frcnn_amd.nms import unpack_match, winner_table
    fr = R.frame(1, 9, 3)
    tab = winner_table(fr["rects"], fr["classes"], fr["conf"], row_stride=12)
    assert tab.shape == (13, 16) and tab[0].view(np.int32)[3] == 9 and not tab[10:].any()
    assert tab[1:10, 8:12].tobytes() == fr["rects"].tobytes() and (tab[1:10, 2].astype(np.float32) == fr["conf"]).all()
    want, io = R.table(fr, [0.5, 0.7])
    u = unpack_match(np.concatenate([want, np.full((3, 4), -7, np.int32)]), np.concatenate([io, [9.0] * 3]))
    assert u["n"] == 9 and u["G"] == 3 and u["T"] == 2 and u["winners"] == 9
    assert u["cls"].tolist() == fr["classes"].tolist() and u["confidence"].tobytes() == fr["conf"].tobytes()
    assert u["tp"].tolist() == want[2:, 2].tolist() and u["gt"].tolist() == want[2:, 3].tolist() and u["iou"].tolist() == io.tolist()


# ------------------------------------------------------------------------------------------------------------ the declarations
def _symbols(text):
    return set(re.findall(r"\b(frcnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_entry_points_are_declared_for_both_hosts(F):
    """the two entry points live in include/frcnn_hip_eval.h, which frcnn_hip.h includes: the library exports them, the host
    mirror's sixth ctypes table and the Lua binding's sixth generated cdef declare exactly them with the header's argument counts,
    and the Lua files call them through the CE handle only"""
    names = {"frcnn_eval_match_batch", "frcnn_eval_conf_rows"}
    main = open(os.path.join(ROOT, "include", "frcnn_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "frcnn_hip_eval.h")).read()
    assert '#include "frcnn_hip_eval.h"' in main and not names & _symbols(main)
    assert _symbols(hdr) == names == set(F._lib.EVAL_SIGS)
    others = (set(F._lib.exported_symbols()) | set(F._lib.HARD_SIGS) | set(F._lib.LOSS_SIGS) | set(F._lib.BOX_SIGS) | set(F._lib.CLASSBOX_SIGS)
              | set(F._lib.HEADS_SIGS))
    assert not names & others
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("frcnn_eval_match_batch", 14), ("frcnn_eval_conf_rows", 6)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, code, re.M)
        assert m and len(m.group(1).split(",")) == len(F._lib.EVAL_SIGS[name][0]) == nargs, name
    lib = C.CDLL(F._lib.SO_PATH)
    assert all(hasattr(lib, n) for n in names) and all(getattr(F._lib.load(), n).argtypes for n in names)
    lua = open(os.path.join(ROOT, "bindings", "frcnn_hip.lua")).read()
    sixth = re.findall(r"ffi\.cdef \[==\[(.*?)\]==\]", lua, re.S)
    assert len(sixth) == 1 and _symbols(sixth[0]) == names
    for name in names:
        h = re.sub(r"\s+", " ", re.search(r"int %s\([^;]*\);" % name, code).group(0))
        assert h in re.sub(r"\s+", " ", sixth[0]), name
    first = lua[lua.index("ffi.cdef[["):lua.index("]]")]
    assert not names & _symbols(first)
    used = set()
    for fn in ("frcnn_hip.lua", "objective_hip.lua", "Detector_hip.lua", "frcnn_shims.lua.in"):
        txt = open(os.path.join(ROOT, "bindings", fn)).read()
        used |= set(re.findall(r"\bCE\.(frcnn_[a-z0-9_]+)", txt))
        for n in names:
            assert not re.search(r"\bC[HLBX]?\.%s\b" % n, txt), (fn, n)
    assert used == names
    assert "eval_match.hip" in open(os.path.join(ROOT, "build_lib.sh")).read()
    for name in ("eval_match", "average_precision_from_matches"):
        assert name in F.__all__ and callable(getattr(F, name))
    # counted with the NMS kernels, like box voting; fp64 with contraction off; no atomics
    src = open(os.path.join(ROOT, "faster-rcnn.torch_amd", "csrc", "eval_match.hip")).read()
    assert src.count("FR_LAUNCH(KC_NMS") == 3 and "#pragma clang fp contract(off)" in src
    assert "atomic" not in src.replace("no atomics", "")


def test_the_lua_drop_in_carries_the_path():
    det = open(os.path.join(ROOT, "bindings", "Detector_hip.lua")).read()
    shim = open(os.path.join(ROOT, "bindings", "frcnn_shims.lua.in")).read()
    assert "M.CE = C" in shim
    for text in ("function Detector:match_batch(inputs, ground_truth, opts)", "function Detector:match_tables(match, out, B, rows, prefix)",
                 "function Detector.average_precision_from_matches(matches, ground_truth, thresholds, use_07_metric)",
                 "function Detector:evaluate_detections(frames, ground_truth, opts)", "function Detector:detect_chunk(frames, shared, prefix, match)",
                 "CE.frcnn_eval_conf_rows(out, B, rows, conf, wcnt, nil)",
                 "CE.frcnn_eval_match_batch(out, B, rows, sel, kcap, kd, drect, dcls, row0, thr, T, ffi.cast('int*', dev), diou, nil)",
                 "how ~= 'host' and how ~= 'device'"):
        assert text in det, text
    # behind the gather, in place of the winner tables' read-back; the selection in front of the match
    chunk = det[det.index("function Detector:detect_chunk("):]
    assert chunk.index("C.frcnn_detect_gather_batch(") < chunk.index("self:match_tables(match, out, B, rows, prefix)") < chunk.index("C.frcnn_memcpy_d2h(h, out")
    tabs = det[det.index("function Detector:match_tables("):det.index("function Detector.average_precision_from_matches(")]
    assert tabs.index("CE.frcnn_eval_conf_rows(") < tabs.index("C.frcnn_topk_select(conf") < tabs.index("CE.frcnn_eval_match_batch(")
    assert tabs.count("C.frcnn_stream_sync(nil)") == 1 and tabs.count("C.frcnn_memcpy_d2h(") == 1


def test_the_documents_name_the_path(F):
    for fn in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, fn)).read()
        assert "frcnn_eval_match_batch" in txt and "match_batch" in txt, fn
    assert "device" in F.evaluate_detections.__doc__ and "match_batch" in F.evaluate_detections.__doc__
