"""Detector -- host-side mirror of Detector.lua.  detect(input) keeps the reference's pipeline and
thresholds (p > 0.95, NMS 0.25, class != background and p > 0.2, per-class NMS 0.1) but the 26 544
iteration Lua loop of Detector.lua:39-66 is one scan+compaction kernel (frcnn_rpn_scan_batch), the per-ROI
pooling loop (:94-98) one batched kernel, and both NMS passes run on the device.  Note that both NMS
calls of the reference pass a tensor as `scores`, which nms.lua:37-43 ignores: boxes are processed
by descending max-y.  That behaviour is reproduced.

The frame stays on the device between its big steps: scan -> NMS (the match count is read by the NMS kernels from
device memory), ONE read-back of two counts (the cnet's row count sizes its launches), then ROI windows -> ROI pooling
-> cnet -> class test + rect decode + ordered compaction -> per-class NMS -> one record per winner, and ONE read-back
of the winner table.  The list detect() returns builds its {p, a, r, l, r2, class, confidence} tables on access.

There is ONE pipeline, written for a chunk of B frames (_first_stage + _detect_chunk: ONE scan, frcnn_nms_device_batch twice,
frcnn_detect_gather_batch; frcnn_nms_device for a frame over the first NMS's bound), with ONE front: every frame's slot
offsets, feature-map shape and anchor count come from its size's layout (_layout, host arithmetic, cached per size), the
chunk's strides are those of its largest frame, and the shapes pick the scan -- frcnn_rpn_scan_batch for a chunk of one size,
frcnn_rpn_scan_ragged for one that mixes sizes under detect_batch(mixed_sizes=True).
detect_batch(frames) runs it on chunks of BATCH frames, detect(input) on the chunk [input], proposals(input) runs its first
stage on [input].  A chunk of one frame reads the proposal net's outputs where the model left them: no device copies.

Not in the reference, off by default (cfg["proposals"] / Detector(..., proposals=...), see proposal_settings): the proposal
layer's two caps and score-ordered NMS.  pre_nms_top_n = K keeps the K best-scoring matches in front of the first NMS
(frcnn_topk_select + frcnn_rpn_gather_rows: the selected rows keep their scan order, everything downstream runs unchanged on
compact arrays, the first NMS is sized by min(anchors, K)); order = "score" keys both NMS passes by the score instead of max-y;
post_nms_top_n = M keeps the first min(R, M) picks of the first NMS.

Not in the reference either, off by default (cfg["nms"] / Detector(..., nms=...), see nms_settings): Soft-NMS in the per-class
pass (step 5 of _detect_chunk; the first NMS is untouched).  Under method "linear" or "gaussian" the neighbours of a winner keep
living with a lowered confidence instead of being deleted (frcnn_soft_nms_batch in place of frcnn_nms_device_batch, on the
log-probabilities the class test produced: log_domain 1).  A winner's `confidence` is then its DECAYED log-score, the one it
was ranked by; the undecayed one remains last_cnet["cls"][candidate - 1, class - 1].

Nor is box voting (Gidaris & Komodakis 2015), off by default (cfg["box_voting"] / Detector(..., box_voting=...), see
box_voting_settings): behind the per-class pass ONE frcnn_box_vote_batch launch replaces every winner's r2 by the weighted mean
of the r2 of the class test's survivors of its class that overlap it by at least `overlap` (weights: the confidences, always the
UNDECAYED ones).  Which rows win, their order and every other field of a winner are those of the same Detector without the key.

Nor is scoring a candidate under more than its arg-max class, off by default (cfg["scoring"] / Detector(..., scoring=...), see
scoring_settings): with the key the class test of a chunk is ONE frcnn_detect_classes_batch launch in place of two per frame, its
threshold is min_confidence, and under classes = "all" a candidate yields one row per foreground class over the threshold -- the
rows the per-class NMS, voting and the gather then work on; several winners may share a candidate (field `candidate`), with
bit-identical r2 unless voted.  max_detections caps a frame's winners on the host.  On a per-class box head (cfg["box_head"])
boxes = "class" (scoring_boxes) gives every such row the box of ITS class: one frcnn_detect_class_boxes_batch launch behind the
class test, on the box head's input kept from every pass (cnet.features).

Nor is test-time augmentation, off by default (cfg["tta"] / Detector(..., tta=...), see tta_settings): a frame is detected on V
views of itself -- per scale the rescaled frame (frcnn_image_scale) and, under hflip, its mirror (frcnn_image_crop_flip) -- which
are the SEGMENTS of the chunk: steps 1-4 run on them as they run on frames.  Behind the class test ONE frcnn_detect_merge_views
launch turns the survivors of a frame's views into one segment in the frame's coordinates, on which the per-class pass (hard,
soft, voting) and the gather run unchanged: winners compete, and vote, across views.  A detection gains `view`; its r2 is in the
frame's coordinates, its p, r and a describe the anchor in the VIEW's coordinates, its candidate indexes the concatenation of the
views' classification-net outputs.

Nor is match_batch(frames, ground_truth, iou_thresholds): detect_batch's pipeline up to and including the gather, then the winners
matched to the frames' ground truth on the device for mean average precision (max_detections by frcnn_eval_conf_rows +
frcnn_topk_select, ONE frcnn_eval_match_batch), and read-back 2 of 16 bytes a row -- class, confidence, a true-positive bit per
threshold, matched box -- in place of the 128-byte records.  detect_batch itself launches, allocates and returns what it did."""
import collections
import ctypes as C
import math

import os

import numpy as np

from . import _lib
from .Anchors import Anchors
from .Localizer import Localizer
from .Rect import Rect
from .nms import SOFT_NMS_METHODS, nms
from .objective import align_geometry, roi_pooling_settings, roi_window, roi_windows
from .tensor import DeviceTensor, ptr, stream_ptr, to_device

ASPECTS = 3   # anchors per map position (Anchors.lua:108-109)

PROPOSAL_DEFAULTS = dict(order="y2", pre_nms_top_n=None, post_nms_top_n=None)


def _settings_table(cfg_or_table, name, defaults, optional=False):
    """The table cfg[name] of a model's cfg -- or the table itself, or None -- refused (ValueError) unless it is a table with
    keys of `defaults` only: the prologue of the four validators below.  An absent key or None is {} -- or, optional=True, None:
    the feature is off."""
    t = cfg_or_table
    if isinstance(t, dict) and (name in t or "class_count" in t):     # a model's cfg
        t = t.get(name)
    if t is None:
        if optional:
            return None
        t = {}
    if not isinstance(t, dict):
        raise ValueError("cfg.%s must be a table of {%s}" % (name, ", ".join(defaults)))
    unknown = sorted(set(t) - set(defaults), key=str)
    if unknown:
        raise ValueError("cfg.%s: unknown key(s) %s" % (name, ", ".join(map(str, unknown))))
    return t


def _number(name, key, v):
    """cfg.<name>.<key> = v as a float; refused (ValueError) when it is a bool or not a number."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("cfg.%s.%s = %r is not a number" % (name, key, v))
    return float(v)


def _count(name, key, v):
    """cfg.<name>.<key> = v as None or an int; refused (ValueError) unless it is None or an integer (no bool) of at least 1."""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("cfg.%s.%s = %r is not an integer" % (name, key, v))
    if v < 1:
        raise ValueError("cfg.%s.%s = %d (at least 1)" % (name, key, v))
    return int(v)


def proposal_settings(cfg_or_table):
    """cfg["proposals"] -- or the table itself, or None -- -> (order, pre_nms_top_n, post_nms_top_n), validated on the host.
      order           "y2" (default: the reference -- nms.lua ignores the scores it is handed, boxes go by descending max-y) or
                      "score": the first NMS runs on rows {box, p} keyed by p (key_mode 2, key_col 5), the per-class NMS keyed
                      by the confidence (key_col 5); the NMS tie rule is unchanged
      pre_nms_top_n   None or K >= 1: only the K' = min(n, K) best-ranked of a frame's n matches reach the first NMS.  Rank:
                      the match's fp32 p compared as a value (-0 equals +0, a NaN ranks below everything), ties are broken by
                      the lower scan row.  The selected rows keep their scan order, so K >= n changes nothing.  Either order.
      post_nms_top_n  None or M >= 1: the candidates are the first min(R, M) picks of the first NMS.  Needs order = "score": the
                      first M picks in max-y order are not the best M.
    Raises ValueError (before any device call) for an unknown key, an unknown order, a bool or non-integer or < 1 cap, and
    post_nms_top_n without order = "score"."""
    t = _settings_table(cfg_or_table, "proposals", PROPOSAL_DEFAULTS)
    order = t.get("order", "y2")
    if not isinstance(order, str) or order not in ("y2", "score"):
        raise ValueError("cfg.proposals.order = %r (\"y2\" or \"score\")" % (order,))
    pre_n, post_n = (_count("proposals", k, t.get(k)) for k in ("pre_nms_top_n", "post_nms_top_n"))
    if post_n is not None and order != "score":
        raise ValueError("cfg.proposals.post_nms_top_n needs order = \"score\": the first picks in max-y order are not the best")
    return order, pre_n, post_n


NMS_DEFAULTS = dict(method="hard", overlap=0.1, sigma=0.5, min_score=0.001)


def nms_settings(cfg_or_table):
    """cfg["nms"] -- or the table itself, or None -- -> (method, overlap, sigma, min_score, overlap_given), validated on the host.
    The setting governs the per-class pass only (Detector.lua:125-136); the first NMS is untouched.
      method     "hard" (default: the reference -- a box that overlaps a better one of its class by more than `overlap` is
                 deleted), "linear" (its confidence is multiplied by 1 - IoU instead) or "gaussian" (every box of the class has
                 its confidence multiplied by exp(-IoU^2 / sigma)); a box is dropped when its confidence falls below min_score
      overlap    Nt, in (0, 1]; default 0.1 (the reference's threshold).  "hard" without it: the parent's launches and results
                 exactly; "hard" with it: the same kernels with that threshold
      sigma      > 0; default 0.5
      min_score  in [0, 1), a probability; default 0.001.  0 keeps every class-test survivor
    Raises ValueError (before any device call) for an unknown key, an unknown method, a bool or a non-number, and a value
    outside its range."""
    t = _settings_table(cfg_or_table, "nms", NMS_DEFAULTS)
    method = t.get("method", NMS_DEFAULTS["method"])
    if not isinstance(method, str) or method not in SOFT_NMS_METHODS:
        raise ValueError("cfg.nms.method = %r (\"hard\", \"linear\" or \"gaussian\")" % (method,))
    overlap, sigma, min_score = (_number("nms", k, t.get(k, NMS_DEFAULTS[k])) for k in ("overlap", "sigma", "min_score"))
    if not (0.0 < overlap <= 1.0):
        raise ValueError("cfg.nms.overlap = %r (in (0, 1])" % (overlap,))
    if not (sigma > 0.0) or math.isinf(sigma):
        raise ValueError("cfg.nms.sigma = %r (> 0)" % (sigma,))
    if not (0.0 <= min_score < 1.0):
        raise ValueError("cfg.nms.min_score = %r (in [0, 1))" % (min_score,))
    return method, overlap, sigma, min_score, "overlap" in t


BOX_VOTING_DEFAULTS = dict(overlap=0.5, weight="score")
BOX_VOTING_WEIGHTS = dict(uniform=0, score=2)   # weight_mode of frcnn_box_vote_batch: bb's column 5 is a log-probability


def box_voting_settings(cfg_or_table):
    """cfg["box_voting"] -- or the table itself, or None -- -> None (the key is absent: no voting, the reference's r2) or
    (overlap, weight), validated on the host.  Voting runs behind the per-class pass (step 5 of _detect_chunk) and changes a
    winner's r2 only: it becomes the weighted mean of the r2 of every survivor of the class test that has the winner's class
    and overlaps it (IoU of the fp32 boxes, the per-class NMS's own arithmetic) by at least `overlap`, the winner included.
      overlap  in (0, 1]; default 0.5
      weight   "score" (default: a voter weighs its confidence as a probability, exp of the log-confidence -- the undecayed
               one, also under a soft per-class NMS) or "uniform" (every voter weighs 1)
    An empty table turns voting on with the defaults.  Raises ValueError (before any device call) for an unknown key, an
    unknown weight, a bool or a non-number, and an overlap outside (0, 1]."""
    t = _settings_table(cfg_or_table, "box_voting", BOX_VOTING_DEFAULTS, optional=True)
    if t is None:
        return None
    weight = t.get("weight", BOX_VOTING_DEFAULTS["weight"])
    if not isinstance(weight, str) or weight not in BOX_VOTING_WEIGHTS:
        raise ValueError("cfg.box_voting.weight = %r (\"score\" or \"uniform\")" % (weight,))
    overlap = _number("box_voting", "overlap", t.get("overlap", BOX_VOTING_DEFAULTS["overlap"]))
    if not (0.0 < overlap <= 1.0):
        raise ValueError("cfg.box_voting.overlap = %r (in (0, 1])" % (overlap,))
    return overlap, weight


SCORING_DEFAULTS = dict(classes="top", min_confidence=0.2, max_detections=None, boxes="candidate")
SCORING_MODES = dict(top=0, all=1)   # mode of frcnn_detect_classes_batch
SCORING_BOXES = ("candidate", "class")


def scoring_settings(cfg_or_table):
    """cfg["scoring"] -- or the table itself, or None -- -> None (the key is absent: the reference's class test, launch for
    launch) or (classes, min_confidence, max_detections), validated on the host.  The setting governs the class test between the
    classification net and the per-class NMS (step 4 of _detect_chunk), which under it is ONE frcnn_detect_classes_batch launch
    per chunk.
      classes         "top" (default: the reference -- a candidate is scored under the arg-max of its log-probabilities only, and
                      dropped when that is the background) or "all": one row per foreground class whose probability clears
                      min_confidence, whatever the arg-max is; the per-class NMS, voting and the records then work on those rows
      min_confidence  in [0, 1), a probability; default 0.2 (the reference's literal).  A row needs exp(log-probability) > it
      max_detections  None or M >= 1: a frame keeps the M winners of highest confidence (compared as fp32 values, ties to the
                      earlier pick), applied on the host behind read-back 2
    An empty table is "top" at 0.2: the results of the key absent, from one launch.  Raises ValueError (before any device call)
    for an unknown key, an unknown classes, a bool or a non-number, a min_confidence outside [0, 1) and a max_detections that is
    not an integer >= 1.  The table's fourth key, boxes, is not part of the tuple: scoring_boxes validates and returns it."""
    t = _settings_table(cfg_or_table, "scoring", SCORING_DEFAULTS, optional=True)
    if t is None:
        return None
    classes = t.get("classes", SCORING_DEFAULTS["classes"])
    if not isinstance(classes, str) or classes not in SCORING_MODES:
        raise ValueError("cfg.scoring.classes = %r (\"top\" or \"all\")" % (classes,))
    min_confidence = _number("scoring", "min_confidence", t.get("min_confidence", SCORING_DEFAULTS["min_confidence"]))
    if not (0.0 <= min_confidence < 1.0):
        raise ValueError("cfg.scoring.min_confidence = %r (in [0, 1))" % (min_confidence,))
    return classes, min_confidence, _count("scoring", "max_detections", t.get("max_detections"))


def scoring_boxes(cfg_or_table):
    """cfg["scoring"]["boxes"] -- of a cfg, of the table itself, or of None -- -> "candidate" or "class", validated on the host.
      boxes  "candidate" (default, also without the table): a candidate has ONE box, the one the classification net wrote for it,
             and under classes = "all" every class row of the candidate carries it;
             "class": every emitted row (candidate r, class c) carries the box that class c's four regressor rows predict for
             candidate r -- ONE frcnn_detect_class_boxes_batch launch per chunk behind the class test (step 4 of _detect_chunk).
             Needs a per-class box head (cfg["box_head"]["per_class"]: Detector.set_scoring and box_head_settings refuse it on a
             shared one).  Under classes = "top" a row's class is the arg-max, whose box the net wrote already: accepted, and
             the launches are those of "candidate".
    Raises ValueError (before any device call) for any other value, a bool or a non-string, and whatever is wrong with the table's
    shape (scoring_settings validates the other keys)."""
    t = _settings_table(cfg_or_table, "scoring", SCORING_DEFAULTS, optional=True)
    if t is None:
        return SCORING_DEFAULTS["boxes"]
    boxes = t.get("boxes", SCORING_DEFAULTS["boxes"])
    if not isinstance(boxes, str) or boxes not in SCORING_BOXES:
        raise ValueError("cfg.scoring.boxes = %r (\"candidate\" or \"class\")" % (boxes,))
    return boxes


TTA_DEFAULTS = dict(hflip=False, scales=[1.0])


def tta_settings(cfg_or_table):
    """cfg["tta"] -- or the table itself, or None -- -> None (the key is absent: one forward pass over the frame) or
    (hflip, scales), validated on the host.  Test-time augmentation: the frame is detected on V = len(scales) * (2 if hflip else
    1) views of itself (tta_views) and the per-class pass -- hard or soft NMS, voting -- runs over the union of what they found.
      hflip   False (default) or True: behind every scale's view comes its left-right mirror
      scales  a non-empty list of distinct positive numbers, default {1.0}: per scale s, in the order given, an H x W frame is
              rescaled to max(1, int(H * s)) x max(1, int(W * s)) (truncated, as BatchIterator.lua:52 does); s = 1 is the frame
    A table whose only view is the frame itself ({}, {scales = {1}}) is off: the launches and results of the key absent.  Raises
    ValueError (before any device call) for an unknown key, an hflip that is no bool, scales that are empty or no list, a scale
    that is a bool, no number, not finite or <= 0, and a scale given twice."""
    t = _settings_table(cfg_or_table, "tta", TTA_DEFAULTS, optional=True)
    if t is None:
        return None
    hflip = t.get("hflip", TTA_DEFAULTS["hflip"])
    if not isinstance(hflip, (bool, np.bool_)):
        raise ValueError("cfg.tta.hflip = %r (true or false)" % (hflip,))
    scales = t.get("scales", TTA_DEFAULTS["scales"])
    if not isinstance(scales, (list, tuple)) or len(scales) == 0:
        raise ValueError("cfg.tta.scales = %r (a non-empty list of numbers)" % (scales,))
    out = []
    for v in scales:
        v = _number("tta", "scales", v)
        if not math.isfinite(v) or v <= 0.0:
            raise ValueError("cfg.tta.scales: %r (finite and > 0)" % (v,))
        if v in out:
            raise ValueError("cfg.tta.scales: %r is given twice" % (v,))
        out.append(v)
    return bool(hflip), tuple(out)


def tta_views(settings, H, W):
    """The views of an H x W frame under settings = (hflip, scales) -- or None: the frame alone --, in segment order: a list of
    (scale, flip, dH, dW), scale-major, the unmirrored view first.  View (1.0, False, H, W) is the frame itself."""
    hflip, scales = settings or (False, (1.0,))
    out = []
    for sc in scales:
        dH, dW = (H, W) if sc == 1.0 else (max(1, int(H * sc)), max(1, int(W * sc)))
        out += [(sc, flip, dH, dW) for flip in ((False, True) if hflip else (False,))]
    return out


def scoring_rows(classes, min_confidence, ncls):
    """m: the rows a candidate can emit under a scoring setting, what the per-row buffers of a chunk are sized by (Rmax * m rows a
    frame).  "top": 1.  "all": min(ncls - 1, floor(1 / min_confidence) + 1) -- at most floor(1 / c) classes exceed c when the
    probabilities sum to 1, and one more slot covers the rounding of an fp32 log-softmax, whose exp need not sum to 1 exactly;
    ncls - 1 at min_confidence = 0."""
    if classes != "all":
        return 1
    if min_confidence <= 0.0:
        return ncls - 1
    return min(ncls - 1, int(math.floor(1.0 / min_confidence)) + 1)


def keep_best(conf, M):
    """max_detections: the rows (ascending) of the M highest values of conf, compared as fp32 values, ties to the earlier row."""
    c = np.asarray(conf).astype(np.float32)
    return np.sort(np.argsort(-c, kind="stable")[:M])


MATCH_MAX_THRESHOLDS = 16    # IoU thresholds of one match_batch call (a bit each of the tp mask)
MATCH_MAX_BOXES = 1024       # ground-truth boxes a frame (frcnn_eval_match_batch)


def _gt_arrays(boxes):
    """A frame's ground truth -- (class_index, Rect) pairs, or objects with .class_index and .rect (what nextValidation hands out)
    -> (classes int32[G], rects float64[G][4]), in the given order."""
    cls, rects = [], []
    for g in boxes:
        c, r = (g.class_index, g.rect) if hasattr(g, "rect") else (g[0], g[1])
        cls.append(int(c))
        rects.append((r.minX, r.minY, r.maxX, r.maxY) if hasattr(r, "minX") else tuple(float(v) for v in r))
    return np.array(cls, np.int32), np.array(rects, np.float64).reshape(-1, 4)


def _match_result(table, iou, with_iou):
    """One frame's result of match_batch from its table of frcnn_eval_match_batch ((rows + 2) x 4 int32; None: a frame without
    detections): dict(cls, confidence (float32), tp (uint32: bit t = a true positive at threshold t), gt (1-based, 0: none)[, iou])
    in the order of detect_batch's list -- classes ascending (a stable sort), the table's order within a class."""
    n = 0 if table is None else int(table[1, 0])
    rows = np.zeros((0, 4), np.int32) if table is None else table[2:2 + n]
    order = np.argsort(rows[:, 0], kind="stable")
    rows = np.ascontiguousarray(rows[order])
    out = dict(cls=rows[:, 0].copy(), confidence=rows[:, 1].copy().view(np.float32), tp=rows[:, 2].copy().view(np.uint32),
               gt=rows[:, 3].copy())
    if with_iou:
        out["iou"] = (np.zeros(0, np.float64) if iou is None else iou[:n][order]).copy()
    return out


class _Detections(object):
    """The list Detector:detect returns (Detector.lua:138-140): one table {p, a, r, l, r2, class, confidence} per winner,
    classes ascending (pairs() order is unspecified in Lua), pick order within a class.  Backed by the winner records the
    device wrote; a table is built when it is looked at."""

    def __init__(self, rec, anchors, roff=None):
        self._rec, self._anchors, self._roff = rec, anchors, roff   # roff (cfg.tta): the prefix sums of the views' candidate counts
        self._items = [None] * len(rec)

    def __len__(self):
        return len(self._items)

    def _make(self, q):
        x = self._items[q]
        if x is None:
            v = self._rec[q]
            idx = [int(t) for t in v[12:16]]
            x = dict(p=float(np.float32(v[3])), r=Rect(*v[4:8]), l=idx[0], a=self._anchors.get(*idx), r2=Rect(*v[8:12]),
                     confidence=float(np.float32(v[2])), candidate=int(v[1]), **{"class": int(v[0])})
            if self._roff is not None:     # the 0-based view the candidate came from
                x["view"] = int(np.searchsorted(self._roff, x["candidate"] - 1, side="right")) - 1
            self._items[q] = x
        return x

    def __getitem__(self, q):
        if isinstance(q, slice):
            return [self._make(t) for t in range(*q.indices(len(self)))]
        return self._make(q if q >= 0 else q + len(self))

    def __iter__(self):
        return (self._make(q) for q in range(len(self)))

    def __bool__(self):
        return len(self) > 0


def _frame_shape(x):
    """(3, H, W) of a frame as detect() accepts it, without touching the device."""
    shp = tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))
    if len(shp) != 3 or shp[0] != 3:
        raise ValueError("Detector: expected 3xHxW frames, got %r" % (shp,))
    return shp


def _map_hw(layers, H, W):
    """(h, w) of the output a layer list (rows kW, kH, dW, dH, padW, padH: a Localizer's) yields for an H x W input: per layer
    ceil((n + 2 pad - k) / d) + 1 -- the native model's arithmetic (stride-1 convolutions, ceil-mode 2x2 pooling)."""
    h, w = int(H), int(W)
    for l in layers:
        kW, kH, dW, dH, pW, pH = (int(v) for v in l[:6])
        h = -((h + 2 * pH - kH) // -dH) + 1
        w = -((w + 2 * pW - kW) // -dW) + 1
    return h, w


_Layout = collections.namedtuple("_Layout", "hw fshape hoff fslot anchors")


def _layout(layer_lists, planes, H, W):
    """What a frame of H x W occupies in a chunk, from the layer lists of the proposal net's outputs (the four head maps, then
    the last feature map, of `planes` planes) -- host arithmetic only, no pass: hw (the head maps' (h, w)), fshape (planes, fh,
    fw), hoff (the 5-entry prefix of the head maps' float counts, 18 planes each, every one rounded up to 64: where map i lies
    in the frame's slot, hoff[4] what the frame needs of it), fslot (likewise, the feature map) and anchors (of the four maps)."""
    hw = [_map_hw(l, H, W) for l in layer_lists]
    ceil64 = lambda n: (n + 63) // 64 * 64
    hoff = [0]
    for h, w in hw[:4]:
        hoff.append(hoff[-1] + ceil64(ASPECTS * 6 * h * w))
    fh, fw = hw[-1]
    return _Layout(hw[:4], (planes, fh, fw), hoff, ceil64(planes * fh * fw), ASPECTS * sum(h * w for h, w in hw[:4]))


def _chunk_slots(layouts):
    """(slot, fslot, cap) of a chunk: the strides (floats) of its head-map and feature-map slots and the row stride of its match
    arrays are those of its largest frame.  For a chunk of one size slot == hoff[4]."""
    return max(t.hoff[4] for t in layouts), max(t.fslot for t in layouts), max(t.anchors for t in layouts)


class _BatchRecord(object):
    """One frame's entry of Detector.last_batch, and what last_scan / last_pick / last_cnet / _last read after detect(): reads like a dict with the keys n, idx, box, rect, p (the frame's scan rows),
    pick (1-based candidate rows, pick order), cnet (dict bbox, cls; None for a frame without matches), kept; and pooled --
    the classification net's input rows, kept only by a shared_cnet pass and only for the last chunk of a call (else None).
    The arrays stay on the device and are fetched when they are looked at, like last_scan / last_pick / last_cnet of detect().
    Under pre_nms_top_n the scan rows are the SELECTED rows (n of them) and two more keys exist: row (their 1-based original
    scan rows) and matches (the frame's match count before the cap).  Under a soft per-class NMS (cfg["nms"]) two more: bb (K x 5:
    the class test's survivors {x1 y1 x2 y2 log-confidence} as the pass read them) and kc (K: their classes).  Under box voting
    (cfg["box_voting"]) those two and r2 (K x 4 float64: the survivors' UNVOTED decoded rects), keep_row (K: their 0-based
    candidate positions) and votes (K: the voter count of every row that won, 0 for the others): what it takes to recompute
    every winner's box."""
    _EXTRA = ("bb", "kc", "r2", "keep_row", "votes")    # of a soft pass (the first two) or of box voting (all)
    _KEYS = ("n", "idx", "box", "rect", "p", "pick", "cnet", "kept", "pooled")   # of every record

    def __init__(self, n, R, dev, matches=None):
        self._v = dict(n=n, R=R, kept=0)
        self._dev = dev      # name -> DeviceTensor (views of the chunk's buffers until detach())
        self._view = True
        if matches is not None:
            self._v["matches"] = matches

    def finish(self, kept, **extra):
        """What read-back 2 brings: the class test's survivor count, and -- a soft per-class NMS, box voting -- its rows as
        the pass read them (extra: device arrays of `kept` rows, names of _EXTRA)."""
        self._v["kept"] = kept
        self._dev.update(extra)

    def detach(self):
        """A private device copy of the frame's arrays (one allocation; the copies are queued on the stream, no wait): the
        chunk's buffers are about to be reused by the next chunk of the same call."""
        if not self._view:
            return
        self._view = False
        self._dev.pop("pooled", None)     # (R x 13 824 floats a frame: not carried over)
        off, total = {}, 0
        for k, t in self._dev.items():
            off[k] = total
            total += (t.nbytes + 255) // 256 * 256
        own = DeviceTensor.empty((max(total, 256),), np.uint8)
        for k, t in list(self._dev.items()):
            c = DeviceTensor(own.ptr + off[k], t.shape, t.dtype, owner=own)
            if t.nbytes:
                c.copy_(t)
            self._dev[k] = c

    def scan(self):
        """Detector.last_scan of the frame: n and the device arrays of its scan rows (row and matches under pre_nms_top_n)."""
        out = dict(n=self._v["n"], **{k: self._dev[k] for k in ("p", "idx", "rect", "box", "row") if k in self._dev})
        if "matches" in self._v:
            out["matches"] = self._v["matches"]
        return out

    def keys(self):
        """The keys of every record, then those of what this one holds: row, matches (pre_nms_top_n); bb, kc (a soft pass);
        bb, kc, r2, keep_row, votes (box voting)."""
        ks = list(self._KEYS)
        if "matches" in self._v:
            ks += ["row", "matches"]
        return ks + [k for k in self._EXTRA if k in self._dev]

    def get(self, k, default=None):
        return self[k] if k in self else default

    def __contains__(self, k):
        return k in self.keys()

    def __getitem__(self, k):
        v = self._v
        if k not in v:
            if k not in self:
                raise KeyError(k)
            if k == "pooled":
                v[k] = self._dev[k].numpy() if k in self._dev else None
            elif k == "cnet":
                v[k] = dict(bbox=self._dev["bbox"].numpy(), cls=self._dev["cls"].numpy()) if "bbox" in self._dev else None
            else:
                v[k] = self._dev[k].numpy()
        return v[k]


class _FrameRecord(_BatchRecord):
    """A frame's entry of Detector.last_batch under cfg["tta"]: ONE record for the frame's V views.  Keys: views (the V
    _BatchRecords of the views, in view order: each what a frame's record is without the key, its scan rows and picks in the
    VIEW's coordinates; a view's kept is counted from the merged keep_row when the views are looked at), roff (V + 1 prefix sums of
    the views' candidate counts), n (the views' matches, summed), pick (the frame's candidates: the views' picks concatenated,
    1-based rows of the frame's V * match-stride match rows, as frcnn_detect_merge_views rebased them), cnet (the views' outputs
    concatenated: what `candidate` indexes), kept (the merged survivor count K'), and always bb, kc, r2, keep_row -- the merged
    survivors as the per-class pass read them, r2 in the FRAME's coordinates, keep_row indexing the concatenated candidates --,
    votes under box voting."""
    _KEYS = ("n", "pick", "cnet", "kept", "views", "roff")

    def __init__(self, views, roff, dev):
        _BatchRecord.__init__(self, sum(r["n"] for r in views), int(roff[-1]), dev)
        self._v.update(views=views, roff=np.asarray(roff, np.int64))
        self._counted = False

    def detach(self):
        _BatchRecord.detach(self)
        for r in self._v["views"]:
            r.detach()

    def scan(self):
        """Detector.last_scan of the frame: n and the views' scans."""
        return dict(n=self._v["n"], views=[r.scan() for r in self._v["views"]])

    def keys(self):
        return list(self._KEYS) + [k for k in self._EXTRA if k in self._dev]

    def __getitem__(self, k):
        v = self._v
        if k == "pick" and k not in self._dev:      # (no view of the chunk had a match: nothing was merged)
            return np.zeros(0, np.int64)
        if k == "views" and not self._counted and "keep_row" in self._dev:
            self._counted = True
            per = np.bincount(np.searchsorted(v["roff"][:-1], self["keep_row"], side="right") - 1, minlength=len(v["views"]))
            for r, c in zip(v["views"], per.tolist()):
                r._v["kept"] = c
        if k == "cnet" and k not in v:
            parts = [r["cnet"] for r in v["views"] if r["cnet"] is not None]
            v[k] = dict((t, np.concatenate([p[t] for p in parts])) for t in ("bbox", "cls")) if parts else None
        return _BatchRecord.__getitem__(self, k)


class _DetectorType(type):
    """Detector(model, ..., box_voting=table, scoring=table, tta=table): the voting, scoring and augmentation settings are
    keywords of the class call, not of __init__, whose parameter list stays what it was.  A table is validated before anything is
    built -- before the model is looked at, let alone the device -- and set on the finished object; without it __init__ has read
    model["cfg"]["box_voting"] / model["cfg"]["scoring"] / model["cfg"]["tta"]."""

    def __call__(cls, *args, box_voting=None, scoring=None, tta=None, **kw):
        if box_voting is not None:
            box_voting_settings(box_voting)
        if scoring is not None:
            scoring_settings(scoring)
            scoring_boxes(scoring)
        if tta is not None:
            tta_settings(tta)
        d = super().__call__(*args, **kw)
        if box_voting is not None:
            d.set_box_voting(box_voting)
        if scoring is not None:
            d.set_scoring(scoring)
        if tta is not None:
            d.set_tta(tta)
        return d


class Detector(object, metaclass=_DetectorType):
    proposal_settings = staticmethod(proposal_settings)
    nms_settings = staticmethod(nms_settings)
    box_voting_settings = staticmethod(box_voting_settings)
    scoring_settings = staticmethod(scoring_settings)
    scoring_boxes = staticmethod(scoring_boxes)
    tta_settings = staticmethod(tta_settings)

    def __init__(self, model, static_weights=False, proposals=None, nms=None):  # Detector.lua:8-15
        """static_weights=True: the caller promises not to write the weight vector between detect() calls; the library then packs
        the convolution weights once instead of once per frame (option static_weights of the C ABI; a training-mode pass or
        another Detector(..., static_weights=...) drops the packs).
        proposals: a table as proposal_settings takes it; None: model["cfg"]["proposals"] (absent: the reference's behaviour).
        nms: the per-class NMS, a table as nms_settings takes it -- validated first, before the model is looked at; None:
        model["cfg"]["nms"] (absent: the reference's hard cut at 0.1).
        Box voting is model["cfg"]["box_voting"] (absent: none) unless the call names one: Detector(model, box_voting=table), a
        table as box_voting_settings takes it (see _DetectorType).  Likewise the class test: model["cfg"]["scoring"] (absent: the
        reference's) unless the call names one, Detector(model, scoring=table), a table as scoring_settings takes it.  Likewise
        test-time augmentation: model["cfg"]["tta"] (absent: none) unless the call names one, Detector(model, tta=table), a
        table as tta_settings takes it."""
        if nms is not None:
            nms_settings(nms)
        self.model = model           # (set_scoring looks at the model's box head)
        self.set_proposals(proposals if proposals is not None else model["cfg"])
        self.set_nms(model["cfg"])
        self.set_box_voting(model["cfg"])
        self.set_scoring(model["cfg"])
        self.set_tta(model["cfg"])
        if nms is not None:
            self.set_nms(nms)
        if static_weights or os.environ.get("FRCNN_STATIC_WEIGHTS"):
            _lib.call("frcnn_set_option", b"static_weights", 1)
        cfg = model["cfg"]
        self.anchors = Anchors(model["pnet"], cfg["scales"])
        self.localizer = Localizer(model["pnet"].outnode.children[-1])
        # cfg["roi_pooling"]: the grid and the region feature (roi_pooling_settings; "align" needs a centred backbone)
        self._roi_settings()
        self._loc_layers = np.array([[l["kW"], l["kH"], l["dW"], l["dH"], l["padW"], l["padH"]] for l in self.localizer.layers],
                                    dtype=np.int32).reshape(-1, 6)
        self._aw = DeviceTensor.from_numpy(self.anchors.w)
        self._ah = DeviceTensor.from_numpy(self.anchors.h)
        self._bufs = {}
        self._layouts = {}           # (H, W) -> _Layout: a frame size is worked out once (_layout_of)
        self._host = None            # page-locked landing buffer of the two read-backs
        self._host_bytes = 0
        self.verbose = False
        self.last_scan = None
        self._last = {}              # the last frame's _BatchRecord after detect() or proposals()
        self.last_batch = []

    def set_proposals(self, cfg_or_table):
        """Validates a table as proposal_settings takes it and makes it this Detector's setting from the next frame on."""
        self.proposal_order, self.pre_nms_top_n, self.post_nms_top_n = proposal_settings(cfg_or_table)

    def set_nms(self, cfg_or_table):
        """Validates a table as nms_settings takes it and makes it this Detector's per-class NMS from the next frame on."""
        self.nms_method, self.nms_overlap, self.nms_sigma, self.nms_min_score, _ = nms_settings(cfg_or_table)

    def set_box_voting(self, cfg_or_table):
        """Validates a table as box_voting_settings takes it and makes it this Detector's setting from the next frame on (None,
        or a cfg without the key: no voting)."""
        self.box_voting = box_voting_settings(cfg_or_table)

    def set_scoring(self, cfg_or_table):
        """Validates a table as scoring_settings takes it and makes it this Detector's class test from the next frame on (None,
        or a cfg without the key: the reference's, launch for launch); self.boxes is the table's boxes (scoring_boxes)."""
        scoring, boxes = scoring_settings(cfg_or_table), scoring_boxes(cfg_or_table)
        # a per-class box head (cfg.box_head) has one box per (candidate, class); classes = "all" decodes ONE box per candidate
        # for all its class rows: refused unless boxes = "class" asks for the row's own (frcnn_detect_class_boxes_batch)
        model = getattr(self, "model", None)
        wanted = boxes == "class" or (scoring is not None and scoring[0] == "all")     # (else the model is not looked at)
        per_class = wanted and model is not None and int(model["native"].desc.box_per_class)
        if boxes == "class" and model is not None and not per_class:
            raise _lib.FrcnnError("cfg.scoring.boxes = \"class\" needs cfg.box_head.per_class = true: a shared box head has one box "
                                  "per candidate")
        if scoring is not None and scoring[0] == "all" and per_class and boxes != "class":
            raise _lib.FrcnnError("cfg.scoring.classes = \"all\" cannot be combined with cfg.box_head.per_class = true: that pass decodes "
                             "one box per candidate for all its class rows; cfg.scoring.boxes = \"class\" gives every class row the "
                             "box of its own class")
        self.scoring, self.boxes = scoring, boxes

    def set_tta(self, cfg_or_table):
        """Validates a table as tta_settings takes it and makes it this Detector's setting from the next frame on (None, or a
        cfg without the key: no augmentation).  A table whose only view is the frame itself is kept as given and runs as None."""
        self.tta = tta_settings(cfg_or_table)

    def _view_lists(self, shapes):
        """cfg["tta"]: None when the setting is off -- absent, or the frame alone --, else one tta_views list per frame of
        `shapes` ((3, H, W) each).  Refused (ValueError), on the host: more views a frame than BATCH segments, and a view too
        small for the proposal net (a head map without positions)."""
        if self.tta is None or self.tta == (False, (1.0,)):
            return None
        lists = [tta_views(self.tta, H, W) for _, H, W in shapes]
        V = len(tta_views(self.tta, 1, 1))
        if V > max(int(self.BATCH), 1):
            raise ValueError("cfg.tta: %d views a frame, more than the %d segments of a chunk (Detector.BATCH)" % (V, self.BATCH))
        for vl in lists:
            for sc, _, dH, dW in vl:
                if any(h < 1 or w < 1 for h, w in self._layout_of(dH, dW).hw):
                    raise ValueError("cfg.tta: scale %r makes a %dx%d view, too small for the proposal net's head maps"
                                     % (sc, dW, dH))
        return lists

    def _make_views(self, frame, views, f, pre):
        """The views of frame f of a chunk, on the caller's stream, in buffers of this Detector: per scale the rescaled frame
        (frcnn_image_scale; scale 1 is the frame itself: no launch, no copy), then -- hflip -- its mirror (frcnn_image_crop_flip
        over the whole view)."""
        x = to_device(frame)
        _, H, W = _frame_shape(x)
        s = stream_ptr()
        out = []
        for i, (sc, flip, dH, dW) in enumerate(views):
            if not flip:
                base = x
                if sc != 1.0:
                    base = self._buf("%stta_view_%d_%d" % (pre, f, i), (3, dH, dW))
                    _lib.call("frcnn_image_scale", ptr(x), 3, H, W, ptr(base), dH, dW, ptr(self._buf(pre + "tta_tmp", (3 * H * dW,))),
                              0, s)
                out.append(base)
            else:       # (the unmirrored view of this scale came just before)
                m = self._buf("%stta_view_%d_%d" % (pre, f, i), (3, dH, dW))
                _lib.call("frcnn_image_crop_flip", ptr(base), 3, dH, dW, 0, 0, dW, dH, 1, 0, ptr(m), s)
                out.append(m)
        return out

    def __del__(self):
        if getattr(self, "_host", None):
            try:
                _lib.load().frcnn_host_free(C.c_void_p(self._host))
            except Exception:
                pass

    def _buf(self, name, shape, dtype=np.float32):
        need = int(math.prod(shape)) * np.dtype(dtype).itemsize   # (plain ints: a frame asks for some thirty buffers)
        b = self._bufs.get(name)
        if b is None or b.nbytes < need:
            b = DeviceTensor.empty((max(need, 256),), np.uint8)
            self._bufs[name] = b
        return DeviceTensor(b.ptr, shape, dtype, owner=b)

    def _read(self, dev_ptr, nbytes, dtype):
        """One asynchronous copy into page-locked host memory + one wait: the frame's read-back."""
        if self._host_bytes < nbytes:
            if self._host:
                _lib.call("frcnn_host_free", C.c_void_p(self._host))
            p = C.c_void_p()
            self._host_bytes = max(int(nbytes), 1 << 16)
            _lib.call("frcnn_host_alloc", C.byref(p), self._host_bytes)
            self._host = p.value
        s = stream_ptr()
        _lib.call("frcnn_memcpy_d2h", C.c_void_p(self._host), C.c_void_p(dev_ptr), int(nbytes), s)
        _lib.call("frcnn_stream_sync", s)
        raw = (C.c_char * int(nbytes)).from_address(self._host)
        return np.frombuffer(raw, dtype=dtype).copy()

    NMS_FIRST_CAP = 16384   # rows the first NMS launch is sized for (see _first_stage)
    SOFT_NMS_ROWS = 16384   # rows of a frame a soft per-class NMS takes (frcnn_soft_nms_batch)
    CLASS_NMS_WORKSPACE = 2 << 30   # bytes: under cfg["scoring"] a per-class NMS whose workspace would exceed them is refused

    @property
    def last_pick(self):
        """1-based rows of the match arrays that survived the first NMS, in pick order (Detector.lua:82)."""
        return self._last.get("pick")

    @property
    def last_cnet(self):
        """cnet outputs of the last frame's candidates: dict(bbox R x 4, cls R x (classes + 1) log-probabilities)."""
        return self._last.get("cnet")

    def _select(self, mp, mi, mr, mb, B, cap, K, c_n, pre=""):
        """pre_nms_top_n: the min(n_b, K) best-scoring rows of every frame's matches (B x cap rows, device counts c_n), gathered
        in scan order into compact arrays of kcap = min(cap, K) rows per frame -> dict(p, idx, rect, box, box5, row, cnt (device
        int32[B]: the selected counts), stride)."""
        kcap = min(cap, K)
        sel = self._buf(pre + "sel", (B, kcap), np.int32)
        cnt = self._buf(pre + "sel_count", (B,), np.int32)
        wsb = _lib.load().frcnn_topk_select_workspace_bytes(B, cap)
        ws = self._buf(pre + "sel_ws", (wsb,), np.uint8)
        s = stream_ptr()
        _lib.call("frcnn_topk_select", ptr(mp), B, cap, cap, c_n, K, ptr(sel), kcap, ptr(cnt), ptr(ws), wsb, s)
        out = dict(p=self._buf(pre + "sel_p", (B, kcap)), idx=self._buf(pre + "sel_idx", (B, kcap, 4), np.int32),
                   rect=self._buf(pre + "sel_rect", (B, kcap, 4), np.float64), box=self._buf(pre + "sel_box", (B, kcap, 4)),
                   box5=self._buf(pre + "sel_box5", (B, kcap, 5)), row=self._buf(pre + "sel_row", (B, kcap), np.int32))
        _lib.call("frcnn_rpn_gather_rows", ptr(mp), ptr(mi), ptr(mr), ptr(mb), B, cap, cap, ptr(sel), kcap, ptr(cnt), kcap,
                  ptr(out["p"]), ptr(out["idx"]), ptr(out["rect"]), ptr(out["box"]), ptr(out["box5"]), ptr(out["row"]), kcap, s)
        out.update(cnt=cnt, stride=kcap)
        return out

    def _box5(self, mp, mb, B, cap, c_n, pre=""):
        """order = "score" without a cap: rows {box, p} of every match (the count read on the device), the first NMS's input."""
        box5 = self._buf(pre + "box5", (B, cap, 5))
        _lib.call("frcnn_rpn_gather_rows", ptr(mp), None, None, ptr(mb), B, cap, cap, None, 0, c_n, cap, None, None, None, None,
                  ptr(box5), None, cap, stream_ptr())
        return box5

    def _clamp_candidates(self, c_R, Rs):
        """post_nms_top_n: the candidate counts clamped on the host -> (the clamped list, True when any changed); the device
        copy c_R (what the winner table's header reports) follows."""
        out = [min(R, self.post_nms_top_n) for R in Rs]
        if out == Rs:
            return out, False
        host = np.array(out, np.int32)
        _lib.call("frcnn_memcpy_h2d", ptr(c_R), host.ctypes.data_as(C.c_void_p), host.nbytes, stream_ptr())
        self._clamped = host     # (pageable memory: the copy has been staged when the call returns; kept anyway)
        return out, True

    def proposals(self, input):
        """The candidates of the first NMS (Detector.lua:17-85) without the classification net: a list of {p, a, r, l} as in a
        detection, in pick order (under the proposal settings of this Detector)."""
        st = self._first_stage([input], "")
        rec = self._records(st)[0]
        self.last_scan, self._last = rec.scan(), rec
        if st["ns"][0] == 0 or st["Rs"][0] == 0:
            return []
        p, idx, rect = rec["p"], rec["idx"], rec["rect"]
        out = []
        for i in (rec["pick"] - 1).tolist():
            ix = [int(t) for t in idx[i]]
            out.append(dict(p=float(p[i]), r=Rect(*rect[i].tolist()), l=ix[0], a=self.anchors.get(*ix)))
        return out

    def detect(self, input):  # Detector.lua:17-141
        """The pipeline of detect_batch on a chunk of this one frame (whatever to_device takes; buffers without the b_ prefix, so
        what a detect_batch call left behind stays as it is).  last_scan, last_pick, last_cnet and _last read the frame's record."""
        self._view_lists([_frame_shape(input)])     # (cfg.tta: refused before anything is queued)
        (winners,), (rec,) = self._detect_chunk([input], False, "")
        self.last_scan, self._last = rec.scan(), rec
        return winners

    def _roi_settings(self):
        """cfg["roi_pooling"] as it stands -> (kh, kw, g, inv_sx, inv_sy) with g = 0 for the max pool; validated before any
        device call (roi_pooling_settings; "align" needs a centred backbone)."""
        kh, kw, method, g = roi_pooling_settings(self.model["cfg"])
        if method != "align":
            return kh, kw, 0, 0.0, 0.0
        return (kh, kw, g) + align_geometry(self.localizer)

    def _pool(self, roi, fm, fmC, fmH, fmW, rect, pick, R, cinput, s, rows=None):
        """The region features of R candidates (rows pick of rect) into cinput, roi = _roi_settings(): the ROI windows
        (objective.lua:5-13 for every candidate; the window buffer sized for `rows`) and their max pooling, or -- RoIAlign -- one
        launch that reads the rects and the picks as they are."""
        kh, kw, g, inv_sx, inv_sy = roi
        if g:
            _lib.call("frcnn_roi_align_forward", fm, fmC, fmH, fmW, rect, pick, R, inv_sx, inv_sy, kh, kw, g, ptr(cinput), s)
            return
        dwins = self._buf("wins", (rows or R, 4), np.int32)
        _lib.call("frcnn_roi_windows", rect, pick, R, self._loc_layers.ctypes.data_as(C.c_void_p), len(self._loc_layers), fmH, fmW,
                  ptr(dwins), s)
        _lib.call("frcnn_roi_pool_forward", fm, fmC, fmH, fmW, ptr(dwins), R, kh, kw, ptr(cinput), None, s)

    BATCH = 8   # frames per chunk of detect_batch: bounds the memory of a call

    def detect_batch(self, inputs, shared_cnet=False, mixed_sizes=False):
        """detect() for a sequence of frames -- of one size, or (mixed_sizes=True) of any sizes: a list with one entry per frame,
        in order, each exactly what detect(frame) returns.  The frames are processed in chunks of BATCH: the proposal net runs
        frame by frame, everything between and after those passes once per chunk -- one scan, one segmented NMS, (per frame:
        pooling, classification net, class test), one segmented per-class NMS, one gather -- and the host waits twice per chunk
        instead of twice per frame.
        Results are bit-identical to detect(), which is this pipeline on a chunk of one frame: every stage of a frame sees the
        inputs it sees there, through the same kernels, and a segment of a kernel computes what a one-segment launch computes.
        last_batch holds one record per frame (_BatchRecord).
        shared_cnet=True: ONE classification-net pass over the candidates of all frames of a chunk (frame b's rows at the
        prefix sum of the candidate counts) instead of one per frame -- the large Linear streams its weights once per chunk.
        Everything up to the pooled rows stays bit-identical to detect(); the net's outputs do NOT (the two-plane form scales
        its input by the largest magnitude of the whole tensor, the Linear picks tile shape and arithmetic form by row
        count): they agree with detect()'s within the net's own error (1e-3 bar), and winners follow from them.
        mixed_sizes=False (default): frames of different sizes are refused (ValueError) before anything is queued.  True: the
        chunks are the consecutive BATCH frames whatever their sizes.  Every chunk takes the one front of _first_stage: each
        frame lies in its slot by its own size's layout, the slots are strided by the chunk's largest frame, and ONE scan
        follows -- frcnn_rpn_scan_batch when the chunk has one size (then the strides are that size's own), else
        frcnn_rpn_scan_ragged with per-frame map shapes and image sizes.  Everything behind the scan reads per-frame device
        counts already, so nothing else changes, the two waits per chunk included, and every frame's result and record stay
        bit-identical to detect(frame).
        Under cfg["tta"] a chunk holds max(1, BATCH // V) frames -- its segments are their V views each --, last_batch holds one
        _FrameRecord per frame, and more views than BATCH or a view too small for the proposal net are refused (ValueError)
        before anything is queued; mixed_sizes keeps its meaning for the frames of a call, a frame's own views never need it."""
        frames = list(inputs)
        shapes = [_frame_shape(f) for f in frames]
        if not mixed_sizes and any(shp != shapes[0] for shp in shapes):
            raise ValueError("detect_batch: frames of different sizes in one call: %s" % sorted(set(shapes)))
        results, records = [], []
        step = max(int(self.BATCH), 1)
        views = self._view_lists(shapes)     # (cfg.tta: refused before anything is queued)
        if views is not None:                # a chunk's segments are its frames' views
            step = max(1, step // len(views[0])) if views else step
        for lo in range(0, len(frames), step):
            for r in records:     # (the records of the previous chunk view buffers this chunk writes)
                r.detach()
            res, rec = self._detect_chunk(frames[lo:lo + step], bool(shared_cnet), "b_")
            results += res
            records += rec
        self.last_batch = records
        return results

    def match_batch(self, frames, ground_truth, iou_thresholds=(0.5,), mixed_sizes=False, shared_cnet=False, with_iou=False):
        """detect_batch(frames) matched to the frames' ground truth ON THE DEVICE, for mean average precision: per frame a dict
        of arrays cls, confidence (float32), tp (uint32), gt (and iou, float64, with_iou=True) whose row k describes
        detect_batch(frames)[f][k] -- bit t of tp[k] says that the detection is a true positive at iou_thresholds[t] by
        evaluation.mean_average_precision's rule (it reaches the box of its class it overlaps most, Rect.IoU >= the threshold, and
        no detection of higher confidence -- fp32 values, ties to the earlier one -- reaches that box at that threshold), gt[k] is
        that box (1-based in ground_truth[f], 0: the frame has no box of the class), iou[k] the overlap (-1 without a box).
        ground_truth[f]: the frame's boxes, (class_index, Rect) pairs or objects with .class_index and .rect (what nextValidation
        hands out), at most 1024; up to 16 thresholds.  evaluation.average_precision_from_matches turns the results into AP / mAP.
        The pipeline is detect_batch's, unchanged, up to and including the gather; behind it cfg.scoring's max_detections is
        applied by frcnn_eval_conf_rows + frcnn_topk_select (keep_best's rule) and ONE frcnn_eval_match_batch matches the chunk.
        Read-back 2 brings the match tables -- 16 bytes a row -- INSTEAD of the 128-byte winner records: the host still waits
        twice per chunk.  Every Detector setting applies as in detect_batch (under cfg.tta: one result per original frame);
        last_batch is filled as detect_batch fills it.  Bad arguments are refused (ValueError) before anything is queued."""
        frames = list(frames)
        gts = [_gt_arrays(g) for g in ground_truth]
        if len(gts) != len(frames):
            raise ValueError("match_batch: %d frames, ground truth for %d" % (len(frames), len(gts)))
        thr = [float(t) for t in iou_thresholds]
        if not 1 <= len(thr) <= MATCH_MAX_THRESHOLDS or any(t != t for t in thr):
            raise ValueError("match_batch: 1 ... %d IoU thresholds, none of them NaN (got %r)" % (MATCH_MAX_THRESHOLDS, thr))
        if any(len(c) > MATCH_MAX_BOXES for c, _ in gts):
            raise ValueError("match_batch: a frame with %d ground-truth boxes (at most %d)"
                             % (max(len(c) for c, _ in gts), MATCH_MAX_BOXES))
        shapes = [_frame_shape(f) for f in frames]
        if not mixed_sizes and any(shp != shapes[0] for shp in shapes):
            raise ValueError("match_batch: frames of different sizes in one call: %s" % sorted(set(shapes)))
        results, records = [], []
        step = max(int(self.BATCH), 1)
        views = self._view_lists(shapes)     # (cfg.tta: refused before anything is queued)
        if views is not None:
            step = max(1, step // len(views[0])) if views else step
        for lo in range(0, len(frames), step):
            for r in records:
                r.detach()
            res, rec = self._detect_chunk(frames[lo:lo + step], bool(shared_cnet), "b_",
                                          dict(gt=gts[lo:lo + step], thr=thr, with_iou=bool(with_iou)))
            results += res
            records += rec
        self.last_batch = records
        return results

    def _match_tables(self, match, out, B, rows, pre):
        """The chunk's winner tables `out` (B x (rows + 1) x 16 float64, just queued) against match["gt"], queued on the caller's
        stream: the ground truth's upload, under max_detections frcnn_eval_conf_rows + frcnn_topk_select, ONE
        frcnn_eval_match_batch.  -> a function that reads the tables back in ONE copy and wait: (int32[B][rows + 2][4], float64[B][rows]
        or None)."""
        i32 = np.int32
        s = stream_ptr()
        gts = match["gt"]
        row0 = np.concatenate([[0], np.cumsum([len(c) for c, _ in gts])]).astype(np.int64)
        G = int(row0[-1])
        gt_rect = self._buf(pre + "gt_rect", (max(G, 1), 4), np.float64)
        gt_class = self._buf(pre + "gt_class", (max(G, 1),), i32)
        host = None
        if G:
            host = (np.ascontiguousarray(np.concatenate([r for _, r in gts])), np.ascontiguousarray(np.concatenate([c for c, _ in gts])))
            _lib.call("frcnn_memcpy_h2d", ptr(gt_rect), host[0].ctypes.data_as(C.c_void_p), host[0].nbytes, s)
            _lib.call("frcnn_memcpy_h2d", ptr(gt_class), host[1].ctypes.data_as(C.c_void_p), host[1].nbytes, s)
        sel, kcap, kd = None, 0, None
        M = self.scoring[2] if self.scoring else None
        if M is not None and rows:
            kcap = min(rows, int(M))
            conf = self._buf(pre + "eval_conf", (B, rows)); cnt = self._buf(pre + "eval_count", (B,), i32)
            sel = self._buf(pre + "eval_sel", (B, kcap), i32); kd = self._buf(pre + "eval_k", (B,), i32)
            wsb = _lib.load().frcnn_topk_select_workspace_bytes(B, rows)
            ws = self._buf(pre + "eval_sel_ws", (wsb,), np.uint8)
            _lib.call("frcnn_eval_conf_rows", ptr(out), B, rows, ptr(conf), ptr(cnt), s)
            _lib.call("frcnn_topk_select", ptr(conf), B, rows, rows, ptr(cnt), int(M), ptr(sel), kcap, ptr(kd), ptr(ws), wsb, s)
        tbytes = B * (rows + 2) * 16
        nbytes = tbytes + (B * rows * 8 if match["with_iou"] else 0)
        buf = self._buf(pre + "eval_match", (nbytes,), np.uint8)
        thr = match["thr"]
        _lib.call("frcnn_eval_match_batch", ptr(out), B, rows, ptr(sel), kcap, ptr(kd), ptr(gt_rect), ptr(gt_class),
                  (C.c_longlong * (B + 1))(*[int(v) for v in row0]), (C.c_double * len(thr))(*thr), len(thr), ptr(buf),
                  C.c_void_p(buf.ptr + tbytes) if match["with_iou"] else None, s)

        def read(_alive=host):      # (the uploaded host arrays live as long as this function: until the read-back)
            raw = self._read(buf.ptr, nbytes, np.uint8)
            mt = raw[:tbytes].view(i32).reshape(B, rows + 2, 4)
            return mt, (raw[tbytes:].view(np.float64).reshape(B, rows) if match["with_iou"] else None)
        return read

    def _layout_of(self, H, W):
        """_layout of an H x W frame under this Detector's model, worked out once per size."""
        t = self._layouts.get((H, W))
        if t is None:
            t = self._layouts[H, W] = _layout([n.layers for n in self.model["pnet"].outnode.children],
                                              self.model["layers"][-1]["filters"], H, W)
        return t

    def _first_stage(self, frames, pre):
        """Detector.lua:17-85 for a chunk of B frames, of one size or not: the proposal net frame by frame, ONE scan, (selection or
        score rows), ONE segmented first NMS, read-back 1 of 2, alone again every frame over the bound, the post-NMS clamp ->
        dict(B, counts (device int32[4][B]), cap (rows a frame in p, idx, rect, pick: the match arrays the rest of the chunk
        reads, the selected rows under pre_nms_top_n), fm, fshapes (frame b's last feature map is fm.segment(b), its shape
        fshapes[b]), ns, Rs (rows and candidates per frame), key (key_mode, key_col of both NMS passes), and box, row, matches
        for _records).
        pre: prefix of the buffer names ("" for detect() and proposals(), "b_" for detect_batch: neither overwrites what the other
        left behind)."""
        pnet = self.model["pnet"]
        s = stream_ptr()
        L = _lib.load()
        B = len(frames)
        i32 = np.int32

        # ---- 1. per frame: the proposal net; its head maps and last feature map go to the frame's slot (the model owns and
        #         reuses its output buffers).  Where they lie follows from the frame's size on the host (_layout, checked against
        #         what the net hands back), so the slots -- strided by the chunk's largest frame -- are sized before the first
        #         pass: frame b's four head maps lie packed at hoff[i] of slot b of `heads`, its last feature map at the start of
        #         slot b of `fm`.  A chunk of ONE frame reads the model's buffers where they are: no copies.
        pnet.evaluate()  # :31
        # counts (device int32[4][B]): per frame matches, NMS candidates, candidates that pass the class test, winners
        counts = self._buf(pre + "counts", (4, B), i32)
        c_n, c_R = ptr(counts.segment(0)), counts.segment(1)
        threshold = 0.95
        sizes = [_frame_shape(f)[1:] for f in frames]
        lay = [self._layout_of(H, W) for H, W in sizes]
        slot, fslot, cap = _chunk_slots(lay)
        if B > 1:
            heads, fm = self._buf(pre + "heads", (B, slot)), self._buf(pre + "fm", (B, fslot))
        for b, (f, t) in enumerate(zip(frames, lay)):
            outputs = pnet.forward(to_device(f))  # :33
            got, want = [tuple(o.shape) for o in outputs], [(ASPECTS * 6,) + m for m in t.hw] + [t.fshape]
            if got != want:
                raise _lib.FrcnnError("Detector: a %dx%d frame gives maps %r, expected %r" % (sizes[b] + (got, want)))
            if B == 1:
                maps, fm = [ptr(o) for o in outputs[:4]], outputs[-1].view(1, *t.fshape)
                break
            for i in range(4):
                _lib.call("frcnn_memcpy_d2d", ptr(heads.segment(b).offset_view(t.hoff[i], outputs[i].shape)), ptr(outputs[i]),
                          outputs[i].nbytes, s)
            _lib.call("frcnn_memcpy_d2d", ptr(fm.segment(b)), ptr(outputs[-1]), outputs[-1].nbytes, s)
        # ---- 2. ONE scan over the B slots (Detector.lua:39-66): frame b's matches at rows [b * cap, b * cap + n_b).  Every
        #         anchor of the four maps may pass (vgg_large 1000x600 scans 45 015): the buffers hold them all, nothing is
        #         ever truncated; cap is the largest frame's anchor count.  A chunk of one size takes frcnn_rpn_scan_batch (the
        #         four maps of slot 0 -- or the model's own --, the slot stride, that size), a chunk that mixes sizes
        #         frcnn_rpn_scan_ragged (per-frame map sizes, offsets and image sizes): the same bodies, 3 % dearer a call
        Hs = (C.c_int * (4 * B))(*[h for t in lay for h, _ in t.hw])
        Ws = (C.c_int * (4 * B))(*[w for t in lay for _, w in t.hw])
        if len(set(sizes)) == 1:
            H, W = sizes[0]
            if B > 1:
                maps = [ptr(heads.offset_view(lay[0].hoff[i], (1,))) for i in range(4)]
            wsb = L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, B)
            scan = ("frcnn_rpn_scan_batch", (C.c_void_p * 4)(*[m.value for m in maps]), Hs, Ws, B, slot, ptr(self._aw),
                    ptr(self._ah), float(W), float(H))
        else:
            map_off = (C.c_longlong * (4 * B))(*[b * slot + t.hoff[i] for b, t in enumerate(lay) for i in range(4)])
            img_wh = (C.c_double * (2 * B))(*[float(v) for H, W in sizes for v in (W, H)])
            wsb = L.frcnn_rpn_scan_ragged_workspace_bytes(Hs, Ws, B)
            scan = ("frcnn_rpn_scan_ragged", ptr(heads), map_off, Hs, Ws, img_wh, B, ptr(self._aw), ptr(self._ah))
        ws = self._buf(pre + "scan_ws", (wsb,), np.uint8)
        mp = self._buf(pre + "match_p", (B, cap)); mi = self._buf(pre + "match_idx", (B, cap, 4), i32)
        mr = self._buf(pre + "match_rect", (B, cap, 4), np.float64); mb = self._buf(pre + "match_box", (B, cap, 4))
        _lib.call(*scan, threshold, cap, ptr(mp), ptr(mi), ptr(mr), ptr(mb), c_n, ptr(ws), wsb, s)
        fshapes, anchors = [t.fshape for t in lay], [t.anchors for t in lay]
        # ---- 3. ONE segmented NMS (:74-85) on the device, the match counts read from device memory; the score tensor is ignored
        #         by nms.lua -> key = max-y.  The launch and its workspace are sized for a BOUND on the matches, not for every
        #         anchor of the maps (vgg_large: 45 015 anchors -> 253 MB of masks and a 704 x 704 tile grid per frame for a few
        #         hundred matches); a frame with more matches than the bound repeats the pass alone, sized by the count just read.
        #         Under pre_nms_top_n = K the match arrays are replaced by the compact arrays of the K best-scoring rows (`cap`
        #         rows a frame from here on: min(cap, K)), which no frame can exceed; order = "score": rows {box, p} keyed by p.
        order, pre_n, post_n = self.proposal_order, self.pre_nms_top_n, self.post_nms_top_n
        key_mode, key_col = (2, 5) if order == "score" else (0, 0)
        ncap = min(cap, self.NMS_FIRST_CAP)
        c_first, boxes, ncols, row, matches = c_n, mb, 4, None, None
        if order == "score" and pre_n is None:
            boxes, ncols = self._box5(mp, mb, B, cap, c_n, pre), 5
        if pre_n is not None:
            sel = self._select(mp, mi, mr, mb, B, cap, pre_n, c_n, pre)
            mp, mi, mr, mb, row = sel["p"], sel["idx"], sel["rect"], sel["box"], sel["row"]
            cap = ncap = sel["stride"]
            c_first, boxes = ptr(sel["cnt"]), mb
            if order == "score":
                boxes, ncols = sel["box5"], 5
        wsb = L.frcnn_nms_batch_workspace_bytes(B, ncap)
        ws = self._buf(pre + "nms_ws", (wsb,), np.uint8)
        pick = self._buf(pre + "nms_pick", (B, cap), np.int64)
        _lib.call("frcnn_nms_device_batch", ptr(boxes), B, cap, ncap, c_first, ncols, C.c_float(0.25), key_mode, key_col, None,
                  ptr(pick), ptr(c_R), ptr(ws), wsb, s)
        nR = self._read(counts.ptr, counts.nbytes // 2, i32)                   # ---- read-back 1 of 2: B pairs of counts
        ns, Rs = [int(v) for v in nR[:B]], [int(v) for v in nR[B:]]
        for b in range(B):
            if ns[b] > anchors[b]:
                raise _lib.FrcnnError("Detector: %d anchors pass p > %g, more than the %d the maps hold"
                                      % (ns[b], threshold, anchors[b]))
        if pre_n is not None:
            matches, ns = ns, [min(n, pre_n) for n in ns]
        for b in range(B):
            if ns[b] > ncap:
                wsb = L.frcnn_nms_workspace_bytes(ns[b])
                ws = self._buf(pre + "nms_ws_full", (wsb,), np.uint8)
                c_Rb = c_R.offset_view(b, (1,))
                _lib.call("frcnn_nms_device", ptr(boxes.segment(b)), ns[b], ncols, C.c_float(0.25), key_mode, key_col,
                          ptr(pick.segment(b)), ptr(c_Rb), ptr(ws), wsb, s)
                Rs[b] = int(self._read(c_Rb.ptr, c_Rb.dtype.itemsize, i32)[0])
        if post_n is not None:
            Rs = self._clamp_candidates(c_R, Rs)[0]
        return dict(B=B, counts=counts, cap=cap, p=mp, idx=mi, rect=mr, box=mb, row=row, pick=pick, fm=fm, fshapes=fshapes,
                    ns=ns, Rs=Rs, matches=matches, key=(key_mode, key_col))

    def _records(self, st, more=None):
        """One _BatchRecord per frame of the chunk _first_stage returned st for (views of the chunk's buffers, kept = 0);
        more[b]: further device arrays of frame b (bbox, cls, pooled).  Host work only: _detect_chunk calls it with the whole
        chunk queued, in front of its second wait, not between read-back 1 and the launches that wait for it."""
        row, matches = st["row"], st["matches"]
        records = []
        for b in range(st["B"]):
            n = st["ns"][b]
            R = st["Rs"][b] if n else 0  # :71
            dev = dict({k: st[k].segment(b, n) for k in ("p", "idx", "rect", "box")}, pick=st["pick"].segment(b, R),
                       **(more or {}).get(b, {}))
            if row is not None:   # the rows above are the selected ones: their 1-based original scan rows
                dev.update(row=row.segment(b, n))
            records.append(_BatchRecord(n, R, dev, matches[b] if matches is not None else None))
        return records

    def _detect_chunk(self, frames, shared, pre, match=None):
        """detect() of a chunk of frames -> (one result per frame, their records): _first_stage, then -- unless no frame has a match
        -- per frame the pooling, the classification net and the class test, ONE segmented per-class NMS, ONE gather and
        read-back 2 of 2.
        match (match_batch; None: nothing below is launched, allocated or read differently): dict(gt: per frame (classes, rects),
        thr, with_iou).  Behind the gather the winners are matched to the ground truth on the device (_match_tables) and read-back
        2 brings the match tables in place of the winner tables; a frame's result is then a _match_result.
        Under cfg["tta"] the SEGMENTS of the chunk are the frames' views (frame f's V views at segments f * V ... f * V + V - 1,
        made by _make_views): _first_stage and step 4 run on them as on frames, ONE frcnn_detect_merge_views launch then makes one
        segment per frame of them, and step 5 runs on those -- B frames, V times the rows."""
        model = self.model
        cfg = model["cfg"]
        cnet = model["cnet"]
        roi = self._roi_settings()
        kh, kw = roi[0], roi[1]
        ncls = cfg["class_count"] + 1     # the classes and, last, the background
        planes = model["layers"][-1]["filters"]
        s = stream_ptr()
        L = _lib.load()
        i32 = np.int32

        shapes = [_frame_shape(f) for f in frames]
        view_lists = self._view_lists(shapes)
        V = len(view_lists[0]) if view_lists else 1
        if view_lists:
            frames = [v for f, (x, vl) in enumerate(zip(frames, view_lists)) for v in self._make_views(x, vl, f, pre)]
        st = self._first_stage(frames, pre)   # :17-85
        B, counts, cap, mp, mi, mr, pick = st["B"], st["counts"], st["cap"], st["p"], st["idx"], st["rect"], st["pick"]
        ns, Rs, (key_mode, key_col) = st["ns"], st["Rs"], st["key"]
        c_K, c_W = counts.segment(2), ptr(counts.segment(3))
        Rmax = max([Rs[b] for b in range(B) if ns[b] > 0] + [0])
        if Rmax == 0:   # no frame has a match (:71)
            none = (lambda: []) if match is None else (lambda: _match_result(None, None, match["with_iou"]))
            if view_lists:
                return [none() for _ in range(B // V)], self._frame_records(self._records(st), V, {})
            return [none() for _ in range(B)], self._records(st)
        # ---- 4. per frame with candidates: REGION CLASSIFICATION (:90-101) into the frame's rows.  These launches come first:
        #         the device has been idle since read-back 1, and whatever else the host prepares it prepares while they run
        cnet.evaluate()
        fshapes = st["fshapes"]
        D = kh * kw * planes
        # first row of frame b in the net's input / output arrays: its own segment (Rmax rows per frame), or (shared pass) the
        # prefix sum of R
        row0, total, more = {}, 0, {}
        for b in range(B):
            if ns[b] > 0:
                row0[b] = total if shared else b * Rmax
                total += Rs[b]
        cinput_buf = self._buf(pre + "cinput", (total if shared else Rmax, D))
        bbox_all = self._buf(pre + "bbox", (B, Rmax, 4)); cls_all = self._buf(pre + "cls_out", (B, Rmax, ncls))
        # cfg["scoring"]["boxes"] = "class" under "all": the box head's input of every pass is kept, in the rows of bbox_all and
        # cls_all, for the class-row launch behind the class test ("top": the net's own box IS the row's class's)
        class_boxes = bool(self.scoring) and self.scoring[0] == "all" and self.boxes == "class"
        if class_boxes:
            nf = cnet.feature_count
            feat_all = self._buf(pre + "feat", (B, Rmax, nf))

        def pooled(b):    # the region features of frame b's candidates (_pool) -> its input rows
            R = Rs[b]
            fmC, fmH, fmW = fshapes[b]
            cinput = cinput_buf.offset_view(D * row0[b] if shared else 0, (R, D))
            self._pool(roi, ptr(st["fm"].segment(b)), fmC, fmH, fmW, ptr(mr.segment(b)), ptr(pick.segment(b)), R, cinput, s,
                       rows=Rmax)
            return cinput
        for b in sorted(row0):
            if self.verbose:
                print("candidates: %d" % Rs[b])
            # (the net writes into the frame's rows: its own output buffers are reused by the next pass)
            more[b] = dict(bbox=bbox_all.offset_view(4 * row0[b], (Rs[b], 4)),
                           cls=cls_all.offset_view(ncls * row0[b], (Rs[b], ncls)))
            if shared:
                more[b].update(pooled=pooled(b))
            else:
                cnet.forward(pooled(b), out=(more[b]["bbox"], more[b]["cls"]))  # :101
                if class_boxes:
                    cnet.features(feat_all.offset_view(nf * row0[b], (Rs[b], nf)))
        if shared:
            cnet.forward(cinput_buf, out=(bbox_all.offset_view(0, (total, 4)),
                                          cls_all.offset_view(0, (total, ncls))))  # :101, all frames
            if class_boxes:
                cnet.features(feat_all.offset_view(0, (total, nf)))
        # ---- then, per frame, the class test (:106-122) into the frame's segment: r2 = Anchors.anchorToInput(r, bbox) in double,
        #      survivors compacted in order
        #      Under cfg["scoring"]: ONE frcnn_detect_classes_batch launch for the chunk, which reads the net's log-probabilities
        #      itself (every frame's row count and first row are kernel arguments) -- "top": the same rows; "all": a row per
        #      foreground class over min_confidence, so the per-row buffers and everything behind hold `rows` = Rmax * m a frame
        scoring = self.scoring
        rows = Rmax * (scoring_rows(scoring[0], scoring[1], ncls) if scoring else 1)
        bb = self._buf(pre + "bb", (B, rows, 5)); kc = self._buf(pre + "kc", (B, rows), i32)
        keep_row = self._buf(pre + "keep_row", (B, rows), i32); r2 = self._buf(pre + "r2", (B, rows, 4), np.float64)
        if scoring:
            R_arg = (C.c_int * B)(*[Rs[b] if b in row0 else 0 for b in range(B)])     # (a frame without matches: no rows)
            row0_arg = (C.c_longlong * B)(*[row0.get(b, 0) for b in range(B)])
            _lib.call("frcnn_detect_classes_batch", ptr(cls_all), ptr(bbox_all), R_arg, row0_arg, B, ptr(mr), ptr(pick), cap, ncls,
                      ncls, scoring[1], SCORING_MODES[scoring[0]], ptr(bb), ptr(kc), ptr(keep_row), ptr(r2), rows, ptr(c_K), None, s)
            if class_boxes:
                # ONE launch: row (r, c) gets the box class c's regressor rows predict for candidate r (the one written above
                # was a placeholder), read from the kept features; the row counts stay on the device.  In front of the merge of
                # cfg["tta"], which then transforms the per-class boxes like any others
                W_box, b_box = model["native"].box_head_parameters()
                _lib.call("frcnn_detect_class_boxes_batch", ptr(feat_all), nf, row0_arg, B, ptr(W_box), ptr(b_box), ncls - 1, ptr(mr),
                          ptr(pick), cap, ptr(kc), ptr(keep_row), ptr(c_K), rows, ptr(bb), ptr(r2), s)
        else:
            dcls = self._buf(pre + "cls", (Rmax,), i32); dconf = self._buf(pre + "conf", (Rmax,))
            for b in range(B):
                c_Kb = c_K.offset_view(b, (1,))
                if ns[b] == 0:     # no candidates: an empty segment of the per-class NMS
                    _lib.call("frcnn_zero", ptr(c_Kb), c_Kb.dtype.itemsize, s)
                    continue
                _lib.call("frcnn_cnet_decode", ptr(more[b]["cls"]), Rs[b], ncls, ptr(dcls), ptr(dconf), s)  # :110-113
                _lib.call("frcnn_detect_post", ptr(dcls), ptr(dconf), ptr(more[b]["bbox"]), ptr(mr.segment(b)),
                          ptr(pick.segment(b)), Rs[b], ncls, 0.2, ptr(bb.segment(b)), ptr(kc.segment(b)),
                          ptr(keep_row.segment(b)), ptr(r2.segment(b)), ptr(c_Kb), s)
        #      Under cfg["tta"]: ONE frcnn_detect_merge_views launch -- every frame's V segments of survivors become one segment of
        #      V * rows rows in the frame's coordinates (the geometry of a view and its candidate count are host values since
        #      read-back 1: kernel arguments), the views' picks one pick list over the frame's V * cap match rows.  From here on the
        #      chunk has B / V segments; the match arrays are read where they lie
        if view_lists:
            S, B = B, B // V
            geo = [(fl, float(dW), float(shp[2]) / dW, float(shp[1]) / dH)
                   for shp, vl in zip(shapes, view_lists) for _, fl, dH, dW in vl]
            R_seg = [Rs[b] if b in row0 else 0 for b in range(S)]
            roffs = [np.concatenate([[0], np.cumsum(R_seg[f * V:f * V + V])]) for f in range(B)]
            vbb, vkc, vkeep, vr2 = bb, kc, keep_row, r2
            bb = self._buf(pre + "tta_bb", (B, V * rows, 5)); kc = self._buf(pre + "tta_kc", (B, V * rows), i32)
            keep_row = self._buf(pre + "tta_keep_row", (B, V * rows), i32)
            r2 = self._buf(pre + "tta_r2", (B, V * rows, 4), np.float64)
            vpick, pick = pick, self._buf(pre + "tta_pick", (B, V * cap), np.int64)
            vcounts, counts = counts, self._buf(pre + "tta_counts", (4, B), i32)
            _lib.call("frcnn_detect_merge_views", ptr(vbb), ptr(vkc), ptr(vkeep), ptr(vr2), rows, ptr(vcounts), ptr(vpick), cap, B, V,
                      (C.c_int * S)(*[int(g[0]) for g in geo]), (C.c_double * S)(*[g[1] for g in geo]),
                      (C.c_double * S)(*[g[2] for g in geo]), (C.c_double * S)(*[g[3] for g in geo]), (C.c_int * S)(*R_seg),
                      ptr(bb), ptr(kc), ptr(keep_row), ptr(r2), ptr(pick), ptr(counts), s)
            c_K, c_W = counts.segment(2), ptr(counts.segment(3))
            rows, cap = V * rows, V * cap
        # ---- 5. ONE segmented per-class NMS (:125-136; one segment per frame, rows only suppress rows of their own class: a stable
        #         partition of the picks by class is, per class, exactly nms(bb_class, 0.1, scores) -- key = max-y, or the confidence
        #         column under order = "score"), the survivor counts read from device memory; ONE gather of every frame's winner
        #         records behind a 128-byte header of the frame's four counts
        #         Under a soft method (cfg["nms"]): ONE frcnn_soft_nms_batch launch instead, on the log-confidences (log_domain 1,
        #         min_score as a log), which writes every winner's decayed score into column 5 of a COPY of bb; the gather reads
        #         that copy, so a winner's confidence is the score it was picked at
        wpick = self._buf(pre + "wpick", (B, rows), np.int64)
        soft = self.nms_method != "hard"
        # (a frame's rows are its candidates times m: fewer candidates are the way out of either refusal)
        remedy = " (%d candidates x %d rows each: lower cfg.proposals.post_nms_top_n)" % (Rmax, rows // Rmax) if rows > Rmax else ""
        bb_win = bb
        if soft:
            if rows > self.SOFT_NMS_ROWS:
                raise _lib.FrcnnError("Detector: %d candidates in a frame, more than the %d a soft per-class NMS takes%s"
                                      % (rows, self.SOFT_NMS_ROWS, remedy))
            bb_win = self._buf(pre + "bb_soft", (B, rows, 5))
            _lib.call("frcnn_memcpy_d2d", ptr(bb_win), ptr(bb), bb.nbytes, s)
            wsb2 = L.frcnn_soft_nms_workspace_bytes(B, rows)
            ws2 = self._buf(pre + "soft_nms_ws", (wsb2,), np.uint8)
            log_min = float(math.log(self.nms_min_score)) if self.nms_min_score > 0.0 else -math.inf
            _lib.call("frcnn_soft_nms_batch", ptr(bb), B, rows, rows, ptr(c_K), 5, 5, SOFT_NMS_METHODS.index(self.nms_method),
                      C.c_float(self.nms_overlap), C.c_float(self.nms_sigma), C.c_float(log_min), 1, ptr(kc), ptr(wpick), c_W,
                      ptr(bb_win.offset_view(4, (1,))), 5, ptr(ws2), wsb2, s)      # (column 5 of the copy)
        else:
            wsb2 = L.frcnn_nms_batch_workspace_bytes(B, rows)
            if scoring and wsb2 > self.CLASS_NMS_WORKSPACE:
                raise _lib.FrcnnError("Detector: the per-class NMS of %d frames of %d rows needs a workspace of %d bytes, more than "
                                      "the %d allowed%s" % (B, rows, wsb2, self.CLASS_NMS_WORKSPACE, remedy))
            ws2 = self._buf(pre + "nms_ws2", (wsb2,), np.uint8)
            _lib.call("frcnn_nms_device_batch", ptr(bb), B, rows, rows, ptr(c_K), 5, C.c_float(self.nms_overlap), key_mode, key_col,
                      ptr(kc), ptr(wpick), c_W, ptr(ws2), wsb2, s)
        #         Under box voting (cfg["box_voting"]): ONE frcnn_box_vote_batch launch over the class test's survivors -- rows bb
        #         (the UNDECAYED log-confidences, also under a soft method: weight_mode 2), classes kc, coordinates the fp64 r2,
        #         winners wpick with the device winner counts -- writes the winners' voted rects into a buffer of their own, which
        #         the gather reads in place of r2.  Nothing else changes
        voting = self.box_voting is not None
        r2_win = r2
        if voting:
            r2_win = self._buf(pre + "r2_voted", (B, rows, 4), np.float64)
            votes = self._buf(pre + "votes", (B, rows), i32)
            _lib.call("frcnn_zero", ptr(votes), votes.nbytes, s)      # (a record shows 0 votes for the rows that did not win)
            _lib.call("frcnn_box_vote_batch", ptr(bb), B, rows, rows, ptr(c_K), 5, 5, BOX_VOTING_WEIGHTS[self.box_voting[1]],
                      C.c_float(self.box_voting[0]), ptr(kc), ptr(r2), ptr(wpick), c_W, ptr(r2_win), ptr(votes), s)
        out = self._buf(pre + "winners", (B, rows + 1, 16), np.float64)
        _lib.call("frcnn_detect_gather_batch", ptr(wpick), ptr(counts), B, rows, ptr(keep_row), ptr(kc), ptr(bb_win), ptr(r2_win),
                  ptr(pick), cap, ptr(mp), ptr(mr), ptr(mi), ptr(out), s)
        if match is not None:     # match_batch: the winners against the ground truth, queued behind the gather
            tables = self._match_tables(match, out, B, rows, pre)
        records = self._records(st, more)
        if view_lists:    # one record per frame over its views' records
            records = self._frame_records(records, V, dict((f, dict(pick=pick.segment(f, int(roffs[f][-1])))) for f in range(B)),
                                          roffs)
        if match is None:
            raw = self._read(out.ptr, out.nbytes, np.float64).reshape(out.shape)   # ---- read-back 2 of 2
        else:
            mt, iou = tables()                                                      # ---- read-back 2 of 2: 16 bytes a row
        results = []
        for b in range(B):
            hdr = raw[b, 0].view(i32) if match is None else mt[b, 0]
            K = int(hdr[2])
            # (soft, voting: the class test's survivors as the pass read them, views of the chunk's buffers until detach();
            # cfg.tta: always, and all of them -- the merged survivors exist nowhere else)
            extra = dict(bb=bb.segment(b, K), kc=kc.segment(b, K)) if soft or voting or view_lists else {}
            if voting or view_lists:
                extra.update(r2=r2.segment(b, K), keep_row=keep_row.segment(b, K))
            if voting:
                extra.update(votes=votes.segment(b, K))
            records[b].finish(K, **extra)
            if match is not None:
                results.append(_match_result(mt[b], None if iou is None else iou[b], match["with_iou"]))
                continue
            if records[b]["n"] == 0:
                results.append([])
                continue
            w = raw[b, 1:1 + int(hdr[3])]
            if scoring and scoring[2] is not None and len(w) > scoring[2]:   # max_detections: the best M, still in pick order
                w = w[keep_best(w[:, 2], scoring[2])]
            # classes in ascending order (pairs() order is unspecified in Lua), pick order within a class
            results.append(_Detections(w[np.argsort(w[:, 0], kind="stable")].copy(), self.anchors,
                                       roffs[b][:-1] if view_lists else None))
        return results, records

    def _frame_records(self, records, V, dev, roffs=None):
        """cfg["tta"]: one _FrameRecord per frame over the chunk's per-view records (V consecutive ones a frame); dev[f]: the
        frame's own device arrays; roffs[f]: the prefix sums of its views' candidate counts (None: no view has a candidate)."""
        out = []
        for f in range(len(records) // V):
            views = records[f * V:f * V + V]
            roff = roffs[f] if roffs is not None else np.zeros(V + 1, np.int64)
            out.append(_FrameRecord(views, roff, dev.get(f, {})))
        return out
