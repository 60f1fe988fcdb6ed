"""extract_roi_pooling_input and create_objective -- host-side mirror of objective.lua.

lossAndGradient(w) keeps the structure of objective.lua:45-218 (per image: pnet forward, sparse RPN
loss on the sampled anchors, ROI adaptive max-pooling, cnet forward/backward, ROI-pool backward,
pnet backward; then normalise and log), but every per-example Lua loop that touched the device one
scalar at a time is ONE batched kernel here (frcnn_rpn_loss, frcnn_roi_pool_forward/backward,
frcnn_cnet_losses), and the eight statistics of objective.lua:52-58 stay in a device-side fp64
vector until the single read-back at the end of the call.

Data parallelism (not in the reference): when torch.distributed is initialised, every
rank processes its own images and the flat gradient + the 8 accumulators are all-reduced (sum) just
before `gradient:div(cls_count)` (objective.lua:200), so the result equals the single-process result
on the concatenated batch (not under cfg.roi_sampling.source = "proposals" where a quota cuts: every rank's objective counts its
own images, so the ranks draw with seed + 0, seed + 1, ... each, where the single process draws with seed + k for its k-th image;
under source = "hard" nothing is drawn -- the loss decides -- so there the data-parallel result on the concatenated batch IS the
single-process one).

Not in the reference: cfg["roi_sampling"] (roi_sampling_settings) trains the classification net on a sample of the first NMS's
candidates instead of the example rows -- scan, selection, NMS and frcnn_proposal_targets_batch on the pass's own head maps.
Under source = "hard" (online hard example mining) every labelled candidate is scored first and the rows of largest loss train
(mine_hard).  The scoring pass runs the classification net in evaluate mode: it normalises with the BatchNormalization layers'
RUNNING statistics and applies no dropout, while the training pass behind it uses the batch's statistics and draws its masks --
the loss that ranks a row is the deployed net's, not the one the row's gradient is taken of.

Not in the reference either: cfg["cnet_loss"] (cnet_loss_settings) replaces the fixed losses of objective.lua:170-177 -- SmoothL1 * 10
and ClassNLL -- by frcnn_cnet_loss_rows: focal loss, label smoothing, a GIoU box loss, computed row by row and summed by
frcnn_loss_accumulate; under source = "hard" the same kernel writes the keys the candidates are ranked by."""
import ctypes as C
import math
import os
import sys

import numpy as np

from . import _lib
from .Anchors import Anchors
from .Localizer import Localizer
from .Rect import Rect
from .tensor import DeviceTensor, ptr, stream_ptr, to_device


def roi_window(input_rect, localizer, fm_h, fm_w):
    """The index table of objective.lua:11: rows {min(minY+1,maxY), maxY}, cols {min(minX+1,maxX), maxX}
    (1-based inclusive) of the feature map covered by input_rect."""
    r = localizer.inputToFeatureRect(input_rect)
    r = r.clip(Rect(0, 0, fm_w, fm_h))
    return (int(min(r.minY + 1, r.maxY)), int(r.maxY), int(min(r.minX + 1, r.maxX)), int(r.maxX))


def roi_windows(rects, localizer, fm_h, fm_w):
    """roi_window() for an (n, 4) array of input rects -> int32 (n, 4), vectorised."""
    r = localizer.inputToFeatureRectBatch(rects)
    minX = np.minimum(np.maximum(r[:, 0], 0), fm_w); minY = np.minimum(np.maximum(r[:, 1], 0), fm_h)   # Rect.clip
    maxX = np.maximum(np.minimum(r[:, 2], fm_w), 0); maxY = np.maximum(np.minimum(r[:, 3], fm_h), 0)
    return np.stack([np.minimum(minY + 1, maxY), maxY, np.minimum(minX + 1, maxX), maxX], 1).astype(np.int32)


def extract_roi_pooling_input(input_rect, localizer, feature_layer_output):  # objective.lua:5-13
    """Returns (window, idx): idx = {{}, {row_lo,row_hi}, {col_lo,col_hi}} like the reference; the strided
    view itself is never materialised -- the batched ROI-pool kernel reads the window in place."""
    s = feature_layer_output.shape
    win = roi_window(input_rect, localizer, s[1], s[2])
    idx = ((), (win[0], win[1]), (win[2], win[3]))
    return win, idx


ROI_POOLING_DEFAULTS = dict(method="max", sampling_ratio=2)


def roi_pooling_settings(cfg):
    """cfg["roi_pooling"] of a model's cfg -> (kh, kw, method, g), validated on the host.
      kh, kw          the grid of bins (the classification net's input is filters x kh x kw)
      method          "max" (default: the reference -- the rect goes through Localizer:inputToFeatureRect, is snapped to whole
                      cells and max-pooled) or "align": RoIAlign, bilinear sampling at un-snapped coordinates averaged per bin
                      (frcnn_roi_align_forward / _backward; the backbone must be Localizer.centred(): align_geometry)
      sampling_ratio  g x g samples per bin, an integer 1..4, default 2; only read under "align"
    Raises ValueError (before any device call) for an unknown key, an unknown method, a bool or non-integer or out-of-range
    sampling_ratio."""
    t = cfg.get("roi_pooling")
    if not isinstance(t, dict):
        raise ValueError("cfg.roi_pooling must be a table of {kh, kw, method, sampling_ratio}")
    unknown = sorted(set(t) - set(("kh", "kw")) - set(ROI_POOLING_DEFAULTS), key=str)
    if unknown:
        raise ValueError("cfg.roi_pooling: unknown key(s) %s" % ", ".join(map(str, unknown)))
    kh, kw = t["kh"], t["kw"]
    method = t.get("method", "max")
    if not isinstance(method, str) or method not in ("max", "align"):
        raise ValueError("cfg.roi_pooling.method = %r (\"max\" or \"align\")" % (method,))
    g = ROI_POOLING_DEFAULTS["sampling_ratio"]
    if method == "align":
        g = t.get("sampling_ratio", g)
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise ValueError("cfg.roi_pooling.sampling_ratio = %r is not an integer" % (g,))
        if not 1 <= g <= 4:
            raise ValueError("cfg.roi_pooling.sampling_ratio = %d outside 1..4" % g)
    return kh, kw, method, int(g)


def align_geometry(localizer):
    """(1 / Sx, 1 / Sy) as frcnn_roi_align_* take them; raises ValueError for a backbone that is not centred.  The kernels multiply
    by these where the statement divides by the stride: the same number for a power-of-two stride (16 for both models); for any
    other stride a coordinate may differ from minX / Sx in its last bit."""
    if not localizer.centred():
        raise ValueError("cfg.roi_pooling.method = \"align\" needs a centred backbone (every layer k - d == 2 pad): "
                         "Localizer.centred() is false")
    sx, sy = localizer.stride()
    return 1.0 / sx, 1.0 / sy


ROI_SAMPLING_DEFAULTS = dict(source="examples", batch=128, fg_fraction=0.25, fg_iou=0.5, bg_iou=(0.0, 0.5), include_gt=True,
                             threshold=0.5, nms_overlap=0.7, pre_nms_top_n=6000, post_nms_top_n=2000, seed=0,
                             hard_nms_overlap=0.7)
ROI_SAMPLING_MAX_GT = 64          # ground-truth boxes an image may carry (frcnn_proposal_targets_batch)
ROI_SAMPLING_MAX_CANDIDATES = 4096   # ground truth + picks a segment of frcnn_proposal_targets_batch holds


def roi_sampling_settings(cfg):
    """cfg["roi_sampling"] (which rows the classification net is trained on; not in the reference) -> a dict of the validated
    settings plus fg_quota = floor(batch * fg_fraction + 0.5), or None when the key is absent.
      source          "examples" (default: objective.lua:91-140 -- the ground-truth rects of the positive anchors and the rects of
                      the sampled negative anchors) or "proposals": a sample of the candidates the first NMS leaves on this very
                      forward pass, matched to the image's ground truth by frcnn_proposal_targets_batch; or "hard": online hard
                      example mining (Shrivastava et al. 2016) -- EVERY labelled candidate is scored by the net in evaluate mode,
                      an NMS keyed by the loss removes near-duplicates, and the `batch` survivors of largest loss are the rows
                      the net is trained on
      batch           rows a image contributes at most (1 ... 4096); fg_fraction: the share of them that may be foreground (0 ... 1)
      fg_iou          a candidate whose best IoU reaches it is foreground (0 ... 1)
      bg_iou          {lo, hi}: background is lo <= best IoU < hi, with lo <= hi <= fg_iou; anything else is ignored
      include_gt      the ground-truth boxes themselves are candidates too
      threshold       the anchor scan's probability threshold (0 ... 1; Detector.lua:44 uses 0.95); nms_overlap: the first NMS's,
                      in (0, 1], keyed by the score
      pre_nms_top_n   the best-scoring matches the NMS sees (1 ... Detector.NMS_FIRST_CAP); post_nms_top_n: the picks that become
                      candidates (1 ... 4096 - 64)
      seed            of the sampling hash (0 ... 2^32 - 1); image k of an objective draws with seed + k
      hard_nms_overlap  the overlap of the NMS among the scored candidates under "hard", in (0, 1] (1: no row suppresses another --
                      an IoU never exceeds 1); accepted and unused under the other sources, as every key but source is under "examples"
                      (the validated table of another source carries the key only when cfg sets it)
    Under "hard" batch, fg_iou, bg_iou, include_gt, threshold, nms_overlap, pre_nms_top_n and post_nms_top_n keep their meaning;
    fg_fraction and seed are NOT applied: no quota is drawn, the loss decides which rows train and how many are foreground.
    Raises FrcnnError -- before the model or the device is touched -- for an unknown key, a wrong type or a value out of range."""
    t = cfg.get("roi_sampling")
    if t is None:
        return None
    E = _lib.FrcnnError
    if not isinstance(t, dict):
        raise E("cfg.roi_sampling must be a table of {%s}" % ", ".join(ROI_SAMPLING_DEFAULTS))
    unknown = sorted(set(t) - set(ROI_SAMPLING_DEFAULTS), key=str)
    if unknown:
        raise E("cfg.roi_sampling: unknown key(s) %s" % ", ".join(map(str, unknown)))
    out = dict(ROI_SAMPLING_DEFAULTS)
    out.update(t)

    def number(key, lo, hi, lo_open=False):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise E("cfg.roi_sampling.%s = %r is not a number" % (key, v))
        if not (lo < v if lo_open else lo <= v) or not v <= hi:
            raise E("cfg.roi_sampling.%s = %r outside %s%g, %g]" % (key, v, "(" if lo_open else "[", lo, hi))
        return float(v)

    def integer(key, lo, hi):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise E("cfg.roi_sampling.%s = %r is not an integer" % (key, v))
        if not lo <= v <= hi:
            raise E("cfg.roi_sampling.%s = %d outside %d ... %d" % (key, v, lo, hi))
        return int(v)

    if not isinstance(out["source"], str) or out["source"] not in ("examples", "proposals", "hard"):
        raise E("cfg.roi_sampling.source = %r (\"examples\", \"proposals\" or \"hard\")" % (out["source"],))
    if not isinstance(out["include_gt"], bool):
        raise E("cfg.roi_sampling.include_gt = %r (true or false)" % (out["include_gt"],))
    from .Detector import Detector
    out["batch"] = integer("batch", 1, ROI_SAMPLING_MAX_CANDIDATES)
    out["fg_fraction"] = number("fg_fraction", 0.0, 1.0)
    out["fg_iou"] = number("fg_iou", 0.0, 1.0)
    bg = out["bg_iou"]
    if isinstance(bg, dict):        # (a Lua table {lo, hi} as the t7 reader hands it over)
        bg = [bg[k] for k in sorted(bg)] if sorted(bg) == [1, 2] else None
    if not isinstance(bg, (list, tuple)) or len(bg) != 2:
        raise E("cfg.roi_sampling.bg_iou = %r (a pair {lo, hi})" % (out["bg_iou"],))
    for v in bg:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise E("cfg.roi_sampling.bg_iou: %r is not a number" % (v,))
    if not 0.0 <= bg[0] <= bg[1] <= out["fg_iou"]:
        raise E("cfg.roi_sampling.bg_iou = {%g, %g} (need 0 <= lo <= hi <= fg_iou = %g)" % (bg[0], bg[1], out["fg_iou"]))
    out["bg_iou"] = (float(bg[0]), float(bg[1]))
    out["threshold"] = number("threshold", 0.0, 1.0)
    out["nms_overlap"] = number("nms_overlap", 0.0, 1.0, lo_open=True)
    out["pre_nms_top_n"] = integer("pre_nms_top_n", 1, Detector.NMS_FIRST_CAP)
    out["post_nms_top_n"] = integer("post_nms_top_n", 1, ROI_SAMPLING_MAX_CANDIDATES - ROI_SAMPLING_MAX_GT)
    out["seed"] = integer("seed", 0, 0xFFFFFFFF)
    out["hard_nms_overlap"] = number("hard_nms_overlap", 0.0, 1.0, lo_open=True)
    if out["source"] != "hard" and "hard_nms_overlap" not in t:   # (the validated table of the other sources stays the one it was)
        del out["hard_nms_overlap"]
    out["fg_quota"] = int(math.floor(out["batch"] * out["fg_fraction"] + 0.5))
    return out


CNET_LOSS_DEFAULTS = dict(cls="nll", gamma=2.0, alpha=None, label_smoothing=0.0, box="smooth_l1", beta=1.0, box_weight=10.0)


def cnet_loss_settings(cfg):
    """cfg["cnet_loss"] (not in the reference): which losses the classification net is trained on and reported with -> the
    validated settings, or None when the key is absent (then the pass is the reference's: frcnn_cnet_losses, objective.lua:170-177).
    With the key present -- {} included -- the losses run row by row in frcnn_cnet_loss_rows and are summed by
    frcnn_loss_accumulate (semantics and arithmetic: include/frcnn_hip_loss.h).
      cls              "nll" (default: ClassNLL averaged over the rows) or "focal" (Lin et al. 2017: -w (1 - p_t)^gamma log p_t)
      gamma            the focal exponent, 0 ... 5 (default 2; 0 is nll); unused under "nll"
      alpha            absent (default: every row weighs 1), or in (0, 1): a foreground row weighs alpha, a background row 1 - alpha
      label_smoothing  in [0, 1) (default 0): the target distribution is (1 - e) at the class plus e / classes everywhere; refused
                       with "focal" unless 0
      box              "smooth_l1" (default) or "giou" (Rezatofighi et al. 2019, taken in the space of the box deltas)
      beta             the SmoothL1 threshold, finite and > 0 (default 1: the reference's criterion); unused under "giou"
      box_weight       the factor of the box loss and of its gradient, finite and >= 0 (default 10: objective.lua:172-173)
    Raises FrcnnError -- before the model or the device is touched -- for an unknown key, a wrong type or a value out of range."""
    t = cfg.get("cnet_loss")
    if t is None:
        return None
    E = _lib.FrcnnError
    if not isinstance(t, dict):
        raise E("cfg.cnet_loss must be a table of {%s}" % ", ".join(CNET_LOSS_DEFAULTS))
    unknown = sorted(set(t) - set(CNET_LOSS_DEFAULTS), key=str)
    if unknown:
        raise E("cfg.cnet_loss: unknown key(s) %s" % ", ".join(map(str, unknown)))
    out = dict(CNET_LOSS_DEFAULTS)
    out.update(t)

    def number(key, ok, what):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise E("cfg.cnet_loss.%s = %r is not a finite number" % (key, v))
        if not ok(v):
            raise E("cfg.cnet_loss.%s = %r (%s)" % (key, v, what))
        return float(v)

    for key, names in (("cls", ("nll", "focal")), ("box", ("smooth_l1", "giou"))):
        if not isinstance(out[key], str) or out[key] not in names:
            raise E("cfg.cnet_loss.%s = %r (\"%s\" or \"%s\")" % ((key, out[key]) + names))
    out["gamma"] = number("gamma", lambda v: 0.0 <= v <= 5.0, "0 ... 5")
    if out["alpha"] is not None:
        out["alpha"] = number("alpha", lambda v: 0.0 < v < 1.0, "absent, or in (0, 1)")
    out["label_smoothing"] = number("label_smoothing", lambda v: 0.0 <= v < 1.0, "in [0, 1)")
    if out["cls"] == "focal" and out["label_smoothing"] != 0.0:
        raise E("cfg.cnet_loss.label_smoothing = %r is not defined under cls = \"focal\"" % (out["label_smoothing"],))
    out["beta"] = number("beta", lambda v: v > 0.0, "finite, > 0")
    out["box_weight"] = number("box_weight", lambda v: v >= 0.0, "finite, >= 0")
    return out


def box_head_settings(cfg):
    """cfg["box_head"] (not in the reference): the shape of the classification net's box head -> dict(per_class=bool).
      per_class   false (default; also the key absent and {}): the reference's Linear(nf, 4), one regressor for every class
                  (model_utilities.lua:117-124) -- the model, its parameter count, launches and results are unchanged;
                  true: a Linear(nf, 4 * class_count).  Row 4 (c - 1) + j of its weight and bias is coordinate j of foreground
                  class c; training moves the rows of each example's class, detection decodes the rows of the predicted class
                  (layout, class sources and arithmetic: include/frcnn_hip_box.h).
    Not combined with cfg.scoring.classes = "all", which decodes ONE box per candidate for all its class rows: that raises here --
    unless cfg.scoring.boxes = "class" (Detector.scoring_boxes) asks for the box of its own class for every class row, which in
    turn needs per_class = true and raises here with a shared head.
    Raises FrcnnError -- before the model or the device is touched -- for an unknown key or a value that is not a boolean."""
    t = cfg.get("box_head")
    E = _lib.FrcnnError
    out = dict(per_class=False)
    if t is not None:
        if not isinstance(t, dict):
            raise E("cfg.box_head must be a table of {per_class}")
        unknown = sorted(set(t) - set(out), key=str)
        if unknown:
            raise E("cfg.box_head: unknown key(s) %s" % ", ".join(map(str, unknown)))
        v = t.get("per_class", False)
        if not isinstance(v, (bool, np.bool_)):
            raise E("cfg.box_head.per_class = %r is not a boolean" % (v,))
        out["per_class"] = bool(v)
    sc = cfg.get("scoring")
    boxes = sc.get("boxes") if isinstance(sc, dict) else None      # (its value is validated by Detector.scoring_boxes)
    if out["per_class"] and isinstance(sc, dict) and sc.get("classes") == "all" and boxes != "class":
        raise E("cfg.box_head.per_class = true cannot be combined with cfg.scoring.classes = \"all\": that pass decodes one box per "
                "candidate for all its class rows, a per-class head has one box per (candidate, class); cfg.scoring.boxes = \"class\" "
                "gives every class row the box of its own class")
    if boxes == "class" and not out["per_class"]:
        raise E("cfg.scoring.boxes = \"class\" needs cfg.box_head.per_class = true: a shared box head has one box per candidate")
    return out


def cnet_loss_desc(settings, bgclass):
    """the validated settings of cnet_loss_settings -> the frcnn_cnet_loss_desc frcnn_cnet_loss_rows reads on the host"""
    return _lib.CnetLossDesc(cls=("nll", "focal").index(settings["cls"]), box=("smooth_l1", "giou").index(settings["box"]),
                             bgclass=int(bgclass), gamma=settings["gamma"], alpha=-1.0 if settings["alpha"] is None else settings["alpha"],
                             smoothing=settings["label_smoothing"], beta=settings["beta"], box_weight=settings["box_weight"])


def ground_truth_table(x, class_count=None):
    """The ground truth of a batch entry for frcnn_proposal_targets_batch: x["rois"] (objects with .rect and .class_index) ->
    (gt_rect G x 4 float64, gt_class G int32).  Raises FrcnnError for an entry without the key, more than 64 boxes, a box whose
    width or height is not positive, or (class_count given) a class outside 1 ... class_count."""
    if "rois" not in x or x["rois"] is None:
        raise _lib.FrcnnError("cfg.roi_sampling.source = \"proposals\" needs the ground truth of every batch entry: "
                              "the entry has no key \"rois\"")
    rois = list(x["rois"])
    if len(rois) > ROI_SAMPLING_MAX_GT:
        raise _lib.FrcnnError("roi_sampling: an image with %d ground-truth boxes (at most %d)" % (len(rois), ROI_SAMPLING_MAX_GT))
    gt = np.array([(r.rect.minX, r.rect.minY, r.rect.maxX, r.rect.maxY) for r in rois], dtype=np.float64).reshape(-1, 4)
    cls = np.array([r.class_index for r in rois], dtype=np.int32).reshape(-1)
    if len(rois) and not (np.all(np.isfinite(gt)) and np.all(gt[:, 2] - gt[:, 0] > 0) and np.all(gt[:, 3] - gt[:, 1] > 0)):
        raise _lib.FrcnnError("roi_sampling: a ground-truth box without a positive, finite width and height")
    if class_count is not None and len(rois) and (cls.min() < 1 or cls.max() > class_count):
        raise _lib.FrcnnError("roi.class_index %d outside 1..%d (class_count)"
                              % (int(cls.min() if cls.min() < 1 else cls.max()), class_count))
    return gt, cls


class _Scratch(object):
    """Per-objective device scratch that grows on demand (no allocation in the steady state)."""

    def __init__(self):
        self.bufs = {}

    def get(self, name, shape, dtype=np.float32):
        need = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        b = self.bufs.get(name)
        if b is None or b.nbytes < need:
            b = DeviceTensor.empty((max(need, 256),), np.uint8)
            self.bufs[name] = b
        return DeviceTensor(b.ptr, shape, dtype, owner=b)


class _PinnedRing(object):
    """Page-locked staging buffers for the per-image example tables: an upload from ordinary host memory blocks the host until
    the stream has reached it (the host then issues the launches that follow with the device already waiting: measured as a
    ~0.45 ms hole in every step); from page-locked memory frcnn_memcpy_h2d is asynchronous and the host keeps its lead.  A slot
    is reused only after the copy that read it has run (event)."""

    def __init__(self, slots=4):
        self.slots = [None] * slots
        self.i = 0

    def stage(self, arr):
        """Copy the uint8 array into the next slot; returns (host address, done) -- call done() right after queuing the copy."""
        import torch
        k = self.i
        self.i = (k + 1) % len(self.slots)
        slot = self.slots[k]
        n = int(arr.nbytes)
        if slot is not None and slot["event"] is not None:
            slot["event"].synchronize()
        if slot is None or slot["bytes"] < n:
            if slot is not None:
                _lib.call("frcnn_host_free", C.c_void_p(slot["ptr"]))
            p = C.c_void_p()
            cap = max(n, 1 << 16)
            _lib.call("frcnn_host_alloc", C.byref(p), cap)
            slot = self.slots[k] = dict(ptr=p.value, bytes=cap, event=None)
        C.memmove(slot["ptr"], arr.ctypes.data, n)

        def done():
            ev = torch.cuda.Event()
            ev.record()
            slot["event"] = ev
        return slot["ptr"], done

    def __del__(self):
        for slot in self.slots:
            if slot is not None:
                try:
                    _lib.load().frcnn_host_free(C.c_void_p(slot["ptr"]))
                except Exception:
                    pass


class DeviceDivisor(object):
    """gradient:div(n) (objective.lua:200) with n on the device: the address of an fp64 count (plus what keeps it alive).
    The optimisers of utilities hand it to frcnn_scale_rmsprop_dev / frcnn_sgd / frcnn_nag."""

    def __init__(self, p, owner):
        self.ptr = int(p)
        self._owner = owner


def _dist():
    """The exchange back end of the step: the library's own communicator when one is active (comm.activate: RCCL through
    the C ABI, what a LuaJIT host uses), else an initialised torch.distributed process group, else None."""
    from . import comm
    c = comm.active()
    if c is not None:
        return c
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist
    except ImportError:
        pass
    return None


# bench.py at N = 1: a list that receives (label, lo, hi, waits_on, event) at every point of the pass where the all-reduce of a
# bucket of the flat gradient WOULD start at N > 1 (the same program points, the same streams), plus "step_begin" /
# "backward_end" marks -- the bucket schedule a first multi-GPU run can be compared with.  None: off.
exchange_probe = None


def _probe_mark(label, lo, hi, waits_on):
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()      # (on the current stream: the one the bucket's all-reduce would be ordered behind)
    exchange_probe.append((label, int(lo), int(hi), waits_on, e))


def allreduce_begin(gradient, lo, hi):
    """Start the all-reduce of gradient[lo:hi] (a bucket whose values are final) without waiting for it: RCCL
    runs it on its own stream, ordered after the kernels already queued on the current stream, beside whatever
    the caller queues next.  Returns a handle for allreduce_gradient_and_stats(pending=...) or None (single
    process)."""
    dist = _dist()
    if dist is None or hi <= lo:
        return None
    return (lo, hi, dist.all_reduce(gradient[lo:hi], async_op=True))


def uncovered(done, ranges):
    """The parts of `ranges` (sorted, disjoint [lo, hi) pairs) that no pair of `done` covers, in order."""
    done = sorted(done)
    out = []
    for lo, hi in ranges:
        pos = lo
        for dlo, dhi in done:
            if dhi <= pos or dlo >= hi:
                continue
            if dlo > pos:
                out.append((pos, dlo))
            pos = max(pos, dhi)
        if pos < hi:
            out.append((pos, hi))
    return out


def allreduce_begin_rest(gradient, pending, ranges=None):
    """Start the all-reduce of every part of `gradient` (of `ranges`, the trainable slices of a staged pass) that no
    handle in `pending` covers yet (the vector is final).  Returns the extended list; lets the exchange run while the
    host still reads the accumulators."""
    if _dist() is None:
        return list(pending)
    done = sorted((p[0], p[1]) for p in pending if p is not None)
    out = [p for p in pending if p is not None]
    for lo, hi in uncovered(done, ranges if ranges is not None else [(0, gradient.numel())]):
        out.append(allreduce_begin(gradient, lo, hi))
    return out


def allreduce_gradient_and_stats(gradient, tot, pending=(), ranges=None):
    """Data-parallel exchange step: sum the flat gradient (in place) and the 8 fp64
    accumulators {cls_loss, reg_loss, cls_count, reg_count, creg_loss, creg_count, ccls_loss,
    ccls_count} (objective.lua:52-58) over all ranks.  `gradient` is a torch tensor (CUDA: RCCL over
    xGMI through torch.distributed's "nccl" backend; CPU: gloo, used by the tests).  Buckets already started
    with allreduce_begin() (`pending`) are only waited for; the rest of the vector (of `ranges`, the trainable slices of
    a staged pass) is reduced here.  No-op without an initialised process group."""
    dist = _dist()
    if dist is None:
        return tot
    import torch
    t = torch.from_numpy(np.asarray(tot, dtype=np.float64)).to(gradient.device)
    done = sorted((lo, hi) for lo, hi, _ in [p for p in pending if p is not None])
    works = [w for _, _, w in [p for p in pending if p is not None]]
    for lo, hi in uncovered(done, ranges if ranges is not None else [(0, gradient.numel())]):
        works.append(dist.all_reduce(gradient[lo:hi], async_op=True))
    works.append(dist.all_reduce(t, async_op=True))
    for w in works:
        w.wait()
    return t.cpu().numpy()


TRAIN_DEFAULTS = dict(proposal=True, classification=True, frozen_blocks=0)


def train_settings(cfg, nblocks):
    """cfg["train"] (staged training, Faster R-CNN's 4-step alternating training) -> (frozen_blocks, proposal, classification).
    proposal: the anchor nets are trained and the RPN losses back-propagated; classification: the fine-tuning +
    classification stage (objective.lua:146-186) runs and is trained; frozen_blocks: the leading backbone blocks whose
    parameters stay fixed.  Missing keys take TRAIN_DEFAULTS (everything trained).  Raises FrcnnError on a bad setting."""
    t = cfg.get("train")
    if t is None:
        t = {}
    if not isinstance(t, dict):
        raise _lib.FrcnnError("cfg.train must be a table of {proposal, classification, frozen_blocks}")
    unknown = sorted(set(t) - set(TRAIN_DEFAULTS))
    if unknown:
        raise _lib.FrcnnError("cfg.train: unknown key(s) %s" % ", ".join(map(str, unknown)))
    proposal = t.get("proposal", True)
    classification = t.get("classification", True)
    fb = t.get("frozen_blocks", 0)
    if not isinstance(proposal, bool) or not isinstance(classification, bool):
        raise _lib.FrcnnError("cfg.train: proposal and classification must be booleans")
    if isinstance(fb, bool) or not isinstance(fb, (int, np.integer)) or not 0 <= fb <= nblocks:
        raise _lib.FrcnnError("cfg.train.frozen_blocks = %r outside 0..%d (the backbone's blocks)" % (fb, nblocks))
    if not proposal and not classification:
        raise _lib.FrcnnError("cfg.train: proposal and classification are both off (no loss to back-propagate)")
    return int(fb), proposal, classification


def trainable_ranges(block_ranges, heads_range, cnet_range, frozen_blocks, proposal, classification):
    """The trainable slices of the flat vector, sorted and merged: the backbone blocks from frozen_blocks on (block_ranges:
    [lo, hi) per block, in order), the anchor nets' heads_range when proposal, the classification net's cnet_range when
    classification.  Raises FrcnnError when nothing is trainable."""
    parts = [tuple(block_ranges[b]) for b in range(frozen_blocks, len(block_ranges))]
    if proposal:
        parts.append(tuple(heads_range))
    if classification:
        parts.append(tuple(cnet_range))
    out = []
    for lo, hi in sorted(p for p in parts if p[1] > p[0]):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    if not out:
        raise _lib.FrcnnError("cfg.train: no trainable parameter left")
    return out


def create_objective(model, weights, gradient, batch_iterator, stats):  # objective.lua:15
    cfg = model["cfg"]
    pnet = model["pnet"]
    cnet = model["cnet"]
    native = model["native"]
    bgclass = cfg["class_count"] + 1  # :20
    localizer = Localizer(pnet.outnode.children[4] if len(pnet.outnode.children) == 5
                          else pnet.outnode.children[-1])  # :22 children[5]
    kh, kw, method, sampling = roi_pooling_settings(cfg)
    align = method == "align"
    inv_sx, inv_sy = align_geometry(localizer) if align else (0.0, 0.0)
    cnet_input_planes = model["layers"][-1]["filters"]
    D = kh * kw * cnet_input_planes
    ncls = cfg["class_count"] + 1
    per_class = bool(native.desc.box_per_class)   # cfg.box_head as the model was built with it (box_head_settings)
    scratch = _Scratch()
    pinned = _PinnedRing()
    import torch
    # the accumulators of objective.lua:52-58, and behind them the gradient guard's record {S, norm, D', skipped}
    # (frcnn_grad_clip, queued by the optimisers of utilities when asked for): one device vector, so that a guarded step
    # reads both back in one copy
    acc_all = torch.zeros(12, dtype=torch.float64, device="cuda")
    acc_t = acc_all[:8]
    acc_dev = DeviceTensor(acc_t.data_ptr(), (8,), np.float64, owner=acc_t)
    acc_pin = torch.zeros(8, dtype=torch.float64).pin_memory()
    acc_event = torch.cuda.Event()
    guard = dict(armed=False, deferred=False, divisor=None, pin=None)
    L = _lib.load()
    # Data parallel, device tail: the four example counts of objective.lua:194-198 are host-side numbers known before
    # any kernel runs.  They are uploaded into the unused slots 2, 3, 6, 7 of the accumulator vector at the start of the
    # pass (instead of zeroing it), travel through the same 8-element fp64 all-reduce as the loss sums, and the optimiser
    # reads the divisor of gradient:div(cls_count) from the device (frcnn_scale_rmsprop_dev): no host read-back and no
    # host-side collective between the backward pass and the update, with RCCL through torch.distributed or through the
    # library's own communicator alike.  FRCNN_DP_SYNC_TAIL=1 keeps the synchronous exchange (read-back, then scale).
    dev_tail_ok = not os.environ.get("FRCNN_DP_SYNC_TAIL")

    # data parallel: the slices of the deep backbone blocks are final long before the backward pass ends (the deepest
    # block's weight gradients come first); their all-reduces start behind a per-block event on an auxiliary stream
    early_blocks = []
    aux_stream = [None]
    if os.environ.get("FRCNN_DP_EARLY_BLOCKS", "1") != "0":
        nblk = int(native.desc.nblocks)
        early_blocks = [b for b in range(nblk - 1, 0, -1)
                        if pnet.block_param_range(b)[1] - pnet.block_param_range(b)[0] >= (1 << 18)]

    def cleanAnchors(examples, outputs):  # objective.lua:32-43
        return [e for e in examples
                if not (e[0].index[1] > outputs[e[0].layer - 1].shape[1] or e[0].index[2] > outputs[e[0].layer - 1].shape[2])]

    # ---- cfg["roi_sampling"] (roi_sampling_settings): under source = "proposals" the classification net's rows are a sample of
    # the first NMS's candidates on the pass's own head maps (sample_proposals below); absent or "examples": nothing here runs
    rs_state = dict(images=0, aw=None, ah=None, loc=None)

    loss_state = dict(settings=None, desc=None)   # cfg.cnet_loss of the pass being queued (lossAndGradient sets it)

    def cnet_losses(crout, crtarget, ccout, cctarget, R, npos_rows, crdelta, ccdelta):
        """objective.lua:170-177 on R rows, the first npos_rows of them foreground: frcnn_cnet_losses, or -- under cfg.cnet_loss --
        frcnn_cnet_loss_rows and the fixed-order sum of its rows into the same two accumulators"""
        s = stream_ptr()
        if loss_state["desc"] is None:
            _lib.call("frcnn_cnet_losses", ptr(crout), ptr(crtarget), ptr(ccout), ptr(cctarget), R, npos_rows, ncls,
                      ptr(crdelta), ptr(ccdelta), C.c_void_p(acc_dev.ptr + 4 * 8), s)
            return
        row_loss = scratch.get("cl_row_loss", (R, 2), np.float64)
        _lib.call("frcnn_cnet_loss_rows", ptr(crout), ptr(crtarget), ptr(ccout), ptr(cctarget), None, R, npos_rows, ncls,
                  C.byref(loss_state["desc"]), ptr(crdelta), ptr(ccdelta), ptr(row_loss), None, None, s)
        _lib.call("frcnn_loss_accumulate", ptr(row_loss), R, C.c_void_p(acc_dev.ptr + 4 * 8), s)

    def sampling_on():
        """the validated settings when this pass trains the classification net on sampled proposals, else None"""
        rs = roi_sampling_settings(cfg)
        if rs is None or rs["source"] not in ("proposals", "hard") or not train_settings(cfg, nblk_all)[2]:
            return None
        return rs

    def sample_proposals(rs, outputs, H, W, d_gt, d_gc, G):
        """Detector.lua:39-85 on the training pass's own head maps, then the proposal-target layer, all on the caller's stream
        with the counts on the device: frcnn_rpn_scan_batch (B = 1) at rs.threshold, frcnn_topk_select + frcnn_rpn_gather_rows
        (rects and the score rows {box, p}), frcnn_nms_device_batch keyed by the score, frcnn_proposal_targets_batch; then ONE
        read-back of the four counts -> (record, F, Bq): record holds the device buffers (debug["roi_sampling"])."""
        if rs_state["aw"] is None:
            a = Anchors(pnet, cfg["scales"])
            rs_state["aw"], rs_state["ah"] = DeviceTensor.from_numpy(a.w), DeviceTensor.from_numpy(a.h)
            rs_state["loc"] = np.array([[l["kW"], l["kH"], l["dW"], l["dH"], l["padW"], l["padH"]] for l in localizer.layers],
                                       dtype=np.int32).reshape(-1, 6)
        s = stream_ptr()
        i32 = np.int32
        hw = [tuple(o.shape[1:]) for o in outputs[:4]]
        Hs = (C.c_int * 4)(*[h for h, _ in hw]); Ws = (C.c_int * 4)(*[w for _, w in hw])
        cap = sum(int(o.shape[0]) // 6 * h * w for o, (h, w) in zip(outputs[:4], hw))   # every anchor of the four maps
        maps = (C.c_void_p * 4)(*[o.ptr for o in outputs[:4]])
        ctl = scratch.get("rs_ctl", (8,), i32)     # {nfg, nbg, F, Bq}, matches, selected rows, candidates
        c_n, c_k, c_R = (C.c_void_p(ctl.ptr + 4 * k) for k in (4, 5, 6))
        wsb = L.frcnn_rpn_scan_batch_workspace_bytes(Hs, Ws, 1)
        mp = scratch.get("rs_match_p", (cap,)); mi = scratch.get("rs_match_idx", (cap, 4), i32)
        mr = scratch.get("rs_match_rect", (cap, 4), np.float64); mb = scratch.get("rs_match_box", (cap, 4))
        _lib.call("frcnn_rpn_scan_batch", maps, Hs, Ws, 1, 0, ptr(rs_state["aw"]), ptr(rs_state["ah"]), float(W), float(H),
                  rs["threshold"], cap, ptr(mp), ptr(mi), ptr(mr), ptr(mb), c_n, ptr(scratch.get("rs_scan_ws", (wsb,), np.uint8)),
                  wsb, s)
        kcap = min(cap, rs["pre_nms_top_n"])
        sel = scratch.get("rs_sel", (kcap,), i32)
        wsb = L.frcnn_topk_select_workspace_bytes(1, cap)
        _lib.call("frcnn_topk_select", ptr(mp), 1, cap, cap, c_n, rs["pre_nms_top_n"], ptr(sel), kcap, c_k,
                  ptr(scratch.get("rs_sel_ws", (wsb,), np.uint8)), wsb, s)
        rect = scratch.get("rs_rect", (kcap, 4), np.float64); box5 = scratch.get("rs_box5", (kcap, 5))
        _lib.call("frcnn_rpn_gather_rows", ptr(mp), ptr(mi), ptr(mr), ptr(mb), 1, cap, cap, ptr(sel), kcap, c_k, kcap, None, None,
                  ptr(rect), None, ptr(box5), None, kcap, s)
        pick = scratch.get("rs_pick", (kcap,), np.int64)
        wsb = L.frcnn_nms_batch_workspace_bytes(1, kcap)
        _lib.call("frcnn_nms_device_batch", ptr(box5), 1, kcap, kcap, c_k, 5, C.c_float(rs["nms_overlap"]), 2, 5, None, ptr(pick),
                  c_R, ptr(scratch.get("rs_nms_ws", (wsb,), np.uint8)), wsb, s)
        seed = (rs["seed"] + rs_state["images"]) & 0xFFFFFFFF
        rs_state["images"] += 1
        r_cap = min(kcap, rs["post_nms_top_n"])
        # "hard": no quota cuts and the seed decides nothing -- every labelled candidate leaves, foreground rows first (the "all"
        # table of mine_hard, at most r_cap + 64 rows)
        hard = rs["source"] == "hard"
        rows = r_cap + (ROI_SAMPLING_MAX_GT if rs["include_gt"] else 0) if hard else rs["batch"]
        quota = rows if hard else rs["fg_quota"]
        pre = "rh_all_" if hard else "rs_"
        rec = dict(rect=rect, pick=pick, R=DeviceTensor(ctl.ptr + 24, (1,), i32, owner=ctl), stride=kcap,
                   r_cap=r_cap, seed=seed, settings=rs, bgclass=bgclass,
                   roi=scratch.get(pre + "roi", (rows, 4), np.float64), crtarget=scratch.get(pre + "crtarget", (rows, 4)),
                   cctarget=scratch.get(pre + "cctarget", (rows,)), src=scratch.get(pre + "src", (rows,), i32),
                   gt_idx=scratch.get(pre + "gt_idx", (rows,), i32), iou=scratch.get(pre + "iou", (rows,), np.float64))
        _lib.call("frcnn_proposal_targets_batch", ptr(rect), ptr(pick), kcap, c_R, rec["r_cap"], C.c_void_p(d_gt), C.c_void_p(d_gc),
                  max(G, 1), (C.c_int * 1)(G), 1, 1 if rs["include_gt"] else 0, rs["fg_iou"], rs["bg_iou"][0], rs["bg_iou"][1],
                  quota, rows, bgclass, C.c_uint(seed), ptr(rec["roi"]), ptr(rec["crtarget"]), ptr(rec["cctarget"]),
                  ptr(rec["src"]), ptr(rec["gt_idx"]), ptr(rec["iou"]), rows, ptr(ctl), s)
        host = np.zeros(4, i32)
        _lib.call("frcnn_memcpy_d2h", host.ctypes.data_as(C.c_void_p), ptr(ctl), 16, s)     # the ONE read-back of the stage
        _lib.call("frcnn_stream_sync", s)
        rec["counts"] = tuple(int(v) for v in host)
        return rec, rec["counts"][2], rec["counts"][3]

    def mine_hard(rs, rec, fm):
        """Online hard example mining behind sample_proposals (source = "hard"): rec holds the "all" table -- every labelled
        candidate, the F_all foreground rows first -- and its counts.  The N = F_all + B_all rows are pooled (no arg-max record)
        and scored by the classification net in evaluate mode (cnet.score: nothing is drawn, no state of the module changes);
        frcnn_roi_hard_keys_batch writes {rect, loss} rows, frcnn_nms_device_batch keyed by the loss at rs.hard_nms_overlap picks
        in descending loss order, frcnn_roi_hard_gather_batch writes the first rs.batch picks' rows, in ascending row order, as
        the training tables; then the stage's SECOND read-back, of the gather's four counts -> (F, Bq).  rec keeps its fields
        for the training tables and gains all, score, box5, loss, loss_sel, hard_pick and hard_counts = (F, Bq, survivors, N)."""
        s = stream_ptr()
        i32 = np.int32
        names = ("roi", "crtarget", "cctarget", "src", "gt_idx", "iou")
        nfg, nbg, Fa, Ba = rec["counts"]
        N, Ncap = Fa + Ba, int(rec["roi"].shape[0])
        rec["all"] = dict([(k, rec[k]) for k in names], counts=rec["counts"])
        rows = min(rs["batch"], Ncap)
        rec.update(roi=scratch.get("rs_roi", (rows, 4), np.float64), crtarget=scratch.get("rs_crtarget", (rows, 4)),
                   cctarget=scratch.get("rs_cctarget", (rows,)), src=scratch.get("rs_src", (rows,), i32),
                   gt_idx=scratch.get("rs_gt_idx", (rows,), i32), iou=scratch.get("rs_iou", (rows,), np.float64),
                   loss_sel=scratch.get("rh_loss_sel", (rows,)), score=None, box5=None, loss=None, hard_pick=None,
                   hard_counts=(0, 0, 0, 0), counts=(nfg, nbg, 0, 0))
        if N == 0:
            stats.setdefault("hard", []).append((0, 0))
            return 0, 0
        fmC, fmH, fmW = fm.shape
        cin = scratch.get("rh_cinput", (N, D))
        a = rec["all"]
        if align:
            _lib.call("frcnn_roi_align_forward", ptr(fm), fmC, fmH, fmW, ptr(a["roi"]), None, N, inv_sx, inv_sy, kh, kw, sampling,
                      ptr(cin), s)
        else:
            loc = rs_state["loc"]
            wins = scratch.get("rh_wins", (N, 4), i32)
            _lib.call("frcnn_roi_windows", ptr(a["roi"]), None, N, loc.ctypes.data_as(C.c_void_p), len(loc), fmH, fmW, ptr(wins), s)
            _lib.call("frcnn_roi_pool_forward", ptr(fm), fmC, fmH, fmW, ptr(wins), N, kh, kw, ptr(cin), None, s)
        outs = (scratch.get("rh_crout", (N, 4)), scratch.get("rh_ccout", (N, ncls)))
        # (a per-class box head scores the box of the class a row would be trained on; the shared head is called as ever)
        score = cnet.score(cin, outs, box_classes=("float", a["cctarget"])) if per_class else cnet.score(cin, outs)
        # {N, F_all, survivors, -}, then the gather's {F, Bq, survivors, N}: the row counts are host numbers since the first
        # read-back and travel back as 16 bytes from page-locked memory (the NMS reads its count on the device)
        hctl = scratch.get("rh_ctl", (8,), i32)
        hn, staged = pinned.stage(np.array([N, Fa, 0, 0], i32).view(np.uint8))
        _lib.call("frcnn_memcpy_h2d", ptr(hctl), C.c_void_p(hn), 16, s)
        staged()
        c_n, c_f, c_surv, c_out = (C.c_void_p(hctl.ptr + 4 * k) for k in (0, 1, 2, 4))
        box5 = scratch.get("rh_box5", (Ncap, 5)); loss = scratch.get("rh_loss", (Ncap,))
        if loss_state["desc"] is None:
            _lib.call("frcnn_roi_hard_keys_batch", ptr(a["roi"]), ptr(score[0]), ptr(a["crtarget"]), ptr(score[1]), ptr(a["cctarget"]), 1,
                      Ncap, Ncap, c_n, c_f, ncls, ptr(box5), ptr(loss), s)
        else:   # cfg.cnet_loss: the keys are the loss the rows will be trained on (scoring mode: the scores are only read)
            _lib.call("frcnn_cnet_loss_rows", ptr(score[0]), ptr(a["crtarget"]), ptr(score[1]), ptr(a["cctarget"]), ptr(a["roi"]), N, Fa,
                      ncls, C.byref(loss_state["desc"]), None, None, None, ptr(loss), ptr(box5), s)
        pick = scratch.get("rh_pick", (Ncap,), np.int64)
        wsb = L.frcnn_nms_batch_workspace_bytes(1, Ncap)
        _lib.call("frcnn_nms_device_batch", ptr(box5), 1, Ncap, Ncap, c_n, 5, C.c_float(rs["hard_nms_overlap"]), 2, 5, None, ptr(pick),
                  c_surv, ptr(scratch.get("rh_nms_ws", (wsb,), np.uint8)), wsb, s)
        _lib.call("frcnn_roi_hard_gather_batch", ptr(pick), c_surv, rs["batch"], ptr(a["roi"]), ptr(a["crtarget"]), ptr(a["cctarget"]),
                  ptr(a["src"]), ptr(a["gt_idx"]), ptr(a["iou"]), ptr(loss), 1, Ncap, Ncap, c_n, c_f, ptr(rec["roi"]),
                  ptr(rec["crtarget"]), ptr(rec["cctarget"]), ptr(rec["src"]), ptr(rec["gt_idx"]), ptr(rec["iou"]),
                  ptr(rec["loss_sel"]), rows, c_out, s)
        host = np.zeros(4, i32)
        _lib.call("frcnn_memcpy_d2h", host.ctypes.data_as(C.c_void_p), c_out, 16, s)     # the second read-back of the stage
        _lib.call("frcnn_stream_sync", s)
        F, Bq, surv, n = (int(v) for v in host)
        rec.update(score=score, box5=box5, loss=loss, hard_pick=pick, hard_counts=(F, Bq, surv, n), counts=(nfg, nbg, F, Bq))
        stats.setdefault("hard", []).append((n, surv))
        return F, Bq

    prepared = {}   # id(batch entry) -> (the entry itself, tables packed ahead of the pass: finish(), while the host waits for
                    # the device); the entry is held so that its id cannot be re-used by another object while the tables wait

    def map_sizes(H, W):
        """Sizes of the anchor nets' outputs and of the last pooled map for an H x W image (ceil-mode pooling,
        model_utilities.lua:23; valid k x k head convolution, :31) -- what pnet.forward will hand out."""
        from .synthetic import output_map_sizes
        h, w = H, W
        for l in model["layers"]:
            for _ in range(l["conv_steps"]):
                h = h + 2 * l["padH"] - l["kH"] + 1; w = w + 2 * l["padW"] - l["kW"] + 1
            h = -(-(h - 2) // 2) + 1; w = -(-(w - 2) // 2) + 1
        return [tuple(t) for t in output_map_sizes(model, H, W)], (h, w)

    def prepare_examples(x):
        """The host half of objective.lua:74-140 for one image: cleanAnchors, the example tables (anchor / ground-truth
        rectangles, (layer, aspect, y, x), classes), the ROI-pooling windows and the positions the sparse head backward
        will touch, packed into the ONE blob that is uploaded behind the forward pass."""
        from .synthetic import clean_examples
        shp = x["img"].shape
        sizes, (fmH, fmW) = map_sizes(int(shp[1]), int(shp[2]))
        p = clean_examples(x["positive"], sizes)  # :74-75
        n = clean_examples(x["negative"], sizes)
        npos, E = len(p), len(p) + len(n)
        prep = dict(p=p, n=n, sizes=sizes, fm=(fmH, fmW))
        if sampling_on() is not None:   # the ground-truth table of the proposal-target layer rides at the end of the blob
            gt, gcls = ground_truth_table(x, cfg["class_count"])
            G = len(gcls)
            # (G x 4 doubles, then G ints; an image without boxes carries one unread row)
            prep.update(gt_rect=gt, gt_class=gcls,
                        gt_blob=np.concatenate([gt.view(np.uint8).ravel() if G else np.zeros(32, np.uint8),
                                                gcls.view(np.uint8).ravel() if G else np.zeros(4, np.uint8)]))
        if E == 0:
            if "gt_blob" in prep:
                prep["blob"] = prep["gt_blob"]
                prep["gt_off"] = 0
            return prep
        anch = [e[0] for e in p] + [e[0] for e in n]
        ex_idx = np.array([(a.layer, a.aspect, a.index[1], a.index[2]) for a in anch], dtype=np.int32)
        ex_anchor = np.array([(a.minX, a.minY, a.maxX, a.maxY) for a in anch], dtype=np.float64)
        ex_roi = np.zeros((max(npos, 1), 4), dtype=np.float64)
        ex_class = np.zeros(max(npos, 1), dtype=np.int32)
        if npos:
            ex_roi[:npos] = [(e[1].rect.minX, e[1].rect.minY, e[1].rect.maxX, e[1].rect.maxY) for e in p]
            ex_class[:npos] = [e[1].class_index for e in p]
            if ex_class[:npos].min() < 1 or ex_class[:npos].max() > cfg["class_count"]:
                # nn.ClassNLLCriterion raises on a target outside 1..n (objective.lua:174); the batched loss
                # kernel indexes with it, so a stale index in a training-data file must stop here
                raise _lib.FrcnnError("roi.class_index %d outside 1..%d (class_count)"
                                      % (int(ex_class[:npos].min() if ex_class[:npos].min() < 1 else ex_class[:npos].max()),
                                         cfg["class_count"]))
        # positives pool the GT rect (:117), negatives pool the anchor rect itself (:137); RoIAlign takes the (E, 4) double rects
        # themselves in the place of the snapped windows
        pooled = np.concatenate([ex_roi[:npos], ex_anchor[npos:]], 0)
        wins = np.ascontiguousarray(pooled) if align else roi_windows(pooled, localizer, fmH, fmW)
        # positions where delta_outputs[l] will be non-zero (hint for the sparse head backward)
        sp = []
        for l in range(4):
            sel = ex_idx[ex_idx[:, 0] == l + 1]
            sp.append(np.unique((sel[:, 2] - 1) * sizes[l][1] + (sel[:, 3] - 1)).astype(np.int32))
        sp_all = np.concatenate(sp)
        head = [ex_anchor.view(np.uint8).ravel(), ex_roi.view(np.uint8).ravel(), ex_idx.view(np.uint8).ravel(),
                ex_class.view(np.uint8).ravel()]
        if align:   # (the rects are doubles: their offset in the blob is rounded up to 8 bytes)
            head.append(np.zeros(-sum(a.size for a in head) % 8, np.uint8))
        blob = np.concatenate(head + [wins.view(np.uint8).ravel(), sp_all.view(np.uint8).ravel()])
        if "gt_blob" in prep:   # (doubles: at a multiple of 16 bytes)
            prep["gt_off"] = blob.size + (-blob.size % 16)
            blob = np.concatenate([blob, np.zeros(-blob.size % 16, np.uint8), prep["gt_blob"]])
        prep.update(ex_anchor=ex_anchor, ex_roi=ex_roi, ex_idx=ex_idx, ex_class=ex_class, wins=wins, sp=sp, blob=blob)
        return prep

    nblk_all = int(native.desc.nblocks)

    def stage_ranges():
        """cfg["train"] as it stands -> (frozen_blocks, proposal, classification, trainable ranges, or None for the whole vector)"""
        fb, prop, clsf = train_settings(model["cfg"], nblk_all)
        ranges = trainable_ranges([pnet.block_param_range(b) for b in range(nblk_all)], pnet.heads_param_range(),
                                  (native.pnet_params, gradient.numel()), fb, prop, clsf)
        return fb, prop, clsf, (None if ranges == [(0, gradient.numel())] else ranges)

    def run(w, defer, eager=None):
        """Queues the whole pass.  Returns finish() -> (loss, gradient); with defer=True (single process) the
        accumulators travel to pinned host memory asynchronously and finish() only waits for that copy, so the
        caller may queue more work (the optimiser step) before it looks at the loss."""
        # staged training (cfg.train, read at every call; validated before anything is queued): the library skips the frozen
        # parts' work (frcnn_model_set_trainable), this pass skips a disabled stage, and the optimiser updates `ranges` only
        guarded, guard["armed"] = guard["armed"], False   # (the optimiser armed the gradient guard for this very pass)
        guard["deferred"] = False
        guard["divisor"] = None
        frozen_blocks, proposal, classification, ranges = stage_ranges()
        rs = sampling_on()   # (cfg.roi_sampling: validated, like cfg.train, before anything is queued)
        cl = cnet_loss_settings(cfg)   # (cfg.cnet_loss likewise; None: the reference's losses, frcnn_cnet_losses)
        loss_state.update(settings=cl, desc=None if cl is None else cnet_loss_desc(cl, bgclass))
        if rs is not None:   # ... and so is the ground truth of the batch this pass will process
            if next_batch[0] is None:
                next_batch[0] = batch_iterator.nextTraining()
            try:
                for xb in next_batch[0]:
                    ground_truth_table(xb, cfg["class_count"])
            except _lib.FrcnnError:
                next_batch[0] = None   # (a refused batch is dropped: the next call draws a new one)
                prepared.clear()
                raise
        _lib.call("frcnn_model_set_trainable", native.h, frozen_blocks, int(proposal), int(classification))
        stage[0] = ranges
        trunk_frozen = frozen_blocks == nblk_all
        if w is not weights:  # :46-48
            weights.copy_(w)
        if packs_promise[0] is not None and packs_promise[0] != getattr(weights, "_version", None):
            # the packs renewed beside the previous pass were made from weights somebody has written since (torch counts
            # in-place writes; the library's own updates do not go through torch): the forward pass re-packs
            _lib.call("frcnn_pnet_invalidate_packs", native.h)
        packs_promise[0] = None
        s = stream_ptr()
        probing = exchange_probe is not None and _dist() is None and getattr(gradient, "is_cuda", False)
        if probing:
            _probe_mark("step_begin", 0, 0, "")
        _lib.call("frcnn_zero", ptr(gradient), gradient.numel() * 4, s)  # :49
        cls_count = reg_count = creg_count = ccls_count = 0
        pnet.training()  # :61-62
        cnet.training()
        batch = next_batch[0] if next_batch[0] is not None else batch_iterator.nextTraining()  # :64
        next_batch[0] = None
        pending = []
        early_copy = False
        # The update beside the backward pass (include/frcnn_hip.h): single process, one image per step, the side streams on.
        # eager = {update} from the optimiser (utilities.rmsprop / sgd / nag): update(weights, gradient, lo, hi, gscale, stream)
        # queues its step on elements [lo, hi); eager["done"] collects the slices updated on the update stream.
        if eager is not None:
            side = C.c_int(0)
            _lib.call("frcnn_get_option", b"side_stream", C.byref(side))
            if not (defer == "fold" and _dist() is None and len(batch) == 1 and side.value and w is weights
                    and getattr(gradient, "is_cuda", False)):
                eager = None
        if eager is not None:
            from .synthetic import clean_examples, output_map_sizes
            x0 = batch[0]
            held0 = prepared.get(id(x0))
            if held0 is not None and held0[0] is x0:
                n_ex = len(held0[1]["p"]) + len(held0[1]["n"])
            else:
                sizes0 = output_map_sizes(model, x0["img"].shape[1], x0["img"].shape[2])
                n_ex = len(clean_examples(x0["positive"], sizes0)) + len(clean_examples(x0["negative"], sizes0))
            eager["gscale"] = (1.0 / n_ex) if n_ex > 0 else 1.0   # gradient:div(cls_count), :200 (nothing to scale without examples)
            eager["done"] = []
            eager["ranges"] = ranges   # (staged training: the trainable slices, None = the whole vector)
            us = C.c_void_p()
            _lib.call("frcnn_model_update_stream", native.h, C.byref(us))
            nblk = int(native.desc.nblocks)

            def eager_slice(lo, hi, on, group=None):
                eager["update"](weights, gradient, lo, hi, eager["gscale"], on)
                eager["done"].append((int(lo), int(hi)))
                if group is not None:
                    _lib.call("frcnn_pnet_refresh_packs", native.h, ptr(weights), group, on)
                    eager["groups"].add(group)
            eager["groups"] = set()
            eager["slice"] = eager_slice
        dev_tail = (dev_tail_ok and defer == "fold" and _dist() is not None and getattr(gradient, "is_cuda", False)
                    and ranges is None    # (a staged pass: the optimisers' slice forms take a host divisor)
                    and rs is None)       # (sampled proposals: creg_count is known after the stage's read-back only)
        c4 = None
        if dev_tail:
            from .synthetic import clean_examples, output_map_sizes
            c4 = [0.0, 0.0, 0.0, 0.0]   # cls, reg, creg, ccls exactly as accumulated below (:194-198)
            for x in batch:
                shp = x["img"].shape
                sizes = output_map_sizes(model, shp[1], shp[2])
                np_, nn_ = len(clean_examples(x["positive"], sizes)), len(clean_examples(x["negative"], sizes))
                c4[0] += np_ + nn_; c4[1] += np_; c4[2] += np_; c4[3] += 1
            init = np.array([0.0, 0.0, c4[0], c4[1], 0.0, 0.0, c4[2], c4[3]], dtype=np.float64)
            hinit, staged = pinned.stage(init.view(np.uint8))
            _lib.call("frcnn_memcpy_h2d", ptr(acc_dev), C.c_void_p(hinit), 64, s)
            staged()
        else:
            acc_dev.zero_()
        for bi, x in enumerate(batch):
            last = bi == len(batch) - 1   # (by position: an iterator may hand out the same pooled image twice)
            # the example tables are host work that needs no device result (the map sizes follow from the image size): they
            # were packed while the host waited for the previous step (finish()), or are packed now -- before the forward
            # pass is queued, not between it and the stage that consumes them, where the device would run dry
            held = prepared.pop(id(x), None)
            prep = held[1] if held is not None and held[0] is x else prepare_examples(x)
            if rs is not None and "gt_blob" not in prep:   # (packed ahead, before the setting was switched on)
                prep = prepare_examples(x)
            img = to_device(x["img"])  # :66
            # :71 (the anchor nets stay in flight beside the cnet stage; sampled proposals: the scan reads their dense maps on this
            # stream -- the sampled-position path computes none -- so the pass waits for them)
            outputs = pnet.forward(img, async_heads=rs is None)
            if prep["sizes"] != [tuple(o.shape[1:]) for o in outputs[:len(prep["sizes"])]] or prep["fm"] != tuple(outputs[-1].shape[1:]):
                raise _lib.FrcnnError("lossAndGradient: the example tables were packed for other map sizes than this image's")
            p, n = prep["p"], prep["n"]  # :74-75
            delta_outputs = pnet.delta_outputs(zero=True)  # :78-84
            npos, nneg = len(p), len(n)
            E = npos + nneg
            fm = outputs[-1]
            fmC, fmH, fmW = fm.shape
            if E == 0 and rs is not None:   # (no example: the blob is the ground-truth table alone)
                blob = prep["blob"]
                dblob = scratch.get("blob", (blob.size,), np.uint8)
                hblob, staged = pinned.stage(blob)
                _lib.call("frcnn_memcpy_h2d", ptr(dblob), C.c_void_p(hblob), blob.nbytes, s)
                staged()
            if E > 0:
                ex_anchor, ex_roi, ex_idx, ex_class, wins, sp, blob = (prep[k] for k in ("ex_anchor", "ex_roi", "ex_idx", "ex_class", "wins", "sp", "blob"))
                dblob = scratch.get("blob", (blob.size,), np.uint8)
                hblob, staged = pinned.stage(blob)   # page-locked: the upload is asynchronous, the host keeps its lead
                _lib.call("frcnn_memcpy_h2d", ptr(dblob), C.c_void_p(hblob), blob.nbytes, s)
                staged()
                o = 0
                d_anchor = dblob.ptr + o; o += ex_anchor.nbytes
                d_roi = dblob.ptr + o; o += ex_roi.nbytes
                d_idx = dblob.ptr + o; o += ex_idx.nbytes
                d_class = dblob.ptr + o; o += ex_class.nbytes
                if align:
                    o += -o % 8
                d_wins = dblob.ptr + o; o += wins.nbytes
                for l in range(4):
                    _lib.call("frcnn_pnet_set_sparse_deltas", native.h, l + 1, C.c_void_p(dblob.ptr + o), len(sp[l]))
                    o += sp[l].nbytes
                # ---- RPN loss on the sampled anchors (objective.lua:91-140) ------------------
                # queued behind the anchor nets on the library's side stream, followed by their backward pass
                # (delta_outputs[1..4] are final after the loop: the fine-tuning stage only touches
                # delta_outputs[5], :182-185); this stream goes on with the cnet stage on the last map
                ex_loss = scratch.get("ex_loss", (E, 2), np.float64)
                crtarget = scratch.get("crtarget", (E, 4))
                cctarget = scratch.get("cctarget", (E,))
                pnet.anchor_loss_begin(d_idx, d_anchor, d_roi, d_class, npos, nneg, bgclass, ex_loss, crtarget,
                                       cctarget, acc_dev)
            F_rows = npos
            if rs is not None:
                # ---- the classification net on sampled proposals (cfg.roi_sampling): the candidates of the first NMS on this
                # pass's head maps (only head_forward writes them: the side stream's loss and backward launches read them beside
                # the scan), matched, labelled and sampled on the device; their rects are constants of the pass
                G = len(prep["gt_class"])
                d_gt = dblob.ptr + prep["gt_off"]
                rec, F_rows, Bq = sample_proposals(rs, outputs, int(img.shape[1]), int(img.shape[2]), d_gt, d_gt + 32 * max(G, 1), G)
                if rs["source"] == "hard":   # the rows of largest loss among them, chosen by the net as it stands
                    F_rows, Bq = mine_hard(rs, rec, fm)
                S = F_rows + Bq
                rec.update(gt_rect=prep["gt_rect"], gt_class=prep["gt_class"], cinput=None)
                debug["roi_sampling"] = rec
                stats.setdefault("rois", []).append(rec["counts"])
                if S == 0:
                    native.seed += 1              # (the cnet's dropout draw is skipped: the seed advances as its forward would)
                    pnet.anchor_loss_wait()       # (the accumulators are read on this stream)
                else:
                    cinput = rec["cinput"] = scratch.get("cinput", (S, D))
                    if align:
                        _lib.call("frcnn_roi_align_forward", ptr(fm), fmC, fmH, fmW, ptr(rec["roi"]), None, S, inv_sx, inv_sy,
                                  kh, kw, sampling, ptr(cinput), s)
                    else:
                        loc = rs_state["loc"]
                        dwins = scratch.get("rs_wins", (S, 4), np.int32)
                        pidx = scratch.get("pidx", (S, D), np.int32)
                        _lib.call("frcnn_roi_windows", ptr(rec["roi"]), None, S, loc.ctypes.data_as(C.c_void_p), len(loc), fmH, fmW,
                                  ptr(dwins), s)
                        _lib.call("frcnn_roi_pool_forward", ptr(fm), fmC, fmH, fmW, ptr(dwins), S, kh, kw, ptr(cinput), ptr(pidx), s)
                    crout, ccout = cnet.forward(cinput, box_classes=("float", rec["cctarget"])) if per_class else cnet.forward(cinput)
                    crdelta = scratch.get("crdelta", (S, 4))
                    ccdelta = scratch.get("ccdelta", (S, ncls))
                    pnet.anchor_loss_wait()       # (the accumulators: the anchor losses land in the same vector)
                    cnet_losses(crout, rec["crtarget"], ccout, rec["cctarget"], S, F_rows, crdelta, ccdelta)
                    rec.update(crout=crout, ccout=ccout, crdelta=crdelta, ccdelta=ccdelta)
                    post_roi_delta = cnet.backward(cinput, [crdelta, ccdelta])
                    if not trunk_frozen and align:
                        _lib.call("frcnn_roi_align_backward", ptr(delta_outputs[4]), fmC, fmH, fmW, ptr(post_roi_delta),
                                  ptr(rec["roi"]), None, S, inv_sx, inv_sy, kh, kw, sampling, s)
                    elif not trunk_frozen:
                        _lib.call("frcnn_roi_pool_backward", ptr(delta_outputs[4]), fmC, fmH, fmW, ptr(post_roi_delta), ptr(pidx),
                                  S, kh, kw, s)
            elif E > 0 and not classification:
                # staged training without the detector stage: no ROI pooling, no cnet; dcls / dreg are reported as NaN (finish).
                # The cnet's dropout draw is skipped too: the seed advances as its forward would advance it, so that every
                # later pass draws what it would draw unstaged
                native.seed += 1
                pnet.anchor_loss_wait()   # (the accumulators are read on this stream)
            elif E > 0:
                # ---- ROI pooling of every example in one launch (:117-119, :137-139) ---------
                cinput = scratch.get("cinput", (E, D))
                if align:
                    debug["rects"] = wins
                    _lib.call("frcnn_roi_align_forward", ptr(fm), fmC, fmH, fmW, C.c_void_p(d_wins), None, E, inv_sx, inv_sy,
                              kh, kw, sampling, ptr(cinput), s)
                else:
                    pidx = scratch.get("pidx", (E, D), np.int32)
                    _lib.call("frcnn_roi_pool_forward", ptr(fm), fmC, fmH, fmW, C.c_void_p(d_wins), E, kh, kw,
                              ptr(cinput), ptr(pidx), s)
                # ---- fine-tuning stage (:146-186) --------------------------------------------
                # (a per-class box head reads the classes from the example table: final on this stream since the upload above, so
                # the pass still overlaps frcnn_pnet_anchor_loss_begin, which writes cctarget on the side stream)
                coutputs = cnet.forward(cinput, box_classes=("int", d_class, npos)) if per_class else cnet.forward(cinput)  # :164
                crout, ccout = coutputs
                crdelta = scratch.get("crdelta", (E, 4))
                ccdelta = scratch.get("ccdelta", (E, ncls))
                pnet.anchor_loss_wait()   # crtarget is relative to the anchor nets' proposals (:156)
                cnet_losses(crout, crtarget, ccout, cctarget, E, npos, crdelta, ccdelta)  # :170-177
                debug["cnet_loss"] = dict(crout=crout, ccout=ccout, crtarget=crtarget, cctarget=cctarget, crdelta=crdelta,
                                          ccdelta=ccdelta, R=E, npos=npos, cinput=cinput)
                post_roi_delta = cnet.backward(cinput, [crdelta, ccdelta])  # :179
                if not trunk_frozen and align:   # (a frozen backbone: the library left the input gradient unwritten)
                    _lib.call("frcnn_roi_align_backward", ptr(delta_outputs[4]), fmC, fmH, fmW, ptr(post_roi_delta),
                              C.c_void_p(d_wins), None, E, inv_sx, inv_sy, kh, kw, sampling, s)
                elif not trunk_frozen:
                    _lib.call("frcnn_roi_pool_backward", ptr(delta_outputs[4]), fmC, fmH, fmW, ptr(post_roi_delta),
                              ptr(pidx), E, kh, kw, s)  # :182-185
            if E == 0:
                for l in range(4):
                    _lib.call("frcnn_pnet_set_sparse_deltas", native.h, l + 1, None, 0)
            if last and _dist() is not None:
                # the classification net's slice of the flat gradient (55 % of it) is final, and so is the anchor
                # nets' slice once the side stream's part is joined: their all-reduces run beside the backbone's
                # backward pass; only the backbone's 3.3 M elements remain for the end
                _lib.call("frcnn_cnet_backward_join", native.h, stream_ptr())   # its weight gradients ride on a stream of their own
                if classification:
                    pending.append(allreduce_begin(gradient, native.pnet_params, gradient.numel()))
                # The decision must not depend on this rank's data (every rank issues the same collectives): with the
                # side stream on and one image per batch the slice is final here on every rank -- either the
                # anchor nets' backward was started early and is joined now, or the image had no example and
                # contributes nothing to that slice.
                side = C.c_int(0)
                _lib.call("frcnn_get_option", b"side_stream", C.byref(side))
                if len(batch) == 1 and side.value and proposal:
                    pnet.backward_heads_join()
                    lo, hi = pnet.heads_param_range()
                    pending.append(allreduce_begin(gradient, lo, hi))
            if last and probing:   # (the same program points as the branch above, nothing exchanged)
                _lib.call("frcnn_cnet_backward_join", native.h, stream_ptr())
                _probe_mark("classification net", native.pnet_params, gradient.numel(), "frcnn_cnet_backward_join (its weight-gradient stream)")
                side = C.c_int(0)
                _lib.call("frcnn_get_option", b"side_stream", C.byref(side))
                if len(batch) == 1 and side.value:
                    pnet.backward_heads_join()
                    lo, hi = pnet.heads_param_range()
                    _probe_mark("anchor nets", lo, hi, "frcnn_pnet_backward_heads_join (the anchor nets' streams)")
            if last and defer and _dist() is None and not guarded:
                # (a guarded step reads the accumulators with the guard's record, behind the backward pass: guard_queued)
                # the eight statistics are final before the backbone's backward pass: their read-back is queued
                # here, so the caller's wait ends mid-step and the host queues the next step while this one
                # is still running (the device never drains between steps)
                acc_pin.copy_(acc_t, non_blocking=True)
                acc_event.record()
                early_copy = True
            debug["E"] = E
            pnet.backward(img, delta_outputs)  # :189
            if eager is not None:
                # On the update stream, once the caller's stream is inside the backbone's backward pass (matrix-core bound: the
                # bandwidth-bound update costs least beside it): the classification net's slice (55 % of the vector; its weight
                # gradients ran on this very stream), the anchor nets' slice and packs, then each backbone block as the pass leaves it
                # (that event follows the whole classification-net stage in stream order: its slice is final, its weights have
                # had their last reader -- also for an image without examples; the anchor nets may still be adding up their
                # parameter gradients)
                _lib.call("frcnn_pnet_wait_backward_begun", native.h, us)
                if classification:
                    eager_slice(native.pnet_params, gradient.numel(), us)
                _lib.call("frcnn_pnet_wait_heads_done", native.h, us)
                lo, hi = pnet.heads_param_range()
                if proposal:
                    eager_slice(lo, hi, us, nblk)
                for b in range(nblk, max(frozen_blocks, 1), -1):   # deepest block first: the order in which the pass leaves them; block 1 ends the pass
                    _lib.call("frcnn_pnet_wait_block_done", native.h, b, us)
                    lo, hi = pnet.block_param_range(b - 1)
                    eager_slice(lo, hi, us, b - 1)
                _lib.call("frcnn_model_update_join", native.h, stream_ptr())
            if last and _dist() is not None and early_blocks and getattr(gradient, "is_cuda", False):
                if aux_stream[0] is None:
                    aux_stream[0] = torch.cuda.Stream()
                for b in [b for b in early_blocks if b >= frozen_blocks]:   # deepest first: the order in which their gradients become final
                    lo, hi = pnet.block_param_range(b)
                    with torch.cuda.stream(aux_stream[0]):
                        pnet.wait_block_gradients(b)
                        pending.append(allreduce_begin(gradient, lo, hi))
            if last and probing:
                covered = []
                if early_blocks:
                    if aux_stream[0] is None:
                        aux_stream[0] = torch.cuda.Stream()
                    for b in early_blocks:
                        lo, hi = pnet.block_param_range(b)
                        with torch.cuda.stream(aux_stream[0]):
                            pnet.wait_block_gradients(b)
                            _probe_mark("backbone block %d" % (b + 1), lo, hi, "frcnn_pnet_wait_block_gradients(%d) on an auxiliary stream" % (b + 1))
                        covered.append((lo, hi))
                _probe_mark("backward_end", 0, 0, "")
                lo_rest = 0
                hi_rest = min([c[0] for c in covered] + [pnet.heads_param_range()[0]])
                _probe_mark("rest of the backbone", lo_rest, hi_rest, "end of frcnn_pnet_backward on the caller's stream")
            reg_count += npos  # :194-198
            cls_count += npos + nneg
            creg_count += F_rows   # (sampled proposals: the foreground rows regress)
            ccls_count += 1

        # ---- statistics: one read-back per call ------------------------------------------
        single = _dist() is None
        fold = single and defer == "fold" and cls_count > 0   # the optimiser folds gradient:div into its own pass
        if single and cls_count > 0 and not fold:  # the divisor is host-known: queue the scaling before the read-back
            _lib.call("frcnn_scale", ptr(gradient), gradient.numel(), 1.0 / cls_count, stream_ptr())  # :200
        counts = (cls_count, reg_count, creg_count, ccls_count)
        if not single:   # the rest of the gradient is final too: its exchange starts before the host read-back below
            pending[:] = allreduce_begin_rest(gradient, pending, ranges)
        if dev_tail:
            # asynchronous data-parallel tail: loss sums AND counts reduced on the device in one 8-element all-reduce
            assert [float(v) for v in (cls_count, reg_count, creg_count, ccls_count)] == c4, "count bookkeeping diverged"
            acc_work = _dist().all_reduce(acc_t, async_op=True)
            for pnd in pending:
                pnd[2].wait()           # RCCL: the current stream waits, the host does not
            acc_work.wait()
            if not guarded:
                acc_pin.copy_(acc_t, non_blocking=True)
                acc_event.record()
            fin = lambda: finish(None, None, (), True, reduced=True)
            guard["deferred"] = guarded
            guard["divisor"] = DeviceDivisor(acc_dev.ptr + 2 * 8, acc_all)
            return (fin, DeviceDivisor(acc_dev.ptr + 2 * 8, acc_t))   # slot 2 = the all-reduced cls_count (:200)
        if single and defer:
            if not early_copy and not guarded:
                acc_pin.copy_(acc_t, non_blocking=True)
                acc_event.record()
            guard["deferred"] = guarded
            guard["divisor"] = float(cls_count) if cls_count > 0 else None
            fin = lambda: finish(None, counts, pending, single, staged=(classification, ranges))
            if eager is not None:
                assert cls_count == 0 or eager["gscale"] == 1.0 / cls_count, "example count bookkeeping diverged"
                return (fin, eager["gscale"] if cls_count > 0 else None)
            return (fin, 1.0 / cls_count) if fold else fin
        if defer == "fold" and not single:   # the all-reduced count is known after finish(): scaling left to the caller
            res = finish(acc_dev.numpy(), counts, pending, single, fold=True, staged=(classification, ranges))
            gs = dp_gscale[0]
            guard["divisor"] = dp_count[0]
            fin = (lambda: (guard_stats(acc_all[8:12].cpu().numpy()), res)[1]) if guarded else (lambda: res)   # (this tail waits anyway)
            return (fin, gs) if gs is not None else fin
        return (lambda r: (lambda: r))(finish(acc_dev.numpy(), counts, pending, single, staged=(classification, ranges)))

    dp_gscale = [None]
    dp_count = [None]    # the all-reduced cls_count behind dp_gscale, as the gradient guard's divisor
    packs_promise = [None]   # weights._version at the moment every pack group had been renewed beside a pass (else None)
    debug = dict(scratch=scratch, E=0)
    next_batch = [None]
    prefetch_batches = os.environ.get("FRCNN_PREFETCH_BATCH", "1") != "0"

    stage = [None]   # the trainable ranges of the last pass queued (None: the whole vector)

    def finish(a, counts, pending, single, fold=False, reduced=False, staged=(True, None)):
        if a is None:
            # deferred read-back: the whole step is queued, the device is busy -- the next batch (image decoding hand-over,
            # processImage launches, example assembly: host work of the loader) is drawn now instead of at the start of
            # the next call, where the device would wait for it.  Same call sequence on the iterator, one call early.
            if next_batch[0] is None and prefetch_batches:
                next_batch[0] = batch_iterator.nextTraining()
                prepared.clear()
                for xb in next_batch[0]:   # ... and its example tables are packed (host work with no device input)
                    prepared[id(xb)] = (xb, prepare_examples(xb))
            acc_event.synchronize()
            a = (guard["pin"] if guard["deferred"] else acc_pin).numpy().copy()
        if counts is None:   # device tail: the (all-reduced) counts sit in the slots the kernels leave alone
            counts = (a[2], a[3], a[6], a[7])
        cls_count, reg_count, creg_count, ccls_count = counts
        tot = np.array([a[0], a[1], cls_count, reg_count, a[4], creg_count, a[5], ccls_count], dtype=np.float64)
        if not reduced:   # (asynchronous data-parallel tail: gradient, accumulators and counts are already summed)
            tot = allreduce_gradient_and_stats(gradient, tot, pending, staged[1])  # DP: no-op for a single process
        cls_loss, reg_loss, cls_count, reg_count, creg_loss, creg_count, ccls_loss, ccls_count = tot
        dp_gscale[0] = dp_count[0] = None
        if not single and cls_count > 0:
            if fold:
                dp_gscale[0] = 1.0 / cls_count
                dp_count[0] = float(cls_count)
            else:
                _lib.call("frcnn_scale", ptr(gradient), gradient.numel(), 1.0 / cls_count, stream_ptr())  # :200
        with np.errstate(divide="ignore", invalid="ignore"):
            pcls = float(np.float64(cls_loss) / cls_count)  # :202-205
            preg = float(np.float64(reg_loss) / reg_count)
            dcls = float(np.float64(ccls_loss) / ccls_count)
            dreg = float(np.float64(creg_loss) / creg_count)
        if not staged[0]:   # staged training without the detector stage: nothing was computed for it
            dcls = dreg = float("nan")
        if stats.get("verbose"):
            print("prop: cls: %f (%d), reg: %f (%d); det: cls: %f, reg: %f" % (pcls, cls_count, preg, reg_count, dcls, dreg))
        stats["pcls"].append(pcls); stats["preg"].append(preg)  # :211-214
        stats["dcls"].append(dcls); stats["dreg"].append(dreg)
        if guard["deferred"]:
            guard_stats(a[8:12])
        return pcls + preg, gradient  # :216-217

    def guard_stats(rec):
        """the gradient guard ran in this step: its norm (before clipping) joins the loss series, a skipped step is counted"""
        stats.setdefault("gnorm", []).append(float(rec[1]))
        stats["skipped"] = stats.get("skipped", 0) + int(rec[3] != 0)

    class _Guard(object):
        """What guard_arm() hands the optimiser: ptr = the device address of the record double[4] {S, norm, D', skipped},
        record = D' as the DeviceDivisor of the update that follows, divisor() = D of the pass just queued (None: nothing to
        scale, a host count, or a DeviceDivisor), queued() = frcnn_grad_clip has been queued."""
        ptr = acc_all.data_ptr() + 8 * 8
        record = DeviceDivisor(acc_all.data_ptr() + 10 * 8, acc_all)

        @staticmethod
        def divisor():
            return guard["divisor"]

        @staticmethod
        def queued():
            if guard["deferred"]:   # the accumulators and the record travel to the host in one copy; finish() waits for it
                if guard["pin"] is None:
                    guard["pin"] = torch.zeros(12, dtype=torch.float64).pin_memory()
                guard["pin"].copy_(acc_all, non_blocking=True)
                acc_event.record()

    def guard_arm():
        guard["armed"] = True
        return _Guard

    def lossAndGradient(w):
        return run(w, False)()

    # private protocol with the optimisers of utilities: begin(w) queues the pass and returns (finish, gradient); the
    # optimiser queues its update and only then calls finish() for the loss (no device idle during the read-back)
    lossAndGradient.begin = lambda w: (run(w, True), gradient)
    # begin_fold(w) -> (finish, gradient, gscale): gradient:div(cls_count) (:200) is left to the caller, who folds it
    # into the first pass of its update (frcnn_scale_rmsprop, frcnn_sgd, frcnn_nag); gscale is None when there is nothing to scale
    def begin_fold(w, eager=None):
        """eager = dict(update=) (utilities.rmsprop / sgd / nag; update(weights, gradient, lo, hi, gscale, stream) queues the
        optimiser's step on elements [lo, hi), gscale = 1 meaning unscaled): the pass may apply that step to slices of the
        vectors as they become final (the update beside the backward pass, include/frcnn_hip.h); eager["done"] then lists the
        slices it has updated, eager["slice"](lo, hi, stream, group) updates another one, eager["groups"] the pack groups
        already renewed, and the caller finishes with eager["complete"]()."""
        r = run(w, "fold", eager)
        if eager is not None and "done" in eager:
            ngroups = int(native.desc.nblocks) + 1

            def complete():
                """The caller has updated the rest of the vector: renew the packs nobody has renewed yet (on the current
                stream) and remember which weights every pack now belongs to."""
                for g in range(ngroups):
                    if g not in eager["groups"]:
                        _lib.call("frcnn_pnet_refresh_packs", native.h, ptr(weights), g, stream_ptr())
                        eager["groups"].add(g)
                packs_promise[0] = getattr(weights, "_version", None)
            eager["complete"] = complete
        return (r[0], gradient, r[1]) if isinstance(r, tuple) else (r, gradient, None)
    lossAndGradient.begin_fold = begin_fold
    # the gradient guard (state.clipNorm / state.skipNonFinite of the optimisers): guard_arm() before begin_fold tells the coming
    # pass to leave the read-back of its accumulators to the optimiser, which queues frcnn_grad_clip behind the pass and then
    # calls queued(); finish() appends stats["gnorm"] and counts stats["skipped"]
    lossAndGradient.guard_arm = guard_arm
    # staged training (cfg["train"]): trainable_ranges() validates the configuration as it stands and returns the slices a
    # pass would train (None: the whole vector) -- what optim.nag's look-ahead needs before the pass; pass_ranges() returns
    # those of the last pass queued.  The optimisers of utilities update these slices only.
    lossAndGradient.trainable_ranges = lambda: stage_ranges()[3]
    lossAndGradient.pass_ranges = lambda: stage[0]
    lossAndGradient.debug = debug   # (tests: the scratch buffers, the example count and -- RoIAlign -- the rects of the image being processed)
    # cfg.roi_sampling.source = "proposals" / "hard": debug["roi_sampling"] holds the last image's sampler record -- the candidates (rect, pick, R,
    # stride, r_cap), the kernel's outputs (roi, crtarget, cctarget, src, gt_idx, iou, counts), the seed, the ground truth and cinput;
    # under "hard" those are the tables the net trained on, and the record gains all (every labelled candidate: the six tensors and
    # their counts), score (crout, ccout of the scoring pass), box5, loss, loss_sel, hard_pick and hard_counts (mine_hard)
    return lossAndGradient


def _accumulate_losses(ex_loss, E, acc_dev, s):
    """acc[0] += sum cls, acc[1] += sum reg (objective.lua:104,112,132), on device, fixed order."""
    _lib.call("frcnn_loss_accumulate", ptr(ex_loss), E, ptr(acc_dev), s)
