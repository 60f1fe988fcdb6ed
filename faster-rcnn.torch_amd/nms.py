"""nms(boxes, overlap, scores) -- host-side mirror of nms.lua:23-102 over frcnn_nms_host /
frcnn_nms_device.  Key dispatch is the reference's (nms.lua:37-43): a number selects that column
(1-based), the string 'area' selects the area, ANYTHING ELSE -- including a score tensor or None,
which is what both call sites of the reference pass (Detector.lua:82,133) -- sorts by max-y.
Returns the 1-based row ids of the survivors in pick order (a LongTensor in the reference).

soft_nms(boxes, overlap, score_col, ...) -- not in the reference: Soft-NMS (Bodla et al. 2017) over frcnn_soft_nms_batch, the
greedy loop that lowers the neighbours' scores instead of deleting them (semantics: include/frcnn_hip.h).

box_vote(boxes, picks, ...) and proposal_targets(rect, pick, R, gt_rect, gt_class, ...) -- not in the reference either: bounding-box
voting (frcnn_box_vote_batch) and the proposal-target layer of training on sampled proposals (frcnn_proposal_targets_batch).

roi_hard_select(roi, crout, crtarget, ccout, cctarget, nfg, ...) -- online hard example mining of the classification net's rows:
frcnn_roi_hard_keys_batch, the NMS keyed by the loss, frcnn_roi_hard_gather_batch.

cnet_loss(crout, crtarget, ccout, cctarget, npos, settings, ...) -- the losses of cfg["cnet_loss"] row by row: frcnn_cnet_loss_rows.

eval_match(rects, classes, confidences, gt_rects, gt_classes, iou_thresholds, ...) -- one frame's detections matched to its ground
truth at several IoU thresholds at once, for mean average precision: frcnn_eval_match_batch."""
import ctypes as C
import math
import numbers

import numpy as np

from . import _lib
from .tensor import DeviceTensor, ptr, stream_ptr


def _key(scores):
    if isinstance(scores, numbers.Number) and not isinstance(scores, bool):
        return 2, int(scores)
    if isinstance(scores, str) and scores == "area":
        return 1, 0
    return 0, 0  # nms.lua:42 "use max_y"


def nms(boxes, overlap, scores=None):
    key_mode, key_col = _key(scores)
    on_device = isinstance(boxes, DeviceTensor) or (hasattr(boxes, "is_cuda") and boxes.is_cuda)
    if on_device:
        n = boxes.shape[0] if len(boxes.shape) == 2 else 0
        if n == 0 or int(np.prod(boxes.shape)) == 0:
            return np.zeros(0, dtype=np.int64)
        ncols = boxes.shape[1]
        wsb = _lib.load().frcnn_nms_workspace_bytes(n)
        ws = DeviceTensor.empty((wsb,), np.uint8)
        # picks and their count in ONE device buffer (the count behind the n ids): one read-back, one wait for the device
        pick = DeviceTensor.empty((n + 1,), np.int64)
        _lib.call("frcnn_nms_device", ptr(boxes), n, ncols, C.c_float(overlap), key_mode, key_col, ptr(pick),
                  C.c_void_p(pick.ptr + 8 * n), ptr(ws), wsb, stream_ptr())
        host = pick.numpy()
        k = int(host[n:].view(np.int32)[0])
        return host[:k].copy()
    b = np.ascontiguousarray(boxes.detach().cpu().numpy() if hasattr(boxes, "detach") else boxes, dtype=np.float32)
    if b.size == 0:  # nms.lua:26-28
        return np.zeros(0, dtype=np.int64)
    n, ncols = b.shape
    pick = np.zeros(n, dtype=np.int64)
    count = C.c_int(0)
    _lib.call("frcnn_nms_host", b.ctypes.data_as(C.c_void_p), n, ncols, C.c_float(overlap), key_mode, key_col,
              pick.ctypes.data_as(C.c_void_p), C.byref(count))
    return pick[:count.value].copy()


SOFT_NMS_METHODS = ("hard", "linear", "gaussian")   # the C ABI's method 0, 1, 2


def soft_nms(boxes, overlap, score_col, method="gaussian", sigma=0.5, min_score=0.001, log_scores=False, classes=None):
    """Soft-NMS of the rows of boxes (n x ncols fp32, columns 1-4 = x1 y1 x2 y2, column score_col -- 1-based, >= 5 -- the score)
    -> (pick, scores): the 1-based int64 rows in pick order and their fp32 scores AT PICK (never increasing along pick).
      method      "hard": a row dies when its IoU with a pick exceeds overlap; "linear": its score is multiplied by 1 - IoU
                  then; "gaussian": every row's score is multiplied by exp(-IoU^2 / sigma) at every pick
      min_score   a row is alive while its score >= min_score, on the scale of the scores (log_scores: a log-probability)
      log_scores  the scores are log-probabilities: decays are added (linear: + log1p(-IoU), gaussian: - IoU^2 / sigma)
      classes     optional n integers: a pick only touches rows of its own class (all classes in one pass; a stable partition
                  of pick by class gives the per-class lists)
    Ties go to the higher row, as in nms().  A host array is uploaded; a device tensor is used where it is.  Runs on the
    device: there is no host twin."""
    if method not in SOFT_NMS_METHODS:
        raise ValueError("soft_nms: method = %r (one of %s)" % (method, ", ".join(SOFT_NMS_METHODS)))
    on_device = isinstance(boxes, DeviceTensor) or (hasattr(boxes, "is_cuda") and boxes.is_cuda)
    if not on_device:
        b = np.ascontiguousarray(boxes.detach().cpu().numpy() if hasattr(boxes, "detach") else boxes, dtype=np.float32)
        if b.size == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        if b.ndim != 2:
            raise ValueError("soft_nms: boxes must be n x ncols")
        boxes = DeviceTensor.from_numpy(b)
    shape = tuple(int(v) for v in boxes.shape)
    if len(shape) != 2 or shape[0] == 0 or int(np.prod(shape)) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    n, ncols = shape
    cls = None
    if classes is not None:
        if isinstance(classes, DeviceTensor) or (hasattr(classes, "is_cuda") and classes.is_cuda):
            cls = classes
        else:
            c = np.ascontiguousarray(classes.detach().cpu().numpy() if hasattr(classes, "detach") else classes).astype(np.int32)
            if c.shape != (n,):
                raise ValueError("soft_nms: %d rows, classes of shape %r" % (n, c.shape))
            cls = DeviceTensor.from_numpy(c)
    wsb = _lib.load().frcnn_soft_nms_workspace_bytes(1, n)
    ws = DeviceTensor.empty((wsb,), np.uint8)
    # the row count, the picks and their count in ONE device buffer of 8-byte words, the scores behind it
    ctl = DeviceTensor.from_numpy(np.array([n] + [0] * (n + 1), np.int64))
    out = DeviceTensor.empty((n,), np.float32)
    _lib.call("frcnn_soft_nms_batch", ptr(boxes), 1, n, n, ptr(ctl), ncols, int(score_col), SOFT_NMS_METHODS.index(method),
              C.c_float(overlap), C.c_float(sigma), C.c_float(min_score), 1 if log_scores else 0, ptr(cls) if cls is not None else None,
              C.c_void_p(ctl.ptr + 8), C.c_void_p(ctl.ptr + 8 * (n + 1)), ptr(out), 1, ptr(ws), wsb, stream_ptr())
    host = ctl.numpy()
    k = int(host[n + 1:].view(np.int32)[0])
    pick = host[1:1 + k].copy()
    return pick, out.numpy()[pick - 1].copy()


BOX_VOTE_WEIGHTS = ("uniform", "score", "log_score")   # the C ABI's weight_mode 0, 1, 2


def _on_device(x):
    return isinstance(x, DeviceTensor) or (hasattr(x, "is_cuda") and x.is_cuda)


def _device_array(x, dtype, shape, what):
    """x where it is when it is on the device, else uploaded as a contiguous array of dtype; shape: the shape a host array must have"""
    if _on_device(x):
        return x
    a = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x).astype(dtype)
    if a.shape != shape:
        raise ValueError("box_vote: %s of shape %r, expected %r" % (what, a.shape, shape))
    return DeviceTensor.from_numpy(a)


def box_vote(boxes, picks, overlap=0.5, score_col=5, weights="score", classes=None, rects=None):
    """Bounding-box voting (Gidaris & Komodakis 2015; not in the reference) over frcnn_box_vote_batch: for every winner -- the
    1-based rows `picks` of boxes (n x ncols fp32, columns 1-4 = x1 y1 x2 y2), e.g. what nms() or soft_nms() returned -- the
    weighted mean of the rows of its class that overlap it by an IoU >= overlap -> (rects: k x 4 float64, votes: k int32), in
    the order of picks.
      weights   "score": column score_col (1-based, >= 5) is a plain score and the weight; "log_score": it is a log-probability,
                the weight is its exp; "uniform": every voter weighs 1 (score_col is ignored).  A row whose weight is not a
                finite number > 0 does not vote
      classes   optional n integers: only rows of the winner's class vote
      rects     optional n x 4 float64: the coordinates that are averaged (membership is always decided on the fp32 boxes)
    A winner with fewer than two voters keeps its own coordinates bit for bit.  Host arrays are uploaded; device tensors are
    used where they are.  Runs on the device: there is no host twin (semantics: include/frcnn_hip.h)."""
    if weights not in BOX_VOTE_WEIGHTS:
        raise ValueError("box_vote: weights = %r (one of %s)" % (weights, ", ".join(BOX_VOTE_WEIGHTS)))
    empty = (np.zeros((0, 4), dtype=np.float64), np.zeros(0, dtype=np.int32))
    if not _on_device(boxes):
        b = np.ascontiguousarray(boxes.detach().cpu().numpy() if hasattr(boxes, "detach") else boxes, dtype=np.float32)
        if b.size == 0:
            return empty
        if b.ndim != 2:
            raise ValueError("box_vote: boxes must be n x ncols")
        boxes = DeviceTensor.from_numpy(b)
    shape = tuple(int(v) for v in boxes.shape)
    if len(shape) != 2 or int(np.prod(shape)) == 0:
        return empty
    n, ncols = shape
    hp = picks.numpy() if isinstance(picks, DeviceTensor) else (picks.detach().cpu().numpy() if hasattr(picks, "detach") else picks)
    hp = np.ascontiguousarray(hp).astype(np.int64).reshape(-1)
    k = int(hp.size)
    if k == 0:
        return empty
    if k > n or hp.min() < 1 or hp.max() > n:
        raise ValueError("box_vote: picks are 1-based rows of boxes, at most one per row (%d picks in [%d, %d], %d rows)"
                         % (k, hp.min(), hp.max(), n))
    dpick = picks if _on_device(picks) else DeviceTensor.from_numpy(hp)
    cls = None if classes is None else _device_array(classes, np.int32, (n,), "classes")
    rect = None if rects is None else _device_array(rects, np.float64, (n, 4), "rects")
    ctl = DeviceTensor.from_numpy(np.array([n, k], np.int32))          # the row count and the winner count
    out = DeviceTensor.empty((n, 4), np.float64)
    votes = DeviceTensor.empty((n,), np.int32)
    _lib.call("frcnn_box_vote_batch", ptr(boxes), 1, n, n, ptr(ctl), ncols, int(score_col), BOX_VOTE_WEIGHTS.index(weights),
              C.c_float(overlap), ptr(cls) if cls is not None else None, ptr(rect) if rect is not None else None, ptr(dpick),
              C.c_void_p(ctl.ptr + 4), ptr(out), ptr(votes), stream_ptr())
    return out.numpy()[hp - 1].copy(), votes.numpy()[hp - 1].copy()


def proposal_targets(rect, pick, R, gt_rect, gt_class, bgclass, include_gt=True, fg_iou=0.5, bg_iou=(0.0, 0.5), fg_quota=32,
                     batch=128, seed=0, r_cap=None):
    """The proposal-target layer of training on sampled proposals (cfg["roi_sampling"]; not in the reference) over
    frcnn_proposal_targets_batch, one segment on host arrays: the candidates -- the ground-truth boxes first (include_gt), then
    the first min(R, r_cap) of the 1-based rows `pick` of rect (n x 4 float64) -- are matched to gt_rect (G x 4 float64, classes
    gt_class, 1-based) by Rect.IoU, labelled foreground (best IoU >= fg_iou), background (bg_iou[0] <= best IoU < bg_iou[1]) or
    ignored, and thinned to at most fg_quota foreground and batch rows in all (a class over its quota keeps the rows with the
    smallest keys of the seeded hash) -> dict(roi S x 4 float64, crtarget S x 4 float32, cctarget S float32, src, gt_idx S int32,
    iou S float64, counts (nfg, nbg, F, Bq)) with S = F + Bq rows: the F foreground rows in candidate order, then the Bq background
    rows.  r_cap: the post-NMS cap (default: every pick).  Runs on the device: there is no host twin (semantics:
    include/frcnn_hip.h); a refused setting raises FrcnnError before anything is launched."""
    rect = np.ascontiguousarray(rect, dtype=np.float64).reshape(-1, 4)
    pick = np.ascontiguousarray(pick, dtype=np.int64).reshape(-1)
    gt_rect = np.ascontiguousarray(gt_rect, dtype=np.float64).reshape(-1, 4)
    gt_class = np.ascontiguousarray(gt_class, dtype=np.int32).reshape(-1)
    if gt_class.shape[0] != gt_rect.shape[0]:
        raise ValueError("proposal_targets: %d ground-truth boxes, %d classes" % (gt_rect.shape[0], gt_class.shape[0]))
    if pick.size and (pick.min() < 1 or pick.max() > rect.shape[0]):
        raise ValueError("proposal_targets: picks are 1-based rows of rect (picks in [%d, %d], %d rows)"
                         % (pick.min(), pick.max(), rect.shape[0]))
    r_cap = int(pick.size if r_cap is None else r_cap)
    if r_cap > pick.size:
        raise ValueError("proposal_targets: r_cap %d beyond the %d picks" % (r_cap, pick.size))
    G, batch = int(gt_rect.shape[0]), int(batch)
    rows = max(batch, 1)
    d_rect = DeviceTensor.from_numpy(rect if rect.size else np.zeros((1, 4)))
    d_pick = DeviceTensor.from_numpy(pick if pick.size else np.zeros(1, np.int64))
    d_gt = DeviceTensor.from_numpy(gt_rect if G else np.zeros((1, 4)))
    d_gc = DeviceTensor.from_numpy(gt_class if G else np.zeros(1, np.int32))
    ctl = DeviceTensor.from_numpy(np.array([0, 0, 0, 0, int(R), 0, 0, 0], np.int32))     # counts, then the candidate count
    out = dict(roi=DeviceTensor.empty((rows, 4), np.float64), crtarget=DeviceTensor.empty((rows, 4), np.float32),
               cctarget=DeviceTensor.empty((rows,), np.float32), src=DeviceTensor.empty((rows,), np.int32),
               gt_idx=DeviceTensor.empty((rows,), np.int32), iou=DeviceTensor.empty((rows,), np.float64))
    _lib.call("frcnn_proposal_targets_batch", ptr(d_rect), ptr(d_pick), max(int(rect.shape[0]), r_cap), C.c_void_p(ctl.ptr + 16), r_cap,
              ptr(d_gt), ptr(d_gc), G, (C.c_int * 1)(G), 1, 1 if include_gt else 0, float(fg_iou), float(bg_iou[0]),
              float(bg_iou[1]), int(fg_quota), batch, int(bgclass), C.c_uint(int(seed) & 0xFFFFFFFF), ptr(out["roi"]),
              ptr(out["crtarget"]), ptr(out["cctarget"]), ptr(out["src"]), ptr(out["gt_idx"]), ptr(out["iou"]), rows, ptr(ctl),
              stream_ptr())
    counts = tuple(int(c) for c in ctl.numpy()[:4])
    S = counts[2] + counts[3]
    res = dict((k, t.numpy()[:S].copy()) for k, t in out.items())
    res["counts"] = counts
    return res


def roi_hard_select(roi, crout, crtarget, ccout, cctarget, nfg, batch=128, overlap=0.7, src=None, gt_idx=None, iou=None):
    """Online hard example mining (cfg["roi_sampling"].source = "hard"; not in the reference) on host arrays, one segment:
    frcnn_roi_hard_keys_batch, frcnn_nms_device_batch keyed by the loss, frcnn_roi_hard_gather_batch.  roi (n x 4 float64), crout and
    crtarget (n x 4 float32), ccout (n x ncls float32 log-probabilities), cctarget (n float32, 1-based classes): the n <= 4096 labelled
    candidates, the first nfg of them foreground; src, gt_idx (int32) and iou (float64) travel with their rows (default: src = the
    row, gt_idx = -1, iou = 0).  A row's loss is -ccout[target] + 10 * SmoothL1(crout - crtarget) (foreground only) in fp32; the NMS
    at `overlap` picks in descending loss order (equal losses: the higher row first), and the first `batch` picks leave in ascending
    row order -> dict(roi, crtarget, cctarget, src, gt_idx, iou, loss: the S = F + Bq selected rows, foreground first; counts
    (F, Bq, survivors, n); box5 n x 5 float32, loss_all n float32, pick: the survivors, 1-based, in pick order).  Runs on the
    device: there is no host twin (semantics: include/frcnn_hip_hard.h); a refused setting raises FrcnnError before anything is launched."""
    roi = np.ascontiguousarray(roi, dtype=np.float64).reshape(-1, 4)
    n = int(roi.shape[0])
    crout = np.ascontiguousarray(crout, dtype=np.float32).reshape(-1, 4)
    crtarget = np.ascontiguousarray(crtarget, dtype=np.float32).reshape(-1, 4)
    cctarget = np.ascontiguousarray(cctarget, dtype=np.float32).reshape(-1)
    ccout = np.ascontiguousarray(ccout, dtype=np.float32)
    if ccout.ndim != 2 or ccout.shape[0] != n or ccout.shape[1] < 1:
        raise ValueError("roi_hard_select: ccout must be %d x ncls" % n)
    ncls = int(ccout.shape[1])
    src = np.arange(n, dtype=np.int32) if src is None else np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
    gt_idx = np.full(n, -1, np.int32) if gt_idx is None else np.ascontiguousarray(gt_idx, dtype=np.int32).reshape(-1)
    iou = np.zeros(n, np.float64) if iou is None else np.ascontiguousarray(iou, dtype=np.float64).reshape(-1)
    for name, a in (("crout", crout), ("crtarget", crtarget), ("cctarget", cctarget), ("src", src), ("gt_idx", gt_idx), ("iou", iou)):
        if a.shape[0] != n:
            raise ValueError("roi_hard_select: %s has %d rows, roi %d" % (name, a.shape[0], n))
    if not 0 <= int(nfg) <= n:
        raise ValueError("roi_hard_select: nfg %d outside 0 ... %d" % (nfg, n))
    batch = int(batch)
    rows = max(min(batch, n), 1)

    def dev(a):
        return DeviceTensor.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype))
    d = dict(roi=dev(roi), crout=dev(crout), crtarget=dev(crtarget), ccout=dev(ccout), cctarget=dev(cctarget), src=dev(src),
             gt_idx=dev(gt_idx), iou=dev(iou))
    ctl = DeviceTensor.from_numpy(np.array([n, int(nfg), 0, 0, 0, 0, 0, 0], np.int32))   # n, nfg, survivors, -, then the counts
    c_n, c_f, c_surv, c_out = (C.c_void_p(ctl.ptr + 4 * k) for k in (0, 1, 2, 4))
    box5 = DeviceTensor.empty((max(n, 1), 5), np.float32)
    loss = DeviceTensor.empty((max(n, 1),), np.float32)
    pick = DeviceTensor.empty((max(n, 1),), np.int64)
    out = dict(roi=DeviceTensor.empty((rows, 4), np.float64), crtarget=DeviceTensor.empty((rows, 4), np.float32),
               cctarget=DeviceTensor.empty((rows,), np.float32), src=DeviceTensor.empty((rows,), np.int32),
               gt_idx=DeviceTensor.empty((rows,), np.int32), iou=DeviceTensor.empty((rows,), np.float64),
               loss=DeviceTensor.empty((rows,), np.float32))
    s = stream_ptr()
    _lib.call("frcnn_roi_hard_keys_batch", ptr(d["roi"]), ptr(d["crout"]), ptr(d["crtarget"]), ptr(d["ccout"]), ptr(d["cctarget"]), 1, n, n,
              c_n, c_f, ncls, ptr(box5), ptr(loss), s)
    if n:
        wsb = _lib.load().frcnn_nms_batch_workspace_bytes(1, n)
        ws = DeviceTensor.empty((wsb,), np.uint8)
        _lib.call("frcnn_nms_device_batch", ptr(box5), 1, n, n, c_n, 5, C.c_float(overlap), 2, 5, None, ptr(pick), c_surv, ptr(ws),
                  wsb, s)
    _lib.call("frcnn_roi_hard_gather_batch", ptr(pick), c_surv, batch, ptr(d["roi"]), ptr(d["crtarget"]), ptr(d["cctarget"]),
              ptr(d["src"]), ptr(d["gt_idx"]), ptr(d["iou"]), ptr(loss), 1, n, n, c_n, c_f, ptr(out["roi"]), ptr(out["crtarget"]),
              ptr(out["cctarget"]), ptr(out["src"]), ptr(out["gt_idx"]), ptr(out["iou"]), ptr(out["loss"]), rows, c_out, s)
    counts = tuple(int(c) for c in ctl.numpy()[4:8])
    S = counts[0] + counts[1]
    res = dict((k, t.numpy()[:S].copy()) for k, t in out.items())
    res.update(counts=counts, box5=box5.numpy()[:n].copy(), loss_all=loss.numpy()[:n].copy(), pick=pick.numpy()[:counts[2]].copy())
    return res


def cnet_loss(crout, crtarget, ccout, cctarget, npos, settings=None, roi=None, train=True):
    """The losses of the classification net under cfg["cnet_loss"] (not in the reference beyond its defaults) on host arrays:
    frcnn_cnet_loss_rows.  crout and crtarget (R x 4 float32), ccout (R x ncls float32 log-probabilities), cctarget (R float32,
    1-based classes), the first npos rows foreground; settings: a table as cfg["cnet_loss"] takes it (None or {}: the defaults --
    NLL and SmoothL1 * 10), validated by cnet_loss_settings, with the background class ncls; roi (R x 4 float64): the rects of
    box5.  train=True: the training mode -- crdelta and ccdelta are written and the rows >= npos of crout zeroed; False: the
    scoring mode -- crout is only read.  -> dict(row_loss R x 2 float64 {box_weight * box, cls / R}, key R float32, loss
    (creg, ccls): frcnn_loss_accumulate's sums of row_loss, box5 R x 5 float32 with roi, and under train crout, crdelta, ccdelta).
    Runs on the device: there is no host twin (semantics: include/frcnn_hip_loss.h); a refused setting raises FrcnnError before
    anything is launched."""
    from .objective import cnet_loss_desc, cnet_loss_settings
    st = cnet_loss_settings(dict(cnet_loss={} if settings is None else settings))
    crout = np.ascontiguousarray(crout, dtype=np.float32).reshape(-1, 4)
    R = int(crout.shape[0])
    crtarget = np.ascontiguousarray(crtarget, dtype=np.float32).reshape(-1, 4)
    cctarget = np.ascontiguousarray(cctarget, dtype=np.float32).reshape(-1)
    ccout = np.ascontiguousarray(ccout, dtype=np.float32)
    if ccout.ndim != 2 or ccout.shape[0] != R or ccout.shape[1] < 1:
        raise ValueError("cnet_loss: ccout must be %d x ncls" % R)
    ncls = int(ccout.shape[1])
    if crtarget.shape[0] != R or cctarget.shape[0] != R:
        raise ValueError("cnet_loss: crtarget and cctarget need %d rows" % R)
    if roi is not None:
        roi = np.ascontiguousarray(roi, dtype=np.float64).reshape(-1, 4)
        if roi.shape[0] != R:
            raise ValueError("cnet_loss: roi has %d rows, crout %d" % (roi.shape[0], R))
    desc = cnet_loss_desc(st, ncls)

    def dev(a):
        return DeviceTensor.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype))
    n = max(R, 1)
    d_crout, d_crt, d_cco, d_cct = dev(crout), dev(crtarget), dev(ccout), dev(cctarget)
    d_roi = dev(roi) if roi is not None else None
    crdelta = DeviceTensor.zeros((n, 4)) if train else None
    ccdelta = DeviceTensor.zeros((n, ncls)) if train else None
    row_loss = DeviceTensor.zeros((n, 2), np.float64)
    key = DeviceTensor.zeros((n,))
    box5 = DeviceTensor.zeros((n, 5)) if roi is not None else None
    acc = DeviceTensor.zeros((2,), np.float64)
    s = stream_ptr()
    _lib.call("frcnn_cnet_loss_rows", ptr(d_crout), ptr(d_crt), ptr(d_cco), ptr(d_cct), ptr(d_roi) if d_roi is not None else None, R,
              int(npos), ncls, C.byref(desc), ptr(crdelta) if train else None, ptr(ccdelta) if train else None, ptr(row_loss),
              ptr(key), ptr(box5) if box5 is not None else None, s)
    _lib.call("frcnn_loss_accumulate", ptr(row_loss), R, ptr(acc), s)
    res = dict(row_loss=row_loss.numpy()[:R].copy(), key=key.numpy()[:R].copy(), loss=tuple(float(v) for v in acc.numpy()))
    if box5 is not None:
        res["box5"] = box5.numpy()[:R].copy()
    if train:
        res.update(crout=d_crout.numpy()[:R].copy(), crdelta=crdelta.numpy()[:R].copy(), ccdelta=ccdelta.numpy()[:R].copy())
    return res


def box_head(x, W, b, classes=None, lsm=None, n_fg=None, g=None, gW=None, gb=None):
    """The per-class box head of cfg["box_head"] (not in the reference) on host arrays: frcnn_box_head_forward and, with g given,
    frcnn_box_head_backward.  x (R x nf float32), W (4C x nf), b (4C).  The class source: classes as an int32 array with n_fg given
    (the first n_fg rows are foreground with those classes, the rest background), classes as a float32 array (a 1-based class
    per row, the cctarget format), or classes=None and lsm (R x ncls log-probabilities: the first maximum of each row).
    -> dict(out R x 4, sel R int32); with g (R x 4) also gfeat (R x nf) and gW, gb: the given arrays (default zeros) plus the
    gradient, classes without a row untouched.  Runs on the device: there is no host twin (semantics: include/frcnn_hip_box.h)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("box_head: x must be R x nf")
    R, nf = int(x.shape[0]), int(x.shape[1])
    W = np.ascontiguousarray(W, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    if W.ndim != 2 or W.shape[1] != nf or W.shape[0] % 4 or W.shape[0] < 4 or b.shape[0] != W.shape[0]:
        raise ValueError("box_head: W must be 4C x %d and b 4C" % nf)
    Cn = int(W.shape[0]) // 4
    kind, n, d_cls, d_lsm, ncls = 0, 0, None, None, 0

    def dev(a):
        return DeviceTensor.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype))
    if classes is None:
        if lsm is None:
            raise ValueError("box_head: classes or lsm")
        lsm = np.ascontiguousarray(lsm, dtype=np.float32)
        if lsm.ndim != 2 or lsm.shape[0] != R or lsm.shape[1] < 1:
            raise ValueError("box_head: lsm must be %d x ncls" % R)
        d_lsm, ncls = dev(lsm), int(lsm.shape[1])
    elif n_fg is not None:
        classes = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
        kind, n = 1, int(n_fg)
        if classes.shape[0] < n:
            raise ValueError("box_head: %d classes for n_fg = %d" % (classes.shape[0], n))
        d_cls = dev(classes)
    else:
        classes = np.ascontiguousarray(classes, dtype=np.float32).reshape(-1)
        if classes.shape[0] != R:
            raise ValueError("box_head: a float class per row (%d rows)" % R)
        kind, d_cls = 2, dev(classes)
    rows = max(R, 1)
    d_x, d_W, d_b = dev(x), dev(W), dev(b)
    out = DeviceTensor.zeros((rows, 4))
    sel = DeviceTensor.zeros((rows,), np.int32)
    s = stream_ptr()
    _lib.call("frcnn_box_head_forward", ptr(d_x), R, nf, ptr(d_W), ptr(d_b), Cn, ptr(d_cls) if d_cls is not None else None, kind, n,
              ptr(d_lsm) if d_lsm is not None else None, ncls, ptr(out), ptr(sel), s)
    res = dict(out=out.numpy()[:R].copy(), sel=sel.numpy()[:R].copy())
    if g is not None:
        g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1, 4)
        if g.shape[0] != R:
            raise ValueError("box_head: g must be %d x 4" % R)
        gW0 = np.zeros_like(W) if gW is None else np.ascontiguousarray(gW, dtype=np.float32).reshape(W.shape)
        gb0 = np.zeros_like(b) if gb is None else np.ascontiguousarray(gb, dtype=np.float32).reshape(b.shape)
        d_g, d_gW, d_gb = dev(g), dev(gW0), dev(gb0)
        gfeat = DeviceTensor.zeros((rows, nf))
        _lib.call("frcnn_box_head_backward", ptr(d_g), ptr(d_x), ptr(sel), R, nf, ptr(d_W), Cn, ptr(gfeat), ptr(d_gW), ptr(d_gb), s)
        res.update(gfeat=gfeat.numpy()[:R].copy(), gW=d_gW.numpy().copy(), gb=d_gb.numpy().copy())
    return res


def class_boxes(feat, row0, W, b, rect, pick, kc, keep_row, K, bb, r2, overrides=None):
    """frcnn_detect_class_boxes_batch (cfg["scoring"]["boxes"] = "class"; not in the reference) on host arrays: the box of ITS
    class for every row of an all-class class test.  feat (N x nf float32, every frame's feature rows), row0 (B first rows of
    the frames in feat), W (4C x nf) and b (4C) of a per-class box head, rect (B x match_stride x 4 float64) and pick
    (B x match_stride int64, 1-based rows of rect), kc and keep_row (B x row_stride int32: a row's 1-based class and 0-based
    candidate), K (B int32: the frames' row counts, read on the device), bb (B x row_stride x 5 float32) and r2
    (B x row_stride x 4 float64): the arrays the launch rewrites, as they are before it.
    -> dict(code, bb, r2): the library's return code (0: done; an argument error has launched nothing) and the two arrays after
    the call.  overrides: scalar arguments (nf, B, C, match_stride, row_stride) passed in place of the arrays' own, for the error
    paths.  Runs on the device: there is no host twin (semantics: include/frcnn_hip_classbox.h)."""
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    rect = np.ascontiguousarray(rect, dtype=np.float64)
    pick = np.ascontiguousarray(pick, dtype=np.int64)
    kc = np.ascontiguousarray(kc, dtype=np.int32)
    keep_row = np.ascontiguousarray(keep_row, dtype=np.int32)
    K = np.ascontiguousarray(K, dtype=np.int32).reshape(-1)
    bb = np.ascontiguousarray(bb, dtype=np.float32)
    r2 = np.ascontiguousarray(r2, dtype=np.float64)
    row0 = [int(v) for v in row0]
    if feat.ndim != 2 or W.ndim != 2 or W.shape[1] != feat.shape[1] or W.shape[0] % 4 or b.shape[0] != W.shape[0]:
        raise ValueError("class_boxes: feat must be N x nf, W 4C x nf and b 4C")
    B = len(row0)
    if rect.ndim != 3 or rect.shape[0] != B or rect.shape[2] != 4 or pick.shape != rect.shape[:2]:
        raise ValueError("class_boxes: rect must be B x match_stride x 4 and pick B x match_stride")
    if kc.ndim != 2 or kc.shape[0] != B or keep_row.shape != kc.shape or K.shape[0] != B:
        raise ValueError("class_boxes: kc and keep_row must be B x row_stride and K B")
    if bb.shape != kc.shape + (5,) or r2.shape != kc.shape + (4,):
        raise ValueError("class_boxes: bb must be B x row_stride x 5 and r2 B x row_stride x 4")
    a = dict(nf=int(feat.shape[1]), B=B, C=int(W.shape[0]) // 4, match_stride=int(rect.shape[1]), row_stride=int(kc.shape[1]))
    a.update(overrides or {})

    def dev(x):
        return DeviceTensor.from_numpy(x if x.size else np.zeros((1,) + x.shape[1:], x.dtype).reshape(-1))
    d = [dev(x) for x in (feat, W, b, rect, pick, kc, keep_row, K, bb, r2)]
    d_feat, d_W, d_b, d_rect, d_pick, d_kc, d_keep, d_K, d_bb, d_r2 = d
    row0_arg = (C.c_longlong * max(len(row0), 1))(*row0)
    code = _lib.load().frcnn_detect_class_boxes_batch(ptr(d_feat), a["nf"], row0_arg, a["B"], ptr(d_W), ptr(d_b), a["C"], ptr(d_rect),
                                                      ptr(d_pick), a["match_stride"], ptr(d_kc), ptr(d_keep), ptr(d_K),
                                                      a["row_stride"], ptr(d_bb), ptr(d_r2), stream_ptr())
    out_bb = d_bb.numpy().reshape(-1)[:bb.size].reshape(bb.shape).copy()
    out_r2 = d_r2.numpy().reshape(-1)[:r2.size].reshape(r2.shape).copy()
    return dict(code=int(code), bb=out_bb, r2=out_r2)


def winner_table(rects, classes, confidences, row_stride=None):
    """One frame's winner table as frcnn_detect_gather_batch lays it out ((row_stride + 1) x 16 float64: a 128-byte header whose
    int 3 is the winner count, then a record per winner with its class in column 0, its confidence in column 2 and its box r2 in
    columns 8-11; everything else zero) from host arrays: what eval_match() and the tests feed frcnn_eval_match_batch with."""
    rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
    n = int(rects.shape[0])
    classes = np.ascontiguousarray(classes).reshape(-1)
    confidences = np.ascontiguousarray(confidences, dtype=np.float32).reshape(-1)
    if classes.shape[0] != n or confidences.shape[0] != n:
        raise ValueError("winner_table: %d rects, %d classes, %d confidences" % (n, classes.shape[0], confidences.shape[0]))
    stride = n if row_stride is None else int(row_stride)
    if stride < n:
        raise ValueError("winner_table: row_stride %d below the %d winners" % (stride, n))
    tab = np.zeros((stride + 1, 16), np.float64)
    tab[0].view(np.int32)[:4] = (n, n, n, n)
    tab[1:n + 1, 0] = classes
    tab[1:n + 1, 2] = confidences
    tab[1:n + 1, 8:12] = rects
    return tab


def unpack_match(table, iou=None):
    """One frame's table of frcnn_eval_match_batch ((row_stride + 2) x 4 int32) -> dict(counts: the frame's four counts, n, G, T,
    winners, cls int32[n], confidence float32[n], tp uint32[n], gt int32[n]) and, with the frame's iou row given, iou float64[n]."""
    table = np.asarray(table).reshape(-1, 4)
    n = int(table[1, 0])
    rows = table[2:2 + n]
    out = dict(counts=tuple(int(v) for v in table[0]), n=n, G=int(table[1, 1]), T=int(table[1, 2]), winners=int(table[1, 3]),
               cls=rows[:, 0].astype(np.int32), confidence=np.ascontiguousarray(rows[:, 1]).view(np.float32).copy(),
               tp=np.ascontiguousarray(rows[:, 2]).view(np.uint32).copy(), gt=rows[:, 3].astype(np.int32))
    if iou is not None:
        out["iou"] = np.asarray(iou, dtype=np.float64).reshape(-1)[:n].copy()
    return out


def eval_match(rects, classes, confidences, gt_rects, gt_classes, iou_thresholds, max_detections=None):
    """frcnn_eval_match_batch (not in the reference) on host arrays, one frame: the detections (rects n x 4 float64, classes,
    confidences: in the order Detector.detect_batch lists them, or any other) matched to the frame's ground truth (gt_rects G x 4
    float64, gt_classes, 1-based; G <= 1024) at up to 16 IoU thresholds at once, by evaluation.mean_average_precision's rule: a
    detection looks at the box of its class it overlaps most (Rect.IoU, the first maximum), and at a threshold that box goes to the
    first detection, by decreasing fp32 confidence and then by row, that reaches it.
    max_detections = M: the M most confident detections only (frcnn_eval_conf_rows + frcnn_topk_select: Detector.keep_best's rule).
    -> dict(rows: the 0-based rows matched, ascending; cls, confidence (float32), tp (uint32: bit t set for a true positive at
    iou_thresholds[t]), gt (1-based box, 0: none), iou (float64: the best overlap, -1 without a box of the class)), one entry per
    matched row.  Runs on the device: there is no host twin (semantics: include/frcnn_hip_eval.h); a refused setting raises
    FrcnnError before anything is launched."""
    tab = winner_table(rects, classes, confidences)
    n = tab.shape[0] - 1
    gt_rects = np.ascontiguousarray(gt_rects, dtype=np.float64).reshape(-1, 4)
    gt_classes = np.ascontiguousarray(gt_classes, dtype=np.int32).reshape(-1)
    G = int(gt_rects.shape[0])
    if gt_classes.shape[0] != G:
        raise ValueError("eval_match: %d ground-truth boxes, %d classes" % (G, gt_classes.shape[0]))
    thr = [float(t) for t in iou_thresholds]
    if max_detections is not None and int(max_detections) < 1:
        raise ValueError("eval_match: max_detections = %r (at least 1)" % (max_detections,))
    s = stream_ptr()
    rec = DeviceTensor.from_numpy(tab)
    d_gt = DeviceTensor.from_numpy(gt_rects if G else np.zeros((1, 4)))
    d_gc = DeviceTensor.from_numpy(gt_classes if G else np.zeros(1, np.int32))
    match = DeviceTensor.empty((n + 2, 4), np.int32)
    iou = DeviceTensor.empty((max(n, 1),), np.float64)
    sel = cnt = None
    rows = np.arange(n, dtype=np.int64)
    if max_detections is not None and n:
        M = int(max_detections)
        conf = DeviceTensor.empty((n,), np.float32)
        cnt = DeviceTensor.empty((1,), np.int32)
        sel = DeviceTensor.empty((n,), np.int32)
        kd = DeviceTensor.empty((1,), np.int32)
        wsb = _lib.load().frcnn_topk_select_workspace_bytes(1, n)
        ws = DeviceTensor.empty((max(wsb, 1),), np.uint8)
        _lib.call("frcnn_eval_conf_rows", ptr(rec), 1, n, ptr(conf), ptr(cnt), s)
        _lib.call("frcnn_topk_select", ptr(conf), 1, n, n, ptr(cnt), M, ptr(sel), n, ptr(kd), ptr(ws), wsb, s)
    _lib.call("frcnn_eval_match_batch", ptr(rec), 1, n, ptr(sel) if sel is not None else None, n if sel is not None else 0,
              ptr(kd) if sel is not None else None, ptr(d_gt), ptr(d_gc), (C.c_longlong * 2)(0, G),
              (C.c_double * max(len(thr), 1))(*thr), len(thr), ptr(match), ptr(iou), s)
    out = unpack_match(match.numpy(), iou.numpy())
    if sel is not None:
        rows = sel.numpy()[:out["n"]].astype(np.int64)
    out["rows"] = rows
    return out
