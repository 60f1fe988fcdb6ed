"""nms(boxes, overlap, scores) -- host-side mirror of nms.lua:23-102 over frcnn_nms_host /
frcnn_nms_device.  Key dispatch is the reference's (nms.lua:37-43): a number selects that column
(1-based), the string 'area' selects the area, ANYTHING ELSE -- including a score tensor or None,
which is what both call sites of the reference pass (Detector.lua:82,133) -- sorts by max-y.
Returns the 1-based row ids of the survivors in pick order (a LongTensor in the reference).

soft_nms(boxes, overlap, score_col, ...) -- not in the reference: Soft-NMS (Bodla et al. 2017) over frcnn_soft_nms_batch, the
greedy loop that lowers the neighbours' scores instead of deleting them (semantics: include/frcnn_hip.h)."""
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
