"""Evaluation loop -- what the reference lists as still to do (README.md:11,13) and only sketches as
`evaluation_demo` (main.lua:183-216: `nextValidation(1)` -> `Detector:detect` -> draw): validation losses and a
PASCAL-VOC style mean average precision over `BatchIterator:nextValidation` (BatchIterator.lua:279-317).

  validation_losses(model, batch_iterator, count)  -> {pcls, preg, dcls, dreg, ...}: the four statistics of
      objective.lua:202-205 on `count` validation images, forward only, networks in evaluate() mode (SpatialDropout x(1-p),
      Dropout identity, BatchNormalization running statistics); the examples of an image are assembled exactly like the
      training ones (BatchIterator.lua:198-225) from a generator of their own, so the training stream is not disturbed.
  mean_average_precision_range(detections, ground_truth, iou_thresholds) -> {mAP, by_iou}: the same at several IoU thresholds
      (0.5 ... 0.95 by default) and their mean; evaluate_detections(..., iou_threshold=<a sequence>) routes to it.
  evaluate_detections(detector, batch_iterator, count) -> {mAP, ap: {class: AP}, ...}: Detector:detect on `count`
      validation images against their ground-truth boxes.  A detection (class c, box r2, confidence) is a true positive when
      its Rect.IoU (Rect.lua:138-141) with a not yet matched ground-truth box of class c in the same image is >= iou_threshold
      (0.5); detections are taken in order of decreasing confidence; AP is the area under the monotone precision envelope
      (VOC2010+) or the 11-point average (use_07_metric=True); mAP averages the classes that have ground truth.
      match="device": the matching itself runs on the device between the two read-backs of a chunk (Detector.match_batch,
      frcnn_eval_match_batch) at all thresholds at once, and average_precision_from_matches(matches, ground_truth, thresholds)
      turns the true-positive masks into the same dict.
  proposal_recall(detector, batch_iterator, count) -> {recall, ground_truth, proposals_per_image}: the share of ground-truth
      boxes that some candidate of the first NMS (Detector.proposals: no classification net) covers with Rect.IoU >=
      iou_threshold -- the figure by which the proposal settings (order, pre_nms_top_n, post_nms_top_n) are chosen.

All arithmetic of the networks runs through the C ABI (frcnn_pnet_forward, frcnn_rpn_loss, frcnn_loss_accumulate,
frcnn_roi_pool_forward or frcnn_roi_align_forward, frcnn_cnet_forward, frcnn_cnet_losses, Detector.detect); the bookkeeping here is host code."""
import ctypes as C

import numpy as np

from . import _lib
from .Anchors import MT19937
from .BatchIterator import assemble_examples
from .Localizer import Localizer
from .Rect import Rect
from .objective import align_geometry, cnet_loss_desc, cnet_loss_settings, roi_pooling_settings, roi_windows
from .synthetic import clean_examples, output_map_sizes
from .tensor import DeviceTensor, ptr, stream_ptr, to_device


def validation_losses(model, batch_iterator, count, seed=1234, negatives=16, debug=None):
    """-> dict(pcls, preg, dcls, dreg, images, examples, positives).  `batch_iterator` needs nextValidation(n) -> [{img, rois}]
    and .anchors (BatchIterator / any object with the same two members).  dcls / dreg are the losses of cfg["cnet_loss"] when the
    model's cfg carries that key (cnet_loss_settings), else the reference's.  debug: a list that receives, per image with
    examples, the host copies of the classification net's rows (crout, ccout, crtarget, cctarget, R, npos)."""
    import torch
    cfg = model["cfg"]
    pnet, cnet, native = model["pnet"], model["cnet"], model["native"]
    bgclass = cfg["class_count"] + 1
    ncls = cfg["class_count"] + 1
    cl = cnet_loss_settings(cfg)     # cfg.cnet_loss (validated before the device is touched); None: the reference's losses
    cl_desc = None if cl is None else cnet_loss_desc(cl, bgclass)
    kh, kw, method, sampling = roi_pooling_settings(cfg)
    planes = model["layers"][-1]["filters"]
    D = kh * kw * planes
    localizer = Localizer(pnet.outnode.children[-1])
    align = method == "align"
    inv_sx, inv_sy = align_geometry(localizer) if align else (0.0, 0.0)
    anchors = batch_iterator.anchors
    rng = MT19937(seed)
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")     # {cls, reg, -, -, creg, ccls, -, -} like the objective
    cls_count = reg_count = creg_count = ccls_count = 0
    was_training = (pnet.train, cnet.train)
    pnet.evaluate(); cnet.evaluate()
    s = stream_ptr()
    keep = []
    try:
        images = 0
        while images < count:
            for x in batch_iterator.nextValidation(1):
                img = to_device(x["img"])
                _, H, W = img.shape
                outputs = pnet.forward(img)
                sizes = [(o.shape[1], o.shape[2]) for o in outputs[:-1]]
                pos, neg = assemble_examples(anchors, cfg, x["rois"], W, H, rng, negatives=negatives)
                pos, neg = clean_examples(pos, sizes), clean_examples(neg, sizes)   # cleanAnchors, objective.lua:74-75
                npos, nneg = len(pos), len(neg)
                E = npos + nneg
                images += 1
                ccls_count += 1        # objective.lua:198: one per image
                if E == 0:
                    continue
                anch = [e[0] for e in pos] + [e[0] for e in neg]
                ex_idx = np.array([(a.layer, a.aspect, a.index[1], a.index[2]) for a in anch], dtype=np.int32)
                ex_anchor = np.array([(a.minX, a.minY, a.maxX, a.maxY) for a in anch], dtype=np.float64)
                ex_roi = np.zeros((max(npos, 1), 4), dtype=np.float64)
                ex_class = np.zeros(max(npos, 1), dtype=np.int32)
                if npos:
                    ex_roi[:npos] = [(e[1].rect.minX, e[1].rect.minY, e[1].rect.maxX, e[1].rect.maxY) for e in pos]
                    ex_class[:npos] = [e[1].class_index for e in pos]
                fm = outputs[-1]
                fmC, fmH, fmW = fm.shape
                pooled = np.concatenate([ex_roi[:npos], ex_anchor[npos:]], 0)
                wins = np.ascontiguousarray(pooled) if align else roi_windows(pooled, localizer, fmH, fmW)   # (RoIAlign: the rects themselves)
                d_idx, d_anchor = DeviceTensor.from_numpy(ex_idx), DeviceTensor.from_numpy(ex_anchor)
                d_roi, d_class, d_wins = DeviceTensor.from_numpy(ex_roi), DeviceTensor.from_numpy(ex_class), DeviceTensor.from_numpy(wins)
                # anchor losses on the sampled anchors (objective.lua:91-140); the gradients it also writes go to scratch maps
                maps = (C.c_void_p * 4)(*[outputs[l].ptr for l in range(4)])
                scratch = [DeviceTensor.zeros(outputs[l].shape) for l in range(4)]
                deltas = (C.c_void_p * 4)(*[t.ptr for t in scratch])
                Hs = (C.c_int * 4)(*[outputs[l].shape[1] for l in range(4)])
                Ws = (C.c_int * 4)(*[outputs[l].shape[2] for l in range(4)])
                ex_loss = DeviceTensor.empty((E, 2), np.float64)
                crtarget = DeviceTensor.empty((E, 4)); cctarget = DeviceTensor.empty((E,))
                _lib.call("frcnn_rpn_loss", maps, deltas, Hs, Ws, ptr(d_idx), ptr(d_anchor), ptr(d_roi), ptr(d_class), npos, nneg,
                          bgclass, ptr(ex_loss), ptr(crtarget), ptr(cctarget), s)
                _lib.call("frcnn_loss_accumulate", ptr(ex_loss), E, C.c_void_p(acc.data_ptr()), s)
                # region classification on the pooled examples (:117-119, :137-139, :146-177), forward only
                cinput = DeviceTensor.empty((E, D)); pidx = None
                if align:
                    _lib.call("frcnn_roi_align_forward", ptr(fm), fmC, fmH, fmW, ptr(d_wins), None, E, inv_sx, inv_sy, kh, kw,
                              sampling, ptr(cinput), s)
                else:
                    pidx = DeviceTensor.empty((E, D), np.int32)
                    _lib.call("frcnn_roi_pool_forward", ptr(fm), fmC, fmH, fmW, ptr(d_wins), E, kh, kw, ptr(cinput), ptr(pidx), s)
                # (a per-class box head, cfg.box_head: the rows of each example's class, as the objective trains them)
                if model["native"].desc.box_per_class:
                    crout, ccout = cnet.forward(cinput, box_classes=("int", d_class, npos))
                else:
                    crout, ccout = cnet.forward(cinput)
                crdelta = DeviceTensor.empty((E, 4)); ccdelta = DeviceTensor.empty((E, ncls))
                row_loss = None
                if cl_desc is None:
                    _lib.call("frcnn_cnet_losses", ptr(crout), ptr(crtarget), ptr(ccout), ptr(cctarget), E, npos, ncls,
                              ptr(crdelta), ptr(ccdelta), C.c_void_p(acc.data_ptr() + 4 * 8), s)
                else:   # cfg.cnet_loss: the loss the objective trains on, row by row, summed in frcnn_loss_accumulate's order
                    row_loss = DeviceTensor.empty((E, 2), np.float64)
                    _lib.call("frcnn_cnet_loss_rows", ptr(crout), ptr(crtarget), ptr(ccout), ptr(cctarget), None, E, npos, ncls,
                              C.byref(cl_desc), ptr(crdelta), ptr(ccdelta), ptr(row_loss), None, None, s)
                    _lib.call("frcnn_loss_accumulate", ptr(row_loss), E, C.c_void_p(acc.data_ptr() + 4 * 8), s)
                if debug is not None:
                    debug.append(dict(crout=crout.numpy(), ccout=ccout.numpy(), crtarget=crtarget.numpy(), cctarget=cctarget.numpy(),
                                      R=E, npos=npos))
                keep.append((d_idx, d_anchor, d_roi, d_class, d_wins, scratch, ex_loss, crtarget, cctarget, cinput, pidx, crdelta, ccdelta,
                             row_loss))
                reg_count += npos; cls_count += E; creg_count += npos      # :194-197
        a = acc.cpu().numpy()
    finally:
        pnet.train, cnet.train = was_training
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(pcls=float(np.float64(a[0]) / cls_count), preg=float(np.float64(a[1]) / reg_count),
                    dcls=float(np.float64(a[5]) / ccls_count), dreg=float(np.float64(a[4]) / creg_count),
                    images=images, examples=cls_count, positives=reg_count)


def voc_ap(recall, precision, use_07_metric=False):
    """Average precision of one class from its recall / precision points (in order of decreasing confidence)."""
    recall = np.asarray(recall, dtype=np.float64); precision = np.asarray(precision, dtype=np.float64)
    if use_07_metric:   # VOC2007: mean over t = 0, 0.1, ..., 1 of the best precision at recall >= t
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = precision[recall >= t].max() if np.any(recall >= t) else 0.0
            ap += p / 11.0
        return float(ap)
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision, [0.0]])
    for i in range(len(mpre) - 2, -1, -1):      # monotone precision envelope
        mpre[i] = max(mpre[i], mpre[i + 1])
    idx = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1]))


def mean_average_precision(detections, ground_truth, iou_threshold=0.5, use_07_metric=False):
    """detections: list of (image_id, class, confidence, Rect); ground_truth: list of (image_id, class, Rect).
    -> dict(mAP, ap={class: AP}, npos={class: #ground truth}, tp, fp)."""
    gt = {}
    for image_id, cls, rect in ground_truth:
        gt.setdefault(cls, {}).setdefault(image_id, []).append(rect)
    ap, npos_of = {}, {}
    tp_total = fp_total = 0
    for cls in sorted(gt):
        npos = sum(len(v) for v in gt[cls].values())
        npos_of[cls] = npos
        dets = [d for d in detections if d[1] == cls]
        dets.sort(key=lambda d: -d[2])            # stable: equal confidences keep their detection order
        used = dict((image_id, [False] * len(v)) for image_id, v in gt[cls].items())
        tp = np.zeros(len(dets)); fp = np.zeros(len(dets))
        for k, (image_id, _, conf, rect) in enumerate(dets):
            best, best_j = -1.0, -1
            for j, g in enumerate(gt[cls].get(image_id, [])):
                iou = Rect.IoU(rect, g)
                if iou > best:
                    best, best_j = iou, j
            if best >= iou_threshold and not used[image_id][best_j]:
                tp[k] = 1; used[image_id][best_j] = True
            else:
                fp[k] = 1                           # low overlap, or a second detection of an already matched box
        ctp, cfp = np.cumsum(tp), np.cumsum(fp)
        recall = ctp / float(npos)
        precision = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
        ap[cls] = voc_ap(recall, precision, use_07_metric) if len(dets) else 0.0
        tp_total += int(tp.sum()); fp_total += int(fp.sum())
    return dict(mAP=float(np.mean(list(ap.values()))) if ap else float("nan"), ap=ap, npos=npos_of, tp=tp_total, fp=fp_total)


IOU_RANGE = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))     # 0.5, 0.55, ... 0.95


def mean_average_precision_range(detections, ground_truth, iou_thresholds=IOU_RANGE, use_07_metric=False):
    """mean_average_precision at several IoU thresholds (default 0.5, 0.55, ... 0.95: the average that rewards localisation, where
    a setting such as cfg["box_voting"] shows; at 0.5 alone it barely does).
    -> dict(mAP = the mean of the thresholds' mAP, by_iou = {t: the dict mean_average_precision returns at t})."""
    ts = [float(t) for t in iou_thresholds]
    if not ts:
        raise ValueError("mean_average_precision_range: no IoU threshold")
    by_iou = dict((t, mean_average_precision(detections, ground_truth, t, use_07_metric)) for t in ts)
    return dict(mAP=float(np.mean([by_iou[t]["mAP"] for t in ts])), by_iou=by_iou)


def average_precision_from_matches(matches, ground_truth, iou_thresholds=0.5, use_07_metric=False):
    """mean_average_precision / mean_average_precision_range from what Detector.match_batch returns: matches[f] the dict of frame
    f (cls, confidence, tp: bit t = a true positive at threshold t), ground_truth[f] its boxes ((class_index, Rect) pairs or
    objects with .class_index and .rect), iou_thresholds the thresholds match_batch was called with -- a number (one threshold,
    bit 0) -> the dict of mean_average_precision; a sequence -> the dict of mean_average_precision_range, threshold t from bit t.
    The matching is done: what is left is, per class, the stable sort by decreasing confidence across the frames in their order,
    the cumulative sums and voc_ap, on arrays.  Equal key by key to the host functions on the same detections."""
    single = not isinstance(iou_thresholds, (tuple, list, np.ndarray))
    ts = [float(iou_thresholds)] if single else [float(t) for t in iou_thresholds]
    if not ts:
        raise ValueError("average_precision_from_matches: no IoU threshold")
    if len(matches) != len(ground_truth):
        raise ValueError("average_precision_from_matches: %d frames, ground truth for %d" % (len(matches), len(ground_truth)))
    npos_of = {}
    for boxes in ground_truth:
        for g in boxes:
            c = int(g.class_index if hasattr(g, "rect") else g[0])
            npos_of[c] = npos_of.get(c, 0) + 1
    cls = np.concatenate([np.asarray(m["cls"], np.int64) for m in matches] + [np.zeros(0, np.int64)])
    conf = np.concatenate([np.asarray(m["confidence"], np.float32) for m in matches] + [np.zeros(0, np.float32)]).astype(np.float64)
    mask = np.concatenate([np.asarray(m["tp"], np.uint32) for m in matches] + [np.zeros(0, np.uint32)])
    per_class = {}
    for c in sorted(npos_of):
        rows = np.nonzero(cls == c)[0]
        per_class[c] = mask[rows[np.argsort(-conf[rows], kind="stable")]]     # equal confidences keep their detection order
    by_iou = {}
    for bit, t in enumerate(ts):
        ap = {}
        tp_total = fp_total = 0
        for c in sorted(npos_of):
            tp = ((per_class[c] >> np.uint32(bit)) & np.uint32(1)).astype(np.float64)
            fp = 1.0 - tp
            ctp, cfp = np.cumsum(tp), np.cumsum(fp)
            recall = ctp / float(npos_of[c])
            precision = ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
            ap[c] = voc_ap(recall, precision, use_07_metric) if len(tp) else 0.0
            tp_total += int(tp.sum()); fp_total += int(fp.sum())
        by_iou[t] = dict(mAP=float(np.mean(list(ap.values()))) if ap else float("nan"), ap=ap, npos=dict(npos_of), tp=tp_total,
                         fp=fp_total)
    if single:
        return by_iou[ts[0]]
    return dict(mAP=float(np.mean([by_iou[t]["mAP"] for t in ts])), by_iou=by_iou)


def _evaluate_on_device(detector, batch_iterator, count, iou_threshold, use_07_metric, batch, mixed_sizes):
    """evaluate_detections(match="device"): the same chunks through Detector.match_batch, then average_precision_from_matches."""
    single = not isinstance(iou_threshold, (tuple, list, np.ndarray))
    thr = [float(iou_threshold)] if single else [float(t) for t in iou_threshold]
    if not thr:
        raise ValueError("mean_average_precision_range: no IoU threshold")
    matches, ground_truth = [], []
    pending = []     # frames -- of one size unless mixed_sizes -- waiting for match_batch; their boxes are the tail of ground_truth
    images = 0

    def flush():
        matches.extend(detector.match_batch(pending, ground_truth[len(matches):], thr, mixed_sizes=bool(mixed_sizes) and batch > 1))
        del pending[:]
    while images < count:
        for x in batch_iterator.nextValidation(1):
            images += 1
            if batch > 1 and not mixed_sizes and pending and tuple(pending[0].shape) != tuple(x["img"].shape):
                flush()
            ground_truth.append([(int(roi.class_index), roi.rect) for roi in x["rois"]])
            pending.append(x["img"])
            if len(pending) >= max(batch, 1):
                flush()
    if pending:
        flush()
    res = average_precision_from_matches(matches, ground_truth, thr[0] if single else thr, use_07_metric)
    res.update(images=images, detections=sum(len(m["cls"]) for m in matches), ground_truth=sum(len(g) for g in ground_truth))
    return res


def evaluate_detections(detector, batch_iterator, count, iou_threshold=0.5, use_07_metric=False, batch=1, mixed_sizes=False,
                        match="host"):
    """Detector:detect on `count` validation images (main.lua:198-206) scored against their ground truth.
    match = "host" (default): the detections are read back and matched here (mean_average_precision).  "device": every chunk goes
    through Detector.match_batch -- the matching runs on the device at all thresholds at once, 16 bytes a detection come back
    instead of a 128-byte record, and average_precision_from_matches does the rest; batch=1 is a chunk of one frame.  The same
    dict either way; anything else is a ValueError before the device is touched.
    iou_threshold: a number, or a sequence of them -> the dict of mean_average_precision_range (mAP, by_iou).
    batch > 1: up to that many consecutive frames of one size go through Detector.detect_batch in one call (same detections,
    two host waits per chunk instead of two per frame); 1 is the frame-by-frame loop of the reference.
    mixed_sizes=True (with batch > 1): a change of size no longer ends a chunk -- `batch` consecutive frames, whatever their
    sizes, go through detect_batch(..., mixed_sizes=True) (a data set whose every file has a size of its own).
    The precision/recall curves are only as long as the detector's list: mAP is meant to be computed under a detector with
    cfg["scoring"] = {classes = "all", min_confidence = a low value such as 0.05} (Detector.scoring_settings), which scores a
    region under every class over the threshold; the reference's class test (arg-max only, p > 0.2) cuts the low-confidence
    tail off every curve.  A model with a per-class box head (cfg["box_head"]) is evaluated that way with boxes = "class" in the
    same table (Detector.scoring_boxes): every (region, class) row is then scored with the box of its own class."""
    if match not in ("host", "device"):
        raise ValueError("evaluate_detections: match = %r (\"host\" or \"device\")" % (match,))
    if match == "device":
        return _evaluate_on_device(detector, batch_iterator, count, iou_threshold, use_07_metric, batch, mixed_sizes)
    detections, ground_truth = [], []
    images = 0
    pending = []     # (image id, frame) -- of one size unless mixed_sizes -- waiting for detect_batch

    def flush():
        imgs = [img for _, img in pending]
        results = detector.detect_batch(imgs, mixed_sizes=True) if mixed_sizes else detector.detect_batch(imgs)
        for (image_id, _), winners in zip(pending, results):
            for w in winners:
                detections.append((image_id, int(w["class"]), float(w["confidence"]), w["r2"]))
        del pending[:]
    while images < count:
        for x in batch_iterator.nextValidation(1):
            image_id = images
            images += 1
            for roi in x["rois"]:
                ground_truth.append((image_id, int(roi.class_index), roi.rect))
            if batch > 1:
                if not mixed_sizes and pending and tuple(pending[0][1].shape) != tuple(x["img"].shape):
                    flush()
                pending.append((image_id, x["img"]))
                if len(pending) >= batch:
                    flush()
                continue
            for w in detector.detect(x["img"]):
                detections.append((image_id, int(w["class"]), float(w["confidence"]), w["r2"]))
    if pending:
        flush()
    if isinstance(iou_threshold, (tuple, list, np.ndarray)):
        res = mean_average_precision_range(detections, ground_truth, iou_threshold, use_07_metric)
    else:
        res = mean_average_precision(detections, ground_truth, iou_threshold, use_07_metric)
    res.update(images=images, detections=len(detections), ground_truth=len(ground_truth))
    return res


def proposal_recall(detector, batch_iterator, count, iou_threshold=0.5):
    """Detector.proposals on `count` validation images against their ground truth, classes ignored: a ground-truth box counts
    as recalled when the rect `r` of some proposal of its image has Rect.IoU (Rect.lua:138-141) >= iou_threshold with it.
    -> dict(recall (nan without ground truth), ground_truth, proposals_per_image).  Host bookkeeping: `detector` is any object
    with proposals(img) -> [{r: Rect, ...}], `batch_iterator` any with nextValidation(n) -> [{img, rois}]."""
    images = hit = total = proposals = 0
    while images < count:
        for x in batch_iterator.nextValidation(1):
            images += 1
            props = detector.proposals(x["img"])
            proposals += len(props)
            for roi in x["rois"]:
                total += 1
                if any(Rect.IoU(p["r"], roi.rect) >= iou_threshold for p in props):
                    hit += 1
    return dict(recall=hit / float(total) if total else float("nan"), ground_truth=total,
                proposals_per_image=proposals / float(images) if images else 0.0)
