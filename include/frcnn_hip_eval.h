/*
 * frcnn_hip_eval.h -- the part of libfrcnn_hip.so's C ABI that matches a chunk's detections to its ground truth on the device, for
 * mean average precision (Detector:match_batch, evaluate_detections with match = "device"): entry points 150-151 of the library.
 * Included by frcnn_hip.h (include that one); kept apart from it, like frcnn_hip_hard.h, frcnn_hip_loss.h, frcnn_hip_box.h and
 * frcnn_hip_classbox.h, so that the lists of entry points of the five other headers stay the ones their hosts bind today.
 * bindings/frcnn_hip.lua carries a sixth generated cdef for this file, and the host mirror a sixth ctypes table (_lib.EVAL_SIGS);
 * tests/test_eval_match_host.py keeps them in step.
 */
#ifndef FRCNN_HIP_EVAL_H
#define FRCNN_HIP_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Detections against ground truth (not in the reference, whose evaluation is a sketch: main.lua:183-216; csrc/eval_match.hip)
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.
 *
 * frcnn_eval_match_batch matches the winners of a chunk of B frames to the frames' ground-truth boxes at T IoU thresholds at once.
 * INPUTS.  rec: the winner tables exactly as frcnn_detect_gather_batch writes them, double[B][row_stride + 1][16] -- frame b's
 * winner count W_b is int 3 of its 128-byte header (read ON THE DEVICE, clamped to 0 ... row_stride), a record's column 0 its class,
 * column 2 its confidence, columns 8-11 its box r2.  The rows of frame b that are matched are its W_b winners in table order, or --
 * sel_row / k_dev given (both or neither) -- the rows sel_row[b * sel_stride + i], i < min(k_dev[b], W_b, sel_stride), 0-based and
 * ascending as frcnn_topk_select writes them; a row outside 0 ... W_b - 1 is emitted as {0, 0, 0, 0} and nothing is read for it.
 * Ground truth: gt_rect double[.][4] {minX, minY, maxX, maxY} and gt_class int[.]; frame b's boxes are the rows
 * gt_row0_host[b] ... gt_row0_host[b + 1] - 1 (B + 1 HOST values, passed by value to the kernels in groups of 64 frames: no device
 * table, no wait), at most 1024 a frame.  A class < 1 in gt_class is no class: such a box is never matched.  thr_host[T]: the IoU
 * thresholds, host values, passed by value.
 * SEMANTICS, per frame (evaluation.mean_average_precision restated without its sequential dependence):
 *   1. Best box.  Detection d of class c walks the frame's boxes of class c in their given order, from best = -1, gt = none:
 *      v = Rect.IoU(r2_d, g) = i / ((area(r2_d) + area(g)) - i), i the area of the intersection (0 unless maxx >= minx and
 *      maxy >= miny), in fp64, every operation rounded on its own (no contraction), a NaN staying a NaN; the box is taken when
 *      v > best.  The first maximum wins, a NaN (two empty rects) never wins, boxes of other classes are not looked at.
 *   2. Claim.  At threshold t, d is a true positive exactly when it has a box, best_d >= thr[t], and d comes first among the
 *      frame's detections e with gt_e == gt_d and best_e >= thr[t] in the order of decreasing confidence -- compared as fp32 values
 *      by frcnn_topk_select's rank (-0 equals +0, a NaN below everything) --, ties to the earlier row.  Every other detection is a
 *      false positive at t.
 * OUTPUTS.  match int[B][row_stride + 2][4], frame b's table:
 *   row 0       the frame's four counts (matches, candidates, survivors of the class test, winners), copied from rec's header;
 *   row 1       {n = rows emitted, G = the frame's boxes, T, W_b = winners before selection};
 *   rows 2 ...  n rows {class, the confidence's fp32 bits, tp mask (bit t: a true positive at thr[t]), gt (1-based within the
 *               frame; 0: none)}.
 * iou double[B][row_stride] (NULL: not written): best_d of the n rows, -1 without a box.  Nothing is written at or behind row
 * n + 2 of a frame's table, or at or behind row n of its iou; a frame without winners writes its two header rows only.
 * Two launches per 64 frames: one thread a detection for step 1, one wave per (box, frame) for step 2 -- a minimum over
 * (confidence image, row) per threshold: no sort, no atomics, no floating-point accumulation.  Every result is a function of the
 * inputs alone, bit-reproducible run to run.  Counted under FRCNN_KC_NMS.
 * Errors, returned on the host before any launch (a refused call has written nothing): B outside 0 ... 65535, row_stride outside
 * 0 ... 2^27 (no ceiling of the design: both grids stride over the rows; the bound keeps a row's byte offset inside an int), T
 * outside 1 ... 16, NULL thresholds or a NaN among them, a negative sel_stride; then -- B = 0 returns at once -- a
 * NULL rec, match or gt_row0_host, only one of sel_row / k_dev, first rows that are negative or not ascending, more than 1024 boxes
 * in a frame, NULL ground truth with boxes, a pointer that is not aligned (match: 16 bytes; the others: their element). */
int frcnn_eval_match_batch(const double *rec, int B, int row_stride,
                           const int *sel_row, long long sel_stride, const int *k_dev,
                           const double *gt_rect, const int *gt_class, const long long *gt_row0_host,
                           const double *thr_host, int T, int *match, double *iou, void *stream);

/* frcnn_eval_conf_rows writes what frcnn_topk_select needs to apply cfg.scoring's max_detections to the winner tables on the
 * device: conf[b * row_stride + i] = (float) rec[b][1 + i][2] for i < W_b, count[b] = W_b (W_b as above).  frcnn_topk_select on
 * (conf, stride row_stride, n_cap row_stride, n_dev count, K = max_detections) then gives the sel_row / k_dev of
 * frcnn_eval_match_batch: its rank is Detector.keep_best's.  Nothing is written at or behind row W_b of a frame's conf.
 * Errors: B outside 0 ... 65535, row_stride outside 0 ... 2^27; then -- B = 0 returns at once -- a NULL or misaligned pointer.
 * Counted under FRCNN_KC_NMS. */
int frcnn_eval_conf_rows(const double *rec, int B, int row_stride, float *conf, int *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_EVAL_H */
