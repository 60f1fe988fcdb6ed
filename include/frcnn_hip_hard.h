/*
 * frcnn_hip_hard.h -- the part of libfrcnn_hip.so's C ABI that serves online hard example mining: entry points 142 and 143 of
 * the library.  Included by frcnn_hip.h (include that one); kept apart from it so that frcnn_hip.h's own list of entry points
 * stays the one its hosts bind today.  bindings/frcnn_hip.lua carries a second generated ffi.cdef for this file, and the host
 * mirror a second ctypes table (_lib.HARD_SIGS); tests/test_roi_hard_host.py keeps the three in step.
 */
#ifndef FRCNN_HIP_HARD_H
#define FRCNN_HIP_HARD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Online hard example mining for the classification net (Shrivastava, Gupta, Girshick 2016; not in the reference;
 * csrc/roi_hard.hip) -----------------------------------------------------------------------------------------------------------
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.  The entry points named below without a declaration are declared there.
 * Under cfg.roi_sampling = { source = "hard", ... } the rows the classification net is trained on are not drawn: EVERY labelled
 * candidate leaves frcnn_proposal_targets_batch (batch = out_stride = fg_quota = r_cap + 64: the "all" table, foreground rows
 * first), is pooled and scored by the net in evaluate mode, and the rows of largest loss are kept after an NMS among them:
 *     frcnn_roi_hard_keys_batch -> frcnn_nms_device_batch(box5, key_mode 2, key_col 5, overlap = hard_nms_overlap)
 *                               -> frcnn_roi_hard_gather_batch
 * The NMS in between is the library's own ON PURPOSE, and its arithmetic is part of the setting's definition: its fp32 IoU with
 * the + 1 areas (area = (x2-x1+1)*(y2-y1+1), nms.lua:23-102; unlike Rect.IoU of the proposal-target layer), on the rects ROUNDED
 * to fp32, "suppressed" meaning !(iou <= overlap), and its tie rule -- equal keys: the HIGHER row is picked first.  Picks come
 * in descending loss order.
 * Segments as in frcnn_proposal_targets_batch: B of them, one frame each, strides in rows, counts on the device.  Segment b has
 * n = min(max(n_dev[b], 0), n_cap) rows at row offset b*row_stride, n_cap <= 4096, the first nfg = min(max(nfg_dev[b], 0), n) of
 * them foreground (the layout of the "all" table).
 *
 * frcnn_roi_hard_keys_batch: the per-row loss and the NMS's rows.  Reads roi (double[4]), crout (float[4], the net's regression
 * output), crtarget (float[4]), ccout (float[ncls], log-probabilities), cctarget (float, the 1-based class); inputs are only
 * read.  fp32, every operation rounded on its own (no fused multiply-add), in this order -- the per-row terms of
 * frcnn_cnet_losses with the reference's factor 10 (objective.lua:170-177):
 *     t = (int) cctarget[r];  cls = -ccout[r][t-1]
 *     a foreground row (r < nfg), k = 0..3: z = crout[r][k] - crtarget[r][k]; a = |z|; term_k = a < 1 ? (0.5f*z)*z : a - 0.5f
 *                                           reg = ((term_0 + term_1) + term_2) + term_3; reg = reg * 10.0f
 *     a background row: reg = 0, and crout is not read for it
 *     loss = cls + reg;  a loss that is not a number is stored as +inf (a diverged row is the hardest one, and the order the
 *     NMS sorts by stays total);  a target that is not in [1, ncls] (a NaN included) gives -inf: it is never picked ahead of a
 *     valid row, and nothing is read out of bounds for it
 * Writes box5[r] = { (float) roi[r][0..3], loss } (float[5], the NMS's ncols = 5) and loss[r] for r < n; nothing behind row n.
 * One thread a row, 16-byte loads, coalesced stores through LDS; at <= 4096 rows of ~100 bytes the launch itself is the cost.
 *
 * frcnn_roi_hard_gather_batch: the selection behind the NMS.  pick + b*row_stride (device int64, 1-based rows within the
 * segment, in pick order) and count_dev[b] as frcnn_nms_device_batch leaves them; count = min(max(count_dev[b], 0), n_cap).
 *   RULE     walk the first `count` picks in order; a pick outside [1, n] is skipped and does not count; the first `batch` of
 *            the others are SELECTED (picks are distinct as the NMS leaves them; were one repeated, it counts each time and
 *            selects its row once).
 *   OUTPUTS  the selected rows leave in ASCENDING ROW ORDER -- the F foreground rows first, then the Bq background rows, each
 *            in candidate order (the rule of frcnn_topk_select for its selection), NOT in pick order -- at rows
 *            b*out_stride + [0, F + Bq): roi_out, crtarget_out, cctarget_out, src_out, gt_idx_out, iou_out, loss_out are bit
 *            copies of that row of roi, crtarget, cctarget, src, gt_idx, iou (the "all" table) and loss.  Nothing is stored
 *            behind row F + Bq.  counts[b][4] = {F, Bq, count, n}, stored as one 16-byte word.  A segment with n = 0 writes
 *            its counts {0, 0, count, 0} and nothing else.
 * One workgroup a segment, a byte flag per row in LDS, the ordered compaction of frcnn_proposal_targets_batch.  Neither kernel
 * uses atomics or a workspace: a segment's output is a function of its own data.  The outputs may not alias the inputs.
 * Errors of both, returned before any launch (B = 0 returns at once; a refused call has written nothing): B outside 0 ... 65535,
 * n_cap outside 0 ... 4096, row_stride < n_cap, a NULL required pointer (the counts always; the tables with n_cap > 0), ncls < 1
 * (keys), batch < 1 or out_stride < min(batch, n_cap) (gather), a pointer that is moved 16 bytes at a time -- roi, crout, crtarget,
 * roi_out, crtarget_out, counts -- and is not 16-byte aligned.  Counted under FRCNN_KC_RPN. */
int frcnn_roi_hard_keys_batch(const double *roi, const float *crout, const float *crtarget, const float *ccout,
                              const float *cctarget, int B, long long row_stride, int n_cap, const int *n_dev, const int *nfg_dev,
                              int ncls, float *box5, float *loss, void *stream);
int frcnn_roi_hard_gather_batch(const long long *pick, const int *count_dev, int batch, const double *roi, const float *crtarget,
                                const float *cctarget, const int *src, const int *gt_idx, const double *iou, const float *loss,
                                int B, long long row_stride, int n_cap, const int *n_dev, const int *nfg_dev, double *roi_out,
                                float *crtarget_out, float *cctarget_out, int *src_out, int *gt_idx_out, double *iou_out,
                                float *loss_out, int out_stride, int *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_HARD_H */
