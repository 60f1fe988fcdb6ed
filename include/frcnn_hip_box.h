/*
 * frcnn_hip_box.h -- the part of libfrcnn_hip.so's C ABI that serves the per-class box head of the classification net
 * (cfg.box_head): entry points 145-147 of the library.  Included by frcnn_hip.h (include that one); kept apart from it, like
 * frcnn_hip_hard.h and frcnn_hip_loss.h, so that the lists of entry points of the three other headers stay the ones their hosts
 * bind today.  bindings/frcnn_hip.lua carries a fourth generated cdef for this file, and the host mirror a fourth ctypes table
 * (_lib.BOX_SIGS); tests/test_box_head_host.py keeps them in step.
 */
#ifndef FRCNN_HIP_BOX_H
#define FRCNN_HIP_BOX_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Per-class box regression (not in the reference, whose box head is one Linear(nf, 4): model_utilities.lua:117-124;
 * csrc/box_head.hip) ---------------------------------------------------------------------------------------------------------
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.
 *
 * LAYOUT.  With frcnn_model_desc.box_per_class set the box head is a Linear(nf, 4 C), C = class_count: weight float[4 C][nf], bias
 * float[4 C].  Row 4 (c - 1) + j is coordinate j of foreground class c (classes are 1-based; the background, class_count + 1, has
 * no rows).  The block sits where the shared head's [4][nf] + [4] sit in the flat vector; everything behind it moves by
 * 4 (C - 1) (nf + 1).  frcnn_model_param_table reports the two tensors with kinds 3 and 4.  With class_count = 1 the layout IS
 * the shared one.  With the field zero the model, its launches and its results are the shared head's.
 *
 * A row of the batch uses the four rows of ONE class.  THE CLASS SOURCE (`kind`):
 *   1  int32 classes[r] for the first n rows, every row behind them background (the example table of
 *      frcnn_pnet_anchor_loss_begin);
 *   2  an fp32 1-based class per row (the cctarget of frcnn_proposal_targets_batch / frcnn_roi_hard_gather_batch): the class is
 *      (int) classes[r] where 1 <= classes[r] <= C as floats; a NaN, like every other value, is outside;
 *   0  none: the first maximum of the row's own log-probabilities lsm[r][0 .. ncls), by frcnn_cnet_decode's comparison (`best`
 *      starts at column 0 and moves only on a strict >: a NaN in column 0 stays, a NaN elsewhere is never taken, ties keep the
 *      lowest column); the class is that column + 1.
 * A class outside 1 ... C -- the background, or garbage -- is no class: the row's four outputs are 0, sel[r] = 0, and nothing is
 * read for it out of range.
 *
 * frcnn_box_head_forward:  out[r][j] = b[4 (c-1) + j] + sum_k x[r][k] W[4 (c-1) + j][k], c the row's class; sel[r] = c.
 *   x float[R][nf], W float[4 C][nf], b float[4 C], out float[R][4], sel int[R]; lsm / ncls only for kind 0, classes / n only
 *   for kinds 1 and 2 (n only for kind 1).
 * frcnn_box_head_backward, on the sel the forward call wrote (a value outside 1 ... C counts as 0):
 *   gfeat[r][k]       = ((g[r][0] W[4 (s-1)][k] + g[r][1] W[4 (s-1) + 1][k]) + g[r][2] W[..+2][k]) + g[r][3] W[..+3][k], s = sel[r],
 *                       STORED; a row with sel[r] = 0 stores zeros whatever g holds.  gfeat NULL: not computed.
 *   gW[4 (c-1) + j][k] += sum_{r: sel[r] = c} g[r][j] x[r][k];  gb[4 (c-1) + j] += sum_{r: sel[r] = c} g[r][j]: ADDED to what the
 *                       arrays hold.  The rows of a class are summed in ascending order within each run of 64 rows that one
 *                       wave owns (rows 64 w + 1024 i ..., wave w of 16), and the 16 partial sums are folded in wave order.  The
 *                       rows of a class without a row in the batch are NOT WRITTEN at all.  gW and gb NULL (both): not computed.
 * fp32 multiply-adds; the forward sum runs over the features in 64 interleaved partial sums folded by a butterfly.  No atomics, no
 * workspace: every result is bit-reproducible run to run, with option "deterministic" on or off.  Any nf >= 1: rows move 16 bytes
 * at a time where nf % 4 == 0 and the arrays involved are 16-byte aligned, one float at a time otherwise.  Nothing is written
 * behind row R of an output.
 * Errors, returned before any launch (a refused call has written nothing; R <= 0 returns at once, after the checks of the
 * scalar arguments): nf < 1, C < 1, kind outside 0 ... 2, 4 C nf >= 2^31, a NULL array that the call needs, n outside 0 ... R
 * (kind 1), only one of gW / gb, no output at all, a pointer that is not 4-byte aligned.  Counted under FRCNN_KC_ELEMWISE. */
int frcnn_box_head_forward(const float *x, int R, int nf, const float *W, const float *b, int C,
                           const void *classes, int kind, int n, const float *lsm, int ncls,
                           float *out, int *sel, void *stream);
int frcnn_box_head_backward(const float *g, const float *x, const int *sel, int R, int nf,
                            const float *W, int C, float *gfeat, float *gW, float *gb, void *stream);

/* The class source of the NEXT frcnn_cnet_forward of a model with box_per_class (and of that call only: the call after it has no
 * source again unless this is called again).  kind as above; `classes` must stay valid and unchanged until that forward pass has
 * run on its stream.  Without a call -- Detector's case -- the box of the predicted class is computed (kind 0 on the pass's own
 * log-probabilities).  frcnn_cnet_backward uses the classes the forward pass used.  Errors: a model without box_per_class, kind
 * outside 0 ... 2, kind 1 or 2 without classes, n < 0 (kind 1; n above the pass's row count is refused by that pass). */
int frcnn_cnet_box_classes(frcnn_model *, const void *classes, int kind, int n);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_BOX_H */
