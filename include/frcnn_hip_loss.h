/*
 * frcnn_hip_loss.h -- the part of libfrcnn_hip.so's C ABI that serves the configurable losses of the classification net
 * (cfg.cnet_loss): entry point 144 of the library.  Included by frcnn_hip.h (include that one); kept apart from it, like
 * frcnn_hip_hard.h, so that the lists of entry points of the two other headers stay the ones their hosts bind today.
 * bindings/frcnn_hip.lua carries a third generated ffi.cdef for this file, and the host mirror a third ctypes table
 * (_lib.LOSS_SIGS); tests/test_cnet_loss_host.py keeps the three in step.
 */
#ifndef FRCNN_HIP_LOSS_H
#define FRCNN_HIP_LOSS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The losses of the classification net, row by row (not in the reference beyond its defaults; csrc/cnet_loss.hip) ---------
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.
 * frcnn_cnet_losses is objective.lua:170-177 and nothing else: SmoothL1 * 10 on the box deltas, ClassNLL averaged over the rows,
 * one workgroup.  frcnn_cnet_loss_rows computes the same two losses -- or a focal loss (Lin et al. 2017), a label-smoothed NLL, a
 * GIoU box loss (Rezatofighi et al. 2019) -- in tiles of 64 rows, one workgroup a tile, and leaves the SUMS to
 * frcnn_loss_accumulate: a row's outputs are a function of that row alone.  No atomics, no workspace.
 *
 * The description (read on the host before the launch): */
typedef struct {
  int cls;              /* 0 nll, 1 focal */
  int box;              /* 0 smooth_l1, 1 giou */
  int bgclass;          /* 1-based background class, for alpha */
  double gamma, alpha /* < 0: none */, smoothing, beta, box_weight;
} frcnn_cnet_loss_desc;
/* Ranges: cls, box in {0, 1}; gamma in [0, 5]; alpha < 0 (none) or in (0, 1); smoothing in [0, 1), and 0 under focal; beta finite
 * and > 0; box_weight finite and >= 0; bgclass in [1, ncls] when alpha is given.
 *
 * Inputs: crout float[R][4] (the net's box deltas), crtarget float[R][4], ccout float[R][ncls] (log-probabilities), cctarget
 * float[R] (1-based class), roi double[R][4] (only for box5).  The first npos rows are foreground.
 * MODES  training: crdelta float[R][4] and ccdelta float[R][ncls] are both given; rows r >= npos of crout are set to 0, as
 *        frcnn_cnet_losses does.  scoring: both are NULL; crout is only read (a row r >= npos counts as 0 all the same) and no
 *        gradient is written.
 * OUTPUTS, each optional, at least one of the gradients, row_loss, key, box5 given:
 *   row_loss[r] = { box_weight * box_r, cls_r / R } (double[R][2], the order of frcnn_cnet_losses' loss2); the step's sums are
 *                 frcnn_loss_accumulate(row_loss, R, acc + 4), whose order and bound are stated at its declaration
 *   key[r]      = (float)(cls_r + box_weight * box_r)
 *   box5[r]     = { (float) roi[r][0..3], key[r] } (float[R][5], the layout frcnn_roi_hard_keys_batch writes); requires roi
 *   key and box5 follow that kernel's two rules: a key that is not a number is stored as +inf; a target outside [1, ncls] (a NaN
 *   included) gives -inf, and nothing is read out of bounds for it.  In training mode such a row has cls_r = NaN and an all-zero
 *   ccdelta row; its box terms are the ones of any row.
 * Nothing is written behind row R.
 *
 * ARITHMETIC, per row in fp64 (IEEE operations in the order written, no fused multiply-add), every stored float one rounding
 * of the fp64 value.  t = (int) cctarget[r]; w = 1 without alpha, else alpha for t != bgclass and 1 - alpha for t == bgclass.
 *   nll (also focal with gamma == 0), smoothing == 0:
 *       cls_r = -(w * ccout[r][t-1]);  ccdelta[r][j] = 0 but (float)(-w / R) at the target
 *   nll, smoothing = e > 0:  u = e / ncls; q_j = u, and u + (1 - e) at the target
 *       cls_r = -(w * sum_j q_j * ccout[r][j]), summed in ascending j from 0;  ccdelta[r][j] = (float)(-(w * q_j) / R)
 *   focal, gamma = g > 0:  lp = ccout[r][t-1]; q = -expm1(lp), and 0 unless that is > 0
 *       cls_r = -((w * pow(q, g)) * lp)
 *       ccdelta at the target = (float)((w * (-pow(q, g) + x)) / R), x = ((g * pow(q, g-1)) * (1 - q)) * lp where q > 0 and
 *       lp > -inf, else 0 (lp = -inf: p log p -> 0, where the product itself would be 0 * inf); the rest of the row is 0
 *   smooth_l1, beta = b:  z_k = v_k - crtarget[r][k] in fp32, v = crout[r] for r < npos and 0 behind (with the zero targets the
 *       target layers write for background rows, those rows give 0), a = |z_k|
 *       term_k = a < b ? ((0.5 * z) * z) / b : a - 0.5 * b;  box_r = ((term_0 + term_1) + term_2) + term_3
 *       crdelta[r][k] = (float)(box_weight * (a < b ? z / b : (z > 0 ? 1 : -1)))
 *       With b = 1 and box_weight = 10 crdelta, ccdelta and the zeroed crout are frcnn_cnet_losses' bit for bit: the fp32
 *       rounding of the exact product z * 10 is what z * 10.0f is.
 *   giou (foreground rows; a background row has box_r = 0 and a zero crdelta row):  the deltas encode corners and log-sizes
 *       ((gx0 - ax0) / aw, ..., log(gw / aw), ...: frcnn_proposal_targets_batch), and GIoU is invariant under a scaling of
 *       each axis, so it is taken in the delta space.  K = log(1000 / 16).
 *       prediction: x0 = crout0, y0 = crout1, x1 = x0 + exp(min(crout2, K)), y1 = y0 + exp(min(crout3, K))
 *       target: the same from crtarget, without the clamp.  Areas are taken from the corners: (x1 - x0) * (y1 - y0).
 *       iw = min(x1, tx1) - max(x0, tx0), ih likewise;  I = iw * ih for iw > 0 and ih > 0, else 0;  U = (Ap + At) - I;
 *       C = the area of the enclosing box;  box_r = (2 - I / U) - U / C
 *       In every min / max a tie selects the prediction's edge.  With the edge gradients gI, gA, gC (through the selected
 *       edges) and gU = gA - gI:  g_edge = ((-(gI * (1/U)) + gU * ((I/U)/U)) - gU * (1/C)) + gC * ((U/C)/C);
 *       d/dcrout0 = g_x0 + g_x1, d/dcrout2 = g_x1 * exp(crout2) for crout2 <= K and 0 above it; crdelta = (float)(box_weight * d).
 *       A prediction equal to its target has box_r = 0 and an exactly zero gradient.
 *
 * One workgroup owns 64 rows: one thread a row computes the terms, then the whole workgroup writes the tile's ccdelta rows with
 * 16-byte stores (a tile starts at a multiple of 64 * ncls floats), scalar stores at the tail when R * ncls is no multiple of 4.
 * Errors, returned before any launch (a refused call has written nothing; R == 0 returns at once): R < 0, npos outside 0 ... R,
 * ncls < 1, a NULL input (crout, crtarget, ccout, cctarget, desc_host), only one of crdelta / ccdelta, box5 without roi, no
 * output at all, crout, crtarget, crdelta, ccdelta or roi not 16-byte aligned, a description outside the ranges above.
 * Counted under FRCNN_KC_ELEMWISE. */
int frcnn_cnet_loss_rows(float *crout, const float *crtarget, const float *ccout,
                         const float *cctarget, const double *roi,
                         int R, int npos, int ncls,
                         const frcnn_cnet_loss_desc *desc_host,
                         float *crdelta, float *ccdelta,
                         double *row_loss, float *key, float *box5, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_LOSS_H */
