/*
 * frcnn_hip.h -- C ABI of libfrcnn_hip.so: the MI355X (gfx950) Faster R-CNN detection/training
 * hot path of andreaskoepf/faster-rcnn.torch.
 *
 * The reference has no FFI of its own: its hot path reaches its arithmetic through the Torch7
 * Lua object protocol (nn.Module:forward/backward, nn.SpatialAdaptiveMaxPooling, criteria,
 * nms(), optim.rmsprop) implemented by the un-vendored cunn/cutorch packages.  This header is
 * the boundary a LuaJIT `ffi.cdef` -- or any other host -- binds in their
 * place.  Each entry point names the reference call site it replaces (file:line in the
 * reference tree).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types, no exceptions.
 *  - Every function returns FRCNN_OK (0) or an FRCNN_ERR_* code; frcnn_last_error() returns a
 *    thread-local message that a Lua wrapper turns into error().
 *  - Pointers are DEVICE pointers unless the parameter name ends in _host.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All work is
 *    asynchronous on that stream unless a function says it synchronises.
 *  - Tensors are fp32, CHW (or row-major R x D), contiguous, exactly like the reference's
 *    CudaTensors.  Index values exchanged through this ABI are 1-based like the Lua surface
 *    wherever the reference's own tables are 1-based (anchor indices, NMS ids, ROI windows,
 *    class ids); this is stated per function.
 */
#ifndef FRCNN_HIP_H
#define FRCNN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_OK 0
#define FRCNN_ERR_ARG 1
#define FRCNN_ERR_HIP 2
#define FRCNN_ERR_STATE 3

/* ---- library / device --------------------------------------------------------------- */
int frcnn_version(void);
const char *frcnn_last_error(void);
int frcnn_device_count(int *n);
int frcnn_set_device(int device);            /* cutorch.setDevice, main.lua:52 (0-based here) */
int frcnn_device_name(char *buf_host, int len);
/* Library options.  "side_stream" (default 1; environment FRCNN_SIDE_STREAM): independent parts of a
 * pass (anchor nets, weight gradients) are issued on a library-owned second HIP stream and joined before the
 * entry point's results are used on the caller's stream.  0 = strictly serial on the caller's stream.
 * "deterministic" (default 0): the places where floating-point partial results meet in fp32 atomics (bias / slope
 * gradient partials of the activation backward passes, the scatter-adds of the ROI-pooling and sparse anchor-net backward
 * passes, the anchor deltas of two examples naming one anchor) switch to order-independent forms -- partials folded in
 * index order, gathers, 64-bit fixed-point accumulation -- so that two runs on the same inputs are bit-identical.
 * "split_bf16" (default 1; environment FRCNN_SPLIT_BF16): the 3x3 convolutions whose shapes fit (forward and input gradient:
 * input channels a multiple of 16, filters a multiple of 64; weight gradient: both multiples of 64) run in the split-operand
 * form: fp32 tensors in and out, fp32 accumulation, every fp32 product formed from six exact bf16 x bf16 partial products of
 * three-way split operands on the bf16 matrix cores (24 significand bits per operand; against an fp64 reference the error
 * equals that of the fp32 matrix-core kernels, tests/test_gpu_convx.py).  0 = fp32 matrix-core kernels only.  Applies to the
 * operator-level entry points at once and to a model from its next (re)shaping on.
 * "gemm_x_roles" (default -1; environment FRCNN_GEMM_X): which products of a large nn.Linear (the cnet's Linear(13824, 1024))
 * take the split-bf16 operand form of csrc/gemmx.hip -- bit 1 forward, 2 input gradient, 4 weight gradient; -1 = the
 * measured rule (the input gradient always; forward and weight gradient from 192 rows on, where they beat the fp32 kernels),
 * 0 = fp32 matrix-core kernels for all three.
 * "x3_f16" (default 1; environment FRCNN_X3_F16): the operand form of the split convolutions (with "split_bf16" on).  1 = two
 * fp16 planes per operand and THREE exact partial products per fp32 product: each tensor is scaled by a power of two taken from
 * its largest magnitude (recorded by the launch that wrote it), h = f16(x 2^e), l = f16(x 2^e - h), 22 significand bits per
 * operand; measured against fp64 the error is that of the fp32 matrix-core kernels (tools/x3_f16_check.py,
 * tests/test_gpu_convx.py run both forms).  0 = three bf16 planes and six partial products: the split is exact (24 bits, no
 * dependence on the tensor's range) at twice the matrix-pipe time.  Takes effect with the next forward pass.
 * "static_weights" (default 0): the host promises that it does not write the weight vector between evaluate-mode forward passes
 * (Detector:detect on a trained model); the library then re-uses the packed / split copies of the convolution weights instead of
 * remaking them per pass.  A training-mode pass, a change of the frame size and every frcnn_set_option("static_weights", v) call
 * drop the copies -- a host that has written the weights itself says so by setting the option again.
 * "drop_compact" (default 1; environment FRCNN_DROP_COMPACT): a training pass leaves out the channels an nn.SpatialDropout
 * (models/model_utilities.lua:10-12) drops.  In a block of two or more convolutions the dropout follows the first one, so for the
 * length of a step the dropped filters of the first convolution and the dropped input channels of the second multiply zeros --
 * forward (objective.lua:71) and backward (:189).  With the keep vector known on the host (drawn with the hash the device kernel
 * uses; an explicit mask is read back -- a synchronous copy, parity runs) the step computes the first convolution for the kept
 * filters only, stores its output and that output's gradient compact, and runs the second convolution, both input gradients and
 * both weight gradients on the kept channels (padded to the kernels' 16 / 64-channel granularity); packs gather, the weight-
 * gradient folds scatter.  Results equal the dense pass's to rounding (sums of exact zeros are left out); the dropped filters'
 * and channels' gradients stay the zeros objective.lua:49 put there.  0 = multiply by the zeros like the reference does. */
int frcnn_set_option(const char *name, int value);
int frcnn_get_option(const char *name, int *value_host);

/* ---- device buffers (torch.CudaTensor storage; main.lua:86-89, objective.lua:66,147-149) */
int frcnn_malloc(void **ptr_out_host, size_t bytes);
int frcnn_free(void *ptr);
/* Page-locked host memory: a frcnn_memcpy_h2d / _d2h whose host side lives in such a buffer is truly asynchronous (the call
 * returns at once and the copy runs in stream order).  From ordinary (pageable) host memory the same call only returns when
 * the stream has reached the copy -- the host loses whatever lead it had over the device (in the training step: the example
 * tables of objective.lua:91-140 are uploaded mid-step, and a blocking upload made the device wait ~0.45 ms per step for
 * the launches that follow it).  The caller keeps the buffer untouched until the copy has run (an event or a later sync). */
int frcnn_host_alloc(void **ptr_out_host, size_t bytes);
int frcnn_host_free(void *ptr_host);
int frcnn_memcpy_h2d(void *dst, const void *src_host, size_t bytes, void *stream);
int frcnn_memcpy_d2h(void *dst_host, const void *src, size_t bytes, void *stream);
int frcnn_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int frcnn_stream_sync(void *stream);
int frcnn_zero(void *ptr, size_t bytes, void *stream);            /* gradient:zero(), objective.lua:49 */
int frcnn_scale(float *x, long long n, float s, void *stream);    /* gradient:div(n), objective.lua:200 */
int frcnn_add(float *y, const float *x, long long n, void *stream);   /* y:add(x), objective.lua:106,114,184 */

/* ---- per-kernel-class HIP-event profile (bench.py roofline leg) ---------------------- */
#define FRCNN_KC_CONV_IGEMM_K3 0
#define FRCNN_KC_CONV_IGEMM_OTHER 1
#define FRCNN_KC_CONV_WGRAD_K3 2
#define FRCNN_KC_CONV_WGRAD_OTHER 3
#define FRCNN_KC_GEMM 4
#define FRCNN_KC_ELEMWISE 5
#define FRCNN_KC_ROI 6
#define FRCNN_KC_RPN 7
#define FRCNN_KC_NMS 8
#define FRCNN_KC_OPTIM 9
#define FRCNN_KC_IMAGE 10
#define FRCNN_KC_CONV_X3 11      /* 3x3 forward + input gradient, split-bf16 operand form */
#define FRCNN_KC_CONV_WGRADX 12  /* 3x3 weight gradient, split-bf16 operand form */
#define FRCNN_KC_SOFT_NMS 13     /* Soft-NMS of the per-class pass (frcnn_soft_nms_batch); numbered in front of TOPK, which stays last */
#define FRCNN_KC_TOPK 14         /* proposal selection in front of the first NMS (frcnn_topk_select, frcnn_rpn_gather_rows) */
#define FRCNN_KC_COUNT 15
/* class_mask: bit k set -> every launch of kernel class k is bracketed by two hipEvents on its
 * launch stream (0 = profiling off). */
int frcnn_prof_enable(int class_mask);
/* Synchronises the device; per class: launches, total ms, algorithmic flops, algorithmic bytes.
 * Arrays of FRCNN_KC_COUNT entries (host).  Resets the profile. */
int frcnn_prof_collect(long long *launches_host, double *ms_host, double *flops_host,
                       double *bytes_host);

/* ---- nms(boxes, overlap, scores): nms.lua:23-102 ------------------------------------- */
/* key_mode: 0 = y2 (what every reference call site gets, Detector.lua:82,133: a tensor/nil
 * `scores` falls through to nms.lua:42), 1 = 'area' (nms.lua:39-40), 2 = column key_col
 * (1-based; nms.lua:37-38).  pick: int64[n] of 1-based row ids in pick order; *count = number
 * picked.  Bit-exact with the reference's fp32 CPU arithmetic. */
size_t frcnn_nms_workspace_bytes(int n);
int frcnn_nms_device(const float *boxes, int n, int ncols, float overlap, int key_mode,
                     int key_col, long long *pick, int *count, void *workspace,
                     size_t workspace_bytes, void *stream);
/* The per-class loop of Detector.lua:125-136 (`for i,c in pairs(yclass) do ... nms(bb, 0.1, ...)`) in ONE call: row i only
 * suppresses rows of the same class cls[i] (device int[n]; any integers).  Picks come in global pick order (descending key),
 * i.e. the per-class pick lists interleaved: a stable partition of the picks by class gives, per class, exactly the result
 * of nms() on that class's rows (same relative order, same fp32 arithmetic).  cls == NULL: frcnn_nms_device. */
int frcnn_nms_device_classes(const float *boxes, int n, int ncols, float overlap, int key_mode, int key_col,
                             const int *cls, long long *pick, int *count, void *workspace,
                             size_t workspace_bytes, void *stream);
/* The same with the row count in DEVICE memory: n = min(*n_dev, n_cap); launches and workspace are sized for n_cap
 * (frcnn_nms_workspace_bytes(n_cap)).  Lets Detector.lua:39-85 run scan -> NMS, and :115-136 class test -> per-class NMS,
 * without a host round trip for the count in between.  cls may be NULL. */
int frcnn_nms_device_n(const float *boxes, int n_cap, const int *n_dev, int ncols, float overlap, int key_mode, int key_col,
                       const int *cls, long long *pick, int *count, void *workspace, size_t workspace_bytes, void *stream);
/* B independent problems in ONE pass (Detector:detect_batch, and :detect with B = 1; every stage one launch with the segment
 * as a grid dimension, the greedy scans as B workgroups side by side; the entry points above are this pass with B = 1).
 * Segment b: rows boxes + b*row_stride*ncols, count min(n_dev[b], n_cap) (device int[B], required), cls + b*row_stride
 * (optional), picks pick + b*row_stride (1-based rows WITHIN the segment), survivor count count[b].  row_stride >= n_cap.
 * Per segment the result is bit for bit frcnn_nms_device_n on that segment; a segment with count 0 writes count[b] = 0 and
 * nothing else.  Workspace: frcnn_nms_batch_workspace_bytes(B, n_cap) -- the masks are n_cap^2 / 8 bytes per segment
 * (33.5 MB at 16 384). */
size_t frcnn_nms_batch_workspace_bytes(int B, int n_cap);
int frcnn_nms_device_batch(const float *boxes, int B, long long row_stride, int n_cap, const int *n_dev, int ncols, float overlap,
                           int key_mode, int key_col, const int *cls, long long *pick, int *count, void *workspace,
                           size_t workspace_bytes, void *stream);
/* ---- Soft-NMS (Bodla et al. 2017; not in the reference; csrc/soft_nms.hip) ----------------------------------------------
 * The per-class pass of Detector.lua:125-136 deletes every box that overlaps a better one of its class by more than 0.1;
 * Soft-NMS lowers the neighbours' scores instead (cfg.nms = { method = "hard" | "linear" | "gaussian", overlap, sigma,
 * min_score }; default: the reference).  One SEGMENT is one frame's rows: n rows of ncols fp32 columns, columns 1-4 =
 * x1 y1 x2 y2, column score_col (1-based, 5 .. ncols) the score, cls[i] an optional integer class.
 *   method 0 hard, 1 linear, 2 gaussian; overlap = Nt; sigma > 0; min_score; log_domain 0: scores are plain non-negative
 *   numbers, 1: scores are log-probabilities (what frcnn_detect_post puts in bb[:,4]) and decays are ADDED, and min_score
 *   is a log too.
 *   s[i] = score column; row i is alive iff s[i] >= min_score (a NaN is never alive)
 *   repeat: m = the alive, unpicked row of largest s (compared as fp32 values); ties: the HIGHER row id (the tie rule of
 *           frcnn_nms_device: ascending key, ties ascending row, picks from the end); none left -> stop
 *           pick m; score_out[m] = s[m]; for every alive unpicked j with cls[j] == cls[m] (all j when cls is NULL):
 *             hard:     if !(iou <= Nt): j dies
 *             linear:   if !(iou <= Nt): s[j] = s[j] * (1 - iou)               (log_domain: s[j] + log1pf(-iou))
 *             gaussian: (every j)        s[j] = s[j] * expf(-(iou*iou)/sigma)  (log_domain: s[j] - (iou*iou)/sigma)
 *             then: if !(s[j] >= min_score): j dies
 * All arithmetic is fp32, every operation rounded on its own; area and IoU are those of frcnn_nms_device:
 * area = (x2-x1+1)*(y2-y1+1), w = max(0, (xx2 + (-1)*xx1) + 1), iou = (w*h) / ((area_j + area_m) - w*h).  hard (either
 * domain), linear with log_domain 0 and gaussian with log_domain 1 contain no transcendental and are EXACT (a function of the
 * inputs' bits); linear with log_domain 1 (log1pf) and gaussian with log_domain 0 (expf) are within the math library's error.
 * No atomics: the result depends on the data alone.
 * Outputs: pick[0 .. count) = 1-based rows within the segment in pick order -- the scores at pick never increase along it, so
 * it is the rows sorted by final score descending, ties by the higher row, and a stable partition by class gives the
 * per-class lists (as frcnn_nms_device_classes); score_out[row * score_stride] (optional) = the score at pick, written for
 * picked rows only.  Nothing is stored outside [0, count) of pick, for unpicked rows, or -- beyond count[b] = 0 -- for an
 * empty segment.
 * Segments as in frcnn_nms_device_batch: segment b = boxes + b*row_stride*ncols, count min(n_dev[b], n_cap) read on the
 * device, row_stride >= n_cap; cls, pick and score_out are offset by b*row_stride rows; one workgroup per segment, whose
 * result does not depend on its slot or its neighbours.  n_cap <= 16 384.  Errors (before any launch): B < 1, n_cap out of
 * range, row_stride < n_cap, ncols < 5, score_col outside [5, ncols], bad method, sigma <= 0, NULL boxes / n_dev / pick /
 * count, short workspace (frcnn_soft_nms_workspace_bytes(B, n_cap)). */
size_t frcnn_soft_nms_workspace_bytes(int B, int n_cap);
int frcnn_soft_nms_batch(const float *boxes, int B, long long row_stride, int n_cap, const int *n_dev, int ncols, int score_col,
                         int method, float overlap, float sigma, float min_score, int log_domain, const int *cls,
                         long long *pick, int *count, float *score_out, long long score_stride, void *workspace,
                         size_t workspace_bytes, void *stream);
/* ---- Bounding-box voting (Gidaris & Komodakis 2015; not in the reference; csrc/box_vote.hip) -------------------------------
 * A winner of the per-class pass carries the one regressed box of the candidate that won; the other survivors of its class
 * that sit on the same object are dropped (or re-scored by Soft-NMS).  Voting replaces the winner's box by the weighted mean
 * of all of them (cfg.box_voting = { overlap, weight }; default: off).  One SEGMENT is one frame's rows: n rows of ncols fp32
 * columns, columns 1-4 = x1 y1 x2 y2, column score_col (1-based, 5 .. ncols; ignored under weight_mode 0) the score, cls[i] an
 * optional integer class, rect[i][0..3] optional fp64 coordinates.
 * Winners of a segment: the 1-based rows pick[0 .. min(count, n)).  For a winner row m:
 *   VOTERS   row j of the segment votes iff cls[j] == cls[m] (every row when cls is NULL) AND iou(j, m) >= overlap AND its
 *            weight w_j is finite and > 0.  iou is frcnn_nms_device's fp32 arithmetic, every operation rounded on its own:
 *            area = (x2-x1+1)*(y2-y1+1), w = max(0, (xx2 + (-1)*xx1) + 1), iou = (w*h) / ((area_j + area_m) - w*h).  A NaN IoU
 *            is not a vote; m itself goes through the same test.  Who votes is a function of the inputs' bits: EXACT.
 *   WEIGHTS  fp64.  weight_mode 0: 1.  1: (double)score_j, a plain score.  2: exp((double)score_j), a log-probability (what
 *            frcnn_detect_post puts in bb[:,4]); within the math library's error of exp.
 *   COORDS   c_j = rect[j][0..3] when rect is given, else (double)boxes[j][0..3].
 *   RESULT   rect_out[m][t] = (sum w_j c_j[t]) / (sum w_j) over the voters, in fp64: one rounded product per term, the sums in a
 *            fixed order (lane l of a 64-lane wave adds rows l, l+64, ... ascending; a butterfly 32 .. 1 adds the lanes), one
 *            division.  No atomics: the value is a function of the segment's data alone -- not of the slot, of B, of the
 *            neighbours or of the run.  votes_out[m] (optional) = the number of voters.  With FEWER THAN TWO voters
 *            rect_out[m] = c_m bit for bit: an isolated detection is unchanged by voting (a lone voter other than m exists only
 *            when m itself is barred by its weight or a NaN IoU; it does not move m either).
 * Nothing is stored for rows that are not winners, for an empty segment or for a segment with count[b] == 0; a pick outside
 * [1, n] is skipped.  Inputs are only read.
 * Segments as in frcnn_nms_device_batch: segment b = boxes + b*row_stride*ncols, n = min(n_dev[b], n_cap) read on the device,
 * row_stride >= n_cap; cls, rect, pick, rect_out and votes_out are offset by b*row_stride rows; count is a device int[B].  One
 * wave per winner; no limit on n_cap beyond int (up to 2048 rows a segment is staged in LDS, beyond that read from global
 * memory).  No workspace.  Errors (before any launch): B < 1 (or > 65535), n_cap < 0, row_stride < n_cap, ncols < 4, score_col
 * outside [5, ncols] under weight_mode 1 / 2, bad weight_mode, overlap not in (0, 1] or NaN, NULL boxes / n_dev / pick / count /
 * rect_out.  Counted under FRCNN_KC_NMS. */
int frcnn_box_vote_batch(const float *boxes, int B, long long row_stride, int n_cap, const int *n_dev, int ncols, int score_col,
                         int weight_mode, float overlap, const int *cls, const double *rect, const long long *pick,
                         const int *count, double *rect_out, int *votes_out, void *stream);
/* ---- The proposal-target layer (Ren et al. 2015, training the detector on the RPN's proposals; not in the reference;
 * csrc/proposal_targets.hip) ---------------------------------------------------------------------------------------------------
 * objective.lua:91-140 trains the classification net on the ground-truth rects of the positive anchors and the rects of the sampled
 * negative anchors; under cfg.roi_sampling = { source = "proposals", ... } its rows are a sample of what the first NMS leaves.  This
 * ONE launch sits between frcnn_nms_device_batch and frcnn_roi_windows / RoIAlign: it matches a segment's candidates to its
 * ground truth, labels them, draws a batch and writes the rect table and the targets frcnn_cnet_losses reads.
 * Segment b (one frame): rect + b*match_stride*4 (device double[match_stride][4]) and pick + b*match_stride (device int64, 1-based
 * rows of the segment's rect) as the first NMS leaves them; r_dev[b] (device int) the candidate count, of which the kernel uses the
 * first R = min(max(r_dev[b], 0), r_cap) picks -- the post-NMS cap, applied on the device; gt_rect + b*gt_stride*4 (device
 * double[gt_stride][4]), gt_class + b*gt_stride (device int, 1-based); G_host[b] its ground-truth count, a HOST array that travels
 * as a kernel argument (no upload, no wait).
 *   CANDIDATES  index i in [0, G) is ground-truth box i when include_gt != 0; behind them i = G' + j is pick j (G' = G or 0);
 *               N = G' + R <= 4096.  A pick outside 1 ... match_stride is read nowhere and counts as an ignored candidate.
 *   RULE        fp64, every operation rounded on its own, the formula of Rect.lua:126-141 (no + 1, unlike nms): with max(a, b) = b
 *               when b > a else a, min(a, b) = b when b < a else a, minx = max(c.minX, g.minX) ..., the intersection is
 *               (maxx - minx) * (maxy - miny) when maxx >= minx && maxy >= miny, else 0; iou = inter / ((area_c + area_g) - inter),
 *               a quotient that is not a number counts as 0.  best = the FIRST maximum over g (the lowest g wins a tie); G = 0:
 *               best_iou = 0, gt_idx = -1.  A candidate with a coordinate that is not finite, or a width or height <= 0, is
 *               ignored.  fg: gt_idx >= 0 && best_iou >= fg_iou -- foreground needs a box it matched, so a segment with G = 0 has none
 *               whatever fg_iou is (fg_iou = 0 included).  bg: not fg && bg_lo <= best_iou < bg_hi.  Everything else is ignored.
 *   QUOTAS      F = min(nfg, fg_quota), Bq = min(nbg, batch - F).  A class over its quota keeps the rows with the smallest keys;
 *               key of row i, all operations uint32: x = seed + 0x9E3779B9*(i+1) + 0x85EBCA6B*b; x ^= x>>16; x *= 0x85EBCA6B;
 *               x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16.  The mix is a bijection and a segment's pre-images differ: keys never tie.
 *   OUTPUTS     rows at b*out_stride: the F fg rows in candidate order, then the Bq bg rows in candidate order; nothing is stored
 *               behind row F + Bq.  roi[4] (double) = the candidate's rect bit for bit; crtarget[4] (float) =
 *               (float) Anchors.inputToAnchor(candidate, gt[best]) (Anchors.lua:237-243: (gx - cx) / cw, (gy - cy) / ch,
 *               log(gw / cw), log(gh / ch) in fp64) for fg, zeros for bg; cctarget (float) = gt_class[best] for fg, bgclass for bg;
 *               src (int) = i; gt_idx (int) = best; iou (double) = best_iou.  counts[b][4] = {nfg, nbg, F, Bq}.  A segment with
 *               N = 0 writes its counts (all 0) and nothing else.
 * One workgroup per segment, no atomics, no workspace: a segment's output is a function of its own data, b and seed -- not of B, of
 * its neighbours or of the run.  One launch for up to 128 segments.  Everything but log() is exact; log is the device library's
 * (within an ulp).  roi, crtarget and counts are stored 16 bytes at a time and must be 16-byte aligned.
 * Errors, returned before any launch (B = 0 returns at once): B outside 0 ... 65535, G_host[b] outside 0 ... 64 or above gt_stride,
 * r_cap negative or r_cap + 64 > 4096, match_stride < r_cap, bg_hi > fg_iou or bg_lo > bg_hi (or a NaN), batch < 1, fg_quota
 * outside 0 ... batch, out_stride < batch, bgclass < 1, a NULL required pointer (rect / pick only with r_cap > 0, gt_rect / gt_class
 * only with a G_host > 0), a misaligned roi / crtarget / counts.  Counted under FRCNN_KC_RPN. */
int frcnn_proposal_targets_batch(const double *rect, const long long *pick, long long match_stride, const int *r_dev, int r_cap,
                                 const double *gt_rect, const int *gt_class, int gt_stride, const int *G_host, int B,
                                 int include_gt, double fg_iou, double bg_lo, double bg_hi, int fg_quota, int batch, int bgclass,
                                 unsigned int seed, double *roi, float *crtarget, float *cctarget, int *src, int *gt_idx,
                                 double *iou, int out_stride, int *counts, void *stream);
/* ---- Detector:detect glue kept on the device (Detector.lua:88-136; csrc/detect.hip) ------------------------------
 * frcnn_roi_windows: extract_roi_pooling_input (objective.lua:5-13) for k ROIs at once -- Localizer:inputToFeatureRect
 * (Localizer.lua:41-67, the reference's double arithmetic incl. its dH/dW mix-ups) over layers_host[nlayers][6] =
 * {kW,kH,dW,dH,padW,padH} (frcnn_model_localizer_layers), clip to the fmH x fmW map, 1-based inclusive window
 * wins[k][4] = {row_lo,row_hi,col_lo,col_hi}.  rect: device double[n][4]; pick: optional device int64[k] of 1-based rows of
 * rect (the NMS candidates), NULL = rows 0..k-1. */
int frcnn_roi_windows(const double *rect, const long long *pick, int k, const int *layers_host, int nlayers, int fmH, int fmW,
                      int *wins, void *stream);
/* frcnn_detect_post: Detector.lua:106-122 for the R candidates (cls / conf from frcnn_cnet_decode, bbox = cnet's R x 4
 * output, rect / pick as above): candidate r survives iff cls[r] != bgclass and exp(conf[r]) > min_conf; survivors, in
 * candidate order, get r2 = Anchors.anchorToInput(anchor rect, bbox row) in double (r2[K][4]), bb[K][5] = {float(r2), conf},
 * kc[K] = class, keep_row[K] = r (0-based); *K_dev = their number (device).  All outputs need room for R rows. */
int frcnn_detect_post(const int *cls, const float *conf, const float *bbox, const double *rect, const long long *pick, int R,
                      int bgclass, double min_conf, float *bb, int *kc, int *keep_row, double *r2, int *K_dev, void *stream);
/* frcnn_detect_classes_batch: the class test of B frames in ONE launch (Detector under cfg.scoring), read from the net's outputs:
 * frame b's R_host[b] candidates are rows row0_host[b] ... of cls_out (ncls fp32 log-probabilities a row) and of bbox (4 a row);
 * both arrays are HOST values and travel as kernel arguments (no upload, no wait).  rect / pick: the match arrays, match_stride
 * rows a frame.  Candidate r of frame b emits, in candidate order,
 *   mode 0 (top class)    the row (r, c*), c* the first maximum of its log-probabilities (frcnn_cnet_decode), iff c* != bgclass and
 *                         exp((double)lp[c*]) > min_conf: per frame exactly frcnn_cnet_decode + frcnn_detect_post, bit for bit;
 *   mode 1 (all classes)  one row (r, c) for every class c != bgclass with exp((double)lp[c]) > min_conf, c ascending (a NaN emits
 *                         nothing).
 * A row j of frame b lies at row b*row_stride + j of the outputs: bb[5] = {float(r2), lp[c]}, kc = c (1-based), keep_row = r
 * (0-based), r2[4] = Anchors.anchorToInput(anchor rect, bbox row) in double, decoded once per candidate (the rows of one candidate
 * carry identical coordinates).  total_dev[b] (device int[B], optional) = the rows the rule emits, K_dev[b] (device int[B]) =
 * min(total, row_stride): only the first row_stride rows are stored, nothing is written behind row K_dev[b].  A frame with
 * R_host[b] = 0 writes its two counts (0) and nothing else.  Errors (B outside 0 ... 65535, ncls < 2, bgclass outside 1 ... ncls,
 * mode, a negative stride, R or row0, a NULL required pointer) are returned before any launch. */
int frcnn_detect_classes_batch(const float *cls_out, const float *bbox, const int *R_host, const long long *row0_host, int B,
                               const double *rect, const long long *pick, long long match_stride, int ncls, int bgclass,
                               double min_conf, int mode, float *bb, int *kc, int *keep_row, double *r2, int row_stride, int *K_dev,
                               int *total_dev, void *stream);
/* frcnn_detect_gather_batch: the winner tables of B frames in one launch (Detector:detect_batch, and Detector:detect with
 * B = 1), all in ONE buffer (one read-back): frame b's table starts at rec + b*(row_stride + 1)*16 doubles -- a 128-byte header
 * whose first four ints are the frame's counts, then one record of 16 doubles per winner q < min(winners, row_stride), in the
 * pick order wpick of the per-class NMS over bb/kc: {class, candidate row (1-based), confidence (log-prob), p (anchor
 * log-prob), anchor rect x4, r2 x4, anchor index {layer,aspect,y,x}} -- everything Detector.lua:116-122 puts into a
 * detection's table.  counts: device int[4][B] = {matches, candidates, survivors of the class test, winners} per frame.
 * wpick / keep_row / kc / bb / r2 hold row_stride rows per frame, pick / match_* match_stride rows. */
int frcnn_detect_gather_batch(const long long *wpick, const int *counts, int B, int row_stride, const int *keep_row,
                              const int *kc, const float *bb, const double *r2, const long long *pick, long long match_stride,
                              const float *match_p, const double *match_rect, const int *match_idx, double *rec, void *stream);
/* frcnn_detect_merge_views: test-time augmentation (Detector under cfg.tta; not in the reference).  A frame was detected on V
 * views of itself (rescaled and / or mirrored copies), V consecutive segments of a chunk of F*V segments; this ONE launch turns the
 * class-test survivors of every frame's views into one segment of V*row_stride rows in the frame's own coordinates, which the
 * per-class pass, voting and frcnn_detect_gather_batch then read with B = F, row stride V*row_stride, match stride V*match_stride.
 * Inputs: bb / kc / keep_row / r2 as frcnn_detect_post or frcnn_detect_classes_batch left them (row_stride rows a segment),
 * counts = device int[4][F*V] (row 0: the segments' matches, row 2: their survivors K, clipped to row_stride), pick = the first
 * NMS's picks (match_stride rows a segment).  Geometry of view i = f*V + v, HOST arrays of F*V entries that travel as kernel
 * arguments (no upload, no wait): flip_host (the view is mirrored left-right), wv_host (its width), ax_host / ay_host (frame width
 * / view width, frame height / view height), R_host (its candidates, 0 ... match_stride).
 * Frame f's outputs start at row f*V*row_stride (bb_out, kc_out, keep_row_out, r2_out) and f*V*match_stride (pick_out):
 *   ROWS    survivor j of view v lies at row sum_{u<v} K_u + j: view order, row order within a view; nothing is written behind
 *           row K' = sum K_u.  No atomics: a frame's output is a function of its own segments.
 *   COORDS  fp64, every operation rounded on its own, in this order: a mirrored view un-mirrors (x1' = wv - x2, x2' = wv - x1:
 *           BatchIterator.lua:57-62, its own inverse), then x1, x2 are multiplied by ax (unless ax == 1) and y1, y2 by ay (unless
 *           ay == 1) -- an unmirrored view with ax == ay == 1 keeps its bits.  r2_out holds these doubles, bb_out[0..3] their
 *           (float); bb_out[4] (the log-confidence) and kc_out are copied.
 *   PICKS   the candidates of a frame are the concatenation of its views' candidates: keep_row_out = Roff_v + keep_row with
 *           Roff_v = sum_{u<v} R_host[u], and pick_out[Roff_v + r] = v*match_stride + pick[r] (still 1-based) for EVERY candidate
 *           r < R_host of view v; nothing behind sum R_host.  The match arrays stay where they are: a frame's views are
 *           consecutive segments, so row pick_out - 1 of frame f's V*match_stride match rows is the view's own row.
 *   COUNTS  counts_out = device int[4][F]: rows 0 ... 2 of frame f = the sum of its views' matches, of R_host, and K'; row 3 is
 *           left to the per-class pass.
 * Errors, returned before the launch: F outside 1 ... 65535, V outside 1 ... 8, a negative stride, V * stride beyond int, a NULL
 * required pointer, an R_host outside 0 ... match_stride, a width or factor that is not finite or not positive.  One launch for
 * up to 64 views (more: one per 64 / V frames).  Counted under FRCNN_KC_ELEMWISE. */
int frcnn_detect_merge_views(const float *bb, const int *kc, const int *keep_row, const double *r2, long long row_stride,
                             const int *counts, const long long *pick, long long match_stride, int F, int V,
                             const int *flip_host, const double *wv_host, const double *ax_host, const double *ay_host,
                             const int *R_host, float *bb_out, int *kc_out, int *keep_row_out, double *r2_out,
                             long long *pick_out, int *counts_out, void *stream);
/* Host-pointer variant (the reference's nms runs on CPU FloatTensors): uploads, runs the same
 * kernels, downloads, synchronises. */
int frcnn_nms_host(const float *boxes_host, int n, int ncols, float overlap, int key_mode,
                   int key_col, long long *pick_host, int *count_host);

/* ---- nn.SpatialConvolution (models/model_utilities.lua:8,31,33) ---------------------- */
/* out[O][Ho][Wo] = bias + W (*) act(in), Ho = H + 2*pad - k + 1.  act(x) = in_scale[c] *
 * prelu(x, *in_slope) is the producing layer's nn.PReLU + nn.SpatialDropout fused into the
 * load (pass NULL for identity).  weight is the canonical [O][C][k][k] tensor.  k in {1,3,5,7},
 * stride 1.  :updateOutput, reached from objective.lua:71 / Detector.lua:33. */
int frcnn_conv2d_forward(const float *in, int C, int H, int W, const float *in_slope,
                         const float *in_scale, const float *weight, const float *bias, int O,
                         int k, int pad, float *out, void *stream);
/* :updateGradInput (objective.lua:189): gin[C][H][W] = W^T (*) gout. accumulate!=0 -> += */
int frcnn_conv2d_backward_input(const float *gout, int O, int Ho, int Wo, const float *weight,
                                int C, int k, int pad, float *gin, int accumulate, void *stream);
/* :accGradParameters (objective.lua:189): gweight += gout (x) act(in); gbias += sum gout. */
int frcnn_conv2d_backward_weight(const float *in, int C, int H, int W, const float *in_slope,
                                 const float *in_scale, const float *gout, int O, int k, int pad,
                                 float *gweight, float *gbias, void *stream);

/* ---- nn.PReLU + nn.SpatialDropout + nn.SpatialMaxPooling(2,2,2,2):ceil()
 *      (models/model_utilities.lua:9-12,23) -------------------------------------------- */
/* out = maxpool2x2_ceil(in_scale[c]*prelu(x)); idx[c][oy][ox] = dy*2+dx of the (first) max. */
int frcnn_maxpool_act_forward(const float *x, int C, int H, int W, const float *slope,
                              const float *scale, float *out, unsigned char *idx, void *stream);
/* gx = unpool(gpool) * scale[c] * prelu'(x); gbias[c] += sum gx; *gslope += sum_{x<=0} x*g. */
int frcnn_maxpool_act_backward(const float *gpool, const unsigned char *idx, const float *x, int C,
                               int H, int W, const float *slope, const float *scale, float *gx,
                               float *gbias, float *gslope, void *stream);
int frcnn_act_forward(const float *x, int C, long long hw, const float *slope, const float *scale,
                      float *y, void *stream);
int frcnn_act_backward(const float *gy, const float *x, int C, long long hw, const float *slope,
                       const float *scale, float *gx, float *gbias, float *gslope, void *stream);
/* Test entry points of two fused launches that the model's training step makes and no other entry point reaches.
 *
 * frcnn_conv2d_forward_pool: the last 3x3 convolution of a backbone block on the fp32 kernel (whatever the split-form
 * options say), with the block's nn.PReLU + nn.SpatialDropout + 2x2 ceil-mode max pool offered to the launch's epilogue:
 * out[O][Ho][Wo] as frcnn_conv2d_forward (k = 3); pooled[O][Hp][Wp], pidx[O][Hp][Wp] as frcnn_maxpool_act_forward(out, O,
 * Ho, Wo, pool_slope, pool_scale), Hp = (Ho - 1) / 2 + 1; rec (NULL: none) the record of `pooled`.  The launch takes the
 * pool only for some shapes; for the others the pooling kernel runs behind it, as in the model.  *fused_out (host int,
 * NULL: not wanted) = 1 when the launch took it.  Synchronises. */
int frcnn_conv2d_forward_pool(const float *in, int C, int H, int W, const float *in_slope,
                              const float *in_scale, const float *weight, const float *bias, int O, int pad,
                              const float *pool_slope, const float *pool_scale, float *out, float *pooled,
                              unsigned char *pidx, float *rec, int *fused_out, void *stream);
/* frcnn_conv2d_backward_weight_pooled: :accGradParameters of a first-layer 3x3 convolution (C <= 3, O <= 64, Wo >= 2)
 * straight from the gradient of its pooled map: with g = unpool(gpool, pidx) * prelu'(x, *slope), x[O][Ho][Wo] the
 * convolution's output, gweight += g (x) in, gbias += sum g, *gslope += sum_{x<=0} x * unpool(gpool, pidx).  An error,
 * and nothing is written, for any other shape or a NULL slope.  Synchronises. */
int frcnn_conv2d_backward_weight_pooled(const float *in, int C, int H, int W, const float *gpool,
                                        const unsigned char *pidx, const float *x, const float *slope, int O,
                                        int pad, float *gweight, float *gbias, float *gslope, void *stream);

/* ---- magnitude records of the two-plane fp16 form (option "x3_f16") ----------------------------
 * The split convolutions scale each operand by a power of two taken from the tensor's largest magnitude.  That number
 * travels as a RECORD: device memory of frcnn_amax_record_floats() floats, rec[0] = the bit pattern of an int n
 * (1 <= n <= 16384), rec[1..n] = one max|x| per block of the launch that wrote the tensor; the tensor's largest magnitude
 * is the maximum of the n entries.  A launch that keeps a record rewrites the count and all its n entries; nothing else.
 * The entry points above take the records they need in passes of their own; the *_rec forms below let a host that drives
 * single layers chain them instead (the producer of a tensor keeps the record its consumer reads), and let tests read what
 * each producer keeps. */
int frcnn_amax_record_floats(void);
/* rec = the record of x[0..n) (n >= 1; x at any 4-byte boundary), in a pass of its own. */
int frcnn_tensor_absmax(const float *x, long long n, float *rec, void *stream);
/* The entry points of the same names that also keep the record of what they store (out / gx) in rec (NULL: none). */
int frcnn_maxpool_act_forward_rec(const float *x, int C, int H, int W, const float *slope,
                                  const float *scale, float *out, unsigned char *idx, void *stream, float *rec);
int frcnn_maxpool_act_backward_rec(const float *gpool, const unsigned char *idx, const float *x, int C,
                                   int H, int W, const float *slope, const float *scale, float *gx,
                                   float *gbias, float *gslope, void *stream, float *rec);
int frcnn_act_backward_rec(const float *gy, const float *x, int C, long long hw, const float *slope,
                           const float *scale, float *gx, float *gbias, float *gslope, void *stream, float *rec);
/* frcnn_conv2d_forward in the two-plane fp16 form.  rec_in: the record of `in` kept by its producer (NULL: taken here in a
 * pass over `in`); rec_out: receives the record of `out` (NULL: none).  An error, and nothing is launched, when the shape
 * does not take the split form, when option "x3_f16" is off, or when an entry of in_scale exceeds 1 in magnitude. */
int frcnn_conv2d_forward_rec(const float *in, int C, int H, int W, const float *in_slope,
                             const float *in_scale, const float *weight, const float *bias, int O,
                             int k, int pad, float *out, const float *rec_in, float *rec_out, void *stream);
/* frcnn_conv2d_backward_input in the two-plane fp16 form.  rec_g: the record of gout (NULL: taken here); rec_out: receives
 * the record of what is stored in gin (with accumulate: of the sums).  post_x != NULL (k = 3, accumulate = 0): gin passes
 * through the backward of the nn.PReLU + nn.SpatialDropout in front of this convolution inside the launch --
 * gin = prelu'(post_x) * post_scale[c] * (W^T (*) gout), *gslope += sum over post_x <= 0 of post_x * post_scale[c] * (...) --
 * with post_x float [C][H][W] the pre-activation values, post_slope a device scalar, post_scale float [C] or NULL, gslope a
 * device scalar or NULL.  Same refusals as frcnn_conv2d_forward_rec. */
int frcnn_conv2d_backward_input_rec(const float *gout, int O, int Ho, int Wo, const float *weight,
                                    int C, int k, int pad, float *gin, int accumulate, const float *rec_g,
                                    float *rec_out, const float *post_x, const float *post_slope,
                                    const float *post_scale, float *gslope, void *stream);

/* ---- extract_roi_pooling_input + nn.SpatialAdaptiveMaxPooling, batched over ROIs
 *      (objective.lua:5-13,117-118,137-138,182-185; Detector.lua:96-97) ----------------- */
/* wins: int[R][4] = {row_lo,row_hi,col_lo,col_hi}, 1-based inclusive (objective.lua:11).
 * out: [R][C*kh*kw] (row r = amp:forward(view):view(kh*kw*C)); idx: int[R][C*kh*kw], flat
 * 0-based y*W+x position of each max inside the full map (amp.indices equivalent). */
int frcnn_roi_pool_forward(const float *fmap, int C, int H, int W, const int *wins, int R, int kh,
                           int kw, float *out, int *idx, void *stream);
/* gmap[C][H][W] += scatter(gout) -- delta_outputs[5][idx]:add(amp:backward(...)) */
int frcnn_roi_pool_backward(float *gmap, int C, int H, int W, const float *gout, const int *idx,
                            int R, int kh, int kw, void *stream);

/* ---- RoIAlign, the alternative region feature (cfg.roi_pooling.method = "align"; not in the reference; csrc/roi_align.hip)
 * Bilinear sampling at un-snapped coordinates, g x g samples averaged per bin (the torchvision `aligned=True` rule).
 * rect: device double[n][4] of INPUT-space rects {minX, minY, maxX, maxY}; pick: optional device int64[R] of 1-based rows of
 * rect, NULL = rows 0..R-1 (as in frcnn_roi_windows: the Detector hands over match_rect and the first NMS's picks as they
 * are).  inv_sx / inv_sy: one over the backbone's stride (Localizer.stride(); the backbone must be centred: cell i covers input
 * pixels [i S, (i+1) S)).  The kernels multiply by inv_sx where the convention reads minX/Sx: the same number for a power-of-two
 * stride (16 for both models); for another stride a coordinate may differ from the quotient in its last bit.  1 <= g <= 4.
 * All in double, in this order:
 *     x1 = minX*inv_sx - 0.5                y1 = minY*inv_sy - 0.5
 *     w  = max((maxX-minX)*inv_sx, 0)       h  = max((maxY-minY)*inv_sy, 0)         bin_w = w/kw    bin_h = h/kh
 *     sample (i, j, iy, ix):  y = y1 + (i + (iy+0.5)/g)*bin_h ,  x = x1 + (j + (ix+0.5)/g)*bin_w
 * A sample with y < -1 || y > H || x < -1 || x > W contributes 0.  Otherwise y = max(y, 0), y_lo = (int)y; y_lo >= H-1:
 * y_lo = y_hi = H-1, y = y_lo; else y_hi = y_lo + 1; ly = y - y_lo; the same in x.  Weights (1-ly)(1-lx), (1-ly)lx, ly(1-lx),
 * ly*lx, computed in double and rounded to fp32.  out[r][c][i][j] = the fp32 sum over the g*g samples (iy outer, ix inner, the
 * four taps in the order above) times 1/g^2; rows [R][C*kh*kw] like frcnn_roi_pool_forward.  No atomics: two runs are bit-equal.
 * R <= 0: no launch. */
int frcnn_roi_align_forward(const float *fmap, int C, int H, int W, const double *rect, const long long *pick, int R,
                            double inv_sx, double inv_sy, int kh, int kw, int g, float *out, void *stream);
/* gmap[C][H][W] += scatter: every bin spreads gout/g^2 over its 4 g^2 taps.  No index tensor: the geometry is recomputed from
 * the rects.  Option "deterministic": 64-bit fixed-point accumulation, the result does not depend on the order of the atomics. */
int frcnn_roi_align_backward(float *gmap, int C, int H, int W, const float *gout, const double *rect, const long long *pick,
                             int R, double inv_sx, double inv_sy, int kh, int kw, int g, void *stream);

/* ---- RPN anchor scan: Detector.lua:39-66 --------------------------------------------- */
/* maps_host: 4 device pointers to the [18][H_l][W_l] head outputs (pnet outputs 1..4).
 * anchor_w / anchor_h: the fp32 tables of Anchors.lua:18-19, [4][3][200][2].
 * Outputs in scan order (layer, y, x, aspect), at most cap entries:
 *   match_p[i]    = c[1] (log-prob of foreground)
 *   match_idx[i]  = {layer, aspect, y, x} 1-based (Anchors:get arguments)
 *   match_rect[i] = decoded rect as doubles (Lua numbers), {minX,minY,maxX,maxY}
 *   match_box[i]  = the same as fp32 (the FloatTensor row of Detector.lua:74-79, NMS input)
 *   *count        = number of matches found (may exceed cap; only cap are written) */
size_t frcnn_rpn_scan_workspace_bytes(const int *H_host, const int *W_host);
int frcnn_rpn_scan(const float *const *maps_host, const int *H_host, const int *W_host,
                   const float *anchor_w, const float *anchor_h, double img_w, double img_h,
                   double p_threshold, int cap, float *match_p, int *match_idx,
                   double *match_rect, float *match_box, int *count, void *workspace,
                   size_t workspace_bytes, void *stream);
/* The same for B frames in one pass (Detector:detect_batch, and Detector:detect with B = 1): maps_host are the four maps of
 * frame 0, frame b's are slot_stride
 * floats further (every map); one launch for the threshold test, one for the ordered compaction with one workgroup per
 * frame.  Frame b's matches are rows [b*cap, b*cap + min(count[b], cap)) of the match arrays, count: device int[B].  Per
 * frame bit-identical to frcnn_rpn_scan, which is this pass with B = 1. */
size_t frcnn_rpn_scan_batch_workspace_bytes(const int *H_host, const int *W_host, int B);
int frcnn_rpn_scan_batch(const float *const *maps_host, const int *H_host, const int *W_host, int B, long long slot_stride,
                         const float *anchor_w, const float *anchor_h, double img_w, double img_h, double p_threshold,
                         int cap, float *match_p, int *match_idx, double *match_rect, float *match_box, int *count,
                         void *workspace, size_t workspace_bytes, void *stream);
/* The same for B frames of DIFFERENT sizes (Detector:detect_batch with mixed_sizes).  Host arrays, read before the call
 * returns: H_host / W_host [B][4] (frame b's head-map sizes), map_off_host [B][4] (floats from `heads` to frame b's map l),
 * img_wh_host [B][2] = {img_w, img_h}.  Per frame exactly frcnn_rpn_scan on that frame's maps, sizes and image size, bit for
 * bit: frame b's matches are rows [b*cap, b*cap + min(count[b], cap)) of the match arrays, count (device int[B]) holds the
 * full numbers, nothing is stored behind a frame's matches.  Two launches per group of at most 16 frames (the frames'
 * descriptors travel as a kernel argument: no device table, no copy, no wait).  The workspace holds one slice per frame,
 * sized by that frame's anchors: for frames of one size the byte count is frcnn_rpn_scan_batch_workspace_bytes', for B = 1
 * frcnn_rpn_scan_workspace_bytes'.  Refused on the host before any launch: B < 0 or > 65535, an H or W outside 1 ... 200, a
 * negative cap or offset, a workspace that is too small, a NULL array with B > 0.  B == 0 does nothing.
 * The size query validates nothing: it counts a frame with an H or W outside 1 ... 200 as no anchors and returns the 256-byte
 * head alone for NULL arrays or B <= 0; the scan call checks the sizes before it looks at the workspace. */
size_t frcnn_rpn_scan_ragged_workspace_bytes(const int *H_host, const int *W_host, int B);
int frcnn_rpn_scan_ragged(const float *heads, const long long *map_off_host, const int *H_host, const int *W_host,
                          const double *img_wh_host, int B, const float *anchor_w, const float *anchor_h, double p_threshold,
                          int cap, float *match_p, int *match_idx, double *match_rect, float *match_box, int *count,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- score-ordered proposals with pre- and post-NMS caps (not in the reference; csrc/topk.hip) -----------------------
 * Detector.lua:39-85 hands every anchor with exp(p) > 0.95 to nms(), which ignores the scores it is given (key = max-y).  A
 * host may instead (cfg.proposals = { order = "y2" | "score", pre_nms_top_n = K, post_nms_top_n = M }; default: the reference)
 *   - keep only the K best-scoring matches in front of the first NMS (pre_nms_top_n; either order),
 *   - run both NMS passes keyed by the score (order = "score": the first on rows {box, p} with key_mode 2, key_col 5, the
 *     per-class one with key_col 5, the confidence; the NMS tie rule is the one of frcnn_nms_device),
 *   - keep only the first min(R, M) picks of the first NMS as candidates (post_nms_top_n; needs order = "score"; a clamp of
 *     the count on the host after the first read-back, no kernel).
 * RANK of a match: its fp32 p (the log-probability frcnn_rpn_scan stores), compared as fp32 VALUES: -0 equals +0, a NaN
 * ranks below everything (the scan never produces one); ties are broken by the LOWER scan row.
 * SELECTION: the K' = min(n, K) best-ranked rows, and they KEEP THEIR SCAN ORDER (ascending original row).  For K >= n the
 * selection is the identity, and everything downstream is bit-identical to the uncapped run with the same order.
 *
 * frcnn_topk_select: B segments in one launch (one workgroup per segment).  Segment b: keys score + b*stride, row count
 * min(n_dev[b], n_cap) read from DEVICE memory (as in frcnn_nms_device_batch; stride >= n_cap); writes the ascending 0-based
 * rows of the selected set to sel_row + b*sel_stride (sel_stride >= min(n_cap, K)) and k_dev[b] = K'.  A segment of count 0
 * writes k_dev[b] = 0 and nothing else; no segment stores outside [0, K') of its slice.  Exact and deterministic (radix
 * select on the order-preserving integer image of the key, integer counts only): the result depends on the data alone.
 * K >= 1.  Workspace: frcnn_topk_select_workspace_bytes(B, n_cap) (the keys' images). */
size_t frcnn_topk_select_workspace_bytes(int B, int n_cap);
int frcnn_topk_select(const float *score, int B, long long stride, int n_cap, const int *n_dev, int K, int *sel_row,
                      long long sel_stride, int *k_dev, void *workspace, size_t workspace_bytes, void *stream);
/* frcnn_rpn_gather_rows: the match arrays of frcnn_rpn_scan[_batch] (src_stride rows per segment, src_rows of them valid)
 * gathered into compact arrays of the same layouts (dst_stride rows per segment), all segments in one launch.  Row
 * j < min(k_dev[b], k_cap) of segment b comes from source row sel_row[b*sel_stride + j] (0-based, as frcnn_topk_select wrote
 * it; sel_row NULL: row j itself, k_dev then being the scan's own count).  Destinations, any of which may be NULL: dst_p,
 * dst_idx[4], dst_rect[4] (double), dst_box[4], box5[5] = {box, p} (the first NMS's input under order = "score"), row = the
 * 1-based original scan row.  frcnn_roi_windows, frcnn_detect_post and frcnn_detect_gather_batch then run unchanged on the
 * compact arrays; with sel_row NULL the call only builds box5 for all matches -- no host round trip between scan and NMS in
 * any mode.  The 16-byte rows (idx, box, rect) must be 16-byte aligned. */
int frcnn_rpn_gather_rows(const float *match_p, const int *match_idx, const double *match_rect, const float *match_box, int B,
                          long long src_stride, int src_rows, const int *sel_row, long long sel_stride, const int *k_dev,
                          int k_cap, float *dst_p, int *dst_idx, double *dst_rect, float *dst_box, float *box5, int *row,
                          long long dst_stride, void *stream);

/* ---- sparse RPN loss: objective.lua:91-140 (+ cnet targets, objective.lua:149-159) ---- */
/* Examples: positives first (npos) then negatives (nneg).  ex_idx int[E][4] {layer,aspect,y,x}
 * 1-based; ex_anchor double[E][4]; ex_roi double[npos][4] (roi.rect of each positive);
 * ex_class int[npos] (roi.class_index).  deltas_host: 4 device pointers to delta_outputs[1..4]
 * (gradients are ADDED).  ex_loss double[E][2] = {cls, reg*10}; crtarget float[E][4];
 * cctarget float[E] (class index, bgclass for negatives). */
int frcnn_rpn_loss(const float *const *maps_host, float *const *deltas_host, const int *H_host,
                   const int *W_host, const int *ex_idx, const double *ex_anchor,
                   const double *ex_roi, const int *ex_class, int npos, int nneg, int bgclass,
                   double *ex_loss, float *crtarget, float *cctarget, void *stream);

/* acc[0] += sum_e ex_loss[e][0]; acc[1] += sum_e ex_loss[e][1] (device fp64; the Lua accumulators
 * cls_loss / reg_loss of objective.lua:52).  The order of the sum is FIXED but is not example order: 64 partial sums
 * (partial k: examples k, k + 64, ... in that order), folded pairwise (k with k + 32, then + 16, ... + 1), and the total added
 * to acc last.  Two runs give the same bits; the result is within E * 2^-53 * (|acc| + sum_e |ex_loss[e]|) of the exact sum.
 * E <= 0: no launch, acc is not touched. */
int frcnn_loss_accumulate(const double *ex_loss, int E, double *acc, void *stream);

/* ---- nn.Linear (models/model_utilities.lua:82,99,103) -------------------------------- */
/* The products of one layer exactly as the classification net runs them (both run csrc/linear.h): fp32, or at large shapes
 * three bf16 planes or, with option x3_f16, two fp16 planes; FRCNN_GEMM_F16=0 / FRCNN_GEMM_WGRAD_F16=0 hold here as there.
 * Scratch for the requested roles is allocated and freed by the call; a call that took a split form synchronises the stream. */
int frcnn_linear_forward(const float *x, int R, int I, const float *weight, const float *bias,
                         int O, float *y, void *stream);
/* gx (may be NULL) = gy W ; gweight += gy^T x ; gbias += colsum(gy) (either may be NULL) */
int frcnn_linear_backward(const float *x, const float *gy, int R, int I, const float *weight,
                          int O, float *gx, float *gweight, float *gbias, void *stream);

/* ---- optim.rmsprop (main.lua:122,133): m = a*m + (1-a)*g^2 ; x -= lr*g/(sqrt(m)+eps) -- */
int frcnn_rmsprop(float *x, const float *g, float *m, long long n, float lr, float alpha,
                  float eps, void *stream);
/* frcnn_scale(g, n, gscale) followed by frcnn_rmsprop in ONE pass over the flat vectors: gradient:div(n)
 * (objective.lua:200) folded into the optimiser step that follows it in main.lua:133.  g holds the scaled
 * gradient afterwards, exactly as after the two separate calls (gscale = 1: the gradient is left unscaled). */
int frcnn_scale_rmsprop(float *x, float *g, float gscale, float *m, long long n, float lr, float alpha,
                        float eps, void *stream);
/* The same with the divisor read from the device: gscale = 1 / *gcount_dev (a count of 0 leaves g unscaled).  For the
 * data-parallel step, where objective.lua:200's cls_count is the all-reduced sum that frcnn_allreduce_f64 left in
 * the accumulator vector: the update is queued behind the exchange without any host read-back. */
int frcnn_scale_rmsprop_dev(float *x, float *g, const double *gcount_dev, float *m, long long n, float lr,
                            float alpha, float eps, void *stream);
/* frcnn_scale_rmsprop on elements [lo, hi) of the vectors only (x, g, m = the 16-byte aligned STARTS of the flat vectors; any
 * bounds; gscale = 1: the gradient is left unscaled): what main.lua:133 does to that slice, bit for bit.  See "the update beside
 * the backward pass" below. */
int frcnn_scale_rmsprop_slice(float *x, float *g, float gscale, float *m, long long lo, long long hi, float lr,
                              float alpha, float eps, void *stream);

/* ---- optim.sgd / optim.nag (main.lua:122-124 sgd_state / nag_state, main.lua:134-135 the calls beside optim.rmsprop) ----
 * One step of Torch's optim function on the flat vectors, every Lua statement one separately rounded fp32 operation.
 * x = weights, g = the gradient the objective returned, v = state.dfdx (the momentum vector, n floats).  The host keeps
 * state.evalCounter and computes clr = learningRate / (1 + evalCounter * learningRateDecay) in double.  `first`: state.dfdx
 * did not exist before this step (the kernel then creates its contents; v need not be initialised).  gradient:div(n)
 * (objective.lua:200) rides on the same pass as in frcnn_scale_rmsprop: g *= gscale first (gscale = 1: g unscaled), or
 * gscale = 1 / *gcount_dev read on the device when gcount_dev is not NULL (a count of 0 leaves g unscaled).  g is left holding
 * what Torch leaves in it.  x, g, v: 16-byte aligned.
 *
 * optim.sgd: g += wd*x (wd != 0); with mom != 0: v = g on the first step, else v = v*mom + one_minus_damp*g; then
 * g += mom*v (nesterov) and x += -clr*g, or x += -clr*v; with mom == 0: x += -clr*g, and v may be NULL.  nesterov needs
 * mom > 0 and a zero dampening (one_minus_damp == 1). */
int frcnn_sgd(float *x, float *g, float *v, long long n, float gscale, const double *gcount_dev, float clr, float wd,
              float mom, float one_minus_damp, int nesterov, int first, void *stream);
/* frcnn_sgd on elements [lo, hi) of the vectors only (x, g, v = the STARTS of the flat vectors; any bounds): what the
 * whole-vector call does to that slice, bit for bit -- the update beside the backward pass (below) for optim.sgd. */
int frcnn_sgd_slice(float *x, float *g, float *v, long long lo, long long hi, float gscale, float clr, float wd, float mom,
                    float one_minus_damp, int nesterov, int first, void *stream);
/* optim.nag after its look-ahead (frcnn_nag_lookahead) and opfunc: g += wd*x (wd != 0); v = 0 on the first step, else
 * v = v*mom; v += -clr*g; x += v.  mom > 0. */
int frcnn_nag(float *x, float *g, float *v, long long n, float gscale, const double *gcount_dev, float clr, float wd,
              float mom, int first, void *stream);
int frcnn_nag_slice(float *x, float *g, float *v, long long lo, long long hi, float gscale, float clr, float wd, float mom,
                    int first, void *stream);
/* The slice forms with the divisor read from the device (gscale = 1 / *gcount_dev, a count of 0 leaves g unscaled): what
 * frcnn_scale_rmsprop_dev / frcnn_sgd / frcnn_nag with that gcount_dev do to elements [lo, hi), bit for bit. */
int frcnn_scale_rmsprop_slice_dev(float *x, float *g, const double *gcount_dev, float *m, long long lo, long long hi,
                                  float lr, float alpha, float eps, void *stream);
int frcnn_sgd_slice_dev(float *x, float *g, float *v, long long lo, long long hi, const double *gcount_dev, float clr,
                        float wd, float mom, float one_minus_damp, int nesterov, int first, void *stream);
int frcnn_nag_slice_dev(float *x, float *g, float *v, long long lo, long long hi, const double *gcount_dev, float clr,
                        float wd, float mom, int first, void *stream);

/* ---- optim.adam (Torch's optim/adam.lua; not among main.lua's -opti values), with AdamW's decoupled weight decay beside it ----
 * One step on the flat vectors through the kernel of the three optimisers above, every Lua statement one separately rounded
 * fp32 operation.  x = weights, g = the gradient the objective returned, m = state.m, v = state.v (n floats each; the host
 * creates both as zeros, as Torch does, and every step reads and writes both: there is no first-step form).  The host keeps
 * state.t and computes in double, as Lua does: clr = learningRate / (1 + t * learningRateDecay) with the t from before the
 * increment, then with t + 1: step = clr * sqrt(1 - beta2^t) / (1 - beta1^t), Torch's stepSize.  The divisor of gradient:div
 * rides on the pass as in frcnn_sgd (gscale, or 1 / *gcount_dev when gcount_dev is not NULL; gscale = 1 or a count of 0: g
 * unscaled).  Per element, in this order:
 *   g += wd*x                                   (wd != 0: Torch's coupled L2 decay)
 *   m = m*beta1 + one_minus_beta1*g ;  v = v*beta2 + (one_minus_beta2*g)*g ;  denom = sqrt(v) + eps (not kept)
 *   x += -decay*x                               (decay != 0: AdamW, decay = clr * weightDecay; g, m and v never see it)
 *   x += (-step*m)/denom
 * step and decay arrive positive.  wd and decay exclude each other (both non-zero: an error).  g is left holding what Torch
 * leaves in it: written back only where it was scaled or wd != 0.  x, g, m, v: 16-byte aligned, none NULL.  Argument errors are
 * reported before anything is queued; an empty range succeeds and writes nothing. */
int frcnn_adam(float *x, float *g, float *m, float *v, long long n, float gscale, const double *gcount_dev, float step,
               float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float wd, float decay,
               void *stream);
/* frcnn_adam on elements [lo, hi) of the vectors only (x, g, m, v = the STARTS of the flat vectors; any bounds): what the
 * whole-vector call does to that slice, bit for bit -- staged training and the update beside the backward pass (below). */
int frcnn_adam_slice(float *x, float *g, float *m, float *v, long long lo, long long hi, float gscale, float step,
                     float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float wd, float decay,
                     void *stream);
/* The slice form with the divisor read from the device (not NULL): what frcnn_adam with that gcount_dev does to [lo, hi). */
int frcnn_adam_slice_dev(float *x, float *g, float *m, float *v, long long lo, long long hi, const double *gcount_dev,
                         float step, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                         float wd, float decay, void *stream);

/* ---- gradient-norm clipping and the non-finite-step guard (not in the reference: main.lua:133-135 applies whatever the pass
 * produced).  Queued between the pass (and the all-reduce, when data parallel) and the optimiser's update; off unless a host
 * asks for it.  g = the flat gradient, T = the trainable slices of the pass (ranges_host: nranges sorted, disjoint pairs
 * {lo, hi}, hi exclusive, any bounds, empty ones allowed, at most 16; NULL: the whole vector), D = the divisor of
 * gradient:div (objective.lua:200): *divisor_dev when that is not NULL (the all-reduced count), else `divisor` (positive; 1: nothing
 * to scale); a device count that is not positive counts as 1, as in the optimiser kernels.
 *   S     = sum over T of (double)g[i] * (double)g[i].  Each product is exact in fp64; the sum is taken in fp64 in a fixed
 *           order that depends on n and the slice bounds only (per-block partials, then one block folds them; no atomics):
 *           two calls on the same data give the same bits, and so do the ranks of a data-parallel step.
 *   norm  = sqrt(S) / D: the L2 norm of the gradient the optimiser is about to see.
 *   D'    = D * max(1, norm / clip_norm) in fp64, each operation correctly rounded; clip_norm <= 0: D' = D (norm recorded,
 *           nothing clipped).  A CLIPPED STEP IS the optimiser's existing update with the device divisor D':
 *           frcnn_scale_rmsprop_dev / frcnn_sgd / frcnn_nag / frcnn_adam (or their _slice_dev forms) handed record_dev + 2.
 *   S not finite (inf or NaN; fp32 values as large as 3e38 have finite squares in fp64): the step treats the gradient as zero --
 *           g is overwritten with zeros on T (untouched elsewhere), D' = D, skipped = 1.  optim.rmsprop then leaves x as it
 *           is and decays m; optim.sgd / optim.nag continue on their momentum (and weight decay) alone, and so does
 *           optim.adam on its moments m and v (and its weight decay, coupled or decoupled, if any).
 *   record_dev: double[4] = {S, norm, D', skipped} on the device; a host reads it when it reads its loss sums.
 * workspace: frcnn_grad_clip_workspace_bytes(n) bytes of device memory (the per-block partials).  Three launches on `stream`;
 * argument errors are reported before anything is queued. */
size_t frcnn_grad_clip_workspace_bytes(long long n);
int frcnn_grad_clip(float *g, long long n, const long long *ranges_host, int nranges, double divisor,
                    const double *divisor_dev, double clip_norm, double *record_dev, void *workspace,
                    size_t workspace_bytes, void *stream);

/* optim.nag's look-ahead, before opfunc is called (when state.dfdx exists): x += mom*v.  A host that holds a pack promise
 * (frcnn_pnet_refresh_packs below) withdraws it afterwards with frcnn_pnet_invalidate_packs: the weights have changed. */
int frcnn_nag_lookahead(float *x, const float *v, long long n, float mom, void *stream);
/* frcnn_nag_lookahead on elements [lo, hi) only (x, v = the STARTS of the vectors; any bounds): staged training
 * (frcnn_model_set_trainable) looks ahead on the trainable slices, a frozen slice keeps its weights. */
int frcnn_nag_lookahead_slice(float *x, const float *v, long long lo, long long hi, float mom, void *stream);

/* ---- model runtime: models/model_utilities.lua:3-136 --------------------------------- */
typedef struct {
  int nblocks;                      /* vgg_small.lua:5-10 `layers` */
  int filters[8], ksize[8], pad[8], conv_steps[8];
  float dropout[8];
  int nheads;                       /* vgg_small.lua:12-17 `anchor_nets` */
  int head_k[8], head_n[8], head_input[8]; /* head_input 1-based */
  int ncls;                         /* vgg_small.lua:19-22 `class_layers` */
  int cls_n[8], cls_bn[8];
  float cls_dropout[8];
  int class_count;                  /* cfg.class_count (excluding background) */
  int kh, kw;                       /* cfg.roi_pooling */
  int box_per_class;                /* cfg.box_head.per_class: the box head is a Linear(nf, 4 * class_count), one box per
                                       foreground class (frcnn_hip_box.h); 0: the reference's shared Linear(nf, 4) */
} frcnn_model_desc;

typedef struct frcnn_model frcnn_model;

int frcnn_model_create(const frcnn_model_desc *desc_host, frcnn_model **out_host);
int frcnn_model_destroy(frcnn_model *);
/* Flat parameter vector (utilities.lua:136-147): total and pnet-only element counts. */
int frcnn_model_param_count(const frcnn_model *, long long *total_host, long long *pnet_host);
/* Parameter table, one row per tensor in flat order: {offset, count, kind, aux}.
 * kind: 0 conv weight (aux = kW*kH*nOutputPlane, model_utilities.lua:63-64), 1 conv bias,
 * 2 PReLU slope, 3 Linear weight (aux = fan_in), 4 Linear bias (aux = fan_in),
 * 5 BatchNorm weight, 6 BatchNorm bias. */
int frcnn_model_param_table(const frcnn_model *, long long *table_host, int cap, int *n_host);
/* Localizer.lua:6-39 for output node i (1..nheads = anchor heads, nheads+1 = last feature map):
 * int[n][6] = {kW,kH,dW,dH,padW,padH}, input first. */
int frcnn_model_localizer_layers(const frcnn_model *, int output_index, int *layers_host, int cap,
                                 int *n_host);
/* Staged training (Faster R-CNN's 4-step alternating training, cfg.train of the objective).  frozen_blocks (0..nblocks): the
 * leading backbone blocks whose parameters stay fixed; heads = 0: the anchor nets are frozen AND the RPN losses' deltas are not
 * back-propagated; cnet = 0: the classification net is frozen (its stage is the host's to skip: the library is not called for
 * it).  Default 0, 1, 1: everything trainable, every entry point launch for launch as without the call.  Errors: frozen_blocks
 * out of range, heads = cnet = 0, no trainable parameter.  The training entry points honour it as follows, and never write a
 * frozen slice of `grad` (the caller zeroes the vector before the pass):
 *   frcnn_pnet_anchor_loss_begin  : heads = 0: the losses, crtarget, cctarget and acc as always; no anchor-net backward
 *   frcnn_pnet_backward_heads_begin: heads = 0: starts nothing
 *   frcnn_pnet_backward           : no anchor-net launch when heads = 0; otherwise an anchor net's parameter gradients, and its
 *                                   input gradient only when its input block is trainable.  The backbone chain stops at block
 *                                   frozen_blocks + 1, whose first convolution computes its weight gradient and no input
 *                                   gradient; no launch at all for the backbone when every block is frozen.  The waits below
 *                                   (frcnn_pnet_wait_block_gradients, _wait_block_done, _wait_heads_done, _wait_backward_begun)
 *                                   stay valid: a frozen block's events mark the start of the backbone's part of the pass.
 *   frcnn_cnet_backward           : every block frozen: the input-gradient chain's last product is not queued and gx is left
 *                                   unwritten (frcnn_roi_pool_backward has nothing to do then).
 * The optimiser entry points take ranges: a host restricts its update to the trainable slices itself. */
int frcnn_model_set_trainable(frcnn_model *, int frozen_blocks, int heads, int cnet);
int frcnn_model_get_trainable(const frcnn_model *, int *frozen_blocks_host, int *heads_host, int *cnet_host);

/* pnet:forward(img) (objective.lua:71, Detector.lua:33).  training!=0: SpatialDropout masks are
 * drop_masks_host[b] (device float[filters_b] of 0/1, for parity runs) or, when NULL, drawn on
 * device from `seed`.  training==0: x(1-p) (pnet:evaluate(), Detector.lua:31). */
int frcnn_pnet_forward(frcnn_model *, const float *weights, const float *img, int H, int W,
                       int training, const float *const *drop_masks_host, unsigned long long seed,
                       void *stream);
/* Training-mode pnet:forward (objective.lua:71) that leaves the anchor nets in flight on the library's side
 * stream: on return only outputs[nheads+1] (the last pooled map) is final in `stream` order, so the
 * fine-tuning stage (objective.lua:146-186) can start beside them.  outputs[1..nheads] are consumed by
 * frcnn_pnet_anchor_loss_begin; frcnn_pnet_backward (or the next forward) joins whatever is still running.
 * With the side stream off this is frcnn_pnet_forward(training=1). */
int frcnn_pnet_forward_async_heads(frcnn_model *, const float *weights, const float *img, int H, int W,
                                   const float *const *drop_masks_host, unsigned long long seed,
                                   void *stream);
/* outputs[i], i = 1..nheads+1; the buffers are owned by the model and reused by the next
 * forward (callers that keep results must copy: objective.lua:119). */
int frcnn_pnet_output(frcnn_model *, int i, float **ptr_host, int *C_host, int *H_host,
                      int *W_host);
/* Inspection of what the last forward pass left in HBM -- for parity tests, which hand the path's DISCRETE decisions
 * (max-pool window winners, PReLU branches) to the CPU restatement so that gradients can be compared at the strict
 * tolerance (oracle/frcnn_oracle.h orc_set_decisions).  The pointer stays owned by the model and valid until the next
 * forward pass of another image size.
 *   kind 0: pre-activation output of backbone convolution `index` (float [O][Ho][Wo]; model_utilities.lua:8).  A training pass
 *           with option "drop_compact" does not compute the output channels the block's SpatialDropout (:10-12) drops: they read 0
 *   kind 1: arg-max of block `index`'s 2x2 ceil-mode max pool (unsigned char [C][Hp][Wp], value dy*2+dx; :23)
 *   kind 2: pre-activation output of anchor net `index`'s k x k convolution (float [n][Ho][Wo]; :31)
 *   kind 3: input of classification layer `index`'s PReLU (float [R][n]; :85-86), after frcnn_cnet_forward
 *   kind 4: the nn.SpatialDropout scale vector of block `index` in the last pass (float [C]; a 0/1 keep vector while training)
 * Magnitude records (see frcnn_amax_record_floats; option "x3_f16") and the tensors they describe.  A record kind is an
 * error unless the LAST pass handed that record to the launch that writes it (a forward pass for kinds 5, 6 and 10, a
 * backward pass for kind 8): a layer whose consumer does not take the fp16 form, a frozen block, a pass that re-used
 * packs made earlier (weights) or option "x3_f16" off keep none.
 *   kind 5: record of backbone convolution `index`'s stored output -- the tensor of kind 0, except that a compact block
 *           (option "drop_compact") stores its first convolution's output compact: float [nkM][Ho][Wo], row i < nk = the i-th
 *           kept channel, rows nk..nkM-1 (padding to a multiple of 64) = 0; kind 7 returns that tensor as stored
 *   kind 6: record of block `index`'s pooled map; kind 9: that map (float [C][Hp][Wp])
 *   kind 7: backbone convolution `index`'s output as stored (kind 0 without the dense layout of a compact block)
 *   kind 8: after frcnn_pnet_backward, record of the finished gradient of convolution `index`'s output (through the
 *           pooling / activation backward); kind 11: that tensor (float [O][Ho][Wo]; compact as kind 7 in a compact block)
 *   kind 10: record of the weight tensor of backbone convolution `index` (index < number of backbone convolutions) or of
 *            anchor net index - that number's k x k convolution */
int frcnn_model_debug_buffer(frcnn_model *, int kind, int index, void **ptr_host, long long *bytes_host);
/* delta_outputs[i] (objective.lua:78-84): gradient buffers with the shapes of the outputs. */
int frcnn_pnet_delta(frcnn_model *, int i, float **ptr_host);
int frcnn_pnet_zero_deltas(frcnn_model *, void *stream);
/* Optional one-shot hint for the next frcnn_pnet_backward: delta_outputs[head] (head = 1..nheads) is
 * zero outside `count` positions (device int array of unique flat indices y*W_head + x, 0-based), which is
 * how objective.lua:91-134 fills it (only the sampled anchors).  The head's backward then runs on those
 * positions only; the result is identical.  count < 0 (default) or > 512: dense backward. */
int frcnn_pnet_set_sparse_deltas(frcnn_model *, int head, const int *positions, int count);
/* Optional early start of pnet:backward (objective.lua:189): once delta_outputs[1..nheads] are final (after
 * the anchor loop, objective.lua:91-140 -- the fine-tuning stage only adds into delta_outputs[nheads+1]),
 * the anchor-net part of the backward pass may begin on the library's side stream, beside the
 * classification network's forward/backward on `stream`.  frcnn_pnet_backward then joins it.  Without this
 * call frcnn_pnet_backward does everything itself; the result is the same. */
int frcnn_pnet_backward_heads_begin(frcnn_model *, const float *weights, float *grad, void *stream);
/* The anchor loop of objective.lua:91-140 on the model's own outputs[1..nheads] / delta_outputs[1..nheads]
 * (arguments as frcnn_rpn_loss + frcnn_loss_accumulate), followed by the anchor-net part of pnet:backward
 * (as frcnn_pnet_backward_heads_begin) -- all on the library's side stream, ordered after everything queued
 * on `stream` so far (example tables, zeroed delta buffers).  frcnn_pnet_anchor_loss_wait makes `stream` wait
 * until ex_loss / crtarget / cctarget / acc are final (needed before frcnn_cnet_losses, objective.lua:156);
 * frcnn_pnet_backward joins the rest.  With the side stream off the losses run on `stream` itself. */
int frcnn_pnet_anchor_loss_begin(frcnn_model *, const float *weights, float *grad, const int *ex_idx,
                                 const double *ex_anchor, const double *ex_roi, const int *ex_class,
                                 int npos, int nneg, int bgclass, double *ex_loss, float *crtarget,
                                 float *cctarget, double *acc, void *stream);
int frcnn_pnet_anchor_loss_wait(frcnn_model *, void *stream);
/* Makes `stream` wait for the anchor-net part started by frcnn_pnet_backward_heads_begin.  *joined_host = 1:
 * the anchor nets' slice of `grad` is final in stream order (e.g. for an early all-reduce of that slice beside
 * the remaining backward pass); 0: nothing had been started, frcnn_pnet_backward will compute that part. */
int frcnn_pnet_backward_heads_join(frcnn_model *, void *stream, int *joined_host);
/* pnet:backward(img, delta_outputs) (objective.lua:189): accumulates into the flat gradient.
 * The (unused) input gradient of the first convolution is not computed (nor anything for frozen parts of the model:
 * frcnn_model_set_trainable). */
int frcnn_pnet_backward(frcnn_model *, const float *weights, float *grad, void *stream);

/* After frcnn_pnet_backward has been queued: makes `stream` (any stream) wait until every gradient of backbone
 * block `block` (1-based; its convolutions' weights, biases and PReLU slopes -- a contiguous slice of the flat
 * vector) is final.  The deepest block finishes first, long before the call's own stream reaches the end of the
 * pass: a data-parallel caller starts that slice's all-reduce behind this wait, beside the remaining backward pass. */
int frcnn_pnet_wait_block_gradients(frcnn_model *, int block, void *stream);

/* ---- the update beside the backward pass (round 6): optim.rmsprop's step (main.lua:133) applied slice by slice ----------
 * main.lua:133 updates the whole flat vector after lossAndGradient (objective.lua:45-218) has returned, and the next
 * pnet:forward (objective.lua:71) re-packs every weight tensor before its first convolution: two serial stretches of a step
 * that is otherwise bound by the matrix cores.  Slices of the gradient are final long before the pass ends -- the classification
 * net's (55 % of the vector) after cnet:backward (objective.lua:179), the anchor nets' once their part of pnet:backward has
 * run, a backbone block's when the pass has left the block -- and the divisor of gradient:div (objective.lua:200) is a host
 * number known before the pass.  A host that owns the optimiser may therefore queue
 *     frcnn_scale_rmsprop_slice(x, g, 1/cls_count, m, lo, hi, ...)  [+ frcnn_pnet_refresh_packs(model, x, group, ...)]
 * on the UPDATE STREAM as each slice becomes final, and frcnn_model_update_join before anything reads the weights again.  The
 * result is bit-identical to frcnn_scale_rmsprop on the whole vector (same arithmetic per element, tests/test_gpu_eager.py).
 * frcnn_sgd_slice / frcnn_nag_slice do the same for optim.sgd / optim.nag (tests/test_gpu_optim.py).
 *   frcnn_model_update_stream : the library-owned stream for this work (the one the classification net's weight gradients
 *                               run on: a slice update queued there is ordered behind them by itself).  Call it BEFORE the pass
 *                               whose slices are to be updated: from then on the passes record the events the waits below
 *                               need (each a marker on the caller's stream, which a host that never asks does not pay for)
 *   frcnn_model_update_fork   : the update stream waits for everything queued on `stream` so far (the last readers of the
 *                               weights about to change, e.g. cnet:backward's input-gradient chain)
 *   frcnn_model_update_join   : `stream` waits for everything queued on the update stream so far
 *   frcnn_pnet_wait_backward_begun : after frcnn_pnet_backward has been queued: `stream` waits until the caller's stream has
 *                               joined the anchor nets and begun the backbone's backward pass (objective.lua:189) -- the
 *                               matrix-core-bound stretch of the step, beside which bandwidth-bound update work costs least
 *   frcnn_pnet_wait_heads_done: after frcnn_pnet_backward has been queued: `stream` waits until the anchor nets' backward pass is
 *                               over, parameter gradients included (they may run on beside the backbone's pass: the caller's
 *                               stream only waits for their contribution to the pooled maps' gradients before it starts)
 *   frcnn_pnet_wait_block_done: after frcnn_pnet_backward has been queued: `stream` waits until block `block` (1-based) may be
 *                               updated -- its gradients are final AND the last launch reading its weights, packs or weight
 *                               magnitudes has run (frcnn_pnet_wait_block_gradients only promises the first)
 *   frcnn_pnet_refresh_packs  : renews on `stream` the packed weight images / weight magnitudes of one owner (group = 0-based
 *                               backbone block, or nblocks for the anchor nets) from `weights`; when EVERY group has been
 *                               renewed from the vector the next training-mode frcnn_pnet_forward is given, that forward skips
 *                               its own re-pack.  The caller promises that between this call and that forward nothing writes
 *                               the weights except updates followed by their refresh; frcnn_pnet_invalidate_packs withdraws
 *                               the promise (a host that wrote the weights some other way calls it). */
int frcnn_model_update_stream(frcnn_model *, void **stream_host);
int frcnn_model_update_fork(frcnn_model *, void *stream);
int frcnn_model_update_join(frcnn_model *, void *stream);
int frcnn_pnet_wait_backward_begun(frcnn_model *, void *stream);
int frcnn_pnet_wait_heads_done(frcnn_model *, void *stream);
int frcnn_pnet_wait_block_done(frcnn_model *, int block, void *stream);
int frcnn_pnet_refresh_packs(frcnn_model *, const float *weights, int group, void *stream);
int frcnn_pnet_invalidate_packs(frcnn_model *);

/* cnet:forward(cinput) (objective.lua:164, Detector.lua:101).  weights/grad point at the START
 * of the flat vectors.  bn_running: float[2*n] {mean,var} per BatchNorm layer (updated when
 * training).  drop_masks_host[l]: device float[R][n_l] keep masks or NULL (seeded RNG). */
int frcnn_cnet_forward(frcnn_model *, const float *weights, const float *x, int R, int training,
                       const float *const *drop_masks_host, unsigned long long seed,
                       float *bn_running, float *bbox_out, float *cls_out, void *stream);
/* cnet:backward(cinput, {crdelta, ccdelta}) (objective.lua:179) -> gx [R][D]; gx is not written when every backbone block is
 * frozen (frcnn_model_set_trainable) */
/* cnet:backward.  The input gradient gx is final on `stream` in stream order; the weight gradients and bias sums it adds to
 * `grad` are queued on a library-owned stream beside that chain (option "cnet_wgrad_async", default 1) and are final on
 * `stream` after frcnn_pnet_backward, the next frcnn_cnet_forward, or frcnn_cnet_backward_join -- or after a device-wide
 * synchronisation.
 * LIFETIME: until one of those joins has been queued, the library-owned stream still READS caller-owned memory -- g_bbox,
 * g_cls, the `x` that was passed to frcnn_cnet_forward (first layer's weight gradient) -- and WRITES `grad`.  The caller
 * must neither modify nor free those buffers, nor let a stream-ordered allocator hand them out again, before the join
 * is queued on the stream that does so (a caching allocator: record the join's stream on the tensors, or hold references
 * until then).  frcnn_set_option("cnet_wgrad_async", 0) keeps everything on `stream` for a caller that cannot promise it. */
int frcnn_cnet_backward_join(frcnn_model *, void *stream);
int frcnn_cnet_backward(frcnn_model *, const float *weights, const float *g_bbox,
                        const float *g_cls, float *gx, float *grad, void *stream);
/* objective.lua:170-177: zero negative rows of crout, SmoothL1*10 and ClassNLL with gradients.
 * loss2 (device double[2]) += {creg_loss, ccls_loss}. */
int frcnn_cnet_losses(float *crout, const float *crtarget, const float *ccout,
                      const float *cctarget, int R, int npos, int ncls, float *crdelta,
                      float *ccdelta, double *loss2, void *stream);
/* Detector.lua:110-113: class (1-based argmax) and confidence (max log-prob) per row */
int frcnn_cnet_decode(const float *cls_out, int R, int ncls, int *cls, float *conf, void *stream);

/* ---- image preparation: BatchIterator:processImage (BatchIterator.lua:101-164) ----
 * The arithmetic the reference delegates to the torch `image` / `nn` packages, on a decoded float frame
 * [C][H][W] resident in device memory.  All calls are asynchronous on `stream`. */
/* image.rgb2yuv (utilities.lua load_image, color_space 'yuv'): rgb, yuv float[3][H][W] (may not alias). */
int frcnn_image_rgb2yuv(const float *rgb, float *yuv, int H, int W, void *stream);
/* image.rgb2hsv / image.rgb2lab (utilities.lua:212-215 load_image, color_space 'hsv' / 'lab'; main.lua:174-177): rgb in [0,1],
 * out float[3][H][W] (may not alias).  hsv: h in [0,1), s, v as image/generic/image.c computes them (h = s = 0 for a grey
 * pixel).  lab: sRGB gamma expansion, XYZ with the D65 white point, CIE L*a*b* (epsilon 216/24389, kappa 24389/27). */
int frcnn_image_rgb2hsv(const float *rgb, float *hsv, int H, int W, void *stream);
int frcnn_image_rgb2lab(const float *rgb, float *lab, int H, int W, void *stream);
/* image.scale(img, dW, dH), 'bilinear' (BatchIterator.lua:51): rows then columns; up-scaling interpolates
 * linearly, down-scaling averages the covered source interval.  tmp: device float[C*H*dW].
 * rgb2yuv != 0 (C == 3): src is the RGB frame and every source sample goes through image.rgb2yuv on the fly --
 * the result of frcnn_image_rgb2yuv followed by the scaling, without the full-resolution round trip. */
int frcnn_image_scale(const float *src, int C, int H, int W, float *dst, int dH, int dW, float *tmp,
                      int rgb2yuv, void *stream);
/* image.load(fn, 3, 'float') + (optionally) image.rgb2yuv + image.scale for a frame that is still the decoder's
 * 8-bit interleaved RGB [H][W][3] in device memory: samples are converted with v * (1/255) on the fly in the row
 * pass (6 MB instead of 25 MB per 1080p frame cross PCIe).  dst float[3][dH][dW]; tmp: device float[3*H*dW]. */
int frcnn_image_scale_u8(const unsigned char *src_hwc, int H, int W, float *dst, int dH, int dW,
                         float *tmp, int rgb2yuv, void *stream);
/* image.crop(img, x0, y0, x0+w, y0+h) followed by image.hflip / image.vflip when the flags are set
 * (BatchIterator.lua:57-80), one pass: dst float[C][h][w]. */
int frcnn_image_crop_flip(const float *src, int C, int H, int W, int x0, int y0, int w, int h, int hflip,
                          int vflip, float *dst, void *stream);
/* img[i]:add(-img[i]:mean()) for every channel (centering != 0), then img[i]:div(img[i]:std()) where
 * std > 1e-8 (scaling != 0), in place (BatchIterator.lua:146-160); mean and the unbiased standard deviation
 * accumulate in fp64 in a fixed order.  workspace: frcnn_image_normalize_workspace_bytes(C) device bytes. */
size_t frcnn_image_normalize_workspace_bytes(int C);
int frcnn_image_normalize(float *img, int C, int H, int W, int centering, int scaling, void *workspace,
                          size_t workspace_bytes, void *stream);
/* nn.SpatialContrastiveNormalization(1, kernel) on one plane (BatchIterator.lua:162, kernel =
 * image.gaussian1D(cfg.normalization.width)): subtractive then divisive normalisation with the 1-D kernel
 * (K odd, <= 15, host pointer) applied along x then y over a zero-padded plane, border-corrected by the
 * response to a plane of ones; threshold = thresval (1e-4 in the reference).  tmp: device float[H*W]. */
int frcnn_image_contrastive_norm(const float *in, int H, int W, const float *kernel_host, int K,
                                 float threshold, float *out, float *tmp, void *stream);

/* ---- example assembly on the host: Anchors.lua:69-235 + BatchIterator.lua:198-225 ----
 * Host-only native code (no device work), for loaders that must keep up with 200+ images/s per GPU.
 * frcnn_anchors_create: w_tab / h_tab = the fp32 tables of Anchors.lua:18-19 ([nscales][3][width][2]), cx / cy = the
 * anchor centres that key the 16-pixel bins of findNearby (double[nscales][3][width]); all host pointers. */
typedef struct frcnn_anchors frcnn_anchors;
int frcnn_anchors_create(const float *w_tab_host, const float *h_tab_host, const double *cx_host,
                         const double *cy_host, int nscales, int width, frcnn_anchors **out_host);
int frcnn_anchors_destroy(frcnn_anchors *);
/* One image of nextTraining: findPositive(rois, image, pos_thr, neg_thr, best_match), sampleNegative(image, rois,
 * neg_thr, negatives) and, when nearby_aversion != 0, the nearby anchors below neg_thr shuffled with shuffle_n
 * (min(#positive, #candidates) of them).  rois_host double[nroi][4].  Random draws come from the MT19937 state
 * mt_state_host[624] / *mt_index_host (torch.random's generator), updated in place.  Output, positives first:
 * ex_host int[cap][5] = {layer, aspect, y, x, roi (1-based; 0 for negatives)} 1-based, ex_rect_host double[cap][4]. */
int frcnn_anchors_assemble(frcnn_anchors *, const double *rois_host, int nroi, double img_w, double img_h,
                           double pos_thr, double neg_thr, int best_match, int nearby_aversion,
                           int negatives, unsigned int *mt_state_host, int *mt_index_host, int *ex_host,
                           double *ex_rect_host, int cap, int *npos_host, int *nneg_host);

/* ---- data-parallel exchange step: communicator + all-reduce (SURVEY 8b last row, 8e) --------------
 * Not in the reference (one process, one device: main.lua:52).  The training step shards over images; the ranks
 * meet once per step, between the last pnet:backward (objective.lua:189) and gradient:div(cls_count)
 * (objective.lua:197-200): sum of the flat gradient (frcnn_allreduce_f32) and of the 8 fp64 accumulators declared
 * at objective.lua:52-58 (frcnn_allreduce_f64), then every rank applies the identical optim.rmsprop step.
 * One process per GPU; the communicator runs RCCL (xGMI inside a node), bound at first use (dlopen "librccl.so.1").
 * Rendezvous: rank 0 creates a 128-byte id (frcnn_comm_get_unique_id) and hands it to the other ranks by any
 * host-side channel; frcnn_comm_init_rank_file does that through a file on a path every rank can see: rank 0 removes
 * whatever a previous job left there and writes {id, job nonce, its pid} atomically; the others poll up to timeout_ms
 * and accept a file only when its nonce equals theirs and (same host) its writer is still alive, so an id left
 * behind by a crashed job is never joined.  The nonce is the environment variable FRCNN_COMM_NONCE (any string
 * common to the ranks of ONE job, e.g. the launcher's pid and start time; default "0").
 * frcnn_comm_init_rank* is a collective call: every rank of the job makes it, after frcnn_set_device.
 * The all-reduces are IN PLACE sums, asynchronous on `stream`, ordered like any other work of that stream. */
#define FRCNN_COMM_ID_BYTES 128
typedef struct frcnn_comm frcnn_comm;
int frcnn_comm_get_unique_id(void *id_host);
int frcnn_comm_exchange_id_file(const char *path, int rank, void *id_host, int timeout_ms);   /* host only, no RCCL */
int frcnn_comm_init_rank(frcnn_comm **out_host, int nranks, int rank, const void *id_host);
/* The same under a watchdog: a peer that died between the rendezvous and this collective call surfaces as an error after
 * timeout_ms instead of a hang (non-blocking ncclCommInitRankConfig + ncclCommAbort where RCCL has them).
 * frcnn_comm_init_rank_file applies its timeout_ms to the file wait and to the initialisation.  Environment:
 * FRCNN_COMM_CHANNELS=n caps the channels (CUs) RCCL's kernels occupy beside the training step. */
int frcnn_comm_init_rank_timeout(frcnn_comm **out_host, int nranks, int rank, const void *id_host, int timeout_ms);
int frcnn_comm_init_rank_file(frcnn_comm **out_host, int nranks, int rank, const char *path, int timeout_ms);
int frcnn_comm_destroy(frcnn_comm *);
int frcnn_comm_info(const frcnn_comm *, int *nranks_host, int *rank_host);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): lets a bench
 * or a test assert that N ranks on N distinct devices really joined.  Any pointer may be NULL. */
int frcnn_comm_query(const frcnn_comm *, int *count_host, int *user_rank_host, int *device_host);
int frcnn_allreduce_f32(frcnn_comm *, float *buf, long long n, void *stream);
int frcnn_allreduce_f64(frcnn_comm *, double *buf, long long n, void *stream);
/* one-time weight broadcast after load_model / restore (main.lua:92-98) so that every replica starts identical */
int frcnn_broadcast_f32(frcnn_comm *, float *buf, long long n, int root, void *stream);

#ifdef __cplusplus
}
#endif

/* Online hard example mining for the classification net (cfg.roi_sampling.source = "hard"): its two entry points are declared,
 * with their semantics, in a header of their own; a host that includes this file gets them too. */
#include "frcnn_hip_hard.h"
/* The configurable losses of the classification net (cfg.cnet_loss): one entry point and its description, likewise. */
#include "frcnn_hip_loss.h"
/* Per-class box regression of the classification net (cfg.box_head): three entry points, likewise. */
#include "frcnn_hip_box.h"
/* The box of its own class for every row of the all-class class test (cfg.scoring.boxes = "class"): two entry points, likewise. */
#include "frcnn_hip_classbox.h"
/* Detections matched to ground truth on the device, for mean average precision (Detector:match_batch): two entry points, likewise. */
#include "frcnn_hip_eval.h"
/* The anchor nets' sparse training chain, its grouped product and position helpers without a model: test-facing, likewise. */
#include "frcnn_hip_heads.h"
/* The launches of a channel-compact dropout block without a model (gathered packs, mapped folds): test-facing, likewise. */
#include "frcnn_hip_compact.h"
#endif /* FRCNN_HIP_H */
