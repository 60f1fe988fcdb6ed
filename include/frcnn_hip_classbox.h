/*
 * frcnn_hip_classbox.h -- the part of libfrcnn_hip.so's C ABI that gives every row of the all-class class test the box of ITS class
 * (cfg.scoring.boxes = "class" on a per-class box head, cfg.box_head): entry points 148-149 of the library.  Included by
 * frcnn_hip.h (include that one); kept apart from it, like frcnn_hip_hard.h, frcnn_hip_loss.h and frcnn_hip_box.h, so that the
 * lists of entry points of the four other headers stay the ones their hosts bind today.  bindings/frcnn_hip.lua carries a fifth
 * generated cdef for this file, and the host mirror a fifth ctypes table (_lib.CLASSBOX_SIGS); tests/test_class_boxes_host.py
 * keeps them in step.
 */
#ifndef FRCNN_HIP_CLASSBOX_H
#define FRCNN_HIP_CLASSBOX_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Per-class boxes under all-class scoring (not in the reference; csrc/class_boxes.hip) --------------------------------------
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.
 *
 * frcnn_cnet_features copies the box head's input of the model's last frcnn_cnet_forward -- float[R][nf], R that pass's row
 * count, nf the last class layer's n (with an empty class-layer table: the caller's input, nf = the pooled row length) -- to dst
 * on `stream`: one device-to-device copy, no launch.  Errors: a NULL model, no forward pass yet, a NULL dst.
 */
int frcnn_cnet_features(frcnn_model *, float *dst, void *stream);

/* frcnn_detect_class_boxes_batch rewrites the boxes of the rows that frcnn_detect_classes_batch (mode 1) emitted for a chunk of
 * B frames.  Frame b's segment is rows b * row_stride ... of kc, keep_row, bb (5 floats a row) and r2 (4 doubles a row); the
 * frame's rows are j < min(K_dev[b], row_stride), K_dev read ON THE DEVICE (no host wait).  Its features are the rows
 * row0_host[b] ... of feat (float[.][nf]; row0_host: host values, passed by value to the kernel like those of
 * frcnn_detect_classes_batch), its match rows b * match_stride ... of rect (4 doubles a row) and pick (1-based rows of rect).
 * For row j, with r = keep_row[j] (the 0-based candidate) and c = kc[j] (the 1-based class):
 *   d[i]  = b[4 (c-1) + i] + sum_k feat[row0[b] + r][k] W[4 (c-1) + i][k], i = 0 ... 3: the arithmetic of frcnn_box_head_forward
 *           (frcnn_hip_box.h: fp32, 64 interleaved partial sums folded by a butterfly; 16-byte pieces where nf % 4 == 0 and feat
 *           and W are 16-byte aligned) -- bit for bit what that entry point gives for class c on that feature row, on arrays
 *           that take the same one of the two paths (the 16-byte pieces and the single floats sum in different orders; a model's
 *           own pass and this launch read the same W, and their feature arrays are both 16-byte aligned).  A class outside
 *           1 ... C is no class: d = 0, and nothing is read for it out of range;
 *   r2[j] = Anchors.anchorToInput(rect[pick[r] - 1], d) in double, every operation rounded on its own: the decode of
 *           frcnn_detect_post and frcnn_detect_classes_batch;  bb[j][0..3] = (float) r2[j].
 * bb[j][4] (the confidence), kc and keep_row are not touched; nothing is written at or behind row K_dev[b] of a segment, and a
 * frame with K_dev[b] = 0 writes nothing.  A row whose r is outside 0 ... match_stride - 1, or whose pick[r] is outside
 * 1 ... match_stride, is left as it is (never an index before it is checked).  W float[4 C][nf] and b float[4 C] are the per-class
 * box head's tensors (kinds 3 and 4 of frcnn_model_param_table in front of the class head's).
 * One launch per 64 frames, grid (row tiles, frames); one wave a row, four rows a workgroup: the rows of a candidate are adjacent
 * and share a feature row.  No atomics, no workspace: bit-reproducible run to run.
 * Errors, returned before any launch (a refused call has written nothing): B outside 0 ... 65535, nf < 1, C < 1,
 * 4 C nf >= 2^31, a negative stride; then -- B = 0 and row_stride = 0 return at once -- a NULL pointer, a pointer not aligned to
 * its element, a negative row0_host[b].  Counted under FRCNN_KC_ELEMWISE. */
int frcnn_detect_class_boxes_batch(const float *feat, int nf, const long long *row0_host, int B,
                                   const float *W, const float *b, int C,
                                   const double *rect, const long long *pick, long long match_stride,
                                   const int *kc, const int *keep_row, const int *K_dev, int row_stride,
                                   float *bb, double *r2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_CLASSBOX_H */
