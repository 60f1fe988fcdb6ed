/*
 * frcnn_hip_compact.h -- the part of libfrcnn_hip.so's C ABI that makes the launches of a channel-compact dropout block
 * (option drop_compact; csrc/net.cpp plan_compact / pack_compact / wgrad_args) callable without a model: TEST-FACING entry
 * points.  A compact block computes only the filters its SpatialDropout keeps: the weight packs GATHER the kept filters /
 * channels out of the full weight tensor (PackXJob::oidx / cidx / Cs / bias_dst, csrc/convx.hip pack_x_job) and the folds of
 * the weight gradients SCATTER the compact result into the full gradient tensor (WgradMap, csrc/conv.hip
 * wgrad_reduce_map_kernel; the bias gradient follows the filter map inside csrc/wgradx.hip).  Included by frcnn_hip.h
 * (include that one); kept apart from it, like frcnn_hip_heads.h, so that frcnn_hip.h's own list of entry points stays the one
 * its hosts bind today.  The host mirror carries a ctypes table for this file (_lib.COMPACT_SIGS); tests/test_compact_plan.py
 * keeps the two in step.  bindings/frcnn_hip.lua has no cdef for it: a training host has no use for these calls.
 *
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.  Everything is fp32 and row-major, every convolution 3 x 3.  The entry points build
 * the job with conv_x3_pack_job and pack through conv_x3_pack_multi on a one-job device table (the launch a training step
 * packs with), then call conv_x3; the weight gradient calls conv_wgrad with a WgradMap: they carry no copy of a kernel.  Both
 * operand forms run (option x3_f16: two fp16 planes / three bf16 planes); all need option split_bf16 = 1.  The calls
 * synchronise the stream before they return.
 *
 * The tables.  oidx[nO] / cidx[nC] (gather) and omap[O] / cmap[Cin] (scatter) are device tables of int.  Entry i names the
 * filter / channel of the FULL tensor that filter / channel i of the launch stands for; a NEGATIVE entry is padding: a filter
 * / channel of zeros in a gather, nothing written in a scatter.  A NULL table is the identity (the launch's size must then
 * fit the full tensor's); with both gather tables NULL the launch is the first nO filters by the first nC channels of the full
 * tensor, read at its row pitch C_full like any other gather.  The non-negative entries of a scatter table are DISTINCT:
 * nothing checks that, two entries naming the same filter / channel would add to the same elements in no order.  Every
 * table is read back and an entry at or beyond the full tensor's size is refused.
 */
#ifndef FRCNN_HIP_COMPACT_H
#define FRCNN_HIP_COMPACT_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the gathered convolution, forward ----------------------------------------------------------------------------------------
 * out[nO][Ho][Wo] = conv(act(in)[nC][H][W], Wg) + bg, Ho = H + 2 pad - 2, where Wg[o'][c'] = weight[oidx[o']][cidx[c']] (the
 * 3 x 3 taps; zeros where either entry is negative) and bg[o'] = bias[oidx[o']] (0 for a negative entry; bias may be NULL: no
 * bias).  weight is the FULL tensor [O_full][C_full][3][3] (C_full becomes PackXJob::Cs, the source row pitch), bias the full
 * [O_full].  act = in_scale[c'] prelu(., *in_slope) where the pointers are non-NULL, as frcnn_conv2d_forward has it.  The
 * launch reads nC channels of `in`: further channels of a larger tensor are not touched.
 * Fp16 form: the packed weights are scaled by the largest magnitude of the FULL weight tensor, as in a training step
 * (net.cpp pack_compact: g.amax = j.amax), not by that of the gathered part.  rec_in (may be NULL: taken here) and rec_out (may
 * be NULL) are the magnitude records of frcnn_conv2d_forward_rec; both must be NULL in the three-plane form.
 * Written: the nO Ho Wo elements of out (rows of a negative oidx entry without a bias: exactly +0) and rec_out.
 * Refused before anything is launched: a NULL in / weight / out, sizes below 1, a shape for which conv_x3_eligible(nC, nO, 3)
 * fails (nC a multiple of 16, nO of 64, split_bf16 on), an empty output map, an identity table larger than the tensor, a table
 * entry out of range, a record in the three-plane form, an in_scale entry above 1 with a record. */
int frcnn_conv2d_forward_gathered(const float *in, int H, int W, const float *in_slope, const float *in_scale, const float *weight,
                                  const float *bias, int O_full, int C_full, const int *oidx, int nO, const int *cidx, int nC,
                                  int pad, float *out, const float *rec_in, float *rec_out, void *stream);

/* ---- the gathered convolution, input gradient (the pack's mode 1) ------------------------------------------------------------------
 * gin[nC][H][W] (= | +=) sum over o' of flip(Wg[o'][c']) applied to gout[o'][Ho][Wo], H = Ho - 2 pad + 2, pad the padding of the
 * FORWARD convolution, Wg as above.  The launch has K = nO channels and M = nC filters: conv_x3_eligible(nO, nC, 3) must hold
 * (nO a multiple of 16, nC of 64).  It reads nO channels of gout.  accumulate, rec_g, rec_out, post_x, post_slope, post_scale and
 * gslope are those of frcnn_conv2d_backward_input_rec: the fused activation backward gin = prelu'(post_x) post_scale[c'] (...),
 * *gslope += the sum over post_x <= 0 of post_x post_scale[c'] (...), post_x[nC][H][W], belongs to a storing launch with a
 * slope; it runs in both operand forms.  Records as above.
 * Written: the nC H W elements of gin (rows of a negative cidx entry of a storing launch: exactly +0, also behind the
 * activation backward; such rows add exactly 0 to *gslope), rec_out, *gslope.
 * Refused before anything is launched: as above, and the activation arguments frcnn_conv2d_backward_input_rec refuses. */
int frcnn_conv2d_backward_input_gathered(const float *gout, int Ho, int Wo, const float *weight, int O_full, int C_full,
                                         const int *oidx, int nO, const int *cidx, int nC, int pad, float *gin, int accumulate,
                                         const float *rec_g, float *rec_out, const float *post_x, const float *post_slope,
                                         const float *post_scale, float *gslope, void *stream);

/* ---- the mapped weight gradient ------------------------------------------------------------------------------------------------
 * The weight gradient of O gathered filters by Cin gathered channels, gw'[o'][c'] = sum over pixels of gout[o'] act(in)[c']
 * (in[Cin][H][W], gout[O][Ho][Wo], act as in frcnn_conv2d_backward_weight), ADDED into the full tensor:
 * gweight[omap[o']][cmap[c']] += gw'[o'][c'] for the pairs with two non-negative entries, gweight being [O_full][Cfull][3][3];
 * gbias[omap[o']] += sum over pixels of gout[o'] (gbias [O_full], may be NULL).  The magnitude records of the fp16 form are
 * taken inside the call, as frcnn_conv2d_backward_weight takes them.  The fold states the summation order of the unmapped
 * fold: each element receives the same bits as frcnn_conv2d_backward_weight on the compact tensors gives.
 * Written: the named elements.  Untouched: every filter / channel of gweight and gbias that no non-negative entry names.
 * Refused before anything is launched: a NULL in / gout / gweight, a shape that conv_wgradx does not take (Cin and O multiples
 * of 64, split_bf16 on), an empty map, Cfull or O_full below 1, two NULL tables with Cfull != Cin, an identity table larger
 * than the tensor, a table entry out of range. */
int frcnn_conv2d_backward_weight_mapped(const float *in, int Cin, int H, int W, const float *in_slope, const float *in_scale,
                                        const float *gout, int O, int pad, float *gweight, float *gbias, int O_full, int Cfull,
                                        const int *omap, const int *cmap, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_COMPACT_H */
