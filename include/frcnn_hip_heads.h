/*
 * frcnn_hip_heads.h -- the part of libfrcnn_hip.so's C ABI that makes the anchor nets' sparse training chain (csrc/heads.hip),
 * the grouped product it launches (csrc/gemm.hip gemm_f32_group) and the per-net position helpers of csrc/elem.hip callable
 * without a model: TEST-FACING entry points.  Included by frcnn_hip.h (include that one); kept apart from it, like
 * frcnn_hip_hard.h, so that frcnn_hip.h's own list of entry points stays the one its hosts bind today.  The host mirror carries
 * a ctypes table for this file (_lib.HEADS_SIGS, structures _lib.GemmJob and _lib.HeadNet); tests/test_heads_plan.py keeps the
 * two in step.  bindings/frcnn_hip.lua has no cdef for it: a training host has no use for these calls.
 *
 * Conventions as in frcnn_hip.h: extern "C", device pointers unless a name ends in _host, FRCNN_OK or an FRCNN_ERR_* code,
 * `stream` a hipStream_t passed as void*.  Everything is fp32 and row-major.  The chain entry points run the very functions a
 * training step runs (heads_chain_forward / heads_chain_backward_input / heads_chain_backward_params on a job table built by
 * heads_add_job, which also holds the K-split rule): they carry no copy of the chain.
 */
#ifndef FRCNN_HIP_HEADS_H
#define FRCNN_HIP_HEADS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the grouped product ------------------------------------------------------------------------------------------------------
 * n = 1 ... 4 independent products in ONE launch: C[M][N] (= | +=) A[M][K] B[K][N], element (m, k) of A at A[m sAm + k sAk],
 * (k, n) of B at B[k sBk + n sBn], (m, n) of C at C[m ldc + n], ldc >= N.  out_mode 0 stores, 1 adds to what C holds.
 * splits > 1: K is cut into `splits` runs of kPer = 32 ceil(ceil(K / splits) / 32) values and C receives the partial sums as
 * dense slabs [split][M][N] instead (ldc and out_mode are ignored; the caller folds them).
 * Every job of a launch is loaded with the orientation flags of job 0 (A k-contiguous: sAk == 1; B k-contiguous: sBk == 1).  The
 * flags only choose which index runs along a wave's lanes; the addresses use the strides, so any mix of strides is computed
 * correctly.  A job with M <= 0 or N <= 0 owns no block and writes nothing, wherever it stands in the group.
 * Written: the M x N elements of C (or the splits x M x N of the slabs) of every job with blocks.  Untouched: the padding
 * C[m ldc + N ... (m + 1) ldc), the operands, and everything of a job without blocks.
 * Refused before any launch: n outside 1 ... 4, a NULL table, K < 1, M or N < 0, out_mode outside {0, 1}, ldc < N of an
 * unsplit job, a NULL operand of a job that has blocks, splits that leave a run empty (K = 64 with 3 splits: runs of 32). */
typedef struct frcnn_gemm_job {
  const float *A; long long sAm, sAk;
  const float *B; long long sBk, sBn;
  float *C; long long ldc;
  int M, N, K, out_mode, splits;
} frcnn_gemm_job;
int frcnn_gemm_group(const frcnn_gemm_job *jobs_host, int n, void *stream);

/* ---- the chain ------------------------------------------------------------------------------------------------------------------
 * One anchor net: a k x k valid convolution of the input map in[Cin][H][W] to n filters (weights w3[n][Cin k k], bias3[n]), PReLU
 * with one slope, a 1 x 1 convolution to 18 planes (w1[18][n], bias1[18]); Ho = H - k + 1, Wo = W - k + 1, ckk = Cin k k.
 * pos[P]: the sampled positions, y Wo + x.  They are DISTINCT and lie inside the output map (0 <= pos < Ho Wo): nothing checks
 * that on the device, a position outside is an out-of-bounds access, and a duplicate would count its gradient twice (and make
 * the forward scatter write one element twice).
 * Scratch, owned by the caller, in floats: COL and DX P ckk each; HX, HY and GH n P each; OUT and D 18 P each; slab
 * splits n P, with slab_floats its capacity (the model gives every net n 4096).
 * force_splits = 0: the K splits of HX = w3 COL^T come from the planner the model uses (frcnn_heads_plan_splits); > 0: that
 * count instead.  Refused: a count whose runs of 32 ceil(ceil(ckk / splits) / 32) values leave one empty, and splits n P above
 * slab_floats (planned or forced).
 *
 * frcnn_heads_chain_forward, 5 launches whatever n is: COL[p][(c, ky, kx)] = in[c][y_p + ky][x_p + kx] | slab[s] = the partial
 * products of w3 COL^T | HX[c][p] = bias3[c] + the slabs in split order, HY = HX > 0 ? HX : slope HX | OUT[18][P] = w1 HY |
 * out[c][pos[p]] = OUT[c][p] + bias1[c].  Written: COL, slab, HX, HY, OUT and the P elements per plane of out[18][Ho Wo] at the
 * positions.  Untouched: every other element of out, DX, GH, D, every gradient (all of which may be NULL here).
 * splits_host (may be NULL): int[n], the split count of each net, 0 for a skipped one.
 *
 * frcnn_heads_chain_backward, after a forward on the same nets (reads COL, HX, HY): 7 launches, 5 when no net has a gin:
 * D[c][p] = delta[c][pos[p]], gbias1[c] += sum_p D | GH[n][P] = w1^T D | GH *= (HX > 0 ? 1 : slope), gbias3[c] += sum_p GH,
 * gslope += sum over HX <= 0 of HX (incoming GH) | for the nets with gin != NULL: DX[P][ckk] = GH^T w3, gin[c][y_p + ky][x_p + kx]
 * += DX (fp32 atomics) | gw1[18][n] += D HY^T | gw3[n][ckk] += GH COL.  Written: D, GH, DX (nets with a gin); ADDED to:
 * gbias1, gbias3, gslope, gw1, gw3 and the elements of gin under the k x k patches of the positions.  Untouched: gin outside the
 * patches, DX and gin of a net with gin == NULL (its parameter gradients are still computed), the forward's buffers.
 *
 * Both: n = 1 ... 4 nets.  A net with P <= 0 is SKIPPED by the job table: none of its buffers is read or written (its pointers
 * may be NULL), and the launches are those of the remaining nets; with no net left nothing is launched.
 * Refused before any launch: n outside 1 ... 4, P above 4096, k < 1, H or W below k, Cin or n < 1, a NULL pointer the pass needs
 * of a net with P > 0, and the split counts above.  Counted under FRCNN_KC_ELEMWISE and FRCNN_KC_GEMM. */
typedef struct frcnn_head_net {
  int Cin, H, W, k, n, P;
  int force_splits;
  const int *pos;
  const float *in; float *gin;
  const float *w3, *bias3, *slope, *w1, *bias1;
  float *gw3, *gbias3, *gslope, *gw1, *gbias1;
  float *out; const float *delta;
  float *COL, *HX, *HY, *OUT, *D, *GH, *DX, *slab;
  long long slab_floats;
} frcnn_head_net;
int frcnn_heads_chain_forward(const frcnn_head_net *nets_host, int n, int *splits_host, void *stream);
int frcnn_heads_chain_backward(const frcnn_head_net *nets_host, int n, void *stream);
/* the planner: K splits of HX[n][P] = w3[n][ckk] COL[P][ckk]^T; n, ckk, P >= 1 (else 0) */
int frcnn_heads_plan_splits(int n, int ckk, int P);

/* ---- the per-net helpers (csrc/elem.hip): what backward_head's sparse branch runs in deterministic mode and whenever the pass
 * was not deferred.  pos as above; P <= 0 launches nothing.
 * frcnn_gather_positions: dst[c][p] = src[c][pos[p]] for c < C planes of hw elements; slope and dst_act both non-NULL: also
 * dst_act = dst > 0 ? dst : slope[0] dst.  Writes C P elements of dst (and dst_act).
 * frcnn_im2col_positions: col[p][(c, ky, kx)] = X[c][y_p + ky][x_p + kx], X[C][H][W], pos = y Wo + x.  Writes P C k k elements.
 * frcnn_col2im_positions_add: gX[c][y_p + ky][x_p + kx] += col[p][(c, ky, kx)].  Option "deterministic" = 0: one fp32 atomic per
 * entry, any order; = 1: one thread per element of gX adds the entries that land on it in position order into a register, then
 * adds that to gX once -- bit-identical run to run.  Elements of gX under no patch are untouched in both forms. */
int frcnn_gather_positions(const float *src, int C, long long hw, const int *pos, int P, float *dst, const float *slope,
                           float *dst_act, void *stream);
int frcnn_im2col_positions(const float *X, int C, int H, int W, int k, int Wo, const int *pos, int P, float *col, void *stream);
int frcnn_col2im_positions_add(const float *col, int C, int H, int W, int k, int Wo, const int *pos, int P, float *gX, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_HEADS_H */
