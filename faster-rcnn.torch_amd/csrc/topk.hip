// topk.hip -- the proposal layer's "keep the K best-scoring matches" in front of the first NMS of Detector:detect
// (not in the reference: Detector.lua:39-85 hands every match to nms()):
//  * topk_select     : per segment (frame) the K' = min(n, K) best-ranked rows of a score column, as ASCENDING 0-based row
//                      numbers -- the selected rows keep their scan order, so for K >= n the selection is the identity.
//                      Rank: the fp32 score compared as a value (-0 equals +0, a NaN ranks below everything), ties are broken
//                      by the lower scan row.  Exact and deterministic: a 4-pass radix select (8 bits a pass, most
//                      significant first) on the order-preserving integer image of the key finds the K'-th best image T and
//                      the number q of rows equal to T that belong to the set; an ordered ballot/prefix compaction then
//                      writes the rows with an image above T and the FIRST q rows equal to T.  Counts meet in integer LDS
//                      atomics only: the result depends on the data, not on the launch geometry or on timing.
//  * rpn_gather_rows : the match arrays of the selected rows (p, idx, rect, box) into compact arrays of the same layouts, plus
//                      box5 = {box, p} (the first NMS's input when it is keyed by the score) and the 1-based original rows.
// One workgroup per segment, the segment on a grid dimension as in nms_device_batch: 45 015 keys are 180 KB, five passes over
// them out of the L2 -- latency-bound work of a few tens of microseconds, not HBM-bound.  No MFMA: compare / count / gather.
#include "kernels.h"

namespace frcnn {

#define TOPK_THREADS 1024
#define TOPK_WAVES (TOPK_THREADS / 64)

// a < b as fp32 values  <=>  image(a) < image(b) as unsigned; image(-0) == image(+0); every NaN -> 0, below image(-inf)
__device__ __forceinline__ unsigned topk_image(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// hist[d] += 1 for every active lane (d = the lane's digit).  The scores of a frame crowd into a few digits (log-probabilities
// in (log 0.95, 0]; a saturated log-softmax gives thousands of exact zeros), and 64 LDS atomics on one address take 64 turns:
// up to four rounds in which the lanes that share the first active lane's digit are counted by a ballot and added once, plain
// atomics for whatever is left.  Called from wave-uniform control flow.
__device__ __forceinline__ void topk_count(unsigned* hist, bool act, unsigned d, int lane) {
  for (int r = 0; r < 4; ++r) {
    const unsigned long long am = __ballot(act);
    if (!am) return;
    const int leader = __ffsll((long long)am) - 1;
    const unsigned d0 = (unsigned)__shfl((int)d, leader, 64);
    const unsigned long long same = __ballot(act && d == d0);
    if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(same));
    if (d == d0) act = false;
  }
  if (act) atomicAdd(&hist[d], 1u);
}

// score: segment b's keys at score + b * stride, n_b = min(n_dev[b], n_cap) of them; sel_row + b * sel_stride receives the K'
// selected rows (ascending), k_dev[b] = K'.  img: n_cap words per segment (the keys' images, written in the first pass; every
// thread reads back only what it wrote itself).  A segment of count 0 writes k_dev[b] = 0 and nothing else; no segment stores
// outside [0, K') of its slice.
__global__ __launch_bounds__(TOPK_THREADS) void topk_select_kernel(const float* __restrict__ score, long stride, int n_cap,
                                                                   const int* __restrict__ n_dev, int K, int* __restrict__ sel_row,
                                                                   long sel_stride, int* __restrict__ k_dev,
                                                                   unsigned* __restrict__ img_ws) {
  __shared__ unsigned hist[256];
  __shared__ int wtot[4];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_remaining;
  __shared__ int wave_g[TOPK_WAVES], wave_e[TOPK_WAVES];
  __shared__ int base_g, base_e;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = max(min(n_dev[b], n_cap), 0);
  const int Kp = min(n, K);
  if (n == 0) {
    if (tid == 0) k_dev[b] = 0;
    return;
  }
  const float* sc = score + (size_t)b * stride;
  int* out = sel_row + (size_t)b * sel_stride;
  if (Kp == n) {   // nothing to leave out: the identity, without a look at the keys
    for (int i = tid; i < n; i += TOPK_THREADS) out[i] = i;
    if (tid == 0) k_dev[b] = n;
    return;
  }
  unsigned* img = img_ws + (size_t)b * n_cap;
  // ---- radix select: after pass q the top 8 (q + 1) bits of T are known, `remaining` = rank of T among the keys that share them
  unsigned prefix = 0u;
  int remaining = Kp;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass ? (0xffffffffu << (shift + 8)) : 0u;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += TOPK_THREADS) {   // (uniform trip count: topk_count holds ballots)
      const int i = i0 + tid;
      unsigned m = 0u;
      if (i < n) {
        if (pass == 0) { m = topk_image(sc[i]); img[i] = m; }
        else m = img[i];
      }
      topk_count(hist, i < n && (m & himask) == prefix, (m >> shift) & 255u, lane);
    }
    __syncthreads();
    // digits in DESCENDING order over threads 0..255: inclusive prefix counts, the digit where they reach `remaining`
    int own = 0, incl = 0;
    if (tid < 256) {
      own = (int)hist[255 - tid];
      incl = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) wtot[wave] = incl;
    }
    __syncthreads();
    if (tid < 256) {
      for (int w = 0; w < wave; ++w) incl += wtot[w];
      if (incl >= remaining && incl - own < remaining) {   // (exactly one thread: 1 <= remaining <= the keys counted)
        sh_prefix = prefix | ((unsigned)(255 - tid) << shift);
        sh_remaining = remaining - (incl - own);
      }
    }
    __syncthreads();
    prefix = sh_prefix;
    remaining = sh_remaining;
  }
  // ---- ordered compaction: rows above T, and the first `quota` rows equal to T; #{above} + quota = K'
  const unsigned T = prefix;
  const int quota = remaining;
  if (tid == 0) { base_g = 0; base_e = 0; }
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += TOPK_THREADS) {
    const int i = i0 + tid;
    const unsigned m = i < n ? img[i] : 0u;
    const bool gt = i < n && m > T, eq = i < n && m == T;
    const unsigned long long bg = __ballot(gt), be = __ballot(eq);
    if (lane == 0) { wave_g[wave] = __popcll(bg); wave_e[wave] = __popcll(be); }
    __syncthreads();
    int g = base_g, e = base_e;
    for (int w = 0; w < wave; ++w) { g += wave_g[w]; e += wave_e[w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    g += __popcll(bg & below);
    e += __popcll(be & below);
    if (gt || (eq && e < quota)) out[g + min(e, quota)] = i;   // (< #{above} + quota = K')
    __syncthreads();
    if (tid == 0) {
      int sg = 0, se = 0;
      for (int w = 0; w < TOPK_WAVES; ++w) { sg += wave_g[w]; se += wave_e[w]; }
      base_g += sg; base_e += se;
    }
    __syncthreads();
  }
  if (tid == 0) k_dev[b] = Kp;
}

size_t topk_select_workspace_bytes(int B, int n_cap) {
  if (B <= 0 || n_cap <= 0) return 256;
  return 256 + (size_t)B * n_cap * 4;
}

int topk_select(const float* score, int B, long stride, int n_cap, const int* n_dev, int K, int* sel_row, long sel_stride,
                int* k_dev, void* ws, size_t ws_bytes, hipStream_t s) {
  if (B <= 0) return FRCNN_OK;
  FR_CHECK(k_dev && n_dev, "topk_select: NULL device counts");
  FR_CHECK(B <= 65535, "topk_select: %d segments (at most 65535)", B);
  FR_CHECK(K >= 1, "topk_select: K = %d (at least 1)", K);
  if (n_cap <= 0) {
    FR_HIP(hipMemsetAsync(k_dev, 0, sizeof(int) * (size_t)B, s));
    return FRCNN_OK;
  }
  FR_CHECK(score && sel_row, "topk_select: NULL argument");
  FR_CHECK(stride >= n_cap, "topk_select: stride %ld < %d rows per segment", stride, n_cap);
  FR_CHECK(sel_stride >= std::min(n_cap, K), "topk_select: sel_stride %ld < min(n_cap, K) = %d", sel_stride, std::min(n_cap, K));
  FR_CHECK(ws && ws_bytes >= topk_select_workspace_bytes(B, n_cap), "topk_select: workspace too small (%zu < %zu)", ws_bytes,
           topk_select_workspace_bytes(B, n_cap));
  unsigned* img = (unsigned*)(((uintptr_t)ws + 255) / 256 * 256);
  FR_LAUNCH(KC_TOPK, 0, 20.0 * B * n_cap, s, topk_select_kernel, dim3(B), dim3(TOPK_THREADS), 0, score, stride, n_cap, n_dev, K,
            sel_row, sel_stride, k_dev, img);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// Row j < min(k_dev[b], k_cap) of segment b: source row r = sel_row[b * sel_stride + j] (sel_row NULL: r = j) of the match
// arrays (src_stride rows per segment, rows >= src_rows are never read) -> row j of the destinations (dst_stride rows per
// segment; any of them may be NULL): p, idx[4], rect[4] (double), box[4], box5 = {box, p}, row = r + 1.
__global__ void rpn_gather_rows_kernel(const float* __restrict__ p, const int4* __restrict__ idx, const double2* __restrict__ rect,
                                       const float4* __restrict__ box, long src_stride, int src_rows,
                                       const int* __restrict__ sel_row, long sel_stride, const int* __restrict__ k_dev, int k_cap,
                                       float* __restrict__ dst_p, int4* __restrict__ dst_idx, double2* __restrict__ dst_rect,
                                       float4* __restrict__ dst_box, float* __restrict__ box5, int* __restrict__ row,
                                       long dst_stride) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(k_dev[b], k_cap)) return;
  const int r = sel_row ? sel_row[(size_t)b * sel_stride + j] : j;
  if ((unsigned)r >= (unsigned)src_rows) return;
  const size_t so = (size_t)b * src_stride + r, d = (size_t)b * dst_stride + j;
  const float pv = p[so];
  const float4 bx = box[so];
  if (dst_p) dst_p[d] = pv;
  if (dst_idx) dst_idx[d] = idx[so];
  if (dst_rect) { dst_rect[2 * d] = rect[2 * so]; dst_rect[2 * d + 1] = rect[2 * so + 1]; }
  if (dst_box) dst_box[d] = bx;
  if (box5) {
    float* o = box5 + 5 * d;
    o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w; o[4] = pv;
  }
  if (row) row[d] = r + 1;
}

int rpn_gather_rows(const float* p, const int* idx, const double* rect, const float* box, int B, long src_stride, int src_rows,
                    const int* sel_row, long sel_stride, const int* k_dev, int k_cap, float* dst_p, int* dst_idx,
                    double* dst_rect, float* dst_box, float* box5, int* row, long dst_stride, hipStream_t s) {
  if (B <= 0 || k_cap <= 0) return FRCNN_OK;
  FR_CHECK(B <= 65535, "rpn_gather_rows: %d segments (at most 65535)", B);
  FR_CHECK(p && box && k_dev, "rpn_gather_rows: NULL argument");
  FR_CHECK((!dst_idx || idx) && (!dst_rect || rect), "rpn_gather_rows: a destination without its source");
  FR_CHECK(src_rows >= 0 && src_stride >= src_rows, "rpn_gather_rows: src_stride %ld < %d source rows", src_stride, src_rows);
  FR_CHECK(dst_stride >= k_cap, "rpn_gather_rows: dst_stride %ld < %d rows per segment", dst_stride, k_cap);
  FR_CHECK(!sel_row || sel_stride >= k_cap, "rpn_gather_rows: sel_stride %ld < %d rows per segment", sel_stride, k_cap);
  FR_CHECK(sel_row || src_rows >= k_cap, "rpn_gather_rows: %d source rows < %d rows per segment", src_rows, k_cap);
  FR_LAUNCH(KC_TOPK, 0, 136.0 * B * k_cap, s, rpn_gather_rows_kernel, dim3(cdiv(k_cap, 256), B), dim3(256), 0, p,
            reinterpret_cast<const int4*>(idx), reinterpret_cast<const double2*>(rect), reinterpret_cast<const float4*>(box),
            src_stride, src_rows, sel_row, sel_stride, k_dev, k_cap, dst_p, reinterpret_cast<int4*>(dst_idx),
            reinterpret_cast<double2*>(dst_rect), reinterpret_cast<float4*>(dst_box), box5, row, dst_stride);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
