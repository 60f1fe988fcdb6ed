// roi_hard.hip -- online hard example mining for the classification net (cfg.roi_sampling.source = "hard"; Shrivastava, Gupta,
// Girshick 2016; not in the reference): every labelled candidate of a frame is scored by the current net, the library's own NMS
// (frcnn_nms_device_batch keyed by the loss) removes the near-duplicates among them, and the `batch` survivors of largest loss
// become the rows the net is trained on.  The two kernels here stand on either side of that NMS.
// Semantics: include/frcnn_hip_hard.h (frcnn_roi_hard_keys_batch, frcnn_roi_hard_gather_batch).
//   roi_hard_keys_batch_kernel    one thread a row: the row's loss (the per-row terms of cnet_losses_kernel, cnet.hip, in fp32) and
//                                 the NMS's row {x1, y1, x2, y2, loss}.  A streaming kernel of at most 4096 rows a segment, ~100 bytes
//                                 a row: it is bound by its launch, not by memory or arithmetic.
//   roi_hard_gather_batch_kernel  one workgroup a segment: the first `batch` picks set a byte flag per row in LDS (distinct picks:
//                                 distinct bytes, plain stores), and the flagged rows leave in ascending row order through the ballot +
//                                 one-wave scan compaction of proposal_targets.hip.
// No atomics, no workspace: a segment's result is a function of its own data.  FMA contraction is off for this translation unit:
// every fp32 operation of the loss is rounded on its own.
#pragma clang fp contract(off)
#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace frcnn {

#define RH_THREADS 1024
#define RH_TILES 4
#define RH_WAVES (RH_THREADS / 64)
#define RH_KEY_THREADS 256
constexpr int RH_MAX_N = RH_THREADS * RH_TILES;   // rows a segment: the candidates of frcnn_proposal_targets_batch
static_assert(RH_TILES * RH_WAVES == 64, "one wave scans the (tile, wave) counts");

__global__ __launch_bounds__(RH_KEY_THREADS) void roi_hard_keys_batch_kernel(
    const double* __restrict__ roi, const float* __restrict__ crout, const float* __restrict__ crtarget,
    const float* __restrict__ ccout, const float* __restrict__ cctarget, long long row_stride, int n_cap,
    const int* __restrict__ n_dev, const int* __restrict__ nfg_dev, int ncls, float* __restrict__ box5,
    float* __restrict__ loss) {
  __shared__ float s_box[RH_KEY_THREADS * 5];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(n_dev[b], 0), n_cap);
  const int r0 = blockIdx.x * RH_KEY_THREADS;
  if (r0 >= n) return;                                  // (the whole workgroup leaves)
  const int nfg = min(max(nfg_dev[b], 0), n);
  const size_t so = (size_t)b * (size_t)row_stride;
  const int r = r0 + tid;
  if (r < n) {
    const size_t o = so + (size_t)r;
    const double2* q = reinterpret_cast<const double2*>(roi + 4 * o);
    const double2 lo = q[0], hi = q[1];
    const float tf = cctarget[o];
    float l = -INFINITY;                                // a target outside 1 ... ncls: never ahead of a valid row, nothing is read
    if (tf >= 1.0f && tf <= (float)ncls) {              // (a NaN fails both)
      const int t = (int)tf - 1;
      const float cls = -ccout[o * (size_t)ncls + t];
      float reg = 0.0f;
      if (r < nfg) {
        const float4 y = *reinterpret_cast<const float4*>(crout + 4 * o);
        const float4 g = *reinterpret_cast<const float4*>(crtarget + 4 * o);
        const float z[4] = {y.x - g.x, y.y - g.y, y.z - g.z, y.w - g.w};
        float term[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float a = fabsf(z[k]);
          const float h = 0.5f * z[k];
          term[k] = a < 1.0f ? h * z[k] : a - 0.5f;
        }
        reg = term[0] + term[1];
        reg = reg + term[2];
        reg = reg + term[3];
        reg = reg * 10.0f;
      }
      l = cls + reg;
      if (l != l) l = INFINITY;                         // a diverged row is the hardest one, and the order stays total
    }
    loss[o] = l;
    float* sb = s_box + 5 * tid;                        // (a stride of 5 words: no bank conflict)
    sb[0] = (float)lo.x; sb[1] = (float)lo.y; sb[2] = (float)hi.x; sb[3] = (float)hi.y; sb[4] = l;
  }
  __syncthreads();
  // the workgroup's rows are 5 * rows consecutive floats of box5: five coalesced stores
  const int words = 5 * min(n - r0, RH_KEY_THREADS);
  float* out = box5 + 5 * (so + (size_t)r0);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int w = k * RH_KEY_THREADS + tid;
    if (w < words) out[w] = s_box[w];
  }
}

__global__ __launch_bounds__(RH_THREADS) void roi_hard_gather_batch_kernel(
    const long long* __restrict__ pick, const int* __restrict__ count_dev, int batch, const double* __restrict__ roi,
    const float* __restrict__ crtarget, const float* __restrict__ cctarget, const int* __restrict__ src,
    const int* __restrict__ gt_idx, const double* __restrict__ iou, const float* __restrict__ loss, long long row_stride,
    int n_cap, const int* __restrict__ n_dev, const int* __restrict__ nfg_dev, double* __restrict__ roi_out,
    float* __restrict__ crtarget_out, float* __restrict__ cctarget_out, int* __restrict__ src_out,
    int* __restrict__ gt_idx_out, double* __restrict__ iou_out, float* __restrict__ loss_out, int out_stride,
    int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned char s_flag[RH_MAX_N];   // row i is selected
  __shared__ int s_cnt[2][64];                                                // per (tile, wave): see the passes below
  __shared__ int s_tot[2];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(n_dev[b], 0), n_cap);
  const int cnt = min(max(count_dev[b], 0), n_cap);     // (the NMS leaves at most n picks; the list holds row_stride >= n_cap)
  if (n == 0) {                                         // (the whole workgroup leaves)
    if (tid == 0) *reinterpret_cast<int4*>(counts + 4 * (size_t)b) = make_int4(0, 0, cnt, 0);
    return;
  }
  const int nfg = min(max(nfg_dev[b], 0), n);
  const size_t si = (size_t)b * (size_t)row_stride, so = (size_t)b * (size_t)out_stride;
  pick += si;
  reinterpret_cast<unsigned int*>(s_flag)[tid] = 0u;    // RH_MAX_N bytes = RH_THREADS words

  // ---- 1. the picks in list order: a pick outside 1 ... n is skipped and does not count; the first `batch` of the others select
  long long p[RH_TILES];
  unsigned long long vmask[RH_TILES];
#pragma unroll
  for (int t = 0; t < RH_TILES; ++t) {
    const int k = t * RH_THREADS + tid;
    p[t] = k < cnt ? pick[k] : 0;
    vmask[t] = __ballot(p[t] >= 1 && p[t] <= (long long)n);
    if (lane == 0) s_cnt[0][t * RH_WAVES + wave] = __popcll(vmask[t]);
  }
  __syncthreads();
  if (wave == 0) {                                      // exclusive scan of the 64 (tile, wave) counts
    const int f = s_cnt[0][lane];
    int fi = f;
    for (int d = 1; d < 64; d <<= 1) {
      const int fu = __shfl_up(fi, d, 64);
      if (lane >= d) fi += fu;
    }
    s_cnt[0][lane] = fi - f;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int t = 0; t < RH_TILES; ++t) {
    if (p[t] >= 1 && p[t] <= (long long)n) {
      const int rank = s_cnt[0][t * RH_WAVES + wave] + __popcll(vmask[t] & below);
      if (rank < batch) s_flag[p[t] - 1] = 1;           // (distinct picks: distinct bytes; a repeated pick stores the same 1)
    }
  }
  __syncthreads();

  // ---- 2. ordered compaction: the selected foreground rows in row order, then the selected background rows
  bool sel[RH_TILES];
  unsigned long long fmask[RH_TILES], bmask[RH_TILES];
#pragma unroll
  for (int t = 0; t < RH_TILES; ++t) {
    const int i = t * RH_THREADS + tid;
    sel[t] = i < n && s_flag[i] != 0;
    fmask[t] = __ballot(sel[t] && i < nfg);
    bmask[t] = __ballot(sel[t] && i >= nfg);
    // (pass 1's offsets in s_cnt[0] were read in front of the barrier above)
    if (lane == 0) { s_cnt[0][t * RH_WAVES + wave] = __popcll(fmask[t]); s_cnt[1][t * RH_WAVES + wave] = __popcll(bmask[t]); }
  }
  __syncthreads();
  if (wave == 0) {
    const int f = s_cnt[0][lane], g = s_cnt[1][lane];
    int fi = f, gi = g;
    for (int d = 1; d < 64; d <<= 1) {
      const int fu = __shfl_up(fi, d, 64), gu = __shfl_up(gi, d, 64);
      if (lane >= d) { fi += fu; gi += gu; }
    }
    s_cnt[0][lane] = fi - f; s_cnt[1][lane] = gi - g;
    if (lane == 63) { s_tot[0] = fi; s_tot[1] = gi; }
  }
  __syncthreads();
  const int F = s_tot[0], Bq = s_tot[1];
#pragma unroll
  for (int t = 0; t < RH_TILES; ++t) {
    if (!sel[t]) continue;
    const int i = t * RH_THREADS + tid;
    const int j = i < nfg ? s_cnt[0][t * RH_WAVES + wave] + __popcll(fmask[t] & below)
                          : F + s_cnt[1][t * RH_WAVES + wave] + __popcll(bmask[t] & below);
    if (j >= out_stride) continue;                      // (F + Bq <= min(batch, n_cap) <= out_stride: checked by the launcher)
    const size_t a = si + (size_t)i, o = so + (size_t)j;
    const double2* ri = reinterpret_cast<const double2*>(roi + 4 * a);
    double2* ro = reinterpret_cast<double2*>(roi_out + 4 * o);
    ro[0] = ri[0]; ro[1] = ri[1];
    *reinterpret_cast<float4*>(crtarget_out + 4 * o) = *reinterpret_cast<const float4*>(crtarget + 4 * a);
    cctarget_out[o] = cctarget[a];
    src_out[o] = src[a];
    gt_idx_out[o] = gt_idx[a];
    iou_out[o] = iou[a];
    loss_out[o] = loss[a];
  }
  if (tid == 0) *reinterpret_cast<int4*>(counts + 4 * (size_t)b) = make_int4(F, Bq, cnt, n);
}

static bool misaligned16(const void* a, const void* b, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) != 0;
}

int roi_hard_keys_batch(const double* roi, const float* crout, const float* crtarget, const float* ccout, const float* cctarget,
                        int B, long long row_stride, int n_cap, const int* n_dev, const int* nfg_dev, int ncls, float* box5,
                        float* loss, hipStream_t s) {
  // everything is checked before the first launch: a refused call has written nothing
  FR_CHECK(B >= 0 && B <= 65535, "roi_hard_keys: %d segments (0 ... 65535)", B);
  if (B == 0) return FRCNN_OK;
  FR_CHECK(n_cap >= 0 && n_cap <= RH_MAX_N, "roi_hard_keys: n_cap %d (0 ... %d)", n_cap, RH_MAX_N);
  FR_CHECK(row_stride >= n_cap, "roi_hard_keys: row_stride %lld < n_cap %d", row_stride, n_cap);
  FR_CHECK(ncls >= 1, "roi_hard_keys: %d classes (at least 1)", ncls);
  FR_CHECK(n_dev && nfg_dev, "roi_hard_keys: NULL count");
  if (n_cap == 0) return FRCNN_OK;
  FR_CHECK(roi && crout && crtarget && ccout && cctarget && box5 && loss, "roi_hard_keys: NULL argument");
  FR_CHECK(!misaligned16(roi, crout, crtarget),
           "roi_hard_keys: roi, crout and crtarget are read 16 bytes at a time and must be 16-byte aligned");
  FR_LAUNCH(KC_RPN, (double)B * n_cap * 16.0, (double)B * n_cap * 96.0, s, roi_hard_keys_batch_kernel,
            dim3((n_cap + RH_KEY_THREADS - 1) / RH_KEY_THREADS, B), dim3(RH_KEY_THREADS), 0, roi, crout, crtarget, ccout, cctarget,
            row_stride, n_cap, n_dev, nfg_dev, ncls, box5, loss);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

int roi_hard_gather_batch(const long long* pick, const int* count_dev, int batch, const double* roi, const float* crtarget,
                          const float* cctarget, const int* src, const int* gt_idx, const double* iou, const float* loss, int B,
                          long long row_stride, int n_cap, const int* n_dev, const int* nfg_dev, double* roi_out,
                          float* crtarget_out, float* cctarget_out, int* src_out, int* gt_idx_out, double* iou_out,
                          float* loss_out, int out_stride, int* counts, hipStream_t s) {
  FR_CHECK(B >= 0 && B <= 65535, "roi_hard_gather: %d segments (0 ... 65535)", B);
  if (B == 0) return FRCNN_OK;
  FR_CHECK(n_cap >= 0 && n_cap <= RH_MAX_N, "roi_hard_gather: n_cap %d (0 ... %d)", n_cap, RH_MAX_N);
  FR_CHECK(row_stride >= n_cap, "roi_hard_gather: row_stride %lld < n_cap %d", row_stride, n_cap);
  FR_CHECK(batch >= 1, "roi_hard_gather: batch %d (at least 1)", batch);
  FR_CHECK(out_stride >= std::min(batch, n_cap), "roi_hard_gather: out_stride %d < min(batch %d, n_cap %d)", out_stride, batch,
           n_cap);
  FR_CHECK(count_dev && n_dev && nfg_dev && counts, "roi_hard_gather: NULL count");
  FR_CHECK(n_cap == 0 || (pick && roi && crtarget && cctarget && src && gt_idx && iou && loss && roi_out && crtarget_out &&
                          cctarget_out && src_out && gt_idx_out && iou_out && loss_out),
           "roi_hard_gather: NULL argument");
  FR_CHECK(!misaligned16(roi, crtarget) && !misaligned16(roi_out, crtarget_out, counts),
           "roi_hard_gather: roi, crtarget, their outputs and counts move 16 bytes at a time and must be 16-byte aligned");
  FR_LAUNCH(KC_RPN, 0, (double)B * (n_cap * 9.0 + std::min(batch, n_cap) * 136.0), s, roi_hard_gather_batch_kernel, dim3(B),
            dim3(RH_THREADS), 0, pick, count_dev, batch, roi, crtarget, cctarget, src, gt_idx, iou, loss, row_stride, n_cap, n_dev,
            nfg_dev, roi_out, crtarget_out, cctarget_out, src_out, gt_idx_out, iou_out, loss_out, out_stride, counts);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
