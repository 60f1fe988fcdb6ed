// proposal_targets.hip -- the proposal-target layer between the first NMS and ROI pooling (cfg.roi_sampling, not in the
// reference): the candidates of a frame -- its ground-truth boxes (optional), then the first NMS's picks -- are matched to the
// ground truth, labelled foreground / background / ignored, thinned to a fixed-size batch at a fixed foreground share, and the
// survivors leave as the rect table, regression targets and class targets frcnn_roi_windows / RoIAlign / frcnn_cnet_losses read.
// Semantics: include/frcnn_hip.h (frcnn_proposal_targets_batch).
// One workgroup per segment, one launch, no atomics, no workspace: a segment's result is a function of its own data, its index
// and the seed.  A thread owns up to PT_TILES candidates (i = t * PT_THREADS + thread) and walks the <= 64 ground-truth boxes in
// LDS; every candidate's {label, key} lies in LDS as ONE 64-bit word (label in the high half: ignored 0 < foreground 1 <
// background 2), so that a row's rank within its class is the count of smaller words minus the rows of the classes in front of
// it -- one broadcast 16-byte LDS read and two 64-bit compares per pair of rows, walked only when a class exceeds its quota.
// The ordered compaction is a ballot per wave and one wave's scan over the (tile, wave) counts -- PT_TILES * 16 = 64 of them.
// fp64 arithmetic follows the host mirror (Rect.lua:126-141, Anchors.lua:237-243) operation by operation; FMA contraction is off
// for this translation unit.  log() is the device library's double log: within an ulp, as the host's.
#pragma clang fp contract(off)
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "kernels.h"

namespace frcnn {

#define PT_THREADS 1024
#define PT_TILES 4
#define PT_WAVES (PT_THREADS / 64)
constexpr int PT_MAX_N = PT_THREADS * PT_TILES;   // candidates a segment: ground truth + picks
constexpr int PT_MAX_G = 64;
constexpr int PT_GROUP = 128;                     // segments a launch
struct TargetGroup { int G[PT_GROUP]; };
static_assert(sizeof(TargetGroup) <= 1024, "the ground-truth counts of a group travel as a kernel argument");
static_assert(PT_TILES * PT_WAVES == 64, "one wave scans the (tile, wave) counts");

// the key of row i of segment b: a bijection of 32 bits applied to pre-images that differ within a segment -- keys never tie
__device__ __forceinline__ unsigned target_key(unsigned seed, unsigned i, unsigned b) {
  unsigned x = seed + 0x9E3779B9u * (i + 1u) + 0x85EBCA6Bu * b;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// Rect.IoU(c, g) (Rect.lua:126-141: no + 1; an empty intersection has area 0); ca / ga: the two areas.  Python's max / min: the
// second operand wins only when it compares greater / less.
__device__ __forceinline__ double rect_iou(const double* c, double ca, const double* g, double ga) {
  const double minx = g[0] > c[0] ? g[0] : c[0], miny = g[1] > c[1] ? g[1] : c[1];
  const double maxx = g[2] < c[2] ? g[2] : c[2], maxy = g[3] < c[3] ? g[3] : c[3];
  double inter = 0.0;
  if (maxx >= minx && maxy >= miny) {
    const double w = maxx - minx, h = maxy - miny;
    inter = w * h;
  }
  double den = ca + ga;
  den = den - inter;
  const double q = inter / den;
  return q != q ? 0.0 : q;
}

__global__ __launch_bounds__(PT_THREADS) void proposal_targets_batch_kernel(
    TargetGroup grp, int b0, const double* __restrict__ rect, const long long* __restrict__ pick, long long match_stride,
    const int* __restrict__ r_dev, int r_cap, const double* __restrict__ gt_rect, const int* __restrict__ gt_class, int gt_stride,
    int include_gt, double fg_iou, double bg_lo, double bg_hi, int fg_quota, int batch, int bgclass, unsigned seed,
    double* __restrict__ roi, float* __restrict__ crtarget, float* __restrict__ cctarget, int* __restrict__ src,
    int* __restrict__ gt_idx, double* __restrict__ iou, int out_stride, int* __restrict__ counts) {
  __shared__ double s_gt[PT_MAX_G][4];
  __shared__ double s_garea[PT_MAX_G];
  __shared__ __attribute__((aligned(16))) unsigned long long s_kl[PT_MAX_N];   // (label << 32) | key; ~0 behind row N
  __shared__ int s_cnt[2][64];                                                  // per (tile, wave): foreground / background rows
  __shared__ int s_tot[2];
  const int b = b0 + blockIdx.x;
  const int G = grp.G[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  rect += (size_t)b * match_stride * 4; pick += (size_t)b * match_stride;
  gt_rect += (size_t)b * gt_stride * 4; gt_class += (size_t)b * gt_stride;
  const size_t so = (size_t)b * out_stride;
  const int R = min(max(r_dev[b], 0), r_cap);
  const int Gp = include_gt ? G : 0;
  const int N = Gp + R;                                 // (<= PT_MAX_N: checked by the launcher)
  if (N == 0) {                                         // (the whole workgroup leaves)
    if (tid == 0) *reinterpret_cast<int4*>(counts + 4 * (size_t)b) = make_int4(0, 0, 0, 0);
    return;
  }
  if (tid < G) {
    const double x0 = gt_rect[4 * tid], y0 = gt_rect[4 * tid + 1], x1 = gt_rect[4 * tid + 2], y1 = gt_rect[4 * tid + 3];
    s_gt[tid][0] = x0; s_gt[tid][1] = y0; s_gt[tid][2] = x1; s_gt[tid][3] = y1;
    const double w = x1 - x0, h = y1 - y0;
    s_garea[tid] = w * h;
  }
  __syncthreads();

  // candidate i: ground-truth box i in front (include_gt), then pick i - Gp.  A pick outside 1 ... match_stride reads nothing and
  // is ignored, as a candidate with a coordinate that is not finite.
  auto load_candidate = [&](int i, double* c) -> bool {
    if (i < Gp) {
      c[0] = s_gt[i][0]; c[1] = s_gt[i][1]; c[2] = s_gt[i][2]; c[3] = s_gt[i][3];
      return true;
    }
    const long long p = pick[i - Gp];
    if (p < 1 || p > match_stride) { c[0] = c[1] = c[2] = c[3] = 0.0; return false; }
    const double* q = rect + 4 * (size_t)(p - 1);
    c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; c[3] = q[3];
    return true;
  };

  // ---- 1. match and label; {label, key} to LDS; rows per (tile, wave)
  int lab[PT_TILES], bestg[PT_TILES];
  double bestv[PT_TILES];
  unsigned long long v[PT_TILES];
#pragma unroll
  for (int t = 0; t < PT_TILES; ++t) {
    const int i = t * PT_THREADS + tid;
    lab[t] = 0; bestg[t] = -1; bestv[t] = 0.0;
    v[t] = ~0ull;
    if (i < N) {
      double c[4];
      bool ok = load_candidate(i, c);
      const double cw = c[2] - c[0], ch = c[3] - c[1];
      ok = ok && isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]) && cw > 0.0 && ch > 0.0;
      if (ok) {
        const double ca = cw * ch;
        for (int g = 0; g < G; ++g) {
          const double q = rect_iou(c, ca, s_gt[g], s_garea[g]);
          if (g == 0 || q > bestv[t]) { bestv[t] = q; bestg[t] = g; }   // the first maximum: the lowest g wins a tie
        }
        if (bestg[t] >= 0 && bestv[t] >= fg_iou) lab[t] = 1;   // foreground needs a box: G = 0 labels background or ignored only
        else if (bg_lo <= bestv[t] && bestv[t] < bg_hi) lab[t] = 2;
      }
      v[t] = ((unsigned long long)lab[t] << 32) | target_key(seed, (unsigned)i, (unsigned)b);
    }
    s_kl[i] = v[t];
    const unsigned long long fm = __ballot(lab[t] == 1), bm = __ballot(lab[t] == 2);
    if (lane == 0) { s_cnt[0][t * PT_WAVES + wave] = __popcll(fm); s_cnt[1][t * PT_WAVES + wave] = __popcll(bm); }
  }
  __syncthreads();
  if (wave == 0) {
    int f = s_cnt[0][lane], g = s_cnt[1][lane];
    for (int d = 32; d >= 1; d >>= 1) { f += __shfl_xor(f, d, 64); g += __shfl_xor(g, d, 64); }
    if (lane == 0) { s_tot[0] = f; s_tot[1] = g; }
  }
  __syncthreads();
  const int nfg = s_tot[0], nbg = s_tot[1], nign = N - nfg - nbg;
  const int F = min(nfg, fg_quota), Bq = min(nbg, batch - F);

  // ---- 2. a class over its quota keeps the rows with the smallest keys: rank = smaller words - rows of the classes in front
  bool keep[PT_TILES];
#pragma unroll
  for (int t = 0; t < PT_TILES; ++t) keep[t] = lab[t] != 0;
  if (nfg > F || nbg > Bq) {                            // (the same in every thread)
    int less[PT_TILES];
    bool ranked = false;                                // a row of this thread belongs to a class that is cut
#pragma unroll
    for (int t = 0; t < PT_TILES; ++t) {
      less[t] = 0;
      ranked = ranked || (lab[t] == 1 && nfg > F) || (lab[t] == 2 && nbg > Bq);
    }
    const ulonglong2* kl2 = reinterpret_cast<const ulonglong2*>(s_kl);
    // the walk is bound by the compares (one workgroup, 16 waves on 4 SIMDs): only the tiles that hold rows are compared, and a
    // wave without a row to rank skips it (no barrier inside)
    auto walk = [&](auto nt) {
      constexpr int NT = decltype(nt)::value;
#pragma unroll 4
      for (int k = 0; k < (N + 1) / 2; ++k) {           // (the word behind an odd N is ~0: smaller than nothing)
        const ulonglong2 w = kl2[k];
#pragma unroll
        for (int t = 0; t < NT; ++t) less[t] += (int)(w.x < v[t]) + (int)(w.y < v[t]);
      }
    };
    if (__any(ranked)) {
      switch ((N + PT_THREADS - 1) / PT_THREADS) {
        case 1: walk(std::integral_constant<int, 1>{}); break;
        case 2: walk(std::integral_constant<int, 2>{}); break;
        case 3: walk(std::integral_constant<int, 3>{}); break;
        default: walk(std::integral_constant<int, PT_TILES>{}); break;
      }
    }
#pragma unroll
    for (int t = 0; t < PT_TILES; ++t) {
      if (lab[t] == 1 && nfg > F) keep[t] = less[t] - nign < F;
      if (lab[t] == 2 && nbg > Bq) keep[t] = less[t] - nign - nfg < Bq;
    }
  }

  // ---- 3. ordered compaction: the kept foreground rows in candidate order, then the kept background rows
  unsigned long long fmask[PT_TILES], bmask[PT_TILES];
#pragma unroll
  for (int t = 0; t < PT_TILES; ++t) {
    fmask[t] = __ballot(keep[t] && lab[t] == 1);
    bmask[t] = __ballot(keep[t] && lab[t] == 2);
    if (lane == 0) { s_cnt[0][t * PT_WAVES + wave] = __popcll(fmask[t]); s_cnt[1][t * PT_WAVES + wave] = __popcll(bmask[t]); }
  }
  __syncthreads();
  if (wave == 0) {                                      // exclusive scan of the 64 (tile, wave) counts, both classes
    const int f = s_cnt[0][lane], g = s_cnt[1][lane];
    int fi = f, gi = g;
    for (int d = 1; d < 64; d <<= 1) {
      const int fu = __shfl_up(fi, d, 64), gu = __shfl_up(gi, d, 64);
      if (lane >= d) { fi += fu; gi += gu; }
    }
    s_cnt[0][lane] = fi - f; s_cnt[1][lane] = gi - g;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int t = 0; t < PT_TILES; ++t) {
    if (!keep[t]) continue;
    const int i = t * PT_THREADS + tid;
    const bool fg = lab[t] == 1;
    const int j = fg ? s_cnt[0][t * PT_WAVES + wave] + __popcll(fmask[t] & below)
                     : F + s_cnt[1][t * PT_WAVES + wave] + __popcll(bmask[t] & below);
    if (j >= batch) continue;                           // (cannot happen while keys differ; nothing is stored behind `batch`)
    double c[4];
    load_candidate(i, c);
    const size_t o = so + (size_t)j;
    double2* ro = reinterpret_cast<double2*>(roi + 4 * o);
    ro[0] = make_double2(c[0], c[1]); ro[1] = make_double2(c[2], c[3]);
    float4 tg = make_float4(0.f, 0.f, 0.f, 0.f);
    float cc = (float)bgclass;
    if (fg) {                                           // Anchors.inputToAnchor(candidate, gt[best]), Anchors.lua:237-243
      const double* g = s_gt[bestg[t]];
      const double cw = c[2] - c[0], ch = c[3] - c[1];
      const double dx = g[0] - c[0], dy = g[1] - c[1];
      const double gw = g[2] - g[0], gh = g[3] - g[1];
      const double rw = gw / cw, rh = gh / ch;
      tg = make_float4((float)(dx / cw), (float)(dy / ch), (float)log(rw), (float)log(rh));
      cc = (float)gt_class[bestg[t]];
    }
    *reinterpret_cast<float4*>(crtarget + 4 * o) = tg;
    cctarget[o] = cc;
    src[o] = i;
    gt_idx[o] = bestg[t];
    iou[o] = bestv[t];
  }
  if (tid == 0) *reinterpret_cast<int4*>(counts + 4 * (size_t)b) = make_int4(nfg, nbg, F, Bq);
}

int proposal_targets_batch(const double* rect, const long long* pick, long long match_stride, const int* r_dev, int r_cap,
                           const double* gt_rect, const int* gt_class, int gt_stride, const int* G_host, int B, int include_gt,
                           double fg_iou, double bg_lo, double bg_hi, int fg_quota, int batch, int bgclass, unsigned seed,
                           double* roi, float* crtarget, float* cctarget, int* src, int* gt_idx, double* iou, int out_stride,
                           int* counts, hipStream_t s) {
  // everything is checked before the first launch: a refused call has written nothing
  FR_CHECK(B >= 0 && B <= 65535, "proposal_targets: %d segments (0 ... 65535)", B);
  if (B == 0) return FRCNN_OK;
  FR_CHECK(r_cap >= 0 && (long long)r_cap + PT_MAX_G <= PT_MAX_N, "proposal_targets: r_cap %d (0 ... %d: r_cap + %d candidates fit %d)",
           r_cap, PT_MAX_N - PT_MAX_G, PT_MAX_G, PT_MAX_N);
  FR_CHECK(bg_hi <= fg_iou && bg_lo <= bg_hi, "proposal_targets: thresholds bg [%g, %g), fg >= %g (need bg_lo <= bg_hi <= fg_iou)",
           bg_lo, bg_hi, fg_iou);   // (a NaN fails both)
  FR_CHECK(batch >= 1, "proposal_targets: batch %d (at least 1)", batch);
  FR_CHECK(fg_quota >= 0 && fg_quota <= batch, "proposal_targets: fg_quota %d (0 ... batch = %d)", fg_quota, batch);
  FR_CHECK(out_stride >= batch, "proposal_targets: out_stride %d < batch %d", out_stride, batch);
  FR_CHECK(bgclass >= 1, "proposal_targets: background class %d (at least 1)", bgclass);
  FR_CHECK(match_stride >= r_cap && gt_stride >= 0, "proposal_targets: match_stride %lld < r_cap %d, or gt_stride %d negative",
           match_stride, r_cap, gt_stride);
  FR_CHECK(r_dev && G_host && roi && crtarget && cctarget && src && gt_idx && iou && counts, "proposal_targets: NULL argument");
  int gmax = 0;
  for (int b = 0; b < B; ++b) {
    FR_CHECK(G_host[b] >= 0 && G_host[b] <= PT_MAX_G, "proposal_targets: segment %d has %d ground-truth boxes (0 ... %d)", b,
             G_host[b], PT_MAX_G);
    gmax = std::max(gmax, G_host[b]);
  }
  FR_CHECK(gmax <= gt_stride, "proposal_targets: %d ground-truth boxes in a segment of gt_stride %d", gmax, gt_stride);
  FR_CHECK(gmax == 0 || (gt_rect && gt_class), "proposal_targets: NULL ground truth");
  FR_CHECK(r_cap == 0 || (rect && pick), "proposal_targets: NULL candidates");
  FR_CHECK(((uintptr_t)roi | (uintptr_t)crtarget | (uintptr_t)counts) % 16 == 0,
           "proposal_targets: roi, crtarget and counts are stored 16 bytes at a time and must be 16-byte aligned");
  for (int b0 = 0; b0 < B; b0 += PT_GROUP) {
    const int nb = std::min(B - b0, PT_GROUP);
    TargetGroup g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < nb; ++i) g.G[i] = G_host[b0 + i];
    FR_LAUNCH(KC_RPN, 0, (double)nb * ((r_cap + gmax) * 48.0 + batch * 80.0), s, proposal_targets_batch_kernel, dim3(nb),
              dim3(PT_THREADS), 0, g, b0, rect, pick, match_stride, r_dev, r_cap, gt_rect, gt_class, gt_stride, include_gt != 0, fg_iou,
              bg_lo, bg_hi, fg_quota, batch, bgclass, seed, roi, crtarget, cctarget, src, gt_idx, iou, out_stride, counts);
  }
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
