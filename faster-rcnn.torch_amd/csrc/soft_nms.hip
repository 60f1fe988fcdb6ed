// soft_nms.hip -- Soft-NMS (Bodla et al. 2017) for the per-class pass of Detector: the neighbours of a pick keep living with a
// lowered score instead of being deleted.  Not in the reference (its per-class pass is the hard cut of Detector.lua:125-136,
// nms.hip here); off unless cfg.nms asks for it.
//
// The bit-matrix pipeline of nms.hip does not apply: it sorts ONCE and turns every pair into one bit, which is all a hard cut
// needs.  Here the next pick is the arg-max of scores the previous pick has just rewritten (no fixed order), and a pair
// contributes the VALUE of its IoU.  So the kernel is the greedy loop itself, one workgroup per segment:
//
//   s[i] = score column; row i is alive iff s[i] >= min_score                      (a NaN is never alive)
//   repeat: m = the alive, unpicked row of largest s (fp32 VALUES: -0 == +0); ties: the HIGHER row id  (nms.hip's tie rule:
//           ascending key, ties ascending row, picks from the end);  none -> stop;  pick m, score_out[m] = s[m];
//           every alive unpicked j of m's class (all j without cls):
//             hard      !(iou <= Nt): j dies
//             linear    !(iou <= Nt): s[j] = s[j] * (1 - iou)                  log domain: s[j] + log1pf(-iou)
//             gaussian  (every j)     s[j] = s[j] * expf(-(iou * iou) / sigma)  log domain: s[j] - (iou * iou) / sigma
//             then      !(s[j] >= min_score): j dies
//
// Arithmetic: fp32, every operation rounded on its own (no contraction, as in nms.hip), area and IoU the box_area and box_iou of
// box_iou.h, which nms.hip computes its own with.  hard, linear outside the log domain and gaussian inside it contain no transcendental: their results are a function of the
// inputs' bits alone.  The scores are plain loads, stores and arithmetic; there is no atomic of any kind in this file, and a
// row's score is only ever read and written by the one thread that owns the row.
//
// A dead or picked row is a row whose working score is a NaN (a NaN is never alive, so no state array is needed).
// The arg-max runs on the order-preserving unsigned image of the score (-0 folded onto +0; 0 = "no row"), reduced over a wave
// with data-parallel-primitive moves (the house style of nms_wave_or32) and taken out with one readlane: first the largest
// image, then the highest row among the lanes that hold it.
//
// Three paths, chosen per segment from its DEVICE-side count n (so a frame with a few hundred rows is fast whatever bound
// the launch was sized for):
//   n <= SNMS_WAVE_ROWS (512)     one wave, the segment in its registers (8 rows a lane: box, area, class, score), the
//                                 pick's box broadcast with readlane: NO barrier and no LDS at all.  The other waves of the
//                                 workgroup leave at once.
//   n <= SNMS_LDS_ROWS (2048)     the workgroup (512 threads: the wave path needs 160 vector registers, which eight waves leave
//                                 it and sixteen would not), boxes / classes / scores in LDS (24 bytes a row, 48 KB), thread
//                                 t owns rows t, t + 512, ...: one pass over its rows per pick (the decay by the previous pick and
//                                 the local arg-max for the next one, fused), a wave reduction, ONE barrier, and every wave
//                                 reduces the 8 wave results for itself (double-buffered, so one barrier is enough).
//   n <= SNMS_MAX_ROWS (16384)    the same loop with the boxes and classes read from global memory (read-only input) and the
//                                 working scores in the workspace (owner-only, so no fence is needed).
#pragma clang fp contract(off)
#include "kernels.h"
#include "box_iou.h"

namespace frcnn {

#define SNMS_WAVE_SLOTS 8
#define SNMS_WAVE_ROWS (64 * SNMS_WAVE_SLOTS)
#define SNMS_LDS_ROWS 2048
#define SNMS_MAX_ROWS 16384
#define SNMS_THREADS 512
#define SNMS_WAVES (SNMS_THREADS / 64)

struct SnmsParams {
  int method;       // 0 hard, 1 linear, 2 gaussian
  int log_domain;
  float overlap, sigma, min_score;
};

// order-preserving image of an fp32 VALUE: a < b <=> img(a) < img(b) for non-NaN a, b; -0 and +0 share an image; every alive
// score (>= -inf) has an image >= 0x007fffff, so 0 stands for "no row"
__device__ __forceinline__ unsigned snms_image(float s) {
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// max of an unsigned value over the 64 lanes of a wave, returned wave-uniform (the moves of nms_wave_or32; a lane without a source
// reads 0, the identity)
__device__ __forceinline__ unsigned snms_wave_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));   // row_shr:1
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));   // row_shr:2
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));   // row_shr:4
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));   // row_shr:8  -> lane 15 of each row
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));   // row_bcast:15 into rows 1, 3
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));   // row_bcast:31 into rows 2, 3 -> lane 63
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// the score of row j (box j*, area ja) after the pick of box m*: the new working score, a NaN when the row dies
__device__ __forceinline__ float snms_decay(const SnmsParams& P, float s, float jx1, float jy1, float jx2, float jy2, float ja,
                                            float mx1, float my1, float mx2, float my2, float ma) {
  const float iou = box_iou(jx1, jy1, jx2, jy2, ja, mx1, my1, mx2, my2, ma);
  const float dead = __builtin_nanf("");
  if (P.method == 2) {
    float t = iou * iou;
    t = t / P.sigma;
    if (P.log_domain) s = s - t;
    else s = s * expf(-t);
  } else if (!(iou <= P.overlap)) {
    if (P.method == 0) return dead;
    if (P.log_domain) s = s + log1pf(-iou);
    else {
      float f = 1.0f - iou;
      s = s * f;
    }
  }
  return s >= P.min_score ? s : dead;
}

// ---- path 1: one wave, everything in registers, no barrier
__device__ __forceinline__ void snms_wave_body(const float* __restrict__ boxes, int n, int ncols, int score_col, const SnmsParams& P,
                                               const int* __restrict__ cls, long long* __restrict__ pick, int* __restrict__ count,
                                               float* __restrict__ score_out, long score_stride) {
  const int lane = threadIdx.x;
  const int nslots = (n + 63) >> 6;   // (uniform)
  float x1[SNMS_WAVE_SLOTS], y1[SNMS_WAVE_SLOTS], x2[SNMS_WAVE_SLOTS], y2[SNMS_WAVE_SLOTS], ar[SNMS_WAVE_SLOTS], s[SNMS_WAVE_SLOTS];
  int cl[SNMS_WAVE_SLOTS];
#pragma unroll
  for (int k = 0; k < SNMS_WAVE_SLOTS; ++k) {
    const int i = k * 64 + lane;
    x1[k] = y1[k] = x2[k] = y2[k] = ar[k] = 0.f;
    cl[k] = 0;
    s[k] = __builtin_nanf("");
    if (i < n) {
      const float* b = boxes + (size_t)i * ncols;
      x1[k] = b[0]; y1[k] = b[1]; x2[k] = b[2]; y2[k] = b[3];
      ar[k] = box_area(x1[k], y1[k], x2[k], y2[k]);
      cl[k] = cls ? cls[i] : 0;
      const float v = b[score_col - 1];
      s[k] = v >= P.min_score ? v : __builtin_nanf("");
    }
  }
  int cnt = 0;
  for (;;) {
    // the lane's best row (the later slot is the higher row: >= lets it win a tie), then the wave's
    unsigned bi = 0u;
    int br = 0;
#pragma unroll
    for (int k = 0; k < SNMS_WAVE_SLOTS; ++k) {
      if (k < nslots) {
        const unsigned im = s[k] == s[k] ? snms_image(s[k]) : 0u;
        if (im != 0u && im >= bi) { bi = im; br = k * 64 + lane + 1; }
      }
    }
    const unsigned best = snms_wave_max(bi);
    if (best == 0u) break;
    const int m = (int)snms_wave_max(bi == best ? (unsigned)br : 0u) - 1;
    const int ml = m & 63, mk = m >> 6;   // (uniform)
    float mx1 = 0.f, my1 = 0.f, mx2 = 0.f, my2 = 0.f, ma = 0.f, msc = 0.f;
    int mc = 0;
#pragma unroll
    for (int k = 0; k < SNMS_WAVE_SLOTS; ++k) {
      if (k == mk) {   // (uniform branch: the slot index stays a compile-time constant)
        mx1 = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(x1[k]), ml));
        my1 = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(y1[k]), ml));
        mx2 = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(x2[k]), ml));
        my2 = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(y2[k]), ml));
        ma = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(ar[k]), ml));
        msc = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(s[k]), ml));
        mc = __builtin_amdgcn_readlane(cl[k], ml);
        if (lane == ml) s[k] = __builtin_nanf("");
      }
    }
    if (lane == 0) {
      pick[cnt] = (long long)m + 1;
      if (score_out) score_out[(size_t)m * score_stride] = msc;
    }
    ++cnt;
#pragma unroll
    for (int k = 0; k < SNMS_WAVE_SLOTS; ++k) {
      if (k < nslots) {
        if (s[k] == s[k] && cl[k] == mc)
          s[k] = snms_decay(P, s[k], x1[k], y1[k], x2[k], y2[k], ar[k], mx1, my1, mx2, my2, ma);
      }
    }
  }
  if (lane == 0) *count = cnt;
}

// ---- paths 2 and 3: the workgroup; LDS = true: box / class / score images in LDS, false: boxes and classes from global memory,
// working scores in ws (n floats).  One barrier per pick.
template <bool LDS>
__device__ __forceinline__ void snms_group_body(const float* __restrict__ boxes, int n, int ncols, int score_col, const SnmsParams& P,
                                                const int* __restrict__ cls, long long* __restrict__ pick, int* __restrict__ count,
                                                float* __restrict__ score_out, long score_stride, float* __restrict__ ws,
                                                float* lds) {
  __shared__ unsigned wbest[2][SNMS_WAVES];
  __shared__ int wrow[2][SNMS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // LDS images: [6][SNMS_LDS_ROWS] x1 y1 x2 y2 score class
  float* lx1 = lds;
  float* ly1 = lds + SNMS_LDS_ROWS;
  float* lx2 = lds + 2 * SNMS_LDS_ROWS;
  float* ly2 = lds + 3 * SNMS_LDS_ROWS;
  float* lsc = lds + 4 * SNMS_LDS_ROWS;
  int* lcl = reinterpret_cast<int*>(lds + 5 * SNMS_LDS_ROWS);
  float* sc = LDS ? lsc : ws;
  for (int i = tid; i < n; i += SNMS_THREADS) {
    const float* b = boxes + (size_t)i * ncols;
    const float v = b[score_col - 1];
    sc[i] = v >= P.min_score ? v : __builtin_nanf("");
    if (LDS) {
      lx1[i] = b[0]; ly1[i] = b[1]; lx2[i] = b[2]; ly2[i] = b[3];
      lcl[i] = cls ? cls[i] : 0;
    }
  }
  if (LDS) __syncthreads();   // (the boxes are read across threads; a score only by its owner)
  int cnt = 0, m = -1;
  float mx1 = 0.f, my1 = 0.f, mx2 = 0.f, my2 = 0.f, ma = 0.f;
  int mc = 0;
  for (;;) {
    // one pass over the thread's rows: the decay by the previous pick, and the best of what is left (ascending rows: >= lets the
    // higher row win a tie)
    unsigned bi = 0u;
    int br = 0;
    for (int i = tid; i < n; i += SNMS_THREADS) {
      float s = sc[i];
      if (!(s == s)) continue;
      if (m >= 0) {
        const int c = LDS ? lcl[i] : (cls ? cls[i] : 0);
        if (c == mc) {
          float jx1, jy1, jx2, jy2;
          if (LDS) { jx1 = lx1[i]; jy1 = ly1[i]; jx2 = lx2[i]; jy2 = ly2[i]; }
          else {
            const float* b = boxes + (size_t)i * ncols;
            jx1 = b[0]; jy1 = b[1]; jx2 = b[2]; jy2 = b[3];
          }
          s = snms_decay(P, s, jx1, jy1, jx2, jy2, box_area(jx1, jy1, jx2, jy2), mx1, my1, mx2, my2, ma);
          sc[i] = s;
          if (!(s == s)) continue;
        }
      }
      const unsigned im = snms_image(s);
      if (im >= bi) { bi = im; br = i + 1; }
    }
    const unsigned wb = snms_wave_max(bi);
    const unsigned wr = snms_wave_max((bi == wb && wb != 0u) ? (unsigned)br : 0u);
    const int par = cnt & 1;
    if (lane == 0) { wbest[par][wave] = wb; wrow[par][wave] = (int)wr; }
    __syncthreads();
    unsigned best = 0u;
    int row = 0;
#pragma unroll
    for (int w = 0; w < SNMS_WAVES; ++w) {
      const unsigned b = wbest[par][w];
      const int r = wrow[par][w];
      if (b > best || (b == best && r > row)) { best = b; row = r; }
    }
    if (best == 0u) break;   // (uniform over the workgroup)
    m = row - 1;
    if (LDS) { mx1 = lx1[m]; my1 = ly1[m]; mx2 = lx2[m]; my2 = ly2[m]; mc = lcl[m]; }
    else {
      const float* b = boxes + (size_t)m * ncols;
      mx1 = b[0]; my1 = b[1]; mx2 = b[2]; my2 = b[3];
      mc = cls ? cls[m] : 0;
    }
    ma = box_area(mx1, my1, mx2, my2);
    if ((m & (SNMS_THREADS - 1)) == tid) {   // the owner: records the pick and retires the row
      pick[cnt] = (long long)m + 1;
      if (score_out) score_out[(size_t)m * score_stride] = sc[m];
      sc[m] = __builtin_nanf("");
    }
    ++cnt;
  }
  if (tid == 0) *count = cnt;
}

// grid.x = segment; block = 64 threads when the host-side bound fits one wave, SNMS_THREADS otherwise; dynamic LDS = the images
// of min(bound, SNMS_LDS_ROWS) rows when the bound exceeds one wave
__global__ __launch_bounds__(SNMS_THREADS) void soft_nms_batch_kernel(const float* __restrict__ boxes, long row_stride, int n_cap,
                                                                       const int* __restrict__ n_dev, int ncols, int score_col,
                                                                       SnmsParams P, const int* __restrict__ cls,
                                                                       long long* __restrict__ pick, int* __restrict__ count,
                                                                       float* __restrict__ score_out, long score_stride,
                                                                       float* __restrict__ ws) {
  extern __shared__ float snms_lds[];
  const int b = blockIdx.x;
  const int n = min(n_dev[b], n_cap);
  boxes += (size_t)b * row_stride * ncols;
  if (cls) cls += (size_t)b * row_stride;
  pick += (size_t)b * row_stride;
  if (score_out) score_out += (size_t)b * row_stride * score_stride;
  count += b;
  if (n <= 0) {
    if (threadIdx.x == 0) *count = 0;
    return;
  }
  if (n <= SNMS_WAVE_ROWS) {
    if (threadIdx.x < 64) snms_wave_body(boxes, n, ncols, score_col, P, cls, pick, count, score_out, score_stride);
  } else if (n <= SNMS_LDS_ROWS) {
    snms_group_body<true>(boxes, n, ncols, score_col, P, cls, pick, count, score_out, score_stride, nullptr, snms_lds);
  } else {
    snms_group_body<false>(boxes, n, ncols, score_col, P, cls, pick, count, score_out, score_stride, ws + (size_t)b * n_cap, nullptr);
  }
}

size_t soft_nms_workspace_bytes(int B, int n_cap) {
  if (B <= 0 || n_cap <= SNMS_LDS_ROWS) return 256;
  return (size_t)B * n_cap * 4 + 256;   // the working scores of the segments that fit neither registers nor LDS
}

int soft_nms_batch(const float* boxes, int B, long row_stride, int n_cap, const int* n_dev, int ncols, int score_col, int method,
                   float overlap, float sigma, float min_score, int log_domain, const int* cls, long long* pick, int* count,
                   float* score_out, long score_stride, void* ws, size_t ws_bytes, hipStream_t s) {
  FR_CHECK(B >= 1 && B <= 65535, "soft_nms: %d segments (1 .. 65535)", B);
  FR_CHECK(boxes && n_dev && pick && count, "soft_nms: NULL argument (boxes, n_dev, pick and count are required)");
  FR_CHECK(n_cap >= 0 && n_cap <= SNMS_MAX_ROWS, "soft_nms: %d rows per segment (at most %d)", n_cap, SNMS_MAX_ROWS);
  FR_CHECK(row_stride >= n_cap, "soft_nms: row stride %ld < %d rows per segment", row_stride, n_cap);
  FR_CHECK(ncols >= 5, "soft_nms: rows need >= 5 columns (got %d)", ncols);
  FR_CHECK(score_col >= 5 && score_col <= ncols, "soft_nms: score column %d outside [5, %d]", score_col, ncols);
  FR_CHECK(method >= 0 && method <= 2, "soft_nms: bad method %d (0 hard, 1 linear, 2 gaussian)", method);
  FR_CHECK(sigma > 0.f, "soft_nms: sigma = %g (must be > 0)", (double)sigma);
  FR_CHECK(log_domain == 0 || log_domain == 1, "soft_nms: log_domain = %d (0 or 1)", log_domain);
  FR_CHECK(score_out == nullptr || score_stride >= 1, "soft_nms: score stride %ld", score_stride);
  FR_CHECK(ws_bytes >= soft_nms_workspace_bytes(B, n_cap) && (ws || n_cap <= SNMS_LDS_ROWS),
           "soft_nms: workspace too small (%zu < %zu)", ws_bytes, soft_nms_workspace_bytes(B, n_cap));
  if (n_cap == 0) {
    FR_HIP(hipMemsetAsync(count, 0, sizeof(int) * (size_t)B, s));
    return FRCNN_OK;
  }
  SnmsParams P;
  P.method = method; P.log_domain = log_domain; P.overlap = overlap; P.sigma = sigma; P.min_score = min_score;
  const int threads = n_cap <= SNMS_WAVE_ROWS ? 64 : SNMS_THREADS;
  const size_t lds = n_cap <= SNMS_WAVE_ROWS ? 0 : (size_t)6 * SNMS_LDS_ROWS * 4;
  float* wsf = n_cap > SNMS_LDS_ROWS ? (float*)(((uintptr_t)ws + 255) / 256 * 256) : nullptr;
  FR_LAUNCH(KC_SOFT_NMS, 40.0 * B * (double)n_cap, 24.0 * B * (double)n_cap, s, soft_nms_batch_kernel, dim3(B), dim3(threads), lds,
            boxes, row_stride, n_cap, n_dev, ncols, score_col, P, cls, pick, count, score_out, score_stride, wsf);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
