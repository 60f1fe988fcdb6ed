// eval_match.hip -- the match of a chunk's winners to the frames' ground truth for mean average precision, on the device
// (include/frcnn_hip_eval.h; not in the reference, whose evaluation is a sketch: main.lua:183-216).  The host's greedy loop
// (evaluation.mean_average_precision: detections by decreasing confidence, a box is used by the first that claims it) restated
// without its sequential dependence, per frame and for up to 16 IoU thresholds at once:
//   1. BEST BOX  detection d of class c walks the frame's boxes of class c in their order: best = -1, gt = none; v = Rect.IoU(r2_d, g)
//                in fp64, every operation rounded on its own (contraction off; a NaN stays a NaN); the box is taken when v > best --
//                the first maximum wins, a NaN never does, boxes of other classes (and of a class < 1) are not looked at.
//                reach_d = { t : best_d >= thr[t] }, empty without a box.
//   2. CLAIM     at threshold t, d is a true positive iff t is in reach_d and d is the FIRST of the frame's detections e with
//                gt_e == gt_d and t in reach_e, in the order (confidence as an fp32 value, decreasing; ties: the earlier row).
// Which box a detection looks at does not depend on who claimed what, so step 1 is one thread a detection and step 2 a minimum
// of the 64-bit word (~image(confidence) << 32 | row) per (box, threshold): no sort, no atomics, no serial scan, and every integer
// is a function of the data alone.
//
// Shape: TWO launches per group of EM_GROUP frames, the frame a grid dimension, no tiers.
//   eval_best_kernel   grid (row tiles, frames), one thread a detection, rows in strides of the grid.  Writes the frame's two
//                      header rows and, per detection, {class, confidence bits, reach mask, gt}; the ground truth is read with
//                      wave-uniform addresses (every lane walks the same boxes).
//   eval_claim_kernel  grid (box tiles, frames), one wave a box, boxes in strides of the grid.  The wave walks the frame's rows
//                      twice: first the minimum word per threshold over the rows whose gt is its box (64 lanes, then a
//                      __shfl_xor butterfly), then it REPLACES the reach mask of each of those rows by the thresholds it won.
//                      A row belongs to one box: one writer per word; rows without a box keep the empty mask step 1 wrote.
// The frames' first ground-truth rows and the thresholds are host values and travel by value as kernel arguments (the way
// detect_class_boxes_batch carries its descriptors): no device table, no wait.
#pragma clang fp contract(off)
#include "kernels.h"

namespace frcnn {

constexpr int EM_GROUP = 64;       // frames a launch
constexpr int EM_THREADS = 256;    // eval_best: detections a workgroup; eval_claim: EM_THREADS / 64 boxes a workgroup
constexpr int EM_WAVES = EM_THREADS / 64;
constexpr int EM_MAX_T = 16;       // thresholds (one bit each of the mask)
constexpr int EM_MAX_G = 1024;     // ground-truth boxes a frame
constexpr int EM_MAX_ROWS = 1 << 27;  // rows a frame: what keeps a row's byte offset in a table and the grid's strides inside an int
constexpr int EM_BLOCKS = 4096;    // workgroups a launch at most

struct EvalGroup { long long g0[EM_GROUP + 1]; };   // frame i of the group: ground-truth rows g0[i] ... g0[i + 1] - 1
struct EvalThr { double v[EM_MAX_T]; };
static_assert(sizeof(EvalGroup) + sizeof(EvalThr) <= 1024, "the descriptors of a group travel as kernel arguments");

// a < b as fp32 values  <=>  image(a) < image(b) as unsigned; image(-0) == image(+0); a NaN ranks below everything: the rank of
// frcnn_topk_select
__device__ __forceinline__ unsigned em_image(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Rect.IoU(a, g) (Rect.py; the arithmetic of rect_iou in proposal_targets.hip, but a NaN is returned as it is)
__device__ __forceinline__ double em_iou(const double a0, const double a1, const double a2, const double a3, double aa,
                                         const double* __restrict__ g) {
  const double g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
  const double minx = g0 > a0 ? g0 : a0, miny = g1 > a1 ? g1 : a1;
  const double maxx = g2 < a2 ? g2 : a2, maxy = g3 < a3 ? g3 : a3;
  double inter = 0.0;
  if (maxx >= minx && maxy >= miny) {
    const double w = maxx - minx, h = maxy - miny;
    inter = w * h;
  }
  const double gw = g2 - g0, gh = g3 - g1;
  const double ga = gw * gh;
  double den = aa + ga;
  den = den - inter;
  return inter / den;
}

// the rows a frame emits: the winners (int 3 of the gather's header, at most row_stride), or the selected ones among them
__device__ __forceinline__ int em_rows(const double* __restrict__ tab, int row_stride, const int* __restrict__ k_dev, int b,
                                       long long sel_stride, int& winners) {
  winners = min(max(reinterpret_cast<const int*>(tab)[3], 0), row_stride);
  if (!k_dev) return winners;
  return (int)min((long long)min(max(k_dev[b], 0), winners), sel_stride);
}

__global__ __launch_bounds__(EM_THREADS) void eval_best_kernel(EvalGroup grp, EvalThr thr, int T, int b0, const double* __restrict__ rec,
                                                               int row_stride, const int* __restrict__ sel_row, long long sel_stride,
                                                               const int* __restrict__ k_dev, const double* __restrict__ gt_rect,
                                                               const int* __restrict__ gt_class, int* __restrict__ match,
                                                               double* __restrict__ iou) {
  const int b = b0 + blockIdx.y;
  const double* tab = rec + (size_t)b * ((size_t)row_stride + 1) * 16;
  int* out = match + (size_t)b * ((size_t)row_stride + 2) * 4;
  int winners;
  const int n = em_rows(tab, row_stride, k_dev, b, sel_stride, winners);
  const long long g_lo = grp.g0[blockIdx.y];
  const int G = (int)(grp.g0[blockIdx.y + 1] - g_lo);
  if (blockIdx.x == 0 && threadIdx.x < 8) {   // the two header rows
    const int q = threadIdx.x;
    out[q] = q < 4 ? reinterpret_cast<const int*>(tab)[q] : q == 4 ? n : q == 5 ? G : q == 6 ? T : winners;
  }
  if (sel_row) sel_row += (size_t)b * (size_t)sel_stride;
  if (iou) iou += (size_t)b * (size_t)row_stride;
  gt_rect += 4 * g_lo;
  gt_class += g_lo;
  for (int i = blockIdx.x * EM_THREADS + threadIdx.x; i < n; i += gridDim.x * EM_THREADS) {
    const int w = sel_row ? sel_row[i] : i;
    int cls = 0, gt = 0;
    unsigned mask = 0u, cbits = 0u;
    double best = -1.0;
    if (w >= 0 && w < winners) {             // (a caller's table: never an index before it is checked)
      const double* r = tab + 16 * ((size_t)w + 1);
      cls = (int)r[0];
      cbits = __float_as_uint((float)r[2]);
      const double a0 = r[8], a1 = r[9], a2 = r[10], a3 = r[11];
      const double aw = a2 - a0, ah = a3 - a1;
      const double aa = aw * ah;
      if (cls >= 1) {
        for (int g = 0; g < G; ++g) {        // (uniform addresses: every lane walks the frame's boxes)
          if (gt_class[g] != cls) continue;
          const double v = em_iou(a0, a1, a2, a3, aa, gt_rect + 4 * (size_t)g);
          if (v > best) { best = v; gt = g + 1; }
        }
      }
      if (gt) {
#pragma unroll
        for (int t = 0; t < EM_MAX_T; ++t)
          if (t < T && best >= thr.v[t]) mask |= 1u << t;
      }
    }
    *reinterpret_cast<int4*>(out + 4 * ((size_t)i + 2)) = make_int4(cls, (int)cbits, (int)mask, gt);
    if (iou) iou[i] = best;
  }
}

__global__ __launch_bounds__(EM_THREADS) void eval_claim_kernel(EvalGroup grp, int T, int b0, int row_stride, int* __restrict__ match) {
  const int b = b0 + blockIdx.y;
  int* out = match + (size_t)b * ((size_t)row_stride + 2) * 4;
  const int n = min(out[4], row_stride);     // (what eval_best_kernel wrote for this frame, on this stream, before this launch)
  const int G = (int)(grp.g0[blockIdx.y + 1] - grp.g0[blockIdx.y]);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int* rows = out + 8;
  for (int g = blockIdx.x * EM_WAVES + wave; g < G; g += gridDim.x * EM_WAVES) {   // (wave-uniform)
    unsigned long long kmin[EM_MAX_T];
#pragma unroll
    for (int t = 0; t < EM_MAX_T; ++t) kmin[t] = ~0ull;
    for (int i = lane; i < n; i += 64) {
      if (rows[4 * (size_t)i + 3] != g + 1) continue;
      const unsigned mask = (unsigned)rows[4 * (size_t)i + 2];   // (a row of this box: only this wave writes it, below)
      const unsigned long long key =
          ((unsigned long long)(~em_image(__uint_as_float((unsigned)rows[4 * (size_t)i + 1]))) << 32) | (unsigned)i;
#pragma unroll
      for (int t = 0; t < EM_MAX_T; ++t)
        if (((mask >> t) & 1u) && key < kmin[t]) kmin[t] = key;
    }
#pragma unroll
    for (int t = 0; t < EM_MAX_T; ++t) {
      if (t < T) {
        for (int off = 32; off >= 1; off >>= 1) {
          const unsigned long long o = __shfl_xor(kmin[t], off, 64);
          if (o < kmin[t]) kmin[t] = o;
        }
      }
    }
    // (every lane's loads of the first walk have returned before the butterfly ran: the stores below cannot reach them)
    for (int i = lane; i < n; i += 64) {
      if (rows[4 * (size_t)i + 3] != g + 1) continue;
      unsigned won = 0u;
#pragma unroll
      for (int t = 0; t < EM_MAX_T; ++t)
        if (kmin[t] != ~0ull && (unsigned)(kmin[t] & 0xffffffffull) == (unsigned)i) won |= 1u << t;
      rows[4 * (size_t)i + 2] = (int)won;
    }
  }
}

__global__ __launch_bounds__(EM_THREADS) void eval_conf_rows_kernel(const double* __restrict__ rec, int row_stride,
                                                                    float* __restrict__ conf, int* __restrict__ count) {
  const int b = blockIdx.y;
  const double* tab = rec + (size_t)b * ((size_t)row_stride + 1) * 16;
  const int winners = min(max(reinterpret_cast<const int*>(tab)[3], 0), row_stride);
  if (blockIdx.x == 0 && threadIdx.x == 0) count[b] = winners;
  conf += (size_t)b * (size_t)row_stride;
  for (int i = blockIdx.x * EM_THREADS + threadIdx.x; i < winners; i += gridDim.x * EM_THREADS)
    conf[i] = (float)tab[16 * ((size_t)i + 1) + 2];
}

int eval_conf_rows(const double* rec, int B, int row_stride, float* conf, int* count, hipStream_t s) {
  FR_CHECK(B >= 0 && B <= 65535, "eval_conf_rows: %d frames (0 ... 65535)", B);
  FR_CHECK(row_stride >= 0 && row_stride <= EM_MAX_ROWS, "eval_conf_rows: row stride %d (0 ... %d)", row_stride, EM_MAX_ROWS);
  if (B == 0) return FRCNN_OK;
  FR_CHECK(rec && count && (conf || row_stride == 0), "eval_conf_rows: NULL argument");
  FR_CHECK((uintptr_t)rec % 8 == 0 && ((uintptr_t)conf | (uintptr_t)count) % 4 == 0,
           "eval_conf_rows: a pointer is not aligned to its element");
  const dim3 grid(std::max(1, std::min(cdiv(row_stride, EM_THREADS), std::max(1, EM_BLOCKS / B))), B);
  FR_LAUNCH(KC_NMS, 0, (double)B * row_stride * 12.0, s, eval_conf_rows_kernel, grid, dim3(EM_THREADS), 0, rec, row_stride, conf,
            count);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

int eval_match_batch(const double* rec, int B, int row_stride, const int* sel_row, long long sel_stride, const int* k_dev,
                     const double* gt_rect, const int* gt_class, const long long* gt_row0, const double* thr, int T, int* match,
                     double* iou, hipStream_t s) {
  // everything is checked before the first launch: a refused call has written nothing
  FR_CHECK(B >= 0 && B <= 65535, "eval_match_batch: %d frames (0 ... 65535)", B);
  FR_CHECK(row_stride >= 0 && row_stride <= EM_MAX_ROWS, "eval_match_batch: row stride %d (0 ... %d)", row_stride, EM_MAX_ROWS);
  FR_CHECK(T >= 1 && T <= EM_MAX_T, "eval_match_batch: %d IoU thresholds (1 ... %d)", T, EM_MAX_T);
  FR_CHECK(thr, "eval_match_batch: NULL thresholds");
  for (int t = 0; t < T; ++t) FR_CHECK(thr[t] == thr[t], "eval_match_batch: threshold %d is NaN", t);
  FR_CHECK(sel_stride >= 0, "eval_match_batch: negative selection stride %lld", sel_stride);
  if (B == 0) return FRCNN_OK;
  FR_CHECK(rec && match && gt_row0, "eval_match_batch: NULL argument (rec, match and the first rows are required)");
  FR_CHECK((sel_row == nullptr) == (k_dev == nullptr), "eval_match_batch: sel_row and k_dev come together");
  FR_CHECK(gt_row0[0] >= 0, "eval_match_batch: first ground-truth row %lld (negative)", gt_row0[0]);
  for (int b = 0; b < B; ++b) {
    FR_CHECK(gt_row0[b + 1] >= gt_row0[b], "eval_match_batch: the first rows are not ascending at frame %d (%lld, then %lld)", b,
             gt_row0[b], gt_row0[b + 1]);
    FR_CHECK(gt_row0[b + 1] - gt_row0[b] <= EM_MAX_G, "eval_match_batch: frame %d has %lld ground-truth boxes (at most %d)", b,
             gt_row0[b + 1] - gt_row0[b], EM_MAX_G);
  }
  FR_CHECK(gt_row0[B] == gt_row0[0] || (gt_rect && gt_class), "eval_match_batch: NULL ground truth");
  FR_CHECK(((uintptr_t)rec | (uintptr_t)gt_rect | (uintptr_t)iou) % 8 == 0 && (uintptr_t)match % 16 == 0 &&
               ((uintptr_t)sel_row | (uintptr_t)k_dev | (uintptr_t)gt_class) % 4 == 0,
           "eval_match_batch: a pointer is not aligned (match: 16 bytes, the others: their element)");
  EvalThr th;
  memset(&th, 0, sizeof(th));
  for (int t = 0; t < T; ++t) th.v[t] = thr[t];
  for (int b0 = 0; b0 < B; b0 += EM_GROUP) {
    const int nb = std::min(B - b0, EM_GROUP);
    EvalGroup g;
    memset(&g, 0, sizeof(g));
    long long gmax = 0;
    for (int i = 0; i <= nb; ++i) g.g0[i] = gt_row0[b0 + i];
    for (int i = 0; i < nb; ++i) gmax = std::max(gmax, g.g0[i + 1] - g.g0[i]);
    const int per = std::max(1, EM_BLOCKS / nb);
    const dim3 grid1(std::max(1, std::min(cdiv(row_stride, EM_THREADS), per)), nb);
    // (the rows are counted on the device: the profile's figures are those of full segments, an upper bound)
    const double rows = (double)nb * row_stride;
    FR_LAUNCH(KC_NMS, 30.0 * rows * (double)gmax, rows * 64.0 + (double)nb * gmax * 36.0, s, eval_best_kernel, grid1, dim3(EM_THREADS),
              0, g, th, T, b0, rec, row_stride, sel_row, sel_stride, k_dev, gt_rect, gt_class, match, iou);
    if (gmax > 0 && row_stride > 0) {
      const dim3 grid2(std::max(1, std::min(cdiv((int)gmax, EM_WAVES), per)), nb);
      FR_LAUNCH(KC_NMS, 0, 2.0 * rows * (double)gmax * 4.0, s, eval_claim_kernel, grid2, dim3(EM_THREADS), 0, g, T, b0, row_stride,
                match);
    }
  }
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
