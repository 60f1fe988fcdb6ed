// detect.hip -- the glue of Detector:detect (Detector.lua:17-141) kept ON THE DEVICE between its big steps, so that a
// frame needs two read-backs instead of a dozen:
//   roi_windows   extract_roi_pooling_input (objective.lua:5-13) for every NMS candidate: Localizer:inputToFeatureRect
//                 (Localizer.lua:41-67) in the reference's double arithmetic, clip, 1-based window -- one thread per ROI
//   detect_post   Detector.lua:106-122: class test (class != background and p > 0.2), r2 = Anchors.anchorToInput(r, bbox)
//                 in double, ORDERED compaction of the survivors into the box / class arrays the per-class NMS reads;
//                 the survivor count stays on the device (frcnn_nms_device_n reads it there)
//   detect_classes_batch  the class test of a chunk of B frames in ONE launch, straight from the net's log-probabilities
//                 (the arg-max of frcnn_cnet_decode folded in): mode 0 the rule above, one row per candidate at most; mode 1
//                 one row per (candidate, foreground class) whose probability clears the threshold
//   detect_merge_views  test-time augmentation: the survivors of a frame's V views (V segments) as ONE segment in the frame's
//                 coordinates, the views' picks rebased for the gather -- one launch per chunk, no atomics
//   detect_gather_batch  one table per frame: its counts, then one record per winner (class, candidate row, confidence, p,
//                 anchor rect, decoded rect, anchor index)
// Gather / scan work on a few thousand rows: latency-bound, no MFMA.  Double arithmetic follows the host mirror
// operation by operation; FMA contraction is off for this translation unit (products and sums separately rounded, as
// Lua numbers are).  exp() is the device library's double exp: it may differ from the host libm in the last bit (both
// are within an ulp), far inside the 1e-3 bar the decoded rects are compared at.
#pragma clang fp contract(off)
#include <cmath>

#include "kernels.h"
#include "anchor_decode.h"

namespace frcnn {

struct LocLayers { int n; int l[24][6]; };   // {kW, kH, dW, dH, padW, padH} per layer, input first

__device__ __forceinline__ double lua_mod(double a, double b) { return a - floor(a / b) * b; }   // Lua 5.1: a - floor(a/b)*b

// rect [n][4] double (input space); pick (optional) 1-based rows of rect; wins [k][4] = {row_lo, row_hi, col_lo, col_hi}
__global__ void roi_windows_kernel(const double* __restrict__ rect, const long long* __restrict__ pick, int k, LocLayers L,
                                   int fmH, int fmW, int* __restrict__ wins) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= k) return;
  const double* q = rect + 4 * (pick ? (size_t)(pick[r] - 1) : (size_t)r);
  double minX = q[0], minY = q[1], maxX = q[2], maxY = q[3];
  for (int i = 0; i < L.n; ++i) {   // Localizer.lua:44-64 (the dH / dW mix-ups are the reference's)
    const double kW = L.l[i][0], kH = L.l[i][1], dW = L.l[i][2], dH = L.l[i][3], padW = L.l[i][4], padH = L.l[i][5];
    if (dW < kW) { minX -= kW - dW; minY -= kH - dH; maxX += kW - dW; maxY += kH - dH; }
    minX += padW; minY += padH; maxX += padW; maxY += padH;
    minX = minX / dH;
    minY = minY / dH;
    const double ax = maxX - kW;
    maxX = fmax(lua_mod(ax, dW) == 0.0 ? ax / dW + 1.0 : ceil(ax / dW) + 1.0, minX + 1.0);
    const double ay = maxY - kH;
    maxY = fmax(lua_mod(ay, dH) == 0.0 ? ay / dW + 1.0 : ceil(ay / dH) + 1.0, minY + 1.0);
  }
  minX = floor(minX); minY = floor(minY); maxX = ceil(maxX); maxY = ceil(maxY);   // :66 snapToInt
  // Rect.clip to [0, W] x [0, H] (Rect.lua:73-80), then objective.lua:11
  minX = fmin(fmax(minX, 0.0), (double)fmW); minY = fmin(fmax(minY, 0.0), (double)fmH);
  maxX = fmax(fmin(maxX, (double)fmW), 0.0); maxY = fmax(fmin(maxY, (double)fmH), 0.0);
  int* w = wins + 4 * r;
  w[0] = (int)fmin(minY + 1.0, maxY); w[1] = (int)maxY; w[2] = (int)fmin(minX + 1.0, maxX); w[3] = (int)maxX;
}

int roi_windows(const double* rect, const long long* pick, int k, const int* layers, int nlayers, int fmH, int fmW, int* wins,
                hipStream_t s) {
  if (k <= 0) return FRCNN_OK;
  FR_CHECK(nlayers >= 0 && nlayers <= 24, "roi_windows: %d localizer layers (at most 24)", nlayers);
  LocLayers L;
  L.n = nlayers;
  for (int i = 0; i < nlayers; ++i)
    for (int j = 0; j < 6; ++j) L.l[i][j] = layers[6 * i + j];
  FR_LAUNCH(KC_ROI, 0, k * 48.0, s, roi_windows_kernel, dim3(cdiv(k, 64)), dim3(64), 0, rect, pick, k, L, fmH, fmW, wins);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// (anchor_to_input -- Anchors.anchorToInput, Anchors.lua:245-252 -- lives in anchor_decode.h: class_boxes.hip decodes with it too)

// One block, ordered compaction.  For candidate r (row pick[r] of the match arrays): keep iff cls != bgclass and
// exp(conf) > min_conf.  Survivor j (in candidate order): bb[j] = {float(r2), conf}, kc[j] = class, keep_row[j] = r,
// r2[j] = decoded rect in double; *K_dev = number of survivors.
#define DP_THREADS 1024
__global__ __launch_bounds__(DP_THREADS) void detect_post_kernel(const int* __restrict__ cls, const float* __restrict__ conf,
                                                                 const float* __restrict__ bbox, const double* __restrict__ rect,
                                                                 const long long* __restrict__ pick, int R, int bgclass,
                                                                 double min_conf, float* __restrict__ bb, int* __restrict__ kc,
                                                                 int* __restrict__ keep_row, double* __restrict__ r2out,
                                                                 int* __restrict__ K_dev) {
  __shared__ int wsum[DP_THREADS / 64];
  __shared__ int base;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = 0; r0 < R; r0 += DP_THREADS) {
    const int r = r0 + threadIdx.x;
    bool keep = false;
    if (r < R) keep = cls[r] != bgclass && exp((double)conf[r]) > min_conf;   // Detector.lua:115
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (keep) {
      const int j = off + before;
      double q[4];
      anchor_to_input(rect + 4 * (size_t)(pick[r] - 1), bbox + 4 * (size_t)r, q);   // the anchor's input rect (Detector.lua:106)
      const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3];
      r2out[4 * (size_t)j] = x0; r2out[4 * (size_t)j + 1] = y0; r2out[4 * (size_t)j + 2] = x1; r2out[4 * (size_t)j + 3] = y1;
      float* b = bb + 5 * (size_t)j;               // r.r2:totensor() (FloatTensor) + the confidence column
      b[0] = (float)x0; b[1] = (float)y0; b[2] = (float)x1; b[3] = (float)y1; b[4] = conf[r];
      kc[j] = cls[r];
      keep_row[j] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < DP_THREADS / 64; ++w) tot += wsum[w];
      base += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *K_dev = base;
}

int detect_post(const int* cls, const float* conf, const float* bbox, const double* rect, const long long* pick, int R,
                int bgclass, double min_conf, float* bb, int* kc, int* keep_row, double* r2, int* K_dev, hipStream_t s) {
  if (R <= 0) { FR_HIP(hipMemsetAsync(K_dev, 0, sizeof(int), s)); return FRCNN_OK; }
  FR_LAUNCH(KC_ELEMWISE, 0, R * 64.0, s, detect_post_kernel, dim3(1), dim3(DP_THREADS), 0, cls, conf, bbox, rect, pick, R, bgclass,
            min_conf, bb, kc, keep_row, r2, K_dev);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---- The class test of B frames in one launch (Detector:detect_batch under cfg.scoring), from the net's outputs as they lie:
// frame b's R[b] candidates are rows row0[b] ... of lsm (ncls log-probabilities a row) and of bbox.  R and row0 are host values and
// travel BY VALUE as a kernel argument, in groups of at most DC_GROUP frames (the way rpn_scan_ragged carries its descriptors): no
// table upload, no copy, no wait.
// One workgroup per frame, tiles of DC_THREADS candidates, one candidate per thread.  The 64 candidates of a wave own 64 * ncls
// CONTIGUOUS floats; the wave moves them through its own LDS tile DC_CLS classes at a time -- DC_CLS consecutive lanes load the
// DC_CLS consecutive floats of one candidate, so a load touches 8 runs of 32 bytes, not 64 rows, and every 128-byte line is used
// up by the wave's next rounds -- and a lane then reads its own candidate's values from the tile (walk_row; rows of DC_CLS + 1
// floats: no bank conflicts).  Two walks per tile of candidates: the first counts a candidate's rows (mode 0: the first maximum,
// exactly cnet_decode_kernel, then the test of detect_post_kernel: 0 or 1; mode 1: every class c != bgclass with
// exp(lp[c]) > min_conf: 0 ... ncls - 1); a wave prefix sum and the cross-wave sums in LDS turn the counts into row numbers
// (ordered: candidate-major, c ascending); the second walk (mode 1) stores the rows.  r2 is decoded ONCE per candidate with a
// row.  No atomics: a frame's output is a function of its own data.  Rows at and behind row_stride are counted, not stored.
#define DC_THREADS 1024
#define DC_CLS 8       // classes a round of walk_row
constexpr int DC_GROUP = 32;
struct ClassFrame { long long row0; int R; };
struct ClassGroup { ClassFrame f[DC_GROUP]; };
static_assert(sizeof(ClassGroup) <= 1024, "the descriptors of a group travel as a kernel argument");

// f(c, v) for c = 0 ... ncls - 1, v = span[lane * ncls + c], in order, on the lanes < cands: `span` is the wave's part of lsm
// (cands <= 64 candidates), `tile` its LDS tile.  Every wave of the block makes the same rounds (the barriers are the block's).
template <class F>
__device__ __forceinline__ void walk_row(const float* __restrict__ span, int cands, int ncls, int lane, float* tile, F f) {
  for (int c0 = 0; c0 < ncls; c0 += DC_CLS) {
    const int nc = min(DC_CLS, ncls - c0);
    __syncthreads();
    for (int i = lane; i < 64 * DC_CLS; i += 64) {
      const int t = i / DC_CLS, cc = i % DC_CLS;
      if (t < cands && cc < nc) tile[t * (DC_CLS + 1) + cc] = span[(size_t)t * ncls + c0 + cc];
    }
    __syncthreads();
    if (lane < cands)
      for (int cc = 0; cc < nc; ++cc) f(c0 + cc, tile[lane * (DC_CLS + 1) + cc]);
  }
}

__global__ __launch_bounds__(DC_THREADS) void detect_classes_batch_kernel(
    ClassGroup g, int b0, const float* __restrict__ lsm, const float* __restrict__ bbox, const double* __restrict__ rect,
    const long long* __restrict__ pick, long long match_stride, int ncls, int bgclass, double min_conf, int mode,
    float* __restrict__ bb, int* __restrict__ kc, int* __restrict__ keep_row, double* __restrict__ r2out, int row_stride,
    int* __restrict__ K_dev, int* __restrict__ total_dev) {
  __shared__ float tiles[DC_THREADS / 64][64 * (DC_CLS + 1)];
  __shared__ int wsum[DC_THREADS / 64];
  __shared__ int base;
  const int b = b0 + blockIdx.x;
  const int R = g.f[blockIdx.x].R;
  const size_t first = (size_t)g.f[blockIdx.x].row0;
  lsm += first * ncls; bbox += first * 4;
  rect += (size_t)b * match_stride * 4; pick += (size_t)b * match_stride;
  const size_t so = (size_t)b * row_stride;
  bb += so * 5; kc += so; keep_row += so; r2out += so * 4;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = tiles[wave];
  for (int r0 = 0; r0 < R; r0 += DC_THREADS) {
    const int r = r0 + threadIdx.x, rw = r0 + wave * 64;     // the thread's candidate, the wave's first
    const float* span = lsm + (size_t)min(rw, R) * ncls;
    const int cands = max(min(R - rw, 64), 0);
    int cnt = 0, best = 0;
    float bestv = 0.0f;
    walk_row(span, cands, ncls, lane, tile, [&](int c, float v) {
      if (mode == 0) {
        if (c == 0 || v > bestv) { best = c; bestv = v; }      // torch.sort(cprob, 1, true)[1]: the first maximum
      } else {
        cnt += c + 1 != bgclass && exp((double)v) > min_conf;
      }
    });
    if (mode == 0 && r < R) cnt = best + 1 != bgclass && exp((double)bestv) > min_conf;   // Detector.lua:115
    // rows before this thread's: inclusive wave scan, then the waves before this one
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int j = base + incl - cnt;
    for (int w = 0; w < wave; ++w) j += wsum[w];
    const bool stores = cnt > 0 && j < row_stride;
    double q[4];
    if (stores) anchor_to_input(rect + 4 * (size_t)(pick[r] - 1), bbox + 4 * (size_t)r, q);
    auto emit = [&](int c, float v) {
      if (j < row_stride) {
        double* o = r2out + 4 * (size_t)j;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
        float* x = bb + 5 * (size_t)j;
        x[0] = (float)q[0]; x[1] = (float)q[1]; x[2] = (float)q[2]; x[3] = (float)q[3]; x[4] = v;
        kc[j] = c + 1;
        keep_row[j] = r;
      }
      ++j;
    };
    if (mode == 0) {
      if (stores) emit(best, bestv);
    } else {   // (the second walk: the rows come from cache)
      walk_row(span, cands, ncls, lane, tile, [&](int c, float v) {
        if (stores && c + 1 != bgclass && exp((double)v) > min_conf) emit(c, v);
      });
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < DC_THREADS / 64; ++w) tot += wsum[w];
      base += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    K_dev[b] = min(base, row_stride);
    if (total_dev) total_dev[b] = base;
  }
}

int detect_classes_batch(const float* cls_out, const float* bbox, const int* R, const long long* row0, int B, const double* rect,
                         const long long* pick, long long match_stride, int ncls, int bgclass, double min_conf, int mode, float* bb,
                         int* kc, int* keep_row, double* r2, int row_stride, int* K_dev, int* total_dev, hipStream_t s) {
  if (B == 0) return FRCNN_OK;
  // everything is checked before the first launch: a refused call has written nothing
  FR_CHECK(B > 0 && B <= 65535, "detect_classes_batch: %d frames (0 ... 65535)", B);
  FR_CHECK(ncls >= 2, "detect_classes_batch: %d classes (at least 2: one and the background)", ncls);
  FR_CHECK(bgclass >= 1 && bgclass <= ncls, "detect_classes_batch: background class %d (1 ... %d)", bgclass, ncls);
  FR_CHECK(mode == 0 || mode == 1, "detect_classes_batch: mode %d (0: top class, 1: all classes)", mode);
  FR_CHECK(row_stride >= 0 && match_stride >= 0, "detect_classes_batch: negative stride (%d / %lld)", row_stride, match_stride);
  FR_CHECK(R && row0 && K_dev, "detect_classes_batch: NULL argument");
  double rows = 0;
  for (int b = 0; b < B; ++b) {
    FR_CHECK(R[b] >= 0 && row0[b] >= 0, "detect_classes_batch: frame %d has R %d, row0 %lld (negative)", b, R[b], row0[b]);
    FR_CHECK((long long)R[b] * ncls <= 0x7fffffffLL, "detect_classes_batch: frame %d: %d x %d log-probabilities", b, R[b], ncls);
    rows += R[b];
  }
  FR_CHECK(rows == 0 || (cls_out && bbox && rect && pick), "detect_classes_batch: NULL argument");
  FR_CHECK(rows == 0 || row_stride == 0 || (bb && kc && keep_row && r2), "detect_classes_batch: NULL output");
  for (int b0 = 0; b0 < B; b0 += DC_GROUP) {
    const int nb = std::min(B - b0, DC_GROUP);
    ClassGroup g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < nb; ++i) { g.f[i].row0 = row0[b0 + i]; g.f[i].R = R[b0 + i]; }
    FR_LAUNCH(KC_ELEMWISE, 0, rows * (ncls * 4.0 + 64.0), s, detect_classes_batch_kernel, dim3(nb), dim3(DC_THREADS), 0, g, b0,
              cls_out, bbox, rect, pick, match_stride, ncls, bgclass, min_conf, mode, bb, kc, keep_row, r2, row_stride, K_dev,
              total_dev);
  }
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---- Test-time augmentation (cfg.tta): the class-test survivors of a frame's V views -- V consecutive segments of the chunk --
// become ONE segment of V * row_stride rows in the frame's own coordinates, in view order and in row order within a view.  A
// view's geometry (mirrored or not, its width, the two factors back to the frame) and its candidate count are HOST values and
// travel by value as a kernel argument, MV_VIEWS views a launch (the way detect_classes_batch carries its descriptors).  Grid
// (row tiles, V, frames): thread j of view v stores survivor j at the prefix of the views' device counts in front of it (at most
// 7 loads: no scan, no atomics), and candidate j's pick at the prefix of the candidate counts, rebased by v * match_stride so that
// detect_gather_batch finds the view's match rows behind it unchanged.  Coordinates in fp64, one rounding per operation:
// BatchIterator.lua:57-62 backwards (x1' = Wv - x2, x2' = Wv - x1), then x * ax, y * ay; a factor of exactly 1 is not applied.
#define MV_THREADS 256
constexpr int MV_MAX_V = 8;
constexpr int MV_VIEWS = 64;
struct MergeView { double Wv, ax, ay; int flip, R, Roff, pad; };
struct MergeGroup { MergeView v[MV_VIEWS]; };
static_assert(sizeof(MergeGroup) <= 3072, "the descriptors of a group travel as a kernel argument");

__global__ __launch_bounds__(MV_THREADS) void detect_merge_views_kernel(
    MergeGroup g, int f0, int F, int V, const float* __restrict__ bb, const int* __restrict__ kc, const int* __restrict__ keep_row,
    const double* __restrict__ r2, long long row_stride, const int* __restrict__ counts, const long long* __restrict__ pick,
    long long match_stride, float* __restrict__ bb_out, int* __restrict__ kc_out, int* __restrict__ keep_row_out,
    double* __restrict__ r2_out, long long* __restrict__ pick_out, int* __restrict__ counts_out) {
  const int v = blockIdx.y, f = f0 + blockIdx.z;
  const long long j = (long long)blockIdx.x * MV_THREADS + threadIdx.x;
  const int S = F * V;                                   // segments of the chunk: counts is int[4][S]
  const MergeView* views = g.v + (size_t)blockIdx.z * V;
  const MergeView d = views[v];
  const int* n_dev = counts + (size_t)f * V;             // the views' match counts; their survivor counts at + 2 * S
  auto survivors = [&](int u) { return (long long)min(max(n_dev[2 * S + u], 0), (int)row_stride); };   // (V * row_stride fits an int)
  long long before = 0;
  for (int u = 0; u < v; ++u) before += survivors(u);
  if (v == 0 && j == 0) {
    long long matches = 0, cand = 0, K = 0;
    for (int u = 0; u < V; ++u) { matches += n_dev[u]; cand += views[u].R; K += survivors(u); }
    counts_out[f] = (int)matches; counts_out[F + f] = (int)cand; counts_out[2 * F + f] = (int)K;
  }
  const size_t seg = (size_t)f * V + v;
  if (j < d.R)
    pick_out[(size_t)f * V * match_stride + d.Roff + j] = (long long)v * match_stride + pick[seg * match_stride + j];
  if (j >= survivors(v)) return;
  const size_t src = seg * row_stride + j, dst = (size_t)f * V * row_stride + before + j;
  double x1 = r2[4 * src], y1 = r2[4 * src + 1], x2 = r2[4 * src + 2], y2 = r2[4 * src + 3];
  if (d.flip) {
    const double a = d.Wv - x2, b = d.Wv - x1;
    x1 = a; x2 = b;
  }
  if (d.ax != 1.0) { x1 = x1 * d.ax; x2 = x2 * d.ax; }
  if (d.ay != 1.0) { y1 = y1 * d.ay; y2 = y2 * d.ay; }
  double* o = r2_out + 4 * dst;
  o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
  float* x = bb_out + 5 * dst;
  x[0] = (float)x1; x[1] = (float)y1; x[2] = (float)x2; x[3] = (float)y2; x[4] = bb[5 * src + 4];
  kc_out[dst] = kc[src];
  keep_row_out[dst] = d.Roff + keep_row[src];
}

int detect_merge_views(const float* bb, const int* kc, const int* keep_row, const double* r2, long long row_stride,
                       const int* counts, const long long* pick, long long match_stride, int F, int V, const int* flip,
                       const double* Wv, const double* ax, const double* ay, const int* R, float* bb_out, int* kc_out,
                       int* keep_row_out, double* r2_out, long long* pick_out, int* counts_out, hipStream_t s) {
  // everything is checked before the first launch: a refused call has written nothing
  FR_CHECK(F >= 1 && F <= 65535, "detect_merge_views: %d frames (1 ... 65535)", F);
  FR_CHECK(V >= 1 && V <= MV_MAX_V, "detect_merge_views: %d views a frame (1 ... %d)", V, MV_MAX_V);
  FR_CHECK(row_stride >= 0 && match_stride >= 0, "detect_merge_views: negative stride (%lld / %lld)", row_stride, match_stride);
  FR_CHECK(row_stride * V <= 0x7fffffffLL && match_stride * V <= 0x7fffffffLL, "detect_merge_views: %d views of %lld / %lld rows",
           V, row_stride, match_stride);
  FR_CHECK(flip && Wv && ax && ay && R && counts && counts_out, "detect_merge_views: NULL argument");
  long long rmax = 0;
  for (int i = 0; i < F * V; ++i) {
    FR_CHECK(std::isfinite(Wv[i]) && Wv[i] > 0 && std::isfinite(ax[i]) && ax[i] > 0 && std::isfinite(ay[i]) && ay[i] > 0,
             "detect_merge_views: view %d of frame %d has width %g, factors %g / %g (finite and positive)", i % V, i / V, Wv[i],
             ax[i], ay[i]);
    FR_CHECK(R[i] >= 0 && R[i] <= match_stride, "detect_merge_views: view %d of frame %d has %d candidates (0 ... %lld)", i % V,
             i / V, R[i], match_stride);
    rmax = std::max(rmax, (long long)R[i]);
  }
  FR_CHECK(rmax == 0 || (pick && pick_out), "detect_merge_views: NULL pick");
  FR_CHECK(row_stride == 0 || (bb && kc && keep_row && r2 && bb_out && kc_out && keep_row_out && r2_out),
           "detect_merge_views: NULL argument");
  const int tiles = (int)std::max(cdivl((long)std::max(row_stride, rmax), MV_THREADS), 1L);
  const int per = MV_VIEWS / V;                          // frames a launch
  for (int f0 = 0; f0 < F; f0 += per) {
    const int nf = std::min(F - f0, per);
    MergeGroup g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < nf; ++i) {
      int off = 0;
      for (int v = 0; v < V; ++v) {
        const int k = (f0 + i) * V + v;
        MergeView& d = g.v[i * V + v];
        d.Wv = Wv[k]; d.ax = ax[k]; d.ay = ay[k]; d.flip = flip[k] != 0; d.R = R[k]; d.Roff = off;
        off += R[k];
      }
    }
    FR_LAUNCH(KC_ELEMWISE, 0, (double)nf * V * (row_stride * 112.0 + rmax * 16.0), s, detect_merge_views_kernel,
              dim3(tiles, V, nf), dim3(MV_THREADS), 0, g, f0, F, V, bb, kc, keep_row, r2, row_stride, counts, pick, match_stride,
              bb_out, kc_out, keep_row_out, r2_out, pick_out, counts_out);
  }
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// The winner tables of B frames in one launch (Detector:detect_batch; Detector:detect is B = 1), all in ONE buffer: frame b's table
// is rec + b * (row_stride + 1) * 16 doubles -- a 128-byte header whose first four ints are the frame's counts (matches,
// candidates, survivors of the class test, winners: counts[k * B + b]), then one record of 16 doubles per winner, in the pick
// order of the per-class NMS:
//   0 class, 1 candidate row (1-based, among the NMS candidates), 2 confidence (log-prob), 3 p (log-prob of the anchor),
//   4-7 anchor rect, 8-11 r2, 12-15 anchor index {layer, aspect, y, x}
// The per-candidate arrays (wpick, keep_row, kc, bb, r2) hold row_stride rows per frame, the match arrays (pick, mp, rect, midx)
// match_stride rows.
__global__ void detect_gather_batch_kernel(const long long* __restrict__ wpick, const int* __restrict__ counts, int B, int row_stride,
                                           const int* __restrict__ keep_row, const int* __restrict__ kc, const float* __restrict__ bb,
                                           const double* __restrict__ r2, const long long* __restrict__ pick, long match_stride,
                                           const float* __restrict__ mp, const double* __restrict__ rect,
                                           const int* __restrict__ midx, double* __restrict__ rec) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  double* tab = rec + (size_t)b * ((size_t)row_stride + 1) * 16;
  if (q < 4) reinterpret_cast<int*>(tab)[q] = counts[q * B + b];
  if (q >= min(counts[3 * B + b], row_stride)) return;
  const size_t so = (size_t)b * row_stride, mo = (size_t)b * match_stride;
  const size_t j = so + (size_t)(wpick[so + q] - 1);
  const int r = keep_row[j];
  const size_t i = mo + (size_t)(pick[mo + r] - 1);
  double* o = tab + 16 * ((size_t)q + 1);
  o[0] = kc[j]; o[1] = r + 1; o[2] = bb[5 * j + 4]; o[3] = mp[i];
  for (int t = 0; t < 4; ++t) { o[4 + t] = rect[4 * i + t]; o[8 + t] = r2[4 * j + t]; o[12 + t] = midx[4 * i + t]; }
}

int detect_gather_batch(const long long* wpick, const int* counts, int B, int row_stride, const int* keep_row, const int* kc,
                        const float* bb, const double* r2, const long long* pick, long match_stride, const float* mp,
                        const double* rect, const int* midx, double* rec, hipStream_t s) {
  if (B <= 0) return FRCNN_OK;
  FR_CHECK(B <= 65535 && row_stride >= 0 && match_stride >= 0, "detect_gather_batch: bad sizes (B %d, strides %d / %ld)", B,
           row_stride, match_stride);
  // (row_stride == 0: one block per frame still writes the header)
  FR_LAUNCH(KC_ELEMWISE, 0, B * (row_stride + 1) * 128.0, s, detect_gather_batch_kernel, dim3(std::max(cdiv(row_stride, 64), 1), B),
            dim3(64), 0, wpick, counts, B, row_stride, keep_row, kc, bb, r2, pick, match_stride, mp, rect, midx, rec);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
