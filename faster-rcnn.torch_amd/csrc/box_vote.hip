// box_vote.hip -- bounding-box voting (Gidaris & Komodakis 2015) behind the per-class pass of Detector: a winner's box becomes
// the score-weighted mean of every same-class survivor of the class test that overlaps it by at least `overlap`.  Not in the
// reference (a winner's r2 there is the one regressed box of the candidate that won); off unless cfg.box_voting asks for it.
//
//   winners of a segment: the 1-based rows pick[0 .. min(count, n)); for a winner row m, row j of the segment VOTES iff
//     cls[j] == cls[m] (every row without cls)  and  iou(j, m) >= overlap (a NaN IoU is no vote)  and  w_j is finite and > 0
//   w_j = 1 (weight_mode 0) | (double)score_j (1) | exp((double)score_j) (2: the score is a log-probability)
//   c_j = rect[j][0..3] (fp64) when rect is given, else (double)boxes[j][0..3]
//   rect_out[m][t] = (sum_j w_j c_j[t]) / (sum_j w_j) over the voters; votes_out[m] = their number;
//   fewer than two voters: rect_out[m] = c_m, bit for bit (m votes for itself through the same test as every other row)
//
// Arithmetic.  Membership is fp32, every operation rounded on its own (no contraction), area and IoU the box_area and box_iou of
// box_iou.h, which nms.hip and soft_nms.hip compute theirs with: who votes is a function of the inputs' bits.  The means are fp64: one product per
// voter and coordinate, sums in a FIXED order -- lane l of the winner's wave adds its rows l, l + 64, ... in ascending order
// into five accumulators (the four numerators and the denominator), then a __shfl_xor butterfly (32, 16, ... 1) adds the lanes
// -- and one division.  No atomics: a winner's result depends on its segment's data alone, not on the slot, the number of
// segments, the neighbours or the run.
//
// Shape: grid (groups of BV_WAVES winners, segment), one wave per winner.  Two tiers, chosen per segment from its DEVICE-side
// count n:
//   n <= BV_LDS_ROWS (2048)  the block stages the segment once in LDS, structure of arrays: weight (fp64), x1 y1 x2 y2, class
//                            -- 28 bytes a row, 56 KB at the cap; the exp of mode 2 is computed once per row of the block, not
//                            once per pair.  The launch asks for the LDS of min(n_cap, BV_LDS_ROWS) rows only.
//   larger                   the waves read the rows from global memory (a 16 384-row segment is under 1 MB and sits in L2) and
//                            compute a weight only for the rows that pass the class and IoU tests.
// The averaged coordinates come from global memory in both tiers: only voters need them.  A block takes the winner groups
// blockIdx.x, blockIdx.x + gridDim.x, ...; the grid has one block per group up to BV_MAX_GRID_X, so there is no bound on the
// rows of a segment other than int.
#pragma clang fp contract(off)
#include "kernels.h"
#include "box_iou.h"

namespace frcnn {

#define BV_LANES 64                        // rows lane l takes: l, l + BV_LANES, ...
#define BV_WAVES 4                         // winners per block (one wave each)
#define BV_THREADS (BV_LANES * BV_WAVES)
#define BV_LDS_ROWS 2048                   // largest segment staged in LDS
#define BV_LDS_ROW_BYTES 28                // weight 8, box 16, class 4
#define BV_MAX_GRID_X 4096                 // blocks per segment; beyond it a block takes several winner groups

// the weight of a row; a row votes only when it is finite and > 0
__device__ __forceinline__ double bv_weight(int weight_mode, const float* __restrict__ row, int score_col) {
  if (weight_mode == 0) return 1.0;
  const double s = (double)row[score_col - 1];
  return weight_mode == 1 ? s : exp(s);
}

__device__ __forceinline__ bool bv_votes(double w) { return w > 0.0 && w < __builtin_inf(); }

__global__ __launch_bounds__(BV_THREADS) void box_vote_batch_kernel(const float* __restrict__ boxes, long row_stride, int n_cap,
                                                                    const int* __restrict__ n_dev, int ncols, int score_col,
                                                                    int weight_mode, float overlap, const int* __restrict__ cls,
                                                                    const double* __restrict__ rect,
                                                                    const long long* __restrict__ pick,
                                                                    const int* __restrict__ count, double* __restrict__ rect_out,
                                                                    int* __restrict__ votes_out, int lds_rows) {
  extern __shared__ double bv_lds[];
  const int b = blockIdx.y;
  const int n = min(n_dev[b], n_cap);
  const int nwin = min(count[b], n);
  if ((long)blockIdx.x * BV_WAVES >= (long)nwin) return;   // (uniform over the block; covers n <= 0 and count <= 0)
  const size_t so = (size_t)b * (size_t)row_stride;
  boxes += so * ncols;
  if (cls) cls += so;
  if (rect) rect += so * 4;
  pick += so;
  rect_out += so * 4;
  if (votes_out) votes_out += so;

  const int tid = threadIdx.x, lane = tid & (BV_LANES - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / BV_LANES);
  const bool staged = n <= lds_rows;   // (uniform; lds_rows = min(n_cap, BV_LDS_ROWS), a multiple of 4 after rounding up)
  const int R = (lds_rows + 3) & ~3;
  double* lw = bv_lds;
  float* lx1 = reinterpret_cast<float*>(lw + R);
  float* ly1 = lx1 + R;
  float* lx2 = ly1 + R;
  float* ly2 = lx2 + R;
  int* lcl = reinterpret_cast<int*>(ly2 + R);
  if (staged) {
    for (int i = tid; i < n; i += BV_THREADS) {
      const float* r = boxes + (size_t)i * ncols;
      lx1[i] = r[0]; ly1[i] = r[1]; lx2[i] = r[2]; ly2[i] = r[3];
      lcl[i] = cls ? cls[i] : 0;
      lw[i] = bv_weight(weight_mode, r, score_col);
    }
    __syncthreads();
  }

  for (long q = (long)blockIdx.x * BV_WAVES + wave; q < (long)nwin; q += (long)gridDim.x * BV_WAVES) {
    const long m = (long)pick[q] - 1;
    if (m < 0 || m >= (long)n) continue;   // (not a row of the segment: nothing is read or stored for it)
    float mx1, my1, mx2, my2;
    int mc;
    if (staged) { mx1 = lx1[m]; my1 = ly1[m]; mx2 = lx2[m]; my2 = ly2[m]; mc = lcl[m]; }
    else {
      const float* r = boxes + (size_t)m * ncols;
      mx1 = r[0]; my1 = r[1]; mx2 = r[2]; my2 = r[3];
      mc = cls ? cls[m] : 0;
    }
    const float ma = box_area(mx1, my1, mx2, my2);
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int votes = 0;
    for (long j = lane; j < (long)n; j += BV_LANES) {
      float jx1, jy1, jx2, jy2;
      int jc;
      const float* r = boxes + (size_t)j * ncols;
      if (staged) { jx1 = lx1[j]; jy1 = ly1[j]; jx2 = lx2[j]; jy2 = ly2[j]; jc = lcl[j]; }
      else {
        jx1 = r[0]; jy1 = r[1]; jx2 = r[2]; jy2 = r[3];
        jc = cls ? cls[j] : 0;
      }
      if (jc != mc) continue;
      const float iou = box_iou(jx1, jy1, jx2, jy2, box_area(jx1, jy1, jx2, jy2), mx1, my1, mx2, my2, ma);
      if (!(iou >= overlap)) continue;
      const double w = staged ? lw[j] : bv_weight(weight_mode, r, score_col);
      if (!bv_votes(w)) continue;
      double c0, c1, c2, c3;
      if (rect) {
        const double* c = rect + 4 * (size_t)j;
        c0 = c[0]; c1 = c[1]; c2 = c[2]; c3 = c[3];
      } else {
        c0 = (double)jx1; c1 = (double)jy1; c2 = (double)jx2; c3 = (double)jy2;
      }
      const double p0 = w * c0, p1 = w * c1, p2 = w * c2, p3 = w * c3;
      sw = sw + w;
      s0 = s0 + p0; s1 = s1 + p1; s2 = s2 + p2; s3 = s3 + p3;
      ++votes;
    }
#pragma unroll
    for (int off = BV_LANES / 2; off >= 1; off >>= 1) {
      sw = sw + __shfl_xor(sw, off, BV_LANES);
      s0 = s0 + __shfl_xor(s0, off, BV_LANES);
      s1 = s1 + __shfl_xor(s1, off, BV_LANES);
      s2 = s2 + __shfl_xor(s2, off, BV_LANES);
      s3 = s3 + __shfl_xor(s3, off, BV_LANES);
      votes = votes + __shfl_xor(votes, off, BV_LANES);
    }
    if (lane == 0) {
      double o0, o1, o2, o3;
      if (votes >= 2) {
        o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw; o3 = s3 / sw;
      } else if (rect) {
        const double* c = rect + 4 * (size_t)m;
        o0 = c[0]; o1 = c[1]; o2 = c[2]; o3 = c[3];
      } else {
        o0 = (double)mx1; o1 = (double)my1; o2 = (double)mx2; o3 = (double)my2;
      }
      double* o = rect_out + 4 * (size_t)m;
      o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
      if (votes_out) votes_out[m] = votes;
    }
  }
}

int box_vote_batch(const float* boxes, int B, long row_stride, int n_cap, const int* n_dev, int ncols, int score_col,
                   int weight_mode, float overlap, const int* cls, const double* rect, const long long* pick, const int* count,
                   double* rect_out, int* votes_out, hipStream_t s) {
  FR_CHECK(B >= 1 && B <= 65535, "box_vote: %d segments (1 .. 65535)", B);
  FR_CHECK(boxes && n_dev && pick && count && rect_out,
           "box_vote: NULL argument (boxes, n_dev, pick, count and rect_out are required)");
  FR_CHECK(n_cap >= 0, "box_vote: %d rows per segment", n_cap);
  FR_CHECK(row_stride >= n_cap, "box_vote: row stride %ld < %d rows per segment", row_stride, n_cap);
  FR_CHECK(ncols >= 4, "box_vote: rows need >= 4 columns (got %d)", ncols);
  FR_CHECK(weight_mode >= 0 && weight_mode <= 2, "box_vote: bad weight_mode %d (0 uniform, 1 score, 2 exp(score))", weight_mode);
  FR_CHECK(weight_mode == 0 || (score_col >= 5 && score_col <= ncols), "box_vote: score column %d outside [5, %d]", score_col,
           ncols);
  FR_CHECK(overlap > 0.f && overlap <= 1.f, "box_vote: overlap = %g (must be in (0, 1])", (double)overlap);
  if (n_cap == 0) return FRCNN_OK;
  const int lds_rows = std::min(n_cap, BV_LDS_ROWS);
  const size_t lds = (size_t)((lds_rows + 3) & ~3) * BV_LDS_ROW_BYTES;
  const int gx = (int)std::min(cdivl(n_cap, BV_WAVES), (long)BV_MAX_GRID_X);
  // (the work of a launch in which every row wins: n_cap pair tests of some 30 operations per winner)
  FR_LAUNCH(KC_NMS, 30.0 * B * (double)n_cap * n_cap, 28.0 * B * (double)n_cap, s, box_vote_batch_kernel, dim3(gx, B),
            dim3(BV_THREADS), lds, boxes, row_stride, n_cap, n_dev, ncols, score_col, weight_mode, overlap, cls, rect, pick, count,
            rect_out, votes_out, lds_rows);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
