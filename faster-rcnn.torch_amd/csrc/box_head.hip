// box_head.hip -- the per-class box head of the classification net (cfg.box_head.per_class; include/frcnn_hip_box.h).
// A Linear(nf, 4 C) of which every row of the batch uses the four weight rows of ONE class: a class-indexed (grouped) product,
// not a dense one -- a dense R x 4C GEMM would throw away all but 4 of its 4C columns.  Three kernels, no atomics, no workspace
// beyond the int sel[R] the forward kernel writes and the two backward kernels read; each is a pure function of its inputs, so
// every result is bit-reproducible run to run, in and out of deterministic mode.
#include "kernels.h"
#include "box_row.h"   // BH_WAVE, bh_wave_sum and the row product, shared with class_boxes.hip

namespace frcnn {

// The class of row r (1-based, 0 = none), uniform over the wave that owns the row.
//   kind 1: int32 classes of the first n rows, every row behind them background;
//   kind 2: an fp32 1-based class per row (the cctarget format), truncated; NaN and anything outside 1 ... C -> none;
//   kind 0: the first maximum of the row's log-probabilities by cnet_decode_kernel's rule (`best` moves only on a strict >, so a
//           NaN at column 0 stays, a NaN elsewhere is never taken, ties keep the lowest column).
__device__ __forceinline__ int bh_row_class(int r, int lane, const void* __restrict__ classes, int kind, int n,
                                            const float* __restrict__ lsm, int ncls, int C) {
  int c = 0;
  if (kind == 1) {
    if (r < n) c = static_cast<const int*>(classes)[r];
  } else if (kind == 2) {
    const float t = static_cast<const float*>(classes)[r];
    if (t >= 1.0f && t <= (float)C) c = (int)t;                       // (a NaN fails both comparisons)
  } else {
    const float* row = lsm + (size_t)r * ncls;
    float bv = 0.f;
    int bi = -1;                                                      // (-1: this lane has seen no column)
    for (int j = lane; j < ncls; j += BH_WAVE) {
      float v = row[j];
      if (v != v) v = -INFINITY;                                      // a NaN behind column 0 never wins
      if (bi < 0 || v > bv) { bv = v; bi = j; }
    }
#pragma unroll
    for (int o = BH_WAVE / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, BH_WAVE);
      const int oi = __shfl_xor(bi, o, BH_WAVE);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    const float first = row[0];
    c = (first != first) ? 1 : bi + 1;
  }
  return (c >= 1 && c <= C) ? c : 0;
}

// ---- 1. forward: out[r][j] = b[4(c-1)+j] + sum_k x[r][k] W[4(c-1)+j][k], c = the row's class; sel[r] = c ------------------------
// One wave a row, four rows a workgroup.  VEC: 16-byte pieces of the row and of the four weight rows (nf % 4 == 0, x and W 16-byte
// aligned), else one float at a time.  Four accumulators a lane, then the butterfly (bh_row_product, box_row.h).
template <bool VEC>
__global__ __launch_bounds__(256) void box_head_forward_kernel(const float* __restrict__ x, int R, int nf, const float* __restrict__ W,
                                                               const float* __restrict__ b, int C, const void* __restrict__ classes,
                                                               int kind, int n, const float* __restrict__ lsm, int ncls,
                                                               float* __restrict__ out, int* __restrict__ sel) {
  const int lane = threadIdx.x & (BH_WAVE - 1);
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                                                  // (wave-uniform)
  const int c = bh_row_class(r, lane, classes, kind, n, lsm, ncls, C);
  float* o = out + 4 * (size_t)r;
  if (c == 0) {                                                        // background or out of range: defined, nothing is read
    if (lane < 4) o[lane] = 0.f;
    if (lane == 0) sel[r] = 0;
    return;
  }
  const float* xr = x + (size_t)r * nf;
  const float* w0 = W + (size_t)(4 * (c - 1)) * nf;
  float a0, a1, a2, a3;
  bh_row_product<VEC>(xr, w0, nf, lane, a0, a1, a2, a3);
  if (lane < 4) {
    const float a = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
    o[lane] = a + b[4 * (c - 1) + lane];
  }
  if (lane == 0) sel[r] = c;
}

// ---- 2. input gradient: gfeat[r][k] = sum_j g[r][j] W[4(sel[r]-1)+j][k], stored; a row without a class stores zeros -------------
template <bool VEC>
__global__ __launch_bounds__(256) void box_head_dgrad_kernel(const float* __restrict__ g, const int* __restrict__ sel, int R, int nf,
                                                             const float* __restrict__ W, int C, float* __restrict__ gfeat) {
  const int lane = threadIdx.x & (BH_WAVE - 1);
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  int c = sel[r];
  if (c < 1 || c > C) c = 0;                                           // (a caller's table: never an index before it is checked)
  float* o = gfeat + (size_t)r * nf;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
  if (c) { const float* gr = g + 4 * (size_t)r; g0 = gr[0]; g1 = gr[1]; g2 = gr[2]; g3 = gr[3]; }
  const float* w0 = W + (size_t)(4 * (c ? c - 1 : 0)) * nf;
  if (VEC) {
    const int nq = nf >> 2;
    float4* oq = reinterpret_cast<float4*>(o);
    if (!c) {
      for (int q = lane; q < nq; q += BH_WAVE) oq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
    const float4* q0 = reinterpret_cast<const float4*>(w0);
    const float4* q1 = reinterpret_cast<const float4*>(w0 + nf);
    const float4* q2 = reinterpret_cast<const float4*>(w0 + 2 * (size_t)nf);
    const float4* q3 = reinterpret_cast<const float4*>(w0 + 3 * (size_t)nf);
    for (int q = lane; q < nq; q += BH_WAVE) {
      const float4 u0 = q0[q], u1 = q1[q], u2 = q2[q], u3 = q3[q];
      float4 v;
      v.x = ((g0 * u0.x + g1 * u1.x) + g2 * u2.x) + g3 * u3.x;
      v.y = ((g0 * u0.y + g1 * u1.y) + g2 * u2.y) + g3 * u3.y;
      v.z = ((g0 * u0.z + g1 * u1.z) + g2 * u2.z) + g3 * u3.z;
      v.w = ((g0 * u0.w + g1 * u1.w) + g2 * u2.w) + g3 * u3.w;
      oq[q] = v;
    }
  } else {
    if (!c) {
      for (int k = lane; k < nf; k += BH_WAVE) o[k] = 0.f;
      return;
    }
    for (int k = lane; k < nf; k += BH_WAVE)
      o[k] = ((g0 * w0[k] + g1 * w0[(size_t)nf + k]) + g2 * w0[2 * (size_t)nf + k]) + g3 * w0[3 * (size_t)nf + k];
  }
}

// ---- 3. weight and bias gradient, segmented by class ----------------------------------------------------------------------------
// gW[4(c-1)+j][k] += sum_{r: sel[r] = c} g[r][j] x[r][k], gb[4(c-1)+j] += sum g[r][j].  One workgroup owns class c = blockIdx.x + 1
// and the 64 features from 64 blockIdx.y: lane = feature, so every element of the gradient has one owner and is read, added to and
// stored by it alone.  The workgroup scans sel 64 BH_WG_WAVES rows at a time; wave w takes rows [64 w, 64 w + 64) of each piece:
// one ballot marks its rows of class c, and it walks the set bits in ascending row order.  The waves' partial sums are then folded
// in wave order 0, 1, ... by wave 0.  A class without a row leaves its gradient rows untouched.
static constexpr int BH_WG_WAVES = 16;
__global__ __launch_bounds__(BH_WG_WAVES * BH_WAVE) void box_head_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                               const int* __restrict__ sel, int R, int nf,
                                                                               float* __restrict__ gW, float* __restrict__ gb) {
  __shared__ float part[BH_WG_WAVES][5][BH_WAVE];                      // [wave][j, 4 = bias sums in lanes 0..3][lane]
  __shared__ int cnt[BH_WG_WAVES];
  const int lane = threadIdx.x & (BH_WAVE - 1);
  const int w = threadIdx.x >> 6;
  const int c = blockIdx.x + 1;
  const int k = blockIdx.y * BH_WAVE + lane;
  const bool live = k < nf;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, ab = 0.f;              // ab: lane j < 4 sums g[.][j]
  int rows = 0;
  for (int base = w * BH_WAVE; base < R; base += BH_WG_WAVES * BH_WAVE) {
    const int r = base + lane;
    unsigned long long m = __ballot(r < R && sel[r] == c);
    rows += __popcll(m);
    while (m) {
      const int rr = base + (__ffsll((long long)m) - 1);
      m &= m - 1;
      const float* gr = g + 4 * (size_t)rr;
      const float g0 = gr[0], g1 = gr[1], g2 = gr[2], g3 = gr[3];
      if (live) {
        const float v = x[(size_t)rr * nf + k];
        a0 += g0 * v; a1 += g1 * v; a2 += g2 * v; a3 += g3 * v;
      }
      ab += lane == 0 ? g0 : lane == 1 ? g1 : lane == 2 ? g2 : g3;
    }
  }
  part[w][0][lane] = a0; part[w][1][lane] = a1; part[w][2][lane] = a2; part[w][3][lane] = a3; part[w][4][lane] = ab;
  if (lane == 0) cnt[w] = rows;
  __syncthreads();
  if (w != 0) return;
  int total = 0;
  for (int i = 0; i < BH_WG_WAVES; ++i) total += cnt[i];
  if (total == 0) return;                                              // no row of this class: nothing is written
  float s[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    float t = part[0][j][lane];
    for (int i = 1; i < BH_WG_WAVES; ++i) t += part[i][j][lane];
    s[j] = t;
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* p = gW + (size_t)(4 * (c - 1) + j) * nf + k;
      *p = *p + s[j];
    }
  }
  if (blockIdx.y == 0 && lane < 4) {
    float* p = gb + 4 * (c - 1) + lane;
    *p = *p + s[4];
  }
}

static bool bh_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) == 0;
}

int box_head_forward(const float* x, int R, int nf, const float* W, const float* b, int C, const void* classes, int kind, int n_fg,
                     const float* lsm, int ncls, float* out, int* sel, hipStream_t s) {
  // everything is checked before the launch: a refused call has written nothing
  FR_CHECK(nf >= 1, "box_head_forward: %d features (at least 1)", nf);
  FR_CHECK(C >= 1, "box_head_forward: %d classes (at least 1)", C);
  FR_CHECK(kind >= 0 && kind <= 2, "box_head_forward: class source %d (0 none, 1 int32, 2 fp32)", kind);
  FR_CHECK((long long)4 * C * nf < (1ll << 31), "box_head_forward: 4 x %d x %d weights do not fit an int", C, nf);
  if (R <= 0) return FRCNN_OK;
  FR_CHECK(x && W && b && out && sel, "box_head_forward: NULL argument");
  FR_CHECK(kind == 0 || classes, "box_head_forward: class source %d without classes", kind);
  FR_CHECK(kind != 1 || (n_fg >= 0 && n_fg <= R), "box_head_forward: %d foreground rows outside 0 ... %d", n_fg, R);
  FR_CHECK(kind != 0 || (lsm && ncls >= 1), "box_head_forward: no class source and no log-probabilities");
  FR_CHECK(((uintptr_t)x | (uintptr_t)W | (uintptr_t)b | (uintptr_t)out | (uintptr_t)sel | (uintptr_t)classes | (uintptr_t)lsm) % 4 == 0,
           "box_head_forward: a pointer is not 4-byte aligned");
  const bool vec = nf % 4 == 0 && bh_aligned16(x, W);
  const double bytes = (double)R * (2.0 * nf + 8) * 4.0;
  if (vec)
    FR_LAUNCH(KC_ELEMWISE, 8.0 * R * nf, bytes, s, box_head_forward_kernel<true>, dim3(cdiv(R, 4)), dim3(256), 0, x, R, nf, W, b, C,
              classes, kind, n_fg, lsm, ncls, out, sel);
  else
    FR_LAUNCH(KC_ELEMWISE, 8.0 * R * nf, bytes, s, box_head_forward_kernel<false>, dim3(cdiv(R, 4)), dim3(256), 0, x, R, nf, W, b, C,
              classes, kind, n_fg, lsm, ncls, out, sel);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

int box_head_backward(const float* g, const float* x, const int* sel, int R, int nf, const float* W, int C, float* gfeat, float* gW,
                      float* gb, hipStream_t s_chain, hipStream_t s_wgrad) {
  FR_CHECK(nf >= 1, "box_head_backward: %d features (at least 1)", nf);
  FR_CHECK(C >= 1, "box_head_backward: %d classes (at least 1)", C);
  FR_CHECK(C <= 65535 && cdiv(nf, BH_WAVE) <= 65535, "box_head_backward: %d classes x %d features exceed the launch grid", C, nf);
  FR_CHECK((long long)4 * C * nf < (1ll << 31), "box_head_backward: 4 x %d x %d weights do not fit an int", C, nf);
  FR_CHECK((gW == nullptr) == (gb == nullptr), "box_head_backward: gW and gb go together (both, or neither)");
  FR_CHECK(gfeat || gW, "box_head_backward: no output");
  if (R <= 0) return FRCNN_OK;
  FR_CHECK(g && sel, "box_head_backward: NULL argument");
  FR_CHECK(!gfeat || W, "box_head_backward: the input gradient needs W");
  FR_CHECK(!gW || x, "box_head_backward: the weight gradient needs x");
  FR_CHECK(((uintptr_t)g | (uintptr_t)x | (uintptr_t)sel | (uintptr_t)W | (uintptr_t)gfeat | (uintptr_t)gW | (uintptr_t)gb) % 4 == 0,
           "box_head_backward: a pointer is not 4-byte aligned");
  if (gfeat) {
    const bool vec = nf % 4 == 0 && bh_aligned16(W, gfeat);
    const double bytes = (double)R * (2.0 * nf + 5) * 4.0;
    if (vec)
      FR_LAUNCH(KC_ELEMWISE, 8.0 * R * nf, bytes, s_chain, box_head_dgrad_kernel<true>, dim3(cdiv(R, 4)), dim3(256), 0, g, sel, R, nf, W,
                C, gfeat);
    else
      FR_LAUNCH(KC_ELEMWISE, 8.0 * R * nf, bytes, s_chain, box_head_dgrad_kernel<false>, dim3(cdiv(R, 4)), dim3(256), 0, g, sel, R, nf, W,
                C, gfeat);
    FR_LAUNCH_CHECK();
  }
  if (gW) {
    FR_LAUNCH(KC_ELEMWISE, 8.0 * R * nf, (double)R * (nf + 5) * 4.0, s_wgrad, box_head_wgrad_kernel, dim3(C, cdiv(nf, BH_WAVE)),
              dim3(BH_WG_WAVES * BH_WAVE), 0, g, x, sel, R, nf, gW, gb);
    FR_LAUNCH_CHECK();
  }
  return FRCNN_OK;
}

}  // namespace frcnn
