// roi_align.hip -- RoIAlign (Mask R-CNN; the torchvision `aligned=True` rule) as the alternative to the max pooling of roi.hip
// (cfg.roi_pooling.method = "align"): every bin of the kh x kw grid over an UN-SNAPPED rect averages g x g bilinear samples of
// the last feature map.  Same batching and the same [R][C*kh*kw] rows as roi.hip; the rects arrive in input space (device
// double[n][4], optionally through the 1-based `pick` rows of the first NMS), so the Detector needs no window kernel.
//
// Geometry (include/frcnn_hip.h has the full statement): cell i of a centred backbone of stride S covers input pixels
// [i S, (i+1) S), its centre sits at (i + 0.5) S, hence x1 = minX / Sx - 0.5.  All of it in double, operation by operation as the
// host reference states it: FMA contraction is off for this translation unit, so the forward pass, the backward pass and a
// host restatement place every sample in the same cell.  Only the four weights of a sample are rounded to fp32.
#pragma clang fp contract(off)
#include <type_traits>

#include "kernels.h"
#include "roi_fix.h"

namespace frcnn {

struct AlignAxis { int lo, hi; double l; bool ok; };

// One coordinate of a sample on an axis of N cells: outside [-1, N] the sample contributes nothing; else clamp to [0, N-1].
__device__ __forceinline__ AlignAxis align_axis(double v, int N) {
  AlignAxis a;
  a.ok = !(v < -1.0 || v > (double)N);
  a.lo = a.hi = 0; a.l = 0.0;
  if (!a.ok) return a;
  v = v > 0.0 ? v : 0.0;
  int lo = (int)v;
  if (lo >= N - 1) { lo = N - 1; a.hi = lo; v = (double)lo; } else a.hi = lo + 1;
  a.lo = lo;
  a.l = v - (double)lo;
  return a;
}

struct AlignRoi { double x1, y1, bin_w, bin_h; };

__device__ __forceinline__ AlignRoi align_roi(const double* __restrict__ rect, const long long* __restrict__ pick, int r,
                                              double inv_sx, double inv_sy, int kh, int kw) {
  const double* q = rect + 4 * (pick ? (size_t)(pick[r] - 1) : (size_t)r);
  const double minX = q[0], minY = q[1], maxX = q[2], maxY = q[3];
  AlignRoi a;
  a.x1 = minX * inv_sx - 0.5;
  a.y1 = minY * inv_sy - 0.5;
  const double w = fmax((maxX - minX) * inv_sx, 0.0), h = fmax((maxY - minY) * inv_sy, 0.0);
  a.bin_w = w / (double)kw;
  a.bin_h = h / (double)kh;
  return a;
}

__device__ __forceinline__ double align_coord(double o, int cell, int s, int g, double bin) {
  return o + ((double)cell + ((double)s + 0.5) / (double)g) * bin;
}

// The four taps of a sample, in the order (y_lo, x_lo), (y_lo, x_hi), (y_hi, x_lo), (y_hi, x_hi).
__device__ __forceinline__ void align_taps(const AlignAxis& ay, const AlignAxis& ax, int W, int* off, float* wt) {
  const double hy = 1.0 - ay.l, hx = 1.0 - ax.l;
  off[0] = ay.lo * W + ax.lo; wt[0] = (float)(hy * hx);
  off[1] = ay.lo * W + ax.hi; wt[1] = (float)(hy * ax.l);
  off[2] = ay.hi * W + ax.lo; wt[2] = (float)(ay.l * hx);
  off[3] = ay.hi * W + ax.hi; wt[3] = (float)(ay.l * ax.l);
}

// ---------------------------------------------------------------- forward
// Like roi_pool_forward_cells_kernel: one block per (ROI, channel slice), a thread owns ONE bin, works out the 4 G^2 tap offsets
// and weights of its bin once (registers: G is a template parameter, the loops unroll) and walks the channels.  The sum is taken
// in a fixed order (samples iy outer, ix inner; taps as above), no atomics: two runs are bit-equal.
template <int G>
__global__ __launch_bounds__(256) void roi_align_forward_bins_kernel(const float* __restrict__ fmap, int C, int H, int W,
                                                                     const double* __restrict__ rect,
                                                                     const long long* __restrict__ pick, double inv_sx,
                                                                     double inv_sy, int kh, int kw, float* __restrict__ out) {
  constexpr int S = G * G;
  const int r = blockIdx.x, cells = kh * kw, groups = blockDim.x / cells;
  const int tid = threadIdx.x;
  if (tid >= groups * cells) return;
  const int cg = tid / cells, cell = tid - cg * cells;
  const int i = cell / kw, j = cell - i * kw;
  const AlignRoi a = align_roi(rect, pick, r, inv_sx, inv_sy, kh, kw);
  int off[4 * S];
  float wt[4 * S];
  unsigned mask = 0;
#pragma unroll
  for (int iy = 0; iy < G; ++iy) {
    const AlignAxis ay = align_axis(align_coord(a.y1, i, iy, G, a.bin_h), H);
#pragma unroll
    for (int ix = 0; ix < G; ++ix) {
      const AlignAxis ax = align_axis(align_coord(a.x1, j, ix, G, a.bin_w), W);
      const int s = iy * G + ix;
      align_taps(ay, ax, W, off + 4 * s, wt + 4 * s);
      if (ay.ok && ax.ok) mask |= 1u << s;
    }
  }
  const int HW = H * W;
  const float inv = 1.0f / (float)S;
  for (int c = blockIdx.y * groups + cg; c < C; c += gridDim.y * groups) {
    const float* ip = fmap + (size_t)c * HW;
    float acc = 0.f;
    if (mask == (1u << S) - 1u) {   // (the common case: every load of the bin is issued before the first use)
      float v[4 * S];
#pragma unroll
      for (int t = 0; t < 4 * S; ++t) v[t] = ip[off[t]];
#pragma unroll
      for (int t = 0; t < 4 * S; ++t) acc = fmaf(wt[t], v[t], acc);
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s)
        if ((mask >> s) & 1u) {
#pragma unroll
          for (int t = 0; t < 4; ++t) acc = fmaf(wt[4 * s + t], ip[off[4 * s + t]], acc);
        }
    }
    out[((size_t)r * C + c) * cells + cell] = acc * inv;
  }
}

// Any grid (kh kw > 256): one output per thread, grid-stride, the geometry recomputed per output.
__global__ void roi_align_forward_kernel(const float* __restrict__ fmap, int C, int H, int W, const double* __restrict__ rect,
                                         const long long* __restrict__ pick, int R, double inv_sx, double inv_sy, int kh, int kw,
                                         int g, float* __restrict__ out) {
  const long total = (long)R * C * kh * kw;
  const float inv = 1.0f / (float)(g * g);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int j = (int)(t % kw);
    long q = t / kw;
    const int i = (int)(q % kh);
    q /= kh;
    const int c = (int)(q % C);
    const int r = (int)(q / C);
    const AlignRoi a = align_roi(rect, pick, r, inv_sx, inv_sy, kh, kw);
    const float* ip = fmap + (size_t)c * H * W;
    float acc = 0.f;
    for (int iy = 0; iy < g; ++iy) {
      const AlignAxis ay = align_axis(align_coord(a.y1, i, iy, g, a.bin_h), H);
      for (int ix = 0; ix < g; ++ix) {
        const AlignAxis ax = align_axis(align_coord(a.x1, j, ix, g, a.bin_w), W);
        if (!(ay.ok && ax.ok)) continue;
        int off[4];
        float wt[4];
        align_taps(ay, ax, W, off, wt);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fmaf(wt[k], ip[off[k]], acc);
      }
    }
    out[t] = acc * inv;
  }
}

int roi_align_forward(const float* fmap, int C, int H, int W, const double* rect, const long long* pick, int R, double inv_sx,
                      double inv_sy, int kh, int kw, int g, float* out, hipStream_t s) {
  if (R <= 0) return FRCNN_OK;
  const long total = (long)R * C * kh * kw;
  const double bytes = total * 4.0 * (1 + 4 * g * g);
  if (kh * kw <= 256) {
    const int groups = 256 / (kh * kw);
    const int slices = std::max(1, std::min(cdiv(C, groups), (int)cdivl(4096, R)));   // enough blocks to fill the chip
    const dim3 grid(R, slices);
#define RA_FWD(G)                                                                                                             \
  FR_LAUNCH(KC_ROI, 0, bytes, s, roi_align_forward_bins_kernel<G>, grid, dim3(256), 0, fmap, C, H, W, rect, pick, inv_sx, inv_sy, \
            kh, kw, out)
    switch (g) {
      case 1: RA_FWD(1); break;
      case 2: RA_FWD(2); break;
      case 3: RA_FWD(3); break;
      default: RA_FWD(4); break;
    }
#undef RA_FWD
    FR_LAUNCH_CHECK();
    return FRCNN_OK;
  }
  const int grid = (int)std::min<long>(cdivl(total, 256), 4096);
  FR_LAUNCH(KC_ROI, 0, bytes, s, roi_align_forward_kernel, dim3(grid), dim3(256), 0, fmap, C, H, W, rect, pick, R, inv_sx, inv_sy,
            kh, kw, g, out);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- backward
// gmap += scatter: every bin spreads gout / g^2 over its 4 g^2 taps and ROIs overlap.  The design of roi_pool_backward_lds_kernel
// (channel planes in LDS, LDS atomics, one add of each plane to HBM) with CB planes per workgroup: a thread works out the
// double-precision geometry of a bin ONCE and applies it to the CB channels of its workgroup.  CB is 2 where that leaves enough
// workgroups, else 1: the kernel's time follows the LDS atomics a compute unit has to retire (16 per bin and channel at g = 2), so
// more planes per workgroup only pay while every compute unit still has work (DESIGN.md has the figures, and those of the tap
// table that lost).  A term is (float)(weight * (double)gout / g^2): one rounding on top of the weight's.  DET: 64-bit
// fixed-point planes (roi_fix.h), the result does not depend on the order of the atomics.
template <typename T> __device__ __forceinline__ void align_add(T* p, float v);
template <> __device__ __forceinline__ void align_add<float>(float* p, float v) { atomicAdd(p, v); }
template <> __device__ __forceinline__ void align_add<unsigned long long>(unsigned long long* p, float v) {
  atomicAdd(p, (unsigned long long)roi_to_fix(v));
}

template <int CB, bool DET>
__global__ __launch_bounds__(1024) void roi_align_backward_lds_kernel(float* __restrict__ gmap, int C, int H, int W,
                                                                      const float* __restrict__ gout, const double* __restrict__ rect,
                                                                      const long long* __restrict__ pick, int R, double inv_sx,
                                                                      double inv_sy, int kh, int kw, int g) {
  typedef typename std::conditional<DET, unsigned long long, float>::type T;
  extern __shared__ unsigned char align_smem[];
  T* plane = reinterpret_cast<T*>(align_smem);
  const int HW = H * W, c0 = blockIdx.x * CB, nc = min(CB, C - c0);
  for (int e = threadIdx.x; e < nc * HW; e += blockDim.x) plane[e] = (T)0;
  __syncthreads();
  const int cells = kh * kw, total = R * cells;
  const double inv_g2 = 1.0 / (double)(g * g);
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int r = e / cells, cell = e - r * cells;
    const int i = cell / kw, j = cell - i * kw;
    double gs[CB];
    bool any = false;
    const float* gp = gout + ((size_t)r * C + c0) * cells + cell;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const float v = c < nc ? gp[(size_t)c * cells] : 0.f;
      any |= v != 0.f;
      gs[c] = (double)v * inv_g2;
    }
    if (!any) continue;
    const AlignRoi a = align_roi(rect, pick, r, inv_sx, inv_sy, kh, kw);
    for (int iy = 0; iy < g; ++iy) {
      const AlignAxis ay = align_axis(align_coord(a.y1, i, iy, g, a.bin_h), H);
      if (!ay.ok) continue;
      for (int ix = 0; ix < g; ++ix) {
        const AlignAxis ax = align_axis(align_coord(a.x1, j, ix, g, a.bin_w), W);
        if (!ax.ok) continue;
        int off[4];
        float wt[4];
        align_taps(ay, ax, W, off, wt);
#pragma unroll
        for (int c = 0; c < CB; ++c) {
          if (c >= nc) break;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float t = (float)((double)wt[k] * gs[c]);
            if (t != 0.f) align_add<T>(plane + c * HW + off[k], t);
          }
        }
      }
    }
  }
  __syncthreads();
  float* gm = gmap + (size_t)c0 * HW;
  for (int e = threadIdx.x; e < nc * HW; e += blockDim.x) {
    if (DET) {
      const long long v = (long long)plane[e];
      if (v != 0) gm[e] += (float)((double)v / ROI_FIX_SCALE);
    } else {
      const float v = (float)plane[e];
      if (v != 0.f) gm[e] += v;
    }
  }
}

// A plane that does not fit in LDS: one thread per (ROI, channel, bin), atomics in device memory -- fp32 on gmap itself, or (DET)
// 64-bit fixed point on a zeroed scratch map that roi_fix_apply then adds to gmap.
template <bool DET>
__global__ void roi_align_backward_kernel(void* __restrict__ dst, int C, int H, int W, const float* __restrict__ gout,
                                          const double* __restrict__ rect, const long long* __restrict__ pick, int R,
                                          double inv_sx, double inv_sy, int kh, int kw, int g) {
  typedef typename std::conditional<DET, unsigned long long, float>::type T;
  const long total = (long)R * C * kh * kw;
  const double inv_g2 = 1.0 / (double)(g * g);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const float v = gout[t];
    if (v == 0.f) continue;
    const int j = (int)(t % kw);
    long q = t / kw;
    const int i = (int)(q % kh);
    q /= kh;
    const int c = (int)(q % C);
    const int r = (int)(q / C);
    const double gs = (double)v * inv_g2;
    const AlignRoi a = align_roi(rect, pick, r, inv_sx, inv_sy, kh, kw);
    T* plane = reinterpret_cast<T*>(dst) + (size_t)c * H * W;
    for (int iy = 0; iy < g; ++iy) {
      const AlignAxis ay = align_axis(align_coord(a.y1, i, iy, g, a.bin_h), H);
      if (!ay.ok) continue;
      for (int ix = 0; ix < g; ++ix) {
        const AlignAxis ax = align_axis(align_coord(a.x1, j, ix, g, a.bin_w), W);
        if (!ax.ok) continue;
        int off[4];
        float wt[4];
        align_taps(ay, ax, W, off, wt);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float term = (float)((double)wt[k] * gs);
          if (term == 0.f) continue;
          if (DET) atomicAdd(reinterpret_cast<unsigned long long*>(plane) + off[k], (unsigned long long)roi_to_fix(term));
          else unsafeAtomicAdd(reinterpret_cast<float*>(plane) + off[k], term);
        }
      }
    }
  }
}

#define ALIGN_MIN_BLOCKS 128
int roi_align_backward(float* gmap, int C, int H, int W, const float* gout, const double* rect, const long long* pick, int R,
                       double inv_sx, double inv_sy, int kh, int kw, int g, hipStream_t s) {
  if (R <= 0) return FRCNN_OK;
  const long total = (long)R * C * kh * kw;
  const double bytes = total * 4.0 * (1 + 4 * g * g);
  const bool det = deterministic();
  const size_t plane_bytes = (size_t)H * W * (det ? 8 : 4);
  FR_CHECK((long)R * kh * kw < (1L << 31), "roi_align_backward: %d ROIs of %d x %d bins: more than 2^31 bins", R, kh, kw);
  if (plane_bytes <= 64 * 1024) {
    // two planes per workgroup while at least ALIGN_MIN_BLOCKS workgroups remain (and both planes fit the 64 KB)
    const bool two = 2 * plane_bytes <= 64 * 1024 && cdiv(C, 2) >= ALIGN_MIN_BLOCKS;
    const dim3 grid(two ? cdiv(C, 2) : C);
    const size_t lds = (two ? 2 : 1) * plane_bytes;
#define RA_BWD(CB)                                                                                                               \
  do {                                                                                                                           \
    if (det)                                                                                                                     \
      FR_LAUNCH(KC_ROI, 0, bytes, s, (roi_align_backward_lds_kernel<CB, true>), grid, dim3(512), lds, gmap, C, H, W, gout, rect, \
                pick, R, inv_sx, inv_sy, kh, kw, g);                                                                             \
    else                                                                                                                         \
      FR_LAUNCH(KC_ROI, 0, bytes, s, (roi_align_backward_lds_kernel<CB, false>), grid, dim3(1024), lds, gmap, C, H, W, gout,     \
                rect, pick, R, inv_sx, inv_sy, kh, kw, g);                                                                       \
  } while (0)
    if (two) RA_BWD(2); else RA_BWD(1);
#undef RA_BWD
    FR_LAUNCH_CHECK();
    return FRCNN_OK;
  }
  const int grid = (int)std::min<long>(cdivl(total, 256), 4096);
  if (det) {
    float* ws = nullptr;
    const long n = (long)C * H * W;
    FR_TRY(det_workspace(s, (size_t)n * 2, &ws));
    FR_HIP(hipMemsetAsync(ws, 0, (size_t)n * 8, s));
    FR_LAUNCH(KC_ROI, 0, bytes, s, roi_align_backward_kernel<true>, dim3(grid), dim3(256), 0, (void*)ws, C, H, W, gout, rect, pick,
              R, inv_sx, inv_sy, kh, kw, g);
    FR_LAUNCH_CHECK();
    return roi_fix_apply((const unsigned long long*)ws, n, gmap, s);
  }
  FR_LAUNCH(KC_ROI, 0, bytes, s, roi_align_backward_kernel<false>, dim3(grid), dim3(256), 0, (void*)gmap, C, H, W, gout, rect, pick,
            R, inv_sx, inv_sy, kh, kw, g);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
