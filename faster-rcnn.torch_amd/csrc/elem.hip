// elem.hip -- bandwidth-bound pieces of the proposal network and the optimiser:
//   nn.PReLU / nn.SpatialDropout / nn.SpatialMaxPooling(2,2,2,2):ceil() forward+backward
//   (models/model_utilities.lua:9-12,23), bias/slope gradient reductions, flat-buffer ops
//   (objective.lua:49,200) and optim.rmsprop / optim.sgd / optim.nag (main.lua:122-124,133-135).
// No MFMA here: these are gather / argmax / streaming kernels; the design rule is coalesced
// 16-byte accesses where the layout allows and one wave-level reduction + one atomic per block.
#include <algorithm>

#include <mutex>
#include <unordered_map>

#include "kernels.h"
#include "amax.h"

namespace frcnn {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// block-wide sum (blockDim.x multiple of 64, <= 1024); result valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x < 64) {
    r = threadIdx.x < (blockDim.x >> 6) ? sh[threadIdx.x] : 0.f;
    r = wave_sum(r);
  }
  __syncthreads();
  return r;
}

// the same in fp64 (the PReLU slope gradient is ONE number summed over a whole layer with cancellation: its partial sums are
// carried in double so that the result is good to fp32 rounding whatever the layer size)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < 64) {
    r = threadIdx.x < (blockDim.x >> 6) ? sh[threadIdx.x] : 0.0;
    r = wave_sum_d(r);
  }
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------- flat buffer ops
int fill_zero(void* p, size_t bytes, hipStream_t s) {
  if (prof_enabled(KC_ELEMWISE)) prof_before(KC_ELEMWISE, s);
  FR_HIP(hipMemsetAsync(p, 0, bytes, s));
  if (prof_enabled(KC_ELEMWISE)) prof_after(KC_ELEMWISE, 0, (double)bytes, s);
  return FRCNN_OK;
}

__global__ void scale_kernel(float* __restrict__ x, long n, float sc) {
  long n4 = n >> 2;
  float4* x4 = reinterpret_cast<float4*>(x);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 v = x4[i];
    v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
    x4[i] = v;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    x[i] *= sc;
}
int scale_inplace(float* x, long n, float sc, hipStream_t s) {
  FR_CHECK(((uintptr_t)x & 15) == 0, "scale_inplace: buffer must be 16-byte aligned");
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(n / 4, 256)), 2048);
  FR_LAUNCH(KC_ELEMWISE, 0, n * 8.0, s, scale_kernel, dim3(grid), dim3(256), 0, x, n, sc);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

__global__ void add_kernel(float* __restrict__ y, const float* __restrict__ x, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] += x[i];
}
int add_inplace(float* y, const float* x, long n, hipStream_t s) {
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(n, 256)), 2048);
  FR_LAUNCH(KC_ELEMWISE, 0, n * 12.0, s, add_kernel, dim3(grid), dim3(256), 0, y, x, n);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

__global__ void fill_kernel(float* x, long n, float v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    x[i] = v;
}
int fill_value(float* x, long n, float v, hipStream_t s) {
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(n, 256)), 2048);
  FR_LAUNCH(KC_ELEMWISE, 0, n * 4.0, s, fill_kernel, dim3(grid), dim3(256), 0, x, n, v);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- activation (tests)
__global__ void act_forward_kernel(const float* __restrict__ x, int C, long hw, const float* slope,
                                   const float* scale, float* __restrict__ y) {
  const float a = slope ? *slope : 1.f;
  long total = (long)C * hw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    float v = x[i];
    if (slope) v = v > 0.f ? v : a * v;
    if (scale) v *= scale[i / hw];
    y[i] = v;
  }
}
int act_forward(const float* x, int C, long hw, const float* slope, const float* scale, float* y,
                hipStream_t s) {
  long total = (long)C * hw;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(total, 256)), 2048);
  FR_LAUNCH(KC_ELEMWISE, 0, total * 8.0, s, act_forward_kernel, dim3(grid), dim3(256), 0, x, C, hw, slope,
            scale, y);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- max pool (fused activation)
// One thread per output element; output rows are contiguous so loads of the two input rows are
// 8-byte-per-lane strided reads (coalesced across the wave).
__global__ void maxpool_act_forward_kernel(const float* __restrict__ x, int C, int H, int W, int Ho,
                                           int Wo, const float* slope, const float* scale,
                                           float* __restrict__ out, unsigned char* __restrict__ idx, float* amax) {
  const float a = slope ? *slope : 1.f;
  long total = (long)C * Ho * Wo;
  float am = 0.f;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    int ox = (int)(t % Wo);
    long r = t / Wo;
    int oy = (int)(r % Ho);
    int c = (int)(r / Ho);
    const float sc = scale ? scale[c] : 1.f;
    const float* xp = x + (size_t)c * H * W;
    float best = -3.402823466e+38f;
    int bi = 0;
    bool any = false;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      int y = oy * 2 + dy;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int xx = ox * 2 + dx;
        if (y < H && xx < W) {
          float v = xp[(size_t)y * W + xx];
          if (slope) v = v > 0.f ? v : a * v;
          if (scale) v *= sc;
          if (!any || v > best) { best = v; bi = dy * 2 + dx; any = true; }
        }
      }
    }
    out[t] = best;
    idx[t] = (unsigned char)bi;
    am = fmaxf(am, fabsf(best));
  }
  if (amax) amax_store_block(am, amax);
}
int maxpool_act_forward(const float* x, int C, int H, int W, const float* slope, const float* scale,
                        float* out, unsigned char* idx, hipStream_t s, float* amax) {
  int Ho = (H - 2 + 1) / 2 + 1, Wo = (W - 2 + 1) / 2 + 1;  // ceil((n-2)/2)+1
  long total = (long)C * Ho * Wo;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(total, 256)), 4096);
  FR_LAUNCH(KC_ELEMWISE, 0, (double)C * H * W * 4.0 + total * 5.0, s, maxpool_act_forward_kernel, dim3(grid),
            dim3(256), 0, x, C, H, W, Ho, Wo, slope, scale, out, idx, amax);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// gx[c][y][x] = (argmax of window == this position ? gpool : 0) * scale[c] * prelu'(x)
// One block per (channel, slab of rows): the bias-gradient and slope-gradient partial sums are
// reduced in the block and leave through one atomic each.
// 512 threads: two waves per SIMD at 40 registers.  In the backward phase this pass runs beside conv_wgradx, whose one block per CU
// holds 392 of a SIMD's 512 registers: a 1024-thread block (4 x 40 registers per SIMD) does not fit beside it and waited for
// weight-gradient blocks to retire -- 60-70 us live for a 15-us pass on the dependent chain (profiles/r05_step_timeline.txt).
// Same-box A/B of the step: 2.824 (1024) / 2.799 (768) / 2.796 ms (512).
#ifndef ACT_BWD_THREADS
#define ACT_BWD_THREADS 512
#endif
template <bool POOLED, bool VEC>
__global__ __launch_bounds__(ACT_BWD_THREADS) void act_backward_kernel(const float* __restrict__ gin, const unsigned char* __restrict__ idx,
                                    const float* __restrict__ x, int C, int H, int W, int Ho, int Wo,
                                    const float* slope, const float* scale, float* __restrict__ gx,
                                    float* gbias, float* gslope, int chunks, float* part_b, float* part_a, float* amax) {
  __shared__ float sh[16];
  __shared__ double shd[16];
  float am = 0.f;   // largest magnitude written (amax.h)
  const int c = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long hw = (long)H * W;
  long per = cdivl(hw, chunks);
  if (VEC) per = (per + 3) & ~3L;
  const long beg = chunk * per, end = beg + per < hw ? beg + per : hw;
  const float a = slope ? *slope : 1.f;
  const float sc = scale ? scale[c] : 1.f;
  const bool has_slope = slope != nullptr;
  float sb = 0.f;
  double sa = 0.0;
  if (VEC) {
    // 4 consecutive elements of one row per thread and load: 16-byte loads/stores (W % 4 == 0, Wo even).
    // Two such groups are in flight per thread (all loads issued before the first use) and the indices are
    // 32-bit (a channel plane has < 2^31 elements): the kernel is a pure HBM stream and was latency-bound.
    const float* xc = x + (size_t)c * hw;
    const float* gc = POOLED ? gin + (size_t)c * Ho * Wo : gin + (size_t)c * hw;
    const unsigned char* ic = POOLED ? idx + (size_t)c * Ho * Wo : nullptr;
    float* oc = gx + (size_t)c * hw;
    const unsigned ibeg = (unsigned)beg, iend = (unsigned)end, uW = (unsigned)W, stride = 4u * blockDim.x;
    auto fetch = [&](unsigned i, bool ok, float* g, float4& xv4) {
      if (!ok) { g[0] = g[1] = g[2] = g[3] = 0.f; xv4 = make_float4(1.f, 1.f, 1.f, 1.f); return; }
      if (POOLED) {
        const unsigned y = i / uW, xx = i - y * uW;
        const unsigned po = (y >> 1) * (unsigned)Wo + (xx >> 1);
        const float2 gp = *reinterpret_cast<const float2*>(gc + po);
        const unsigned short ib = *reinterpret_cast<const unsigned short*>(ic + po);
        const unsigned char code = (unsigned char)((y & 1) * 2);
        g[0] = ((ib & 0xff) == code) ? gp.x : 0.f;
        g[1] = ((ib & 0xff) == code + 1) ? gp.x : 0.f;
        g[2] = ((ib >> 8) == code) ? gp.y : 0.f;
        g[3] = ((ib >> 8) == code + 1) ? gp.y : 0.f;
      } else {
        const float4 gv = *reinterpret_cast<const float4*>(gc + i);
        g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
      }
      xv4 = *reinterpret_cast<const float4*>(xc + i);
    };
    auto finish = [&](unsigned i, const float* g, const float4& xv4) {
      const float xv[4] = {xv4.x, xv4.y, xv4.z, xv4.w};
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gj = g[j];
        if (scale) gj *= sc;
        r[j] = gj;
        if (has_slope && !(xv[j] > 0.f)) { r[j] = a * gj; sa += (double)xv[j] * (double)gj; }
        sb += r[j];
        am = fmaxf(am, fabsf(r[j]));
      }
      *reinterpret_cast<float4*>(oc + i) = make_float4(r[0], r[1], r[2], r[3]);
    };
    for (unsigned i = ibeg + 4u * threadIdx.x; i < iend; i += 2u * stride) {
      const unsigned i2 = i + stride;
      const bool ok2 = i2 < iend;
      float g0[4], g1[4];
      float4 x0, x1;
      fetch(i, true, g0, x0);
      fetch(i2, ok2, g1, x1);
      finish(i, g0, x0);
      if (ok2) finish(i2, g1, x1);
    }
  } else {
    for (long i = beg + threadIdx.x; i < end; i += blockDim.x) {
      float g;
      if (POOLED) {
        int y = (int)(i / W), xx = (int)(i - (long)y * W);
        int oy = y >> 1, ox = xx >> 1;
        long po = ((long)c * Ho + oy) * Wo + ox;
        g = (idx[po] == (unsigned char)((y & 1) * 2 + (xx & 1))) ? gin[po] : 0.f;
      } else {
        g = gin[(size_t)c * hw + i];
      }
      if (scale) g *= sc;
      float xv = x[(size_t)c * hw + i];
      float r = g;
      if (has_slope) {
        if (!(xv > 0.f)) { r = a * g; sa += (double)xv * (double)g; }
      }
      gx[(size_t)c * hw + i] = r;
      sb += r;
      am = fmaxf(am, fabsf(r));
    }
  }
  if (amax) amax_store_block(am, amax);
  float tb = block_sum(sb, sh);
  if (part_b) {   // deterministic mode: partials to scratch, folded in index order by fold_partials_kernel
    if (threadIdx.x == 0) part_b[blockIdx.x] = tb;
    float ta = (slope && gslope) ? (float)block_sum_d(sa, shd) : 0.f;
    if (threadIdx.x == 0) part_a[blockIdx.x] = ta;
    return;
  }
  if (threadIdx.x == 0 && gbias) unsafeAtomicAdd(gbias + c, tb);
  if (slope && gslope) {
    float ta = (float)block_sum_d(sa, shd);
    if (threadIdx.x == 0) unsafeAtomicAdd(gslope, ta);
  }
}

// gbias[c] += sum_chunk part_b[c*chunks + chunk] (index order); *gslope += sum_b part_a[b] (fixed strided order + fixed tree)
__global__ void fold_partials_kernel(const float* __restrict__ part_b, const float* __restrict__ part_a, int C, int chunks,
                                     float* gbias, float* gslope) {
  __shared__ float sh[16];
  if (gbias && part_b)
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float v = 0.f;
      for (int k = 0; k < chunks; ++k) v += part_b[(size_t)c * chunks + k];
      gbias[c] += v;
    }
  if (gslope && part_a) {
    float v = 0.f;
    for (int b = threadIdx.x; b < C * chunks; b += blockDim.x) v += part_a[b];
    const float t = block_sum(v, sh);
    if (threadIdx.x == 0) *gslope += t;
  }
}
static int fold_partials(const float* part_b, const float* part_a, int C, int chunks, float* gbias, float* gslope, hipStream_t s) {
  FR_LAUNCH(KC_ELEMWISE, 0, (double)C * chunks * 8.0, s, fold_partials_kernel, dim3(1), dim3(256), 0, part_b, part_a, C, chunks,
            gbias, gslope);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

static bool g_deterministic = getenv("FRCNN_DETERMINISTIC") && atoi(getenv("FRCNN_DETERMINISTIC")) != 0;   // default of the option
bool deterministic() { return g_deterministic; }
void set_deterministic(bool on) { g_deterministic = on; }
static std::mutex g_det_mu;
static std::unordered_map<hipStream_t, std::pair<float*, size_t>> g_det_ws;
int det_workspace(hipStream_t s, size_t floats, float** out) {
  std::lock_guard<std::mutex> lk(g_det_mu);
  auto& e = g_det_ws[s];
  if (e.second < floats) {
    if (e.first) FR_HIP(hipFree(e.first));
    e.first = nullptr; e.second = 0;
    size_t n = std::max<size_t>(floats, 1 << 16);
    FR_HIP(hipMalloc((void**)&e.first, n * 4));
    e.second = n;
  }
  *out = e.first;
  return FRCNN_OK;
}

// Blocks of 1024 threads, ~512-768 of them: every block ends with ONE atomic on the single slope-gradient
// address, and 2048 of those serialise for ~15 us in the memory-side atomic unit (measured: a 26 MB and a
// 138 MB launch both took 35 us; without the atomic 12-21 us).
static int act_bwd_chunks(int C, long hw) {
  long want = cdivl(512, C);
  long maxc = cdivl(hw, 4096);
  return (int)std::max<long>(1, std::min<long>(want, maxc));
}

int maxpool_act_backward(const float* gpool, const unsigned char* idx, const float* x, int C, int H,
                         int W, const float* slope, const float* scale, float* gx, float* gbias,
                         float* gslope, hipStream_t s, float* amax) {
  int Ho = (H - 2 + 1) / 2 + 1, Wo = (W - 2 + 1) / 2 + 1;
  int chunks = act_bwd_chunks(C, (long)H * W);
  // (more blocks than a record has entries: the magnitude of gx is taken by a pass of its own below, as every other record producer does)
  float* const amax_after = (amax && (long)C * chunks > AMAX_MAX_BLOCKS) ? amax : nullptr;
  if (amax_after) amax = nullptr;
  float *pb = nullptr, *pa = nullptr;
  if (deterministic()) { FR_TRY(det_workspace(s, (size_t)2 * C * chunks, &pb)); pa = pb + (size_t)C * chunks; }
  const bool vec = (W % 4 == 0) && (Wo % 2 == 0) && (((uintptr_t)gpool | (uintptr_t)x | (uintptr_t)gx) % 16 == 0) &&
                   ((uintptr_t)idx % 2 == 0);
  if (vec)
    FR_LAUNCH(KC_ELEMWISE, 0, (double)C * H * W * 9.25, s, (act_backward_kernel<true, true>), dim3(C * chunks),
              dim3(ACT_BWD_THREADS), 0, gpool, idx, x, C, H, W, Ho, Wo, slope, scale, gx, gbias, gslope, chunks, pb, pa, amax);
  else
    FR_LAUNCH(KC_ELEMWISE, 0, (double)C * H * W * 9.25, s, (act_backward_kernel<true, false>), dim3(C * chunks),
              dim3(ACT_BWD_THREADS), 0, gpool, idx, x, C, H, W, Ho, Wo, slope, scale, gx, gbias, gslope, chunks, pb, pa, amax);
  FR_LAUNCH_CHECK();
  if (pb) FR_TRY(fold_partials(gbias ? pb : nullptr, (slope && gslope) ? pa : nullptr, C, chunks, gbias, gslope, s));
  if (amax_after) FR_TRY(tensor_absmax(gx, (long)C * H * W, amax_after, s));
  return FRCNN_OK;
}

int act_backward(const float* gy, const float* x, int C, long hw, const float* slope,
                 const float* scale, float* gx, float* gbias, float* gslope, hipStream_t s, float* amax) {
  int chunks = act_bwd_chunks(C, hw);
  // (more blocks than a record has entries: the magnitude of gx is taken by a pass of its own below, as every other record producer does)
  float* const amax_after = (amax && (long)C * chunks > AMAX_MAX_BLOCKS) ? amax : nullptr;
  if (amax_after) amax = nullptr;
  float *pb = nullptr, *pa = nullptr;
  if (deterministic()) { FR_TRY(det_workspace(s, (size_t)2 * C * chunks, &pb)); pa = pb + (size_t)C * chunks; }
  const bool vec = (hw % 4 == 0) && (((uintptr_t)gy | (uintptr_t)x | (uintptr_t)gx) % 16 == 0);
  if (vec)
    FR_LAUNCH(KC_ELEMWISE, 0, (double)C * hw * 12.0, s, (act_backward_kernel<false, true>), dim3(C * chunks),
              dim3(ACT_BWD_THREADS), 0, gy, (const unsigned char*)nullptr, x, C, 1, (int)hw, 1, 1, slope, scale, gx,
              gbias, gslope, chunks, pb, pa, amax);
  else
    FR_LAUNCH(KC_ELEMWISE, 0, (double)C * hw * 12.0, s, (act_backward_kernel<false, false>), dim3(C * chunks),
              dim3(ACT_BWD_THREADS), 0, gy, (const unsigned char*)nullptr, x, C, 1, (int)hw, 1, 1, slope, scale, gx,
              gbias, gslope, chunks, pb, pa, amax);
  FR_LAUNCH_CHECK();
  if (pb) FR_TRY(fold_partials(gbias ? pb : nullptr, (slope && gslope) ? pa : nullptr, C, chunks, gbias, gslope, s));
  if (amax_after) FR_TRY(tensor_absmax(gx, (long)C * hw, amax_after, s));
  return FRCNN_OK;
}

// (16-byte loads where the chunk allows: the first layer's bias gradient of vgg_large sums 64 x 600 x 1000 values -- 120 us one value
// per load and thread, round 6)
__global__ void channel_sum_kernel(const float* __restrict__ g, long hw, float* gbias, int chunks, float* part_b) {
  __shared__ float sh[16];
  const int c = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  long per = cdivl(hw, chunks);
  per = (per + 3) & ~3L;
  const long beg = chunk * per, end = beg + per < hw ? beg + per : hw;
  const float* gc = g + (size_t)c * hw;
  float sb = 0.f;
  if (beg < end) {
    if ((reinterpret_cast<uintptr_t>(gc + beg) & 15) == 0) {
      const long n4 = (end - beg) >> 2;
      const float4* g4 = reinterpret_cast<const float4*>(gc + beg);
      float s0 = 0.f, s1 = 0.f;
      long i = threadIdx.x;
      for (; i + blockDim.x < n4; i += 2 * blockDim.x) {
        const float4 a = g4[i], b = g4[i + blockDim.x];
        s0 += (a.x + a.y) + (a.z + a.w); s1 += (b.x + b.y) + (b.z + b.w);
      }
      if (i < n4) { const float4 a = g4[i]; s0 += (a.x + a.y) + (a.z + a.w); }
      sb = s0 + s1;
      for (long j = beg + (n4 << 2) + threadIdx.x; j < end; j += blockDim.x) sb += gc[j];
    } else {
      for (long i = beg + threadIdx.x; i < end; i += blockDim.x) sb += gc[i];
    }
  }
  float tb = block_sum(sb, sh);
  if (part_b) { if (threadIdx.x == 0) part_b[blockIdx.x] = tb; return; }
  if (threadIdx.x == 0) unsafeAtomicAdd(gbias + c, tb);
}
int channel_sum(const float* g, int C, long hw, float* gbias, hipStream_t s) {
  int chunks = act_bwd_chunks(C, hw);
  float* pb = nullptr;
  if (deterministic()) FR_TRY(det_workspace(s, (size_t)C * chunks, &pb));
  FR_LAUNCH(KC_ELEMWISE, 0, (double)C * hw * 4.0, s, channel_sum_kernel, dim3(C * chunks), dim3(256), 0, g,
            hw, gbias, chunks, pb);
  FR_LAUNCH_CHECK();
  if (pb) FR_TRY(fold_partials(pb, nullptr, C, chunks, gbias, nullptr, s));
  return FRCNN_OK;
}

// gb[o] += sum_r g[r][o]  (row-major R x O; nn.Linear bias gradient): 64 columns x 16 row groups per block.  fp64 partial sums,
// like the batch normalisation's column sums (cnet.hip): in front of a BatchNormalization the true sum is zero and what is left is
// rounding -- fp32 partial sums left six times the rounding of the summed values themselves at a thousand rows
// (tests/test_gpu_cnet_shapes.py)
__global__ __launch_bounds__(1024) void channel_sum_cols_kernel(const float* __restrict__ g, int R, int O, float* gb) {
  __shared__ double sh[16 * 64];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int o = blockIdx.x * 64 + tx;
  double sacc = 0.0;
  if (o < O) for (int r = ty; r < R; r += 16) sacc += g[(size_t)r * O + o];
  sh[ty * 64 + tx] = sacc;
  __syncthreads();
  if (ty == 0 && o < O) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k * 64 + tx];
    gb[o] = (float)((double)gb[o] + t);
  }
}
int channel_sum_cols(const float* g, int R, int O, float* gb, hipStream_t s) {
  FR_LAUNCH(KC_ELEMWISE, 0, (double)R * O * 4.0, s, channel_sum_cols_kernel, dim3(cdiv(O, 64)), dim3(64, 16), 0, g, R,
            O, gb);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- sparse anchor-head backward helpers
// delta_outputs[1..4] are non-zero only at the sampled anchors (objective.lua:91-134), so the
// backward of an anchor head can run on P gathered positions instead of the whole map.
// dst[c][p] = src[c][pos[p]]  (and dst_act = prelu(dst) when slope != null)
__global__ void gather_positions_kernel(const float* __restrict__ src, int C, long hw, const int* __restrict__ pos, int P,
                                        float* __restrict__ dst, const float* slope, float* __restrict__ dst_act) {
  const long total = (long)C * P;
  const float a = slope ? *slope : 1.f;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int c = (int)(t / P), pi = (int)(t - (long)c * P);
    const float v = src[(size_t)c * hw + pos[pi]];
    dst[t] = v;
    if (dst_act) dst_act[t] = v > 0.f ? v : a * v;
  }
}
int gather_positions(const float* src, int C, long hw, const int* pos, int P, float* dst, const float* slope,
                     float* dst_act, hipStream_t s) {
  long total = (long)C * P;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(total, 256)), 2048);
  FR_LAUNCH(KC_ELEMWISE, 0, total * 8.0, s, gather_positions_kernel, dim3(grid), dim3(256), 0, src, C, hw, pos, P, dst,
            slope, dst_act);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// col[p][(c,ky,kx)] = X[c][y_p + ky][x_p + kx]   (valid convolution: always in bounds); pos = y*Wo + x
__global__ void im2col_positions_kernel(const float* __restrict__ X, int C, int H, int W, int k, int Wo,
                                        const int* __restrict__ pos, int P, float* __restrict__ col) {
  const int ckk = C * k * k;
  const long total = (long)P * ckk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int pi = (int)(t / ckk), q = (int)(t - (long)pi * ckk);
    const int kx = q % k, ky = (q / k) % k, c = q / (k * k);
    const int y = pos[pi] / Wo, x = pos[pi] - y * Wo;
    col[t] = X[((size_t)c * H + y + ky) * W + x + kx];
  }
}
int im2col_positions(const float* X, int C, int H, int W, int k, int Wo, const int* pos, int P, float* col, hipStream_t s) {
  long total = (long)P * C * k * k;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(total, 256)), 4096);
  FR_LAUNCH(KC_ELEMWISE, 0, total * 8.0, s, im2col_positions_kernel, dim3(grid), dim3(256), 0, X, C, H, W, k, Wo, pos, P, col);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// gX[c][y_p + ky][x_p + kx] += col[p][(c,ky,kx)]  (neighbourhoods of different anchors overlap: atomics)
__global__ void col2im_positions_add_kernel(const float* __restrict__ col, int C, int H, int W, int k, int Wo,
                                            const int* __restrict__ pos, int P, float* __restrict__ gX) {
  const int ckk = C * k * k;
  const long total = (long)P * ckk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int pi = (int)(t / ckk), q = (int)(t - (long)pi * ckk);
    const int kx = q % k, ky = (q / k) % k, c = q / (k * k);
    const int y = pos[pi] / Wo, x = pos[pi] - y * Wo;
    unsafeAtomicAdd(gX + ((size_t)c * H + y + ky) * W + x + kx, col[t]);
  }
}
// deterministic variant: one thread per element of gX gathers, in position order, every patch entry that lands on it
__global__ void col2im_positions_gather_kernel(const float* __restrict__ col, int C, int H, int W, int k, int Wo,
                                               const int* __restrict__ pos, int P, float* __restrict__ gX) {
  const int ckk = C * k * k;
  const long total = (long)C * H * W;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(t % W), yy = (int)((t / W) % H), c = (int)(t / ((long)W * H));
    float v = 0.f;
    bool any = false;
    for (int pi = 0; pi < P; ++pi) {
      const int y = pos[pi] / Wo, x = pos[pi] - y * Wo;
      const int ky = yy - y, kx = xx - x;
      if (ky >= 0 && ky < k && kx >= 0 && kx < k) { v += col[(size_t)pi * ckk + (c * k + ky) * k + kx]; any = true; }
    }
    if (any) gX[t] += v;
  }
}
int col2im_positions_add(const float* col, int C, int H, int W, int k, int Wo, const int* pos, int P, float* gX,
                         hipStream_t s) {
  if (deterministic()) {
    long n = (long)C * H * W;
    int g = (int)std::min<long>(std::max<long>(1, cdivl(n, 256)), 8192);
    FR_LAUNCH(KC_ELEMWISE, 0, n * 8.0, s, col2im_positions_gather_kernel, dim3(g), dim3(256), 0, col, C, H, W, k, Wo, pos, P, gX);
    FR_LAUNCH_CHECK();
    return FRCNN_OK;
  }
  long total = (long)P * C * k * k;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(total, 256)), 4096);
  FR_LAUNCH(KC_ELEMWISE, 0, total * 8.0, s, col2im_positions_add_kernel, dim3(grid), dim3(256), 0, col, C, H, W, k, Wo, pos,
            P, gX);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- RNG (throughput runs)
__global__ void bernoulli_kernel(float* m, long n, float p, unsigned long long seed) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    m[i] = frcnn_keep_mask(seed, (unsigned long long)i, p);
}
__global__ void bernoulli_multi_kernel(DropoutJobs j) {
  const int k = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.C[k]; i += gridDim.x * blockDim.x)
    j.ptr[k][i] = frcnn_keep_mask(j.seed[k], (unsigned long long)i, j.p[k]);
}
// the SpatialDropout keep vectors of all blocks of a forward pass in ONE launch
int dropout_channel_masks(const DropoutJobs& j, hipStream_t s) {
  if (j.n <= 0) return FRCNN_OK;
  int maxC = 0;
  for (int k = 0; k < j.n; ++k) maxC = std::max(maxC, j.C[k]);
  FR_LAUNCH(KC_ELEMWISE, 0, maxC * 4.0 * j.n, s, bernoulli_multi_kernel, dim3(cdiv(maxC, 256), j.n), dim3(256), 0, j);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}
int dropout_channel_mask(float* scale, int C, float p, unsigned long long seed, hipStream_t s) {
  FR_LAUNCH(KC_ELEMWISE, 0, C * 4.0, s, bernoulli_kernel, dim3(cdiv(C, 256)), dim3(256), 0, scale, (long)C,
            p, seed);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}
int dropout_mask(float* mask, long n, float p, unsigned long long seed, hipStream_t s) {
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(n, 256)), 1024);
  FR_LAUNCH(KC_ELEMWISE, 0, n * 4.0, s, bernoulli_kernel, dim3(grid), dim3(256), 0, mask, n, p, seed);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- optim.rmsprop / optim.sgd / optim.nag / optim.adam
// The three optimisers of main.lua:122-124,133-135 on the flat vectors, and optim.adam beside them: HBM-bound passes of 3 to 8
// fp32 streams.  x = weights, g = the gradient the objective returned, v = the optimiser's state (rmsprop's m, state.dfdx of sgd
// and nag, adam's state.m), v2 = a second state vector where the Op declares one (kStates == 2: adam's state.v).
// The contract, stated once:
//   - one element of each update is ONE inline function (an Op's operator()), every Lua statement one separately rounded
//     fp32 operation (fp contract off), its variants template parameters and not per-element branches; an Op with
//     kStates == 2 takes (x, g, v, v2) and always reads and writes v2, one with kStates == 1 takes (x, g, v);
//   - ONE kernel, optim_kernel<Op>, applies it to any range [lo, hi) of 16-byte aligned vectors, and the whole vector is the
//     range [0, n) of that kernel.  So an update applied slice by slice (beside the backward pass, as slices of the gradient
//     become final) leaves the same bits as one pass over the whole vector, wherever a slice boundary falls.
// kScale: g is first multiplied by gscale (gradient:div(n), objective.lua:200, folded into the optimiser's pass: 6 streams
// instead of 2 + 5).  The gradient is written back only where Torch leaves something else in it than it was handed (that
// scale, weight decay, Nesterov's look-ahead term).
//
// optim.rmsprop:  g *= gscale ; m = alpha*m + (1-alpha)*g*g ; x -= lr * g / (sqrt(m) + eps).  m travels as v.
template <bool SCALE>
struct RmspropOp {
  static constexpr bool kScale = SCALE, kReadV = true, kWriteV = true, kWriteG = SCALE;
  static constexpr int kStates = 1;
  static constexpr int kStreams = 2 + kReadV + 1 + kWriteG + kWriteV;   // fp32 streams moved per element
  float gscale, lr, alpha, oma, eps;   // oma = 1 - alpha
  __device__ __forceinline__ void operator()(float& x, float& g, float& m) const {
#pragma clang fp contract(off)   // every operation rounded by itself: the same bits from every instantiation
    if (SCALE) g *= gscale;
    m = alpha * m + oma * (g * g);
    x = x - lr * g / (sqrtf(m) + eps);
  }
};

// optim.sgd:  g *= gscale ; g += wd*x ; v = g (first step) | v = v*mom + (1-damp)*g ; g += mom*v (nesterov) ; x += -clr*dir
// MOM: 0 = no momentum (v untouched, may be NULL), 1 = the first step (v = copy(g)), 2 = later steps
template <bool SCALE, bool WD, int MOM, bool NEST>
struct SgdOp {
  static constexpr bool kScale = SCALE, kReadV = MOM == 2, kWriteV = MOM != 0, kWriteG = SCALE || WD || NEST;
  static constexpr int kStates = 1;
  static constexpr int kStreams = 2 + kReadV + 1 + kWriteG + kWriteV;   // fp32 streams moved per element
  float gscale, clr, wd, mom, omd;   // omd = 1 - dampening
  __device__ __forceinline__ void operator()(float& x, float& g, float& v) const {
#pragma clang fp contract(off)   // every operation rounded by itself: the same bits from every kernel that calls this
    if (SCALE) g *= gscale;                      // gradient:div(n) (objective.lua:200)
    if (WD) g = g + wd * x;                      // dfdx:add(wd, x)
    float d = g;
    if (MOM == 1) v = g;                         // state.dfdx = torch.Tensor():typeAs(dfdx):resizeAs(dfdx):copy(dfdx)
    if (MOM == 2) v = v * mom + omd * g;         // state.dfdx:mul(mom):add(1-damp, dfdx)
    if (MOM != 0) {
      if (NEST) { g = g + mom * v; d = g; }      // dfdx:add(mom, state.dfdx)
      else d = v;                                // dfdx = state.dfdx
    }
    x = x + (-clr) * d;                          // x:add(-clr, dfdx)
  }
};

// optim.nag (after its look-ahead x += mom*v, nag_lookahead below):  g *= gscale ; g += wd*x ; v = 0 (first step) | v = v*mom ;
// v += -clr*g ; x += v.  The first step adds to a literal 0 (0 + -0 = +0, as fill(0):add(-clr, dfdx) leaves it).
template <bool SCALE, bool WD, bool FIRST>
struct NagOp {
  static constexpr bool kScale = SCALE, kReadV = !FIRST, kWriteV = true, kWriteG = SCALE || WD;
  static constexpr int kStates = 1;
  static constexpr int kStreams = 2 + kReadV + 1 + kWriteG + kWriteV;
  float gscale, clr, wd, mom;
  __device__ __forceinline__ void operator()(float& x, float& g, float& v) const {
#pragma clang fp contract(off)
    if (SCALE) g *= gscale;                      // gradient:div(n) (objective.lua:200)
    if (WD) g = g + wd * x;                      // dfdx:add(wd, x)
    const float u = (-clr) * g;
    v = (FIRST ? 0.0f : v * mom) + u;            // state.dfdx:fill(0) | :mul(mom), then :add(-clr, dfdx)
    x = x + v;                                   // x:add(state.dfdx)
  }
};

// optim.adam (optim/adam.lua), with AdamW's decoupled decay beside Torch's coupled one:  g *= gscale ; g += wd*x (WD == 1) ;
// m = m*beta1 + (1-beta1)*g ; v = v*beta2 + ((1-beta2)*g)*g ; denom = sqrt(v) + eps ; x += ndecay*x (WD == 2) ;
// x += (nstep*m)/denom.  nstep = -stepSize (the bias corrections folded in on the host, as adam.lua does), ndecay =
// -(clr*weightDecay).  m travels as v, v as v2; both are read and written on every step (the host creates them as zeros, as
// Torch does), state.denom is not kept.  7 fp32 streams, 8 where g is written back.
template <bool SCALE, int WD>
struct AdamOp {
  static constexpr bool kScale = SCALE, kReadV = true, kWriteV = true, kWriteG = SCALE || WD == 1;
  static constexpr int kStates = 2;
  static constexpr int kStreams = 2 + kReadV + 1 + kWriteG + kWriteV + 2;   // (+ 2: v2 read and written)
  float gscale, nstep, beta1, omb1, beta2, omb2, eps, wd, ndecay;   // omb = 1 - beta
  __device__ __forceinline__ void operator()(float& x, float& g, float& m, float& v) const {
#pragma clang fp contract(off)
    if (SCALE) g = g * gscale;                   // gradient:div(n) (objective.lua:200)
    if (WD == 1) g = g + wd * x;                 // dfdx:add(wd, x)
    m = m * beta1 + omb1 * g;                    // state.m:mul(beta1):add(1-beta1, dfdx)
    v = v * beta2 + (omb2 * g) * g;              // state.v:mul(beta2):addcmul(1-beta2, dfdx, dfdx)
    const float d = sqrtf(v) + eps;              // state.denom:copy(state.v):sqrt():add(epsilon)
    if (WD == 2) x = x + ndecay * x;             // AdamW: the decay leaves the gradient and the moments alone
    x = x + (nstep * m) / d;                     // x:addcdiv(-stepSize, state.m, state.denom)
  }
};

template <class Op>
__device__ __forceinline__ void optim_four(float4* x4, float4* g4, float4* v4, float4* u4, long i, const Op& op) {
  float4 xv = x4[i], gv = g4[i], vv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (Op::kReadV) vv = v4[i];
  if constexpr (Op::kStates == 2) {
    float4 uv = u4[i];
    op(xv.x, gv.x, vv.x, uv.x);
    op(xv.y, gv.y, vv.y, uv.y);
    op(xv.z, gv.z, vv.z, uv.z);
    op(xv.w, gv.w, vv.w, uv.w);
    u4[i] = uv;
  } else {
    op(xv.x, gv.x, vv.x);
    op(xv.y, gv.y, vv.y);
    op(xv.z, gv.z, vv.z);
    op(xv.w, gv.w, vv.w);
  }
  if (Op::kWriteG) g4[i] = gv;
  if (Op::kWriteV) v4[i] = vv;
  x4[i] = xv;
}
template <class Op>
__device__ __forceinline__ void optim_scalar(float* x, float* g, float* v, float* u, long i, const Op& op) {
  float xi = x[i], gi = g[i], vi = 0.f;
  if (Op::kReadV) vi = v[i];
  if constexpr (Op::kStates == 2) {
    float ui = u[i];
    op(xi, gi, vi, ui);
    u[i] = ui;
  } else {
    op(xi, gi, vi);
  }
  if (Op::kWriteG) g[i] = gi;
  if (Op::kWriteV) v[i] = vi;
  x[i] = xi;
}

// elements [lo, hi) of 16-byte aligned vectors: 16-byte groups grid-stride where the range covers them whole, the up to three
// elements in front of the first and behind the last such group one by one (thread t < 8 of block 0).  v2 comes last: an Op
// with one state vector never looks at it, and the arguments it does read sit at the offsets they have without it
template <class Op>
__global__ void optim_kernel(float* __restrict__ x, float* __restrict__ g, float* __restrict__ v, long lo, long hi, Op op,
                             const double* __restrict__ gcount, float* __restrict__ v2) {
  // gcount: the divisor of gradient:div (objective.lua:200) read from the device -- the all-reduced example count of a
  // data-parallel step, which no host has seen yet (a count of 0 leaves the gradient as it is)
  if (Op::kScale && gcount) { const double c = *gcount; op.gscale = c > 0.0 ? (float)(1.0 / c) : 1.0f; }
  const long a = min(hi, (lo + 3) & ~3L), b = max(a, hi & ~3L);   // [lo, a) ragged | [a, b) whole groups | [b, hi) ragged
  const long n4 = (b - a) >> 2;
  float4* x4 = reinterpret_cast<float4*>(x + a);
  float4* g4 = reinterpret_cast<float4*>(g + a);
  float4* v4 = reinterpret_cast<float4*>(Op::kReadV || Op::kWriteV ? v + a : v);
  float4* u4 = reinterpret_cast<float4*>(Op::kStates == 2 ? v2 + a : v2);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
    optim_four(x4, g4, v4, u4, i, op);
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const int t = threadIdx.x;
    const long i = t < 4 ? lo + t : b + (t - 4);
    if (t < 4 ? i < a : i < hi) optim_scalar(x, g, v, v2, i, op);
  }
}

namespace {
struct OptimRange {
  float* x; float* g; float* v; float* v2;   // v2: the second state vector of an Op with kStates == 2, else NULL
  long lo, hi;
  bool slice;             // a slice beside the backward pass (its grid capped lower) or the whole vector [0, hi)
  const double* gcount;   // the divisor on the device (NULL: the host's gscale)
  hipStream_t s;
};

template <class Op>
int optim_launch(const Op& op, const OptimRange& r) {
  const long n = r.hi - r.lo;
  if (n == 0) return FRCNN_OK;
  const double bytes = 4.0 * Op::kStreams * n;
  // a slice takes half the wave slots at most: it runs BESIDE other launches (the backward pass) and must not keep them waiting for slots
  const int grid = (int)std::min<long>(std::max<long>(1, cdivl(n / 4, 256)), r.slice ? 1024 : 2048);
  FR_LAUNCH(KC_OPTIM, 0, bytes, r.s, optim_kernel<Op>, dim3(grid), dim3(256), 0, r.x, r.g, r.v, r.lo, r.hi, op, r.gcount, r.v2);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

template <bool SCALE, bool WD, int MOM, bool NEST>
int sgd_go(const OptimRange& r, float gscale, float clr, float wd, float mom, float omd) {
  return optim_launch(SgdOp<SCALE, WD, MOM, NEST>{gscale, clr, wd, mom, omd}, r);
}
template <bool SCALE, bool WD>
int sgd_mom(const OptimRange& r, float gscale, float clr, float wd, float mom, float omd, bool nesterov, bool first) {
  if (mom == 0.f) return sgd_go<SCALE, WD, 0, false>(r, gscale, clr, wd, mom, omd);
  if (first)
    return nesterov ? sgd_go<SCALE, WD, 1, true>(r, gscale, clr, wd, mom, omd) : sgd_go<SCALE, WD, 1, false>(r, gscale, clr, wd, mom, omd);
  return nesterov ? sgd_go<SCALE, WD, 2, true>(r, gscale, clr, wd, mom, omd) : sgd_go<SCALE, WD, 2, false>(r, gscale, clr, wd, mom, omd);
}
template <bool SCALE, bool WD>
int nag_go(const OptimRange& r, float gscale, float clr, float wd, float mom, bool first) {
  return first ? optim_launch(NagOp<SCALE, WD, true>{gscale, clr, wd, mom}, r)
               : optim_launch(NagOp<SCALE, WD, false>{gscale, clr, wd, mom}, r);
}

int optim_check(const char* what, const OptimRange& r, bool uses_v, bool uses_v2 = false) {
  FR_CHECK(r.x && r.g && (r.v || !uses_v) && (r.v2 || !uses_v2), "%s: NULL vector", what);
  FR_CHECK((((uintptr_t)r.x | (uintptr_t)r.g | (uintptr_t)r.v | (uintptr_t)r.v2) & 15) == 0, "%s: the vectors must be 16-byte aligned", what);
  FR_CHECK(r.lo >= 0 && r.lo <= r.hi, "%s: bad range [%ld, %ld)", what, r.lo, r.hi);
  return FRCNN_OK;
}
}  // namespace

int rmsprop_update(float* x, float* g, float* m, long lo, long hi, bool slice, float gscale, const double* gcount_dev, float lr,
                   float alpha, float eps, hipStream_t s) {
  const OptimRange r{x, g, m, nullptr, lo, hi, slice, gcount_dev, s};
  FR_TRY(optim_check("rmsprop", r, true));
  const float oma = 1.0f - alpha;
  if (r.gcount || gscale != 1.f) return optim_launch(RmspropOp<true>{gscale, lr, alpha, oma, eps}, r);
  return optim_launch(RmspropOp<false>{1.f, lr, alpha, oma, eps}, r);
}

int sgd_update(float* x, float* g, float* v, long lo, long hi, bool slice, float gscale, const double* gcount_dev, float clr,
               float wd, float mom, float one_minus_damp, bool nesterov, bool first, hipStream_t s) {
  const OptimRange r{x, g, mom != 0.f ? v : nullptr, nullptr, lo, hi, slice, gcount_dev, s};
  FR_TRY(optim_check("sgd", r, mom != 0.f));
  FR_CHECK(!nesterov || (mom > 0.f && one_minus_damp == 1.f), "sgd: Nesterov momentum requires a momentum and zero dampening");
  const bool scale = r.gcount || gscale != 1.f;
  if (scale)
    return wd != 0.f ? sgd_mom<true, true>(r, gscale, clr, wd, mom, one_minus_damp, nesterov, first)
                     : sgd_mom<true, false>(r, gscale, clr, wd, mom, one_minus_damp, nesterov, first);
  return wd != 0.f ? sgd_mom<false, true>(r, 1.f, clr, wd, mom, one_minus_damp, nesterov, first)
                   : sgd_mom<false, false>(r, 1.f, clr, wd, mom, one_minus_damp, nesterov, first);
}

int nag_update(float* x, float* g, float* v, long lo, long hi, bool slice, float gscale, const double* gcount_dev, float clr,
               float wd, float mom, bool first, hipStream_t s) {
  const OptimRange r{x, g, v, nullptr, lo, hi, slice, gcount_dev, s};
  FR_TRY(optim_check("nag", r, true));
  FR_CHECK(mom > 0.f, "nag: momentum must be positive for Nesterov Accelerated Gradient");
  const bool scale = r.gcount || gscale != 1.f;
  if (scale) return wd != 0.f ? nag_go<true, true>(r, gscale, clr, wd, mom, first) : nag_go<true, false>(r, gscale, clr, wd, mom, first);
  return wd != 0.f ? nag_go<false, true>(r, 1.f, clr, wd, mom, first) : nag_go<false, false>(r, 1.f, clr, wd, mom, first);
}

int adam_update(float* x, float* g, float* m, float* v, long lo, long hi, bool slice, float gscale, const double* gcount_dev,
                float step, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float wd, float decay,
                hipStream_t s) {
  const OptimRange r{x, g, m, v, lo, hi, slice, gcount_dev, s};
  FR_TRY(optim_check("adam", r, true, true));
  FR_CHECK(wd == 0.f || decay == 0.f, "adam: weight decay is either coupled (wd) or decoupled (decay), not both");
  const bool scale = r.gcount || gscale != 1.f;
  const float gs = scale ? gscale : 1.f;
  const float nstep = -step, ndecay = -decay;   // both arrive positive, as Torch's stepSize and clr*weightDecay
#define FR_ADAM(SCALE, WD) optim_launch(AdamOp<SCALE, WD>{gs, nstep, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, wd, ndecay}, r)
  if (scale) return wd != 0.f ? FR_ADAM(true, 1) : decay != 0.f ? FR_ADAM(true, 2) : FR_ADAM(true, 0);
  return wd != 0.f ? FR_ADAM(false, 1) : decay != 0.f ? FR_ADAM(false, 2) : FR_ADAM(false, 0);
#undef FR_ADAM
}

// optim.nag's look-ahead before opfunc: x:add(mom, state.dfdx).  3 streams.
__global__ void nag_lookahead_kernel(float* __restrict__ x, const float* __restrict__ v, long n, float mom) {
#pragma clang fp contract(off)
  const long n4 = n >> 2;
  float4* x4 = reinterpret_cast<float4*>(x);
  const float4* v4 = reinterpret_cast<const float4*>(v);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 xv = x4[i];
    const float4 vv = v4[i];
    xv.x = xv.x + mom * vv.x; xv.y = xv.y + mom * vv.y; xv.z = xv.z + mom * vv.z; xv.w = xv.w + mom * vv.w;
    x4[i] = xv;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    x[i] = x[i] + mom * v[i];
}
int nag_lookahead(float* x, const float* v, long n, float mom, hipStream_t s) {
  FR_CHECK(x && v, "nag_lookahead: NULL vector");
  FR_CHECK((((uintptr_t)x | (uintptr_t)v) & 15) == 0, "nag_lookahead: the vectors must be 16-byte aligned");
  FR_CHECK(n >= 0, "nag_lookahead: bad length %ld", n);
  if (n == 0) return FRCNN_OK;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(n / 4, 256)), 2048);
  FR_LAUNCH(KC_OPTIM, 0, n * 12.0, s, nag_lookahead_kernel, dim3(grid), dim3(256), 0, x, v, n, mom);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// the look-ahead on elements [lo, hi) only (staged training: a frozen slice keeps its weights); the same statement per element
__global__ void nag_lookahead_slice_kernel(float* __restrict__ x, const float* __restrict__ v, long lo, long hi, float mom) {
#pragma clang fp contract(off)
  for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long)gridDim.x * blockDim.x)
    x[i] = x[i] + mom * v[i];
}
int nag_lookahead_slice(float* x, const float* v, long lo, long hi, float mom, hipStream_t s) {
  FR_CHECK(x && v, "nag_lookahead_slice: NULL vector");
  FR_CHECK(lo >= 0 && lo <= hi, "nag_lookahead_slice: bad range [%ld, %ld)", lo, hi);
  const long n = hi - lo;
  if (n == 0) return FRCNN_OK;
  int grid = (int)std::min<long>(std::max<long>(1, cdivl(n, 256)), 2048);
  FR_LAUNCH(KC_OPTIM, 0, n * 12.0, s, nag_lookahead_slice_kernel, dim3(grid), dim3(256), 0, x, v, lo, hi, mom);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- the gradient guard (norm clipping, non-finite steps)
// include/frcnn_hip.h "gradient-norm clipping" defines what is computed.  S = sum over the trainable slices of (double)g*(double)g:
// every product is exact in fp64 (24-bit significands), the sum runs in fp64 in an order fixed by n and the slice bounds alone --
// a thread always adds the same elements in the same order (one fp64 addition per element), a block's 256 sums meet in a fixed
// tree, and one block folds the per-block partials in a fixed order.  No atomics: two calls on the same data leave the same bits.
struct ClipRanges {
  int n;
  long lo[GRAD_CLIP_MAX_RANGES], hi[GRAD_CLIP_MAX_RANGES];
};

// acc += (double)e * (double)e for the four elements in index order, one rounding each (the product is exact, so the fused form
// rounds what a separate add would): a zero element leaves acc as it is, bit for bit
__device__ __forceinline__ double sumsq_add(double acc, const float4 v) {
  acc = fma((double)v.x, (double)v.x, acc);
  acc = fma((double)v.y, (double)v.y, acc);
  acc = fma((double)v.z, (double)v.z, acc);
  return fma((double)v.w, (double)v.w, acc);
}

// 16-byte group q of g (elements [4q, 4q+4)) with everything outside [lo, hi) read as zero: one 16-byte load where the slice
// covers the group, element by element at a slice's ragged ends
__device__ __forceinline__ float4 load_group(const float* __restrict__ g, long q, long lo, long hi) {
  const long base = q << 2;
  if (base >= lo && base + 4 <= hi) return *reinterpret_cast<const float4*>(g + base);
  float e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = (base + j >= lo && base + j < hi) ? g[base + j] : 0.f;
  return make_float4(e[0], e[1], e[2], e[3]);
}

// The work is dealt out by ABSOLUTE position: group q of the vector always belongs to thread q mod (grid * 256), which adds its
// groups in ascending order, the even and the odd of its visits into two accumulators (two loads in flight).  Which slices are
// summed changes what is added, never who adds it or when: the sum over slices whose complement holds exact zeros (the frozen
// slices of a staged pass) is the sum over the whole vector, bit for bit.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, ClipRanges r, double* __restrict__ partial) {
  __shared__ double sh[16];
  double s0 = 0.0, s1 = 0.0;
  const long stride = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < r.n; ++k) {
    const long lo = r.lo[k], hi = r.hi[k];
    const long q0 = lo >> 2, q1 = (hi + 3) >> 2;            // the groups the slice touches
    long visit = q0 > t ? (q0 - t) / stride : 0;            // the thread's last visit at or before q0 ...
    visit &= ~1L;                                           // ... of even number: the pairing below is that of the whole vector
    for (long q = t + visit * stride; q < q1; q += 2 * stride) {
      const long q2 = q + stride;
      const float4 u = q >= q0 ? load_group(g, q, lo, hi) : zero;
      const float4 w = (q2 >= q0 && q2 < q1) ? load_group(g, q2, lo, hi) : zero;
      s0 = sumsq_add(s0, u);
      s1 = sumsq_add(s1, w);
    }
  }
  const double tot = block_sum_d(s0 + s1, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// record = {S, norm, D', skipped}.  Thread t folds partials [t*per, (t+1)*per) in index order, the 256 sums meet in the fixed tree
// of block_sum_d.  sqrt, / and * in fp64 are correctly rounded (no contraction, no reciprocal shortcut): a host that repeats the
// three operations on the recorded S gets the recorded D' bit for bit.
__global__ __launch_bounds__(256) void grad_clip_finish_kernel(const double* __restrict__ partial, int nparts, double divisor,
                                                              const double* __restrict__ divisor_dev, double clip_norm,
                                                              double* __restrict__ record) {
#pragma clang fp contract(off)
  __shared__ double sh[16];
  const int per = (nparts + 255) / 256;
  double v = 0.0;
  for (int i = threadIdx.x * per; i < min(nparts, (threadIdx.x + 1) * per); ++i) v += partial[i];
  const double S = block_sum_d(v, sh);
  if (threadIdx.x == 0) {
    double D = divisor_dev ? *divisor_dev : divisor;
    if (!(D > 0.0)) D = 1.0;                                 // (a count of 0 leaves the gradient as it is: optim_kernel)
    const double norm = __ddiv_rn(__dsqrt_rn(S), D);
    const bool finite = S < __builtin_huge_val();            // false for +inf and for NaN (S is a sum of squares: never negative)
    double Dc = D;
    if (finite && clip_norm > 0.0) {
      const double ratio = __ddiv_rn(norm, clip_norm);
      if (ratio > 1.0) Dc = __dmul_rn(D, ratio);
    }
    record[0] = S; record[1] = norm; record[2] = Dc; record[3] = finite ? 0.0 : 1.0;
  }
}

// a non-finite step: the gradient counts as zero on the trainable slices (every block reads the flag; 0: nothing to do)
__global__ __launch_bounds__(256) void grad_zero_if_kernel(float* __restrict__ g, ClipRanges r, const double* __restrict__ record) {
  if (record[3] == 0.0) return;
  const long stride = (long)gridDim.x * blockDim.x;
  for (int k = 0; k < r.n; ++k) {
    const long lo = r.lo[k], hi = r.hi[k];
    const long a = min(hi, (lo + 3) & ~3L), b = max(a, hi & ~3L);
    const long n4 = (b - a) >> 2;
    float4* g4 = reinterpret_cast<float4*>(g + a);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0 && threadIdx.x < 8) {
      const int t = threadIdx.x;
      const long j = t < 4 ? lo + t : b + (t - 4);
      if (t < 4 ? j < a : j < hi) g[j] = 0.f;
    }
  }
}

// the grid of the two passes over g, from n alone (the RMSprop pass's sizing): also the number of partials
static int grad_clip_grid(long n) { return (int)std::min<long>(std::max<long>(1, cdivl(n / 4, 256)), 2048); }
size_t grad_clip_workspace_bytes(long n) { return (size_t)grad_clip_grid(std::max<long>(n, 0)) * sizeof(double); }

int grad_clip(float* g, long n, const long long* ranges_host, int nranges, double divisor, const double* divisor_dev, double clip_norm,
              double* record, void* workspace, size_t workspace_bytes, hipStream_t s) {
  FR_CHECK(g && record && workspace, "grad_clip: NULL gradient, record or workspace");
  FR_CHECK(n >= 0, "grad_clip: bad length %ld", n);
  FR_CHECK(((uintptr_t)g & 15) == 0, "grad_clip: the gradient must be 16-byte aligned");
  FR_CHECK((((uintptr_t)record | (uintptr_t)workspace | (uintptr_t)divisor_dev) & 7) == 0,
           "grad_clip: the record, the workspace and the device divisor must be 8-byte aligned");
  FR_CHECK(workspace_bytes >= grad_clip_workspace_bytes(n), "grad_clip: workspace of %zu bytes, %zu needed", workspace_bytes,
           grad_clip_workspace_bytes(n));
  FR_CHECK(divisor_dev || divisor > 0.0, "grad_clip: the divisor must be positive (1: nothing to scale)");   // (NaN fails too)
  FR_CHECK(clip_norm == clip_norm && clip_norm < __builtin_huge_val(), "grad_clip: clip_norm must be a finite number (<= 0: no clipping)");
  FR_CHECK(ranges_host || nranges == 0, "grad_clip: %d ranges without a range list", nranges);
  FR_CHECK(nranges >= 0 && nranges <= GRAD_CLIP_MAX_RANGES, "grad_clip: %d ranges (at most %d)", nranges, GRAD_CLIP_MAX_RANGES);
  ClipRanges r;
  r.n = 0;
  if (!ranges_host) {
    r.n = 1; r.lo[0] = 0; r.hi[0] = n;
  } else {
    long prev = 0;
    for (int k = 0; k < nranges; ++k) {
      const long lo = ranges_host[2 * k], hi = ranges_host[2 * k + 1];
      FR_CHECK(lo >= 0 && lo <= hi && hi <= n, "grad_clip: bad range [%ld, %ld) of %ld elements", lo, hi, n);
      FR_CHECK(lo >= prev, "grad_clip: the ranges must be sorted and must not overlap ([%ld, %ld) after an end of %ld)", lo, hi, prev);
      prev = hi;
      if (lo < hi) { r.lo[r.n] = lo; r.hi[r.n] = hi; ++r.n; }
    }
  }
  long covered = 0;
  for (int k = 0; k < r.n; ++k) covered += r.hi[k] - r.lo[k];
  const int grid = grad_clip_grid(n);
  double* partial = static_cast<double*>(workspace);
  FR_LAUNCH(KC_OPTIM, 0, covered * 4.0, s, grad_sumsq_kernel, dim3(grid), dim3(256), 0, g, r, partial);
  FR_LAUNCH_CHECK();
  FR_LAUNCH(KC_OPTIM, 0, grid * 8.0, s, grad_clip_finish_kernel, dim3(1), dim3(256), 0, partial, grid, divisor, divisor_dev, clip_norm, record);
  FR_LAUNCH_CHECK();
  FR_LAUNCH(KC_OPTIM, 0, 0.0, s, grad_zero_if_kernel, dim3(grid), dim3(256), 0, g, r, record);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
