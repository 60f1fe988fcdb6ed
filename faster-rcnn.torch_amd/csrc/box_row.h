// box_row.h -- the row product of the per-class box head (include/frcnn_hip_box.h), shared by its two readers: the forward kernel
// of box_head.hip (one class a row, chosen by the class source) and the class-row kernel of class_boxes.hip (one class a ROW OF
// THE CLASS TEST, cfg.scoring.boxes = "class").  One definition, so that both give the same bits on the same feature row: the
// translation units that include it are built with the same flags and leave the floating-point contraction mode at its default
// up to this point.
#pragma once

namespace frcnn {

static constexpr int BH_WAVE = 64;

// fixed-order sum of one value per lane over the wave (butterfly: every lane ends with the same bits)
__device__ __forceinline__ float bh_wave_sum(float v) {
#pragma unroll
  for (int o = BH_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, BH_WAVE);
  return v;
}

// a[j] = sum_k xr[k] w0[j nf + k], j = 0 ... 3, by the wave that owns the row: lane l sums the pieces l, l + 64, ... (64
// interleaved partial sums), the butterfly folds them; every lane returns the four sums.  VEC: 16-byte pieces of the row and of
// the four weight rows (nf % 4 == 0, xr and w0 16-byte aligned), else one float at a time.
template <bool VEC>
__device__ __forceinline__ void bh_row_product(const float* __restrict__ xr, const float* __restrict__ w0, int nf, int lane, float& r0,
                                               float& r1, float& r2, float& r3) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (VEC) {
    const int nq = nf >> 2;
    const float4* xq = reinterpret_cast<const float4*>(xr);
    const float4* q0 = reinterpret_cast<const float4*>(w0);
    const float4* q1 = reinterpret_cast<const float4*>(w0 + nf);
    const float4* q2 = reinterpret_cast<const float4*>(w0 + 2 * (size_t)nf);
    const float4* q3 = reinterpret_cast<const float4*>(w0 + 3 * (size_t)nf);
    for (int q = lane; q < nq; q += BH_WAVE) {
      const float4 v = xq[q];
      const float4 u0 = q0[q], u1 = q1[q], u2 = q2[q], u3 = q3[q];
      a0 += v.x * u0.x + v.y * u0.y + v.z * u0.z + v.w * u0.w;
      a1 += v.x * u1.x + v.y * u1.y + v.z * u1.z + v.w * u1.w;
      a2 += v.x * u2.x + v.y * u2.y + v.z * u2.z + v.w * u2.w;
      a3 += v.x * u3.x + v.y * u3.y + v.z * u3.z + v.w * u3.w;
    }
  } else {
    for (int k = lane; k < nf; k += BH_WAVE) {
      const float v = xr[k];
      a0 += v * w0[k];
      a1 += v * w0[(size_t)nf + k];
      a2 += v * w0[2 * (size_t)nf + k];
      a3 += v * w0[3 * (size_t)nf + k];
    }
  }
  r0 = bh_wave_sum(a0); r1 = bh_wave_sum(a1); r2 = bh_wave_sum(a2); r3 = bh_wave_sum(a3);
}

}  // namespace frcnn
