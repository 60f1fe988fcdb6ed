// roi_fix.h -- the 64-bit fixed-point accumulation of the deterministic ROI backward passes (roi.hip, roi_align.hip): the
// contributions are accumulated as value * 2^44, rounded to nearest.  Integer addition is exact, so the sum does not depend on the
// order in which the atomics land.  |g| < 2^18, resolution 6e-14.
#pragma once
#include "kernels.h"

namespace frcnn {

#define ROI_FIX_SCALE 17592186044416.0   /* 2^44 */
__device__ __forceinline__ long long roi_to_fix(float g) { return __double2ll_rn((double)g * ROI_FIX_SCALE); }
// gmap[t] += fix[t] / 2^44 for t < n (roi_fix_apply_kernel, roi.hip)
int roi_fix_apply(const unsigned long long* fix, long n, float* gmap, hipStream_t s);

}  // namespace frcnn
