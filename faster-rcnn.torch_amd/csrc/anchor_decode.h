// anchor_decode.h -- Anchors.anchorToInput (Anchors.lua:245-252) + Rect.fromXYWidthHeight on the device, for the kernels that
// decode a box: detect_post, detect_classes_batch (detect.hip) and detect_class_boxes_batch (class_boxes.hip).  One definition, so
// that a box decoded by any of them from the same anchor and the same deltas has the same bits.
#pragma once
#include <cmath>

namespace frcnn {

// a = the anchor's input rect, t = the net's 4 deltas; products and sums separately rounded, as Lua numbers are: contraction is
// off for this body whatever the including translation unit's mode is
__device__ __forceinline__ void anchor_to_input(const double* __restrict__ a, const float* __restrict__ t, double* __restrict__ o) {
#pragma clang fp contract(off)
  const double aw = a[2] - a[0], ah = a[3] - a[1];
  double x0 = (double)t[0] * aw; x0 = x0 + a[0];
  double y0 = (double)t[1] * ah; y0 = y0 + a[1];
  const double ew = exp((double)t[2]) * aw, eh = exp((double)t[3]) * ah;
  o[0] = x0; o[1] = y0; o[2] = x0 + ew; o[3] = y0 + eh;
}

}  // namespace frcnn
