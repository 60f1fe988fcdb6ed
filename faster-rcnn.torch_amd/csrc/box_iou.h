// box_iou.h -- the box arithmetic of the reference's nms (nms.lua:35, 78-96), shared by nms.hip, soft_nms.hip and box_vote.hip:
// who suppresses, decays or votes for whom is the same function of the boxes' bits in all three.  fp32, every operation rounded
// on its own -- contraction is switched off inside each body, wherever the header is included.
#pragma once

namespace frcnn {

// area = (x2 - x1 + 1) * (y2 - y1 + 1)                                                nms.lua:35
__device__ __forceinline__ float box_area(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  float dx = x2 - x1;
  float dy = y2 - y1;
  dx = dx + 1.0f;
  dy = dy + 1.0f;
  return dx * dy;
}

// IoU of box j (area ja) and box m (area ma): w = max(0, (xx2 + (-1) * xx1) + 1), h likewise;
// iou = (w * h) / ((ja + ma) - w * h)                                                   nms.lua:78-96
__device__ __forceinline__ float box_iou(float jx1, float jy1, float jx2, float jy2, float ja,
                                         float mx1, float my1, float mx2, float my2, float ma) {
#pragma clang fp contract(off)
  float xx1 = jx1 > mx1 ? jx1 : mx1;  // cmax, nms.lua:78
  float yy1 = jy1 > my1 ? jy1 : my1;
  float xx2 = jx2 < mx2 ? jx2 : mx2;  // cmin, nms.lua:80
  float yy2 = jy2 < my2 ? jy2 : my2;
  float w = xx2 + (-1.0f) * xx1;
  w = w + 1.0f;
  w = w > 0.0f ? w : 0.0f;
  float h = yy2 + (-1.0f) * yy1;
  h = h + 1.0f;
  h = h > 0.0f ? h : 0.0f;
  float inter = w * h;
  float denom = ja + ma;
  denom = denom - inter;
  return inter / denom;
}

}  // namespace frcnn
