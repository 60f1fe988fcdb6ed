// class_boxes.hip -- the per-class boxes of the class test's rows (cfg.scoring.boxes = "class"; include/frcnn_hip_classbox.h).
// Under cfg.scoring.classes = "all" frcnn_detect_classes_batch emits one row per (candidate, foreground class) and gives all the
// rows of a candidate the one box the net wrote for it.  A per-class box head (cfg.box_head) predicts a box for EVERY class of a
// candidate; this kernel computes, for each emitted row (r, c), the four deltas of class c on candidate r's feature row -- 4 of
// the 4 C columns of the dense R x 4C product, the ones that are needed -- and decodes them against the candidate's anchor.
//   the deltas  bh_row_product (box_row.h), the row product of box_head_forward_kernel: the same bits as
//               frcnn_box_head_forward with class c on that feature row
//   the decode  anchor_to_input (anchor_decode.h), the one of detect_post and detect_classes_batch, fp64, contraction off
// One launch per group of CB_GROUP frames, the frame a grid dimension; every frame's first feature row is a host value and
// travels by value as a kernel argument (the way detect_classes_batch carries its descriptors), its row count is read on the
// device.  No atomics, no workspace: every output element has one writer and is a function of the inputs alone.
#include "kernels.h"
#include "box_row.h"
#include "anchor_decode.h"

namespace frcnn {

constexpr int CB_WAVES = 4;      // rows a workgroup takes per round: one wave a row
constexpr int CB_GROUP = 64;     // frames a launch
constexpr int CB_BLOCKS = 2048;  // workgroups a launch at most (row tiles x frames): a frame's tiles walk its rows in rounds
struct ClassBoxGroup { long long row0[CB_GROUP]; };
static_assert(sizeof(ClassBoxGroup) <= 1024, "the descriptors of a group travel as a kernel argument");

// Grid (row tiles, frames of the group).  Wave w of tile t takes rows j = 4 t + w, then + 4 gridDim.x, ... below
// min(K_dev[b], row_stride).  The rows of a candidate are adjacent (detect_classes_batch emits candidate-major), so the waves of
// a workgroup mostly read ONE feature row: once from memory, then from the cache.
template <bool VEC>
__global__ __launch_bounds__(CB_WAVES * BH_WAVE) void detect_class_boxes_kernel(
    ClassBoxGroup g, int b0, const float* __restrict__ feat, int nf, const float* __restrict__ W, const float* __restrict__ bias, int C,
    const double* __restrict__ rect, const long long* __restrict__ pick, long long match_stride, const int* __restrict__ kc,
    const int* __restrict__ keep_row, const int* __restrict__ K_dev, int row_stride, float* __restrict__ bb, double* __restrict__ r2out) {
  const int b = b0 + blockIdx.y;
  const int K = min(K_dev[b], row_stride);
  const int lane = threadIdx.x & (BH_WAVE - 1);
  feat += (size_t)g.row0[blockIdx.y] * nf;
  rect += (size_t)b * match_stride * 4; pick += (size_t)b * match_stride;
  const size_t so = (size_t)b * row_stride;
  for (int j = blockIdx.x * CB_WAVES + (threadIdx.x >> 6); j < K; j += gridDim.x * CB_WAVES) {   // (wave-uniform)
    const int r = keep_row[so + j];
    if (r < 0 || r >= match_stride) continue;                          // (a caller's table: never an index before it is checked)
    int c = kc[so + j];
    if (c < 1 || c > C) c = 0;                                         // no class: zero deltas, nothing is read for them
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (c) {
      float a0, a1, a2, a3;
      const float* w0 = W + (size_t)(4 * (c - 1)) * nf;
      bh_row_product<VEC>(feat + (size_t)r * nf, w0, nf, lane, a0, a1, a2, a3);
      const float* bc = bias + 4 * (c - 1);
      d[0] = a0 + bc[0]; d[1] = a1 + bc[1]; d[2] = a2 + bc[2]; d[3] = a3 + bc[3];
    }
    if (lane == 0) {
      const long long p = pick[r];
      if (p >= 1 && p <= match_stride) {
        double q[4];
        anchor_to_input(rect + 4 * (size_t)(p - 1), d, q);
        double* o = r2out + 4 * (so + j);
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
        float* x = bb + 5 * (so + j);                                  // (column 5, the confidence, stays)
        x[0] = (float)q[0]; x[1] = (float)q[1]; x[2] = (float)q[2]; x[3] = (float)q[3];
      }
    }
  }
}

int detect_class_boxes_batch(const float* feat, int nf, const long long* row0, int B, const float* W, const float* b, int C,
                             const double* rect, const long long* pick, long long match_stride, const int* kc, const int* keep_row,
                             const int* K_dev, int row_stride, float* bb, double* r2, hipStream_t s) {
  // everything is checked before the first launch: a refused call has written nothing
  FR_CHECK(B >= 0 && B <= 65535, "detect_class_boxes_batch: %d frames (0 ... 65535)", B);
  FR_CHECK(nf >= 1, "detect_class_boxes_batch: %d features (at least 1)", nf);
  FR_CHECK(C >= 1, "detect_class_boxes_batch: %d classes (at least 1)", C);
  FR_CHECK((long long)4 * C * nf < (1ll << 31), "detect_class_boxes_batch: 4 x %d x %d weights do not fit an int", C, nf);
  FR_CHECK(row_stride >= 0 && match_stride >= 0, "detect_class_boxes_batch: negative stride (%d / %lld)", row_stride, match_stride);
  if (B == 0 || row_stride == 0) return FRCNN_OK;
  FR_CHECK(feat && row0 && W && b && rect && pick && kc && keep_row && K_dev && bb && r2, "detect_class_boxes_batch: NULL argument");
  FR_CHECK(((uintptr_t)feat | (uintptr_t)W | (uintptr_t)b | (uintptr_t)kc | (uintptr_t)keep_row | (uintptr_t)K_dev | (uintptr_t)bb) % 4 == 0
               && ((uintptr_t)rect | (uintptr_t)pick | (uintptr_t)r2) % 8 == 0,
           "detect_class_boxes_batch: a pointer is not aligned to its element");
  for (int i = 0; i < B; ++i)
    FR_CHECK(row0[i] >= 0, "detect_class_boxes_batch: frame %d has row0 %lld (negative)", i, row0[i]);
  const bool vec = nf % 4 == 0 && (((uintptr_t)feat | (uintptr_t)W) % 16) == 0;
  for (int b0 = 0; b0 < B; b0 += CB_GROUP) {
    const int nb = std::min(B - b0, CB_GROUP);
    ClassBoxGroup g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < nb; ++i) g.row0[i] = row0[b0 + i];
    const dim3 grid(std::max(1, std::min(cdiv(row_stride, CB_WAVES), CB_BLOCKS / nb)), nb);
    // (the rows are counted on the device: the profile's flops and bytes are those of full segments, an upper bound)
    const double rows = (double)nb * row_stride;
    if (vec)
      FR_LAUNCH(KC_ELEMWISE, 8.0 * rows * nf, rows * (8.0 * nf + 96.0), s, detect_class_boxes_kernel<true>, grid, dim3(CB_WAVES * BH_WAVE),
                0, g, b0, feat, nf, W, b, C, rect, pick, match_stride, kc, keep_row, K_dev, row_stride, bb, r2);
    else
      FR_LAUNCH(KC_ELEMWISE, 8.0 * rows * nf, rows * (8.0 * nf + 96.0), s, detect_class_boxes_kernel<false>, grid,
                dim3(CB_WAVES * BH_WAVE), 0, g, b0, feat, nf, W, b, C, rect, pick, match_stride, kc, keep_row, K_dev, row_stride, bb, r2);
  }
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
