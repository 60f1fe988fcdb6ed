// cnet_loss.hip -- the losses of the classification net, row by row (cfg.cnet_loss; not in the reference beyond its defaults):
// NLL, label-smoothed NLL or focal loss on the class log-probabilities, SmoothL1 or GIoU on the box deltas.
// Semantics and arithmetic: include/frcnn_hip_loss.h (frcnn_cnet_loss_rows).
//   cnet_loss_rows_kernel   one workgroup of 256 threads owns a tile of 64 rows.  Phase 1: the first wave, one thread a row,
//                           computes the row's terms in fp64 and stores the row's small outputs (crdelta as one 16-byte store);
//                           of the class gradient it leaves three words a row in LDS -- the target column, the value there and
//                           the value of every other column.  Phase 2: all four waves write the tile's ccdelta rows, which
//                           are 64 * ncls consecutive floats starting at a multiple of 16 bytes, with 16-byte stores; the
//                           last tile's tail of R * ncls mod 4 floats goes out as scalar stores.
// No atomics, no workspace, no sums: frcnn_loss_accumulate adds the rows' losses in its fixed order.  FMA contraction is off for
// this translation unit: every operation is rounded on its own, which is what makes the numpy restatement of the tests exact
// wherever no exp / expm1 / pow is involved, and a GIoU prediction equal to its target give an exactly zero gradient.
#pragma clang fp contract(off)
#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace frcnn {

#define CL_ROWS 64
#define CL_THREADS 256

struct ClDesc {
  int cls, box, bgclass, smooth;   // smooth: smoothing > 0
  double gamma, alpha, smoothing, beta, box_weight;
};

// GIoU of the prediction (x0, y0, x1, y1) against the target, with the gradient by the prediction's four edges.  In every
// min / max a tie selects the prediction's edge.
__device__ static inline double giou_terms(double x0, double y0, double x1, double y1, double tx0, double ty0, double tx1,
                                           double ty1, double g[4]) {
  const double pw = x1 - x0, ph = y1 - y0;
  const double Ap = pw * ph, At = (tx1 - tx0) * (ty1 - ty0);
  const bool six0 = x0 >= tx0, six1 = x1 <= tx1, siy0 = y0 >= ty0, siy1 = y1 <= ty1;
  const double iw = (six1 ? x1 : tx1) - (six0 ? x0 : tx0);
  const double ih = (siy1 ? y1 : ty1) - (siy0 ? y0 : ty0);
  const bool has = iw > 0.0 && ih > 0.0;
  const double I = has ? iw * ih : 0.0;
  const bool sex0 = x0 <= tx0, sex1 = x1 >= tx1, sey0 = y0 <= ty0, sey1 = y1 >= ty1;
  const double ew = (sex1 ? x1 : tx1) - (sex0 ? x0 : tx0);
  const double eh = (sey1 ? y1 : ty1) - (sey0 ? y0 : ty0);
  const double Cc = ew * eh;
  const double U = (Ap + At) - I;
  const double iou = I / U, fill = U / Cc;
  const double a = 1.0 / U, b = iou / U, c = 1.0 / Cc, d = fill / Cc;
  const double gI[4] = {has && six0 ? -ih : 0.0, has && siy0 ? -iw : 0.0, has && six1 ? ih : 0.0, has && siy1 ? iw : 0.0};
  const double gA[4] = {-ph, -pw, ph, pw};
  const double gC[4] = {sex0 ? -eh : 0.0, sey0 ? -ew : 0.0, sex1 ? eh : 0.0, sey1 ? ew : 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double gU = gA[k] - gI[k];
    g[k] = ((-(gI[k] * a) + gU * b) - gU * c) + gC[k] * d;
  }
  return (2.0 - iou) - fill;
}

__global__ __launch_bounds__(CL_THREADS) void cnet_loss_rows_kernel(
    float* __restrict__ crout, const float* __restrict__ crtarget, const float* __restrict__ ccout,
    const float* __restrict__ cctarget, const double* __restrict__ roi, int R, int npos, int ncls, ClDesc D,
    float* __restrict__ crdelta, float* __restrict__ ccdelta, double* __restrict__ row_loss, float* __restrict__ key,
    float* __restrict__ box5) {
  __shared__ int s_t[CL_ROWS];        // the row's target column, -1: none
  __shared__ float s_gt[CL_ROWS];     // ccdelta at the target column
  __shared__ float s_g0[CL_ROWS];     // ccdelta elsewhere in the row
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * CL_ROWS;                 // (the launch has cdiv(R, 64) workgroups: r0 < R)
  const int rows = min(R - r0, CL_ROWS);
  const bool train = crdelta != nullptr;
  if (tid < rows) {
    const int r = r0 + tid;
    const bool fg = r < npos;
    // ---- the class term
    const float tf = cctarget[r];
    const bool valid = tf >= 1.0f && tf <= (float)ncls;          // (a NaN fails both)
    const int t = valid ? (int)tf - 1 : -1;
    double cls = NAN;
    float gt = 0.0f, g0 = 0.0f;
    if (valid) {
      const float* row = ccout + (size_t)r * (size_t)ncls;
      const double w = D.alpha < 0.0 ? 1.0 : (t + 1 == D.bgclass ? 1.0 - D.alpha : D.alpha);
      const double lp = (double)row[t];
      if (D.cls == 1 && D.gamma > 0.0) {
        double q = -expm1(lp);
        if (!(q > 0.0)) q = 0.0;
        const double qg = pow(q, D.gamma);
        cls = -((w * qg) * lp);
        const double x = (q > 0.0 && lp > -INFINITY) ? ((D.gamma * pow(q, D.gamma - 1.0)) * (1.0 - q)) * lp : 0.0;
        gt = (float)((w * (-qg + x)) / (double)R);
      } else if (D.smooth) {
        const double u = D.smoothing / (double)ncls, ut = u + (1.0 - D.smoothing);
        double sum = 0.0;
        for (int j = 0; j < ncls; ++j) sum = sum + (j == t ? ut : u) * (double)row[j];
        cls = -(w * sum);
        gt = (float)(-(w * ut) / (double)R);
        g0 = (float)(-(w * u) / (double)R);
      } else {
        cls = -(w * lp);
        gt = (float)(-w / (double)R);
      }
    }
    s_t[tid] = t; s_gt[tid] = gt; s_g0[tid] = g0;
    // ---- the box term
    const float4 tg = *reinterpret_cast<const float4*>(crtarget + 4 * (size_t)r);
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (fg) y = *reinterpret_cast<const float4*>(crout + 4 * (size_t)r);
    else if (train) *reinterpret_cast<float4*>(crout + 4 * (size_t)r) = y;
    double box = 0.0;
    double gd[4] = {0.0, 0.0, 0.0, 0.0};
    if (D.box == 0) {
      const float z[4] = {y.x - tg.x, y.y - tg.y, y.z - tg.z, y.w - tg.w};
      double term[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double zd = (double)z[k], a = fabs(zd);
        const bool quad = a < D.beta;
        term[k] = quad ? ((0.5 * zd) * zd) / D.beta : a - 0.5 * D.beta;
        gd[k] = quad ? zd / D.beta : (zd > 0.0 ? 1.0 : -1.0);
      }
      box = ((term[0] + term[1]) + term[2]) + term[3];
    } else if (fg) {
      const double K = 0x1.08a691a12e2a9p+2;           // log(1000 / 16), the double next to it: 4.135166556742356
      const double c2 = (double)y.z, c3 = (double)y.w;
      const bool in2 = c2 <= K, in3 = c3 <= K;
      const double pw = exp(in2 ? c2 : K), ph = exp(in3 ? c3 : K);
      const double x0 = (double)y.x, y0 = (double)y.y, x1 = x0 + pw, y1 = y0 + ph;
      const double tx0 = (double)tg.x, ty0 = (double)tg.y, tx1 = tx0 + exp((double)tg.z), ty1 = ty0 + exp((double)tg.w);
      double g[4];
      box = giou_terms(x0, y0, x1, y1, tx0, ty0, tx1, ty1, g);
      gd[0] = g[0] + g[2];
      gd[1] = g[1] + g[3];
      gd[2] = in2 ? g[2] * pw : 0.0;
      gd[3] = in3 ? g[3] * ph : 0.0;
    }
    const double wbox = D.box_weight * box;
    if (train)
      *reinterpret_cast<float4*>(crdelta + 4 * (size_t)r) =
          make_float4((float)(D.box_weight * gd[0]), (float)(D.box_weight * gd[1]), (float)(D.box_weight * gd[2]),
                      (float)(D.box_weight * gd[3]));
    if (row_loss) { row_loss[2 * (size_t)r] = wbox; row_loss[2 * (size_t)r + 1] = cls / (double)R; }
    if (key || box5) {
      float kf = -INFINITY;                            // a target outside 1 ... ncls: never ahead of a valid row
      if (valid) {
        kf = (float)(cls + wbox);
        if (kf != kf) kf = INFINITY;                   // a diverged row is the hardest one, and the order stays total
      }
      if (key) key[r] = kf;
      if (box5) {
        const double2* q = reinterpret_cast<const double2*>(roi + 4 * (size_t)r);
        const double2 lo = q[0], hi = q[1];
        float* o = box5 + 5 * (size_t)r;
        o[0] = (float)lo.x; o[1] = (float)lo.y; o[2] = (float)hi.x; o[3] = (float)hi.y; o[4] = kf;
      }
    }
  }
  if (!train) return;                                  // (uniform: the whole workgroup leaves)
  __syncthreads();
  // ---- the tile's ccdelta rows: rows * ncls consecutive floats from element r0 * ncls, a multiple of 64
  const size_t base = (size_t)r0 * (size_t)ncls;
  const int words = rows * ncls;                       // <= 64 * ncls
  const int quads = words >> 2;
  float* out = ccdelta + base;
  for (int qd = tid; qd < quads; qd += CL_THREADS) {
    const int e = 4 * qd;
    int row = e / ncls, col = e - row * ncls;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = col == s_t[row] ? s_gt[row] : s_g0[row];
      if (++col == ncls) { col = 0; ++row; }           // (row may reach `rows` only behind the last element read)
    }
    *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
  }
  const int e = 4 * quads + tid;                       // the tail: at most 3 floats, in the last tile only
  if (e < words) {
    const int row = e / ncls, col = e - row * ncls;
    out[e] = col == s_t[row] ? s_gt[row] : s_g0[row];
  }
}

static bool misaligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) % 16) != 0;
}

int cnet_loss_rows(float* crout, const float* crtarget, const float* ccout, const float* cctarget, const double* roi, int R,
                   int npos, int ncls, const frcnn_cnet_loss_desc* desc, float* crdelta, float* ccdelta, double* row_loss,
                   float* key, float* box5, hipStream_t s) {
  // everything is checked before the launch: a refused call has written nothing
  FR_CHECK(R >= 0, "cnet_loss_rows: %d rows", R);
  FR_CHECK(npos >= 0 && npos <= R, "cnet_loss_rows: npos %d outside 0 ... %d", npos, R);
  FR_CHECK(ncls >= 1, "cnet_loss_rows: %d classes (at least 1)", ncls);
  FR_CHECK(desc, "cnet_loss_rows: NULL description");
  FR_CHECK(desc->cls == 0 || desc->cls == 1, "cnet_loss_rows: cls %d (0 nll, 1 focal)", desc->cls);
  FR_CHECK(desc->box == 0 || desc->box == 1, "cnet_loss_rows: box %d (0 smooth_l1, 1 giou)", desc->box);
  FR_CHECK(desc->gamma >= 0.0 && desc->gamma <= 5.0, "cnet_loss_rows: gamma %g outside 0 ... 5", desc->gamma);
  FR_CHECK(desc->alpha < 0.0 || (desc->alpha > 0.0 && desc->alpha < 1.0), "cnet_loss_rows: alpha %g (negative: none, or in (0, 1))",
           desc->alpha);
  FR_CHECK(!(desc->alpha > 0.0) || (desc->bgclass >= 1 && desc->bgclass <= ncls), "cnet_loss_rows: bgclass %d outside 1 ... %d",
           desc->bgclass, ncls);
  FR_CHECK(desc->smoothing >= 0.0 && desc->smoothing < 1.0, "cnet_loss_rows: smoothing %g outside [0, 1)", desc->smoothing);
  FR_CHECK(desc->cls == 0 || desc->smoothing == 0.0, "cnet_loss_rows: label smoothing is not defined under the focal loss");
  FR_CHECK(std::isfinite(desc->beta) && desc->beta > 0.0, "cnet_loss_rows: beta %g (finite, > 0)", desc->beta);
  FR_CHECK(std::isfinite(desc->box_weight) && desc->box_weight >= 0.0, "cnet_loss_rows: box_weight %g (finite, >= 0)",
           desc->box_weight);
  FR_CHECK((crdelta == nullptr) == (ccdelta == nullptr), "cnet_loss_rows: crdelta and ccdelta go together (both, or neither)");
  FR_CHECK(crdelta || row_loss || key || box5, "cnet_loss_rows: no output");
  FR_CHECK(!box5 || roi, "cnet_loss_rows: box5 needs roi");
  if (R == 0) return FRCNN_OK;
  FR_CHECK(crout && crtarget && ccout && cctarget, "cnet_loss_rows: NULL argument");
  FR_CHECK(!misaligned16(crout, crtarget, crdelta, ccdelta, roi),
           "cnet_loss_rows: crout, crtarget, crdelta, ccdelta and roi move 16 bytes at a time and must be 16-byte aligned");
  ClDesc D;
  D.cls = desc->cls; D.box = desc->box; D.bgclass = desc->bgclass; D.smooth = desc->cls == 0 && desc->smoothing > 0.0;
  D.gamma = desc->gamma; D.alpha = desc->alpha; D.smoothing = desc->smoothing; D.beta = desc->beta; D.box_weight = desc->box_weight;
  FR_LAUNCH(KC_ELEMWISE, 0, (double)R * ((crdelta ? 2.0 : 1.0) * ncls * 4.0 + 120.0), s, cnet_loss_rows_kernel,
            dim3(cdiv(R, CL_ROWS)), dim3(CL_THREADS), 0, crout, crtarget, ccout, cctarget, roi, R, npos, ncls, D, crdelta, ccdelta,
            row_loss, key, box5);
  FR_LAUNCH_CHECK();
  return FRCNN_OK;
}

}  // namespace frcnn
