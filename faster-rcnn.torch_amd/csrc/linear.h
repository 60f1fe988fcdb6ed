// linear.h -- one Linear layer's large products and the operand forms they run in.  The classification net (net.cpp) and the
// operator entry points frcnn_linear_forward / frcnn_linear_backward (api.cpp) both run THIS: there is no second copy of the rule.
// Included behind common.h, kernels.h and own.h: it uses their declarations and makes none itself (the host test
// tests/linear_host_check.cpp compiles it against logging stand-ins).
//
// A product runs in one of three forms:
//   fp32        gemm_f32 (gemm.hip), when linear_x_eligible says the role is not split at this shape;
//   three-plane the activation operand as three bf16 planes (split_planes, gemmx.hip);
//   fp16        two fp16 planes scaled by the operand's largest magnitude, with option x3_f16: the product takes the magnitude
//               records (amax.h) of both its operands.
// Launch order, which callers rely on (streams, split-K workspace slots, deferred folds):
//   forward on s:  [tensor_absmax(W -> REC_W)]  then  tensor_absmax(x -> REC_X), split_planes(x -> xp), linear_x_forward
//                  | split_planes, linear_x_forward | gemm_f32
//   dgrad on s:    tensor_absmax(g -> REC_G), split_planes(g -> gp), linear_x_dgrad | split_planes, linear_x_dgrad | gemm_f32;
//                  nothing at all when gx is null
//   wgrad on ws:   tensor_absmax(g -> REC_GT), [tensor_absmax(x -> REC_XT)], split_planes(g -> gpT), split_planes(x -> xpT),
//                  linear_x_wgrad | the two split_planes, linear_x_wgrad | gemm_f32(OUT_ADD);  then channel_sum_cols(g -> gb)
#pragma once
#include <cstdlib>

namespace frcnn {

// the large products in the two-plane fp16 form: with option x3_f16 (FRCNN_GEMM_F16=0: they stay three-plane)
inline bool gemm_f16_on() {
  static const bool env_on = [] { const char* e = getenv("FRCNN_GEMM_F16"); return e ? atoi(e) != 0 : true; }();
  return env_on && get_x3_f16();
}
// ... the weight gradient's too (FRCNN_GEMM_WGRAD_F16=0: it alone stays three-plane)
inline bool gemm_wgrad_f16_on() {
  static const bool env_on = [] { const char* e = getenv("FRCNN_GEMM_WGRAD_F16"); return e ? atoi(e) != 0 : true; }();
  return env_on && gemm_f16_on();
}

struct Linear {   // y[R][O] = x[R][I] * W[O][I]^T + b
  // magnitude records, AMAX_REC floats each.  The weight-gradient stream has two of its own: it forks before the chain takes REC_G,
  // and REC_X is only its to read when this step's forward pass took it.
  enum Rec { REC_X, REC_G, REC_W, REC_GT, REC_XT, REC_COUNT };
  int R = 0, I = 0, O = 0;    // the shape ensure() sized the planes for
  int x_form = 0;             // which products are split at this shape (bit 1 forward, 2 input gradient, 4 weight gradient: linear_x_eligible)
  DevBuf xp, gp;              // planes of the input and of the output gradient, row-major orientation (forward, input gradient)
  DevBuf xpT, gpT;            // ... in the transposed orientation (weight gradient)
  DevBuf am;                  // the records
  const float* am_w_of = nullptr;   // the weight matrix REC_W was taken from by the last forward pass (null: that pass took none) ...
  long am_w_gen = -1;               // ... in an evaluate-mode pass of this static_weights generation (-1: not reusable)

  float* rec(Rec r) const { return am.f() + (size_t)r * AMAX_REC; }

  // Decides the form of each role in `roles` and sizes the planes and records those roles need; other roles run fp32.
  int ensure(int R_, int I_, int O_, int roles) {
    R = R_; I = I_; O = O_;
    x_form = 0;
    for (int role : {1, 2, 4}) if ((roles & role) && linear_x_eligible(role, R, I, O)) x_form |= role;
    const size_t Rp = (size_t)linear_x_rows_padded(R);
    if (x_form & 1) FR_TRY(xp.ensure((size_t)3 * R * I * 2));
    if (x_form & 2) FR_TRY(gp.ensure((size_t)3 * R * O * 2));
    if (x_form & 4) { FR_TRY(xpT.ensure((size_t)3 * I * Rp * 2)); FR_TRY(gpT.ensure((size_t)3 * O * Rp * 2)); }
    if (x_form) FR_TRY(am.ensure((size_t)REC_COUNT * AMAX_REC * 4));
    return FRCNN_OK;
  }

  // fp16 form: the weight matrix's magnitude, which the forward and input-gradient products share.  static_gen >= 0: an
  // evaluate-mode pass under option static_weights in that generation -- the record of an earlier such pass from the same matrix
  // is kept.  When no product takes the fp16 form the matrix is forgotten: the input-gradient product must not scale by an
  // older step's record.
  int weight_record(const float* W, long static_gen, hipStream_t s) {
    if (!((x_form & 3) && gemm_f16_on())) { am_w_of = nullptr; return FRCNN_OK; }
    const bool have = static_gen >= 0 && am_w_gen == static_gen && am_w_of == W;
    if (!have) FR_TRY(tensor_absmax(W, (long)O * I, rec(REC_W), s));
    am_w_of = W; am_w_gen = static_gen;
    return FRCNN_OK;
  }

  int forward(const float* x, const float* W, const float* bias, float* y, long static_gen, hipStream_t s, int ws_slot, GemmFold* defer) {
    FR_TRY(weight_record(W, static_gen, s));
    if ((x_form & 1) && gemm_f16_on()) {
      FR_TRY(tensor_absmax(x, (long)R * I, rec(REC_X), s));
      FR_TRY(split_planes(x, R, I, xp.p, nullptr, s, rec(REC_X)));
      return linear_x_forward(xp.p, R, I, W, bias, O, y, s, ws_slot, defer, rec(REC_X), rec(REC_W));
    }
    if (x_form & 1) {
      FR_TRY(split_planes(x, R, I, xp.p, nullptr, s));
      return linear_x_forward(xp.p, R, I, W, bias, O, y, s, ws_slot, defer);
    }
    return gemm_f32(x, I, 1, W, 1, I, y, O, R, O, I, OUT_STORE, bias, s, ws_slot, defer);
  }

  // gx[R][I] = g[R][O] * W; a null gx queues nothing.  The fp16 form needs REC_W of THIS matrix: weight_record() (the forward
  // pass, or the caller in its place) comes first.
  int dgrad(const float* g, const float* W, float* gx, hipStream_t s, int ws_slot, GemmFold* defer) {
    if (!gx) return FRCNN_OK;
    if ((x_form & 2) && gemm_f16_on() && am_w_of == W) {
      FR_TRY(tensor_absmax(g, (long)R * O, rec(REC_G), s));
      FR_TRY(split_planes(g, R, O, gp.p, nullptr, s, rec(REC_G)));
      return linear_x_dgrad(gp.p, R, O, W, I, gx, OUT_STORE, s, ws_slot, defer, rec(REC_G), rec(REC_W));
    }
    if (x_form & 2) {
      FR_TRY(split_planes(g, R, O, gp.p, nullptr, s));
      return linear_x_dgrad(gp.p, R, O, W, I, gx, OUT_STORE, s, ws_slot, defer);
    }
    return gemm_f32(g, O, 1, W, I, 1, gx, I, R, I, O, OUT_STORE, nullptr, s, ws_slot, defer);
  }

  // gw[O][I] += g^T * x, then gb[o] += sum_r g[r][o]; either may be null.  W: the matrix of the forward pass, to tell whether
  // that pass left the input's record in REC_X.
  int wgrad(const float* g, const float* x, const float* W, float* gw, float* gb, hipStream_t ws, int wslot) {
    if (gw && (x_form & 4) && gemm_wgrad_f16_on()) {
      float *rg = rec(REC_GT), *rx = rec(REC_XT);
      FR_TRY(tensor_absmax(g, (long)R * O, rg, ws));
      if ((x_form & 1) && am_w_of == W) rx = rec(REC_X);
      else FR_TRY(tensor_absmax(x, (long)R * I, rx, ws));
      FR_TRY(split_planes(g, R, O, nullptr, gpT.p, ws, rg));
      FR_TRY(split_planes(x, R, I, nullptr, xpT.p, ws, rx));
      FR_TRY(linear_x_wgrad(gpT.p, xpT.p, R, O, I, gw, ws, wslot, rg, rx));
    } else if (gw && (x_form & 4)) {
      FR_TRY(split_planes(g, R, O, nullptr, gpT.p, ws));
      FR_TRY(split_planes(x, R, I, nullptr, xpT.p, ws));
      FR_TRY(linear_x_wgrad(gpT.p, xpT.p, R, O, I, gw, ws, wslot));
    } else if (gw) {
      FR_TRY(gemm_f32(g, 1, O, x, I, 1, gw, I, O, I, R, OUT_ADD, nullptr, ws, wslot));
    }
    if (gb) FR_TRY(channel_sum_cols(g, R, O, gb, ws));
    return FRCNN_OK;
  }
};

}  // namespace frcnn
