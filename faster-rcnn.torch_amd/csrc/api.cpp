// api.cpp -- C ABI plumbing of libfrcnn_hip.so (include/frcnn_hip.h): errors, device buffers,
// the HIP-event profiler, and the per-operator entry points that wrap the kernels.
#include <cmath>
#include <cstring>
#include <vector>
#include <mutex>

#include "kernels.h"
#include "own.h"
#include "linear.h"

namespace frcnn {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

// ---------------------------------------------------------------- profiler
struct ProfRec { int klass; double flops, bytes; hipEvent_t a, b; hipStream_t s; };
static hipEvent_t g_prof_base = nullptr;
static unsigned g_prof_mask = 0;
static std::vector<ProfRec> g_recs;
static std::vector<hipEvent_t> g_pool;
static hipEvent_t g_pending;
static std::mutex g_mu;

bool prof_enabled(int klass) { return (g_prof_mask >> klass) & 1u; }
static hipEvent_t get_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void prof_before(int, hipStream_t s) {
  g_pending = get_event();
  (void)hipEventRecord(g_pending, s);
}
void prof_after(int klass, double flops, double bytes, hipStream_t s) {
  ProfRec r;
  r.klass = klass; r.flops = flops; r.bytes = bytes; r.a = g_pending; r.b = get_event(); r.s = s;
  (void)hipEventRecord(r.b, s);
  g_recs.push_back(r);
}

}  // namespace frcnn

using namespace frcnn;

static_assert(frcnn::KC_COUNT == FRCNN_KC_COUNT && frcnn::KC_IMAGE == FRCNN_KC_IMAGE && frcnn::KC_OPTIM == FRCNN_KC_OPTIM &&
              frcnn::KC_CONV_IGEMM_K3 == FRCNN_KC_CONV_IGEMM_K3 && frcnn::KC_TOPK == FRCNN_KC_TOPK &&
              frcnn::KC_SOFT_NMS == FRCNN_KC_SOFT_NMS, "kernel classes of common.h and frcnn_hip.h differ");

extern "C" {

int frcnn_version(void) { return 100; }
const char* frcnn_last_error(void) { return g_err.c_str(); }

int frcnn_device_count(int* n) {
  FR_HIP(hipGetDeviceCount(n));
  return FRCNN_OK;
}
int frcnn_set_device(int device) {
  FR_HIP(hipSetDevice(device));
  return FRCNN_OK;
}
int frcnn_device_name(char* buf, int len) {
  int dev;
  FR_HIP(hipGetDevice(&dev));
  hipDeviceProp_t p;
  FR_HIP(hipGetDeviceProperties(&p, dev));
  snprintf(buf, len, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
  return FRCNN_OK;
}

int frcnn_malloc(void** ptr, size_t bytes) {
  FR_HIP(hipMalloc(ptr, (bytes ? bytes : 16) + 64));   // (64 bytes of slack, as the model's own buffers: see conv_wgradx's loaders)
  return FRCNN_OK;
}
int frcnn_free(void* ptr) {
  FR_HIP(hipFree(ptr));
  return FRCNN_OK;
}
int frcnn_host_alloc(void** ptr, size_t bytes) {
  FR_CHECK(ptr, "frcnn_host_alloc: NULL result pointer");
  FR_HIP(hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault));
  return FRCNN_OK;
}
int frcnn_host_free(void* ptr) {
  FR_HIP(hipHostFree(ptr));
  return FRCNN_OK;
}
int frcnn_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  FR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)));
  return FRCNN_OK;
}
int frcnn_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  FR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
  return FRCNN_OK;
}
int frcnn_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  FR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(stream)));
  return FRCNN_OK;
}
int frcnn_stream_sync(void* stream) {
  FR_HIP(hipStreamSynchronize(S(stream)));
  return FRCNN_OK;
}
int frcnn_zero(void* ptr, size_t bytes, void* stream) { return fill_zero(ptr, bytes, S(stream)); }
int frcnn_scale(float* x, long long n, float s, void* stream) { return scale_inplace(x, n, s, S(stream)); }
int frcnn_add(float* y, const float* x, long long n, void* stream) {
  FR_CHECK(y && x && n >= 0, "frcnn_add: bad arguments");
  return n ? add_inplace(y, x, n, S(stream)) : FRCNN_OK;
}

int frcnn_prof_enable(int class_mask) {
  if (class_mask && !g_prof_mask && getenv("FRCNN_PROF_DUMP")) {   // debug: time base for the per-launch start offsets
    if (!g_prof_base) FR_HIP(hipEventCreate(&g_prof_base));
    FR_HIP(hipDeviceSynchronize());
    FR_HIP(hipEventRecord(g_prof_base, nullptr));
  }
  g_prof_mask = (unsigned)class_mask;
  return FRCNN_OK;
}
int frcnn_prof_collect(long long* launches, double* ms, double* flops, double* bytes) {
  FR_HIP(hipDeviceSynchronize());
  for (int k = 0; k < KC_COUNT; ++k) { launches[k] = 0; ms[k] = 0; flops[k] = 0; bytes[k] = 0; }
  FILE* dump = (getenv("FRCNN_PROF_DUMP") && g_prof_base) ? fopen(getenv("FRCNN_PROF_DUMP"), "a") : nullptr;
  for (auto& r : g_recs) {
    float t = 0.f;
    FR_HIP(hipEventElapsedTime(&t, r.a, r.b));
    if (dump) {   // debug timeline: class, stream, start offset (us) from frcnn_prof_enable, duration (us)
      float t0 = 0.f;
      if (hipEventElapsedTime(&t0, g_prof_base, r.a) == hipSuccess)
        fprintf(dump, "%d %p %.1f %.1f\n", r.klass, (void*)r.s, t0 * 1e3, t * 1e3);
    }
    launches[r.klass] += 1; ms[r.klass] += t; flops[r.klass] += r.flops; bytes[r.klass] += r.bytes;
    g_pool.push_back(r.a);
    g_pool.push_back(r.b);
  }
  if (dump) { fprintf(dump, "-1 0 0 0\n"); fclose(dump); }
  g_recs.clear();
  return FRCNN_OK;
}

// ---------------------------------------------------------------- nms
size_t frcnn_nms_workspace_bytes(int n) { return nms_workspace_bytes(n); }
int frcnn_nms_device(const float* boxes, int n, int ncols, float overlap, int key_mode, int key_col,
                     long long* pick, int* count, void* ws, size_t ws_bytes, void* stream) {
  return nms_device(boxes, n, ncols, overlap, key_mode, key_col, pick, count, ws, ws_bytes, S(stream));
}
int frcnn_nms_device_classes(const float* boxes, int n, int ncols, float overlap, int key_mode, int key_col, const int* cls,
                             long long* pick, int* count, void* ws, size_t ws_bytes, void* stream) {
  return nms_device(boxes, n, ncols, overlap, key_mode, key_col, pick, count, ws, ws_bytes, S(stream), cls);
}
int frcnn_nms_device_n(const float* boxes, int n_cap, const int* n_dev, int ncols, float overlap, int key_mode, int key_col,
                       const int* cls, long long* pick, int* count, void* ws, size_t ws_bytes, void* stream) {
  FR_CHECK(n_dev, "frcnn_nms_device_n: NULL device count");
  return nms_device(boxes, n_cap, ncols, overlap, key_mode, key_col, pick, count, ws, ws_bytes, S(stream), cls, n_dev);
}
size_t frcnn_nms_batch_workspace_bytes(int B, int n_cap) { return nms_batch_workspace_bytes(B, n_cap); }
int frcnn_nms_device_batch(const float* boxes, int B, long long row_stride, int n_cap, const int* n_dev, int ncols, float overlap,
                           int key_mode, int key_col, const int* cls, long long* pick, int* count, void* ws, size_t ws_bytes,
                           void* stream) {
  FR_CHECK(B <= 0 || (boxes && pick && count), "frcnn_nms_device_batch: NULL argument");
  FR_CHECK(B <= 0 || n_cap <= 0 || n_dev, "frcnn_nms_device_batch: NULL device counts");
  return nms_device_batch(boxes, B, (long)row_stride, n_cap, n_dev, ncols, overlap, key_mode, key_col, cls, pick, count, ws,
                          ws_bytes, S(stream));
}
size_t frcnn_soft_nms_workspace_bytes(int B, int n_cap) { return soft_nms_workspace_bytes(B, n_cap); }
int frcnn_soft_nms_batch(const float* boxes, int B, long long row_stride, int n_cap, const int* n_dev, int ncols, int score_col,
                         int method, float overlap, float sigma, float min_score, int log_domain, const int* cls, long long* pick,
                         int* count, float* score_out, long long score_stride, void* ws, size_t ws_bytes, void* stream) {
  return soft_nms_batch(boxes, B, (long)row_stride, n_cap, n_dev, ncols, score_col, method, overlap, sigma, min_score, log_domain,
                        cls, pick, count, score_out, (long)score_stride, ws, ws_bytes, S(stream));
}
int frcnn_box_vote_batch(const float* boxes, int B, long long row_stride, int n_cap, const int* n_dev, int ncols, int score_col,
                         int weight_mode, float overlap, const int* cls, const double* rect, const long long* pick,
                         const int* count, double* rect_out, int* votes_out, void* stream) {
  return box_vote_batch(boxes, B, (long)row_stride, n_cap, n_dev, ncols, score_col, weight_mode, overlap, cls, rect, pick, count,
                        rect_out, votes_out, S(stream));
}
size_t frcnn_topk_select_workspace_bytes(int B, int n_cap) { return topk_select_workspace_bytes(B, n_cap); }
int frcnn_topk_select(const float* score, int B, long long stride, int n_cap, const int* n_dev, int K, int* sel_row,
                      long long sel_stride, int* k_dev, void* ws, size_t ws_bytes, void* stream) {
  return topk_select(score, B, (long)stride, n_cap, n_dev, K, sel_row, (long)sel_stride, k_dev, ws, ws_bytes, S(stream));
}
int frcnn_rpn_gather_rows(const float* match_p, const int* match_idx, const double* match_rect, const float* match_box, int B,
                          long long src_stride, int src_rows, const int* sel_row, long long sel_stride, const int* k_dev, int k_cap,
                          float* dst_p, int* dst_idx, double* dst_rect, float* dst_box, float* box5, int* row,
                          long long dst_stride, void* stream) {
  return rpn_gather_rows(match_p, match_idx, match_rect, match_box, B, (long)src_stride, src_rows, sel_row, (long)sel_stride,
                         k_dev, k_cap, dst_p, dst_idx, dst_rect, dst_box, box5, row, (long)dst_stride, S(stream));
}
int frcnn_proposal_targets_batch(const double* rect, const long long* pick, long long match_stride, const int* r_dev, int r_cap,
                                 const double* gt_rect, const int* gt_class, int gt_stride, const int* G_host, int B,
                                 int include_gt, double fg_iou, double bg_lo, double bg_hi, int fg_quota, int batch, int bgclass,
                                 unsigned int seed, double* roi, float* crtarget, float* cctarget, int* src, int* gt_idx,
                                 double* iou, int out_stride, int* counts, void* stream) {
  return proposal_targets_batch(rect, pick, match_stride, r_dev, r_cap, gt_rect, gt_class, gt_stride, G_host, B, include_gt, fg_iou,
                                bg_lo, bg_hi, fg_quota, batch, bgclass, seed, roi, crtarget, cctarget, src, gt_idx, iou, out_stride,
                                counts, S(stream));
}
int frcnn_roi_hard_keys_batch(const double* roi, const float* crout, const float* crtarget, const float* ccout,
                              const float* cctarget, int B, long long row_stride, int n_cap, const int* n_dev, const int* nfg_dev,
                              int ncls, float* box5, float* loss, void* stream) {
  return roi_hard_keys_batch(roi, crout, crtarget, ccout, cctarget, B, row_stride, n_cap, n_dev, nfg_dev, ncls, box5, loss,
                             S(stream));
}
int frcnn_roi_hard_gather_batch(const long long* pick, const int* count_dev, int batch, const double* roi, const float* crtarget,
                                const float* cctarget, const int* src, const int* gt_idx, const double* iou, const float* loss,
                                int B, long long row_stride, int n_cap, const int* n_dev, const int* nfg_dev, double* roi_out,
                                float* crtarget_out, float* cctarget_out, int* src_out, int* gt_idx_out, double* iou_out,
                                float* loss_out, int out_stride, int* counts, void* stream) {
  return roi_hard_gather_batch(pick, count_dev, batch, roi, crtarget, cctarget, src, gt_idx, iou, loss, B, row_stride, n_cap, n_dev,
                               nfg_dev, roi_out, crtarget_out, cctarget_out, src_out, gt_idx_out, iou_out, loss_out, out_stride,
                               counts, S(stream));
}
int frcnn_cnet_loss_rows(float* crout, const float* crtarget, const float* ccout, const float* cctarget, const double* roi, int R,
                         int npos, int ncls, const frcnn_cnet_loss_desc* desc_host, float* crdelta, float* ccdelta,
                         double* row_loss, float* key, float* box5, void* stream) {
  return cnet_loss_rows(crout, crtarget, ccout, cctarget, roi, R, npos, ncls, desc_host, crdelta, ccdelta, row_loss, key, box5,
                        S(stream));
}
int frcnn_box_head_forward(const float* x, int R, int nf, const float* W, const float* b, int C, const void* classes, int kind, int n,
                           const float* lsm, int ncls, float* out, int* sel, void* stream) {
  return box_head_forward(x, R, nf, W, b, C, classes, kind, n, lsm, ncls, out, sel, S(stream));
}
int frcnn_box_head_backward(const float* g, const float* x, const int* sel, int R, int nf, const float* W, int C, float* gfeat,
                            float* gW, float* gb, void* stream) {
  return box_head_backward(g, x, sel, R, nf, W, C, gfeat, gW, gb, S(stream), S(stream));
}
int frcnn_detect_class_boxes_batch(const float* feat, int nf, const long long* row0_host, int B, const float* W, const float* b, int C,
                                   const double* rect, const long long* pick, long long match_stride, const int* kc,
                                   const int* keep_row, const int* K_dev, int row_stride, float* bb, double* r2, void* stream) {
  return detect_class_boxes_batch(feat, nf, row0_host, B, W, b, C, rect, pick, match_stride, kc, keep_row, K_dev, row_stride, bb, r2,
                                  S(stream));
}
int frcnn_eval_match_batch(const double* rec, int B, int row_stride, const int* sel_row, long long sel_stride, const int* k_dev,
                           const double* gt_rect, const int* gt_class, const long long* gt_row0_host, const double* thr_host, int T,
                           int* match, double* iou, void* stream) {
  return eval_match_batch(rec, B, row_stride, sel_row, sel_stride, k_dev, gt_rect, gt_class, gt_row0_host, thr_host, T, match, iou,
                          S(stream));
}
int frcnn_eval_conf_rows(const double* rec, int B, int row_stride, float* conf, int* count, void* stream) {
  return eval_conf_rows(rec, B, row_stride, conf, count, S(stream));
}
int frcnn_detect_gather_batch(const long long* wpick, const int* counts, int B, int row_stride, const int* keep_row, const int* kc,
                              const float* bb, const double* r2, const long long* pick, long long match_stride,
                              const float* match_p, const double* match_rect, const int* match_idx, double* rec, void* stream) {
  FR_CHECK(B <= 0 || (counts && rec), "frcnn_detect_gather_batch: NULL argument");
  return detect_gather_batch(wpick, counts, B, row_stride, keep_row, kc, bb, r2, pick, (long)match_stride, match_p, match_rect,
                             match_idx, rec, S(stream));
}
int frcnn_roi_windows(const double* rect, const long long* pick, int k, const int* layers_host, int nlayers, int fmH, int fmW,
                      int* wins, void* stream) {
  FR_CHECK(rect && wins && (layers_host || nlayers == 0), "frcnn_roi_windows: NULL argument");
  return roi_windows(rect, pick, k, layers_host, nlayers, fmH, fmW, wins, S(stream));
}
int frcnn_detect_post(const int* cls, const float* conf, const float* bbox, const double* rect, const long long* pick, int R,
                      int bgclass, double min_conf, float* bb, int* kc, int* keep_row, double* r2, int* K_dev, void* stream) {
  return detect_post(cls, conf, bbox, rect, pick, R, bgclass, min_conf, bb, kc, keep_row, r2, K_dev, S(stream));
}
int frcnn_detect_classes_batch(const float* cls_out, const float* bbox, const int* R_host, const long long* row0_host, int B,
                               const double* rect, const long long* pick, long long match_stride, int ncls, int bgclass,
                               double min_conf, int mode, float* bb, int* kc, int* keep_row, double* r2, int row_stride, int* K_dev,
                               int* total_dev, void* stream) {
  return detect_classes_batch(cls_out, bbox, R_host, row0_host, B, rect, pick, match_stride, ncls, bgclass, min_conf, mode, bb, kc,
                              keep_row, r2, row_stride, K_dev, total_dev, S(stream));
}
int frcnn_detect_merge_views(const float* bb, const int* kc, const int* keep_row, const double* r2, long long row_stride,
                             const int* counts, const long long* pick, long long match_stride, int F, int V,
                             const int* flip_host, const double* wv_host, const double* ax_host, const double* ay_host,
                             const int* R_host, float* bb_out, int* kc_out, int* keep_row_out, double* r2_out,
                             long long* pick_out, int* counts_out, void* stream) {
  return detect_merge_views(bb, kc, keep_row, r2, row_stride, counts, pick, match_stride, F, V, flip_host, wv_host, ax_host,
                            ay_host, R_host, bb_out, kc_out, keep_row_out, r2_out, pick_out, counts_out, S(stream));
}
int frcnn_nms_host(const float* boxes_host, int n, int ncols, float overlap, int key_mode, int key_col,
                   long long* pick_host, int* count_host) {
  if (n <= 0) { *count_host = 0; return FRCNN_OK; }
  size_t wsb = nms_workspace_bytes(n);
  char* buf = nullptr;
  size_t bb = ((size_t)n * ncols * 4 + 255) / 256 * 256, pb = ((size_t)n * 8 + 255) / 256 * 256;
  FR_HIP(hipMalloc((void**)&buf, bb + pb + 256 + wsb));
  float* dboxes = (float*)buf;
  long long* dpick = (long long*)(buf + bb);
  int* dcount = (int*)(buf + bb + pb);
  void* ws = buf + bb + pb + 256;
  int rc = FRCNN_OK;
  hipError_t e = hipMemcpy(dboxes, boxes_host, (size_t)n * ncols * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) rc = nms_device(dboxes, n, ncols, overlap, key_mode, key_col, dpick, dcount, ws, wsb, 0);
  if (e == hipSuccess && rc == FRCNN_OK) e = hipMemcpy(count_host, dcount, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && rc == FRCNN_OK && *count_host > 0)
    e = hipMemcpy(pick_host, dpick, (size_t)*count_host * 8, hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  if (e != hipSuccess) { set_error("frcnn_nms_host: %s", hipGetErrorString(e)); return FRCNN_ERR_HIP; }
  return rc;
}

// ---------------------------------------------------------------- conv (operator-level, for parity tests
// and hosts that drive single layers; the model runtime keeps packed weights resident instead)
// option x3_f16: the op-level split launches take the two-plane fp16 form; the magnitude records of their two operands (amax.h) and
// the scalar the pack publishes live in a buffer of the CALL (freed with it: two host threads or streams may run these entry points
// side by side)
#define X3_REC_BYTES ((size_t)(2 * AMAX_REC + 4) * 4)
static int x3_f16_records(float** out) {
  *out = nullptr;
  if (!get_x3_f16()) return FRCNN_OK;
  FR_HIP(hipMalloc((void**)out, X3_REC_BYTES));
  return FRCNN_OK;
}

// The two-plane fp16 form leaves ONE binade of headroom for a per-channel input scale (convx.hip: a dropout scale's entries are
// <= 1).  The operator-level entry points accept any caller-supplied scale: entries beyond 1 take the three-plane bf16 form,
// which has fp32's exponent range.  A host read -- these entry points synchronise anyway.
static int scale_fits_f16_form(const float* in_scale, int C, hipStream_t s, bool* ok) {
  *ok = true;
  if (!in_scale) return FRCNN_OK;
  std::vector<float> h((size_t)C);
  FR_HIP(hipMemcpyAsync(h.data(), in_scale, (size_t)C * 4, hipMemcpyDeviceToHost, s));
  FR_HIP(hipStreamSynchronize(s));
  for (float v : h) if (!(std::fabs(v) <= 1.f)) { *ok = false; break; }
  return FRCNN_OK;
}

// The split-operand form of the two entry points below.  f16: the two-plane fp16 form (records: rec_in = the caller's record of
// the launch's input tensor or null = taken here; rec_out = conv_x3's amax_out), else three bf16 planes.
static int conv2d_split(const float* in, int Kc, int H, int W, const float* in_slope, const float* in_scale, const float* weight,
                        const float* bias, int O, int C, int M, int k, int mode, int pad, float* out, int out_mode, bool f16,
                        const float* rec_in, float* rec_out, const X3PostAct* post, hipStream_t s) {
  float* wp = nullptr;
  FR_HIP(hipMalloc((void**)&wp, conv_x3_pack_bytes(Kc, M, k)));
  float* am = nullptr;
  int rcx = f16 ? x3_f16_records(&am) : FRCNN_OK;
  float* const amw = am ? am + AMAX_REC : nullptr;          // the weights' record
  float* const aws = am ? am + 2 * AMAX_REC : nullptr;      // their largest magnitude
  if (am && rcx == FRCNN_OK) {
    if (!rec_in) rcx = tensor_absmax(in, (long)Kc * H * W, am, s);
    if (rcx == FRCNN_OK) rcx = tensor_absmax(weight, (long)O * C * k * k, amw, s);
  }
  if (rcx == FRCNN_OK) rcx = conv_x3_pack(weight, O, C, k, mode, wp, s, H + 2 * pad - k + 1, W + 2 * pad - k + 1, amw, aws);
  if (rcx == FRCNN_OK)
    rcx = conv_x3(in, Kc, H, W, in_slope, in_scale, wp, bias, M, k, pad, out, out_mode, 0, s, 0, post, am ? (rec_in ? rec_in : am) : nullptr,
                  aws, rec_out);
  (void)hipStreamSynchronize(s);
  (void)hipFree(wp); (void)hipFree(am);
  return rcx;
}

int frcnn_conv2d_forward(const float* in, int C, int H, int W, const float* in_slope, const float* in_scale,
                         const float* weight, const float* bias, int O, int k, int pad, float* out,
                         void* stream) {
  float* wf = nullptr;
  if (conv_x3_eligible(C, O, k) && (k == 3 || (!in_slope && !in_scale))) {   // split-bf16 operand form (convx.hip)
    bool unit = true;
    FR_TRY(scale_fits_f16_form(in_scale, C, S(stream), &unit));
    return conv2d_split(in, C, H, W, in_slope, in_scale, weight, bias, O, C, O, k, 0, pad, out, OUT_STORE, unit, nullptr, nullptr, nullptr,
                        S(stream));
  }
  FR_HIP(hipMalloc((void**)&wf, conv_pack_floats(C, O, k) * 4));
  int rc = conv_pack_weights(weight, O, C, k, wf, nullptr, S(stream));
  if (rc == FRCNN_OK) rc = conv_igemm(in, C, H, W, in_slope, in_scale, wf, bias, O, k, pad, out, OUT_STORE, 0, S(stream));
  (void)hipStreamSynchronize(S(stream));
  (void)hipFree(wf);
  return rc;
}
int frcnn_conv2d_backward_input(const float* gout, int O, int Ho, int Wo, const float* weight, int C, int k,
                                int pad, float* gin, int accumulate, void* stream) {
  float* wd = nullptr;
  if (conv_x3_eligible(O, C, k))
    return conv2d_split(gout, O, Ho, Wo, nullptr, nullptr, weight, nullptr, O, C, C, k, 1, k - 1 - pad, gin, accumulate ? OUT_ADD : OUT_STORE,
                        true, nullptr, nullptr, nullptr, S(stream));
  FR_HIP(hipMalloc((void**)&wd, conv_pack_floats(O, C, k) * 4));
  int rc = conv_pack_weights(weight, O, C, k, nullptr, wd, S(stream));
  if (rc == FRCNN_OK)
    rc = conv_igemm(gout, O, Ho, Wo, nullptr, nullptr, wd, nullptr, C, k, k - 1 - pad, gin,
                    accumulate ? OUT_ADD : OUT_STORE, 0, S(stream));
  (void)hipStreamSynchronize(S(stream));
  (void)hipFree(wd);
  return rc;
}
// ---- the same two in the fp16 form only, with the records in the caller's hands (include/frcnn_hip.h "magnitude records")
int frcnn_amax_record_floats(void) { return AMAX_REC; }
int frcnn_tensor_absmax(const float* x, long long n, float* rec, void* stream) {
  FR_CHECK(x && rec && n >= 1, "frcnn_tensor_absmax: bad arguments");
  return tensor_absmax(x, (long)n, rec, S(stream));
}
int frcnn_conv2d_forward_rec(const float* in, int C, int H, int W, const float* in_slope, const float* in_scale, const float* weight,
                             const float* bias, int O, int k, int pad, float* out, const float* rec_in, float* rec_out, void* stream) {
  FR_CHECK(in && weight && out, "frcnn_conv2d_forward_rec: NULL argument");
  FR_CHECK(conv_x3_eligible(C, O, k) && (k == 3 || (!in_slope && !in_scale)),
           "frcnn_conv2d_forward_rec: %d channels -> %d filters, %dx%d does not take the split form", C, O, k, k);
  FR_CHECK(get_x3_f16(), "frcnn_conv2d_forward_rec: option x3_f16 is off");
  bool unit = true;
  FR_TRY(scale_fits_f16_form(in_scale, C, S(stream), &unit));
  FR_CHECK(unit, "frcnn_conv2d_forward_rec: an entry of in_scale exceeds 1: the launch would not take the fp16 form");
  return conv2d_split(in, C, H, W, in_slope, in_scale, weight, bias, O, C, O, k, 0, pad, out, OUT_STORE, true, rec_in, rec_out, nullptr,
                      S(stream));
}
int frcnn_conv2d_backward_input_rec(const float* gout, int O, int Ho, int Wo, const float* weight, int C, int k, int pad, float* gin,
                                    int accumulate, const float* rec_g, float* rec_out, const float* post_x, const float* post_slope,
                                    const float* post_scale, float* gslope, void* stream) {
  FR_CHECK(gout && weight && gin, "frcnn_conv2d_backward_input_rec: NULL argument");
  FR_CHECK(conv_x3_eligible(O, C, k), "frcnn_conv2d_backward_input_rec: %d filters -> %d channels, %dx%d does not take the split form",
           O, C, k, k);
  FR_CHECK(get_x3_f16(), "frcnn_conv2d_backward_input_rec: option x3_f16 is off");
  FR_CHECK(post_x || (!post_slope && !post_scale && !gslope), "frcnn_conv2d_backward_input_rec: a fused activation backward needs post_x");
  FR_CHECK(!post_x || (post_slope && k == 3 && !accumulate),
           "frcnn_conv2d_backward_input_rec: the fused activation backward belongs to a storing 3x3 launch with a slope");
  const X3PostAct post{post_x, post_slope, post_scale, gslope};
  return conv2d_split(gout, O, Ho, Wo, nullptr, nullptr, weight, nullptr, O, C, C, k, 1, k - 1 - pad, gin, accumulate ? OUT_ADD : OUT_STORE,
                      true, rec_g, rec_out, post_x ? &post : nullptr, S(stream));
}
int frcnn_conv2d_backward_weight(const float* in, int C, int H, int W, const float* in_slope,
                                 const float* in_scale, const float* gout, int O, int k, int pad,
                                 float* gweight, float* gbias, void* stream) {
  size_t wsb = conv_wgrad_workspace_bytes(C, H, W, O, k, pad);
  void* ws = nullptr;
  FR_HIP(hipMalloc(&ws, wsb));
  int rc = FRCNN_OK;
  float* am = nullptr;   // (fp16 form: records of both tensors)
  bool unit = true;
  rc = scale_fits_f16_form(in_scale, C, S(stream), &unit);
  if (rc == FRCNN_OK && unit && k == 3 && conv_wgradx_eligible(C, O, k)) rc = x3_f16_records(&am);
  if (am && rc == FRCNN_OK) {
    rc = tensor_absmax(in, (long)C * H * W, am, S(stream));
    if (rc == FRCNN_OK) rc = tensor_absmax(gout, (long)O * (H + 2 * pad - k + 1) * (W + 2 * pad - k + 1), am + AMAX_REC, S(stream));
  }
  if (rc == FRCNN_OK)   // gbias: the split form sums it from the staged gradient tiles, the fp32 kernels in a pass of their own (conv_wgrad)
    rc = conv_wgrad(in, C, H, W, in_slope, in_scale, gout, O, k, pad, gweight, ws, wsb, S(stream), gbias, am, am ? am + AMAX_REC : nullptr);
  (void)hipStreamSynchronize(S(stream));
  (void)hipFree(ws); (void)hipFree(am);
  return rc;
}

int frcnn_maxpool_act_forward(const float* x, int C, int H, int W, const float* slope, const float* scale,
                              float* out, unsigned char* idx, void* stream) {
  return maxpool_act_forward(x, C, H, W, slope, scale, out, idx, S(stream));
}
int frcnn_maxpool_act_backward(const float* gpool, const unsigned char* idx, const float* x, int C, int H, int W,
                               const float* slope, const float* scale, float* gx, float* gbias, float* gslope,
                               void* stream) {
  return maxpool_act_backward(gpool, idx, x, C, H, W, slope, scale, gx, gbias, gslope, S(stream));
}
int frcnn_maxpool_act_forward_rec(const float* x, int C, int H, int W, const float* slope, const float* scale, float* out,
                                  unsigned char* idx, void* stream, float* rec) {
  return maxpool_act_forward(x, C, H, W, slope, scale, out, idx, S(stream), rec);
}
int frcnn_maxpool_act_backward_rec(const float* gpool, const unsigned char* idx, const float* x, int C, int H, int W, const float* slope,
                                   const float* scale, float* gx, float* gbias, float* gslope, void* stream, float* rec) {
  return maxpool_act_backward(gpool, idx, x, C, H, W, slope, scale, gx, gbias, gslope, S(stream), rec);
}
int frcnn_act_backward_rec(const float* gy, const float* x, int C, long long hw, const float* slope, const float* scale, float* gx,
                           float* gbias, float* gslope, void* stream, float* rec) {
  return act_backward(gy, x, C, hw, slope, scale, gx, gbias, gslope, S(stream), rec);
}
int frcnn_act_forward(const float* x, int C, long long hw, const float* slope, const float* scale, float* y,
                      void* stream) {
  return act_forward(x, C, hw, slope, scale, y, S(stream));
}
int frcnn_act_backward(const float* gy, const float* x, int C, long long hw, const float* slope,
                       const float* scale, float* gx, float* gbias, float* gslope, void* stream) {
  return act_backward(gy, x, C, hw, slope, scale, gx, gbias, gslope, S(stream));
}
// ---- test entry points: the two fused launches of the backbone's training step (net.cpp) that nothing else reaches
int frcnn_conv2d_forward_pool(const float* in, int C, int H, int W, const float* in_slope, const float* in_scale, const float* weight,
                              const float* bias, int O, int pad, const float* pool_slope, const float* pool_scale, float* out,
                              float* pooled, unsigned char* pidx, float* rec, int* fused_out, void* stream) {
  FR_CHECK(in && weight && out && pooled && pidx, "frcnn_conv2d_forward_pool: NULL argument");
  if (fused_out) *fused_out = 0;
  float* wf = nullptr;
  FR_HIP(hipMalloc((void**)&wf, conv_pack_floats(C, O, 3) * 4));
  // the model's call for a block's last convolution without the split form, and its fallback when the launch left the pool out
  IgemmPool pl = {pooled, pidx, pool_slope, pool_scale, rec};
  bool fused = false;
  int rc = conv_pack_weights(weight, O, C, 3, wf, nullptr, S(stream));
  if (rc == FRCNN_OK) rc = conv_igemm(in, C, H, W, in_slope, in_scale, wf, bias, O, 3, pad, out, OUT_STORE, 0, S(stream), 0, &pl, &fused);
  if (rc == FRCNN_OK && !fused)
    rc = maxpool_act_forward(out, O, H + 2 * pad - 2, W + 2 * pad - 2, pool_slope, pool_scale, pooled, pidx, S(stream), rec);
  (void)hipStreamSynchronize(S(stream));
  (void)hipFree(wf);
  if (fused_out) *fused_out = fused ? 1 : 0;
  return rc;
}
int frcnn_conv2d_backward_weight_pooled(const float* in, int C, int H, int W, const float* gpool, const unsigned char* pidx,
                                        const float* x, const float* slope, int O, int pad, float* gweight, float* gbias,
                                        float* gslope, void* stream) {
  FR_CHECK(in && gpool && pidx && x && gweight && gbias && gslope, "frcnn_conv2d_backward_weight_pooled: NULL argument");
  FR_CHECK(C >= 1 && O >= 1 && H + 2 * pad - 2 >= 1 && W + 2 * pad - 2 >= 1, "frcnn_conv2d_backward_weight_pooled: empty shape");
  const size_t wsb = conv_wgrad_workspace_bytes(C, H, W, O, 3, pad);   // what the model allocates for its first convolution
  void* ws = nullptr;
  FR_HIP(hipMalloc(&ws, wsb));
  int rc = conv_wgrad_first_pooled(in, C, H, W, gpool, pidx, x, slope, O, pad, gweight, gbias, gslope, ws, wsb, S(stream));
  (void)hipStreamSynchronize(S(stream));
  (void)hipFree(ws);
  return rc;
}

// ---- test entry points (include/frcnn_hip_heads.h): the anchor nets' sparse chain, its grouped product and the per-net helpers
int frcnn_gemm_group(const frcnn_gemm_job* jobs, int n, void* stream) {
  FR_CHECK(jobs && n >= 1 && n <= GEMM_GROUP_MAX, "frcnn_gemm_group: %d jobs", n);
  GemmJob q[GEMM_GROUP_MAX];
  for (int i = 0; i < n; ++i) {
    const frcnn_gemm_job& j = jobs[i];
    FR_CHECK(j.K >= 1 && j.M >= 0 && j.N >= 0 && j.splits >= 1, "frcnn_gemm_group: job %d is %d x %d x %d in %d splits", i, j.M, j.N,
             j.K, j.splits);
    FR_CHECK(j.out_mode == OUT_STORE || j.out_mode == OUT_ADD, "frcnn_gemm_group: job %d: out_mode %d", i, j.out_mode);
    const bool blocks = j.M > 0 && j.N > 0;
    FR_CHECK(!blocks || (j.A && j.B && j.C), "frcnn_gemm_group: job %d: NULL operand", i);
    FR_CHECK(!blocks || j.splits > 1 || j.ldc >= j.N, "frcnn_gemm_group: job %d: ldc %lld below N = %d", i, j.ldc, j.N);
    // (a job without blocks takes no part in the launch: its split count is not held against its K)
    q[i] = GemmJob{j.A, (long)j.sAm, (long)j.sAk, j.B, (long)j.sBk, (long)j.sBn, j.C, (long)j.ldc, j.M, j.N, j.K, j.out_mode,
                   blocks ? j.splits : 1};
  }
  return gemm_f32_group(q, n, S(stream));
}

static int heads_table(const char* who, const frcnn_head_net* nets, int n, bool backward, HeadJobs& g, int* splits_host) {
  FR_CHECK(nets && n >= 1 && n <= 4, "%s: %d nets", who, n);
  g.n = 0;
  for (int i = 0; i < n; ++i) {
    const frcnn_head_net& t = nets[i];
    if (splits_host) splits_host[i] = 0;
    if (t.P <= 0) continue;
    FR_CHECK(t.P <= 4096 && t.k >= 1 && t.H >= t.k && t.W >= t.k && t.Cin >= 1 && t.n >= 1, "%s: net %d: bad geometry", who, i);
    FR_CHECK(t.pos && t.in && t.w3 && t.bias3 && t.slope && t.w1 && t.bias1 && t.out && t.COL && t.HX && t.HY && t.OUT && t.slab,
             "%s: net %d: NULL argument", who, i);
    FR_CHECK(!backward || (t.delta && t.D && t.GH && t.gw3 && t.gbias3 && t.gslope && t.gw1 && t.gbias1 && (!t.gin || t.DX)),
             "%s: net %d: NULL argument of the backward pass", who, i);
    HeadJob j;
    j.Cin = t.Cin; j.H = t.H; j.W = t.W; j.k = t.k; j.Ho = t.H - t.k + 1; j.Wo = t.W - t.k + 1; j.n = t.n;
    j.P = t.P; j.pos = t.pos;
    j.in = t.in; j.gin = t.gin;
    j.bias3 = t.bias3; j.slope = t.slope; j.bias1 = t.bias1;
    j.gbias3 = t.gbias3; j.gslope = t.gslope; j.gbias1 = t.gbias1;
    j.w3 = t.w3; j.w1 = t.w1; j.gw3 = t.gw3; j.gw1 = t.gw1;
    j.out = t.out; j.delta = t.delta;
    j.COL = t.COL; j.HX = t.HX; j.HY = t.HY; j.OUT = t.OUT; j.D = t.D; j.GH = t.GH; j.DX = t.DX;
    j.hx_slab = t.slab; j.hx_splits = 0;
    FR_TRY(heads_add_job(g, j, t.force_splits, t.slab_floats > 0 ? (size_t)t.slab_floats : 0));
    if (splits_host) splits_host[i] = g.j[g.n - 1].hx_splits;
  }
  return FRCNN_OK;
}
int frcnn_heads_chain_forward(const frcnn_head_net* nets, int n, int* splits_host, void* stream) {
  HeadJobs g;
  FR_TRY(heads_table("frcnn_heads_chain_forward", nets, n, false, g, splits_host));
  return heads_chain_forward(g, S(stream));
}
int frcnn_heads_chain_backward(const frcnn_head_net* nets, int n, void* stream) {
  HeadJobs g;
  FR_TRY(heads_table("frcnn_heads_chain_backward", nets, n, true, g, nullptr));
  FR_TRY(heads_chain_backward_input(g, S(stream)));
  return heads_chain_backward_params(g, S(stream));
}
int frcnn_heads_plan_splits(int n, int ckk, int P) { return heads_plan_splits(n, ckk, P); }
int frcnn_gather_positions(const float* src, int C, long long hw, const int* pos, int P, float* dst, const float* slope,
                           float* dst_act, void* stream) {
  if (P <= 0) return FRCNN_OK;
  FR_CHECK(src && pos && dst && C >= 1 && hw >= 1 && (!slope == !dst_act), "frcnn_gather_positions: bad arguments");
  return gather_positions(src, C, hw, pos, P, dst, slope, dst_act, S(stream));
}
int frcnn_im2col_positions(const float* X, int C, int H, int W, int k, int Wo, const int* pos, int P, float* col, void* stream) {
  if (P <= 0) return FRCNN_OK;
  FR_CHECK(X && pos && col && C >= 1 && k >= 1 && H >= k && W >= k && Wo == W - k + 1, "frcnn_im2col_positions: bad arguments");
  return im2col_positions(X, C, H, W, k, Wo, pos, P, col, S(stream));
}
int frcnn_col2im_positions_add(const float* col, int C, int H, int W, int k, int Wo, const int* pos, int P, float* gX, void* stream) {
  if (P <= 0) return FRCNN_OK;
  FR_CHECK(col && pos && gX && C >= 1 && k >= 1 && H >= k && W >= k && Wo == W - k + 1, "frcnn_col2im_positions_add: bad arguments");
  return col2im_positions_add(col, C, H, W, k, Wo, pos, P, gX, S(stream));
}

// ---- test entry points (include/frcnn_hip_compact.h): the launches of a channel-compact dropout block (net.cpp plan_compact,
// pack_compact, wgrad_args) on tensors of the caller -- a gathered pack through the multi-job pack launch + conv_x3, and
// conv_wgrad through a WgradMap
// a gather / scatter table, read back: null = the identity (n entries must exist), negative = padding, every entry below `full`
static int compact_table(const char* who, const char* name, const int* tab, int n, int full, hipStream_t s) {
  if (!tab) {
    FR_CHECK(n <= full, "%s: %s is NULL (the identity) but the launch has %d entries and the tensor %d", who, name, n, full);
    return FRCNN_OK;
  }
  std::vector<int> h((size_t)n);
  FR_HIP(hipMemcpyAsync(h.data(), tab, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  FR_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) FR_CHECK(h[i] < full, "%s: %s[%d] = %d, the tensor has %d", who, name, i, h[i], full);
  return FRCNN_OK;
}

// mode 0: forward (K = nC channels, M = nO filters); mode 1: input gradient (K = nO, M = nC).  Hin x Win: the map the launch
// reads, cpad: conv_x3's padding.
static int conv2d_gathered(const char* who, int mode, const float* in, int Hin, int Win, const float* in_slope, const float* in_scale,
                           const float* weight, const float* bias, int O_full, int C_full, const int* oidx, int nO, const int* cidx,
                           int nC, int cpad, float* out, int out_mode, const float* rec_in, float* rec_out, const X3PostAct* post,
                           hipStream_t s) {
  const int Kc = mode == 0 ? nC : nO, M = mode == 0 ? nO : nC;
  const int Ho = Hin + 2 * cpad - 2, Wo = Win + 2 * cpad - 2;
  FR_CHECK(in && weight && out, "%s: NULL argument", who);
  FR_CHECK(O_full >= 1 && C_full >= 1 && nO >= 1 && nC >= 1 && Hin >= 1 && Win >= 1 && cpad >= 0 && Ho >= 1 && Wo >= 1,
           "%s: %d of %d filters, %d of %d channels, map %d x %d -> %d x %d", who, nO, O_full, nC, C_full, Hin, Win, Ho, Wo);
  FR_CHECK(conv_x3_eligible(Kc, M, 3), "%s: %d channels -> %d filters does not take the split form", who, Kc, M);
  bool f16 = get_x3_f16() != 0;
  if (f16 && in_scale) FR_TRY(scale_fits_f16_form(in_scale, Kc, s, &f16));
  FR_CHECK(f16 || (!rec_in && !rec_out), "%s: magnitude records belong to the fp16 form (option x3_f16, scale entries <= 1)", who);
  FR_TRY(compact_table(who, "oidx", oidx, nO, O_full, s));
  FR_TRY(compact_table(who, "cidx", cidx, nC, C_full, s));
  // the flat vector the pack reads: the full weight tensor, the full bias behind it (PackXJob::bias_off)
  const long nw = (long)O_full * C_full * 9;
  DevBuf flat, wp, bg, am, jobs, ident;
  // pack_x_job reads the source row pitch Cs only in its gathered branch: two NULL tables over a tensor with more channels than
  // the launch take that branch through an identity channel table
  if (!oidx && !cidx && C_full != nC) {
    std::vector<int> h((size_t)nC);
    for (int i = 0; i < nC; ++i) h[i] = i;
    FR_TRY(ident.ensure((size_t)nC * 4));
    FR_HIP(hipMemcpy(ident.p, h.data(), (size_t)nC * 4, hipMemcpyHostToDevice));
    cidx = (const int*)ident.p;
  }
  const float* base = weight;
  if (bias) {
    FR_TRY(flat.ensure((size_t)(nw + O_full) * 4));
    FR_HIP(hipMemcpyAsync(flat.p, weight, (size_t)nw * 4, hipMemcpyDeviceToDevice, s));
    FR_HIP(hipMemcpyAsync(flat.f() + nw, bias, (size_t)O_full * 4, hipMemcpyDeviceToDevice, s));
    FR_TRY(bg.ensure((size_t)nO * 4));
    base = flat.f();
  }
  FR_TRY(wp.ensure(conv_x3_pack_bytes(Kc, M, 3)));
  FR_TRY(jobs.ensure(sizeof(PackXJob)));
  if (f16) FR_TRY(am.ensure(X3_REC_BYTES));
  float* const amw = f16 ? am.f() + AMAX_REC : nullptr;       // the weights' record: of the FULL tensor, as pack_compact has it
  float* const aws = f16 ? am.f() + 2 * AMAX_REC : nullptr;   // their largest magnitude
  if (f16) {
    if (!rec_in) FR_TRY(tensor_absmax(in, (long)Kc * Hin * Win, am.f(), s));
    FR_TRY(tensor_absmax(base, nw, amw, s));
  }
  PackXJob g = conv_x3_pack_job(0, nO, nC, 3, mode, wp.p, Ho, Wo);
  g.oidx = oidx; g.cidx = cidx; g.Cs = C_full;
  if (bias) { g.bias_off = nw; g.bias_dst = bg.f(); }
  g.amax = amw; g.amax_w = aws;
  const int grid = conv_x3_pack_assign_blocks(&g, 1);
  FR_HIP(hipMemcpy(jobs.p, &g, sizeof(PackXJob), hipMemcpyHostToDevice));
  int rc = conv_x3_pack_multi(base, (const PackXJob*)jobs.p, 1, grid, s);
  if (rc == FRCNN_OK)
    rc = conv_x3(in, Kc, Hin, Win, in_slope, in_scale, wp.p, bias ? bg.f() : nullptr, M, 3, cpad, out, out_mode, 0, s, 0, post,
                 f16 ? (rec_in ? rec_in : am.f()) : nullptr, aws, rec_out);
  (void)hipStreamSynchronize(s);
  return rc;
}
int frcnn_conv2d_forward_gathered(const float* in, int H, int W, const float* in_slope, const float* in_scale, const float* weight,
                                  const float* bias, int O_full, int C_full, const int* oidx, int nO, const int* cidx, int nC,
                                  int pad, float* out, const float* rec_in, float* rec_out, void* stream) {
  return conv2d_gathered("frcnn_conv2d_forward_gathered", 0, in, H, W, in_slope, in_scale, weight, bias, O_full, C_full, oidx, nO,
                         cidx, nC, pad, out, OUT_STORE, rec_in, rec_out, nullptr, S(stream));
}
int frcnn_conv2d_backward_input_gathered(const float* gout, int Ho, int Wo, const float* weight, int O_full, int C_full,
                                         const int* oidx, int nO, const int* cidx, int nC, int pad, float* gin, int accumulate,
                                         const float* rec_g, float* rec_out, const float* post_x, const float* post_slope,
                                         const float* post_scale, float* gslope, void* stream) {
  const char* who = "frcnn_conv2d_backward_input_gathered";
  FR_CHECK(pad >= 0 && pad <= 2, "%s: padding %d", who, pad);
  FR_CHECK(post_x || (!post_slope && !post_scale && !gslope), "%s: a fused activation backward needs post_x", who);
  FR_CHECK(!post_x || (post_slope && !accumulate), "%s: the fused activation backward belongs to a storing launch with a slope", who);
  const X3PostAct post{post_x, post_slope, post_scale, gslope};
  return conv2d_gathered(who, 1, gout, Ho, Wo, nullptr, nullptr, weight, nullptr, O_full, C_full, oidx, nO, cidx, nC, 2 - pad, gin,
                         accumulate ? OUT_ADD : OUT_STORE, rec_g, rec_out, post_x ? &post : nullptr, S(stream));
}
int frcnn_conv2d_backward_weight_mapped(const float* in, int Cin, int H, int W, const float* in_slope, const float* in_scale,
                                        const float* gout, int O, int pad, float* gweight, float* gbias, int O_full, int Cfull,
                                        const int* omap, const int* cmap, void* stream) {
  const char* who = "frcnn_conv2d_backward_weight_mapped";
  hipStream_t s = S(stream);
  const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
  FR_CHECK(in && gout && gweight, "%s: NULL argument", who);
  FR_CHECK(Cin >= 1 && O >= 1 && O_full >= 1 && Cfull >= 1 && H >= 1 && W >= 1 && pad >= 0 && Ho >= 1 && Wo >= 1,
           "%s: %d of %d filters, %d of %d channels, map %d x %d -> %d x %d", who, O, O_full, Cin, Cfull, H, W, Ho, Wo);
  FR_CHECK(conv_wgradx_eligible(Cin, O, 3), "%s: a gathered weight gradient needs a conv_wgradx shape, not %d channels x %d filters",
           who, Cin, O);
  FR_CHECK(omap || cmap || Cfull == Cin, "%s: no table, but the tensor has %d channels and the launch %d", who, Cfull, Cin);
  FR_TRY(compact_table(who, "omap", omap, O, O_full, s));
  FR_TRY(compact_table(who, "cmap", cmap, Cin, Cfull, s));
  bool unit = true;
  FR_TRY(scale_fits_f16_form(in_scale, Cin, s, &unit));
  DevBuf ws, am;
  FR_TRY(ws.ensure(conv_wgrad_workspace_bytes(Cin, H, W, O, 3, pad)));
  const bool f16 = unit && get_x3_f16();
  if (f16) {   // (the records of both tensors, as frcnn_conv2d_backward_weight takes them)
    FR_TRY(am.ensure(X3_REC_BYTES));
    FR_TRY(tensor_absmax(in, (long)Cin * H * W, am.f(), s));
    FR_TRY(tensor_absmax(gout, (long)O * Ho * Wo, am.f() + AMAX_REC, s));
  }
  const WgradMap map{omap, cmap, Cfull};
  const int rc = conv_wgrad(in, Cin, H, W, in_slope, in_scale, gout, O, 3, pad, gweight, ws.p, ws.bytes, s, gbias,
                            f16 ? am.f() : nullptr, f16 ? am.f() + AMAX_REC : nullptr, &map);
  (void)hipStreamSynchronize(s);
  return rc;
}

int frcnn_roi_pool_forward(const float* fmap, int C, int H, int W, const int* wins, int R, int kh, int kw,
                           float* out, int* idx, void* stream) {
  return roi_pool_forward(fmap, C, H, W, wins, R, kh, kw, out, idx, S(stream));
}
int frcnn_roi_pool_backward(float* gmap, int C, int H, int W, const float* gout, const int* idx, int R, int kh,
                            int kw, void* stream) {
  return roi_pool_backward(gmap, C, H, W, gout, idx, R, kh, kw, S(stream));
}

static int roi_align_check(const char* who, const void* map, int C, int H, int W, const void* rows, const double* rect, int kh, int kw,
                           int g) {
  FR_CHECK(map && rows && rect, "%s: NULL argument", who);
  FR_CHECK(C >= 1 && H >= 1 && W >= 1 && kh >= 1 && kw >= 1, "%s: map %d x %d x %d, grid %d x %d", who, C, H, W, kh, kw);
  FR_CHECK((long)H * W < (1L << 31), "%s: a plane of %d x %d cells", who, H, W);
  FR_CHECK(g >= 1 && g <= 4, "%s: sampling ratio %d outside 1..4", who, g);
  return FRCNN_OK;
}
int frcnn_roi_align_forward(const float* fmap, int C, int H, int W, const double* rect, const long long* pick, int R, double inv_sx,
                            double inv_sy, int kh, int kw, int g, float* out, void* stream) {
  if (R <= 0) return FRCNN_OK;
  FR_TRY(roi_align_check("frcnn_roi_align_forward", fmap, C, H, W, out, rect, kh, kw, g));
  return roi_align_forward(fmap, C, H, W, rect, pick, R, inv_sx, inv_sy, kh, kw, g, out, S(stream));
}
int frcnn_roi_align_backward(float* gmap, int C, int H, int W, const float* gout, const double* rect, const long long* pick, int R,
                             double inv_sx, double inv_sy, int kh, int kw, int g, void* stream) {
  if (R <= 0) return FRCNN_OK;
  FR_TRY(roi_align_check("frcnn_roi_align_backward", gmap, C, H, W, gout, rect, kh, kw, g));
  return roi_align_backward(gmap, C, H, W, gout, rect, pick, R, inv_sx, inv_sy, kh, kw, g, S(stream));
}

static void to_layers(const float* const* maps, const int* H, const int* W, RpnLayers* L) {
  for (int l = 0; l < 4; ++l) { L->map[l] = maps ? maps[l] : nullptr; L->H[l] = H[l]; L->W[l] = W[l]; }
}
size_t frcnn_rpn_scan_workspace_bytes(const int* H, const int* W) {
  RpnLayers L;
  to_layers(nullptr, H, W, &L);
  return rpn_scan_workspace_bytes(L);
}
int frcnn_rpn_scan(const float* const* maps, const int* H, const int* W, const float* anchor_w,
                   const float* anchor_h, double img_w, double img_h, double p_threshold, int cap,
                   float* match_p, int* match_idx, double* match_rect, float* match_box, int* count,
                   void* ws, size_t ws_bytes, void* stream) {
  RpnLayers L;
  to_layers(maps, H, W, &L);
  return rpn_scan(L, anchor_w, anchor_h, img_w, img_h, p_threshold, cap, match_p, match_idx, match_rect,
                  match_box, count, ws, ws_bytes, S(stream));
}
size_t frcnn_rpn_scan_batch_workspace_bytes(const int* H, const int* W, int B) {
  RpnLayers L;
  to_layers(nullptr, H, W, &L);
  return rpn_scan_batch_workspace_bytes(L, B);
}
int frcnn_rpn_scan_batch(const float* const* maps, const int* H, const int* W, int B, long long slot_stride, const float* anchor_w,
                         const float* anchor_h, double img_w, double img_h, double p_threshold, int cap, float* match_p,
                         int* match_idx, double* match_rect, float* match_box, int* count, void* ws, size_t ws_bytes,
                         void* stream) {
  FR_CHECK(maps && H && W, "frcnn_rpn_scan_batch: NULL argument");
  RpnLayers L;
  to_layers(maps, H, W, &L);
  return rpn_scan_batch(L, B, (long)slot_stride, anchor_w, anchor_h, img_w, img_h, p_threshold, cap, match_p, match_idx,
                        match_rect, match_box, count, ws, ws_bytes, S(stream));
}
size_t frcnn_rpn_scan_ragged_workspace_bytes(const int* Hs, const int* Ws, int B) {
  return rpn_scan_ragged_workspace_bytes(Hs, Ws, B);
}
int frcnn_rpn_scan_ragged(const float* heads, const long long* map_off, const int* Hs, const int* Ws, const double* img_wh, int B,
                          const float* anchor_w, const float* anchor_h, double p_threshold, int cap, float* match_p,
                          int* match_idx, double* match_rect, float* match_box, int* count, void* ws, size_t ws_bytes,
                          void* stream) {
  return rpn_scan_ragged(heads, map_off, Hs, Ws, img_wh, B, anchor_w, anchor_h, p_threshold, cap, match_p, match_idx, match_rect,
                         match_box, count, ws, ws_bytes, S(stream));
}
int frcnn_rpn_loss(const float* const* maps, float* const* deltas, const int* H, const int* W, const int* ex_idx,
                   const double* ex_anchor, const double* ex_roi, const int* ex_class, int npos, int nneg,
                   int bgclass, double* ex_loss, float* crtarget, float* cctarget, void* stream) {
  RpnLayers L;
  to_layers(maps, H, W, &L);
  return rpn_loss(L, deltas, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, bgclass, ex_loss, crtarget,
                  cctarget, S(stream));
}

int frcnn_loss_accumulate(const double* ex_loss, int E, double* acc, void* stream) {
  return loss_accumulate(ex_loss, E, acc, S(stream));
}

// The Linear products as the classification net runs them (linear.h), on scratch of the call: planes and records for the requested
// roles only, freed on return -- so a call that took the split form synchronises first.
int frcnn_linear_forward(const float* x, int R, int I, const float* weight, const float* bias, int O, float* y,
                         void* stream) {
  // Y[R][O] = X[R][I] * W[O][I]^T + b
  Linear L;
  int rc = L.ensure(R, I, O, 1);
  if (rc == FRCNN_OK) rc = L.forward(x, weight, bias, y, -1, S(stream), 0, nullptr);
  if (L.x_form) (void)hipStreamSynchronize(S(stream));
  return rc;
}
int frcnn_linear_backward(const float* x, const float* gy, int R, int I, const float* weight, int O, float* gx,
                          float* gweight, float* gbias, void* stream) {
  Linear L;
  int rc = L.ensure(R, I, O, (gx ? 2 : 0) | (gweight ? 4 : 0));
  if (rc == FRCNN_OK) rc = L.weight_record(weight, -1, S(stream));   // (in the forward pass's place: the input gradient's fp16 form needs it)
  if (rc == FRCNN_OK) rc = L.dgrad(gy, weight, gx, S(stream), 0, nullptr);
  if (rc == FRCNN_OK) rc = L.wgrad(gy, x, weight, gweight, gbias, S(stream), 0);
  if (L.x_form) (void)hipStreamSynchronize(S(stream));
  return rc;
}

// optim.rmsprop (main.lua:122,133)
int frcnn_rmsprop(float* x, const float* g, float* m, long long n, float lr, float alpha, float eps,
                  void* stream) {
  FR_CHECK(n >= 0, "frcnn_rmsprop: bad length %lld", n);
  return rmsprop_update(x, const_cast<float*>(g), m, 0, n, false, 1.f, nullptr, lr, alpha, eps, S(stream));   // unscaled: g is only read
}
int frcnn_scale_rmsprop(float* x, float* g, float gscale, float* m, long long n, float lr, float alpha, float eps,
                        void* stream) {
  FR_CHECK(n >= 0, "frcnn_scale_rmsprop: bad length %lld", n);
  return rmsprop_update(x, g, m, 0, n, false, gscale, nullptr, lr, alpha, eps, S(stream));
}
int frcnn_scale_rmsprop_slice(float* x, float* g, float gscale, float* m, long long lo, long long hi, float lr, float alpha,
                              float eps, void* stream) {
  return rmsprop_update(x, g, m, lo, hi, true, gscale, nullptr, lr, alpha, eps, S(stream));
}
int frcnn_scale_rmsprop_dev(float* x, float* g, const double* gcount_dev, float* m, long long n, float lr, float alpha,
                            float eps, void* stream) {
  FR_CHECK(gcount_dev, "frcnn_scale_rmsprop_dev: NULL divisor");
  FR_CHECK(n >= 0, "frcnn_scale_rmsprop_dev: bad length %lld", n);
  return rmsprop_update(x, g, m, 0, n, false, 1.f, gcount_dev, lr, alpha, eps, S(stream));
}

// optim.sgd / optim.nag (main.lua:122-124,134-135)
int frcnn_sgd(float* x, float* g, float* v, long long n, float gscale, const double* gcount_dev, float clr, float wd, float mom,
              float one_minus_damp, int nesterov, int first, void* stream) {
  FR_CHECK(n >= 0, "frcnn_sgd: bad length %lld", n);
  return sgd_update(x, g, v, 0, n, false, gscale, gcount_dev, clr, wd, mom, one_minus_damp, nesterov != 0, first != 0, S(stream));
}
int frcnn_sgd_slice(float* x, float* g, float* v, long long lo, long long hi, float gscale, float clr, float wd, float mom,
                    float one_minus_damp, int nesterov, int first, void* stream) {
  return sgd_update(x, g, v, lo, hi, true, gscale, nullptr, clr, wd, mom, one_minus_damp, nesterov != 0, first != 0, S(stream));
}
int frcnn_nag(float* x, float* g, float* v, long long n, float gscale, const double* gcount_dev, float clr, float wd, float mom,
              int first, void* stream) {
  FR_CHECK(n >= 0, "frcnn_nag: bad length %lld", n);
  return nag_update(x, g, v, 0, n, false, gscale, gcount_dev, clr, wd, mom, first != 0, S(stream));
}
int frcnn_nag_slice(float* x, float* g, float* v, long long lo, long long hi, float gscale, float clr, float wd, float mom,
                    int first, void* stream) {
  return nag_update(x, g, v, lo, hi, true, gscale, nullptr, clr, wd, mom, first != 0, S(stream));
}
// the device-divisor forms of the slice updates, and the gradient guard in front of them
int frcnn_scale_rmsprop_slice_dev(float* x, float* g, const double* gcount_dev, float* m, long long lo, long long hi, float lr,
                                  float alpha, float eps, void* stream) {
  FR_CHECK(gcount_dev, "frcnn_scale_rmsprop_slice_dev: NULL divisor");
  return rmsprop_update(x, g, m, lo, hi, true, 1.f, gcount_dev, lr, alpha, eps, S(stream));
}
int frcnn_sgd_slice_dev(float* x, float* g, float* v, long long lo, long long hi, const double* gcount_dev, float clr, float wd,
                        float mom, float one_minus_damp, int nesterov, int first, void* stream) {
  FR_CHECK(gcount_dev, "frcnn_sgd_slice_dev: NULL divisor");
  return sgd_update(x, g, v, lo, hi, true, 1.f, gcount_dev, clr, wd, mom, one_minus_damp, nesterov != 0, first != 0, S(stream));
}
int frcnn_nag_slice_dev(float* x, float* g, float* v, long long lo, long long hi, const double* gcount_dev, float clr, float wd,
                        float mom, int first, void* stream) {
  FR_CHECK(gcount_dev, "frcnn_nag_slice_dev: NULL divisor");
  return nag_update(x, g, v, lo, hi, true, 1.f, gcount_dev, clr, wd, mom, first != 0, S(stream));
}
// optim.adam (optim/adam.lua; decay: AdamW)
int frcnn_adam(float* x, float* g, float* m, float* v, long long n, float gscale, const double* gcount_dev, float step, float beta1,
               float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float wd, float decay, void* stream) {
  FR_CHECK(n >= 0, "frcnn_adam: bad length %lld", n);
  return adam_update(x, g, m, v, 0, n, false, gscale, gcount_dev, step, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, wd,
                     decay, S(stream));
}
int frcnn_adam_slice(float* x, float* g, float* m, float* v, long long lo, long long hi, float gscale, float step, float beta1,
                     float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float wd, float decay, void* stream) {
  return adam_update(x, g, m, v, lo, hi, true, gscale, nullptr, step, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, wd,
                     decay, S(stream));
}
int frcnn_adam_slice_dev(float* x, float* g, float* m, float* v, long long lo, long long hi, const double* gcount_dev, float step,
                         float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float wd, float decay,
                         void* stream) {
  FR_CHECK(gcount_dev, "frcnn_adam_slice_dev: NULL divisor");
  return adam_update(x, g, m, v, lo, hi, true, 1.f, gcount_dev, step, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, wd,
                     decay, S(stream));
}
size_t frcnn_grad_clip_workspace_bytes(long long n) { return grad_clip_workspace_bytes(n); }
int frcnn_grad_clip(float* g, long long n, const long long* ranges_host, int nranges, double divisor, const double* divisor_dev,
                    double clip_norm, double* record_dev, void* workspace, size_t workspace_bytes, void* stream) {
  return grad_clip(g, n, ranges_host, nranges, divisor, divisor_dev, clip_norm, record_dev, workspace, workspace_bytes, S(stream));
}
int frcnn_nag_lookahead(float* x, const float* v, long long n, float mom, void* stream) {
  return nag_lookahead(x, v, n, mom, S(stream));
}
int frcnn_nag_lookahead_slice(float* x, const float* v, long long lo, long long hi, float mom, void* stream) {
  return nag_lookahead_slice(x, v, lo, hi, mom, S(stream));
}

int frcnn_cnet_losses(float* crout, const float* crtarget, const float* ccout, const float* cctarget, int R,
                      int npos, int ncls, float* crdelta, float* ccdelta, double* loss2, void* stream) {
  return cnet_losses(crout, crtarget, ccout, cctarget, R, npos, ncls, crdelta, ccdelta, loss2, S(stream));
}
int frcnn_cnet_decode(const float* cls_out, int R, int ncls, int* cls, float* conf, void* stream) {
  return cnet_decode(cls_out, R, ncls, cls, conf, S(stream));
}

// ---------------------------------------------------------------- image preparation (image.hip)
int frcnn_image_rgb2yuv(const float* rgb, float* yuv, int H, int W, void* stream) {
  FR_CHECK(rgb != yuv, "image_rgb2yuv: in-place conversion is not supported");
  return image_rgb2yuv(rgb, yuv, H, W, S(stream));
}
int frcnn_image_rgb2hsv(const float* rgb, float* hsv, int H, int W, void* stream) {
  FR_CHECK(rgb != hsv, "image_rgb2hsv: in-place conversion is not supported");
  return image_rgb2hsv(rgb, hsv, H, W, S(stream));
}
int frcnn_image_rgb2lab(const float* rgb, float* lab, int H, int W, void* stream) {
  FR_CHECK(rgb != lab, "image_rgb2lab: in-place conversion is not supported");
  return image_rgb2lab(rgb, lab, H, W, S(stream));
}
int frcnn_image_scale(const float* src, int C, int H, int W, float* dst, int dH, int dW, float* tmp, int rgb2yuv,
                      void* stream) {
  return image_scale(src, C, H, W, dst, dH, dW, tmp, rgb2yuv, S(stream));
}
int frcnn_image_scale_u8(const unsigned char* src_hwc, int H, int W, float* dst, int dH, int dW, float* tmp, int rgb2yuv,
                         void* stream) {
  return image_scale_u8(src_hwc, H, W, dst, dH, dW, tmp, rgb2yuv, S(stream));
}
int frcnn_image_crop_flip(const float* src, int C, int H, int W, int x0, int y0, int w, int h, int hflip, int vflip,
                          float* dst, void* stream) {
  return image_crop_flip(src, C, H, W, x0, y0, w, h, hflip, vflip, dst, S(stream));
}
size_t frcnn_image_normalize_workspace_bytes(int C) { return image_normalize_workspace_bytes(C); }
int frcnn_image_normalize(float* img, int C, int H, int W, int centering, int scaling, void* ws, size_t ws_bytes,
                          void* stream) {
  return image_normalize(img, C, H, W, centering, scaling, ws, ws_bytes, S(stream));
}
int frcnn_image_contrastive_norm(const float* in, int H, int W, const float* kernel_host, int K, float threshold,
                                 float* out, float* tmp, void* stream) {
  return image_contrastive_norm(in, H, W, kernel_host, K, threshold, out, tmp, S(stream));
}

}  // extern "C"
