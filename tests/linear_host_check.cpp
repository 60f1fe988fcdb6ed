// Host check of csrc/linear.h (Linear: the operand forms of a large Linear layer and the launches each queues) without a GPU.
// The kernels' launchers and the allocation calls are replaced by the stand-ins below, which append one line per call to a log;
// the log is compared with the tables further down, written out by hand from the launch order the classification net has always
// had -- never produced by the code under test.  Built with -fsanitize=address,undefined and run by tests/test_linear_host.py,
// once per setting of FRCNN_GEMM_F16 / FRCNN_GEMM_WGRAD_F16 (read once per process, as in the library); exits 0 when every
// sequence matched and every allocation was freed exactly once.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

// ---- stand-ins for what linear.h and own.h expect from common.h, kernels.h and the HIP runtime ---------------------------
typedef int hipError_t;
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
enum { hipSuccess = 0, hipEventDisableTiming = 2, hipHostMallocDefault = 0 };
enum { FRCNN_OK = 0, FRCNN_ERR_HIP = 2 };
enum { OUT_STORE = 0, OUT_ADD = 1 };
#define AMAX_REC 16400
#define FR_HIP(expr) do { if ((expr) != hipSuccess) return FRCNN_ERR_HIP; } while (0)
#define FR_TRY(expr) do { int r_ = (expr); if (r_ != FRCNN_OK) return r_; } while (0)
struct GemmFold { const float* slab = nullptr; int nSplit = 0; const float* bias = nullptr; };

static std::set<void*> live_dev;
static int mallocs = 0, frees = 0, bad = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { std::fprintf(stderr, "linear_host_check: %s\n", what); ++bad; }
}
static hipError_t hipMalloc(void** p, size_t n) { *p = std::malloc(n); live_dev.insert(*p); ++mallocs; return hipSuccess; }
static hipError_t hipFree(void* p) {
  expect(live_dev.erase(p) == 1, "hipFree of a pointer that is not a live allocation");
  std::free(p); ++frees;
  return hipSuccess;
}
static hipError_t hipEventCreateWithFlags(hipEvent_t*, unsigned) { return hipSuccess; }   // (own.h's Event: not used here)
static hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = std::malloc(n); return hipSuccess; }
static hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }

#include "../faster-rcnn.torch_amd/csrc/own.h"

// the switches the stand-ins answer from
static int g_eligible = 0;   // roles linear_x_eligible grants
static int g_x3_f16 = 0;     // option x3_f16
static bool linear_x_eligible(int role, int, int, int) { return (g_eligible & role) != 0; }
static int linear_x_rows_padded(int R) { return (R + 15) & ~15; }
static int get_x3_f16() { return g_x3_f16; }

// the tensors of the calls: only their addresses matter
static float X[1], G[1], W[1], W2[1], BIAS[1], Y[1], GX[1], GW[1], GB[1];
static int S1_, S2_;
static const hipStream_t S1 = (hipStream_t)&S1_, S2 = (hipStream_t)&S2_;

namespace frcnn { struct Linear; }
static const frcnn::Linear* g_cur = nullptr;   // the layer whose planes and records the log names
static std::string name(const void* p);
static std::vector<std::string> g_log;
static void logf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void logf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_log.push_back(buf);
}
#define N(p) name(p).c_str()
static const char* sname(hipStream_t s) { return s == S1 ? "s1" : s == S2 ? "s2" : "s?"; }

static int tensor_absmax(const float* x, long n, float* rec, hipStream_t s) {
  logf("absmax %s %s %ld -> %s", sname(s), N(x), n, N(rec));
  return FRCNN_OK;
}
static int split_planes(const float* src, int R, int C, void* P, void* PT, hipStream_t s, const float* amax = nullptr) {
  logf("split %s %s %d %d -> %s %s rec=%s", sname(s), N(src), R, C, N(P), N(PT), N(amax));
  return FRCNN_OK;
}
static int linear_x_forward(const void* Xp, int R, int I, const float* w, const float* bias, int O, float* y, hipStream_t s, int ws_slot = 0,
                            GemmFold* defer = nullptr, const float* amax_x = nullptr, const float* amax_w = nullptr) {
  logf("xfwd %s %s %d %d %s %s %d -> %s slot=%d defer=%d rec=%s,%s", sname(s), N(Xp), R, I, N(w), N(bias), O, N(y), ws_slot, defer != nullptr,
       N(amax_x), N(amax_w));
  return FRCNN_OK;
}
static int linear_x_dgrad(const void* Gp, int R, int O, const float* w, int I, float* gx, int out_mode, hipStream_t s, int ws_slot = 0,
                          GemmFold* defer = nullptr, const float* amax_g = nullptr, const float* amax_w = nullptr) {
  logf("xdgrad %s %s %d %d %s %d -> %s %s slot=%d defer=%d rec=%s,%s", sname(s), N(Gp), R, O, N(w), I, N(gx), out_mode == OUT_STORE ? "store" : "add",
       ws_slot, defer != nullptr, N(amax_g), N(amax_w));
  return FRCNN_OK;
}
static int linear_x_wgrad(const void* GpT, const void* XpT, int R, int O, int I, float* gw, hipStream_t s, int ws_slot = 0,
                          const float* amax_g = nullptr, const float* amax_x = nullptr) {
  logf("xwgrad %s %s %s %d %d %d -> %s slot=%d rec=%s,%s", sname(s), N(GpT), N(XpT), R, O, I, N(gw), ws_slot, N(amax_g), N(amax_x));
  return FRCNN_OK;
}
static int gemm_f32(const float* A, long sAm, long sAk, const float* B, long sBk, long sBn, float* C, long ldc, int M, int Nn, int K,
                    int out_mode, const float* bias_n, hipStream_t s, int ws_slot = 0, GemmFold* defer = nullptr) {
  logf("gemm %s %s %ld %ld %s %ld %ld -> %s %ld %d %d %d %s bias=%s slot=%d defer=%d", sname(s), N(A), sAm, sAk, N(B), sBk, sBn, N(C), ldc, M, Nn, K,
       out_mode == OUT_STORE ? "store" : "add", N(bias_n), ws_slot, defer != nullptr);
  return FRCNN_OK;
}
static int channel_sum_cols(const float* g, int R, int O, float* gb, hipStream_t s) {
  logf("bias %s %s %d %d -> %s", sname(s), N(g), R, O, N(gb));
  return FRCNN_OK;
}

#include "../faster-rcnn.torch_amd/csrc/linear.h"
using namespace frcnn;

static std::string name(const void* p) {
  if (!p) return "-";
  const struct { const void* q; const char* n; } fixed[] = {{X, "x"}, {G, "g"}, {W, "W"}, {W2, "W2"}, {BIAS, "b"}, {Y, "y"},
                                                           {GX, "gx"}, {GW, "gw"}, {GB, "gb"}};
  for (auto& f : fixed) if (f.q == p) return f.n;
  if (g_cur) {
    if (p == g_cur->xp.p) return "xp";
    if (p == g_cur->gp.p) return "gp";
    if (p == g_cur->xpT.p) return "xpT";
    if (p == g_cur->gpT.p) return "gpT";
    const char* recs[] = {"rX", "rG", "rW", "rGT", "rXT"};   // the five records, in the order of their slots
    for (int r = 0; r < 5; ++r) if (g_cur->am.p && p == g_cur->am.f() + (size_t)r * AMAX_REC) return recs[r];
  }
  return "?";
}

// ---- the expected sequences, for R = 50 (padded to 64), I = 16, O = 8.  $S: the stream, $K: the workspace slot, $D: whether a
// deferred fold was asked for.
typedef std::vector<std::string> Table;
static const Table REC_W_TAKEN = {"absmax $S W 128 -> rW"};
static const Table FWD_F16 = {
    "absmax $S x 800 -> rX",
    "split $S x 50 16 -> xp - rec=rX",
    "xfwd $S xp 50 16 W b 8 -> y slot=$K defer=$D rec=rX,rW"};
static const Table FWD_X3 = {
    "split $S x 50 16 -> xp - rec=-",
    "xfwd $S xp 50 16 W b 8 -> y slot=$K defer=$D rec=-,-"};
static const Table FWD_F32 = {"gemm $S x 16 1 W 1 16 -> y 8 50 8 16 store bias=b slot=$K defer=$D"};
static const Table DG_F16 = {
    "absmax $S g 400 -> rG",
    "split $S g 50 8 -> gp - rec=rG",
    "xdgrad $S gp 50 8 W 16 -> gx store slot=$K defer=$D rec=rG,rW"};
static const Table DG_X3 = {
    "split $S g 50 8 -> gp - rec=-",
    "xdgrad $S gp 50 8 W 16 -> gx store slot=$K defer=$D rec=-,-"};
static const Table DG_F32 = {"gemm $S g 8 1 W 16 1 -> gx 16 50 16 8 store bias=- slot=$K defer=$D"};
static const Table WG_F16_OWN = {   // both magnitudes taken on the weight-gradient stream
    "absmax $S g 400 -> rGT",
    "absmax $S x 800 -> rXT",
    "split $S g 50 8 -> - gpT rec=rGT",
    "split $S x 50 16 -> - xpT rec=rXT",
    "xwgrad $S gpT xpT 50 8 16 -> gw slot=$K rec=rGT,rXT",
    "bias $S g 50 8 -> gb"};
static const Table WG_F16_BORROW = {   // the input's record is the forward pass's
    "absmax $S g 400 -> rGT",
    "split $S g 50 8 -> - gpT rec=rGT",
    "split $S x 50 16 -> - xpT rec=rX",
    "xwgrad $S gpT xpT 50 8 16 -> gw slot=$K rec=rGT,rX",
    "bias $S g 50 8 -> gb"};
static const Table WG_X3 = {
    "split $S g 50 8 -> - gpT rec=-",
    "split $S x 50 16 -> - xpT rec=-",
    "xwgrad $S gpT xpT 50 8 16 -> gw slot=$K rec=-,-",
    "bias $S g 50 8 -> gb"};
static const Table WG_F32 = {
    "gemm $S g 1 8 x 16 1 -> gw 16 8 16 50 add bias=- slot=$K defer=0",
    "bias $S g 50 8 -> gb"};
static const Table NOTHING = {};

static Table operator+(const Table& a, const Table& b) { Table r(a); r.insert(r.end(), b.begin(), b.end()); return r; }
static std::string subst(std::string t, const char* key, const std::string& v) {
  for (size_t at; (at = t.find(key)) != std::string::npos;) t.replace(at, std::strlen(key), v);
  return t;
}
// compares the log with the table and clears it
static void check(const char* what, const Table& want, const char* stream = "s1", int slot = 0, bool defer = false) {
  bool same = g_log.size() == want.size();
  for (size_t i = 0; same && i < want.size(); ++i)
    same = g_log[i] == subst(subst(subst(want[i], "$S", stream), "$K", std::to_string(slot)), "$D", defer ? "1" : "0");
  if (!same) {
    std::fprintf(stderr, "linear_host_check: %s (stream %s, slot %d, defer %d): queued\n", what, stream, slot, (int)defer);
    for (auto& l : g_log) std::fprintf(stderr, "    %s\n", l.c_str());
    std::fprintf(stderr, "  expected\n");
    for (auto& l : want) std::fprintf(stderr, "    %s\n", l.c_str());
    ++bad;
  }
  g_log.clear();
}

static bool env_on(const char* n) { const char* e = std::getenv(n); return e ? std::atoi(e) != 0 : true; }

int main() {
  // what the fp16 configuration (eligible, option x3_f16 on) queues under this process's environment
  const bool f16 = env_on("FRCNN_GEMM_F16"), wf16 = f16 && env_on("FRCNN_GEMM_WGRAD_F16");
  const Table& REC_W_16 = f16 ? REC_W_TAKEN : NOTHING;
  const Table& FWD_16 = f16 ? FWD_F16 : FWD_X3;
  const Table& DG_16 = f16 ? DG_F16 : DG_X3;
  const Table& WG_16_OWN = wf16 ? WG_F16_OWN : WG_X3;
  const Table& WG_16_BORROW = wf16 ? WG_F16_BORROW : WG_X3;
  GemmFold fold;

  struct Form { const char* name; int eligible, x3; const Table *rec_w, *fwd, *dg, *wg; };
  const Form forms[] = {{"fp32", 0, 0, &NOTHING, &FWD_F32, &DG_F32, &WG_F32},
                        {"fp32, option x3_f16", 0, 1, &NOTHING, &FWD_F32, &DG_F32, &WG_F32},
                        {"three-plane", 7, 0, &NOTHING, &FWD_X3, &DG_X3, &WG_X3},
                        {"fp16", 7, 1, &REC_W_16, &FWD_16, &DG_16, &WG_16_BORROW}};
  for (const Form& f : forms) {   // a training step, on either stream and slot
    g_eligible = f.eligible; g_x3_f16 = f.x3;
    Linear L;
    g_cur = &L;
    const int before = mallocs;
    expect(L.ensure(50, 16, 8, 7) == FRCNN_OK && L.x_form == f.eligible, f.name);
    expect(mallocs - before == (f.eligible ? 5 : 0), "ensure: planes and records exactly when a role is split");
    check("ensure queues nothing", NOTHING);
    expect(L.forward(X, W, BIAS, Y, -1, S1, 0, &fold) == FRCNN_OK, "forward");
    check(f.name, *f.rec_w + *f.fwd, "s1", 0, true);
    expect(L.forward(X, W, BIAS, Y, -1, S2, 7, nullptr) == FRCNN_OK, "forward");
    check(f.name, *f.rec_w + *f.fwd, "s2", 7, false);   // (a training pass takes the weights' record every time)
    expect(L.dgrad(G, W, GX, S1, 0, &fold) == FRCNN_OK, "dgrad");
    check(f.name, *f.dg, "s1", 0, true);
    expect(L.dgrad(G, W, GX, S2, 7, nullptr) == FRCNN_OK, "dgrad");
    check(f.name, *f.dg, "s2", 7, false);
    expect(L.dgrad(G, W, nullptr, S1, 0, &fold) == FRCNN_OK, "dgrad without gx");
    check("a null gx queues nothing", NOTHING);
    expect(L.wgrad(G, X, W, GW, GB, S2, 7) == FRCNN_OK, "wgrad");
    check(f.name, *f.wg, "s2", 7);
    expect(L.wgrad(G, X, W, GW, GB, S1, 0) == FRCNN_OK, "wgrad");
    check(f.name, *f.wg, "s1", 0);
    expect(L.ensure(50, 16, 8, 7) == FRCNN_OK && mallocs - before == (f.eligible ? 5 : 0), "a second ensure of the same shape allocates nothing");
    g_cur = nullptr;
  }
  expect(mallocs == frees && live_dev.empty(), "device allocations after the training steps");

  g_eligible = 7; g_x3_f16 = 1;
  {  // evaluate mode under static_weights: the weights' record is kept within one generation, from one matrix
    Linear L;
    g_cur = &L;
    L.ensure(50, 16, 8, 7);
    L.forward(X, W, BIAS, Y, 5, S1, 0, nullptr);
    check("first static pass takes the weights' record", REC_W_16 + FWD_16);
    L.forward(X, W, BIAS, Y, 5, S1, 0, nullptr);
    check("second static pass keeps it", FWD_16);
    L.forward(X, W, BIAS, Y, 6, S1, 0, nullptr);
    check("a new generation takes it again", REC_W_16 + FWD_16);
    L.forward(X, W, BIAS, Y, 6, S1, 0, nullptr);
    check("... once", FWD_16);
    L.forward(X, W2, BIAS, Y, 6, S1, 0, nullptr);
    Table other = REC_W_16 + FWD_16;
    for (auto& l : other) l = subst(l, " W ", " W2 ");
    check("another matrix takes it again", other);
    L.forward(X, W, BIAS, Y, -1, S1, 0, nullptr);
    check("a training pass takes it", REC_W_16 + FWD_16);
    L.forward(X, W, BIAS, Y, -1, S1, 0, nullptr);
    check("... every time", REC_W_16 + FWD_16);
    L.forward(X, W, BIAS, Y, 6, S1, 0, nullptr);
    check("and leaves nothing for a static pass to keep", REC_W_16 + FWD_16);
    g_cur = nullptr;
  }
  {  // a forward pass outside the fp16 form forgets the matrix: the products behind it do not read an older step's records
    Linear L;
    g_cur = &L;
    L.ensure(50, 16, 8, 7);
    L.forward(X, W, BIAS, Y, -1, S1, 0, nullptr);
    check("fp16 forward", REC_W_16 + FWD_16);
    g_x3_f16 = 0;
    L.forward(X, W, BIAS, Y, -1, S1, 0, nullptr);
    check("three-plane forward", FWD_X3);
    expect(L.am_w_of == nullptr, "a three-plane forward pass forgets the matrix");
    g_x3_f16 = 1;
    L.dgrad(G, W, GX, S1, 0, nullptr);
    check("dgrad behind a three-plane forward runs three-plane", DG_X3);
    L.wgrad(G, X, W, GW, GB, S2, 7);
    check("wgrad behind a three-plane forward takes the input's record itself", WG_16_OWN, "s2", 7);
    L.forward(X, W, BIAS, Y, -1, S1, 0, nullptr);
    check("fp16 forward again", REC_W_16 + FWD_16);
    L.wgrad(G, X, W, GW, GB, S2, 7);
    check("wgrad behind it borrows", WG_16_BORROW, "s2", 7);
    L.wgrad(G, X, W2, GW, GB, S2, 7);
    check("wgrad from another matrix does not", WG_16_OWN, "s2", 7);
    L.dgrad(G, W2, GX, S1, 0, nullptr);
    Table other = DG_X3;
    for (auto& l : other) l = subst(l, " W ", " W2 ");
    check("dgrad from another matrix runs three-plane", other);
    g_cur = nullptr;
  }
  {  // the forward product in fp32, the gradients split: the weights' record is taken for dgrad; wgrad has no input record to borrow
    g_eligible = 6;
    Linear L;
    g_cur = &L;
    L.ensure(50, 16, 8, 7);
    expect(L.xp.p == nullptr && L.gp.p && L.xpT.p && L.gpT.p, "planes for the split roles only");
    L.forward(X, W, BIAS, Y, -1, S1, 0, &fold);
    check("fp32 forward beside a split input gradient", REC_W_16 + FWD_F32, "s1", 0, true);
    L.dgrad(G, W, GX, S1, 0, nullptr);
    check("its dgrad", DG_16);
    L.wgrad(G, X, W, GW, GB, S2, 7);
    check("its wgrad", WG_16_OWN, "s2", 7);
    g_eligible = 7;
    g_cur = nullptr;
  }
  {  // the backward entry point: no forward pass, weight_record in its place; scratch for the requested roles only
    Linear L;
    g_cur = &L;
    const int before = mallocs;
    L.ensure(50, 16, 8, 2);
    expect(L.x_form == 2 && L.gp.p && L.am.p && !L.xp.p && !L.xpT.p && !L.gpT.p && mallocs - before == 2, "roles 2: the gradient's planes and the records");
    expect(L.gp.bytes == (size_t)3 * 50 * 8 * 2 && L.am.bytes == (size_t)5 * AMAX_REC * 4, "their sizes");
    L.weight_record(W, -1, S1);
    check("weight_record", REC_W_16);
    L.dgrad(G, W, GX, S1, 0, nullptr);
    check("the entry point's dgrad is fp16", DG_16);
    L.wgrad(G, X, W, nullptr, GB, S1, 0);
    check("the bias gradient alone", Table{"bias $S g 50 8 -> gb"});
    L.wgrad(G, X, W, GW, nullptr, S1, 0);
    check("a weight gradient whose role was not asked for runs fp32", Table{WG_F32[0]});
    g_cur = nullptr;
  }
  {
    Linear L;
    g_cur = &L;
    L.ensure(50, 16, 8, 6);
    expect(L.x_form == 6 && !L.xp.p && L.gp.p && L.xpT.p && L.gpT.p, "roles 6");
    expect(L.xpT.bytes == (size_t)3 * 16 * 64 * 2 && L.gpT.bytes == (size_t)3 * 8 * 64 * 2, "transposed planes are sized for the padded rows");
    L.weight_record(W, -1, S1);
    L.dgrad(G, W, GX, S1, 0, nullptr);
    L.wgrad(G, X, W, GW, GB, S1, 0);
    check("the backward entry point, everything asked for", REC_W_16 + DG_16 + WG_16_OWN);
    Linear F;
    g_cur = &F;
    F.ensure(50, 16, 8, 1);
    expect(F.x_form == 1 && F.xp.p && F.xp.bytes == (size_t)3 * 50 * 16 * 2 && !F.gp.p && !F.xpT.p && !F.gpT.p, "roles 1");
    F.forward(X, W, BIAS, Y, -1, S1, 0, nullptr);
    check("the forward entry point", REC_W_16 + FWD_16);
    Linear M(std::move(F));   // (a vector of layers moves them)
    g_cur = &M;
    expect(!F.xp.p && !F.am.p && M.xp.p && M.am_w_of == (f16 ? W : nullptr), "a moved layer keeps its planes and records");
    g_cur = nullptr;
  }
  expect(mallocs == frees && live_dev.empty(), "every device allocation freed exactly once");
  std::printf("linear_host_check: %d device buffers, %d failures\n", mallocs, bad);
  return bad ? 1 : 0;
}
