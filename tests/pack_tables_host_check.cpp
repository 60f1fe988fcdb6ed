// Host check of csrc/pack_tables.h (PackTables: which weight tensor gets which pack job, and the named spans of the three job
// tables that the passes launch from) without a GPU.  The job constructors, the three block-assignment functions and the runtime
// calls are replaced by the stand-ins below: a job records the arguments it was made from, an assignment records the list and
// the budget it was given and deals blocks by a rule that depends on the whole list.  The expected content of every span is a
// literal list of (tensor, mode) pairs further down, written out by hand from the rules -- never produced by the code under test.
// Built with -fsanitize=address,undefined and run by tests/test_pack_tables_host.py; exits 0 when every span matched.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

// ---- stand-ins for what pack_tables.h and own.h expect from common.h, kernels.h and the HIP runtime -----------------------
typedef int hipError_t;
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
enum { hipSuccess = 0, hipEventDisableTiming = 2, hipHostMallocDefault = 0, hipMemcpyHostToDevice = 1 };
enum { FRCNN_OK = 0, FRCNN_ERR_ARG = 1, FRCNN_ERR_HIP = 2 };
#define AMAX_REC 16400
#define FR_HIP(expr) do { if ((expr) != hipSuccess) return FRCNN_ERR_HIP; } while (0)
#define FR_TRY(expr) do { int r_ = (expr); if (r_ != FRCNN_OK) return r_; } while (0)
#define FR_CHECK(cond, ...) do { if (!(cond)) return FRCNN_ERR_ARG; } while (0)

static int bad = 0;
static void expect(bool ok, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void expect(bool ok, const char* fmt, ...) {
  if (ok) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  std::fprintf(stderr, "pack_tables_host_check: %s\n", buf);
  ++bad;
}
static std::set<void*> live_dev;
static std::map<void*, size_t> uploaded;   // bytes of the last copy to each device buffer
static int mallocs = 0, frees = 0, copies = 0;
static hipError_t hipMalloc(void** p, size_t n) { *p = std::malloc(n); live_dev.insert(*p); ++mallocs; return hipSuccess; }
static hipError_t hipFree(void* p) {
  expect(live_dev.erase(p) == 1, "hipFree of a pointer that is not a live allocation");
  uploaded.erase(p);
  std::free(p); ++frees;
  return hipSuccess;
}
static hipError_t hipMemcpy(void* dst, const void* src, size_t n, int) {
  expect(live_dev.count(dst) == 1 && n > 0, "hipMemcpy: %zu bytes to a pointer that is no device buffer", n);
  std::memcpy(dst, src, n); uploaded[dst] = n; ++copies;
  return hipSuccess;
}
static hipError_t hipEventCreateWithFlags(hipEvent_t*, unsigned) { return hipSuccess; }   // (own.h's Event and PinBuf: not used here)
static hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = std::malloc(n); return hipSuccess; }
static hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }

#include "../faster-rcnn.torch_amd/csrc/own.h"

static int g_x3_f16 = 1;
static int get_x3_f16() { return g_x3_f16; }

// the jobs: what they were made from, and the block fields
struct PackJob {
  long w_off; float* dst; int O, C, k, mode, blk_begin, nblk;
  bool operator==(const PackJob& o) const {
    return w_off == o.w_off && dst == o.dst && O == o.O && C == o.C && k == o.k && mode == o.mode && blk_begin == o.blk_begin && nblk == o.nblk;
  }
};
struct AmaxJob {
  long off; long n; float* out; int blk_begin;
  bool operator==(const AmaxJob& o) const { return off == o.off && n == o.n && out == o.out && blk_begin == o.blk_begin; }
};
struct PackXJob {
  long w_off; void* dst; const float* amax; float* amax_w; int O, C, k, mode, Ho, Wo, blk_begin, nblk;
  bool operator==(const PackXJob& o) const {
    return w_off == o.w_off && dst == o.dst && amax == o.amax && amax_w == o.amax_w && O == o.O && C == o.C && k == o.k && mode == o.mode &&
           Ho == o.Ho && Wo == o.Wo && blk_begin == o.blk_begin && nblk == o.nblk;
  }
};
static int made_pack = 0, made_x3 = 0;   // constructor calls
static PackJob conv_pack_job(long w_off, int O, int C, int k, int mode, float* dst) {
  ++made_pack;
  return PackJob{w_off, dst, O, C, k, mode, 0, 1};
}
static PackXJob conv_x3_pack_job(long w_off, int O, int C, int k, int mode, void* dst, int Ho, int Wo) {
  ++made_x3;
  return PackXJob{w_off, dst, nullptr, nullptr, O, C, k, mode, Ho, Wo, 0, 1};
}

// tensor i of a model sits at offset 1000 (i + 1) of the flat vector
static int tensor_of(long w_off) { return (int)(w_off / 1000) - 1; }
typedef std::vector<std::pair<int, int>> Ids;   // (tensor, mode)
struct AssignCall { char kind; int budget; Ids ids; };
static std::vector<AssignCall> g_calls;
static bool g_log_calls = true;
static int conv_pack_assign_blocks(PackJob* j, int n, int total) {
  if (g_log_calls) { AssignCall c{'p', total, {}}; for (int i = 0; i < n; ++i) c.ids.push_back({tensor_of(j[i].w_off), j[i].mode}); g_calls.push_back(c); }
  int b = 0;
  for (int i = 0; i < n; ++i) { j[i].blk_begin = b; j[i].nblk = 1 + n + tensor_of(j[i].w_off) + total / 512; b += j[i].nblk; }
  return b;
}
static const long AMAX_TOO_LARGE = 1L << 40;
static int tensor_absmax_assign_blocks(AmaxJob* j, int n) {
  if (g_log_calls) { AssignCall c{'a', 0, {}}; for (int i = 0; i < n; ++i) c.ids.push_back({tensor_of(j[i].off), 0}); g_calls.push_back(c); }
  int b = 0;
  for (int i = 0; i < n; ++i) {
    if (j[i].n >= AMAX_TOO_LARGE) return -1;
    j[i].blk_begin = b; b += 1 + n + tensor_of(j[i].off);
  }
  return b;
}
static int conv_x3_pack_assign_blocks(PackXJob* j, int n) {
  if (g_log_calls) { AssignCall c{'x', 0, {}}; for (int i = 0; i < n; ++i) c.ids.push_back({tensor_of(j[i].w_off), j[i].mode}); g_calls.push_back(c); }
  int b = 0;
  for (int i = 0; i < n; ++i) { j[i].blk_begin = b; j[i].nblk = 2 + n + tensor_of(j[i].w_off) + j[i].mode; b += j[i].nblk; }
  return b;
}

#include "../faster-rcnn.torch_amd/csrc/pack_tables.h"
using namespace frcnn;

// ---- the models -------------------------------------------------------------------------------------------------------------
static float WF[8], WD[8], WS[32];
static char WX[8], WXD[8];
static std::vector<float> REC((size_t)32 * AMAX_REC);
static std::vector<PackTensor> g_model;   // the model under test, as handed to build()

// tensor i: shapes and buffers that tell every argument of a constructor apart
static PackTensor tensor(int i, PackTensor::Kind kind, int group, int conv, int am, bool first, bool x_f, bool x_d) {
  PackTensor t;
  t.kind = kind; t.group = group; t.conv = conv; t.am = am; t.first = first; t.x_f = x_f; t.x_d = x_d;
  t.w_off = 1000L * (i + 1); t.Cout = 8 + i; t.Cin = 4 + i; t.k = 3;
  t.H = 20 + i; t.W = 30 + i; t.Ho = 40 + i; t.Wo = 50 + i;
  t.wf = &WF[i]; t.wd = &WD[i]; t.wx = &WX[i]; t.wxd = &WXD[i];
  return t;
}

// the jobs a (tensor, mode) list stands for, made by hand from the model, with blocks assigned on that list alone
static std::vector<PackJob> want_pack(const Ids& ids, int budget, int* grid) {
  std::vector<PackJob> r;
  for (auto& id : ids) {
    const PackTensor& t = g_model[id.first];
    r.push_back(PackJob{t.w_off, id.second ? t.wd : t.wf, t.Cout, t.Cin, t.k, id.second, 0, 1});
  }
  *grid = r.empty() ? 0 : conv_pack_assign_blocks(r.data(), (int)r.size(), budget);
  return r;
}
static std::vector<AmaxJob> want_amax(const Ids& ids, int* grid) {
  std::vector<AmaxJob> r;
  for (auto& id : ids) {
    const PackTensor& t = g_model[id.first];
    r.push_back(AmaxJob{t.w_off, (long)t.Cout * t.Cin * t.k * t.k, REC.data() + (size_t)(t.am + 2) * AMAX_REC, 0});
  }
  *grid = r.empty() ? 0 : tensor_absmax_assign_blocks(r.data(), (int)r.size());
  return r;
}
static std::vector<PackXJob> want_x3(const Ids& ids, bool twin, int* grid) {
  std::vector<PackXJob> r;
  for (auto& id : ids) {
    const PackTensor& t = g_model[id.first];
    PackXJob j = id.second ? PackXJob{t.w_off, t.wxd, nullptr, nullptr, t.Cout, t.Cin, t.k, 1, t.H, t.W, 0, 1}
                           : PackXJob{t.w_off, t.wx, nullptr, nullptr, t.Cout, t.Cin, t.k, 0, t.Ho, t.Wo, 0, 1};
    if (twin) { j.amax = REC.data() + (size_t)(t.am + 2) * AMAX_REC; j.amax_w = WS + t.am; }
    r.push_back(j);
  }
  *grid = r.empty() ? 0 : conv_x3_pack_assign_blocks(r.data(), (int)r.size());
  return r;
}

// build() made exactly one assignment call for this list, with this budget (none for an empty list)
static void check_call(const char* what, char kind, const Ids& ids, int budget) {
  int n = 0;
  for (auto& c : g_calls) if (c.kind == kind && c.ids == ids && c.budget == budget) ++n;
  if (!ids.empty()) expect(n >= 1, "%s: no block assignment on this list with budget %d", what, budget);
}

template <class Job>
static void check_span(const char* what, const JobTable<Job>& T, const Span& sp, const std::vector<Job>& want, int grid) {
  expect(sp.n == (int)want.size(), "%s: %d jobs, expected %zu", what, sp.n, want.size());
  expect(sp.grid == grid, "%s: grid %d, expected %d", what, sp.grid, grid);
  expect(sp.off >= 0 && (size_t)sp.off + sp.n <= T.host.size(), "%s: span [%d, %d) outside a table of %zu jobs", what, sp.off, sp.off + sp.n, T.host.size());
  if (sp.n != (int)want.size() || (size_t)sp.off + sp.n > T.host.size()) return;
  // span to device pointer: inside what was uploaded, and the same jobs there
  const size_t up = T.dev.p && uploaded.count(T.dev.p) ? uploaded[T.dev.p] : 0;
  expect(up == T.host.size() * sizeof(Job), "%s: %zu bytes uploaded for a table of %zu jobs", what, up, T.host.size());
  if (sp.n) expect(T.at(sp) >= (const Job*)T.dev.p && (const char*)(T.at(sp) + sp.n) <= (const char*)T.dev.p + up, "%s: device pointer outside the uploaded table", what);
  for (int i = 0; i < sp.n; ++i) {
    expect(T.host_at(sp)[i] == want[i], "%s: job %d differs (host)", what, i);
    if (up == T.host.size() * sizeof(Job)) expect(T.at(sp)[i] == want[i], "%s: job %d differs (device)", what, i);
  }
}
static void check_pack(const char* what, const PackTables& P, const Span& sp, const Ids& ids, int budget) {
  g_log_calls = false;
  int grid;
  std::vector<PackJob> want = want_pack(ids, budget, &grid);
  g_log_calls = true;
  check_span(what, P.pack, sp, want, grid);
  check_call(what, 'p', ids, budget);
}
static void check_amax(const char* what, const PackTables& P, const Span& sp, const std::vector<int>& tensors) {
  Ids ids;
  for (int t : tensors) ids.push_back({t, 0});
  g_log_calls = false;
  int grid;
  std::vector<AmaxJob> want = want_amax(ids, &grid);
  g_log_calls = true;
  check_span(what, P.amax, sp, want, grid);
  check_call(what, 'a', ids, 0);
}
static void check_x3(const char* what, const PackTables& P, const Span* sp, const Ids& ids) {   // sp[0] plain, sp[1] the fp16 twin
  g_log_calls = false;
  int grid, grid16;
  std::vector<PackXJob> want = want_x3(ids, false, &grid), want16 = want_x3(ids, true, &grid16);
  g_log_calls = true;
  check_span(what, P.x3, sp[0], want, grid);
  check_span(what, P.x3, sp[1], want16, grid16);
  check_call(what, 'x', ids, 0);
  int n = 0;   // blocks are assigned on the twin separately
  for (auto& c : g_calls) if (c.kind == 'x' && c.ids == ids) ++n;
  if (!ids.empty()) expect(n >= 2, "%s: the twin had no block assignment of its own", what);
  if (sp[0].n != sp[1].n || (size_t)sp[1].off + sp[1].n > P.x3.host.size()) return;
  for (int i = 0; i < sp[0].n; ++i) {   // the twin is the plain job with the weight magnitude attached, nothing else
    PackXJob a = P.x3.host_at(sp[0])[i], b = P.x3.host_at(sp[1])[i];
    expect(a.amax == nullptr && a.amax_w == nullptr && b.amax != nullptr && b.amax_w != nullptr, "%s: job %d: magnitude pointers", what, i);
    b.amax = nullptr; b.amax_w = nullptr;
    expect(a == b, "%s: job %d: the twin differs in more than its magnitude pointers", what, i);
  }
}

struct Expected {
  Ids pk_train, pk_fwd, pk_heads, pk_bb;
  std::vector<int> am_all, am_bb;
  Ids x3_train, x3_fwd;
  std::vector<int> x3_conv;
  std::vector<Ids> g_pk;
  std::vector<std::vector<int>> g_am;
  std::vector<Ids> g_x3;
  int made_pack, made_x3;   // distinct jobs: each is constructed once
  int tables;               // non-empty tables: device buffers and uploads
};

static void run(const char* name, std::vector<PackTensor> model, int nblocks, const Expected& e) {
  char what[128];
  g_model = model;
  g_calls.clear();
  made_pack = made_x3 = 0;
  const int mallocs0 = mallocs, copies0 = copies;
  {
    PackTables P;
    expect(P.build(model, nblocks, REC.data(), WS) == FRCNN_OK, "%s: build", name);
    expect(mallocs == mallocs0 && copies == copies0, "%s: build uploads nothing", name);
    expect(P.upload() == FRCNN_OK, "%s: upload", name);
    expect(mallocs - mallocs0 == e.tables && copies - copies0 == e.tables, "%s: %d buffers, %d copies for %d non-empty tables", name,
           mallocs - mallocs0, copies - copies0, e.tables);
    expect(made_pack == e.made_pack && made_x3 == e.made_x3, "%s: %d PackJob and %d PackXJob constructor calls, expected %d and %d", name,
           made_pack, made_x3, e.made_pack, e.made_x3);
    for (auto& c : g_calls) expect(!c.ids.empty(), "%s: a block assignment on an empty list", name);
#define WHAT(s) (std::snprintf(what, sizeof(what), "%s: %s", name, s), what)
    check_pack(WHAT("pack / train"), P, P.pk_train, e.pk_train, 2048);
    check_pack(WHAT("pack / forward-only"), P, P.pk_fwd, e.pk_fwd, 2048);
    check_pack(WHAT("pack / heads' input-gradient"), P, P.pk_heads, e.pk_heads, 2048);
    check_pack(WHAT("pack / backbone-only"), P, P.pk_bb, e.pk_bb, 512);
    check_amax(WHAT("magnitude / all"), P, P.am_all, e.am_all);
    check_amax(WHAT("magnitude / backbone-only"), P, P.am_bb, e.am_bb);
    check_x3(WHAT("split-operand / train"), P, P.x3_train, e.x3_train);
    check_x3(WHAT("split-operand / forward-only"), P, P.x3_fwd, e.x3_fwd);
    expect(P.x3_conv == e.x3_conv, "%s: x3_conv", name);
    expect((int)P.groups.size() == nblocks + 1, "%s: %zu groups", name, P.groups.size());
    for (int g = 0; g <= nblocks && g < (int)P.groups.size(); ++g) {
      char s[64];
      std::snprintf(s, sizeof(s), "group %d pack", g);
      check_pack(WHAT(s), P, P.groups[g].pk, e.g_pk[g], 512);
      std::snprintf(s, sizeof(s), "group %d magnitude", g);
      check_amax(WHAT(s), P, P.groups[g].am, e.g_am[g]);
      std::snprintf(s, sizeof(s), "group %d split-operand", g);
      check_x3(WHAT(s), P, P.groups[g].x3, e.g_x3[g]);
    }
#undef WHAT
    g_x3_f16 = 1; expect(P.f16() == !e.am_all.empty(), "%s: the fp16 form needs the option and a magnitude job", name);
    g_x3_f16 = 0; expect(!P.f16(), "%s: no fp16 form with the option off", name);
    g_x3_f16 = 1;
    int live = 0;   // has_record is the magnitude table's test
    for (auto& t : P.tensors) live += t.has_record();
    expect(live == (int)e.am_all.size(), "%s: has_record holds for %d tensors, the magnitude table has %zu", name, live, e.am_all.size());
    // a change of shape builds the tables again: nothing is left of the first build
    const size_t n_pk = P.pack.host.size(), n_am = P.amax.host.size(), n_x3 = P.x3.host.size();
    expect(P.build(model, nblocks, REC.data(), WS) == FRCNN_OK && P.upload() == FRCNN_OK, "%s: second build", name);
    expect(P.pack.host.size() == n_pk && P.amax.host.size() == n_am && P.x3.host.size() == n_x3 && P.x3_conv == e.x3_conv, "%s: a second build repeats the first", name);
    expect(mallocs - mallocs0 == e.tables, "%s: a second build of the same size allocates nothing", name);
    check_pack("second build: pack / train", P, P.pk_train, e.pk_train, 2048);
  }
  expect(mallocs == frees && live_dev.empty(), "%s: every device buffer freed exactly once", name);
}

int main() {
  const PackTensor::Kind BB = PackTensor::BACKBONE, C3 = PackTensor::HEAD_C3, C1 = PackTensor::HEAD_C1;
  {  // (a) 2 blocks of 2 convolutions, 2 anchor nets (on block 1 and block 2; group 2 owns both).
     //   0: the first convolution, x_f      1: neither      2: x_d only      3: both      4: c3, eligible   5: its c1
     //   6: c3, not eligible   7: its c1
    std::vector<PackTensor> m = {
        tensor(0, BB, 0, 0, 0, true, true, false),  tensor(1, BB, 0, 1, 3, false, false, false),
        tensor(2, BB, 1, 2, 6, false, false, true), tensor(3, BB, 1, 3, 9, false, true, true),
        tensor(4, C3, 2, -1, 12, false, true, false), tensor(5, C1, 2, -1, -1, false, false, false),
        tensor(6, C3, 2, -1, 15, false, false, false), tensor(7, C1, 2, -1, -1, false, false, false)};
    Expected e;
    e.pk_train = {{1, 0}, {2, 0}, {5, 0}, {6, 0}, {7, 0}, {1, 1}};
    e.pk_fwd = {{1, 0}, {2, 0}, {5, 0}, {6, 0}, {7, 0}};
    e.pk_heads = {{4, 1}, {5, 1}, {6, 1}, {7, 1}};
    e.pk_bb = {{1, 0}, {1, 1}, {2, 0}};
    e.am_all = {0, 2, 3, 4};
    e.am_bb = {0, 2, 3};
    e.x3_train = {{0, 0}, {2, 1}, {3, 0}, {3, 1}, {4, 0}};
    e.x3_fwd = {{0, 0}, {3, 0}, {4, 0}};
    e.x3_conv = {0, 2, 3, 3, -1};
    e.g_pk = {{{1, 0}, {1, 1}}, {{2, 0}}, {{5, 0}, {6, 0}, {7, 0}}};
    e.g_am = {{0}, {2, 3}, {4}};
    e.g_x3 = {{{0, 0}}, {{2, 1}, {3, 0}, {3, 1}}, {{4, 0}}};
    e.made_pack = 10; e.made_x3 = 5; e.tables = 3;
    run("model a", m, 2, e);
  }
  {  // (b) 1 block of 1 convolution, no anchor nets: the heads' span and the last group are empty
    Expected e;
    e.pk_train = {{0, 0}}; e.pk_fwd = {{0, 0}}; e.pk_bb = {{0, 0}};
    e.g_pk = {{{0, 0}}, {}}; e.g_am = {{}, {}}; e.g_x3 = {{}, {}};
    e.made_pack = 1; e.made_x3 = 0; e.tables = 1;
    run("model b", {tensor(0, BB, 0, 0, 0, true, false, false)}, 1, e);
    // ... the same with its convolution in the split form: no fp32 pack at all
    Expected s;
    s.am_all = {0}; s.am_bb = {0};
    s.x3_train = {{0, 0}}; s.x3_fwd = {{0, 0}}; s.x3_conv = {0};
    s.g_pk = {{}, {}}; s.g_am = {{0}, {}}; s.g_x3 = {{{0, 0}}, {}};
    s.made_pack = 0; s.made_x3 = 1; s.tables = 2;
    run("model b, split", {tensor(0, BB, 0, 0, 0, true, true, false)}, 1, s);
  }
  {  // (c) no tensor is eligible: 2 blocks of 1 convolution, 1 anchor net.  No magnitude and no split-operand table.
    std::vector<PackTensor> m = {tensor(0, BB, 0, 0, 0, true, false, false), tensor(1, BB, 1, 1, 3, false, false, false),
                                 tensor(2, C3, 2, -1, 6, false, false, false), tensor(3, C1, 2, -1, -1, false, false, false)};
    Expected e;
    e.pk_train = {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {1, 1}};
    e.pk_fwd = {{0, 0}, {1, 0}, {2, 0}, {3, 0}};
    e.pk_heads = {{2, 1}, {3, 1}};
    e.pk_bb = {{0, 0}, {1, 0}, {1, 1}};
    e.g_pk = {{{0, 0}}, {{1, 0}, {1, 1}}, {{2, 0}, {3, 0}}};
    e.g_am = {{}, {}, {}}; e.g_x3 = {{}, {}, {}};
    e.made_pack = 7; e.made_x3 = 0; e.tables = 1;
    run("model c", m, 2, e);
  }
  {  // a weight tensor too large for its magnitude record stays an error
    PackTensor t = tensor(0, BB, 0, 0, 0, true, true, false);
    t.Cout = 1 << 20; t.Cin = 1 << 20;
    PackTables P;
    expect(P.build({t}, 1, REC.data(), WS) == FRCNN_ERR_ARG, "a negative grid of the magnitude assignment is an error");
  }
  expect(mallocs == frees && live_dev.empty(), "every device buffer freed exactly once");
  std::printf("pack_tables_host_check: %d device buffers, %d failures\n", mallocs, bad);
  return bad ? 1 : 0;
}
