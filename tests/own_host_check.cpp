// Host check of csrc/own.h (Event, DevBuf, PinBuf) without a GPU: the runtime calls the header makes are replaced by the
// counting stand-ins below, which also catch a handle given back twice or never.  Built with -fsanitize=address,undefined and
// run by tests/test_own_host.py; exits 0 when every created handle was destroyed exactly once and every allocation freed
// exactly once.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

// ---- stand-ins for what own.h expects from common.h and the HIP runtime ------------------------------------------------
typedef int hipError_t;
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipStream_t* hipStream_t;
enum { hipSuccess = 0, hipEventDisableTiming = 2, hipHostMallocDefault = 0 };
enum { FRCNN_OK = 0, FRCNN_ERR_HIP = 2 };

static std::set<void*> live_events, live_dev, live_pin;
static int created = 0, destroyed = 0, mallocs = 0, frees = 0, pins = 0, unpins = 0, records = 0, waits = 0, syncs = 0, bad = 0;
static bool fail_next_malloc = false;

static void expect(bool ok, const char* what) {
  if (!ok) { std::fprintf(stderr, "own_host_check: %s\n", what); ++bad; }
}
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  expect(flags == hipEventDisableTiming, "an event created with timing");
  *e = (hipEvent_t)std::malloc(1);
  live_events.insert(*e); ++created;
  return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
  expect(live_events.erase(e) == 1, "hipEventDestroy of a handle that is not live");
  std::free(e); ++destroyed;
  return hipSuccess;
}
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { expect(live_events.count(e) == 1, "record on a dead event"); ++records; return hipSuccess; }
static hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned) { expect(live_events.count(e) == 1, "wait on a dead event"); ++waits; return hipSuccess; }
static hipError_t hipEventSynchronize(hipEvent_t e) { expect(live_events.count(e) == 1, "synchronize on a dead event"); ++syncs; return hipSuccess; }
static hipError_t hipMalloc(void** p, size_t n) {
  if (fail_next_malloc) { fail_next_malloc = false; *p = nullptr; return 1; }
  *p = std::malloc(n);
  live_dev.insert(*p); ++mallocs;
  return hipSuccess;
}
static hipError_t hipFree(void* p) {
  expect(live_dev.erase(p) == 1, "hipFree of a pointer that is not a live allocation");
  std::free(p); ++frees;
  return hipSuccess;
}
static hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = std::malloc(n); live_pin.insert(*p); ++pins; return hipSuccess; }
static hipError_t hipHostFree(void* p) {
  expect(live_pin.erase(p) == 1, "hipHostFree of a pointer that is not a live allocation");
  std::free(p); ++unpins;
  return hipSuccess;
}
#define FR_HIP(expr) do { if ((expr) != hipSuccess) return FRCNN_ERR_HIP; } while (0)

#include "../faster-rcnn.torch_amd/csrc/own.h"
using namespace frcnn;

// a model in small: the member kinds of frcnn_model, destroyed by `delete` in reverse order of declaration
struct Holder {
  DevBuf arena, slice;          // (slice views arena and is destroyed first)
  std::vector<DevBuf> bufs;
  Event ring[4];
  std::vector<Event> per_block;
  PinBuf pin;
};

int main() {
  hipStream_t s = nullptr, t = (hipStream_t)&bad;
  {  // Event: lazy creation, no-op waits, move, reset, double reset
    Event e;
    expect(!e.recorded() && e.wait(s) == FRCNN_OK && e.sync() == FRCNN_OK, "a fresh event");
    expect(created == 0 && waits == 0 && syncs == 0, "a never-recorded event made a runtime call");
    expect(e.record(s) == FRCNN_OK && e.record(t) == FRCNN_OK && created == 1 && records == 2, "record creates once");
    expect(e.wait(t) == FRCNN_OK && e.sync() == FRCNN_OK && waits == 1 && syncs == 1, "wait / sync after a record");
    Event f(std::move(e));
    expect(!e.recorded() && f.recorded() && e.wait(s) == FRCNN_OK && waits == 1, "moved-from event is empty");
    Event g;
    g.record(s);
    g = std::move(f);             // g's own handle is destroyed here
    expect(destroyed == 1 && g.recorded() && !f.recorded(), "move assignment destroys the target's handle");
    g = std::move(g);             // self-move keeps the handle
    expect(g.recorded() && destroyed == 1, "self move");
    g.reset(); g.reset();
    expect(destroyed == 2 && !g.recorded() && g.wait(s) == FRCNN_OK && waits == 1, "reset, twice");
    g.record(s);                  // usable again after reset; destroyed by the destructor
  }
  expect(created == 3 && destroyed == 3 && live_events.empty(), "events after the first scope");
  {  // a vector of events: sized without a runtime call, grown (elements move), shrunk
    std::vector<Event> v(3);
    expect(created == 3, "sizing a vector of events made a runtime call");
    v[1].record(s);
    for (int i = 0; i < 40; ++i) v.emplace_back();   // reallocation moves the recorded one
    expect(v[1].recorded() && created == 4 && destroyed == 3, "reallocation moved the handle");
    v[20].record(s);
    v.resize(2);
    expect(destroyed == 4, "shrinking destroys the dropped element's handle");
    Event ring[4];
    ring[0].record(s); ring[2].record(s);
    for (auto& e : ring) e.reset();                   // the re-allocation of the ring of tables
    expect(destroyed == 6 && !ring[0].recorded() && ring[0].sync() == FRCNN_OK, "ring reset");
    ring[0].record(s);
  }
  expect(created == 8 && destroyed == 8 && live_events.empty(), "events after the vector scope");
  {  // DevBuf: ensure, growth, view, ensure after view, move, failed allocation
    DevBuf a;
    expect(a.ensure(100) == FRCNN_OK && mallocs == 1 && a.bytes == 100, "ensure");
    void* p0 = a.p;
    expect(a.ensure(50) == FRCNN_OK && a.p == p0 && mallocs == 1, "ensure of less keeps the buffer");
    expect(a.ensure(200) == FRCNN_OK && mallocs == 2 && frees == 1, "growth frees the old buffer");
    DevBuf v;
    v.view(a.p, 64);
    expect(!v.owned && v.p == a.p, "view");
    v.view((char*)a.p + 64, 64);                      // re-viewed: nothing freed
    expect(frees == 1, "view freed something");
    expect(v.ensure(32) == FRCNN_OK && mallocs == 2, "ensure within a view keeps it");
    expect(v.ensure(500) == FRCNN_OK && v.owned && mallocs == 3 && frees == 1 && live_dev.count(a.p) == 1, "ensure after view allocates and leaves the arena alone");
    DevBuf w;
    w.view(a.p, 16);
    DevBuf b(std::move(a));
    expect(a.p == nullptr && a.bytes == 0 && b.bytes == 200, "move construction");
    a = std::move(b);
    expect(b.p == nullptr && a.bytes == 200 && frees == 1, "move assignment");
    DevBuf c;
    c.ensure(10);
    c = std::move(v);                                 // c's own buffer is freed
    expect(frees == 2 && c.bytes == 500, "move assignment frees the target's buffer");
    fail_next_malloc = true;
    expect(c.ensure(1000) == FRCNN_ERR_HIP && c.p == nullptr && c.bytes == 0 && frees == 3, "failed allocation leaves an empty buffer");
    c.release(); c.release();
    std::vector<DevBuf> vec;
    for (int i = 0; i < 20; ++i) { DevBuf d; d.ensure(8 + i); vec.push_back(std::move(d)); }
    // w (a view) and a (its arena) die in either order without a double free
  }
  expect(mallocs == frees && live_dev.empty(), "device allocations after the DevBuf scope");
  {  // PinBuf
    PinBuf p;
    expect(p.alloc(64) == FRCNN_OK && p.alloc(128) == FRCNN_OK && pins == 2 && unpins == 1, "re-allocation frees the old ring");
    p.release(); p.release();
    p.alloc(16);
  }
  expect(pins == unpins && live_pin.empty(), "pinned allocations");
  {  // destruction order of a whole model
    Holder* h = new Holder();
    h->arena.ensure(1024);
    h->slice.view(h->arena.p, 256);
    h->bufs.resize(5);
    for (auto& b : h->bufs) b.ensure(33);
    h->per_block.resize(4);
    h->per_block[2].record(s);
    h->ring[1].record(s);
    h->pin.alloc(99);
    delete h;
    Holder* never_used = new Holder();                // create and destroy without a pass: no runtime call at all
    const int calls = created + mallocs + pins;
    never_used->per_block.resize(4);
    delete never_used;
    expect(calls == created + mallocs + pins, "an unused model made a runtime call");
  }
  expect(created == destroyed && live_events.empty(), "every event destroyed exactly once");
  expect(mallocs == frees && live_dev.empty(), "every device allocation freed exactly once");
  expect(pins == unpins && live_pin.empty(), "every pinned allocation freed exactly once");
  std::printf("own_host_check: %d events, %d device buffers, %d pinned buffers, %d failures\n", created, mallocs, pins, bad);
  return bad ? 1 : 0;
}
