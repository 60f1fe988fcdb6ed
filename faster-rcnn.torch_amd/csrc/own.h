// own.h -- the handle-owning types of net.cpp: an event, a device buffer, a page-locked host buffer.  Each is move-only and
// gives its handle back in its destructor, so a model is destroyed by `delete` and a handle is destroyed exactly once.
// Included behind common.h: it uses FR_HIP and the runtime's declarations, and declares none of them itself (the host test
// tests/own_host_check.cpp compiles it against counting stand-ins).
#pragma once
#include <cstddef>

namespace frcnn {

// An ordering point between streams.  The handle is made by the first record(): an Event that was never recorded costs no
// runtime call, and wait() / sync() on it queue nothing -- there is nothing to wait for.
struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) { reset(); h = o.h; o.h = nullptr; }
    return *this;
  }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { reset(); }
  void reset() { if (h) (void)hipEventDestroy(h); h = nullptr; }
  bool recorded() const { return h != nullptr; }   // at least once
  int record(hipStream_t s) {
    if (!h) FR_HIP(hipEventCreateWithFlags(&h, hipEventDisableTiming));
    FR_HIP(hipEventRecord(h, s));
    return FRCNN_OK;
  }
  int wait(hipStream_t s) const {   // stream s waits for the last record
    if (h) FR_HIP(hipStreamWaitEvent(s, h, 0));
    return FRCNN_OK;
  }
  int sync() const {                // the host waits for the last record
    if (h) FR_HIP(hipEventSynchronize(h));
    return FRCNN_OK;
  }
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), owned(o.owned) { o.p = nullptr; o.bytes = 0; o.owned = true; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; owned = o.owned; o.p = nullptr; o.bytes = 0; o.owned = true; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void view(void* ptr, size_t n) { release(); p = ptr; bytes = n; owned = false; }  // slice of an arena: not freed here
  int ensure(size_t need) {
    if (need <= bytes) return FRCNN_OK;
    release();
    FR_HIP(hipMalloc(&p, need + 64));   // (64 bytes of slack: conv_wgradx's unaligned 16-byte segment loads may read 12 bytes past a tensor)
    bytes = need;
    return FRCNN_OK;
  }
  void release() { if (p && owned) (void)hipFree(p); p = nullptr; bytes = 0; owned = true; }
  float* f() const { return (float*)p; }
};

struct PinBuf {   // page-locked host memory
  char* p = nullptr;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  int alloc(size_t n) {
    release();
    FR_HIP(hipHostMalloc((void**)&p, n, hipHostMallocDefault));
    return FRCNN_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; }
};

}  // namespace frcnn
