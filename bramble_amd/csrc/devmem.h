// Device and pinned host memory of the host units: growable buffers that free what they hold when they go (a context or a
// reader frees its buffers by being deleted).  They are move-only: a move hands the memory over (br_project_staged swaps
// two sets of row tables).
#pragma once
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <utility>

#include "../../include/bramble_amd.h"

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      fprintf(stderr, "[bramble_amd] HIP error %s at %s:%d: %s\n", hipGetErrorName(_e), __FILE__, \
              __LINE__, #expr);                                                               \
      return BR_ERR_HIP;                                                                      \
    }                                                                                         \
  } while (0)

#define RC(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// Large pinned host buffers: an anonymous mapping on transparent huge pages, touched, then registered -- 10-12 ms for 250 MB
// and the same for two threads at once, where hipHostMalloc takes 33-41 ms and 83-101 ms for the second of two concurrent
// calls (profiles/pin_probe.cpp: the command line's workers all pin their download buffers when their first bundles finish)
struct BigPinned {
  uint8_t *p = nullptr; size_t cap = 0; void *map = nullptr; size_t map_bytes = 0; bool registered = false;
  BigPinned() = default;
  BigPinned(BigPinned &&o) noexcept { *this = std::move(o); }
  BigPinned &operator=(BigPinned &&o) noexcept {
    std::swap(p, o.p); std::swap(cap, o.cap); std::swap(map, o.map); std::swap(map_bytes, o.map_bytes); std::swap(registered, o.registered);
    return *this;
  }
  ~BigPinned() { release(); }
  int alloc(size_t bytes) {
    release();
    const size_t huge = (size_t)2 << 20;
    map_bytes = ((bytes + huge - 1) & ~(huge - 1)) + huge;
    map = mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (map == MAP_FAILED) { map = nullptr; map_bytes = 0; return BR_ERR_CAPACITY; }
    p = (uint8_t *)(((uintptr_t)map + huge - 1) & ~(uintptr_t)(huge - 1));
    const size_t span = (bytes + huge - 1) & ~(huge - 1);
    (void)madvise(p, span, MADV_HUGEPAGE);
    for (size_t i = 0; i < span; i += 4096) p[i] = 0;
    if (hipHostRegister(p, span, hipHostRegisterDefault) != hipSuccess) {   // (no registration: the plain way)
      (void)hipGetLastError();
      munmap(map, map_bytes); map = nullptr; map_bytes = 0; p = nullptr;
      HIPCHK(hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
      registered = false; cap = bytes;
      return BR_OK;
    }
    registered = true; cap = span;
    return BR_OK;
  }
  void release() {
    if (p && registered) { (void)hipHostUnregister(p); munmap(map, map_bytes); }
    else if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0; map = nullptr; map_bytes = 0; registered = false;
  }
};

struct DevBuf {
  void *p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return BR_OK;
    if (p) { HIPCHK(hipFree(p)); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    return BR_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T *as() { return (T *)p; }
};

// an exactly sized device buffer (the collator's and the sorter's arenas and tables: their owners count the bytes and turn a
// failed allocation into BR_ERR_CAPACITY -- the records do not fit -- instead of a HIP error)
struct ColBuf {
  void *p = nullptr; size_t cap = 0;
  ColBuf() = default;
  ColBuf(ColBuf &&o) noexcept { *this = std::move(o); }
  ColBuf &operator=(ColBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~ColBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T *as() const { return (T *)p; }
};

// growable pinned host array (contents are not preserved across growth: every call rewrites it)
// (large ones on huge pages, registered: BigPinned; small ones from hipHostMalloc)
template <typename T>
struct PinnedVec {
  T *p = nullptr; size_t n = 0, cap = 0; BigPinned big;
  PinnedVec() = default;
  PinnedVec(PinnedVec &&o) noexcept { *this = std::move(o); }
  PinnedVec &operator=(PinnedVec &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); std::swap(big, o.big); return *this; }
  ~PinnedVec() { release(); }
  int resize(size_t m) {
    if (m > cap) {
      release();
      size_t want = m + m / 4 + 64;
      if (want * sizeof(T) >= ((size_t)4 << 20)) { const int brc = big.alloc(want * sizeof(T)); if (brc) return brc; p = (T *)big.p; }
      else HIPCHK(hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault));
      cap = want;
    }
    n = m;
    return BR_OK;
  }
  T *data() { return p; }
  void release() { if (big.p) big.release(); else if (p) (void)hipHostFree(p); p = nullptr; n = cap = 0; }
};
