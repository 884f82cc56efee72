// The host base of the run accumulators (br_collator, br_sorter, br_quant, br_coverage): objects that hold a whole run's data in
// one device's HBM through new -> set_param -> add... -> finish -> read out -> free.  The base holds the device, the object's
// stream and event and the count of the device bytes it holds; beside it, what more than one of them needs: the guard that drops
// a call's tables, a timer, the scans' scratch size, the scan with its total read back, the radix driver, the upload of a window of
// host rows, the growth of a record arena and the read-out of a table of 32-byte fields.  Host only.  (name_window.h: the front end of
// the adds that take read names.)
#pragma once
#include <algorithm>
#include <chrono>
#include <vector>

#include "collate_kernels.h"
#include "devmem.h"
#include "names.h"
#include "scan_kernels.h"

namespace br {

// a host row table's window [r0, r1) on the device: row r of the table is entry r - bias of a and cigar; the pool is whole (the
// CIGAR references are offsets from its start).  cigar and pool stay empty where the CIGARs are not asked for.
struct RowWindow {
  ColBuf a, cigar, pool;
  int64_t bias = 0;
  uint64_t n_pool_words = 0;
};

struct Accum {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev = nullptr;
  uint64_t live = 0, peak = 0;   // device bytes held by the object now / at most

  int open(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || dev < 0 || dev >= n) { (void)hipGetLastError(); return BR_ERR_NO_DEVICE; }
    HIPCHK(hipSetDevice(dev));
    device = dev;
    return hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? BR_OK : BR_ERR_HIP;
  }
  // what br_*_new does after the new: the device, and `words` zeroed counters
  int open(int dev, ColBuf &small, size_t words) {
    RC(open(dev)); RC(alloc(small, words * 8));
    return hipMemsetAsync(small.p, 0, words * 8, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess ? BR_OK : BR_ERR_HIP;
  }
  // what br_*_free does before the delete (an object that open refused has nothing to close)
  void close() {
    if (!st) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(st);
    if (ev) (void)hipEventDestroy(ev);
    (void)hipStreamDestroy(st);
    st = nullptr; ev = nullptr;
  }

  // b holds at least `bytes` (keep: with what it held).  The new buffer is made before the old one goes -- the old one beside the
  // new -- and the stream has finished with the old one by then; memory that is not there is BR_ERR_CAPACITY, not a HIP error
  int alloc(ColBuf &b, size_t bytes, bool keep = false) {
    if (bytes <= b.cap) return BR_OK;
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? BR_ERR_CAPACITY : BR_ERR_HIP; }
    live += bytes; peak = std::max(peak, live);
    if (keep && b.p) HIPCHK(hipMemcpyAsync(q, b.p, b.cap, hipMemcpyDeviceToDevice, st));
    if (b.p) { HIPCHK(hipStreamSynchronize(st)); live -= b.cap; b.release(); }
    b.p = q; b.cap = bytes;
    return BR_OK;
  }
  void drop(ColBuf &b) { live -= b.cap; b.release(); }

  // the stream's next work comes after whatever the caller's stream holds now (NULL: the null stream's work)
  int after(hipStream_t caller) {
    HIPCHK(hipEventRecord(ev, caller)); HIPCHK(hipStreamWaitEvent(st, ev, 0));
    return BR_OK;
  }

  // room for `bytes` more behind the `used` bytes of a record arena, which keeps ARENA_SLACK behind its end: it grows by half, with
  // what it held, and to no more than max_bytes (0: no cap but the device's memory)
  int grow_arena(ColBuf &arena, uint64_t used, uint64_t bytes, uint64_t max_bytes) {
    const uint64_t need = used + bytes;
    if (max_bytes && need > max_bytes) return BR_ERR_CAPACITY;
    if (need + ARENA_SLACK <= arena.cap) return BR_OK;
    uint64_t want = std::max<uint64_t>(need + ARENA_SLACK, arena.cap + arena.cap / 2);
    if (max_bytes) want = std::min<uint64_t>(want, max_bytes + ARENA_SLACK);
    return alloc(arena, (size_t)want, true);
  }

  // flag (n items, then one more) scanned in place; -> its total.  tmp: made scan_tmp_bytes(n) at least; the stream is done
  int scan_total(ColBuf &flag, int64_t n, ColBuf &tmp, uint64_t *total);

  // n fields of a table from item `first` on: 32 bytes each from the words that hold them in comparison order, and the lengths
  int fetch_fields(const ColBuf &words, const ColBuf &lens, int64_t first, int64_t n, uint8_t *out, uint8_t *len) {
    if (n == 0) return BR_OK;
    HIPCHK(hipSetDevice(device));
    std::vector<uint64_t> w;
    if (out) {
      w.resize((size_t)n * 4);
      HIPCHK(hipMemcpyAsync(w.data(), words.as<uint64_t>() + 4 * first, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    }
    if (len) HIPCHK(hipMemcpyAsync(len, lens.as<uint8_t>() + first, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out) for (size_t i = 0; i < (size_t)n * 32; i++) out[i] = (uint8_t)(w[i >> 3] >> (56 - 8 * (i & 7)));
    return BR_OK;
  }

  // a stable LSD radix sort of (key, idx) pairs over the digits in which the keys differ (bits: the OR and the AND of the keys);
  // tmp: scan_tmp_bytes(n) at least.  *cur = the buffer that holds the result; the stream is done when it returns
  int radix_sort(ColBuf key[2], ColBuf idx[2], int64_t n, const uint64_t bits[2], const ColBuf &tmp, int *cur);

  // rows' window [r0, r1) into w, whose buffers the caller holds under a DropGuard; the copies are on the stream, not waited for
  int upload_rows(const br_device_rows &rows, uint64_t r0, uint64_t r1, bool with_cigar, RowWindow &w) {
    const size_t n = (size_t)(r1 - r0), np = (size_t)rows.n_pool_words;
    RC(alloc(w.a, (n + 1) * sizeof(br_row_a)));
    if (n) HIPCHK(hipMemcpyAsync(w.a.p, rows.a + r0, n * sizeof(br_row_a), hipMemcpyHostToDevice, st));
    w.bias = (int64_t)r0;
    if (!with_cigar) return BR_OK;
    RC(alloc(w.cigar, (n + 1) * 8)); RC(alloc(w.pool, (np + 1) * 4));
    if (n) HIPCHK(hipMemcpyAsync(w.cigar.p, rows.cigar + r0, n * 8, hipMemcpyHostToDevice, st));
    if (np) HIPCHK(hipMemcpyAsync(w.pool.p, rows.pool, np * 4, hipMemcpyHostToDevice, st));
    w.n_pool_words = np;
    return BR_OK;
  }
};

// device tables of one call: whatever the outcome, they go (and leave the byte count) when the call returns.  What the call keeps
// is swapped out of them; dropping an empty buffer counts nothing
struct DropGuard {
  Accum *c; std::vector<ColBuf *> b;
  ~DropGuard() { for (auto *x : b) c->drop(*x); }
};

// adds the seconds it lives to *to (NULL: to nothing, the caller reads seconds())
struct ScopeTimer {
  double *to;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit ScopeTimer(double *to_ = nullptr) : to(to_) {}
  double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  ~ScopeTimer() { if (to) *to += seconds(); }
};

// scratch of the scans (over n + 1 items or the radix histograms: scan_kernels.h) and of the OR / AND reduction (2 words a
// block of 256)
inline size_t scan_tmp_bytes(int64_t n) {
  const int64_t blocks = (n + 255) / 256, nh = 256 * ((n + COL_TILE - 1) / COL_TILE);
  return (size_t)std::max<int64_t>(2 * blocks + 2, scan_tiles_for(std::max<int64_t>(nh, n + 1))) * 8;
}

inline int Accum::scan_total(ColBuf &flag, int64_t n, ColBuf &tmp, uint64_t *total) {
  RC(alloc(tmp, scan_tmp_bytes(n)));
  launch_scan(st, flag.as<uint64_t>(), n, tmp.as<uint64_t>());
  HIPCHK(hipMemcpyAsync(total, flag.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

// [first, first + n) lies within [0, total)
inline bool in_range(uint64_t total, int64_t first, int64_t n) {
  return first >= 0 && n >= 0 && (uint64_t)first <= total && (uint64_t)n <= total - (uint64_t)first;
}

inline int Accum::radix_sort(ColBuf key[2], ColBuf idx[2], int64_t n, const uint64_t bits[2], const ColBuf &tmp, int *cur) {
  ColBuf hist;   // 256 counts a tile of COL_TILE
  DropGuard dropper{this, {&hist}};
  RC(alloc(hist, (size_t)(256 * ((n + COL_TILE - 1) / COL_TILE) + 1) * 8));
  *cur = 0;
  for (int shift = 0; shift < 64; shift += 8) {
    if ((((bits[0] ^ bits[1]) >> shift) & 255u) == 0) continue;   // the digit is the same in every key
    launch_col_radix_pass(st, key[*cur].as<uint64_t>(), idx[*cur].as<uint32_t>(), key[*cur ^ 1].as<uint64_t>(), idx[*cur ^ 1].as<uint32_t>(),
                          n, shift, hist.as<uint64_t>(), tmp.as<uint64_t>());
    *cur ^= 1;
  }
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

}  // namespace br
