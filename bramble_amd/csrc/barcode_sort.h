// The (group, length, bytes) order of 32-byte fields, shared by the cells (cells.cpp), the whitelist (whitelist.cpp) and br_dedup
// (dedup.cpp): key / index pairs of the accumulators' radix driver, the sort of one key over the digits in which the keys differ
// (the quantifier's sorts too), and the five stable passes -- the four words from the least significant one, then the length under
// the group -- that leave idx in ascending (group, length, bytes) order with equal fields' items in ascending index.  Host only.
#pragma once
#include <algorithm>

#include "accum.h"
#include "barcode_kernels.h"
#include "quant_kernels.h"

namespace br {

// key / index pairs of a radix sort: the sorted pairs are those of [0] when sort returns
struct SortBufs {
  ColBuf key[2], idx[2];
  int make(Accum *c, size_t items) {
    for (int k = 0; k < 2; k++) { RC(c->alloc(key[k], (items + 1) * 8)); RC(c->alloc(idx[k], (items + 1) * 4)); }
    return BR_OK;
  }
};

// the radix sort of (key[0], idx[0]) over the digits in which the keys differ; the sorted pairs are those of [0] when it returns.
// d_bits: two words of the caller's on the device
inline int sort_pairs(Accum *c, ColBuf key[2], ColBuf idx[2], int64_t n, ColBuf &tmp, uint64_t *d_bits) {
  if (n <= 0) return BR_OK;
  hipStream_t st = c->st;
  RC(c->alloc(tmp, scan_tmp_bytes(n)));
  launch_q_bits(st, key[0].as<uint64_t>(), n, tmp.as<uint64_t>(), d_bits);
  uint64_t bits[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(bits, d_bits, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int cur = 0;
  RC(c->radix_sort(key, idx, n, bits, tmp, &cur));
  if (cur) { std::swap(key[0], key[1]); std::swap(idx[0], idx[1]); }
  return BR_OK;
}
inline int sort_pairs(Accum *c, SortBufs &s, int64_t n, ColBuf &tmp, uint64_t *d_bits) { return sort_pairs(c, s.key, s.idx, n, tmp, d_bits); }

// s.idx[0] (n items of the table words / len) into ascending (gid, length, bytes) order -- gid NULL: (length, bytes) -- least
// significant word first, every sort stable
inline int sort_by_barcode(Accum *c, SortBufs &s, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int64_t n, ColBuf &tmp, uint64_t *d_bits) {
  for (int w = 3; w >= -1; w--) {
    launch_bc_key(c->st, s.idx[0].as<uint32_t>(), words, len, gid, n, w < 0 ? 4 : w, s.key[0].as<uint64_t>());
    RC(sort_pairs(c, s, n, tmp, d_bits));
  }
  return BR_OK;
}

}  // namespace br
