// A projected row's rewritten CIGAR, as every kernel that reads rows takes it (device code only; include after hip_runtime.h).
//
// An op is a BAM word: the code in its low four bits (M I D N S H P = X: 0 .. 8), the length above them.  A row of one or two
// ops carries them in its 64-bit CIGAR reference (the first in the low word); a longer one carries an offset into the pool of
// op words, which is the caller's and is checked before it is followed.
//
//   cigar_covers(op) / cigar_skips(op)       M = X lay bases on the reference; D N pass over it
//   cigar_ref_len(op)                        the reference bases of one op: its length for M D N = X, else 0
//   pool_holds(n_pool_words, off, n)         the n words from off on lie inside the pool
//   cigar_ref_len_inline(c, n)               the reference bases of a row of n <= 2 ops held in c
//   wave_cigar_ref_len(pool, off, n)         those of a pooled CIGAR, summed by the wave: every lane gets the sum
#pragma once
#include <stdint.h>

#include "wave_inl.h"

namespace br {

__device__ __forceinline__ bool cigar_covers(uint32_t op) { return (0x181u >> (op & 15u)) & 1u; }   // M = X (0, 7, 8)
__device__ __forceinline__ bool cigar_skips(uint32_t op) { return (0x00cu >> (op & 15u)) & 1u; }    // D N (2, 3)
__device__ __forceinline__ uint64_t cigar_ref_len(uint32_t op) { return ((0x181u | 0x00cu) >> (op & 15u)) & 1u ? (uint64_t)(op >> 4) : 0ull; }

// (off is a word read from a table: nothing is added to it before it was compared)
__device__ __forceinline__ bool pool_holds(uint64_t n_pool_words, uint64_t off, uint32_t n) { return off <= n_pool_words && (uint64_t)n <= n_pool_words - off; }

__device__ __forceinline__ uint64_t cigar_ref_len_inline(uint64_t c, uint32_t n) {
  return (n >= 1u ? cigar_ref_len((uint32_t)c) : 0ull) + (n >= 2u ? cigar_ref_len((uint32_t)(c >> 32)) : 0ull);
}

// lane l takes the ops l, l + 64, ...; every lane of the wave calls it, with the same off and n
__device__ __forceinline__ uint64_t wave_cigar_ref_len(const uint32_t *pool, uint64_t off, uint32_t n) {
  uint64_t s = 0;
  for (uint32_t k = threadIdx.x & 63u; k < n; k += 64u) s += cigar_ref_len(pool[off + k]);
  return wave_sum(s);
}

}  // namespace br
