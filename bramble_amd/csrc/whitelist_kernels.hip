// The cell barcode whitelist on the device (host side: whitelist.cpp, which holds the pipeline's description; the definitions are in
// bramble_amd.h, br_whitelist).
//
//   build     the barcodes sorted by (length, bytes) with the cells' radix passes and cut into distinct entries (k_wl_gather);
//             k_wl_insert: a lane per entry claims a slot of the open-addressing table with a 64-bit compare-and-swap, linear probing
//   resolve   k_wl_flag + scan + compact, the same sort and cut over the names' observed barcodes; k_wl_exact: a lane per distinct
//             observed barcode probes once; k_wl_near: a wave per observed barcode that missed probes its up to 128 one-byte variants,
//             two a lane, and decides with ballots and one max-reduction; k_wl_apply: a lane per name
//
// A probe walks at most n_slots slots and stops at an empty one; it loads an entry's 32 bytes only where the slot's tag matches.  Which
// slot an entry sits in depends on the order of the inserts' atomics; what a probe returns does not.  No LDS, no floating point; the
// integer atomics besides the table's count names per status.  No cross-lane operation stands inside a probe loop: the lanes of a wave
// leave it at different times.
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "wave_inl.h"
#include "whitelist_kernels.h"

namespace br {

namespace {
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
__device__ __forceinline__ uint64_t fmix64(uint64_t h) {   // (murmur3's, as dedup_kernels.hip has it)
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
// the masked hash of a barcode: the home slot is its low bits, the tag its high word
__device__ __forceinline__ uint64_t wl_hash(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t len, uint64_t mask) {
  uint64_t h = fmix64(w0 ^ (uint64_t)len * 0x9E3779B97F4A7C15ull);
  h = fmix64(h ^ w1 + 0xD6E8FEB86659FD93ull);
  h = fmix64(h ^ w2 + 0xA0761D6478BD642Full);
  h = fmix64(h ^ w3 + 0xE7037ED1A0B428DBull);
  return h & mask;
}
// the entry of a barcode, or WL_NONE
__device__ __forceinline__ uint32_t wl_probe(const WlTable &T, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t len) {
  const uint64_t h = wl_hash(w0, w1, w2, w3, len, T.mask), last = T.n_slots - 1;
  const uint32_t tag = (uint32_t)(h >> 32);
  uint64_t at = h & last;
  for (uint64_t k = 0; k < T.n_slots; k++, at = (at + 1) & last) {
    const uint64_t s = T.slots[at];
    if (s == 0) return WL_NONE;
    if ((uint32_t)(s >> 32) != tag) continue;
    const uint64_t e = (uint64_t)(uint32_t)s - 1;
    if (e >= (uint64_t)T.n_entries || T.len[e] != len) continue;
    const uint64_t *q = T.cb + 4 * e;
    if (q[0] == w0 && q[1] == w1 && q[2] == w2 && q[3] == w3) return (uint32_t)e;
  }
  return WL_NONE;
}
}  // namespace

// ---- build -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_wl_gather(const uint64_t *pos, const uint32_t *idx, int64_t n, const uint64_t *cb, const uint8_t *len,
                                                   uint64_t *out_cb, uint8_t *out_len) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n || pos[j + 1] == pos[j]) return;
  const uint64_t e = pos[j], i = idx[j];
#pragma unroll
  for (int w = 0; w < 4; w++) out_cb[4 * e + w] = cb[4 * i + w];
  out_len[e] = len[i];
}
void launch_wl_gather(hipStream_t st, const uint64_t *pos, const uint32_t *idx, int64_t n, const uint64_t *cb, const uint8_t *len, uint64_t *out_cb,
                      uint8_t *out_len) {
  if (n > 0) hipLaunchKernelGGL(k_wl_gather, dim3(blocks256(n)), dim3(256), 0, st, pos, idx, n, cb, len, out_cb, out_len);
}

__global__ void __launch_bounds__(256) k_wl_insert(WlTable T, uint64_t *slots, unsigned long long *counters) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= T.n_entries) return;
  const uint64_t *q = T.cb + 4 * e;
  const uint64_t h = wl_hash(q[0], q[1], q[2], q[3], T.len[e], T.mask), last = T.n_slots - 1;
  const unsigned long long mine = (h >> 32) << 32 | (uint64_t)(e + 1);
  uint64_t at = h & last, k = 0;
  bool placed = false;
  for (; k < T.n_slots && !placed; k++, at = (at + 1) & last)
    placed = atomicCAS((unsigned long long *)slots + at, 0ull, mine) == 0ull;   // (the entries are distinct: none is in the table yet)
  if (!placed) atomicAdd(counters + WL_FULL, 1ull);
  atomicMax(counters + WL_CHAIN, (unsigned long long)k);
}
void launch_wl_insert(hipStream_t st, const WlTable &T, uint64_t *slots, unsigned long long *counters) {
  if (T.n_entries > 0) hipLaunchKernelGGL(k_wl_insert, dim3(blocks256(T.n_entries)), dim3(256), 0, st, T, slots, counters);
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_wl_flag(const uint8_t *cblen, int64_t n, uint64_t *flag, uint32_t *entry) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flag[i] = cblen[i] != 0 ? 1 : 0;
  if (entry) entry[i] = WL_NONE;
}
void launch_wl_flag(hipStream_t st, const uint8_t *cblen, int64_t n, uint64_t *flag, uint32_t *entry) {
  if (n > 0) hipLaunchKernelGGL(k_wl_flag, dim3(blocks256(n)), dim3(256), 0, st, cblen, n, flag, entry);
}

__global__ void __launch_bounds__(256) k_wl_exact(WlTable T, const uint32_t *idx, const uint64_t *obeg, int64_t n_obs, const uint64_t *cb,
                                                  const uint8_t *cblen, uint32_t *obs_entry, uint64_t *count, uint64_t *miss) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_obs) return;
  const uint64_t b = obeg[o], i = idx[b];
  const uint64_t *q = cb + 4 * i;
  const uint32_t e = wl_probe(T, q[0], q[1], q[2], q[3], cblen[i]);
  obs_entry[o] = e;
  miss[o] = e == WL_NONE ? 1 : 0;
  if (e != WL_NONE) count[e] = obeg[o + 1] - b;   // (distinct observed barcodes hit distinct entries)
}
void launch_wl_exact(hipStream_t st, const WlTable &T, const uint32_t *idx, const uint64_t *obeg, int64_t n_obs, const uint64_t *cb, const uint8_t *cblen,
                     uint32_t *obs_entry, uint64_t *count, uint64_t *miss) {
  if (n_obs > 0) hipLaunchKernelGGL(k_wl_exact, dim3(blocks256(n_obs)), dim3(256), 0, st, T, idx, obeg, n_obs, cb, cblen, obs_entry, count, miss);
}

// Variant v = 4 * position + base of the wave's barcode, v in [0, 4 L): lane l takes v = l and v = l + 64.  A candidate is a variant
// that is an entry; distinct variants are distinct barcodes, so distinct candidates.  Its weight is 1 ("correct" 1) or count[entry]
// ("correct" 2, where a weight of 0 is no candidate): the wave's largest (weight, entry) is the answer when exactly one candidate has
// that weight, two or more having it are ambiguous, none is no match.
__global__ void __launch_bounds__(256) k_wl_near(WlTable T, const uint32_t *list, int64_t n_list, const uint32_t *idx, const uint64_t *obeg,
                                                 const uint64_t *cb, const uint8_t *cblen, const uint64_t *count, int correct, uint32_t *obs_entry) {
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= n_list) return;   // (the whole wave)
  const uint32_t lane = threadIdx.x & 63, o = list[wv];
  const uint64_t i = idx[obeg[o]];
  const uint64_t w0 = cb[4 * i], w1 = cb[4 * i + 1], w2 = cb[4 * i + 2], w3 = cb[4 * i + 3];
  const uint32_t len = cblen[i];
  uint64_t key[2] = {0, 0};
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const uint32_t v = lane + 64u * pass, p = v >> 2, word = p >> 3, shift = 56u - 8u * (p & 7u);
    const uint64_t base = (uint64_t)((0x54474341u >> (8u * (v & 3u))) & 255u);   // "ACGT"
    const uint64_t mine = word == 0 ? w0 : word == 1 ? w1 : word == 2 ? w2 : w3;
    const bool live = p < len && ((mine >> shift) & 255u) != base;
    const uint64_t put = (mine & ~(255ull << shift)) | base << shift;
    uint32_t e = WL_NONE;
    if (live) e = wl_probe(T, word == 0 ? put : w0, word == 1 ? put : w1, word == 2 ? put : w2, word == 3 ? put : w3, len);
    if (e != WL_NONE) {
      const uint64_t weight = correct == 2 ? count[e] : 1;
      if (weight) key[pass] = weight << 32 | e;
    }
  }
  const uint64_t best = wave_max<uint64_t>(key[0] > key[1] ? key[0] : key[1]), top = best >> 32;
  const uint32_t ties = (uint32_t)__popcll((unsigned long long)__ballot(key[0] && key[0] >> 32 == top)) +
                        (uint32_t)__popcll((unsigned long long)__ballot(key[1] && key[1] >> 32 == top));
  if (lane == 0) obs_entry[o] = best == 0 ? WL_NONE : ties > 1 ? WL_AMBIG : (uint32_t)best;
}
void launch_wl_near(hipStream_t st, const WlTable &T, const uint32_t *list, int64_t n_list, const uint32_t *idx, const uint64_t *obeg, const uint64_t *cb,
                    const uint8_t *cblen, const uint64_t *count, int correct, uint32_t *obs_entry) {
  if (n_list > 0) hipLaunchKernelGGL(k_wl_near, dim3((unsigned)((n_list + 3) / 4)), dim3(256), 0, st, T, list, n_list, idx, obeg, cb, cblen, count, correct, obs_entry);
}

__global__ void __launch_bounds__(256) k_wl_apply(WlTable T, const uint64_t *oid, const uint32_t *idx, int64_t n, const uint32_t *obs_entry, uint64_t *cb,
                                                  uint8_t *cblen, uint8_t *status, uint32_t *entry, unsigned long long *counters) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t s = 0;
  if (j < n) {
    const uint64_t i = idx[j];
    const uint32_t e = obs_entry[oid[j + 1] - 1];
    uint64_t w[4] = {0, 0, 0, 0};
    uint32_t len = 0;
    if (e == WL_NONE) s = 3;
    else if (e == WL_AMBIG) s = 4;
    else {
      len = T.len[e];
      bool same = len == cblen[i];
#pragma unroll
      for (int k = 0; k < 4; k++) { w[k] = T.cb[4 * (uint64_t)e + k]; same = same && w[k] == cb[4 * i + k]; }
      s = same ? 1 : 2;
    }
    if (s != 1) {
#pragma unroll
      for (int k = 0; k < 4; k++) cb[4 * i + k] = w[k];
      cblen[i] = (uint8_t)len;
    }
    status[i] = (uint8_t)s;
    if (entry) entry[i] = s <= 2 ? e : WL_NONE;
  }
#pragma unroll
  for (uint32_t k = 1; k <= 4; k++) count_lanes(s == k, counters + WL_STATUS + k);
}
void launch_wl_apply(hipStream_t st, const WlTable &T, const uint64_t *oid, const uint32_t *idx, int64_t n, const uint32_t *obs_entry, uint64_t *cb,
                     uint8_t *cblen, uint8_t *status, uint32_t *entry, unsigned long long *counters) {
  if (n > 0) hipLaunchKernelGGL(k_wl_apply, dim3(blocks256(n)), dim3(256), 0, st, T, oid, idx, n, obs_entry, cb, cblen, status, entry, counters);
}

}  // namespace br
