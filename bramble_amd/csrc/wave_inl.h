// Wave and block primitives every kernel unit shares (device code only; include after hip_runtime.h).
//
// The lanes of a wave are taken in groups of W consecutive lanes (W = 64: the wave; 8, 16, 32: the sub-wave groups of the
// kernels that give a group of lanes one alignment or one record).  A lane's place in its group is threadIdx.x & (W - 1):
// every kernel here has one-dimensional blocks whose size is a multiple of 64.
//
//   wave_scan<T, W>(v)                                inclusive prefix sum over the group (lane k: v of lanes 0 .. k)
//   wave_sum / wave_max / wave_min / wave_or / wave_and   butterfly reductions: every lane of the group gets the result
//   count_lanes(cond, word)                           *word += the wave's lanes with cond, one atomic a wave
//   wave_turns(mine, f)                               f(src) for every lane src with mine set, lowest first, the wave converged
//   block_excl_scan_256(v, sh, total)                 exclusive prefix sum over a block of 256 threads
//   block_bits(o, a, out)                             OR of o and AND of a over a block of 256 threads (the radix sort's digits)
//   load8 / store8                                    a thread's eight consecutive scan items as 16-byte accesses
//   kth_set_bit64(mask, k)                            the index of a mask's k-th set bit, without a loop
//   wave_match(v, bits, on)                           the mask of the wave's lanes that hold the same value
//   scan_top_rounds<C, ITEMS>(...)                    a scan's tile sums scanned in place by one block
#pragma once
#include <stdint.h>

namespace br {

template <typename T, int W = 64>
__device__ __forceinline__ T wave_scan(T v) {
  const int gl = (int)(threadIdx.x & (W - 1));
#pragma unroll
  for (int d = 1; d < W; d <<= 1) { const T y = __shfl_up(v, d, W); if (gl >= d) v += y; }
  return v;
}

// The xor order W/2, ..., 1 is part of the contract: the quantification's EM sums doubles with wave_sum and its results are
// compared bit by bit.
template <typename T, int W = 64>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, W);
  return v;
}
template <typename T, int W = 64>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) { const T y = __shfl_xor(v, d, W); v = y > v ? y : v; }
  return v;
}
template <typename T, int W = 64>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) { const T y = __shfl_xor(v, d, W); v = y < v ? y : v; }
  return v;
}
template <typename T, int W = 64>
__device__ __forceinline__ T wave_or(T v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) v |= __shfl_xor(v, d, W);
  return v;
}
template <typename T, int W = 64>
__device__ __forceinline__ T wave_and(T v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) v &= __shfl_xor(v, d, W);
  return v;
}

// one atomic a wave for a per-lane condition (every lane of the wave calls it)
__device__ __forceinline__ void count_lanes(bool cond, unsigned long long *word) {
  const uint64_t b = __ballot(cond);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(word, (unsigned long long)__popcll((unsigned long long)b));
}

// The lanes whose item is too long for one lane take turns, and the wave does each one: f(src) runs once for every lane src
// of the wave that has `mine` set, lowest lane first, with all 64 lanes in it (they fetch src's item by __shfl(.., src), share
// its work and leave the result to the lane with lane == src).  Every lane of the wave calls it.
template <typename F>
__device__ __forceinline__ void wave_turns(bool mine, F f) {
  for (uint64_t todo = __ballot(mine); todo; todo &= todo - 1) f(__ffsll((unsigned long long)todo) - 1);
}

// Exclusive prefix sum of v over the block's 256 threads; total = the block's sum, in every thread.  Wave scans by shuffles,
// then across the 4 waves through sh[4].  Two barriers: sh is free again when it returns.
template <typename T>
__device__ __forceinline__ T block_excl_scan_256(T v, T *sh, T &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T x = wave_scan(v);
  if (lane == 63) sh[w] = x;
  __syncthreads();
  T wbase = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { if (i < w) wbase += sh[i]; tot += sh[i]; }
  __syncthreads();
  total = tot;
  return wbase + x - v;
}

// OR of o and AND of a over the block's 256 threads -> out[0], out[1] (thread 0 stores them).  The radix sorts skip the digits
// in which OR and AND agree.
__device__ __forceinline__ void block_bits(uint64_t o, uint64_t a, uint64_t *out) {
  __shared__ uint64_t sh[2][4];
  o = wave_or(o); a = wave_and(a);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = o; sh[1][threadIdx.x >> 6] = a; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { o |= sh[0][w]; a &= sh[1][w]; }
    out[0] = o; out[1] = a;
  }
}

// A thread's eight consecutive items p[base .. base + 8) as 16-byte accesses (base is a multiple of 8 items).  One 4-byte
// load per item made a wave touch every eighth word of a 2 KB span eight times over.  Items at or past n read as 0 and are
// not written.  The arrays are allocations or offsets into one, and an offset need not be a multiple of 16 bytes (the
// collation's byte counts sit behind its own n + 1 words): those, and the tile that holds n, go item by item.
template <typename T>
__device__ __forceinline__ void load8(const T *p, int64_t base, int64_t n, T v[8]) {
  constexpr int V = 16 / sizeof(T);   // items per 16 bytes
  typedef T vec_t __attribute__((ext_vector_type(V)));
  if (base + 8 <= n && ((uintptr_t)(p + base) & 15u) == 0) {
#pragma unroll
    for (int k = 0; k < 8; k += V) {
      const vec_t a = *(const vec_t *)(p + base + k);
#pragma unroll
      for (int j = 0; j < V; j++) v[k + j] = a[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = (base + k < n) ? p[base + k] : (T)0;
  }
}
template <typename T>
__device__ __forceinline__ void store8(T *p, int64_t base, int64_t n, const T v[8]) {
  constexpr int V = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  if (base + 8 <= n && ((uintptr_t)(p + base) & 15u) == 0) {
#pragma unroll
    for (int k = 0; k < 8; k += V) {
      vec_t a;
#pragma unroll
      for (int j = 0; j < V; j++) a[j] = v[k + j];
      *(vec_t *)(p + base + k) = a;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) if (base + k < n) p[base + k] = v[k];
  }
}

// The index of the k-th set bit of mask (k = 0: the lowest), for k < popcount(mask): six fixed steps, each keeping the half
// whose population count holds k.  Clearing the lowest bit k times made a wave wait for its largest k.
__device__ __forceinline__ uint32_t kth_set_bit64(uint64_t mask, uint32_t k) {
  uint32_t w = (uint32_t)mask, r = 0;
  uint32_t c = (uint32_t)__popc(w);
  if (k >= c) { k -= c; w = (uint32_t)(mask >> 32); r = 32; }
  c = (uint32_t)__popc(w & 0xffffu); if (k >= c) { k -= c; w >>= 16; r += 16; }
  c = (uint32_t)__popc(w & 0xffu); if (k >= c) { k -= c; w >>= 8; r += 8; }
  c = (uint32_t)__popc(w & 0xfu); if (k >= c) { k -= c; w >>= 4; r += 4; }
  c = (uint32_t)__popc(w & 3u); if (k >= c) { k -= c; w >>= 2; r += 2; }
  if (k >= (w & 1u)) r += 1;
  return r;
}

// lane 63's v, in every lane of the wave (a scalar)
__device__ __forceinline__ uint64_t wave_last64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// The lanes of the wave that hold the same v as this lane, as a mask (the lane's own bit is set); a lane with `on` false is in
// nobody's mask and gets 0.  v < 2^bits, bits the same in every lane: one ballot a bit, so the cost does not depend on how many
// values are equal (a loop over the distinct values took 64 rounds for 64 different ones).  The whole wave calls it.
__device__ __forceinline__ uint64_t wave_match(uint32_t v, int bits, bool on) {
  uint64_t m = __ballot(on);
  for (int b = 0; b < bits; b++) {
    const bool set = (v >> b) & 1u;
    const uint64_t y = __ballot(set);
    m &= set ? y : ~y;
  }
  return on ? m : 0ull;
}

// The tile sums of a scan, scanned in place by ONE block of 256 threads: C arrays of n_tiles sums, one behind the other,
// 256 * ITEMS sums a round.  A wave takes 64 * ITEMS consecutive sums as ITEMS rows of 64: lane l loads and stores word
// 64 k + l of them, so every access of a wave is one run of 512 bytes, and all of a round's loads are in flight before the
// first use.  The rows are scanned by wave_scan, one behind the other with a running (scalar) carry; the four waves'
// totals meet in sh[4].  (ITEMS consecutive sums per thread needed no shuffles but put a wave's lanes ITEMS * 8 bytes
// apart: 64 cache lines per load and per store instruction; one sum per thread and round before that was a chain of
// n_tiles / 256 load-scan-store rounds.)  total_out[c] = the sum of array c (NULL: not wanted).
template <int C, int ITEMS>
__device__ __forceinline__ void scan_top_rounds(uint64_t *tile_sums, int64_t n_tiles, uint64_t *total_out, uint64_t *sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t carry[C];
#pragma unroll
  for (int c = 0; c < C; c++) carry[c] = 0;
  for (int64_t base = 0; base < n_tiles; base += 256 * ITEMS) {
    const int64_t i0 = base + (int64_t)w * (64 * ITEMS) + lane;
    uint64_t v[C][ITEMS];
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
      for (int k = 0; k < ITEMS; k++) v[c][k] = i0 + 64 * k < n_tiles ? tile_sums[(int64_t)c * n_tiles + i0 + 64 * k] : 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
      uint64_t run = 0;   // the wave's sums before row k
#pragma unroll
      for (int k = 0; k < ITEMS; k++) {
        const uint64_t x = wave_scan(v[c][k]);
        v[c][k] = run + x - v[c][k];
        run += wave_last64(x);
      }
      if (lane == 0) sh[w] = run;
      __syncthreads();
      uint64_t ex = carry[c], tot = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) { if (i < w) ex += sh[i]; tot += sh[i]; }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < ITEMS; k++) if (i0 + 64 * k < n_tiles) tile_sums[(int64_t)c * n_tiles + i0 + 64 * k] = ex + v[c][k];
      carry[c] += tot;
    }
  }
  if (total_out && threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < C; c++) total_out[c] = carry[c];
  }
}

}  // namespace br
