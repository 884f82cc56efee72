// Collation by read name on the device (host side: collate.cpp, which holds the pipeline's description).
//
//   append   k_col_lens -> scan (launch_scan, scan_kernels.h) -> k_col_copy: records into one arena, compacted, [block_size][record]
//   key      k_col_key: FNV-1a over l_read_name and the name bytes, a 64-bit finaliser, masked (hash_bits)
//   sort     k_col_hist + scan + k_col_scatter per 8-bit digit: a stable LSD radix sort of (key, input index)
//   runs     k_col_heads: group starts in sorted order; equal keys with different names are counted and listed
//   place    k_col_gbeg, k_col_head_count + scan, k_col_place, scan, k_col_starts: groups in order of their first record
//   cut      k_col_cut: the first group start at or after a target
#include <hip/hip_runtime.h>

#include "collate_kernels.h"
#include "scan_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
__device__ __forceinline__ const uint8_t *rec_at(const uint8_t *arena, const uint64_t *off, uint32_t i) { return arena + off[i]; }
// read names equal: l_read_name and its bytes (the NUL included)
__device__ __forceinline__ bool same_name(const uint8_t *a, const uint8_t *b) {
  const uint32_t la = a[8], lb = b[8];
  if (la != lb) return false;
  for (uint32_t k = 0; k < la; k++) if (a[32 + k] != b[32 + k]) return false;
  return true;
}
}  // namespace

__global__ void __launch_bounds__(256) k_col_lens(const uint64_t *rec_off, const uint32_t *rec_len, int64_t n, uint64_t *bytes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bytes[i] = 4 + (rec_len ? (uint64_t)rec_len[i] : rec_off[i + 1] - rec_off[i]);
}

// one wave per record, grid-stride; byte copies (source and destination offsets have any alignment)
__global__ void __launch_bounds__(256) k_col_copy(const uint8_t *blob, const uint64_t *rec_off, const uint32_t *rec_len, int64_t n,
                                                  const uint64_t *dst, uint64_t base, uint8_t *arena, uint64_t *off_out, uint32_t *len_out) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += waves) {
    const uint64_t so = rec_off[i] - 4, d = base + dst[i];
    const uint32_t len = rec_len ? rec_len[i] : (uint32_t)(rec_off[i + 1] - rec_off[i]);
    const uint8_t *s = blob + so;
    uint8_t *t = arena + d;
    for (uint32_t k = (uint32_t)lane; k < len + 4; k += 64) t[k] = s[k];
    if (lane == 0) { off_out[i] = d + 4; len_out[i] = len; }
  }
}

__global__ void __launch_bounds__(256) k_col_key(const uint8_t *arena, const uint64_t *off, int64_t n, uint64_t mask, uint64_t *key,
                                                 uint32_t *idx, uint64_t *part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t o = 0, a = ~0ull;
  if (i < n) {
    const uint8_t *r = arena + off[i];
    const uint32_t l = r[8];
    uint64_t h = 1469598103934665603ull;   // FNV-1a
    h = (h ^ l) * 1099511628211ull;
    for (uint32_t k = 0; k < l; k++) h = (h ^ r[32 + k]) * 1099511628211ull;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;   // (murmur3 fmix64: every bit of the low digits mixes)
    h &= mask;
    key[i] = h; idx[i] = (uint32_t)i;
    o = h; a = h;
  }
  block_bits(o, a, part + 2 * blockIdx.x);
}
__global__ void __launch_bounds__(256) k_col_bits(const uint64_t *part, int64_t blocks, uint64_t *bits) {
  uint64_t o = 0, a = ~0ull;
  for (int64_t b = threadIdx.x; b < blocks; b += 256) { o |= part[2 * b]; a &= part[2 * b + 1]; }
  block_bits(o, a, bits);
}

// per-tile digit counts in LDS, one store per digit per tile: hist[digit * n_tiles + tile]
__global__ void __launch_bounds__(256) k_col_hist(const uint64_t *key, int64_t n, int shift, uint64_t *hist, int64_t n_tiles) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * COL_TILE;
  for (int r = 0; r < COL_TILE / 256; r++) {
    const int64_t i = base + r * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[(uint32_t)(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// Stable scatter.  A tile's items are taken in 8 rounds of 256 (round-major, then wave, then lane = input order).  Inside a
// wave, the lanes with the same digit come from 8 ballots; an item's rank is the popcount of its match mask below its lane, the
// waves in front add their counts for the digit from LDS, and the rounds in front theirs (run[]).
__global__ void __launch_bounds__(256) k_col_scatter(const uint64_t *key_in, const uint32_t *idx_in, uint64_t *key_out,
                                                     uint32_t *idx_out, int64_t n, int shift, const uint64_t *hist, int64_t n_tiles) {
  __shared__ uint32_t wcnt[4][256];
  __shared__ uint32_t run[256];
  __shared__ uint64_t gbase[256];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  run[t] = 0;
  gbase[t] = hist[(int64_t)t * n_tiles + blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * COL_TILE;
  for (int r = 0; r < COL_TILE / 256; r++) {
    for (int q = 0; q < 4; q++) wcnt[q][t] = 0;
    __syncthreads();
    const int64_t i = base + r * 256 + t;
    const bool valid = i < n;
    const uint64_t k = valid ? key_in[i] : 0;
    const uint32_t d = (uint32_t)(k >> shift) & 255u;
    uint64_t m = __ballot(valid);
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(m & lt);
    if (valid && rank == 0) wcnt[w][d] = (uint32_t)__popcll(m);
    __syncthreads();
    if (valid) {
      uint32_t pre = run[d];
      for (int q = 0; q < w; q++) pre += wcnt[q][d];
      const uint64_t pos = gbase[d] + pre + rank;
      key_out[pos] = k; idx_out[pos] = idx_in[i];
    }
    __syncthreads();
    run[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
    __syncthreads();
  }
}

// head[j] = item j starts a group; a pair of equal keys with different names is a collision: its run goes to the list
__global__ void __launch_bounds__(256) k_col_heads(const uint8_t *arena, const uint64_t *off, const uint64_t *key, const uint32_t *idx,
                                                   int64_t n, uint64_t *head, unsigned long long *n_coll, unsigned long long *n_runs,
                                                   uint64_t *runs, uint64_t cap) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool coll = false;
  if (j < n) {
    uint64_t h = 1;
    if (j > 0) {
      const uint64_t kj = key[j];
      if (kj == key[j - 1]) {
        const bool same = same_name(rec_at(arena, off, idx[j]), rec_at(arena, off, idx[j - 1]));
        h = same ? 0 : 1;
        coll = !same;
        if (coll) {   // the run of kj: [lower_bound, upper_bound) in the sorted keys
          int64_t lo = 0, hi = j - 1;
          while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] < kj) lo = mid + 1; else hi = mid; }
          const int64_t b = lo;
          lo = j + 1; hi = n;
          while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] <= kj) lo = mid + 1; else hi = mid; }
          const unsigned long long s = atomicAdd(n_runs, 1ull);
          if (s < cap) { runs[2 * s] = (uint64_t)b; runs[2 * s + 1] = (uint64_t)lo; }
        }
      }
    }
    head[j] = h;
  }
  const uint64_t bal = __ballot(coll);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_coll, (unsigned long long)__popcll(bal));   // (collisions only: none at all with 64-bit keys in practice)
}

__global__ void __launch_bounds__(256) k_col_names(const uint8_t *arena, const uint64_t *off, const uint32_t *list, int64_t m, uint8_t *slots) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= m) return;
  const uint8_t *r = arena + off[list[k]];
  const uint32_t l = r[8];
  uint8_t *s = slots + (uint64_t)k * 256;
  if (lane == 0) s[0] = (uint8_t)l;
  for (uint32_t q = (uint32_t)lane; q < l && q < 255u; q += 64) s[1 + q] = r[32 + q];
}

__global__ void __launch_bounds__(256) k_col_gbeg(const uint64_t *gid, int64_t n, uint64_t *gbeg) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n && gid[j + 1] != gid[j]) gbeg[gid[j]] = (uint64_t)j;
  if (j == n) gbeg[gid[n]] = (uint64_t)n;
}
// hc[input index of a group's head] = the group's size (hc zeroed before)
__global__ void __launch_bounds__(256) k_col_head_count(const uint64_t *gbeg, const uint32_t *idx, int64_t g, uint64_t *hc) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < g) hc[idx[gbeg[k]]] = gbeg[k + 1] - gbeg[k];
}
// item j of group g (sorted items [b, e)) goes to start(g) + (j - b); start(g) = the scanned count at its head's input index
__global__ void __launch_bounds__(256) k_col_place(const uint64_t *gid, const uint64_t *gbeg, const uint64_t *start, const uint32_t *idx,
                                                   const uint64_t *off, const uint32_t *len, int64_t n, uint64_t *out_off,
                                                   uint32_t *out_len, uint32_t *out_idx, uint64_t *mark) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t g = gid[j + 1] - 1;
  const uint64_t b = gbeg[g];
  const uint32_t x = idx[j];
  const uint64_t pos = start[idx[b]] + ((uint64_t)j - b);
  out_off[pos] = off[x]; out_len[pos] = len[x]; out_idx[pos] = x;
  mark[pos] = (uint64_t)j == b ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_col_starts(const uint64_t *ms, int64_t n, uint64_t *starts) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n && ms[p + 1] != ms[p]) starts[ms[p]] = (uint64_t)p;
  if (p == n) starts[ms[n]] = (uint64_t)n;
}
__global__ void k_col_cut(const uint64_t *starts, int64_t g, uint64_t target, uint64_t *res) {
  int64_t lo = 0, hi = g;   // starts[g] = n >= target
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (starts[mid] < target) lo = mid + 1; else hi = mid; }
  *res = starts[lo];
}

static unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

void launch_col_lens(hipStream_t st, const uint64_t *rec_off, const uint32_t *rec_len, int64_t n, uint64_t *bytes) {
  if (n > 0) hipLaunchKernelGGL(k_col_lens, dim3(blocks256(n)), dim3(256), 0, st, rec_off, rec_len, n, bytes);
}
void launch_col_copy(hipStream_t st, const uint8_t *blob, const uint64_t *rec_off, const uint32_t *rec_len, int64_t n,
                     const uint64_t *dst, uint64_t base, uint8_t *arena, uint64_t *off_out, uint32_t *len_out) {
  if (n <= 0) return;
  const int64_t g = (n + 3) / 4;
  hipLaunchKernelGGL(k_col_copy, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(256), 0, st, blob, rec_off, rec_len, n, dst, base, arena, off_out, len_out);
}
void launch_col_bits(hipStream_t st, const uint64_t *part, int64_t blocks, uint64_t *bits) {
  hipLaunchKernelGGL(k_col_bits, dim3(1), dim3(256), 0, st, part, blocks, bits);
}
void launch_col_key(hipStream_t st, const uint8_t *arena, const uint64_t *off, int64_t n, uint64_t mask, uint64_t *key,
                    uint32_t *idx, uint64_t *part, uint64_t *bits) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_col_key, dim3(blocks256(n)), dim3(256), 0, st, arena, off, n, mask, key, idx, part);
  launch_col_bits(st, part, (int64_t)blocks256(n), bits);
}
void launch_col_radix_pass(hipStream_t st, const uint64_t *key_in, const uint32_t *idx_in, uint64_t *key_out, uint32_t *idx_out,
                           int64_t n, int shift, uint64_t *hist, uint64_t *tmp) {
  if (n <= 0) return;
  const int64_t tiles = (n + COL_TILE - 1) / COL_TILE;
  hipLaunchKernelGGL(k_col_hist, dim3((unsigned)tiles), dim3(256), 0, st, key_in, n, shift, hist, tiles);
  launch_scan(st, hist, 256 * tiles, tmp);
  hipLaunchKernelGGL(k_col_scatter, dim3((unsigned)tiles), dim3(256), 0, st, key_in, idx_in, key_out, idx_out, n, shift,
                     (const uint64_t *)hist, tiles);
}
void launch_col_heads(hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint64_t *key, const uint32_t *idx, int64_t n,
                      uint64_t *head, unsigned long long *n_coll, unsigned long long *n_runs, uint64_t *runs, uint64_t cap) {
  if (n > 0) hipLaunchKernelGGL(k_col_heads, dim3(blocks256(n)), dim3(256), 0, st, arena, off, key, idx, n, head, n_coll, n_runs, runs, cap);
}
void launch_col_names(hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint32_t *list, int64_t m, uint8_t *slots) {
  if (m > 0) hipLaunchKernelGGL(k_col_names, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, arena, off, list, m, slots);
}
void launch_col_gbeg(hipStream_t st, const uint64_t *gid, int64_t n, uint64_t *gbeg) {
  hipLaunchKernelGGL(k_col_gbeg, dim3(blocks256(n + 1)), dim3(256), 0, st, gid, n, gbeg);
}
void launch_col_head_count(hipStream_t st, const uint64_t *gbeg, const uint32_t *idx, int64_t g, uint64_t *hc) {
  if (g > 0) hipLaunchKernelGGL(k_col_head_count, dim3(blocks256(g)), dim3(256), 0, st, gbeg, idx, g, hc);
}
void launch_col_place(hipStream_t st, const uint64_t *gid, const uint64_t *gbeg, const uint64_t *start, const uint32_t *idx,
                      const uint64_t *off, const uint32_t *len, int64_t n, uint64_t *out_off, uint32_t *out_len, uint32_t *out_idx,
                      uint64_t *mark) {
  if (n > 0) hipLaunchKernelGGL(k_col_place, dim3(blocks256(n)), dim3(256), 0, st, gid, gbeg, start, idx, off, len, n, out_off, out_len, out_idx, mark);
}
void launch_col_starts(hipStream_t st, const uint64_t *mark_scan, int64_t n, uint64_t *starts) {
  hipLaunchKernelGGL(k_col_starts, dim3(blocks256(n + 1)), dim3(256), 0, st, mark_scan, n, starts);
}
void launch_col_cut(hipStream_t st, const uint64_t *starts, int64_t g, uint64_t target, uint64_t *res) {
  hipLaunchKernelGGL(k_col_cut, dim3(1), dim3(1), 0, st, starts, g, target, res);
}

}  // namespace br
