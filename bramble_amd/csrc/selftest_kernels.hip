// Test-only probes of the shared scan unit, the wave and block primitives and the rows' CIGARs (scan_kernels.h, wave_inl.h,
// launch_scan3, cigar_inl.h):
// libbramble_selftest.so, loaded by tests/scan_probe.py and by nothing in the product.  Every entry point takes raw device
// pointers, launches the product's own code on the stream it is given (0: the null stream), synchronises and returns the
// HIP error code.  The probe kernels only move values between memory and the primitive under test.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cigar_inl.h"
#include "kernels.h"
#include "scan_kernels.h"
#include "wave_inl.h"

namespace br {

// thread i: out[i] = primitive<T, W>(in[i]), blocks of 256
enum { WOP_SCAN = 0, WOP_SUM, WOP_MAX, WOP_MIN, WOP_OR, WOP_AND };
template <int OP, typename T, int W>
__global__ void __launch_bounds__(256) k_probe_wave(const T *in, T *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const T v = in[i];
  T r;
  if constexpr (OP == WOP_SCAN) r = wave_scan<T, W>(v);
  else if constexpr (OP == WOP_SUM) r = wave_sum<T, W>(v);
  else if constexpr (OP == WOP_MAX) r = wave_max<T, W>(v);
  else if constexpr (OP == WOP_MIN) r = wave_min<T, W>(v);
  else if constexpr (OP == WOP_OR) r = wave_or<T, W>(v);
  else r = wave_and<T, W>(v);
  out[i] = r;
}

// three scans in a row through the same sh[4], as k_scan3_* does: in, out and tot are three planes of n_blocks * 256 values
template <typename T>
__global__ void __launch_bounds__(256) k_probe_block_scan(const T *in, T *out, T *tot) {
  __shared__ T sh[4];
  const int64_t plane = (int64_t)gridDim.x * 256, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    T t;
    out[j * plane + i] = block_excl_scan_256(in[j * plane + i], sh, t);
    tot[j * plane + i] = t;
  }
}

__global__ void __launch_bounds__(256) k_probe_block_bits(const uint64_t *o, const uint64_t *a, uint64_t *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  block_bits(o[i], a[i], out + 2 * (int64_t)blockIdx.x);
}

// load8 and store8 as the scan kernels use them: thread t of a tile takes the items [base, base + 8); dst[i] = ~src[i] for
// i < n (an item stored at or past n would not be what the guard behind dst holds), sums[thread] = the sum of the eight items
// as loaded (items at or past n read as 0)
template <typename T>
__global__ void __launch_bounds__(256) k_probe_copy8(const T *src, int64_t n, T *dst, uint64_t *sums) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  T v[SCAN_ITEMS];
  load8(src, base, n, v);
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { sum += v[k]; v[k] = ~v[k]; }
  store8(dst, base, n, v);
  sums[(int64_t)blockIdx.x * 256 + threadIdx.x] = sum;
}

template <int C, int ITEMS>
__global__ void __launch_bounds__(256) k_probe_top(uint64_t *tile_sums, int64_t n_tiles, uint64_t *total_out) {
  __shared__ uint64_t sh[4];
  scan_top_rounds<C, ITEMS>(tile_sums, n_tiles, total_out, sh);
}

// out[i] = kth_set_bit64(masks[i], ks[i]), blocks of 256
__global__ void __launch_bounds__(256) k_probe_kth_bit(const uint64_t *masks, const uint32_t *ks, uint32_t *out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = kth_set_bit64(masks[i], ks[i]);
}

// one block of 256: f(src) appends (src, the value of lane src by shuffle, the lanes that are in f) to the list of its wave (64
// entries of three words); counts[wave] = the calls
__global__ void __launch_bounds__(256) k_probe_turns(const uint32_t *flag, const uint32_t *val, uint32_t *lists, uint32_t *counts) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t v = val[threadIdx.x];
  uint32_t n = 0;
  wave_turns(flag[threadIdx.x] != 0u, [&](int src) {
    const uint32_t x = (uint32_t)__shfl((int)v, src), in = (uint32_t)__popcll((unsigned long long)__ballot(true));
    if (n < 64u && lane == 0) { uint32_t *e = lists + 3 * (64 * w + n); e[0] = (uint32_t)src; e[1] = x; e[2] = in; }
    n++;
  });
  if (lane == 0) counts[w] = n;
}

// one block of 256: its waves take the CIGARs (offs[i], ns[i]) in turn: sums[i] = wave_cigar_ref_len, same[i] = the lanes that
// got lane 0's sum.  Thread t < 16 probes the op tables with ops[t]: tab[t] = covers | skips << 1, tab_len[t] = cigar_ref_len,
// and inl[3 t + n] = cigar_ref_len_inline(ops[t] | ops[(t + 1) & 15] << 32, n) for n = 0, 1, 2
__global__ void __launch_bounds__(256) k_probe_cigar(const uint32_t *pool, const uint64_t *offs, const uint32_t *ns, int n_cigars, uint64_t *sums,
                                                    uint32_t *same, const uint32_t *ops, uint32_t *tab, uint64_t *tab_len, uint64_t *inl) {
  const uint32_t lane = threadIdx.x & 63;
  for (int i = threadIdx.x >> 6; i < n_cigars; i += 4) {
    const uint64_t s = wave_cigar_ref_len(pool, offs[i], ns[i]);
    const uint64_t agree = __ballot(s == __shfl(s, 0));
    if (lane == 0) { sums[i] = s; same[i] = (uint32_t)__popcll((unsigned long long)agree); }
  }
  if (threadIdx.x < 16) {
    const uint32_t t = threadIdx.x, op = ops[t];
    tab[t] = (cigar_covers(op) ? 1u : 0u) | (cigar_skips(op) ? 2u : 0u);
    tab_len[t] = cigar_ref_len(op);
    const uint64_t c = (uint64_t)op | (uint64_t)ops[(t + 1) & 15u] << 32;
    for (uint32_t n = 0; n < 3; n++) inl[3 * t + n] = cigar_ref_len_inline(c, n);
  }
}

// out[i] = pool_holds(n_pool_words, offs[i], ns[i]) for i < n <= 256
__global__ void __launch_bounds__(256) k_probe_pool_holds(uint64_t n_pool_words, const uint64_t *offs, const uint32_t *ns, int n, uint32_t *out) {
  if ((int)threadIdx.x < n) out[threadIdx.x] = pool_holds(n_pool_words, offs[threadIdx.x], ns[threadIdx.x]) ? 1u : 0u;
}

static int finish(hipStream_t st) {
  hipError_t e = hipGetLastError();
  hipError_t s = hipStreamSynchronize(st);
  return (int)(e != hipSuccess ? e : s);
}

template <int OP, typename T>
static bool wave_widths(hipStream_t st, int width, const void *in, void *out, int n_blocks) {
  const dim3 g((unsigned)n_blocks), b(256);
  switch (width) {
    case 8: hipLaunchKernelGGL((k_probe_wave<OP, T, 8>), g, b, 0, st, (const T *)in, (T *)out); return true;
    case 16: hipLaunchKernelGGL((k_probe_wave<OP, T, 16>), g, b, 0, st, (const T *)in, (T *)out); return true;
    case 32: hipLaunchKernelGGL((k_probe_wave<OP, T, 32>), g, b, 0, st, (const T *)in, (T *)out); return true;
    case 64: hipLaunchKernelGGL((k_probe_wave<OP, T, 64>), g, b, 0, st, (const T *)in, (T *)out); return true;
  }
  return false;
}
template <int C>
static bool top_items(hipStream_t st, int items, uint64_t *tile_sums, int64_t n_tiles, uint64_t *total_out) {
  const dim3 g(1), b(256);
  switch (items) {
    case 8: hipLaunchKernelGGL((k_probe_top<C, 8>), g, b, 0, st, tile_sums, n_tiles, total_out); return true;
    case 32: hipLaunchKernelGGL((k_probe_top<C, 32>), g, b, 0, st, tile_sums, n_tiles, total_out); return true;
  }
  return false;
}
template <typename T>
static bool wave_ops(hipStream_t st, int op, int width, const void *in, void *out, int n_blocks) {
  switch (op) {
    case WOP_SCAN: return wave_widths<WOP_SCAN, T>(st, width, in, out, n_blocks);
    case WOP_SUM: return wave_widths<WOP_SUM, T>(st, width, in, out, n_blocks);
    case WOP_MAX: return wave_widths<WOP_MAX, T>(st, width, in, out, n_blocks);
    case WOP_MIN: return wave_widths<WOP_MIN, T>(st, width, in, out, n_blocks);
    case WOP_OR: return wave_widths<WOP_OR, T>(st, width, in, out, n_blocks);
    case WOP_AND: return wave_widths<WOP_AND, T>(st, width, in, out, n_blocks);
  }
  return false;
}

}  // namespace br

using namespace br;

extern "C" {

int64_t brst_scan_tiles_for(int64_t n) { return scan_tiles_for(n); }
int64_t brst_scan_small_tiles(void) { return SCAN_SMALL_TILES; }

// launch_scan, u32 -> u32 (out64 = 0) or u32 -> u64; total_out may be null
int brst_scan_u32(void *st, const uint32_t *src, int64_t n, uint64_t *tile_sums, void *out, int out64, uint64_t *total_out) {
  launch_scan((hipStream_t)st, src, n, tile_sums, out, out64 != 0, total_out);
  return finish((hipStream_t)st);
}

// launch_scan, u64 in place (no total_out)
int brst_scan_u64_inplace(void *st, uint64_t *a, int64_t n, uint64_t *tmp) {
  launch_scan((hipStream_t)st, a, n, tmp);
  return finish((hipStream_t)st);
}

// launch_scan3 with expand = nullptr; cigar_off and ideal_cap both null or both set; tile_sums: 3 x scan_tiles_for(n) words
int brst_scan3(void *st, int64_t n, const uint32_t *n_matches, const uint32_t *cigar_off, const uint32_t *ideal_cap,
               const uint32_t *fast_flag, uint64_t *tile_sums, uint32_t *match_off, uint64_t *cig_base, uint32_t *fast_pre,
               uint64_t *total_out3) {
  ScanArgs S{};
  S.n = n; S.src32 = n_matches; S.cigar_off = cigar_off; S.ideal_cap = ideal_cap; S.fast_flag = fast_flag; S.tile_sums = tile_sums;
  if (launch_scan3((hipStream_t)st, S, match_off, cig_base, fast_pre, total_out3, nullptr)) return (int)hipErrorUnknown;
  return finish((hipStream_t)st);
}

// load8 / store8 over max(scan_tiles_for(n), 1) tiles; type: 0 u32, 1 u64; dst: n items, sums: 256 words a tile
int brst_copy8(void *st, int type, const void *src, int64_t n, void *dst, uint64_t *sums) {
  const int64_t tiles = scan_tiles_for(n) < 1 ? 1 : scan_tiles_for(n);
  const dim3 g((unsigned)tiles), b(256);
  if (type == 0) hipLaunchKernelGGL((k_probe_copy8<uint32_t>), g, b, 0, (hipStream_t)st, (const uint32_t *)src, n, (uint32_t *)dst, sums);
  else if (type == 1) hipLaunchKernelGGL((k_probe_copy8<uint64_t>), g, b, 0, (hipStream_t)st, (const uint64_t *)src, n, (uint64_t *)dst, sums);
  else return (int)hipErrorInvalidValue;
  return finish((hipStream_t)st);
}

// scan_top_rounds<C, ITEMS> by one block over C arrays of n_tiles sums, in place; total_out (C words) may be null;
// channels: 1 or 3, items: 8 or 32
int brst_top_rounds(void *st, int channels, int items, uint64_t *tile_sums, int64_t n_tiles, uint64_t *total_out) {
  bool ok = false;
  if (channels == 1) ok = top_items<1>((hipStream_t)st, items, tile_sums, n_tiles, total_out);
  else if (channels == 3) ok = top_items<3>((hipStream_t)st, items, tile_sums, n_tiles, total_out);
  if (!ok) return (int)hipErrorInvalidValue;
  return finish((hipStream_t)st);
}

// kth_set_bit64(masks[i], ks[i]) -> out[i] for i < n; every ks[i] is below the population count of masks[i]
int brst_kth_bit(void *st, const uint64_t *masks, const uint32_t *ks, uint32_t *out, int64_t n) {
  if (n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_kth_bit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)st, masks, ks, out, n);
  return finish((hipStream_t)st);
}

// wave_turns by one block of 256: flag and val hold 256 words, lists 4 x 64 x 3, counts 4
int brst_wave_turns(void *st, const uint32_t *flag, const uint32_t *val, uint32_t *lists, uint32_t *counts) {
  hipLaunchKernelGGL(k_probe_turns, dim3(1), dim3(256), 0, (hipStream_t)st, flag, val, lists, counts);
  return finish((hipStream_t)st);
}

// wave_cigar_ref_len over n_cigars pooled CIGARs (the caller keeps them inside the pool) and the op tables over the 16 words of
// ops, by one block of 256: sums and same hold n_cigars items, tab and tab_len 16, inl 48
int brst_cigar(void *st, const uint32_t *pool, const uint64_t *offs, const uint32_t *ns, int n_cigars, uint64_t *sums, uint32_t *same,
               const uint32_t *ops, uint32_t *tab, uint64_t *tab_len, uint64_t *inl) {
  if (n_cigars < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_cigar, dim3(1), dim3(256), 0, (hipStream_t)st, pool, offs, ns, n_cigars, sums, same, ops, tab, tab_len, inl);
  return finish((hipStream_t)st);
}

// pool_holds(n_pool_words, offs[i], ns[i]) -> out[i] for i < n <= 256
int brst_pool_holds(void *st, uint64_t n_pool_words, const uint64_t *offs, const uint32_t *ns, int n, uint32_t *out) {
  if (n < 1 || n > 256) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_pool_holds, dim3(1), dim3(256), 0, (hipStream_t)st, n_pool_words, offs, ns, n, out);
  return finish((hipStream_t)st);
}

// op: 0 scan, 1 sum, 2 max, 3 min, 4 or, 5 and; type: 0 u32, 1 u64, 2 double (sum only); width: 8, 16, 32, 64;
// in and out hold n_blocks * 256 values
int brst_wave(void *st, int op, int type, int width, const void *in, void *out, int n_blocks) {
  bool ok = false;
  if (n_blocks < 1) return (int)hipErrorInvalidValue;
  if (type == 0) ok = wave_ops<uint32_t>((hipStream_t)st, op, width, in, out, n_blocks);
  else if (type == 1) ok = wave_ops<uint64_t>((hipStream_t)st, op, width, in, out, n_blocks);
  else if (type == 2 && op == WOP_SUM) ok = wave_widths<WOP_SUM, double>((hipStream_t)st, width, in, out, n_blocks);
  if (!ok) return (int)hipErrorInvalidValue;
  return finish((hipStream_t)st);
}

// block_excl_scan_256 three times through one sh[4]; type: 0 u32, 1 u64; in, out, tot: 3 * n_blocks * 256 values each
int brst_block_scan(void *st, int type, const void *in, void *out, void *tot, int n_blocks) {
  const dim3 g((unsigned)n_blocks), b(256);
  if (n_blocks < 1) return (int)hipErrorInvalidValue;
  if (type == 0) hipLaunchKernelGGL((k_probe_block_scan<uint32_t>), g, b, 0, (hipStream_t)st, (const uint32_t *)in, (uint32_t *)out, (uint32_t *)tot);
  else if (type == 1) hipLaunchKernelGGL((k_probe_block_scan<uint64_t>), g, b, 0, (hipStream_t)st, (const uint64_t *)in, (uint64_t *)out, (uint64_t *)tot);
  else return (int)hipErrorInvalidValue;
  return finish((hipStream_t)st);
}

// block_bits per block: out[2 * block] = OR of o, out[2 * block + 1] = AND of a.  With out2, a second launch right behind the
// first writes there (no synchronisation between the two).
int brst_block_bits(void *st, const uint64_t *o, const uint64_t *a, uint64_t *out, uint64_t *out2, int n_blocks) {
  const dim3 g((unsigned)n_blocks), b(256);
  if (n_blocks < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_block_bits, g, b, 0, (hipStream_t)st, o, a, out);
  if (out2) hipLaunchKernelGGL(k_probe_block_bits, g, b, 0, (hipStream_t)st, o, a, out2);
  return finish((hipStream_t)st);
}

}  // extern "C"
