// The single-value exclusive scan: see scan_kernels.h for its shape, its scratch and why it may run in place.
#include <hip/hip_runtime.h>

#include "scan_kernels.h"
#include "wave_inl.h"

namespace br {

template <typename InT>
__global__ void __launch_bounds__(256) k_scan_tiles(const InT *src, int64_t n, uint64_t *tile_sums) {
  __shared__ uint64_t sh[4];
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  InT v[SCAN_ITEMS];
  load8(src, base, n, v);
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) sum += v[k];
  uint64_t tot;
  block_excl_scan_256(sum, sh, tot);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) k_scan_top(uint64_t *tile_sums, int64_t n_tiles, uint64_t *total_out) {
  __shared__ uint64_t sh[4];
  scan_top_rounds<1, 8>(tile_sums, n_tiles, total_out, sh);
}

// (src == out for the scan in place: the thread's items are in v before store8 writes them)
template <typename InT, typename OutT>
__global__ void __launch_bounds__(256) k_scan_apply(const InT *src, int64_t n, const uint64_t *tile_sums, OutT *out) {
  __shared__ uint64_t sh[4];
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  InT v[SCAN_ITEMS];
  load8(src, base, n, v);
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) sum += v[k];
  uint64_t tot;
  uint64_t ex = block_excl_scan_256(sum, sh, tot) + tile_sums[blockIdx.x];
  OutT o[SCAN_ITEMS];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) { o[k] = (OutT)ex; ex += v[k]; }
  store8(out, base, n, o);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) out[n] = (OutT)ex;
}

// Small inputs (at most SCAN_SMALL_TILES tiles): the whole scan by ONE block, tile after tile with a running carry -- one
// launch instead of three (tile sums, their scan, apply): what a batch of a few thousand alignments spends its time on is
// launches, not bytes.
template <typename InT, typename OutT>
__global__ void __launch_bounds__(256) k_scan_small(const InT *src, int64_t n, OutT *out, uint64_t *total_out) {
  __shared__ uint64_t sh[4];
  uint64_t carry = 0;
  for (int64_t t0 = 0; t0 < n || t0 == 0; t0 += SCAN_TILE) {
    const int64_t base = t0 + (int64_t)threadIdx.x * SCAN_ITEMS;
    InT v[SCAN_ITEMS];
    load8(src, base, n, v);
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) sum += v[k];
    uint64_t tot;
    uint64_t ex = block_excl_scan_256(sum, sh, tot) + carry;
    OutT o[SCAN_ITEMS];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { o[k] = (OutT)ex; ex += v[k]; }
    store8(out, base, n, o);
    carry += tot;
  }
  if (threadIdx.x == 0) { out[n] = (OutT)carry; if (total_out) total_out[0] = carry; }
}

template <typename InT, typename OutT>
static void scan(hipStream_t st, const InT *src, int64_t n, uint64_t *tile_sums, OutT *out, uint64_t *total_out) {
  int64_t tiles = scan_tiles_for(n);
  if (tiles < 1) tiles = 1;
  dim3 g((unsigned)tiles), b(256);
  if (tiles <= SCAN_SMALL_TILES) { hipLaunchKernelGGL((k_scan_small<InT, OutT>), dim3(1), b, 0, st, src, n, out, total_out); return; }
  hipLaunchKernelGGL((k_scan_tiles<InT>), g, b, 0, st, src, n, tile_sums);
  hipLaunchKernelGGL(k_scan_top, dim3(1), b, 0, st, tile_sums, tiles, total_out);
  hipLaunchKernelGGL((k_scan_apply<InT, OutT>), g, b, 0, st, src, n, (const uint64_t *)tile_sums, out);
}

void launch_scan(hipStream_t st, const uint32_t *src, int64_t n, uint64_t *tile_sums, void *out, bool out64, uint64_t *total_out) {
  if (out64) scan(st, src, n, tile_sums, (uint64_t *)out, total_out);
  else scan(st, src, n, tile_sums, (uint32_t *)out, total_out);
}

void launch_scan(hipStream_t st, uint64_t *a, int64_t n, uint64_t *tmp) {
  scan(st, (const uint64_t *)a, n, tmp, a, (uint64_t *)nullptr);
}

}  // namespace br
