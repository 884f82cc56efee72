// The single-value exclusive scan (scan_kernels.hip): every prefix sum of one array in the library goes through it.
//
// A tile is 256 threads x SCAN_ITEMS items, read and written with 16-byte accesses.  Up to SCAN_SMALL_TILES tiles are one
// launch (one block, tile after tile with a carry); more are three: the tile sums, their scan by one block (2048 sums a
// round), and the tiles again with their offsets.  The fused scans of the projection (k_scan3_*, k_scan5_*) have the same
// shape and take it from here and from wave_inl.h.
//
// Scratch: scan_tiles_for(n) 64-bit words (tile_sums / tmp below), not touched up to SCAN_SMALL_TILES tiles;
// scan_scratch_bytes(n) is what the callers allocate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

constexpr int SCAN_ITEMS = 8;                   // load8 / store8 and the kernels' register arrays are written for eight
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;
constexpr int SCAN_SMALL_TILES = 4;

inline int64_t scan_tiles_for(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
// bytes of scratch for a scan of n items (never 0: the buffers that hold it are allocated for any n)
inline size_t scan_scratch_bytes(int64_t n) { return (size_t)(scan_tiles_for(n) + 1) * 8; }

// out[i] = src[0] + ... + src[i - 1] for i in [0, n], so out has n + 1 entries and out[n] is the total; out64: out is
// uint64_t[], else uint32_t[] (the sums modulo 2^32).  *total_out gets the 64-bit total as well.
void launch_scan(hipStream_t st, const uint32_t *src, int64_t n, uint64_t *tile_sums, void *out, bool out64, uint64_t *total_out);

// The same in place: a[0, n) -> its exclusive prefix sums, a[n] = the total.  In place is safe because a thread reads its
// eight items before it writes them and no thread reads another's (a[n] is only written).  a may be any 8-byte aligned
// address: an offset into a larger allocation takes the item-by-item path of load8 / store8.
void launch_scan(hipStream_t st, uint64_t *a, int64_t n, uint64_t *tmp);

}  // namespace br
