// The bigWig of a finished br_coverage, on the device (bigwig_kernels.hip; host side: bigwig.cpp, which holds the pipeline's
// description; the definitions are in bramble_amd.h, br_coverage_bigwig).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

constexpr uint32_t BW_MAX_PAYLOAD = 131072;   // bytes of one zlib section: 4096 zoom records of 32 bytes
constexpr uint32_t BW_ADLER_CHUNK = 256;      // a lane's bytes in the Adler-32 of a payload of up to 16384 bytes (more: n / 64, rounded up to 4)
constexpr uint32_t BW_SEGMENT = 32768;        // the parse sees this many bytes at a time (deflate_inl.h: 16-bit table entries)
constexpr unsigned BW_TOTAL_BLOCKS = 256;     // blocks of the total summary: one partial each, summed on the host in order

// Stream i is written into a slot of its own before its size is known: the slots begin here.  A slot takes the fixed code's worst case
// (9 bits a byte, 10 more, 6 bytes of frame) and the stored form (5 bytes a block of 65535, 6 of frame)
__host__ __device__ inline uint64_t bw_slot_off(uint64_t off, uint64_t i) { return off + (off >> 3) + 32 * i; }

// first[t] = the first run whose transcript is >= t, for t in [0, n_tx] (the runs are ordered by transcript)
void launch_bw_run_first(hipStream_t st, const uint4 *runs, uint64_t n_runs, int64_t n_tx, uint64_t *first);

// The sections of the full data.  Chromosome c (in chromId order) owns the runs run0[c] + [0, cum[c + 1] - cum[c]) and the
// sections sec0[c] .. sec0[c + 1]: S runs each, the last shorter.  Section s begins at raw_off[s] = 24 s + 12 (runs in front of
// it) in `raw`; raw_off has n_sec + 1 entries.  The section kernel writes the headers, raw_off and the bounds lo[s] = chromId << 32 |
// first start, hi[s] = chromId << 32 | last end; the pack kernel the items, a lane per run.
struct BwPackArgs {
  const uint4 *runs; const uint64_t *run_depth;   // run_depth: the weighted modes (NULL: the depth is runs[r].w)
  uint64_t n_runs, n_sec, n_chrom; uint32_t S;
  const uint64_t *run0, *cum, *sec0;              // n_chrom, n_chrom + 1, n_chrom + 1
  uint8_t *raw; uint64_t *raw_off, *lo, *hi;
};
void launch_bw_sections(hipStream_t st, const BwPackArgs &A);
void launch_bw_pack(hipStream_t st, const BwPackArgs &A);

// The total summary from the runs: partial[5 b ..] = covered bases, least depth, greatest depth (integers), and as doubles' bits the
// sum of value x length and of value^2 x length, of block b's runs (thread k of the grid takes runs k, k + grid, ...)
void launch_bw_total(hipStream_t st, const uint4 *runs, const uint64_t *run_depth, uint64_t n_runs, uint64_t *partial);

// One zoom level: window w of chromosome c (win0[c] <= w < win0[c + 1]) is the bases [(w - win0[c]) R, ...) of transcript tid[c].
// G lanes (a power of two up to 64) take a window; rec[w] = its 32-byte record, flag[w] = 1 where it has a covered base.
struct BwZoomArgs {
  const void *depth; int wide;                    // uint32 words, or uint64 (wide) in units of 2^-32
  const uint64_t *off;                            // the transcripts' first bases (br_coverage's off)
  const uint32_t *tid; const uint64_t *win0; uint64_t n_chrom, n_win;
  uint32_t R; int G;
  uint4 *rec; uint64_t *flag;
};
void launch_bw_zoom_windows(hipStream_t st, const BwZoomArgs &A);
// flag scanned (exclusive): the records of the flagged windows, in order
void launch_bw_zoom_compact(hipStream_t st, const uint4 *rec, const uint64_t *pos, uint64_t n_win, uint4 *out);
// block b = records [b S, min((b + 1) S, n)): off[b] = 32 b S (n_blocks + 1 entries), lo[b], hi[b] as for the sections
void launch_bw_zoom_blocks(hipStream_t st, const uint4 *rec, uint64_t n_rec, uint32_t S, uint64_t n_blocks, uint64_t *off, uint64_t *lo, uint64_t *hi);

// zlib streams: payload i = src[off[i] .. off[i + 1]) (at most BW_MAX_PAYLOAD bytes) -> slots + bw_slot_off(off[i], i), sizes[i]
// bytes.  mode 0: one fixed-code block, or stored where that is not smaller than the payload; 1: stored.  One wave a payload.
void launch_bw_zlib(hipStream_t st, const uint8_t *src, const uint64_t *off, uint64_t n, int mode, uint8_t *slots, uint64_t *sizes);
// pos = sizes scanned: stream i from its slot to dst + pos[i]
void launch_bw_gather(hipStream_t st, const uint8_t *slots, const uint64_t *off, const uint64_t *pos, uint64_t n, uint8_t *dst);

// One level of an R-tree.  lo / hi: the bounds of the level's n items.  reduce: the bounds of its ceil(n / bs) nodes.  nodes: the
// level's nodes at `out` (4 + bs x item bytes each, the unused tail zero).  A leaf item (32 bytes) points at data_base + pos[i],
// pos[i + 1] - pos[i] bytes; an inner item (24 bytes) at child_off + i x child_size.
void launch_bw_tree_reduce(hipStream_t st, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t bs, uint64_t *lo_out, uint64_t *hi_out);
struct BwNodeArgs {
  const uint64_t *lo, *hi; uint64_t n; uint32_t bs; int leaf;
  const uint64_t *pos; uint64_t data_base;        // leaf
  uint64_t child_off, child_size;                 // inner
  uint64_t n_nodes;                               // ceil(n / bs), 1 for an empty tree
  uint8_t *out;
};
void launch_bw_tree_nodes(hipStream_t st, const BwNodeArgs &A);

}  // namespace br
