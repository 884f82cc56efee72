// Coordinate sort of device-resident projected records and their BAI index (sort_kernels.hip; host side: sort.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

constexpr uint64_t SORT_NO_BIN = ~0ull;         // (refID, bin) key of a record that is in no bin
constexpr uint32_t SORT_END_MAX = 0x7fffffffu;  // ends[]: bit 31 = flag 0x4, the rest = min(end, this)
#ifndef SORT_GATHER_LANES
#define SORT_GATHER_LANES 64   // lanes that copy one record in k_sort_gather (8 .. 64, a power of two).  64 is what profiles/sort records;
                               // 32 and 16 were faster in profiles/sort/gather_lanes.txt and wait for a profile of their own
#endif
constexpr uint32_t BAI_MAX_END = 1u << 29;      // the binning scheme's reach
constexpr uint32_t BAI_ERR_RANGE = 1, BAI_ERR_BLOCKS = 2, BAI_ERR_REF = 4;   // k_bai_rec's error bits

// add: off[i] = base + row_off[i] - row_off[0] for i in [0, m] (the last entry is the arena's new end); *bad = 1 when row_off
// descends somewhere
void launch_sort_offs(hipStream_t st, const uint64_t *row_off, int64_t m, uint64_t base, uint64_t *off, uint32_t *bad);
// key: record i = arena[off[i], off[i + 1]) as [block_size][record].  key[i] = (u32)refID << 32 | (u32)(pos + 1) << 1 | reverse,
// idx[i] = i, ends[i] = end of the alignment on the reference (pos + the CIGAR's M D N = X lengths, pos + 1 without any) and the
// unmapped flag; bits[0] = OR, bits[1] = AND over all keys (part: 2 words per block of 256); *bad = 1 when a record has a pos below
// -1 or of 2^31 - 1
void launch_sort_key(hipStream_t st, const uint8_t *arena, const uint64_t *off, int64_t n, uint64_t *key, uint32_t *idx, uint32_t *ends,
                     uint64_t *part, uint64_t *bits, uint32_t *bad);
// len[j] = bytes of sorted record j (its exclusive scan is the sorted stream's offset table)
void launch_sort_lens(hipStream_t st, const uint64_t *off, const uint32_t *idx, int64_t n, uint64_t *len);
// cut: res[0] = the largest e in (cur, n] with s_off[e] - s_off[cur] <= max_bytes, or cur + 1; res[1] = s_off[e] - s_off[cur]
void launch_sort_cut(hipStream_t st, const uint64_t *s_off, int64_t n, int64_t cur, uint64_t max_bytes, uint64_t *res);
// gather: sorted records [cur, e) -> dst, contiguous; row_off[j - cur] = their offsets in dst (e - cur + 1 entries).  The arena is
// read up to 7 bytes past a record's end (whole 8-byte words): it keeps that slack
void launch_sort_gather(hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint32_t *idx, const uint64_t *s_off, int64_t cur,
                        int64_t e, uint8_t *dst, uint64_t *row_off);

// ---- the index ----
struct BaiRef {   // one reference
  uint64_t jb, je;     // its records with a position, in the sorted order
  uint64_t bin0, chunk0, n_bin, n_chunk;   // its first bin / chunk among all, and how many
  uint64_t n_intv;
};
struct BaiArgs {
  int64_t n; int32_t n_ref;
  const uint64_t *key; const uint32_t *idx; const uint32_t *ends; const uint64_t *s_off;   // the sorter's tables
  const uint64_t *blk; int64_t n_blk; uint64_t eof_coffset;   // blk: (coffset, uoffset) pairs
  uint64_t *vo;        // n + 1 virtual offsets
  uint64_t *key2[2]; uint32_t *idx2[2]; int cur;   // (refID << 32 | bin, sorted index): before / after the radix passes
  uint64_t *um;        // n + 1: flag 0x4, then its exclusive scan
  uint64_t *bh, *ch;   // bin heads and chunk heads in (refID, bin) order, then their exclusive scans: n + 1 entries are used
                       // (the scan's total is the last), sort.cpp allocates n + 2
  uint64_t *binc0;     // first chunk of every bin, then the number of chunks: at most n + 1 entries, n + 2 allocated
  uint32_t *refmax;    // largest end per reference
  BaiRef *ref; uint64_t *lin_off, *ref_pos;   // n_ref (+ 1): the reference's first window / byte (exclusive scans)
  uint64_t *lin;       // the windows
  uint64_t *part, *small;   // small: [0] OR [1] AND of key2, [2] records without coordinate, [3] error bits
  uint8_t *out;
};
void launch_bai_rec(hipStream_t st, const BaiArgs &A);     // vo, key2 / idx2 [0], um, refmax, small
void launch_bai_heads(hipStream_t st, const BaiArgs &A);   // bh, ch (flags)
void launch_bai_binc0(hipStream_t st, const BaiArgs &A);   // after the scans of bh and ch
void launch_bai_refs(hipStream_t st, const BaiArgs &A);    // ref[], lin_off / ref_pos (sizes, to be scanned)
void launch_bai_lin(hipStream_t st, const BaiArgs &A);     // lin (filled with ~0 before)
void launch_bai_write(hipStream_t st, const BaiArgs &A);   // the file image

}  // namespace br
