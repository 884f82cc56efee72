// Collation of device-resident records by read name (collate_kernels.hip; host side: collate.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

constexpr int COL_TILE = 2048;   // items per radix tile: 256 threads x 8 rounds

// append: bytes[i] = 4 + rec_len[i] (rec_len NULL: rec_off[i + 1] - rec_off[i])
void launch_col_lens(hipStream_t st, const uint64_t *rec_off, const uint32_t *rec_len, int64_t n, uint64_t *bytes);
// append: record i ([block_size][record], from rec_off[i] - 4) -> arena[base + dst[i] ..); off_out[i] / len_out[i] its table entry
void launch_col_copy(hipStream_t st, const uint8_t *blob, const uint64_t *rec_off, const uint32_t *rec_len, int64_t n,
                     const uint64_t *dst, uint64_t base, uint8_t *arena, uint64_t *off_out, uint32_t *len_out);
// key: key[i] = hash(name of record i) & mask, idx[i] = i; bits[0] = OR, bits[1] = AND over all keys (part: a block's)
// part: 2 words per block of 256
void launch_col_key(hipStream_t st, const uint8_t *arena, const uint64_t *off, int64_t n, uint64_t mask, uint64_t *key,
                    uint32_t *idx, uint64_t *part, uint64_t *bits);
// bits[0] = OR, bits[1] = AND of the blocks' (OR, AND) pairs in part (the coordinate sort's keys go through the same reduction)
void launch_col_bits(hipStream_t st, const uint64_t *part, int64_t blocks, uint64_t *bits);
// one stable LSD pass over the 8-bit digit at `shift`: hist = 256 x n_tiles (digit-major), tmp: scan_tiles_for(256 * n_tiles) words, for its scan
void launch_col_radix_pass(hipStream_t st, const uint64_t *key_in, const uint32_t *idx_in, uint64_t *key_out, uint32_t *idx_out,
                           int64_t n, int shift, uint64_t *hist, uint64_t *tmp);
// runs: head[j] = 1 where sorted item j starts a read-name group (key or name differs from item j - 1); *n_coll = adjacent
// pairs with equal keys and different names; their runs' [begin, end) go to runs[0 .. *n_runs) (up to cap; duplicates possible)
void launch_col_heads(hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint64_t *key, const uint32_t *idx, int64_t n,
                      uint64_t *head, unsigned long long *n_coll, unsigned long long *n_runs, uint64_t *runs, uint64_t cap);
// the name bytes of records list[0 .. m): slot k = 256 bytes (l_read_name, then the name)
void launch_col_names(hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint32_t *list, int64_t m, uint8_t *slots);
// place: gid = exclusive scan of the head flags (n + 1), G groups
void launch_col_gbeg(hipStream_t st, const uint64_t *gid, int64_t n, uint64_t *gbeg);
void launch_col_head_count(hipStream_t st, const uint64_t *gbeg, const uint32_t *idx, int64_t g, uint64_t *hc);
void launch_col_place(hipStream_t st, const uint64_t *gid, const uint64_t *gbeg, const uint64_t *start, const uint32_t *idx,
                      const uint64_t *off, const uint32_t *len, int64_t n, uint64_t *out_off, uint32_t *out_len, uint32_t *out_idx,
                      uint64_t *mark);
void launch_col_starts(hipStream_t st, const uint64_t *mark_scan, int64_t n, uint64_t *starts);
// cut: *res = the first starts[k] >= target (starts[g] = n)
void launch_col_cut(hipStream_t st, const uint64_t *starts, int64_t g, uint64_t target, uint64_t *res);

}  // namespace br
