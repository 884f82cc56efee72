// The field sort's kernels (barcode_kernels.hip; host side: barcode_sort.h).  A field is a UMI or a cell barcode as barcode_inl.h
// leaves it: four 64-bit words, bytes in comparison order, zero padded, and its length.  The cells, the whitelist and br_dedup sort
// the items of a table of such fields and cut the sorted items where the field changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

// idx[pos[i]] = i for the items whose flag was set (pos: the scanned flags, n + 1 entries)
void launch_bc_compact(hipStream_t st, const uint64_t *pos, int64_t n, uint32_t *idx);
// key[j] = word w of the field of idx[j] (w = 0 .. 3); w = 4: its length, under the item's group (gid[idx[j]] << 8) where gid != NULL
void launch_bc_key(hipStream_t st, const uint32_t *idx, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int64_t n, int w, uint64_t *key);
// head[j] = sorted item j starts a run: its field -- and, gid != NULL, its group -- differs from item j - 1's; empty_is_head: or it
// has no field (items without one never share a run)
void launch_bc_heads(hipStream_t st, const uint32_t *idx, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int empty_is_head, int64_t n,
                     uint64_t *head);

}  // namespace br
