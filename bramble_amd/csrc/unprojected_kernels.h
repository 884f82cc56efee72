// The input records that no transcript accepted (unprojected_kernels.hip; host side: unprojected.cpp, which holds the
// pipeline's description).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

// the device words of a call (UnprojArgs::small), read back in one copy
enum { UNPROJ_BYTES = 0, UNPROJ_RECORDS = 1, UNPROJ_NAMES_NONE = 2, UNPROJ_NAMES_PART = 3, UNPROJ_SMALL_N = 4 };

struct UnprojArgs {
  int64_t n_aln, n_rows, n_groups;
  const uint8_t *blob;       // the input records, BAM layout from refID on
  const uint64_t *rec_off;   // [n_aln + 1] (or [n_aln] with rec_len)
  const uint32_t *rec_len;   // [n_aln] or null: rec_off[i + 1] - rec_off[i]
  const uint4 *r_rec;        // the detail column the encoder reads: the input alignment of row r is word rec_x ? 0 : 1 of r_rec[r]
  int32_t rec_x;
  const uint32_t *group_off; // [n_groups + 1] the read-name groups
  int32_t scope;             // 1: record, 2: name
  uint8_t *flag;             // [n_aln] zeroed; 1: the alignment has an output record (scope name: or another of its name has)
  uint64_t *small;           // UNPROJ_*: the two name counters zeroed before the names kernel, the two totals left by the scans
  uint32_t *len;             // [n_aln] 4 + block_size of an unprojected record, else 0 -> out_off, its exclusive scan
  uint32_t *one;             // [n_aln] 1 for an unprojected record, else 0              -> rank, its exclusive scan
  const uint64_t *out_off;   // [n_aln + 1]
  const uint32_t *rank;      // [n_aln + 1]
  // the gather
  uint8_t *arena;            // the context's arena; this call's records begin at arena_base
  uint64_t arena_base;
  uint64_t *off;             // the arena's offset table from this call's first entry on (n_new + 1 entries are written)
  uint64_t n_new, new_bytes; // the scans' totals (read back by the host)
};

void launch_unproj_mark(hipStream_t st, const UnprojArgs &A);    // flag
void launch_unproj_names(hipStream_t st, const UnprojArgs &A);   // the name counters; scope name: flag rewritten per read name
void launch_unproj_size(hipStream_t st, const UnprojArgs &A);    // len, one
// lanes: 16, 32 or 64 lanes copy one record; grid-stride over at most 8 blocks a compute unit
void launch_unproj_gather(hipStream_t st, const UnprojArgs &A, int lanes, int n_cu);

}  // namespace br
