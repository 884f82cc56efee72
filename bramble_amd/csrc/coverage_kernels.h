// Per-base transcript coverage on the device: rows -> interval events -> depth -> per-transcript summary and runs
// (coverage_kernels.hip; host side: coverage.cpp, which holds the pipeline's description).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "names.h"

namespace br {

constexpr uint32_t COV_SMALL_OPS = 64;      // a CIGAR of up to this many ops is one lane's walk in k_cov_add, a longer one the wave's
constexpr int64_t COV_TILE = 4096;          // bases a block of 256 takes in the scan, the head count and the run writer (4 x uint4 a lane)
constexpr int64_t COV_WAVE_LEN = 16384;     // a transcript of up to this many bases is a wave's work in the summary, a longer one a block's
constexpr unsigned COV_LONG_GRID = 1024;    // blocks that walk the transcripts above COV_WAVE_LEN
// words of the counters
enum { CV_COUNTED = 0, CV_SKIPPED = 1, CV_CLIPPED = 2, CV_BAD_POOL = 3, CV_BAD_TID = 4, CV_WORDS = 8 };

// One add: the rows [r_first, r_last) of the caller's table.  a and cigar may be slices (a host add uploads only its rows): row r of
// the caller's table is at [r - bias] here.
struct CovAddArgs {
  const uint4 *a; const uint64_t *cigar; int64_t bias;   // br_row_a, the CIGAR references
  const uint32_t *pool; uint64_t n_pool_words;
  uint64_t r_first, r_last;
  int64_t n_tx; const uint64_t *off;                     // off[t] = the first base of transcript t among the B bases; off[n_tx] = B
  uint32_t primary_only;
  uint32_t *diff;                                        // B + 1 words: + 1 where an interval begins, - 1 (mod 2^32) where it ends
  unsigned long long *records;                           // per transcript
  unsigned long long *counters;                          // CV_*
};
void launch_cov_add(hipStream_t st, const CovAddArgs &A);

// depth[0, n) <- its inclusive prefix sums modulo 2^32, in place.  tile_sum: n / COV_TILE + 2 words, scan_tmp: what launch_scan
// (scan_kernels.h) needs for that many
void launch_cov_scan(hipStream_t st, uint32_t *depth, int64_t n, uint64_t *tile_sum, uint64_t *scan_tmp);
// per transcript: the sum, the number of non-zero entries and the maximum of depth[off[t], off[t + 1])
void launch_cov_summary(hipStream_t st, const uint32_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned, uint64_t *covered,
                        uint32_t *max_depth);
// tile_cnt[k] = the run heads among the bases of tile k (a base of depth > 0 that is its transcript's first or differs from the
// base in front of it)
void launch_cov_count(hipStream_t st, const uint32_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt);
// tile_cnt scanned (exclusive): run k is (transcript, start, end, depth); the head's lane stores the first two words, the lane of
// the run's last base the other two
void launch_cov_runs(hipStream_t st, const uint32_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *runs);

// ---- the weighted modes ("weight" = 1, 2; definitions: bramble_amd.h, br_coverage).  A depth word is uint64, one unit is 2^32 ----
// more words of the counters: rows with nh == 0 (weight nh), rows whose name the offsets do not give (weight em), entries kept
// by all adds so far, entries of the add that runs; and what the apply met: a name past the count, a class past C or none at all,
// a transcript that is not in the class, an entry that leaves the bases
enum { CV_BAD_NH = 5, CV_BAD_NAMES = 6, CV_KEPT = 7, CV_ADD_ENTRIES = 8, CV_BAD_NAME = 9, CV_BAD_CLASS = 10, CV_BAD_LABEL = 11, CV_BAD_ENTRY = 12,
       CV_WORDS_W = 16 };
// A kept entry (weight em), 16 bytes: x | y << 32 = the absolute first base (below 2^40) with COV_KEEP_FIRST set on the first entry
// of its row, z = the length, w = the add-order name index.  A counted row without a clamped, non-empty interval leaves one entry of
// length 0 whose x is its transcript id: its weight still counts in weight_sum
constexpr uint64_t COV_KEEP_FIRST = 1ull << 63;
constexpr uint64_t COV_KEEP_MAX_BASES = 1ull << 40;
enum { COV_ADD_NH = 1, COV_ADD_COUNT = 2, COV_ADD_KEEP = 3 };
struct CovAddWArgs {
  CovAddArgs A;                      // (A.diff is not used; A.counters has CV_WORDS_W words)
  unsigned long long *diff;          // B + 1 words of 64 bits
  unsigned long long *weight_sum;    // per transcript (COV_ADD_NH)
  // COV_ADD_COUNT / COV_ADD_KEEP: entries per row of the add, at [r - r_first]; the count pass writes them and leaves their sum
  // in counters[CV_ADD_ENTRIES], the keep pass places a wave's entries by one atomic on counters[CV_KEPT]
  uint32_t *row_entries;
  uint4 *arena; uint64_t arena_cap;
  // the names of the add (names.h; their rows are A's [r_first, r_last)): row r belongs to alignment a with row_off[a] <= r <
  // row_off[a + 1], a to name g with group_off[g] <= a < group_off[g + 1]; its add-order index is name_base + g
  NameWindow names; uint64_t name_base;
};
void launch_cov_add_w(hipStream_t st, const CovAddWArgs &W, int mode);
// the kept entries [0, n) applied to diff with the quantifier's posteriors; every index taken from a table is checked first
struct CovApplyArgs {
  const uint4 *arena; uint64_t n;
  const uint64_t *off; int64_t n_tx; uint64_t n_bases;
  const uint32_t *name_cls; uint64_t n_names;
  const uint64_t *label_off; const uint32_t *labels; uint64_t n_cls, n_lab;
  const double *post;
  unsigned long long *diff, *weight_sum, *counters;
};
void launch_cov_apply(hipStream_t st, const CovApplyArgs &P);
// launch_cov_scan / summary / count / runs over 64-bit words, modulo 2^64.  The summary: the sums of the high and of the low words
// of the depth.  A run is 24 bytes: (transcript, start, end, 0) in run4[k] and the depth in run_depth[k]
void launch_cov_scan64(hipStream_t st, uint64_t *depth, int64_t n, uint64_t *tile_sum, uint64_t *scan_tmp);
void launch_cov_summary64(hipStream_t st, const uint64_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned_hi, uint64_t *aligned_lo,
                          uint64_t *covered, uint64_t *max_depth);
void launch_cov_count64(hipStream_t st, const uint64_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt);
void launch_cov_runs64(hipStream_t st, const uint64_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *run4,
                       uint64_t *run_depth);

}  // namespace br
