// Per-base transcript coverage on the device: rows -> interval events -> depth -> per-transcript summary and runs
// (coverage_kernels.hip; host side: coverage.cpp, which holds the pipeline's description).  One pipeline for the three weights
// (bramble_amd.h, br_coverage): a depth word W is uint32_t and one row one unit (weight 0), or uint64_t and one unit 2^32 (weights
// nh and em); the add has a mode per way of ending an interval, everything behind it is a template on W.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "names.h"

namespace br {

constexpr uint32_t COV_SMALL_OPS = 64;      // a CIGAR of up to this many ops is one lane's walk in k_cov_add, a longer one the wave's
constexpr int64_t COV_TILE = 4096;          // bases a block of 256 takes in the scan, the head count and the run writer (4 x 4 words a lane)
constexpr int64_t COV_WAVE_LEN = 16384;     // a transcript of up to this many bases is a wave's work in the summary, a longer one a block's
constexpr unsigned COV_LONG_GRID = 1024;    // blocks that walk the transcripts above COV_WAVE_LEN
// Words of the counters.  Weight 0 has the first CV_WORDS of them, the weighted modes CV_WORDS_W: rows with nh == 0 (weight nh),
// rows whose name the offsets do not give (weight em), entries kept by all adds so far, entries of the add that runs; and what the
// apply met: a name past the count, a class past C or none at all, a transcript that is not in the class, an entry that leaves the
// bases
enum { CV_COUNTED = 0, CV_SKIPPED = 1, CV_CLIPPED = 2, CV_BAD_POOL = 3, CV_BAD_TID = 4, CV_WORDS = 8 };
enum { CV_BAD_NH = 5, CV_BAD_NAMES = 6, CV_KEPT = 7, CV_ADD_ENTRIES = 8, CV_BAD_NAME = 9, CV_BAD_CLASS = 10, CV_BAD_LABEL = 11, CV_BAD_ENTRY = 12,
       CV_WORDS_W = 16 };

// A kept entry (weight em), 16 bytes: x | y << 32 = the absolute first base (below 2^40) with COV_KEEP_FIRST set on the first entry
// of its row, z = the length, w = the add-order name index.  A counted row without a clamped, non-empty interval leaves one entry of
// length 0 whose x is its transcript id: its weight still counts in weight_sum
constexpr uint64_t COV_KEEP_FIRST = 1ull << 63;
constexpr uint64_t COV_KEEP_MAX_BASES = 1ull << 40;

// What the add does with a clamped, non-empty interval [at, at + len) of the B bases:
//   COV_ADD_UNIT   + 1 at diff[at], - 1 (mod 2^32) at diff[at + len], diff in 32-bit words (weight 0)
//   COV_ADD_NH     + q / - q (mod 2^64) in 64-bit words, q = 2^32 / nh rounded, and q into weight_sum (weight nh)
//   COV_ADD_COUNT  nothing but counting: row_entries and counters[CV_ADD_ENTRIES] (weight em, whose q is not known yet, runs the
//   COV_ADD_KEEP   add twice: once the host has made room, the second pass keeps the entries in the arena)
enum { COV_ADD_UNIT = 0, COV_ADD_NH = 1, COV_ADD_COUNT = 2, COV_ADD_KEEP = 3 };

// One add, the part every mode has: the rows [r_first, r_last) of the caller's table.  a and cigar may be slices (a host add uploads
// only its rows): row r of the caller's table is at [r - bias] here.
struct CovAddArgs {
  const uint4 *a; const uint64_t *cigar; int64_t bias;   // br_row_a, the CIGAR references
  const uint32_t *pool; uint64_t n_pool_words;
  uint64_t r_first, r_last;
  int64_t n_tx; const uint64_t *off;                     // off[t] = the first base of transcript t among the B bases; off[n_tx] = B
  uint32_t primary_only;
  void *diff;                                            // B + 1 words of the mode's width (COV_ADD_UNIT, COV_ADD_NH)
  unsigned long long *records;                           // per transcript
  unsigned long long *counters;                          // CV_*: CV_WORDS words for COV_ADD_UNIT, else CV_WORDS_W
};
struct CovAddWArgs {
  CovAddArgs A;
  unsigned long long *weight_sum;    // per transcript (COV_ADD_NH)
  // COV_ADD_COUNT / COV_ADD_KEEP: entries per row of the add, at [r - r_first]; the count pass writes them and leaves their sum
  // in counters[CV_ADD_ENTRIES], the keep pass places a wave's entries by one atomic on counters[CV_KEPT]
  uint32_t *row_entries;
  uint4 *arena; uint64_t arena_cap;
  // the names of the add (names.h; their rows are A's [r_first, r_last)): row r belongs to alignment a with row_off[a] <= r <
  // row_off[a + 1], a to name g with group_off[g] <= a < group_off[g + 1]; its add-order index is name_base + g
  NameWindow names; uint64_t name_base;
};
void launch_cov_add(hipStream_t st, const CovAddWArgs &W, int mode);
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

// The depth pipeline, for W = uint32_t and W = uint64_t (arithmetic modulo 2^32 and 2^64).
// depth[0, n) <- its inclusive prefix sums, in place.  tile_sum: n / COV_TILE + 2 words, scan_tmp: what launch_scan
// (scan_kernels.h) needs for that many
template <typename W>
void launch_cov_scan(hipStream_t st, W *depth, int64_t n, uint64_t *tile_sum, uint64_t *scan_tmp);
// per transcript: the sum, the number of non-zero entries and the maximum of depth[off[t], off[t + 1]).  32-bit words: the sum in
// aligned (aligned_lo is not used).  64-bit words: the sum of their high words in aligned, of their low words in aligned_lo
template <typename W>
void launch_cov_summary(hipStream_t st, const W *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned, uint64_t *aligned_lo,
                        uint64_t *covered, W *max_depth);
// tile_cnt[k] = the run heads among the bases of tile k (a base of depth > 0 that is its transcript's first or differs from the
// base in front of it)
template <typename W>
void launch_cov_count(hipStream_t st, const W *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt);
// tile_cnt scanned (exclusive): run k is (transcript, start, end, depth) in run4[k]; the head's lane stores the first two words, the
// lane of the run's last base the other two.  64-bit words: a run is 24 bytes, (transcript, start, end, 0) in run4[k] and the depth
// in run_depth[k] (32-bit words: not used)
template <typename W>
void launch_cov_runs(hipStream_t st, const W *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *run4,
                     uint64_t *run_depth);

}  // namespace br
