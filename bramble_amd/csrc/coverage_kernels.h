// Per-base transcript coverage on the device: rows -> interval events -> depth -> per-transcript summary and runs
// (coverage_kernels.hip; host side: coverage.cpp, which holds the pipeline's description).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace br
