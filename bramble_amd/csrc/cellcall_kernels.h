// Cell calling on the device (cellcall_kernels.hip; host side: cellcall.cpp, which holds the pipeline's description; the definitions
// -- rank, the three methods, the simulation's draws and sums -- are in bramble_amd.h, br_cellcall).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

constexpr uint32_t CC_NONE = 0xffffffffu;   // want[n]: n is no wanted total
// bits of the counters' CC_BAD word: what a refused matrix had
enum { CC_BAD_OFFSET = 1, CC_BAD_FEATURE = 2, CC_BAD_ORDER = 4, CC_BAD_COUNT = 8, CC_BAD_TOTAL = 16 };
// words of the counters
enum { CC_BAD = 0, CC_BITS = 2 /* OR and AND of the sort keys (two words) */, CC_WORDS = 16 };

// The matrix checked and summed, a lane per cell: total[c], key[c] = (0xffffffff - total) << 32 | c, idx[c] = c; what is wrong is
// ORed into counters[CC_BAD] (a cell whose offsets descend or leave [0, nnz] is not read)
void launch_cc_totals(hipStream_t st, int64_t n_cells, int64_t n_features, uint64_t nnz, const uint64_t *cell_off, const uint32_t *feature,
                      const uint32_t *count, uint64_t *total, uint64_t *key, uint32_t *idx, unsigned long long *counters);
// order: the cells in rank order (the sorted idx).  rank[order[r]] = r; status[order[r]] = r < n_called
void launch_cc_rank(hipStream_t st, const uint32_t *order, int64_t n_cells, int64_t n_called, uint32_t *rank, uint8_t *status);
// amb[g] += count over the cells at ranks [r0, r1): a wave per cell, integer atomics
void launch_cc_ambient(hipStream_t st, const uint32_t *order, int64_t r0, int64_t r1, const uint64_t *cell_off, const uint32_t *feature,
                       const uint32_t *count, unsigned long long *amb);
// active[feature[i]] = 1 over the matrix's entries
void launch_cc_active(hipStream_t st, const uint32_t *feature, uint64_t nnz, uint8_t *active);
// candidate j is the cell order[r0 + j]: cell[j], and O[j] by the recurrence over its entries (one lane, in order)
void launch_cc_observed(hipStream_t st, const uint32_t *order, int64_t r0, int64_t m, const uint64_t *cell_off, const uint32_t *feature,
                        const uint32_t *count, const double *ln, const double *lp, uint32_t *cell, double *O);

// The simulations [s_first, s_first + n_sims) of one launch, a wave each.  T and lp are over the n_active active features in index
// order (T: the thresholds, the last one 2^32); bits: n_active - 1 < 2^bits.  table: n_sims x n_active counts, zeroed by the caller.
// ln: n_max + 2 entries; want: n_max + 1 entries, want[n] = the index of the wanted total n or CC_NONE.  L[index * sims + s].
struct CcSimArgs {
  const uint64_t *T; const double *lp; uint32_t n_active; int bits;
  const double *ln; const uint32_t *want; uint32_t n_max;
  uint32_t s_first, n_sims, sims, k0, k1;
  uint32_t *table; double *L;
};
void launch_cc_simulate(hipStream_t st, const CcSimArgs &A);
// lower[j] = #{ s : L[widx[j] * sims + s] < O[j] }: a block per candidate
void launch_cc_lower(hipStream_t st, const double *L, uint32_t sims, const uint32_t *widx, const double *O, int64_t m, uint32_t *lower);
// status[cell[j]] = 2 where called[j]
void launch_cc_mark(hipStream_t st, const uint32_t *cell, const uint8_t *called, int64_t m, uint8_t *status);


// For an accumulator that holds a matrix with real values (br_cells).  out[i] = (uint32)val[i]: the integer counts of "unique"
void launch_cc_counts(hipStream_t st, const double *val, uint64_t n, uint32_t *out);
// flag[k] = the cell is called (status != 0), len[k] = its entries if it is, else 0; both to be scanned (K + 1 words each)
void launch_cc_called(hipStream_t st, const uint8_t *status, const uint64_t *m_off, int64_t n_cells, uint64_t *flag, uint64_t *len);
// the called cells' rows, a wave per cell, from the scanned flag / len: cells[pos] = k, off[pos] = len[k] (off[n_called] is the
// caller's), the row's features and values copied
void launch_cc_rows(hipStream_t st, const uint8_t *status, const uint64_t *pos, const uint64_t *noff, int64_t n_cells, const uint64_t *m_off,
                    const uint32_t *m_feat, const double *m_val, uint32_t *cells, uint64_t *off, uint32_t *feat, double *val);

}  // namespace br
