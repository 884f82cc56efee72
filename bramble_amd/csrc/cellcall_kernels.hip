// Cell calling kernels (gfx950, wave64; the definitions: bramble_amd.h, br_cellcall; the pipeline: cellcall.cpp).
//
//   k_cc_totals    a lane per cell: the matrix checked, the cell's total, its sort key
//   k_cc_rank      a lane per rank: the cell's rank and its status by the rank prefix
//   k_cc_ambient   a wave per cell of the window: integer atomics into the 64-bit ambient counts
//   k_cc_active    a lane per entry: the flag of its feature
//   k_cc_observed  a lane per candidate: its log-likelihood, the terms added in the order of the definition
//   k_cc_simulate  a wave per simulation, 64 draws a step (below)
//   k_cc_lower     a block per candidate: the simulations below its log-likelihood, counted by ballots
//   k_cc_mark      a lane per candidate: status 2
//   k_cc_counts, k_cc_called, k_cc_rows   for br_cells: its counts as integers; the called cells' rows of its matrix (a wave per row)
//
// No floating-point atomic, and every floating-point sum is one chain in the order of the definition: the bits of a result
// depend neither on the launch shape nor on how the simulations are cut into launches.
#include <hip/hip_runtime.h>

#include "cellcall_kernels.h"
#include "wave_inl.h"

namespace br {

__global__ void __launch_bounds__(256) k_cc_totals(int64_t n_cells, int64_t n_features, uint64_t nnz, const uint64_t *cell_off, const uint32_t *feature,
                                                   const uint32_t *count, uint64_t *total, uint64_t *key, uint32_t *idx, unsigned long long *counters) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cells) return;
  const uint64_t a = cell_off[c], b = cell_off[c + 1];
  uint32_t bad = 0;
  uint64_t sum = 0;
  if (a > b || b > nnz) bad = CC_BAD_OFFSET;
  else {
    uint32_t prev = 0;
    for (uint64_t p = a; p < b; p++) {
      const uint32_t g = feature[p], k = count[p];
      if ((int64_t)g >= n_features) bad |= CC_BAD_FEATURE;
      if (p > a && g <= prev) bad |= CC_BAD_ORDER;
      if (k == 0) bad |= CC_BAD_COUNT;
      prev = g; sum += k;
    }
    if (sum > 0xffffffffull) { bad |= CC_BAD_TOTAL; sum = 0xffffffffull; }
  }
  if (bad) atomicOr(counters + CC_BAD, (unsigned long long)bad);
  total[c] = sum;
  key[c] = (0xffffffffull - sum) << 32 | (uint64_t)c;
  idx[c] = (uint32_t)c;
}

__global__ void __launch_bounds__(256) k_cc_rank(const uint32_t *order, int64_t n_cells, int64_t n_called, uint32_t *rank, uint8_t *status) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_cells) return;
  const uint32_t c = order[r];
  rank[c] = (uint32_t)r;
  status[c] = r < n_called ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_cc_ambient(const uint32_t *order, int64_t r0, int64_t r1, const uint64_t *cell_off, const uint32_t *feature,
                                                    const uint32_t *count, unsigned long long *amb) {
  const int64_t r = r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= r1) return;
  const uint32_t c = order[r];
  const uint64_t b = cell_off[c + 1];
  for (uint64_t p = cell_off[c] + (threadIdx.x & 63); p < b; p += 64) atomicAdd(amb + feature[p], (unsigned long long)count[p]);
}

__global__ void __launch_bounds__(256) k_cc_active(const uint32_t *feature, uint64_t nnz, uint8_t *active) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < nnz) active[feature[p]] = 1;
}

__global__ void __launch_bounds__(256) k_cc_observed(const uint32_t *order, int64_t r0, int64_t m, const uint64_t *cell_off, const uint32_t *feature,
                                                     const uint32_t *count, const double *ln, const double *lp, uint32_t *cell, double *O) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const uint32_t c = order[r0 + j];
  double o = 0.0;
  uint32_t i = 0;
  for (uint64_t p = cell_off[c]; p < cell_off[c + 1]; p++) {
    const double l = lp[feature[p]];
    const uint32_t k = count[p];
    for (uint32_t q = 0; q < k; q++) { i++; o = o + ((ln[i] - ln[q + 1]) + l); }
  }
  cell[j] = c; O[j] = o;
}

namespace {
// Philox4x32-10 of counter (c0, c1, 0, 2) under key (k0, k1): output word `word`
__device__ __forceinline__ uint32_t philox_word(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t word) {
  uint32_t c2 = 0, c3 = 2;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
}  // namespace

// A wave per simulation; a step is 64 consecutive draws, lane l the draw 64 step + l.  The lane draws its feature (Philox, then the
// first threshold above the draw by a binary search: the result stays inside [0, n_active) whatever the table holds).  How often
// the feature was drawn before is the simulation's count table -- read and raised by ONE returning integer atomic of the lowest
// lane that drew it, so the read is the L2's value and not a line an earlier step left in the vector cache -- plus the lanes below
// this one with the same feature (wave_match).  The 64 terms are then added to the running sum in draw order through readlane: every
// lane holds the same chain, lane q keeps its value after term q, and the lanes whose draw count is a wanted total store theirs.
__global__ void __launch_bounds__(256) k_cc_simulate(CcSimArgs A) {
  const uint32_t lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= A.n_sims) return;   // (the whole wave)
  const uint32_t s = A.s_first + w;
  uint32_t *tab = A.table + (uint64_t)w * A.n_active;
  const uint64_t below = (1ull << lane) - 1;
  double acc = 0.0;
  for (uint32_t base = 0; base < A.n_max; base += 64) {
    const uint32_t i = base + lane;
    const bool on = i < A.n_max;
    uint32_t j = 0;
    if (on) {
      const uint64_t u = philox_word(i >> 2, s, A.k0, A.k1, i & 3u);
      uint32_t lo = 0, hi = A.n_active - 1;
      while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (u < A.T[mid]) hi = mid; else lo = mid + 1; }
      j = lo;
    }
    const uint64_t same = wave_match(j, A.bits, on);
    const int first = on ? __ffsll((unsigned long long)same) - 1 : (int)lane;
    uint32_t before = 0;
    if (on && (int)lane == first) before = atomicAdd(tab + j, (uint32_t)__popcll(same));
    before = __shfl(before, first);
    double term = 0.0;
    uint32_t wi = CC_NONE;
    if (on) {
      const uint32_t k = before + (uint32_t)__popcll(same & below);
      term = (A.ln[i + 1] - A.ln[k + 1]) + A.lp[j];
      wi = A.want[i + 1];
    }
    const int cnt = (int)min(64u, A.n_max - base);
    double mine = 0.0;
    for (int q = 0; q < cnt; q++) {   // (q is a scalar: readlane takes it as it is)
      acc = acc + readlane_f64(term, q);
      if ((int)lane == q) mine = acc;
    }
    if (wi != CC_NONE) A.L[(uint64_t)wi * A.sims + s] = mine;
  }
}

__global__ void __launch_bounds__(256) k_cc_lower(const double *L, uint32_t sims, const uint32_t *widx, const double *O, uint32_t *lower) {
  __shared__ uint32_t sh[4];
  const int64_t j = blockIdx.x;
  const double *row = L + (uint64_t)widx[j] * sims;
  const double o = O[j];
  uint32_t n = 0;   // the wave's count, the same in every lane
  for (uint32_t s0 = 0; s0 < sims; s0 += 256) {
    const uint32_t s = s0 + threadIdx.x;
    n += (uint32_t)__popcll(__ballot(s < sims && row[s] < o));
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) lower[j] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void __launch_bounds__(256) k_cc_mark(const uint32_t *cell, const uint8_t *called, int64_t m, uint8_t *status) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < m && called[j]) status[cell[j]] = 2;
}

__global__ void __launch_bounds__(256) k_cc_counts(const double *val, uint64_t n, uint32_t *out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint32_t)val[i];
}

__global__ void __launch_bounds__(256) k_cc_called(const uint8_t *status, const uint64_t *m_off, int64_t n_cells, uint64_t *flag, uint64_t *len) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cells) return;
  const bool on = status[k] != 0;
  flag[k] = on; len[k] = on ? m_off[k + 1] - m_off[k] : 0;
}

__global__ void __launch_bounds__(256) k_cc_rows(const uint8_t *status, const uint64_t *pos, const uint64_t *noff, int64_t n_cells, const uint64_t *m_off,
                                                 const uint32_t *m_feat, const double *m_val, uint32_t *cells, uint64_t *off, uint32_t *feat, double *val) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_cells || !status[k]) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t a = m_off[k], n = m_off[k + 1] - a, to = noff[k];
  if (lane == 0) { cells[pos[k]] = (uint32_t)k; off[pos[k]] = to; }
  for (uint64_t i = lane; i < n; i += 64) { feat[to + i] = m_feat[a + i]; val[to + i] = m_val[a + i]; }
}

static inline unsigned blocks_for(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }

void launch_cc_totals(hipStream_t st, int64_t n_cells, int64_t n_features, uint64_t nnz, const uint64_t *cell_off, const uint32_t *feature,
                      const uint32_t *count, uint64_t *total, uint64_t *key, uint32_t *idx, unsigned long long *counters) {
  if (n_cells <= 0) return;
  hipLaunchKernelGGL(k_cc_totals, dim3(blocks_for((uint64_t)n_cells, 256)), dim3(256), 0, st, n_cells, n_features, nnz, cell_off, feature, count, total, key,
                     idx, counters);
}

void launch_cc_rank(hipStream_t st, const uint32_t *order, int64_t n_cells, int64_t n_called, uint32_t *rank, uint8_t *status) {
  if (n_cells <= 0) return;
  hipLaunchKernelGGL(k_cc_rank, dim3(blocks_for((uint64_t)n_cells, 256)), dim3(256), 0, st, order, n_cells, n_called, rank, status);
}

void launch_cc_ambient(hipStream_t st, const uint32_t *order, int64_t r0, int64_t r1, const uint64_t *cell_off, const uint32_t *feature,
                       const uint32_t *count, unsigned long long *amb) {
  if (r1 <= r0) return;
  hipLaunchKernelGGL(k_cc_ambient, dim3(blocks_for((uint64_t)(r1 - r0), 4)), dim3(256), 0, st, order, r0, r1, cell_off, feature, count, amb);
}

void launch_cc_active(hipStream_t st, const uint32_t *feature, uint64_t nnz, uint8_t *active) {
  if (nnz == 0) return;
  hipLaunchKernelGGL(k_cc_active, dim3(blocks_for(nnz, 256)), dim3(256), 0, st, feature, nnz, active);
}

void launch_cc_observed(hipStream_t st, const uint32_t *order, int64_t r0, int64_t m, const uint64_t *cell_off, const uint32_t *feature,
                        const uint32_t *count, const double *ln, const double *lp, uint32_t *cell, double *O) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_cc_observed, dim3(blocks_for((uint64_t)m, 256)), dim3(256), 0, st, order, r0, m, cell_off, feature, count, ln, lp, cell, O);
}

void launch_cc_simulate(hipStream_t st, const CcSimArgs &A) {
  if (A.n_sims == 0 || A.n_max == 0 || A.n_active == 0) return;
  hipLaunchKernelGGL(k_cc_simulate, dim3(blocks_for(A.n_sims, 4)), dim3(256), 0, st, A);
}

void launch_cc_lower(hipStream_t st, const double *L, uint32_t sims, const uint32_t *widx, const double *O, int64_t m, uint32_t *lower) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_cc_lower, dim3((unsigned)m), dim3(256), 0, st, L, sims, widx, O, lower);
}

void launch_cc_mark(hipStream_t st, const uint32_t *cell, const uint8_t *called, int64_t m, uint8_t *status) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_cc_mark, dim3(blocks_for((uint64_t)m, 256)), dim3(256), 0, st, cell, called, m, status);
}

void launch_cc_counts(hipStream_t st, const double *val, uint64_t n, uint32_t *out) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_cc_counts, dim3(blocks_for(n, 256)), dim3(256), 0, st, val, n, out);
}

void launch_cc_called(hipStream_t st, const uint8_t *status, const uint64_t *m_off, int64_t n_cells, uint64_t *flag, uint64_t *len) {
  if (n_cells <= 0) return;
  hipLaunchKernelGGL(k_cc_called, dim3(blocks_for((uint64_t)n_cells, 256)), dim3(256), 0, st, status, m_off, n_cells, flag, len);
}

void launch_cc_rows(hipStream_t st, const uint8_t *status, const uint64_t *pos, const uint64_t *noff, int64_t n_cells, const uint64_t *m_off,
                    const uint32_t *m_feat, const double *m_val, uint32_t *cells, uint64_t *off, uint32_t *feat, double *val) {
  if (n_cells <= 0) return;
  hipLaunchKernelGGL(k_cc_rows, dim3(blocks_for((uint64_t)n_cells, 4)), dim3(256), 0, st, status, pos, noff, n_cells, m_off, m_feat, m_val, cells, off, feat,
                     val);
}

}  // namespace br
