// Single-cell count matrices on the device (host side: cells.cpp, which holds the pipeline's description; the definitions are in
// bramble_amd.h, br_cells).
//
//   add      k_cl_rows: a lane per row checks its record's offsets; k_cl_names: a lane per name reads the barcode of its first record
//   finish   k_cl_flag + scan + the field sort's compact: the names that count; the field sort (barcode_sort.h), its heads + scan,
//            k_cl_cells: the cells; a sort of (cell, class), k_qg_flag + scan, k_cl_entries: the entries; k_cl_pairs, a stable sort
//            of (cell, feature), k_qg_flag + scan, k_cl_transpose, k_cl_slots: the slots and the per-slot lists; k_cl_route; k_cl_em or k_cl_unique;
//            k_cl_cell_stats, k_cl_keep + scan, k_cl_matrix
//
// No floating-point atomic anywhere.  The integer atomics count lanes and append cells to the route lists, whose order no result
// depends on.
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "barcode_inl.h"
#include "cells_kernels.h"
#include "names_inl.h"
#include "wave_inl.h"

namespace br {

namespace {
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// ---- add -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cl_rows(ClAddArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, n = A.names.r_last - A.names.r_first;
  bool bad = false;
  if (i < n) { const uint8_t *rec; uint64_t len; bad = !record_of(A.names, A.recs, A.names.r_first + i, rec, len); }
  if (__ballot(bad) && bad) A.counters[CL_BAD] = 1;
}

__global__ void __launch_bounds__(256) k_cl_names(ClAddArgs A) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool is_bad = false, none = false, too_long = false, bad_aux = false;
  if (g < A.names.n_groups) {
    uint64_t r0, r1, w[4] = {0, 0, 0, 0};
    uint32_t l = 0;
    if (!name_rows(A.names, g, r0, r1)) is_bad = true;
    else if (r1 > r0) {
      const uint8_t *rec; uint64_t len;
      if (record_of(A.names, A.recs, r0, rec, len)) { l = record_field(rec, len, A.where, A.sep, A.tag, w, too_long, bad_aux); none = l == 0u; }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) A.cb[4 * g + k] = w[k];
    A.cblen[g] = (uint8_t)l;
  }
  count_lanes(none, A.counters + CL_NO_BC);
  count_lanes(too_long, A.counters + CL_TOO_LONG);
  count_lanes(bad_aux, A.counters + CL_BAD_AUX);
  if (__ballot(is_bad) && is_bad) A.counters[CL_BAD] = 1;
}

void launch_cl_add(hipStream_t st, const ClAddArgs &A) {
  const uint64_t n = A.names.r_last - A.names.r_first;
  if (n) hipLaunchKernelGGL(k_cl_rows, dim3(blocks256((int64_t)n)), dim3(256), 0, st, A);
  if (A.names.n_groups > 0) hipLaunchKernelGGL(k_cl_names, dim3(blocks256(A.names.n_groups)), dim3(256), 0, st, A);
}

// ---- finish: cells, entries, slots ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cl_flag(const uint8_t *cblen, const uint32_t *name_cls, int64_t n, uint64_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = cblen[i] != 0 && name_cls[i] != 0xffffffffu ? 1 : 0;
}
void launch_cl_flag(hipStream_t st, const uint8_t *cblen, const uint32_t *name_cls, int64_t n, uint64_t *flag) {
  if (n > 0) hipLaunchKernelGGL(k_cl_flag, dim3(blocks256(n)), dim3(256), 0, st, cblen, name_cls, n, flag);
}

__global__ void __launch_bounds__(256) k_cl_cells(const uint64_t *cid, const uint32_t *idx, int64_t n, const uint64_t *cb, const uint8_t *cblen,
                                                  const uint32_t *name_cls, uint32_t *name_cell, uint64_t *cell_cb, uint8_t *cell_len, uint64_t *key) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t k = cid[j + 1] - 1, i = idx[j];
  name_cell[i] = (uint32_t)k;
  key[j] = k << 32 | (uint64_t)name_cls[i];
  if (cid[j + 1] != cid[j]) {
#pragma unroll
    for (int w = 0; w < 4; w++) cell_cb[4 * k + w] = cb[4 * i + w];
    cell_len[k] = cblen[i];
  }
}
void launch_cl_cells(hipStream_t st, const uint64_t *cid, const uint32_t *idx, int64_t n, const uint64_t *cb, const uint8_t *cblen,
                     const uint32_t *name_cls, uint32_t *name_cell, uint64_t *cell_cb, uint8_t *cell_len, uint64_t *key) {
  if (n > 0) hipLaunchKernelGGL(k_cl_cells, dim3(blocks256(n)), dim3(256), 0, st, cid, idx, n, cb, cblen, name_cls, name_cell, cell_cb, cell_len, key);
}

__global__ void __launch_bounds__(256) k_cl_entries(const uint64_t *key, const uint64_t *ebeg, int64_t n_ent, int64_t n_cells, const uint32_t *gk,
                                                    uint32_t *e_cell, uint32_t *e_cls, uint32_t *e_n, uint64_t *pair_cnt, uint64_t *cell_eoff) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_ent) return;
  const uint64_t k = key[ebeg[e]];
  const uint32_t cell = (uint32_t)(k >> 32), cls = (uint32_t)k;
  e_cell[e] = cell; e_cls[e] = cls; e_n[e] = (uint32_t)(ebeg[e + 1] - ebeg[e]);
  pair_cnt[e] = gk[cls];
  if (e == 0 || (uint32_t)(key[ebeg[e - 1]] >> 32) != cell) cell_eoff[cell] = (uint64_t)e;
  if (e == n_ent - 1) cell_eoff[n_cells] = (uint64_t)n_ent;
}
void launch_cl_entries(hipStream_t st, const uint64_t *key, const uint64_t *ebeg, int64_t n_ent, int64_t n_cells, const uint32_t *gk,
                       uint32_t *e_cell, uint32_t *e_cls, uint32_t *e_n, uint64_t *pair_cnt, uint64_t *cell_eoff) {
  if (n_ent > 0) hipLaunchKernelGGL(k_cl_entries, dim3(blocks256(n_ent)), dim3(256), 0, st, key, ebeg, n_ent, n_cells, gk, e_cell, e_cls, e_n, pair_cnt, cell_eoff);
}

__global__ void __launch_bounds__(256) k_cl_pairs(int64_t n_ent, const uint32_t *e_cell, const uint32_t *e_cls, const uint64_t *pair_off,
                                                  const uint32_t *glab, const uint64_t *goff, uint64_t *key, uint32_t *idx, uint32_t *p_ent) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_ent) return;
  const uint64_t p0 = pair_off[e], m = pair_off[e + 1] - p0, g0 = goff[e_cls[e]], cell = e_cell[e];
  for (uint64_t j = 0; j < m; j++) { key[p0 + j] = cell << 32 | (uint64_t)glab[g0 + j]; idx[p0 + j] = (uint32_t)(p0 + j); p_ent[p0 + j] = (uint32_t)e; }
}
void launch_cl_pairs(hipStream_t st, int64_t n_ent, const uint32_t *e_cell, const uint32_t *e_cls, const uint64_t *pair_off, const uint32_t *glab,
                     const uint64_t *goff, uint64_t *key, uint32_t *idx, uint32_t *p_ent) {
  if (n_ent > 0) hipLaunchKernelGGL(k_cl_pairs, dim3(blocks256(n_ent)), dim3(256), 0, st, n_ent, e_cell, e_cls, pair_off, glab, goff, key, idx, p_ent);
}

__global__ void __launch_bounds__(256) k_cl_transpose(const uint32_t *idx, const uint64_t *sid, int64_t n_pairs, const uint32_t *p_ent, uint32_t *pslot,
                                                      uint32_t *t_ent) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_pairs) return;
  const uint32_t p = idx[q];
  pslot[p] = (uint32_t)(sid[q + 1] - 1);
  t_ent[q] = p_ent[p];
}
void launch_cl_transpose(hipStream_t st, const uint32_t *idx, const uint64_t *sid, int64_t n_pairs, const uint32_t *p_ent, uint32_t *pslot,
                         uint32_t *t_ent) {
  if (n_pairs > 0) hipLaunchKernelGGL(k_cl_transpose, dim3(blocks256(n_pairs)), dim3(256), 0, st, idx, sid, n_pairs, p_ent, pslot, t_ent);
}

__global__ void __launch_bounds__(256) k_cl_slots(const uint64_t *key, const uint64_t *sbeg, int64_t n_slots, int64_t n_cells, uint32_t *s_feat,
                                                  uint64_t *cell_soff) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_slots) return;
  const uint64_t k = key[sbeg[s]];
  const uint32_t cell = (uint32_t)(k >> 32);
  s_feat[s] = (uint32_t)k;
  if (s == 0 || (uint32_t)(key[sbeg[s - 1]] >> 32) != cell) cell_soff[cell] = (uint64_t)s;
  if (s == n_slots - 1) cell_soff[n_cells] = (uint64_t)n_slots;
}
void launch_cl_slots(hipStream_t st, const uint64_t *key, const uint64_t *sbeg, int64_t n_slots, int64_t n_cells, uint32_t *s_feat, uint64_t *cell_soff) {
  if (n_slots > 0) hipLaunchKernelGGL(k_cl_slots, dim3(blocks256(n_slots)), dim3(256), 0, st, key, sbeg, n_slots, n_cells, s_feat, cell_soff);
}

// ---- finish: the values ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cl_route(ClTables T, uint32_t lds_bytes, uint32_t *wave_list, uint32_t *blk_list, unsigned long long *counters) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= T.n_cells) return;
  const uint64_t e0 = T.cell_eoff[k], e1 = T.cell_eoff[k + 1];
  const uint64_t n_s = T.cell_soff[k + 1] - T.cell_soff[k], n_p = T.pair_off[e1] - T.pair_off[e0], n_e = e1 - e0;
  if (n_s <= CL_WAVE_ITEMS && n_p <= CL_WAVE_ITEMS) { wave_list[atomicAdd(counters + CL_NWAVE, 1ull)] = (uint32_t)k; return; }
  blk_list[atomicAdd(counters + CL_NBLK, 1ull)] = (uint32_t)k;
  const uint64_t need = (2 * n_s + n_e) * 8 + CL_LDS_HEAD;
  if (need <= (uint64_t)lds_bytes) atomicMax(counters + CL_NEED, (unsigned long long)need);
  else atomicAdd(counters + CL_NHBM, 1ull);
}
void launch_cl_route(hipStream_t st, const ClTables &T, uint32_t lds_bytes, uint32_t *wave_list, uint32_t *blk_list, unsigned long long *counters) {
  if (T.n_cells > 0) hipLaunchKernelGGL(k_cl_route, dim3(blocks256(T.n_cells)), dim3(256), 0, st, T, lds_bytes, wave_list, blk_list, counters);
}

namespace {
// sum of v[at[b + j] - base] over j in [0, n), one after the other: one lane's list
__device__ __forceinline__ double list_sum(const double *v, const uint32_t *at, uint64_t b, uint64_t n, uint64_t base) {
  double s = 0;
  for (uint64_t j = 0; j < n; j++) s += v[at[b + j] - base];
  return s;
}
// the lists of the wave's lanes (b, n; n = 0: none): up to CL_WAVE_ITEMS items by the lane, a longer list by the wave.  Every lane of
// the wave calls it
__device__ __forceinline__ double lists_sum(const double *v, const uint32_t *at, uint64_t b, uint64_t n, uint64_t base) {
  const int lane = threadIdx.x & 63;
  double d = n <= CL_WAVE_ITEMS ? list_sum(v, at, b, n, base) : 0.0;
  wave_turns(n > CL_WAVE_ITEMS, [&](int src) {
    const uint64_t bb = __shfl(b, src), nn = __shfl(n, src);
    double s = 0;
    for (uint64_t j = (uint64_t)lane; j < nn; j += 64) s += v[at[bb + j] - base];
    s = wave_sum(s);
    if (lane == src) d = s;
  });
  return d;
}

// one cell by the block's 256 threads; th[0], th[1] (slots) and q (entries) in LDS or in HBM, red: 4 doubles of LDS
__device__ void em_block_cell(const ClEmArgs &E, uint32_t k, double *th0, double *th1, double *q, double *red) {
  const ClTables &T = E.T;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t e0 = T.cell_eoff[k], s0 = T.cell_soff[k];
  const uint64_t n_e = T.cell_eoff[k + 1] - e0, n_s = T.cell_soff[k + 1] - s0;
  double *th[2] = {th0, th1};
  for (uint64_t s = tid; s < n_s; s += 256) th[0][s] = 1.0;
  __syncthreads();
  uint32_t it = 0;
  int cur = 0;
  while (it < E.max_iters) {
    for (uint64_t base = 0; base < n_e; base += 256) {
      const uint64_t e = base + tid;
      uint64_t b = 0, n = 0;
      if (e < n_e) { b = T.pair_off[e0 + e]; n = T.pair_off[e0 + e + 1] - b; }
      const double d = lists_sum(th[cur], T.pslot, b, n, s0);
      if (e < n_e) q[e] = d != 0.0 ? (double)T.e_n[e0 + e] / d : 0.0;
    }
    __syncthreads();
    double rel = 0;
    for (uint64_t base = 0; base < n_s; base += 256) {
      const uint64_t s = base + tid;
      uint64_t b = 0, n = 0;
      if (s < n_s) { b = T.sbeg[s0 + s]; n = T.sbeg[s0 + s + 1] - b; }
      const double sum = lists_sum(q, T.t_ent, b, n, e0);
      if (s < n_s) {
        const double t = th[cur][s], tn = t * sum;
        th[cur ^ 1][s] = tn;
        if (tn > 1e-8) { const double r = fabs(tn - t) / tn; rel = r > rel ? r : rel; }
      }
    }
    rel = wave_max(rel);
    if (lane == 0) red[wv] = rel;
    __syncthreads();
    for (int w = 0; w < 4; w++) rel = red[w] > rel ? red[w] : rel;
    __syncthreads();
    cur ^= 1; it++;
    if (rel < E.tolerance) break;   // (the same in every thread of the block)
  }
  for (uint64_t s = tid; s < n_s; s += 256) E.theta[s0 + s] = th[cur][s];
  if (tid == 0) E.n_iters[k] = it;
}

// one cell of up to 64 slots and 64 pairs by a wave: lane l holds slot l's theta, entry l's q, and pair l's slot and pair l's entry
// (in slot order) for the others to fetch
__device__ void em_wave_cell(const ClEmArgs &E, uint32_t k) {
  const ClTables &T = E.T;
  const int lane = threadIdx.x & 63;
  const uint64_t e0 = T.cell_eoff[k], s0 = T.cell_soff[k], p0 = T.pair_off[e0];
  const int n_e = (int)(T.cell_eoff[k + 1] - e0), n_s = (int)(T.cell_soff[k + 1] - s0), n_p = (int)(T.pair_off[e0 + n_e] - p0);
  const int my_slot = lane < n_p ? (int)(T.pslot[p0 + lane] - s0) : 0, my_ent = lane < n_p ? (int)(T.t_ent[p0 + lane] - e0) : 0;
  int eb = 0, en = 0, sb = 0, sn = 0;
  double cnt = 0;
  if (lane < n_e) { eb = (int)(T.pair_off[e0 + lane] - p0); en = (int)(T.pair_off[e0 + lane + 1] - p0) - eb; cnt = (double)T.e_n[e0 + lane]; }
  if (lane < n_s) { sb = (int)(T.sbeg[s0 + lane] - p0); sn = (int)(T.sbeg[s0 + lane + 1] - p0) - sb; }
  const int max_en = wave_max(en), max_sn = wave_max(sn);
  double theta = 1.0;
  uint32_t it = 0;
  while (it < E.max_iters) {
    double d = 0;
    for (int j = 0; j < max_en; j++) {
      const int src = __shfl(my_slot, (eb + j) & 63);
      const double v = __shfl(theta, src & 63);
      if (j < en) d += v;
    }
    const double q = lane < n_e && d != 0.0 ? cnt / d : 0.0;
    double sum = 0;
    for (int j = 0; j < max_sn; j++) {
      const int src = __shfl(my_ent, (sb + j) & 63);
      const double v = __shfl(q, src & 63);
      if (j < sn) sum += v;
    }
    const double tn = theta * sum;
    double rel = lane < n_s && tn > 1e-8 ? fabs(tn - theta) / tn : 0.0;
    rel = wave_max(rel);
    theta = tn; it++;
    if (rel < E.tolerance) break;
  }
  if (lane < n_s) E.theta[s0 + lane] = theta;
  if (lane == 0) E.n_iters[k] = it;
}
}  // namespace

__global__ void __launch_bounds__(256) k_cl_em(ClEmArgs E) {
  extern __shared__ double cl_lds[];
  if (blockIdx.x < E.n_blk) {
    const uint32_t k = E.blk_list[blockIdx.x];
    const uint64_t e0 = E.T.cell_eoff[k], s0 = E.T.cell_soff[k];
    const uint64_t n_e = E.T.cell_eoff[k + 1] - e0, n_s = E.T.cell_soff[k + 1] - s0;
    const uint64_t need = (2 * n_s + n_e) * 8 + CL_LDS_HEAD;
    double *body = cl_lds + CL_LDS_HEAD / 8;
    if (need <= (uint64_t)E.lds_bytes && need <= (uint64_t)E.lds) em_block_cell(E, k, body, body + n_s, body + 2 * n_s, cl_lds);
    else em_block_cell(E, k, E.theta + s0, E.scratch + s0, E.scratch + E.n_slots + e0, cl_lds);
    return;
  }
  const uint32_t i = (blockIdx.x - E.n_blk) * 4 + (threadIdx.x >> 6);
  if (i < E.n_wave) em_wave_cell(E, E.wave_list[i]);
}
void launch_cl_em(hipStream_t st, const ClEmArgs &E) {
  const unsigned blocks = E.n_blk + (E.n_wave + 3) / 4;
  const uint32_t lds = E.lds < CL_LDS_HEAD ? CL_LDS_HEAD : E.lds;
  if (blocks) hipLaunchKernelGGL(k_cl_em, dim3(blocks), dim3(256), lds, st, E);
}

__global__ void __launch_bounds__(256) k_cl_unique(ClTables T, int64_t n_slots, double *val) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_slots) return;
  uint64_t sum = 0;
  for (uint64_t p = T.sbeg[s]; p < T.sbeg[s + 1]; p++) {
    const uint32_t e = T.t_ent[p];
    if (T.pair_off[e + 1] - T.pair_off[e] == 1) sum += T.e_n[e];
  }
  val[s] = (double)sum;
}
void launch_cl_unique(hipStream_t st, const ClTables &T, int64_t n_slots, double *val) {
  if (n_slots > 0) hipLaunchKernelGGL(k_cl_unique, dim3(blocks256(n_slots)), dim3(256), 0, st, T, n_slots, val);
}

__global__ void __launch_bounds__(256) k_cl_cell_stats(ClTables T, uint64_t *names, uint64_t *unique, uint64_t *multi) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= T.n_cells) return;
  uint64_t u = 0, m = 0;
  for (uint64_t e = T.cell_eoff[k]; e < T.cell_eoff[k + 1]; e++) {
    if (T.pair_off[e + 1] - T.pair_off[e] == 1) u += T.e_n[e]; else m += T.e_n[e];
  }
  names[k] = u + m; unique[k] = u; multi[k] = m;
}
void launch_cl_cell_stats(hipStream_t st, const ClTables &T, uint64_t *names, uint64_t *unique, uint64_t *multi) {
  if (T.n_cells > 0) hipLaunchKernelGGL(k_cl_cell_stats, dim3(blocks256(T.n_cells)), dim3(256), 0, st, T, names, unique, multi);
}

__global__ void __launch_bounds__(256) k_cl_keep(const double *val, int64_t n_slots, int drop_zero, uint64_t *flag) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < n_slots) flag[s] = !drop_zero || val[s] != 0.0 ? 1 : 0;
}
void launch_cl_keep(hipStream_t st, const double *val, int64_t n_slots, int drop_zero, uint64_t *flag) {
  if (n_slots > 0) hipLaunchKernelGGL(k_cl_keep, dim3(blocks256(n_slots)), dim3(256), 0, st, val, n_slots, drop_zero, flag);
}

__global__ void __launch_bounds__(256) k_cl_matrix(ClTables T, const uint64_t *pos, int64_t n_slots, const uint32_t *s_feat, const double *val,
                                                   uint64_t *m_off, uint32_t *m_feat, double *m_val, uint32_t *n_feat) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_slots && pos[i + 1] != pos[i]) { m_feat[pos[i]] = s_feat[i]; m_val[pos[i]] = val[i]; }
  if (i <= T.n_cells) m_off[i] = pos[T.cell_soff[i]];
  if (i < T.n_cells) n_feat[i] = (uint32_t)(pos[T.cell_soff[i + 1]] - pos[T.cell_soff[i]]);
}
void launch_cl_matrix(hipStream_t st, const ClTables &T, const uint64_t *pos, int64_t n_slots, const uint32_t *s_feat, const double *val,
                      uint64_t *m_off, uint32_t *m_feat, double *m_val, uint32_t *n_feat) {
  const int64_t m = n_slots > T.n_cells + 1 ? n_slots : T.n_cells + 1;
  hipLaunchKernelGGL(k_cl_matrix, dim3(blocks256(m)), dim3(256), 0, st, T, pos, n_slots, s_feat, val, m_off, m_feat, m_val, n_feat);
}

}  // namespace br
