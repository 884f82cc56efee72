// UMI-aware duplicate removal by read name on the device (host side: dedup.cpp, which holds the pipeline's description; the
// definitions are in bramble_amd.h, br_dedup).
//
//   add      k_dd_rows: a lane per row: the entry (t, five, f) from the row's CIGAR and the record's flag word, a pooled CIGAR of
//            more than DD_WAVE_OPS ops summed by the wave; k_dd_names: a lane per name: the UMI of its first record, and for a name
//            of up to DD_SMALL_ROWS rows the entries in order and their hash; k_dd_sig_big: a wave per longer name
//   finish   the names sorted by hash and cut into position groups by the quantifier's kernels (a signature is a list of words to
//            them); k_dd_groups; the field sort by (group, length, UMI) and its heads (barcode_sort.h);
//            k_dd_node_key and a sort: the node order; k_dd_nodes, k_dd_gn0, k_dd_work; k_dd_edges twice (count, fill): a wave per
//            pair of tiles of 64 nodes; k_dd_sweep until nothing changes; k_dd_msize, k_dd_hist, k_dd_verdict
//   next     k_dd_keep, k_dd_select, k_dd_write: DD_WRITE_LANES lanes per record
//
// Integers and bytes only.  The atomics are integer adds and maxima whose results do not depend on their order, with one exception
// that no result depends on: the order of a node's incoming edges in esrc, of which only the minimum label is ever taken.
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "barcode_inl.h"
#include "cigar_inl.h"
#include "dedup_kernels.h"
#include "names_inl.h"
#include "wave_inl.h"

namespace br {

namespace {
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }
__device__ __forceinline__ uint64_t fmix64(uint64_t h) {   // (murmur3's)
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
// an entry as the arena's four words: x = t, (y, z) = five, w = f
__device__ __forceinline__ bool ent_less(const uint4 a, const uint4 b, bool &eq) {
  eq = false;
  if (a.x != b.x) return a.x < b.x;
  const int64_t fa = (int64_t)((uint64_t)a.y | (uint64_t)a.z << 32), fb = (int64_t)((uint64_t)b.y | (uint64_t)b.z << 32);
  if (fa != fb) return fa < fb;
  if (a.w != b.w) return a.w < b.w;
  eq = true;
  return false;
}
// a signature's hash: the sum of its entries' hashes (a multiset's: no order), closed with the count
__device__ __forceinline__ uint64_t ent_hash(const uint4 e) {
  return fmix64(((uint64_t)e.x | (uint64_t)e.w << 32) * 0x9E3779B97F4A7C15ull + fmix64(((uint64_t)e.y | (uint64_t)e.z << 32) ^ 0xD6E8FEB86659FD93ull));
}
__device__ __forceinline__ uint64_t sig_hash(uint64_t sum, uint64_t k) { return fmix64(sum ^ fmix64(k + 0x9E3779B97F4A7C15ull)); }

// the UMI of a record and, with "cell_source", its cell barcode (barcode_inl.h)
__device__ __forceinline__ uint32_t umi_of(const DdAddArgs &A, const uint8_t *rec, uint64_t len, uint64_t w[4], bool &too_long, bool &bad_aux) {
  return record_field(rec, len, A.umi_source == 0 ? BC_NAME_LAST : BC_TAG, A.umi_sep, A.umi_tag, w, too_long, bad_aux);
}
__device__ __forceinline__ uint32_t cell_of(const DdAddArgs &A, const uint8_t *rec, uint64_t len, uint64_t w[4]) {
  bool too_long, bad_aux;
  return record_field(rec, len, A.cell_source == 1 ? BC_NAME_PREV : BC_TAG, A.umi_sep, A.cell_tag, w, too_long, bad_aux);
}
}  // namespace

// ---- add -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_dd_rows(DdAddArgs A) {
  const NameWindow &N = A.names;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, n = N.r_last - N.r_first;
  const int lane = threadIdx.x & 63;
  bool bad = false, live = false;
  uint32_t t = 0, f = 0, wide_n = 0;
  uint64_t pos = 0, lead = 0, trail = 0, reflen = 0, wide_off = 0;
  if (i < n) {
    const uint64_t r = N.r_first + i;
    const uint4 m = A.a[(int64_t)r - A.a_bias];
    const uint64_t c = A.cigar[(int64_t)r - A.a_bias];
    const uint32_t nc = BR_ROW_NCIGAR(m.z);
    const uint8_t *rec; uint64_t len;
    t = m.x; pos = m.y;
    if (!record_of(N, A.recs, r, rec, len)) bad = true;
    else {
      f = ld16(rec + 18) & 0xD1u;
      if (A.rec_at) {
        const uint64_t *ro = A.recs.rec_off - A.recs.rec_bias;
        A.rec_at[i] = A.arena_base + (ro[r] - ro[N.r_first]);
        if (i == n - 1) A.rec_at[n] = A.arena_base + (ro[r + 1] - ro[N.r_first]);
      }
      if (nc <= 2u) {
        const uint32_t o0 = (uint32_t)c, o1 = (uint32_t)(c >> 32);
        reflen = cigar_ref_len_inline(c, nc);
        if (nc >= 1u && (o0 & 15u) == 4u) lead = o0 >> 4;
        if (nc == 2u && (o0 & 15u) == 5u && (o1 & 15u) == 4u) lead = o1 >> 4;
        if (nc == 1u) trail = lead;
        if (nc == 2u) { if ((o1 & 15u) == 4u) trail = o1 >> 4; else if ((o1 & 15u) == 5u && (o0 & 15u) == 4u) trail = o0 >> 4; }
      } else if (!pool_holds(A.n_pool_words, c, nc)) bad = true;
      else {
        const uint32_t *ops = A.pool + c;
        uint32_t k = 0;
        while (k < nc && (ops[k] & 15u) == 5u) k++;
        if (k < nc && (ops[k] & 15u) == 4u) lead = ops[k] >> 4;
        k = nc;
        while (k > 0u && (ops[k - 1u] & 15u) == 5u) k--;
        if (k > 0u && (ops[k - 1u] & 15u) == 4u) trail = ops[k - 1u] >> 4;
        if (nc <= DD_WAVE_OPS) { for (uint32_t j = 0; j < nc; j++) reflen += cigar_ref_len(ops[j]); }
        else { wide_off = c; wide_n = nc; }
      }
      // the record holds the ops of a row on a '-' transcript in reverse order (the encoder's), and five is the record's
      if (m.z & BR_ROW_MINUS) { const uint64_t x = lead; lead = trail; trail = x; }
      live = !bad;
    }
  }
  wave_turns(wide_n != 0u, [&](int src) {
    const uint64_t s = wave_cigar_ref_len(A.pool, __shfl(wide_off, src), (uint32_t)__shfl((int)wide_n, src));
    if (lane == src) reflen = s;
  });
  if (i < n) {
    const int64_t five = live ? ((f & 0x10u) ? (int64_t)(pos + reflen + trail) : (int64_t)pos - (int64_t)lead) : 0;
    A.raw[i] = make_uint4(t, (uint32_t)(uint64_t)five, (uint32_t)((uint64_t)five >> 32), f);
  }
  if (__ballot(bad) && bad) A.counters[DD_BAD] = 1;
}

// the entries of name g in order and their hash: one lane
__device__ __forceinline__ void sig_small(const DdAddArgs &A, uint64_t r0, uint64_t r1, uint64_t o, uint64_t &hash) {
  const uint4 *raw = A.raw + (r0 - A.names.r_first);
  const uint32_t k = (uint32_t)(r1 - r0);
  uint64_t sum = 0;
  for (uint32_t j = 0; j < k; j++) {
    const uint4 e = raw[j];
    uint32_t rank = 0;
    for (uint32_t i = 0; i < k; i++) { bool eq; const bool less = ent_less(raw[i], e, eq); rank += (less || (eq && i < j)) ? 1u : 0u; }
    ((uint4 *)A.ent)[o / 4 + rank] = e;
    sum += ent_hash(e);
  }
  hash = sig_hash(sum, k);
}

__global__ void __launch_bounds__(256) k_dd_names(DdAddArgs A) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool is_big = false, is_bad = false, no_umi = false, too_long = false, bad_aux = false;
  if (g < A.names.n_groups) {
    uint64_t r0, r1, w[4] = {0, 0, 0, 0}, cw[4] = {0, 0, 0, 0};
    uint32_t ul = 0, cl = 0;
    if (!name_rows(A.names, g, r0, r1)) { is_bad = true; A.noff[g] = 4 * A.row_base; A.nk[g] = 0; A.hash[g] = 0; }
    else {
      const uint64_t o = 4 * (A.row_base + (r0 - A.names.r_first));
      A.noff[g] = o; A.nk[g] = (uint32_t)(4 * (r1 - r0));
      if (r1 - r0 >= (1ull << 30)) is_bad = true;   // (the signature's length in words is 32-bit)
      else if (r1 > r0) {
        const uint8_t *rec; uint64_t len;
        if (record_of(A.names, A.recs, r0, rec, len)) {
          ul = umi_of(A, rec, len, w, too_long, bad_aux); no_umi = ul == 0u;
          if (A.cell_source) cl = cell_of(A, rec, len, cw);
        }
        if (r1 - r0 > (uint64_t)DD_SMALL_ROWS) is_big = true;
        else { uint64_t h; sig_small(A, r0, r1, o, h); A.hash[g] = h; }
      } else A.hash[g] = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) A.umi[4 * g + k] = w[k];
    A.ulen[g] = (uint8_t)ul;
    if (A.cell_source) {
#pragma unroll
      for (int k = 0; k < 4; k++) A.cb[4 * g + k] = cw[k];
      A.cblen[g] = (uint8_t)cl;
    }
  }
  const uint64_t bal = __ballot(is_big);
  if (bal) {
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = (uint32_t)atomicAdd(A.counters + DD_NBIG, (unsigned long long)__popcll(bal));
    base = __shfl(base, 0);
    if (is_big) A.big[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)g;
  }
  count_lanes(no_umi, A.counters + DD_NO_UMI);
  count_lanes(too_long, A.counters + DD_TOO_LONG);
  count_lanes(bad_aux, A.counters + DD_BAD_AUX);
  if (__ballot(is_bad) && is_bad) A.counters[DD_BAD] = 1;
}

// one wave per listed name, grid-stride over a list whose length is on the device: lane l ranks the entries l, l + 64, ... among all
__global__ void __launch_bounds__(256) k_dd_sig_big(DdAddArgs A) {
  const int lane = threadIdx.x & 63;
  const uint32_t n_big = (uint32_t)A.counters[DD_NBIG];
  for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < n_big; b += gridDim.x * 4) {
    const int64_t g = A.big[b];
    uint64_t r0, r1;
    (void)name_rows(A.names, g, r0, r1);   // (k_dd_names listed it: its rows are inside the add's)
    const uint4 *raw = A.raw + (r0 - A.names.r_first);
    const uint64_t k = r1 - r0, o = A.noff[g];
    uint64_t sum = 0;
    for (uint64_t j = (uint64_t)lane; j < k; j += 64) {
      const uint4 e = raw[j];
      uint64_t rank = 0;
      for (uint64_t i = 0; i < k; i++) { bool eq; const bool less = ent_less(raw[i], e, eq); rank += (less || (eq && i < j)) ? 1u : 0u; }
      ((uint4 *)A.ent)[o / 4 + rank] = e;
      sum += ent_hash(e);
    }
    sum = wave_sum(sum);
    if (lane == 0) A.hash[g] = sig_hash(sum, k);
  }
}

void launch_dd_add(hipStream_t st, const DdAddArgs &A) {
  const uint64_t n = A.names.r_last - A.names.r_first;
  if (n) hipLaunchKernelGGL(k_dd_rows, dim3(blocks256((int64_t)n)), dim3(256), 0, st, A);
  if (A.names.n_groups > 0) {
    hipLaunchKernelGGL(k_dd_names, dim3(blocks256(A.names.n_groups)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_dd_sig_big, dim3(DD_BIG_GRID), dim3(256), 0, st, A);
  }
}

// ---- finish --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_dd_groups(const uint64_t *gid, const uint64_t *gbeg, const uint32_t *idx, int64_t n, uint32_t *group_first,
                                                   uint32_t *name_gid) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t g = gid[j + 1] - 1;
  group_first[idx[j]] = idx[gbeg[g]];
  name_gid[idx[j]] = (uint32_t)g;
}
void launch_dd_groups(hipStream_t st, const uint64_t *gid, const uint64_t *gbeg, const uint32_t *idx, int64_t n, uint32_t *group_first, uint32_t *name_gid) {
  if (n > 0) hipLaunchKernelGGL(k_dd_groups, dim3(blocks256(n)), dim3(256), 0, st, gid, gbeg, idx, n, group_first, name_gid);
}

__global__ void __launch_bounds__(256) k_dd_node_key(const uint64_t *nbeg, const uint32_t *idx, const uint32_t *name_gid, int64_t n_nodes, uint64_t *key,
                                                     uint32_t *val) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_nodes) return;
  const uint64_t c = nbeg[q + 1] - nbeg[q];   // (below 2^32: the names are)
  key[q] = (uint64_t)name_gid[idx[nbeg[q]]] << 32 | (0xffffffffull - c);
  val[q] = (uint32_t)q;
}
void launch_dd_node_key(hipStream_t st, const uint64_t *nbeg, const uint32_t *idx, const uint32_t *name_gid, int64_t n_nodes, uint64_t *key, uint32_t *val) {
  if (n_nodes > 0) hipLaunchKernelGGL(k_dd_node_key, dim3(blocks256(n_nodes)), dim3(256), 0, st, nbeg, idx, name_gid, n_nodes, key, val);
}

__global__ void __launch_bounds__(256) k_dd_nodes(DdNodes N, const uint32_t *val, const uint64_t *nbeg, const uint32_t *idx, const uint64_t *umi,
                                                  const uint8_t *ulen, const uint32_t *name_gid) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= N.n_nodes) return;
  const uint32_t q = val[p];
  const uint64_t name = idx[nbeg[q]];
#pragma unroll
  for (int k = 0; k < 4; k++) N.umi[4 * p + k] = umi[4 * name + k];
  N.len[p] = ulen[name]; N.cnt[p] = (uint32_t)(nbeg[q + 1] - nbeg[q]); N.first[p] = (uint32_t)name; N.gid[p] = name_gid[name];
  N.inv[q] = (uint32_t)p;
}
__global__ void __launch_bounds__(256) k_dd_gn0(DdNodes N) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= N.n_nodes) return;
  const uint32_t g = N.gid[p];
  if (p == 0 || N.gid[p - 1] != g) N.gn0[g] = (uint64_t)p;
  if (p == N.n_nodes - 1) N.gn0[N.n_groups] = (uint64_t)N.n_nodes;
}
__global__ void __launch_bounds__(256) k_dd_work(DdNodes N) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t m = 0;
  if (g < N.n_groups) {
    m = N.gn0[g + 1] - N.gn0[g];
    const uint64_t tiles = (m + 63) / 64;
    N.work[g] = m < 2 ? 0 : tiles * tiles;
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m) atomicMax(N.counters + DD_MAXM, (unsigned long long)m);
}
void launch_dd_nodes(hipStream_t st, const DdNodes &N, const uint32_t *val, const uint64_t *nbeg, const uint32_t *idx, const uint64_t *umi,
                     const uint8_t *ulen, const uint32_t *name_gid) {
  if (N.n_nodes <= 0) return;
  hipLaunchKernelGGL(k_dd_nodes, dim3(blocks256(N.n_nodes)), dim3(256), 0, st, N, val, nbeg, idx, umi, ulen, name_gid);
  hipLaunchKernelGGL(k_dd_gn0, dim3(blocks256(N.n_nodes)), dim3(256), 0, st, N);
  hipLaunchKernelGGL(k_dd_work, dim3(blocks256(N.n_groups)), dim3(256), 0, st, N);
}

namespace {
// bytes in which two words differ
__device__ __forceinline__ uint32_t bytes_differ(uint64_t a, uint64_t b) {
  const uint64_t x = a ^ b, lo7 = 0x7f7f7f7f7f7f7f7full;
  return (uint32_t)__popcll((unsigned long long)((((x & lo7) + lo7) | x) & ~lo7));
}
}  // namespace

// A wave takes one pair of tiles of its group: its lanes hold the 64 sources, the 64 targets pass by shuffle, so no lane walks more
// than 64 nodes however large the group.  An edge u -> v: equal length, one byte apart, c_u >= 2 c_v - 1
template <bool FILL>
__global__ void __launch_bounds__(256) k_dd_edges(DdNodes N, const uint64_t *eoff, uint64_t n_work) {
  const int lane = threadIdx.x & 63;
  for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_work; w += (uint64_t)gridDim.x * 4) {
    int64_t lo = 0, hi = N.n_groups;   // the last group whose pairs begin at or in front of w
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (N.work[mid] <= w) lo = mid + 1; else hi = mid; }
    const int64_t g = lo - 1;
    const uint64_t p0 = N.gn0[g], m = N.gn0[g + 1] - p0, tiles = (m + 63) / 64, local = w - N.work[g];
    const uint64_t vt = local / tiles, ut = local % tiles;
    const uint64_t u = ut * 64 + (uint64_t)lane, v_mine = vt * 64 + (uint64_t)lane;
    const bool u_ok = u < m, v_ok = v_mine < m;
    uint64_t uw[4] = {0, 0, 0, 0}, vw[4] = {0, 0, 0, 0};
    uint32_t ulen = 0, vlen = 0;
    uint64_t uc = 0, vc = 0;
    if (u_ok) {
#pragma unroll
      for (int k = 0; k < 4; k++) uw[k] = N.umi[4 * (p0 + u) + k];
      ulen = N.len[p0 + u]; uc = N.cnt[p0 + u];
    }
    if (v_ok) {
#pragma unroll
      for (int k = 0; k < 4; k++) vw[k] = N.umi[4 * (p0 + v_mine) + k];
      vlen = N.len[p0 + v_mine]; vc = N.cnt[p0 + v_mine];
    }
    const int nv = (int)(m - vt * 64 < 64 ? m - vt * 64 : 64);
    for (int i = 0; i < nv; i++) {
      const uint64_t v = vt * 64 + (uint64_t)i;
      const uint32_t len_v = (uint32_t)__shfl((int)vlen, i);
      const uint64_t c_v = __shfl(vc, i);
      uint32_t d = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) d += bytes_differ(uw[k], __shfl(vw[k], i));
      const bool edge = u_ok && u != v && ulen != 0u && ulen == len_v && d == 1u && uc + 1 >= 2 * c_v;
      const uint64_t bal = __ballot(edge);
      if (!bal) continue;
      const unsigned long long cnt = (unsigned long long)__popcll((unsigned long long)bal);
      if (!FILL) { if (lane == 0) atomicAdd((unsigned long long *)N.indeg + (p0 + v), cnt); }
      else {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(N.cursor + (p0 + v), (uint32_t)cnt);
        base = __shfl(base, 0);
        if (edge) N.esrc[eoff[p0 + v] + base + (uint32_t)__popcll((unsigned long long)(bal & ((1ull << lane) - 1ull)))] = (uint32_t)(p0 + u);
      }
    }
  }
}
void launch_dd_edges(hipStream_t st, const DdNodes &N, const uint64_t *eoff, uint64_t n_work, bool fill) {
  if (!n_work) return;
  const uint64_t blocks = (n_work + 3) / 4;
  const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
  if (fill) hipLaunchKernelGGL(k_dd_edges<true>, grid, dim3(256), 0, st, N, eoff, n_work);
  else hipLaunchKernelGGL(k_dd_edges<false>, grid, dim3(256), 0, st, N, eoff, n_work);
}

__global__ void __launch_bounds__(256) k_dd_label_init(uint32_t *label, int64_t n_nodes) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n_nodes) label[p] = (uint32_t)p;
}
void launch_dd_label_init(hipStream_t st, uint32_t *label, int64_t n_nodes) {
  if (n_nodes > 0) hipLaunchKernelGGL(k_dd_label_init, dim3(blocks256(n_nodes)), dim3(256), 0, st, label, n_nodes);
}

// reads `in` only and writes `out` only: the sweeps a run needs do not depend on the schedule
__global__ void __launch_bounds__(256) k_dd_sweep(DdNodes N, const uint64_t *eoff, const uint32_t *in, uint32_t *out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (p < N.n_nodes) {
    const uint32_t mine = in[p];
    uint32_t best = mine;
    for (uint64_t e = eoff[p]; e < eoff[p + 1]; e++) { const uint32_t l = in[N.esrc[e]]; best = l < best ? l : best; }
    out[p] = best;
    changed = best != mine;
  }
  if (__ballot(changed) && changed) N.counters[DD_CHANGED] = 1;
}
void launch_dd_sweep(hipStream_t st, const DdNodes &N, const uint64_t *eoff, const uint32_t *in, uint32_t *out) {
  if (N.n_nodes > 0) hipLaunchKernelGGL(k_dd_sweep, dim3(blocks256(N.n_nodes)), dim3(256), 0, st, N, eoff, in, out);
}

__global__ void __launch_bounds__(256) k_dd_msize(DdNodes N, const uint32_t *label) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < N.n_nodes) atomicAdd(N.msize + label[p], N.cnt[p]);
}
__global__ void __launch_bounds__(256) k_dd_hist(DdNodes N, const uint32_t *label, uint64_t *hist, uint32_t hist_max) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool root = p < N.n_nodes && label[p] == (uint32_t)p;
  if (root) { const uint32_t s = N.msize[p]; atomicAdd((unsigned long long *)hist + (s < hist_max ? s : hist_max), 1ull); }
  count_lanes(root, N.counters + DD_MOLS);
}
void launch_dd_molecules(hipStream_t st, const DdNodes &N, const uint32_t *label, uint64_t *hist, uint32_t hist_max) {
  if (N.n_nodes <= 0) return;
  hipLaunchKernelGGL(k_dd_msize, dim3(blocks256(N.n_nodes)), dim3(256), 0, st, N, label);
  hipLaunchKernelGGL(k_dd_hist, dim3(blocks256(N.n_nodes)), dim3(256), 0, st, N, label, hist, hist_max);
}

__global__ void __launch_bounds__(256) k_dd_verdict(DdNodes N, const uint32_t *label, const uint64_t *nid, const uint32_t *idx, int64_t n, uint32_t *rep,
                                                    uint8_t *dup) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t name = idx[j], r = N.first[label[N.inv[nid[j + 1] - 1]]];
  rep[name] = r; dup[name] = r != name ? 1 : 0;
}
void launch_dd_verdict(hipStream_t st, const DdNodes &N, const uint32_t *label, const uint64_t *nid, const uint32_t *idx, int64_t n, uint32_t *rep,
                       uint8_t *dup) {
  if (n > 0) hipLaunchKernelGGL(k_dd_verdict, dim3(blocks256(n)), dim3(256), 0, st, N, label, nid, idx, n, rep, dup);
}

// ---- records -------------------------------------------------------------------------------------------------------------------
// a record's name: the last name whose rows begin at or in front of it (a name without rows begins where the next one does)
__global__ void __launch_bounds__(256) k_dd_keep(const uint64_t *noff, int64_t n_names, const uint8_t *dup, uint64_t n_rows, int mark, uint64_t *rank,
                                                 uint8_t *rdup) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  int64_t lo = 0, hi = n_names;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (noff[mid] <= 4 * r) lo = mid + 1; else hi = mid; }
  const uint8_t d = lo > 0 ? dup[lo - 1] : 0;
  rdup[r] = d;
  rank[r] = (mark || !d) ? 1 : 0;
}
void launch_dd_keep(hipStream_t st, const uint64_t *noff, int64_t n_names, const uint8_t *dup, uint64_t n_rows, int mark, uint64_t *rank, uint8_t *rdup) {
  if (n_rows) hipLaunchKernelGGL(k_dd_keep, dim3(blocks256((int64_t)n_rows)), dim3(256), 0, st, noff, n_names, dup, n_rows, mark, rank, rdup);
}

__global__ void __launch_bounds__(256) k_dd_select(const uint64_t *rank, const uint64_t *rec_at, uint64_t n_rows, uint32_t *sel, uint64_t *out_len) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows || rank[r + 1] == rank[r]) return;
  sel[rank[r]] = (uint32_t)r;
  out_len[rank[r]] = rec_at[r + 1] - rec_at[r];
}
void launch_dd_select(hipStream_t st, const uint64_t *rank, const uint64_t *rec_at, uint64_t n_rows, uint32_t *sel, uint64_t *out_len) {
  if (n_rows) hipLaunchKernelGGL(k_dd_select, dim3(blocks256((int64_t)n_rows)), dim3(256), 0, st, rank, rec_at, n_rows, sel, out_len);
}

__global__ void __launch_bounds__(256) k_dd_write(const uint8_t *arena, const uint64_t *rec_at, const uint32_t *sel, const uint64_t *out_off,
                                                  const uint8_t *rdup, uint64_t cur, uint64_t e, uint8_t *dst, uint64_t *row_off) {
  constexpr uint64_t per_block = 256 / DD_WRITE_LANES;
  const uint32_t sub = threadIdx.x % DD_WRITE_LANES;
  const uint64_t base = out_off[cur];
  for (uint64_t k = cur + (uint64_t)blockIdx.x * per_block + threadIdx.x / DD_WRITE_LANES; k < e; k += (uint64_t)gridDim.x * per_block) {
    const uint32_t r = sel[k];
    const uint8_t *src = arena + rec_at[r];
    const uint64_t len = rec_at[r + 1] - rec_at[r], to = out_off[k] - base;
    const bool mark = rdup[r] != 0;
    for (uint64_t b = sub; b < len; b += DD_WRITE_LANES) dst[to + b] = (mark && b == 19) ? (uint8_t)(src[b] | 0x04u) : src[b];   // 0x400 of the flag word at 18
    if (sub == 0) { row_off[k - cur] = to; if (k == e - 1) row_off[e - cur] = out_off[e] - base; }
  }
}
void launch_dd_write(hipStream_t st, const uint8_t *arena, const uint64_t *rec_at, const uint32_t *sel, const uint64_t *out_off, const uint8_t *rdup,
                     uint64_t cur, uint64_t e, uint8_t *dst, uint64_t *row_off) {
  const uint64_t n = e - cur;
  if (!n) return;
  const uint64_t blocks = (n + 256 / DD_WRITE_LANES - 1) / (256 / DD_WRITE_LANES);
  hipLaunchKernelGGL(k_dd_write, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, arena, rec_at, sel, out_off, rdup, cur, e, dst, row_off);
}

}  // namespace br
