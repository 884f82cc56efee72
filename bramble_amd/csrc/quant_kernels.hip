// Transcript quantification on the device (host side: quant.cpp, which holds the pipeline's description).
//
//   add      k_q_span, k_q_names (one lane per read name of up to Q_SMALL_ROWS rows) + k_q_names_big (one wave per larger name):
//            the name's distinct transcript ids in ascending order, by repeated selection of the smallest id above the last one,
//            into the label arena at the slot of the name's first row; a 64-bit hash of (labels, k)
//   classes  k_q_flag + scan + k_q_compact: the names with labels; k_q_bits; the collator's radix passes over (hash, name);
//            k_q_heads compares the label lists of neighbours; k_q_resolve orders a run of equal hashes that holds different
//            lists by (k, labels, name); k_q_class_key + radix passes: classes by their first name; k_q_class_fill, k_q_labels
//   names    ("keep_names") k_q_class_inv + k_q_name_cls: every sorted item's class, in the classes' final order, to name_cls[item];
//            k_q_post, after the EM: a lane per class, the posteriors of its label entries
//   table    radix passes over (transcript, label entry) + k_q_transpose: per transcript its classes, ascending; k_q_bin;
//            k_q_counts: unique / ambiguous names per transcript
//   EM       k_q_em_init; k_q_em_classes / k_q_em_tx over a chunk of W replicates with the replicate innermost, a lane per (item,
//            replicate) of up to Q_WAVE_ITEMS entries and a wave per larger item; the point EM is their instantiation for W = 1
//   vb       k_q_vb_part / k_q_vb_sum / k_q_vb_x behind the EM's two kernels: x = exp(psi(alpha + p) - psi(S)) w, S without atomics
//   bootstrap  k_q_boot_sample (a lane per draw: Philox4x32-10, a binary search in the scanned counts, an integer atomicAdd), the
//            EM's kernels on the resampled counts, k_q_boot_store, k_q_boot_summary
//   genes    k_qg_key + radix passes + k_qg_flag + scan + k_qg_arena: a class's distinct genes, ascending; k_qg_hash (a lane, or a
//            wave above Q_WAVE_ITEMS genes); the classes' kernels on the gene lists -- radix passes, k_q_heads, k_q_resolve,
//            k_q_class_key, k_q_class_fill -- with k_qg_member_cnt + scan for the members' counts (an item's weight); k_qg_labels
//            (with the unique / ambiguous names per gene: integer atomics); k_qg_sums (a lane a gene, its transcripts one after
//            the other) and k_qg_boot (a lane per replicate and gene)
//   lengths  ("eff_len") k_q_frag / k_q_frag_big behind the names of an add: per read name of one label the length of its first
//            fragment, counted in LDS by integer atomics and flushed to the add's own table with one integer atomicAdd per
//            non-zero bin and block; k_q_fld_commit adds a good add's table to the run's; at finish k_q_fld_prefix (C and S) and
//            k_q_efflen (eff and w per transcript)
//
// No floating-point atomic anywhere: every sum is one lane's loop in ascending order, or a wave's -- lane l takes the entries
// l, l + 64, ... in ascending order, then the 64 partial sums meet in a fixed xor tree -- so its shape depends on the number of
// entries alone and a result has the same bits in every run.  The largest relative change goes through an integer atomicMax on
// the doubles' bit patterns (a maximum does not depend on the order it is taken in).
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "cigar_inl.h"
#include "collate_kernels.h"
#include "names_inl.h"
#include "quant_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
constexpr uint64_t Q_NO_TID = 1ull << 40;   // above every transcript id
__device__ __forceinline__ uint64_t hash_step(uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; }   // FNV-1a over words
__device__ __forceinline__ uint64_t hash_end(uint64_t h, uint64_t k) {
  h = hash_step(h, k);
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;   // (murmur3 fmix64)
  return h;
}
// the rows of name g of the add: false when they leave the add's rows
// label lists a < b by (k, labels)?  eq: they are equal
__device__ __forceinline__ bool list_less(const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, uint32_t a, uint32_t b, bool &eq) {
  const uint32_t ka = nk[a], kb = nk[b];
  eq = false;
  if (ka != kb) return ka < kb;
  const uint32_t *x = lab + noff[a], *y = lab + noff[b];
  for (uint32_t i = 0; i < ka; i++) if (x[i] != y[i]) return x[i] < y[i];
  eq = true;
  return false;
}
// the class of label entry e: the last c with label_off[c] <= e
__device__ __forceinline__ int64_t class_of_entry(const uint64_t *label_off, int64_t n_cls, int64_t e) {
  int64_t lo = 0, hi = n_cls;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (label_off[mid] <= (uint64_t)e) lo = mid + 1; else hi = mid; }
  return lo - 1;
}
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

__global__ void k_q_span(const uint64_t *row_off, const uint32_t *group_off, int64_t n_groups, uint64_t *span) {
  span[0] = row_off[group_off[0]];
  span[1] = row_off[group_off[n_groups]];
}

__global__ void __launch_bounds__(256) k_q_names(QAddArgs A) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool is_big = false, is_bad = false;
  uint32_t top = 0;
  if (g < A.names.n_groups) {
    uint64_t r0, r1;
    if (!name_rows(A.names, g, r0, r1)) { is_bad = true; A.noff[g] = A.lab_base; A.nk[g] = 0; A.hash[g] = 0; }
    else if (r1 - r0 > (uint64_t)Q_SMALL_ROWS) { is_big = true; A.noff[g] = A.lab_base + (r0 - A.names.r_first); }
    else {
      const uint64_t o = A.lab_base + (r0 - A.names.r_first);
      uint32_t k = 0;
      uint64_t h = 1469598103934665603ull, prev = Q_NO_TID;   // (prev: no label yet)
      for (;;) {
        uint64_t best = Q_NO_TID;
        for (uint64_t r = r0; r < r1; r++) {
          const uint64_t t = A.a[(int64_t)r - A.a_bias].x;
          if ((prev == Q_NO_TID || t > prev) && t < best) best = t;
        }
        if (best == Q_NO_TID) break;
        A.lab[o + k++] = (uint32_t)best;   // k <= r1 - r0: inside the name's slots
        h = hash_step(h, best);
        prev = best;
      }
      if (k) top = (uint32_t)prev;
      A.noff[g] = o; A.nk[g] = k; A.hash[g] = hash_end(h, k);
    }
  }
  const uint64_t bal = __ballot(is_big);
  if (bal) {
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(A.n_big, (uint32_t)__popcll(bal));
    base = __shfl(base, 0);
    if (is_big) A.big[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)g;
  }
  top = wave_max(top);
  if ((threadIdx.x & 63) == 0 && top) atomicMax(A.max_tid, top);
  if (__ballot(is_bad) && is_bad) *A.bad = 1;
}

// one wave per listed name, grid-stride over a list whose length is on the device
__global__ void __launch_bounds__(256) k_q_names_big(QAddArgs A) {
  const int lane = threadIdx.x & 63;
  const uint32_t n_big = *A.n_big;
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n_big; i += gridDim.x * 4) {
    const int64_t g = A.big[i];
    uint64_t r0, r1;
    (void)name_rows(A.names, g, r0, r1);   // (k_q_names listed it: its rows are inside the add's)
    const uint64_t o = A.noff[g];
    uint32_t k = 0;
    uint64_t h = 1469598103934665603ull, prev = Q_NO_TID;
    for (;;) {
      uint64_t best = Q_NO_TID;
      for (uint64_t r = r0 + (uint64_t)lane; r < r1; r += 64) {
        const uint64_t t = A.a[(int64_t)r - A.a_bias].x;
        if ((prev == Q_NO_TID || t > prev) && t < best) best = t;
      }
      best = wave_min(best);
      if (best == Q_NO_TID) break;
      if (lane == 0) A.lab[o + k] = (uint32_t)best;
      k++;
      h = hash_step(h, best);
      prev = best;
    }
    if (lane == 0) {
      A.nk[g] = k; A.hash[g] = hash_end(h, k);
      if (k) atomicMax(A.max_tid, (uint32_t)prev);
    }
  }
}

// ---- fragment lengths ("eff_len"; the definitions: bramble_amd.h, br_quant) --------------------------------------------------------
namespace {
typedef uint32_t q_u4 __attribute__((ext_vector_type(4)));
constexpr uint32_t Q_LEAD = BR_ROW_PAIRED | BR_ROW_SAME_TX | BR_ROW_FIRST;
constexpr uint64_t Q_NO_ROW = ~0ull;
// the rows are read once here: non-temporal, as the projection's other consumers take them
__device__ __forceinline__ q_u4 row_a(const QAddArgs &A, uint64_t r) { return __builtin_nontemporal_load((const q_u4 *)A.a + ((int64_t)r - A.a_bias)); }
__device__ __forceinline__ uint64_t row_cigar(const QAddArgs &A, uint64_t r) { return __builtin_nontemporal_load(A.cigar + ((int64_t)r - A.a_bias)); }
// (the definition's three conditions on the neighbour; on a name of one label, the only kind looked at, its transcript is the leader's anyway)
__device__ __forceinline__ bool is_fragment(const q_u4 lead, const q_u4 mate) {
  return (lead.z & Q_LEAD) == Q_LEAD && (mate.z & (BR_ROW_PAIRED | BR_ROW_FIRST)) == BR_ROW_PAIRED && mate.x == lead.x;
}
__device__ __forceinline__ void count_length(const QAddArgs &A, uint32_t *sh_hist, bool lds, uint64_t lo, uint64_t hi, uint32_t &n_obs, uint32_t &n_oor) {
  const uint64_t len = hi - lo;
  if (len == 0 || len > (uint64_t)A.fld_max) { n_oor++; return; }
  n_obs++;
  if (lds) atomicAdd(sh_hist + len, 1u); else atomicAdd(A.stage + len, 1ull);
}
// the block's counts leave it once: the side counters through LDS, then one integer atomicAdd per non-zero word of the block
__device__ __forceinline__ void frag_flush(const QAddArgs &A, uint32_t *sh_hist, uint32_t *sh_side, bool lds, uint32_t n_obs, uint32_t n_nofrag,
                                           uint32_t n_oor, bool is_bad) {
  n_obs = wave_sum(n_obs); n_nofrag = wave_sum(n_nofrag); n_oor = wave_sum(n_oor);
  if ((threadIdx.x & 63) == 0) {
    if (n_obs) atomicAdd(sh_side + 0, n_obs);
    if (n_nofrag) atomicAdd(sh_side + 1, n_nofrag);
    if (n_oor) atomicAdd(sh_side + 2, n_oor);
  }
  if (__ballot(is_bad) && is_bad) *A.bad = 1;
  __syncthreads();
  const uint32_t n_bins = A.fld_max + 1u;
  if (lds) for (uint32_t i = threadIdx.x; i < n_bins; i += 256) { const uint32_t v = sh_hist[i]; if (v) atomicAdd(A.stage + i, (unsigned long long)v); }
  if (threadIdx.x < Q_FLD_SIDE && sh_side[threadIdx.x]) atomicAdd(A.stage + n_bins + threadIdx.x, (unsigned long long)sh_side[threadIdx.x]);
}
__device__ __forceinline__ void frag_begin(const QAddArgs &A, uint32_t *sh_hist, uint32_t *sh_side, bool lds) {
  if (lds) for (uint32_t i = threadIdx.x; i <= A.fld_max; i += 256) sh_hist[i] = 0;
  if (threadIdx.x < Q_FLD_SIDE) sh_side[threadIdx.x] = 0;
  __syncthreads();
}
}  // namespace

// one lane per read name of one label and at most Q_SMALL_ROWS rows; a pooled CIGAR of more than 64 ops is summed by the wave
template <bool LDS>
__global__ void __launch_bounds__(256) k_q_frag(QAddArgs A) {
  extern __shared__ uint32_t sh_hist[];
  __shared__ uint32_t sh_side[Q_FLD_SIDE];
  frag_begin(A, sh_hist, sh_side, LDS);
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool unique = false, found = false, is_bad = false;
  uint64_t pos[2] = {0, 0}, ref[2] = {0, 0}, wide_off[2] = {0, 0};
  uint32_t wide_n[2] = {0, 0};   // a CIGAR left to the wave
  if (g < A.names.n_groups && A.nk[g] == 1u) {
    uint64_t r0, r1;
    if (name_rows(A.names, g, r0, r1) && r1 - r0 <= (uint64_t)Q_SMALL_ROWS) {   // (one label: it has a row)
      unique = true;
      uint64_t fr = 0;
      q_u4 lead = row_a(A, r0), mate = lead;
      for (uint64_t r = r0; r + 1 < r1; r++) {
        mate = row_a(A, r + 1);
        if (is_fragment(lead, mate)) { found = true; fr = r; break; }
        lead = mate;
      }
      if (found) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const q_u4 m = j ? mate : lead;
          const uint32_t n = BR_ROW_NCIGAR(m.z);
          const uint64_t c = row_cigar(A, fr + (uint64_t)j);
          pos[j] = m.y;
          if (n <= 2u) ref[j] = cigar_ref_len_inline(c, n);
          else if (!pool_holds(A.n_pool_words, c, n)) is_bad = true;
          else if (n <= 64u) { uint64_t s = 0; for (uint32_t k = 0; k < n; k++) s += cigar_ref_len(A.pool[c + k]); ref[j] = s; }
          else { wide_off[j] = c; wide_n[j] = n; }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; j++)
    wave_turns(wide_n[j] != 0u && !is_bad, [&](int src) {
      const uint64_t s = wave_cigar_ref_len(A.pool, __shfl(wide_off[j], src), (uint32_t)__shfl((int)wide_n[j], src));
      if (lane == src) ref[j] = s;
    });
  uint32_t n_obs = 0, n_oor = 0;
  if (found && !is_bad) {
    const uint64_t lo = pos[0] < pos[1] ? pos[0] : pos[1], e0 = pos[0] + ref[0], e1 = pos[1] + ref[1];
    count_length(A, sh_hist, LDS, lo, e0 > e1 ? e0 : e1, n_obs, n_oor);
  }
  frag_flush(A, sh_hist, sh_side, LDS, n_obs, unique && !found ? 1u : 0u, n_oor, is_bad);
}

// one wave per listed name (the list k_q_names made of the names of more than Q_SMALL_ROWS rows), grid-stride: the lanes scan the
// rows in strides of 64 (one load a row; the neighbour by shuffle), the lowest row that leads a fragment is a wave minimum, and the
// wave sums the two CIGARs
template <bool LDS>
__global__ void __launch_bounds__(256) k_q_frag_big(QAddArgs A) {
  extern __shared__ uint32_t sh_hist[];
  __shared__ uint32_t sh_side[Q_FLD_SIDE];
  frag_begin(A, sh_hist, sh_side, LDS);
  const int lane = threadIdx.x & 63;
  const uint32_t n_big = *A.n_big;
  uint32_t n_obs = 0, n_nofrag = 0, n_oor = 0;   // (lane 0 counts for the wave)
  bool is_bad = false;
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n_big; i += gridDim.x * 4) {
    const int64_t g = A.big[i];
    if (A.nk[g] != 1u) continue;   // (wave-uniform, as everything below that branches)
    uint64_t r0, r1;
    (void)name_rows(A.names, g, r0, r1);
    uint64_t fr = Q_NO_ROW;
    for (uint64_t base = r0; fr == Q_NO_ROW && base + 1 < r1; base += 64) {
      // a row is loaded once: the neighbour's transcript and meta come from the next lane, lane 63's from the stride's edge
      const uint64_t r = base + (uint64_t)lane;
      q_u4 lead = {0u, 0u, 0u, 0u}, mate = {0u, 0u, 0u, 0u};
      if (r < r1) lead = row_a(A, r);
      mate.x = (uint32_t)__shfl_down((int)lead.x, 1); mate.z = (uint32_t)__shfl_down((int)lead.z, 1);
      if (lane == 63 && r + 1 < r1) mate = row_a(A, r + 1);
      fr = wave_min(r + 1 < r1 && is_fragment(lead, mate) ? r : Q_NO_ROW);
    }
    if (fr == Q_NO_ROW) { if (lane == 0) n_nofrag++; continue; }
    uint64_t pos[2], ref[2];
    bool ok = true;
    for (int j = 0; j < 2; j++) {
      const q_u4 m = row_a(A, fr + (uint64_t)j);
      const uint32_t n = BR_ROW_NCIGAR(m.z);
      const uint64_t c = row_cigar(A, fr + (uint64_t)j);
      pos[j] = m.y; ref[j] = 0;
      if (n <= 2u) ref[j] = cigar_ref_len_inline(c, n);
      else if (!pool_holds(A.n_pool_words, c, n)) ok = false;
      else ref[j] = wave_cigar_ref_len(A.pool, c, n);
    }
    if (!ok) { is_bad = true; continue; }
    if (lane == 0) {
      const uint64_t lo = pos[0] < pos[1] ? pos[0] : pos[1], e0 = pos[0] + ref[0], e1 = pos[1] + ref[1];
      count_length(A, sh_hist, LDS, lo, e0 > e1 ? e0 : e1, n_obs, n_oor);
    }
  }
  frag_flush(A, sh_hist, sh_side, LDS, n_obs, n_nofrag, n_oor, is_bad);
}

__global__ void __launch_bounds__(256) k_q_fld_commit(unsigned long long *stage, unsigned long long *total, uint32_t n_words) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_words) return;
  const unsigned long long v = stage[i];
  if (v) { total[i] += v; stage[i] = 0; }
}

// one block: thread k takes bins [k * per, (k + 1) * per), the 256 partial sums are scanned by thread 0 (integers: exact in any order)
__global__ void __launch_bounds__(256) k_q_fld_prefix(const unsigned long long *hist, uint32_t n_bins, uint64_t *cs) {
  __shared__ uint64_t sh_c[256], sh_s[256];
  const uint32_t per = (n_bins + 255u) / 256u, b = threadIdx.x * per, e = b + per < n_bins ? b + per : n_bins;
  uint64_t c = 0, s = 0;
  for (uint32_t f = b; f < e; f++) { c += hist[f]; s += (uint64_t)f * hist[f]; }
  sh_c[threadIdx.x] = c; sh_s[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t tc = 0, ts = 0;
    for (int k = 0; k < 256; k++) { const uint64_t vc = sh_c[k], vs = sh_s[k]; sh_c[k] = tc; sh_s[k] = ts; tc += vc; ts += vs; }
  }
  __syncthreads();
  c = sh_c[threadIdx.x]; s = sh_s[threadIdx.x];
  for (uint32_t f = b; f < e; f++) { c += hist[f]; s += (uint64_t)f * hist[f]; cs[f] = c; cs[n_bins + f] = s; }
}

// one lane per transcript: eff = ((L + 1) C(x) - S(x)) / C(x) at x = min(L, fld_max), L where C(x) is 0; w = 1 / eff
template <bool LDS>
__global__ void __launch_bounds__(256) k_q_efflen(const int64_t *lens, int64_t n_tx, const uint64_t *cs, uint32_t n_bins, double *eff, double *w) {
  extern __shared__ uint64_t sh_cs[];
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < 2u * n_bins; i += 256) sh_cs[i] = cs[i];
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tx) return;
  const uint64_t *tab = LDS ? sh_cs : cs;
  const int64_t len = lens[t];
  double e = 0.0;
  if (len > 0) {
    const uint64_t x = (uint64_t)len < (uint64_t)(n_bins - 1u) ? (uint64_t)len : (uint64_t)(n_bins - 1u);
    const uint64_t c = tab[x], s = tab[n_bins + x];
    e = c == 0 ? (double)len : (double)(((uint64_t)len + 1ull) * c - s) / (double)c;
  }
  eff[t] = e; w[t] = e > 0.0 ? 1.0 / e : 0.0;
}

__global__ void __launch_bounds__(256) k_q_drop(const uint8_t *flags, int64_t n, uint32_t *nk, unsigned long long *n_dropped) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool drop = i < n && flags[i] != 0;
  if (drop) nk[i] = 0;
  const uint64_t bal = __ballot(drop);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_dropped, (unsigned long long)__popcll((unsigned long long)bal));
}
__global__ void __launch_bounds__(256) k_q_flag(const uint32_t *nk, int64_t n, uint64_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = nk[i] ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_q_compact(const uint32_t *nk, const uint64_t *hash, const uint64_t *pos, int64_t n, uint64_t mask,
                                                   uint64_t *key, uint32_t *idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && nk[i]) { key[pos[i]] = hash[i] & mask; idx[pos[i]] = (uint32_t)i; }
}
__global__ void __launch_bounds__(256) k_q_bits_part(const uint64_t *key, int64_t n, uint64_t *part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  block_bits(i < n ? key[i] : 0, i < n ? key[i] : ~0ull, part + 2 * blockIdx.x);
}

__global__ void __launch_bounds__(256) k_q_heads(const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, const uint64_t *key,
                                                 const uint32_t *idx, int64_t n, uint64_t *head, unsigned long long *n_coll, uint32_t *mark) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool coll = false;
  if (j < n) {
    uint64_t h = 1;
    if (j > 0 && key[j] == key[j - 1]) {
      bool eq;
      (void)list_less(lab, noff, nk, idx[j], idx[j - 1], eq);
      h = eq ? 0 : 1;
      coll = !eq;
      if (coll && mark) {   // the run's first item: the lower bound of the key (every writer stores the same 1)
        const uint64_t kj = key[j];
        int64_t lo = 0, hi = j - 1;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] < kj) lo = mid + 1; else hi = mid; }
        mark[lo] = 1;
      }
    }
    head[j] = h;
  }
  const uint64_t bal = __ballot(coll);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_coll, (unsigned long long)__popcll(bal));   // (collisions only: none with 64-bit keys in practice)
}

// an item of a marked run goes to the run's start + the number of the run's items in front of it by (k, labels, name index);
// quadratic in the run, which is as long as hash_bits makes it (the test hook) and not at all with 64 bits
__global__ void __launch_bounds__(256) k_q_resolve(const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, const uint64_t *key,
                                                   const uint32_t *idx, int64_t n, const uint32_t *mark, uint64_t *key_out, uint32_t *idx_out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t kj = key[j];
  const uint32_t me = idx[j];
  int64_t lo = 0, hi = j;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] < kj) lo = mid + 1; else hi = mid; }
  const int64_t b = lo;
  int64_t pos = j;
  if (mark[b]) {
    lo = j + 1; hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] <= kj) lo = mid + 1; else hi = mid; }
    int64_t rank = 0;
    for (int64_t i = b; i < lo; i++) {
      if (i == j) continue;
      const uint32_t other = idx[i];
      bool eq;
      const bool less = list_less(lab, noff, nk, other, me, eq);
      if (less || (eq && other < me)) rank++;
    }
    pos = b + rank;
  }
  key_out[pos] = kj; idx_out[pos] = me;
}

// An item's first name is item_first[i], or i itself where the table is NULL; the items of a class ascend, and so do their first
// names, so a class's first item has its first name
__global__ void __launch_bounds__(256) k_q_class_key(const uint64_t *gbeg, const uint32_t *idx, const uint64_t *item_first, int64_t n_cls,
                                                     uint64_t *key, uint32_t *val) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cls) return;
  const uint32_t i = idx[gbeg[c]];
  key[c] = item_first ? item_first[i] : (uint64_t)i; val[c] = (uint32_t)c;
}
// An item's weight is 1 where pre is NULL (a class counts its items), else pre holds the scanned weights of the sorted items
__global__ void __launch_bounds__(256) k_q_class_fill(const uint64_t *key, const uint32_t *val, const uint64_t *gbeg, const uint32_t *idx,
                                                      const uint64_t *pre, const uint32_t *nk, int64_t n_cls, uint64_t *first, uint64_t *cnt,
                                                      uint64_t *label_off, uint32_t *rep) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cls) return;
  const uint32_t s = val[c], r = idx[gbeg[s]];
  first[c] = key[c]; cnt[c] = pre ? pre[gbeg[s + 1]] - pre[gbeg[s]] : gbeg[s + 1] - gbeg[s]; label_off[c] = nk[r];
  if (rep) rep[c] = r;
}
// "keep_names": inv[class in hash order] = the class in its final order (val, after the second sort), then a lane per sorted item
// j -- its class in hash order is the heads up to and including j, less one, and head holds the exclusive scan -- stores
// name_cls[item] = that class's final index.  The names without labels were never items: they keep the caller's 0xffffffff
__global__ void __launch_bounds__(256) k_q_class_inv(const uint32_t *val, int64_t n_cls, uint32_t *inv) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < n_cls) inv[val[c]] = (uint32_t)c;
}
__global__ void __launch_bounds__(256) k_q_name_cls(const uint64_t *head, const uint32_t *idx, int64_t n, const uint32_t *inv, int64_t n_cls,
                                                    uint32_t *name_cls) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint64_t s = head[j + 1] - 1;
  if (s < (uint64_t)n_cls) name_cls[idx[j]] = inv[s];
}
// The posteriors (bramble_amd.h, br_quant): a lane per class, its labels one after the other whatever their number, so that the
// shape of the sum is the definition's; one rounding per operation (the unit is built without contraction)
__global__ void __launch_bounds__(256) k_q_post(const uint64_t *label_off, const uint32_t *labels, int64_t n_cls, const double *theta,
                                                const double *w, double *post) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cls) return;
  const uint64_t b = label_off[c], e = label_off[c + 1];
  double d = 0.0;
  if (!w) {   // (theta is x itself: a variational run's)
    for (uint64_t i = b; i < e; i++) d += theta[labels[i]];
    for (uint64_t i = b; i < e; i++) post[i] = d == 0.0 ? 0.0 : theta[labels[i]] / d;
    return;
  }
  for (uint64_t i = b; i < e; i++) { const uint32_t t = labels[i]; d += theta[t] * w[t]; }
  for (uint64_t i = b; i < e; i++) { const uint32_t t = labels[i]; post[i] = d == 0.0 ? 0.0 : (theta[t] * w[t]) / d; }
}
__global__ void __launch_bounds__(256) k_q_labels(const uint64_t *label_off, const uint64_t *first, const uint64_t *noff, const uint32_t *lab,
                                                  int64_t n_cls, int64_t n_lab, const int64_t *lens, uint32_t *labels, uint32_t *ecls,
                                                  uint64_t *tkey, uint32_t *tidx, uint32_t *bad) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_lab) return;
  const int64_t c = class_of_entry(label_off, n_cls, e);
  const uint32_t t = lab[noff[first[c]] + ((uint64_t)e - label_off[c])];
  labels[e] = t; ecls[e] = (uint32_t)c; tkey[e] = t; tidx[e] = (uint32_t)e;
  if (lens && lens[t] <= 0) *bad = 1;
}
__global__ void __launch_bounds__(256) k_q_transpose(const uint64_t *tkey, const uint32_t *tidx, const uint32_t *ecls, int64_t n_lab,
                                                     int64_t n_tx, uint32_t *t_cls, uint64_t *t_off) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_lab) t_cls[i] = ecls[tidx[i]];
  if (i <= n_tx) {   // the first pair of transcript i (n_lab for i = n_tx)
    int64_t lo = 0, hi = n_lab;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (tkey[mid] < (uint64_t)i) lo = mid + 1; else hi = mid; }
    t_off[i] = (uint64_t)lo;
  }
}
__global__ void __launch_bounds__(256) k_q_bin(const uint64_t *off, int64_t n, uint32_t *list, uint32_t *n_list) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool big = i < n && off[i + 1] - off[i] > (uint64_t)Q_WAVE_ITEMS;
  const uint64_t bal = __ballot(big);
  if (!bal) return;
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(n_list, (uint32_t)__popcll(bal));
  base = __shfl(base, 0);
  if (big) list[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)i;
}

// names per transcript whose class is the transcript alone / holds it beside others
template <bool BIG>
__global__ void __launch_bounds__(256) k_q_counts(const uint32_t *t_cls, const uint64_t *t_off, const uint64_t *label_off, const uint64_t *cnt,
                                                  int64_t n_tx, const uint32_t *big, uint32_t n_big, uint64_t *uniq, uint64_t *ambig) {
  if (BIG) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_big) return;
    const uint32_t t = big[i];
    uint64_t u = 0, a = 0;
    for (uint64_t p = t_off[t] + (uint64_t)lane; p < t_off[t + 1]; p += 64) {
      const uint32_t c = t_cls[p];
      if (label_off[c + 1] - label_off[c] == 1) u += cnt[c]; else a += cnt[c];
    }
    u = wave_sum(u); a = wave_sum(a);
    if (lane == 0) { uniq[t] = u; ambig[t] = a; }
  } else {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tx || t_off[t + 1] - t_off[t] > (uint64_t)Q_WAVE_ITEMS) return;
    uint64_t u = 0, a = 0;
    for (uint64_t p = t_off[t]; p < t_off[t + 1]; p++) {
      const uint32_t c = t_cls[p];
      if (label_off[c + 1] - label_off[c] == 1) u += cnt[c]; else a += cnt[c];
    }
    uniq[t] = u; ambig[t] = a;
  }
}

// ---- EM (the definitions: bramble_amd.h, br_quant) ---------------------------------------------------------------------------------
// A chunk is W = 1 << lw replicates; x, theta, q and the resampled counts hold replicate j of item i at [i * W + j], so one read of
// an index table serves W replicates and a gather is W * 8 contiguous bytes.  A replicate's sums do not know W -- a lane's
// ascending loop, or lane l's entries l, l + 64, ... and the xor tree -- so its bits are those of the EM run alone on its counts.
// A replicate whose bit in `active` is clear is frozen: its theta and x are copied through.  POINT: the point EM, a chunk of one
// replicate on the observed counts -- lw = 0, active = 1 and one replicate a walk are compile-time facts, E's own are not read
__global__ void __launch_bounds__(256) k_q_em_init(const double *w, int64_t n_tx, int lw, double *theta, double *x) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if ((g >> lw) >= n_tx) return;
  theta[g] = 1.0; x[g] = w[g >> lw];
}

__device__ __forceinline__ uint64_t rel_bits(double now, double before) {
  if (!(now > 1e-8)) return 0;
  return (uint64_t)__double_as_longlong(fabs(now - before) / now);
}

constexpr int Q_BOOT_SUB = 4;   // replicates a wave carries through one walk over a large item's entries

template <bool BIG, bool POINT>
__global__ void __launch_bounds__(256) k_q_em_classes(QEmArgs E, const double *x) {
  constexpr int SUB = POINT ? 1 : Q_BOOT_SUB;
  const int lw = POINT ? 0 : E.lw, W = 1 << lw;
  const uint64_t active = POINT ? 1ull : E.active;
  if (BIG) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= E.n_big_cls) return;
    const uint64_t c = E.big_cls[i];
    const uint64_t e0 = E.label_off[c], e1 = E.label_off[c + 1];
    for (int j0 = 0; j0 < W; j0 += SUB) {
      if (((active >> j0) & ((1ull << SUB) - 1ull)) == 0) continue;
      double d[SUB];
#pragma unroll
      for (int k = 0; k < SUB; k++) d[k] = 0.0;
      for (uint64_t e = e0 + (uint64_t)lane; e < e1; e += 64) {
        const double *p = x + (((uint64_t)E.labels[e] << lw) + (uint64_t)j0);
#pragma unroll
        for (int k = 0; k < SUB; k++) if (j0 + k < W) d[k] += p[k];
      }
#pragma unroll
      for (int k = 0; k < SUB; k++) {
        const double s = wave_sum(d[k]);
        if (lane == 0 && j0 + k < W && ((active >> (j0 + k)) & 1ull)) {
          const uint64_t g = (c << lw) + (uint64_t)(j0 + k);
          E.q[g] = s > 0.0 ? (POINT ? (double)E.cnt[g] : (double)E.boot_cnt[g]) / s : 0.0;
        }
      }
    }
  } else {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t c = g >> lw;
    const int j = (int)(g & (int64_t)(W - 1));
    if (c >= E.n_cls || !((active >> j) & 1ull)) return;
    const uint64_t b = E.label_off[c], e1 = E.label_off[c + 1];
    if (e1 - b > (uint64_t)Q_WAVE_ITEMS) return;
    double d = 0.0;
    for (uint64_t e = b; e < e1; e++) d += x[((uint64_t)E.labels[e] << lw) + (uint64_t)j];
    E.q[g] = d > 0.0 ? (POINT ? (double)E.cnt[g] : (double)E.boot_cnt[g]) / d : 0.0;
  }
}

template <bool BIG, bool POINT>
__global__ void __launch_bounds__(256) k_q_em_tx(QEmArgs E, const double *theta, const double *x, double *theta_out, double *x_out,
                                                 unsigned long long *rel) {
  constexpr int SUB = POINT ? 1 : Q_BOOT_SUB;
  const int lw = POINT ? 0 : E.lw, W = 1 << lw;
  const uint64_t active = POINT ? 1ull : E.active;
  const int lane = threadIdx.x & 63;
  if (BIG) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= E.n_big_tx) return;   // (wave-uniform)
    const uint64_t t = E.big_tx[i];
    const uint64_t p0 = E.t_off[t], p1 = E.t_off[t + 1];
    for (int j0 = 0; j0 < W; j0 += SUB) {
      if (((active >> j0) & ((1ull << SUB) - 1ull)) == 0) continue;
      double s[SUB];
#pragma unroll
      for (int k = 0; k < SUB; k++) s[k] = 0.0;
      for (uint64_t p = p0 + (uint64_t)lane; p < p1; p += 64) {
        const double *qp = E.q + (((uint64_t)E.t_cls[p] << lw) + (uint64_t)j0);
#pragma unroll
        for (int k = 0; k < SUB; k++) if (j0 + k < W) s[k] += qp[k];
      }
#pragma unroll
      for (int k = 0; k < SUB; k++) {
        const double sum = wave_sum(s[k]);
        if (lane == 0 && j0 + k < W && ((active >> (j0 + k)) & 1ull)) {
          const uint64_t g = (t << lw) + (uint64_t)(j0 + k);
          const double now = x[g] * sum;
          theta_out[g] = now; x_out[g] = now * E.w[t];
          if (rel) { const uint64_t r = rel_bits(now, theta[g]); if (r) atomicMax(rel + j0 + k, (unsigned long long)r); }
        }
      }
    }
    if (lane < W && !((active >> lane) & 1ull)) {   // the frozen ones
      const uint64_t g = (t << lw) + (uint64_t)lane;
      theta_out[g] = theta[g]; x_out[g] = x[g];
    }
  } else {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = g >> lw;
    const int j = (int)(g & (int64_t)(W - 1));
    uint64_t r = 0;
    if (t < E.n_tx && E.t_off[t + 1] - E.t_off[t] <= (uint64_t)Q_WAVE_ITEMS) {
      if ((active >> j) & 1ull) {
        double s = 0.0;
        for (uint64_t p = E.t_off[t]; p < E.t_off[t + 1]; p++) s += E.q[((uint64_t)E.t_cls[p] << lw) + (uint64_t)j];
        const double now = x[g] * s;
        theta_out[g] = now; x_out[g] = now * E.w[t];
        if (rel) r = rel_bits(now, theta[g]);
      } else { theta_out[g] = theta[g]; x_out[g] = x[g]; }
    }
    if (rel) {   // lanes l, l + W, ... of a wave hold replicate l: a xor tree over those, then one atomicMax a wave and replicate
      for (int d = 32; d >= W; d >>= 1) { const uint64_t y = __shfl_xor(r, d); r = y > r ? y : r; }
      if (lane < W && r) atomicMax(rel + lane, (unsigned long long)r);
    }
  }
}

// ---- bootstrap replicates (the definitions: bramble_amd.h, br_quant) -------------------------------------------------------------
namespace {
// Philox4x32-10 of counter (c0, c1, c2, 0) under key (k0, k1): the first two output words as one 64-bit number
__device__ __forceinline__ uint64_t philox_u64(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1) {
  uint32_t c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (uint64_t)c0 | ((uint64_t)c1 << 32);
}
}  // namespace

// one lane per draw; blockIdx.y: the replicate of the launch.  The count of class c and replicate y is out[c * stride_c + y * stride_b]
__global__ void __launch_bounds__(256) k_q_boot_sample(const uint64_t *cum, int64_t n_cls, uint64_t n, uint32_t k0, uint32_t k1, uint32_t b_first,
                                                       uint32_t *out, int64_t stride_c, int64_t stride_b) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t u = philox_u64((uint32_t)i, (uint32_t)(i >> 32), b_first + blockIdx.y, k0, k1);
  const uint64_t r = __umul64hi(u, n);   // < n = cum[n_cls]
  int64_t lo = 0, hi = n_cls;            // the last class c with cum[c] <= r (cum[0] = 0: there is one)
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (cum[mid] <= r) lo = mid + 1; else hi = mid; }
  atomicAdd(out + (lo - 1) * stride_c + (int64_t)blockIdx.y * stride_b, 1u);
}

// the chunk's theta (replicate innermost) -> the rows of its first n_rep replicates in the result (replicate-major)
__global__ void __launch_bounds__(256) k_q_boot_store(const double *theta, int64_t n_tx, int lw, int n_rep, double *out) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t t = g >> lw;
  const int j = (int)(g & (int64_t)((1 << lw) - 1));
  if (t < n_tx && j < n_rep) out[(int64_t)j * n_tx + t] = theta[g];
}

// one lane per transcript over the n_boot x n_tx result, both sums in replicate order (built with -ffp-contract=off: no fused multiply-add)
__global__ void __launch_bounds__(256) k_q_boot_summary(const double *res, int64_t n_tx, int32_t n_boot, double *mean, double *var) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tx) return;
  double s = 0.0;
  for (int32_t b = 0; b < n_boot; b++) s += res[(int64_t)b * n_tx + t];
  const double m = s / (double)n_boot;
  double v = 0.0;
  for (int32_t b = 0; b < n_boot; b++) { const double d = res[(int64_t)b * n_tx + t] - m; v = __dadd_rn(v, __dmul_rn(d, d)); }
  mean[t] = m; var[t] = n_boot > 1 ? v / (double)(n_boot - 1) : 0.0;
}

// ---- variational Bayes (the definitions: bramble_amd.h, br_quant, paragraph `variational`) -------------------------------------------
// An iteration is the EM's two kernels -- they read x and write alpha' = x * (sum of q); the x they write beside it is replaced --
// and then x = exp(psi(alpha' + p) - psi(S)) * w, which needs S of the whole new alpha: k_q_vb_part (a partial per 256
// transcripts), k_q_vb_sum (the partials in a fixed order, psi(S) once a replicate), k_q_vb_x (a lane per (transcript,
// replicate)).  The point EM is a chunk of one replicate (lw = 0, active = 1).  No atomics: the shape of S depends on n_tx alone.
namespace {
// psi(a), a > 0: psi(a) = psi(a + 1) - 1 / a until the argument is 16 or more, then the asymptotic series through 1 / (132 a^10).
// The trip count differs between lanes (0 for a transcript with 16 reads or more, 16 below 1); the body is one division and two adds
__device__ __forceinline__ double q_digamma(double a) {
  double r = 0.0;
  while (a < 16.0) { r += 1.0 / a; a += 1.0; }
  const double i = 1.0 / a, z = i * i;
  const double tail = z * (1.0 / 12.0 - z * (1.0 / 120.0 - z * (1.0 / 252.0 - z * (1.0 / 240.0 - z * (1.0 / 132.0)))));
  return ((log(a) - 0.5 * i) - tail) - r;
}
constexpr int Q_VB_SUB = 8;   // replicates a lane loads before it reduces them: 64 contiguous bytes of its transcript's row
}  // namespace

__global__ void __launch_bounds__(256) k_q_digamma(const double *a, int64_t n, double *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = a[i];
  out[i] = v > 0.0 && v <= 1.79769313486231570815e308 ? q_digamma(v) : __longlong_as_double(0x7ff8000000000000ll);   // (the recurrence ends only for these)
}

// part[b * W + j] = the sum of theta[t * W + j] + prior[t] over the transcripts t of block b = [256 b, 256 b + 256): a xor tree per
// wave, then the four waves in order -- whatever W is, so a replicate's partials are the point run's
__global__ void __launch_bounds__(256) k_q_vb_part(const double *theta, const double *prior, int64_t n_tx, int lw, uint64_t active, double *part) {
  __shared__ double sh[64 * 4];
  const int W = 1 << lw;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = t < n_tx;
  const double p = in ? prior[t] : 0.0;
  const double *row = theta + ((in ? t : 0) << lw);
  for (int j0 = 0; j0 < W; j0 += Q_VB_SUB) {
    if (((active >> j0) & ((1ull << Q_VB_SUB) - 1ull)) == 0) continue;   // (block-uniform)
    double v[Q_VB_SUB];
#pragma unroll
    for (int k = 0; k < Q_VB_SUB; k++) v[k] = in && j0 + k < W ? row[j0 + k] + p : 0.0;
#pragma unroll
    for (int k = 0; k < Q_VB_SUB; k++) {
      const double s = wave_sum(v[k]);
      if ((threadIdx.x & 63) == 0 && j0 + k < W) sh[(j0 + k) * 4 + (threadIdx.x >> 6)] = s;
    }
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < W && ((active >> j) & 1ull)) part[(int64_t)blockIdx.x * W + j] = ((sh[j * 4] + sh[j * 4 + 1]) + sh[j * 4 + 2]) + sh[j * 4 + 3];
}

// block j: S of replicate j from its n_part partials -- thread i adds partials i, i + 256, ... in ascending order, then the block
// sum of k_q_vb_part -- and psi_s[j] = psi(S) (0 where S is 0: every A is 0 then, and no x reads it)
__global__ void __launch_bounds__(256) k_q_vb_sum(const double *part, int64_t n_part, int lw, uint64_t active, double *psi_s) {
  __shared__ double sh[4];
  const int j = blockIdx.x;
  if (!((active >> j) & 1ull)) return;   // (block-uniform)
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < n_part; b += 256) s += part[(b << lw) + j];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double S = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    psi_s[j] = S > 0.0 ? q_digamma(S) : 0.0;
  }
}

// x[t * W + j] = exp(psi(A) - psi(S_j)) * w[t] with A = theta[t * W + j] + prior[t], 0 where A <= 1e-10 (salmon's digammaMin); a
// frozen replicate keeps the x the transcript kernel copied through
__global__ void __launch_bounds__(256) k_q_vb_x(const double *theta, const double *prior, const double *w, int64_t n_tx, int lw, uint64_t active,
                                                const double *psi_s, double *x_out) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t t = g >> lw;
  const int j = (int)(g & (int64_t)((1 << lw) - 1));
  if (t >= n_tx || !((active >> j) & 1ull)) return;
  const double A = theta[g] + prior[t];
  x_out[g] = A > 1e-10 ? exp(q_digamma(A) - psi_s[j]) * w[t] : 0.0;
}

void launch_q_digamma(hipStream_t st, const double *a, int64_t n, double *out) {
  if (n > 0) hipLaunchKernelGGL(k_q_digamma, dim3(blocks256(n)), dim3(256), 0, st, a, n, out);
}
void launch_q_vb_x(hipStream_t st, const double *theta, const double *prior, const double *w, int64_t n_tx, int lw, uint64_t active, double *part,
                   double *psi_s, double *x_out) {
  if (n_tx <= 0 || !active) return;
  const int64_t n_part = (n_tx + 255) / 256;
  hipLaunchKernelGGL(k_q_vb_part, dim3((unsigned)n_part), dim3(256), 0, st, theta, prior, n_tx, lw, active, part);
  hipLaunchKernelGGL(k_q_vb_sum, dim3(1u << lw), dim3(256), 0, st, (const double *)part, n_part, lw, active, psi_s);
  hipLaunchKernelGGL(k_q_vb_x, dim3(blocks256(n_tx << lw)), dim3(256), 0, st, theta, prior, w, n_tx, lw, active, (const double *)psi_s, x_out);
}

// ---- gene level (the definitions: bramble_amd.h, br_quant) -------------------------------------------------------------------------
// The transcript classes relabelled by gene and merged.  A class's gene list -- the distinct genes of its labels, ascending --
// comes from one radix sort of (class, gene) keys; the lists then go through the classes' kernels as items whose first name is
// the transcript class's and whose weight is its count (k_qg_member_cnt gathers the weights in sorted order, to be scanned).
__global__ void __launch_bounds__(256) k_qg_key(const uint64_t *label_off, const uint32_t *labels, const uint32_t *tx_gene, int64_t n_cls,
                                                int64_t n_lab, uint64_t *key, uint32_t *idx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_lab) return;
  key[e] = ((uint64_t)class_of_entry(label_off, n_cls, e) << 32) | (uint64_t)tx_gene[labels[e]];
  idx[e] = (uint32_t)e;
}
__global__ void __launch_bounds__(256) k_qg_flag(const uint64_t *key, int64_t n, uint64_t *flag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) flag[e] = e == 0 || key[e] != key[e - 1] ? 1 : 0;
}
// pos: the scanned flags.  The sorted keys keep a class's entries in its own range of label_off, so its list starts at
// pos[label_off[c]] of the arena
__global__ void __launch_bounds__(256) k_qg_arena(const uint64_t *key, const uint64_t *pos, const uint64_t *label_off, int64_t n_lab,
                                                  int64_t n_cls, uint32_t *glab, uint64_t *goff, uint32_t *gk) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_lab && pos[i + 1] != pos[i]) glab[pos[i]] = (uint32_t)key[i];
  if (i <= n_cls) goff[i] = pos[label_off[i]];
  if (i < n_cls) gk[i] = (uint32_t)(pos[label_off[i + 1]] - pos[label_off[i]]);
}
// the hash the names get, of a class's gene list: a lane per list of up to Q_WAVE_ITEMS genes; a wave per larger one loads 64
// genes at a time and every lane steps through them (the chain is sequential)
template <bool BIG>
__global__ void __launch_bounds__(256) k_qg_hash(const uint32_t *glab, const uint64_t *goff, int64_t n_cls, const uint32_t *big, uint32_t n_big,
                                                 uint64_t mask, uint64_t *key, uint32_t *idx) {
  if (BIG) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_big) return;   // (wave-uniform)
    const uint32_t c = big[i];
    const uint64_t o = goff[c], k = goff[c + 1] - o;
    uint64_t h = 1469598103934665603ull;
    for (uint64_t base = 0; base < k; base += 64) {
      const uint32_t v = base + (uint64_t)lane < k ? glab[o + base + (uint64_t)lane] : 0u;
      const int n = k - base < 64 ? (int)(k - base) : 64;
      for (int j = 0; j < n; j++) h = hash_step(h, (uint64_t)(uint32_t)__shfl((int)v, j));
    }
    if (lane == 0) { key[c] = hash_end(h, k) & mask; idx[c] = c; }
  } else {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cls) return;
    const uint64_t o = goff[c], k = goff[c + 1] - o;
    if (k > (uint64_t)Q_WAVE_ITEMS) return;
    uint64_t h = 1469598103934665603ull;
    for (uint64_t j = 0; j < k; j++) h = hash_step(h, glab[o + j]);
    key[c] = hash_end(h, k) & mask; idx[c] = (uint32_t)c;
  }
}
__global__ void __launch_bounds__(256) k_qg_member_cnt(const uint32_t *idx, const uint64_t *cnt, int64_t n, uint64_t *w) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) w[j] = cnt[idx[j]];
}
// one lane per gene-label entry: the label, and the class's count to its gene's unique or ambiguous names (integer atomics)
__global__ void __launch_bounds__(256) k_qg_labels(const uint64_t *label_off, const uint32_t *rep, const uint64_t *goff, const uint32_t *glab,
                                                   const uint64_t *cnt, int64_t n_cls, int64_t n_lab, uint32_t *labels,
                                                   unsigned long long *uniq, unsigned long long *ambig) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_lab) return;
  const int64_t c = class_of_entry(label_off, n_cls, e);
  const uint32_t g = glab[goff[rep[c]] + ((uint64_t)e - label_off[c])];
  labels[e] = g;
  atomicAdd((label_off[c + 1] - label_off[c] == 1 ? uniq : ambig) + g, (unsigned long long)cnt[c]);
}
// one lane per gene, its transcripts one after the other in ascending order; every product is rounded before it is added
__global__ void __launch_bounds__(256) k_qg_sums(const uint64_t *g_toff, const uint32_t *g_tx, int64_t n_genes, const double *theta,
                                                 const double *tpm_t, const int64_t *lens, const double *eff, double *num_reads, double *tpm,
                                                 double *length, double *eff_length) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_genes) return;
  const uint64_t p0 = g_toff[g], p1 = g_toff[g + 1];
  double nr = 0.0, tp = 0.0, wl = 0.0, sl = 0.0, we = 0.0, se = 0.0;
  for (uint64_t p = p0; p < p1; p++) {
    const uint32_t t = g_tx[p];
    const double v = tpm_t[t];
    nr = __dadd_rn(nr, theta[t]); tp = __dadd_rn(tp, v);
    if (lens) { const double l = (double)lens[t]; wl = __dadd_rn(wl, __dmul_rn(v, l)); sl = __dadd_rn(sl, l); }
    if (eff) { const double l = eff[t]; we = __dadd_rn(we, __dmul_rn(v, l)); se = __dadd_rn(se, l); }
  }
  const double n = (double)(p1 - p0);
  num_reads[g] = nr; tpm[g] = tp;
  length[g] = !lens || p1 == p0 ? 0.0 : tp > 0.0 ? wl / tp : sl / n;
  if (eff_length) eff_length[g] = !eff || p1 == p0 ? 0.0 : tp > 0.0 ? we / tp : se / n;
}
// one lane per (replicate, gene) of the n_boot x n_tx result
__global__ void __launch_bounds__(256) k_qg_boot(const double *res, int64_t n_tx, int64_t n_boot, const uint64_t *g_toff, const uint32_t *g_tx,
                                                 int64_t n_genes, double *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_boot * n_genes) return;
  const int64_t b = i / n_genes, g = i - b * n_genes;
  const double *row = res + b * n_tx;
  double s = 0.0;
  for (uint64_t p = g_toff[g]; p < g_toff[g + 1]; p++) s = __dadd_rn(s, row[g_tx[p]]);
  out[i] = s;
}

void launch_qg_key(hipStream_t st, const uint64_t *label_off, const uint32_t *labels, const uint32_t *tx_gene, int64_t n_cls, int64_t n_lab,
                   uint64_t *key, uint32_t *idx) {
  if (n_lab > 0) hipLaunchKernelGGL(k_qg_key, dim3(blocks256(n_lab)), dim3(256), 0, st, label_off, labels, tx_gene, n_cls, n_lab, key, idx);
}
void launch_qg_flag(hipStream_t st, const uint64_t *key, int64_t n, uint64_t *flag) {
  if (n > 0) hipLaunchKernelGGL(k_qg_flag, dim3(blocks256(n)), dim3(256), 0, st, key, n, flag);
}
void launch_qg_arena(hipStream_t st, const uint64_t *key, const uint64_t *pos, const uint64_t *label_off, int64_t n_lab, int64_t n_cls,
                     uint32_t *glab, uint64_t *goff, uint32_t *gk) {
  const int64_t m = n_lab > n_cls + 1 ? n_lab : n_cls + 1;
  hipLaunchKernelGGL(k_qg_arena, dim3(blocks256(m)), dim3(256), 0, st, key, pos, label_off, n_lab, n_cls, glab, goff, gk);
}
void launch_qg_hash(hipStream_t st, const uint32_t *glab, const uint64_t *goff, int64_t n_cls, const uint32_t *big, uint32_t n_big, uint64_t mask,
                    uint64_t *key, uint32_t *idx) {
  if (n_cls > 0) hipLaunchKernelGGL(k_qg_hash<false>, dim3(blocks256(n_cls)), dim3(256), 0, st, glab, goff, n_cls, big, n_big, mask, key, idx);
  if (n_big) hipLaunchKernelGGL(k_qg_hash<true>, dim3((n_big + 3) / 4), dim3(256), 0, st, glab, goff, n_cls, big, n_big, mask, key, idx);
}
void launch_qg_member_cnt(hipStream_t st, const uint32_t *idx, const uint64_t *cnt, int64_t n, uint64_t *w) {
  if (n > 0) hipLaunchKernelGGL(k_qg_member_cnt, dim3(blocks256(n)), dim3(256), 0, st, idx, cnt, n, w);
}
void launch_qg_labels(hipStream_t st, const uint64_t *label_off, const uint32_t *rep, const uint64_t *goff, const uint32_t *glab, const uint64_t *cnt,
                      int64_t n_cls, int64_t n_lab, uint32_t *labels, uint64_t *uniq, uint64_t *ambig) {
  if (n_lab > 0) hipLaunchKernelGGL(k_qg_labels, dim3(blocks256(n_lab)), dim3(256), 0, st, label_off, rep, goff, glab, cnt, n_cls, n_lab, labels,
                                    (unsigned long long *)uniq, (unsigned long long *)ambig);
}
void launch_qg_sums(hipStream_t st, const uint64_t *g_toff, const uint32_t *g_tx, int64_t n_genes, const double *theta, const double *tpm_t,
                    const int64_t *lens, const double *eff, double *num_reads, double *tpm, double *length, double *eff_length) {
  if (n_genes > 0) hipLaunchKernelGGL(k_qg_sums, dim3(blocks256(n_genes)), dim3(256), 0, st, g_toff, g_tx, n_genes, theta, tpm_t, lens, eff, num_reads,
                                      tpm, length, eff_length);
}
void launch_qg_boot(hipStream_t st, const double *res, int64_t n_tx, int64_t n_boot, const uint64_t *g_toff, const uint32_t *g_tx, int64_t n_genes,
                    double *out) {
  if (n_boot * n_genes > 0) hipLaunchKernelGGL(k_qg_boot, dim3(blocks256(n_boot * n_genes)), dim3(256), 0, st, res, n_tx, n_boot, g_toff, g_tx, n_genes, out);
}

void launch_q_boot_sample(hipStream_t st, const uint64_t *cum, int64_t n_cls, uint64_t n, uint64_t seed, uint32_t b_first, uint32_t n_rep,
                          uint32_t *out, int64_t stride_c, int64_t stride_b) {
  if (n == 0 || n_cls <= 0 || n_rep == 0) return;
  hipLaunchKernelGGL(k_q_boot_sample, dim3(blocks256((int64_t)n), n_rep), dim3(256), 0, st, cum, n_cls, n, (uint32_t)seed, (uint32_t)(seed >> 32),
                     b_first, out, stride_c, stride_b);
}
void launch_q_boot_store(hipStream_t st, const double *theta, int64_t n_tx, int lw, int n_rep, double *out) {
  if (n_tx > 0 && n_rep > 0) hipLaunchKernelGGL(k_q_boot_store, dim3(blocks256(n_tx << lw)), dim3(256), 0, st, theta, n_tx, lw, n_rep, out);
}
void launch_q_boot_summary(hipStream_t st, const double *res, int64_t n_tx, int32_t n_boot, double *mean, double *var) {
  if (n_tx > 0) hipLaunchKernelGGL(k_q_boot_summary, dim3(blocks256(n_tx)), dim3(256), 0, st, res, n_tx, n_boot, mean, var);
}

void launch_q_span(hipStream_t st, const uint64_t *row_off, const uint32_t *group_off, int64_t n_groups, uint64_t *span) {
  hipLaunchKernelGGL(k_q_span, dim3(1), dim3(1), 0, st, row_off, group_off, n_groups, span);
}
void launch_q_names(hipStream_t st, const QAddArgs &A) {
  if (A.names.n_groups <= 0) return;
  hipLaunchKernelGGL(k_q_names, dim3(blocks256(A.names.n_groups)), dim3(256), 0, st, A);
  const int64_t most = (A.names.n_groups + 3) / 4;   // (the list is no longer than the names)
  hipLaunchKernelGGL(k_q_names_big, dim3((unsigned)(most < (int64_t)Q_BIG_GRID ? most : (int64_t)Q_BIG_GRID)), dim3(256), 0, st, A);
}
void launch_q_frag(hipStream_t st, const QAddArgs &A) {
  if (A.names.n_groups <= 0) return;
  const bool lds = A.fld_max < Q_FLD_LDS_BINS;
  const size_t sh = lds ? (size_t)(A.fld_max + 1u) * 4 : 0;
  const int64_t most = (A.names.n_groups + 3) / 4;
  const dim3 big_grid((unsigned)(most < (int64_t)Q_BIG_GRID ? most : (int64_t)Q_BIG_GRID));
  if (lds) {
    hipLaunchKernelGGL(k_q_frag<true>, dim3(blocks256(A.names.n_groups)), dim3(256), sh, st, A);
    hipLaunchKernelGGL(k_q_frag_big<true>, big_grid, dim3(256), sh, st, A);
  } else {
    hipLaunchKernelGGL(k_q_frag<false>, dim3(blocks256(A.names.n_groups)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_q_frag_big<false>, big_grid, dim3(256), 0, st, A);
  }
}
void launch_q_fld_commit(hipStream_t st, unsigned long long *stage, unsigned long long *total, uint32_t n_words) {
  hipLaunchKernelGGL(k_q_fld_commit, dim3(blocks256(n_words)), dim3(256), 0, st, stage, total, n_words);
}
void launch_q_fld_prefix(hipStream_t st, const unsigned long long *hist, uint32_t n_bins, uint64_t *cs) {
  hipLaunchKernelGGL(k_q_fld_prefix, dim3(1), dim3(256), 0, st, hist, n_bins, cs);
}
void launch_q_efflen(hipStream_t st, const int64_t *lens, int64_t n_tx, const uint64_t *cs, uint32_t n_bins, double *eff, double *w) {
  if (n_tx <= 0) return;
  if (n_bins <= Q_EFF_LDS_BINS) hipLaunchKernelGGL(k_q_efflen<true>, dim3(blocks256(n_tx)), dim3(256), (size_t)n_bins * 16, st, lens, n_tx, cs, n_bins, eff, w);
  else hipLaunchKernelGGL(k_q_efflen<false>, dim3(blocks256(n_tx)), dim3(256), 0, st, lens, n_tx, cs, n_bins, eff, w);
}
void launch_q_drop(hipStream_t st, const uint8_t *flags, int64_t n, uint32_t *nk, unsigned long long *n_dropped) {
  if (n > 0) hipLaunchKernelGGL(k_q_drop, dim3(blocks256(n)), dim3(256), 0, st, flags, n, nk, n_dropped);
}
void launch_q_flag(hipStream_t st, const uint32_t *nk, int64_t n, uint64_t *flag) {
  if (n > 0) hipLaunchKernelGGL(k_q_flag, dim3(blocks256(n)), dim3(256), 0, st, nk, n, flag);
}
void launch_q_compact(hipStream_t st, const uint32_t *nk, const uint64_t *hash, const uint64_t *pos, int64_t n, uint64_t mask,
                      uint64_t *key, uint32_t *idx) {
  if (n > 0) hipLaunchKernelGGL(k_q_compact, dim3(blocks256(n)), dim3(256), 0, st, nk, hash, pos, n, mask, key, idx);
}
void launch_q_bits(hipStream_t st, const uint64_t *key, int64_t n, uint64_t *part, uint64_t *bits) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_q_bits_part, dim3(blocks256(n)), dim3(256), 0, st, key, n, part);
  launch_col_bits(st, part, (int64_t)blocks256(n), bits);
}
void launch_q_heads(hipStream_t st, const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, const uint64_t *key,
                    const uint32_t *idx, int64_t n, uint64_t *head, unsigned long long *n_coll, uint32_t *mark) {
  if (n > 0) hipLaunchKernelGGL(k_q_heads, dim3(blocks256(n)), dim3(256), 0, st, lab, noff, nk, key, idx, n, head, n_coll, mark);
}
void launch_q_resolve(hipStream_t st, const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, const uint64_t *key,
                      const uint32_t *idx, int64_t n, const uint32_t *mark, uint64_t *key_out, uint32_t *idx_out) {
  if (n > 0) hipLaunchKernelGGL(k_q_resolve, dim3(blocks256(n)), dim3(256), 0, st, lab, noff, nk, key, idx, n, mark, key_out, idx_out);
}
void launch_q_class_key(hipStream_t st, const uint64_t *gbeg, const uint32_t *idx, const uint64_t *item_first, int64_t n_cls, uint64_t *key,
                        uint32_t *val) {
  if (n_cls > 0) hipLaunchKernelGGL(k_q_class_key, dim3(blocks256(n_cls)), dim3(256), 0, st, gbeg, idx, item_first, n_cls, key, val);
}
void launch_q_class_fill(hipStream_t st, const uint64_t *key, const uint32_t *val, const uint64_t *gbeg, const uint32_t *idx, const uint64_t *pre,
                         const uint32_t *nk, int64_t n_cls, uint64_t *first, uint64_t *cnt, uint64_t *label_off, uint32_t *rep) {
  if (n_cls > 0) hipLaunchKernelGGL(k_q_class_fill, dim3(blocks256(n_cls)), dim3(256), 0, st, key, val, gbeg, idx, pre, nk, n_cls, first, cnt, label_off, rep);
}
void launch_q_name_cls(hipStream_t st, const uint64_t *head, const uint32_t *idx, int64_t n, const uint32_t *val, int64_t n_cls, uint32_t *inv,
                       uint32_t *name_cls) {
  if (n_cls <= 0 || n <= 0) return;
  hipLaunchKernelGGL(k_q_class_inv, dim3(blocks256(n_cls)), dim3(256), 0, st, val, n_cls, inv);
  hipLaunchKernelGGL(k_q_name_cls, dim3(blocks256(n)), dim3(256), 0, st, head, idx, n, (const uint32_t *)inv, n_cls, name_cls);
}
void launch_q_post(hipStream_t st, const uint64_t *label_off, const uint32_t *labels, int64_t n_cls, const double *theta, const double *w,
                   double *post) {
  if (n_cls > 0) hipLaunchKernelGGL(k_q_post, dim3(blocks256(n_cls)), dim3(256), 0, st, label_off, labels, n_cls, theta, w, post);
}
void launch_q_labels(hipStream_t st, const uint64_t *label_off, const uint64_t *first, const uint64_t *noff, const uint32_t *lab,
                     int64_t n_cls, int64_t n_lab, const int64_t *lens, uint32_t *labels, uint32_t *ecls, uint64_t *tkey,
                     uint32_t *tidx, uint32_t *bad) {
  if (n_lab > 0) hipLaunchKernelGGL(k_q_labels, dim3(blocks256(n_lab)), dim3(256), 0, st, label_off, first, noff, lab, n_cls, n_lab, lens, labels, ecls, tkey, tidx, bad);
}
void launch_q_transpose(hipStream_t st, const uint64_t *tkey, const uint32_t *tidx, const uint32_t *ecls, int64_t n_lab,
                        int64_t n_tx, uint32_t *t_cls, uint64_t *t_off) {
  const int64_t m = n_lab > n_tx + 1 ? n_lab : n_tx + 1;
  hipLaunchKernelGGL(k_q_transpose, dim3(blocks256(m)), dim3(256), 0, st, tkey, tidx, ecls, n_lab, n_tx, t_cls, t_off);
}
void launch_q_bin(hipStream_t st, const uint64_t *off, int64_t n, uint32_t *list, uint32_t *n_list) {
  if (n > 0) hipLaunchKernelGGL(k_q_bin, dim3(blocks256(n)), dim3(256), 0, st, off, n, list, n_list);
}
void launch_q_counts(hipStream_t st, const uint32_t *t_cls, const uint64_t *t_off, const uint64_t *label_off, const uint64_t *cnt,
                     int64_t n_tx, const uint32_t *big, uint32_t n_big, uint64_t *uniq, uint64_t *ambig) {
  if (n_tx > 0) hipLaunchKernelGGL(k_q_counts<false>, dim3(blocks256(n_tx)), dim3(256), 0, st, t_cls, t_off, label_off, cnt, n_tx, big, n_big, uniq, ambig);
  if (n_big) hipLaunchKernelGGL(k_q_counts<true>, dim3((n_big + 3) / 4), dim3(256), 0, st, t_cls, t_off, label_off, cnt, n_tx, big, n_big, uniq, ambig);
}
void launch_q_em_init(hipStream_t st, const double *w, int64_t n_tx, int lw, double *theta, double *x) {
  if (n_tx > 0) hipLaunchKernelGGL(k_q_em_init, dim3(blocks256(n_tx << lw)), dim3(256), 0, st, w, n_tx, lw, theta, x);
}
void launch_q_em_classes(hipStream_t st, const QEmArgs &E, const double *x) {
  const bool point = !E.boot_cnt;
  const auto lanes = point ? k_q_em_classes<false, true> : k_q_em_classes<false, false>, waves = point ? k_q_em_classes<true, true> : k_q_em_classes<true, false>;
  if (E.n_cls > 0) hipLaunchKernelGGL(lanes, dim3(blocks256(E.n_cls << E.lw)), dim3(256), 0, st, E, x);
  if (E.n_big_cls) hipLaunchKernelGGL(waves, dim3((E.n_big_cls + 3) / 4), dim3(256), 0, st, E, x);
}
void launch_q_em_tx(hipStream_t st, const QEmArgs &E, const double *theta, const double *x, double *theta_out, double *x_out,
                    unsigned long long *rel) {
  const bool point = !E.boot_cnt;
  const auto lanes = point ? k_q_em_tx<false, true> : k_q_em_tx<false, false>, waves = point ? k_q_em_tx<true, true> : k_q_em_tx<true, false>;
  if (E.n_tx > 0) hipLaunchKernelGGL(lanes, dim3(blocks256(E.n_tx << E.lw)), dim3(256), 0, st, E, theta, x, theta_out, x_out, rel);
  if (E.n_big_tx) hipLaunchKernelGGL(waves, dim3((E.n_big_tx + 3) / 4), dim3(256), 0, st, E, theta, x, theta_out, x_out, rel);
}

}  // namespace br
