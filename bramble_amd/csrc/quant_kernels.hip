// Transcript quantification on the device (host side: quant.cpp, which holds the pipeline's description).
//
//   add      k_q_span, k_q_names (one lane per read name of up to Q_SMALL_ROWS rows) + k_q_names_big (one wave per larger name):
//            the name's distinct transcript ids in ascending order, by repeated selection of the smallest id above the last one,
//            into the label arena at the slot of the name's first row; a 64-bit hash of (labels, k)
//   classes  k_q_flag + scan + k_q_compact: the names with labels; k_q_bits; the collator's radix passes over (hash, name);
//            k_q_heads compares the label lists of neighbours; k_q_resolve orders a run of equal hashes that holds different
//            lists by (k, labels, name); k_q_class_key + radix passes: classes by their first name; k_q_class_fill, k_q_labels
//   table    radix passes over (transcript, label entry) + k_q_transpose: per transcript its classes, ascending; k_q_bin;
//            k_q_counts: unique / ambiguous names per transcript
//   EM       k_q_em_classes / k_q_em_tx, a lane per item of up to Q_WAVE_ITEMS entries and a wave per larger one
//
// No floating-point atomic anywhere: every sum is one lane's loop in ascending order, or a wave's -- lane l takes the entries
// l, l + 64, ... in ascending order, then the 64 partial sums meet in a fixed xor tree -- so its shape depends on the number of
// entries alone and a result has the same bits in every run.  The largest relative change goes through an integer atomicMax on
// the doubles' bit patterns (a maximum does not depend on the order it is taken in).
#include <hip/hip_runtime.h>

#include "collate_kernels.h"
#include "quant_kernels.h"

namespace br {

namespace {
constexpr uint64_t Q_NO_TID = 1ull << 40;   // above every transcript id
__device__ __forceinline__ uint64_t hash_step(uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; }   // FNV-1a over words
__device__ __forceinline__ uint64_t hash_end(uint64_t h, uint64_t k) {
  h = hash_step(h, k);
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;   // (murmur3 fmix64)
  return h;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
  for (int s = 32; s; s >>= 1) { const uint64_t o = __shfl_xor(v, s); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
  for (int s = 32; s; s >>= 1) { const uint64_t o = __shfl_xor(v, s); v = o > v ? o : v; }
  return v;
}
// the rows of name g of the add: false when they leave the add's rows
__device__ __forceinline__ bool name_rows(const QAddArgs &A, int64_t g, uint64_t &r0, uint64_t &r1) {
  r0 = A.row_off[(int64_t)A.group_off[g] - A.ro_bias];
  r1 = A.row_off[(int64_t)A.group_off[g + 1] - A.ro_bias];
  return r0 >= A.r_first && r1 <= A.r_last && r0 <= r1;
}
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
  if (g < A.n_groups) {
    uint64_t r0, r1;
    if (!name_rows(A, g, r0, r1)) { is_bad = true; A.noff[g] = A.lab_base; A.nk[g] = 0; A.hash[g] = 0; }
    else if (r1 - r0 > (uint64_t)Q_SMALL_ROWS) { is_big = true; A.noff[g] = A.lab_base + (r0 - A.r_first); }
    else {
      const uint64_t o = A.lab_base + (r0 - A.r_first);
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
  for (int s = 32; s; s >>= 1) { const uint32_t o = __shfl_xor(top, s); top = o > top ? o : top; }
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
    (void)name_rows(A, g, r0, r1);   // (k_q_names listed it: its rows are inside the add's)
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
  __shared__ uint64_t sh[2][4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t o = i < n ? key[i] : 0, a = i < n ? key[i] : ~0ull;
  for (int s = 32; s; s >>= 1) { o |= __shfl_xor(o, s); a &= __shfl_xor(a, s); }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = o; sh[1][threadIdx.x >> 6] = a; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { o |= sh[0][w]; a &= sh[1][w]; }
    part[2 * blockIdx.x] = o; part[2 * blockIdx.x + 1] = a;
  }
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

__global__ void __launch_bounds__(256) k_q_class_key(const uint64_t *gbeg, const uint32_t *idx, int64_t n_cls, uint64_t *key, uint32_t *val) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < n_cls) { key[c] = idx[gbeg[c]]; val[c] = (uint32_t)c; }   // (names inside a class ascend: its first item is its first name)
}
__global__ void __launch_bounds__(256) k_q_class_fill(const uint64_t *key, const uint32_t *val, const uint64_t *gbeg, const uint32_t *nk,
                                                      int64_t n_cls, uint64_t *first, uint64_t *cnt, uint64_t *label_off) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cls) return;
  const uint32_t s = val[c];
  first[c] = key[c]; cnt[c] = gbeg[s + 1] - gbeg[s]; label_off[c] = nk[key[c]];
}
__global__ void __launch_bounds__(256) k_q_labels(const uint64_t *label_off, const uint64_t *first, const uint64_t *noff, const uint32_t *lab,
                                                  int64_t n_cls, int64_t n_lab, const int64_t *lens, uint32_t *labels, uint32_t *ecls,
                                                  uint64_t *tkey, uint32_t *tidx, uint32_t *bad) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_lab) return;
  int64_t lo = 0, hi = n_cls;   // the class of entry e: the last c with label_off[c] <= e
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (label_off[mid] <= (uint64_t)e) lo = mid + 1; else hi = mid; }
  const int64_t c = lo - 1;
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

template <bool BIG>
__global__ void __launch_bounds__(256) k_q_em_classes(QEmArgs E, const double *x) {
  if (BIG) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= E.n_big_cls) return;
    const uint32_t c = E.big_cls[i];
    double d = 0.0;
    for (uint64_t e = E.label_off[c] + (uint64_t)lane; e < E.label_off[c + 1]; e += 64) d += x[E.labels[e]];
    d = wave_sum(d);
    if (lane == 0) E.q[c] = d > 0.0 ? (double)E.cnt[c] / d : 0.0;
  } else {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= E.n_cls) return;
    const uint64_t b = E.label_off[c], e1 = E.label_off[c + 1];
    if (e1 - b > (uint64_t)Q_WAVE_ITEMS) return;
    double d = 0.0;
    for (uint64_t e = b; e < e1; e++) d += x[E.labels[e]];
    E.q[c] = d > 0.0 ? (double)E.cnt[c] / d : 0.0;
  }
}

__device__ __forceinline__ uint64_t rel_bits(double now, double before) {
  if (!(now > 1e-8)) return 0;
  return (uint64_t)__double_as_longlong(fabs(now - before) / now);
}

template <bool BIG>
__global__ void __launch_bounds__(256) k_q_em_tx(QEmArgs E, const double *theta, const double *x, double *theta_out, double *x_out,
                                                 unsigned long long *rel) {
  uint64_t r = 0;
  if (BIG) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= E.n_big_tx) return;   // (wave-uniform)
    const uint32_t t = E.big_tx[i];
    double s = 0.0;
    for (uint64_t p = E.t_off[t] + (uint64_t)lane; p < E.t_off[t + 1]; p += 64) s += E.q[E.t_cls[p]];
    s = wave_sum(s);
    const double now = x[t] * s;
    if (lane == 0) { theta_out[t] = now; x_out[t] = now * E.w[t]; if (rel) r = rel_bits(now, theta[t]); }
  } else {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < E.n_tx && E.t_off[t + 1] - E.t_off[t] <= (uint64_t)Q_WAVE_ITEMS) {
      double s = 0.0;
      for (uint64_t p = E.t_off[t]; p < E.t_off[t + 1]; p++) s += E.q[E.t_cls[p]];
      const double now = x[t] * s;
      theta_out[t] = now; x_out[t] = now * E.w[t];
      if (rel) r = rel_bits(now, theta[t]);
    }
  }
  if (rel) {
    r = wave_max(r);
    if ((threadIdx.x & 63) == 0 && r) atomicMax(rel, (unsigned long long)r);
  }
}

void launch_q_span(hipStream_t st, const uint64_t *row_off, const uint32_t *group_off, int64_t n_groups, uint64_t *span) {
  hipLaunchKernelGGL(k_q_span, dim3(1), dim3(1), 0, st, row_off, group_off, n_groups, span);
}
void launch_q_names(hipStream_t st, const QAddArgs &A) {
  if (A.n_groups <= 0) return;
  hipLaunchKernelGGL(k_q_names, dim3(blocks256(A.n_groups)), dim3(256), 0, st, A);
  const int64_t most = (A.n_groups + 3) / 4;   // (the list is no longer than the names)
  hipLaunchKernelGGL(k_q_names_big, dim3((unsigned)(most < (int64_t)Q_BIG_GRID ? most : (int64_t)Q_BIG_GRID)), dim3(256), 0, st, A);
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
void launch_q_class_key(hipStream_t st, const uint64_t *gbeg, const uint32_t *idx, int64_t n_cls, uint64_t *key, uint32_t *val) {
  if (n_cls > 0) hipLaunchKernelGGL(k_q_class_key, dim3(blocks256(n_cls)), dim3(256), 0, st, gbeg, idx, n_cls, key, val);
}
void launch_q_class_fill(hipStream_t st, const uint64_t *key, const uint32_t *val, const uint64_t *gbeg, const uint32_t *nk,
                         int64_t n_cls, uint64_t *first, uint64_t *cnt, uint64_t *label_off) {
  if (n_cls > 0) hipLaunchKernelGGL(k_q_class_fill, dim3(blocks256(n_cls)), dim3(256), 0, st, key, val, gbeg, nk, n_cls, first, cnt, label_off);
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
void launch_q_em_classes(hipStream_t st, const QEmArgs &E, const double *x) {
  if (E.n_cls > 0) hipLaunchKernelGGL(k_q_em_classes<false>, dim3(blocks256(E.n_cls)), dim3(256), 0, st, E, x);
  if (E.n_big_cls) hipLaunchKernelGGL(k_q_em_classes<true>, dim3((E.n_big_cls + 3) / 4), dim3(256), 0, st, E, x);
}
void launch_q_em_tx(hipStream_t st, const QEmArgs &E, const double *theta, const double *x, double *theta_out, double *x_out,
                    unsigned long long *rel) {
  if (E.n_tx > 0) hipLaunchKernelGGL(k_q_em_tx<false>, dim3(blocks256(E.n_tx)), dim3(256), 0, st, E, theta, x, theta_out, x_out, rel);
  if (E.n_big_tx) hipLaunchKernelGGL(k_q_em_tx<true>, dim3((E.n_big_tx + 3) / 4), dim3(256), 0, st, E, theta, x, theta_out, x_out, rel);
}

}  // namespace br
