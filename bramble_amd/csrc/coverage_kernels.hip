// Kernels of br_coverage (coverage.cpp holds the pipeline's description; the definitions are in bramble_amd.h).  Every kernel is
// here once: the add is a template on what it does with an interval (COV_ADD_*), the depth pipeline on the depth word W (uint32_t:
// weight 0, modulo 2^32; uint64_t: the weighted modes, modulo 2^64, one unit 2^32).
//
//   add      k_cov_add<MODE>: a lane per row.  It walks the row's rewritten CIGAR in 64-bit arithmetic, merges covering ops that
//            touch (10M 2I 5M is one interval), clamps every interval to its transcript and hands it to the mode's CovSink: two
//            events in diff, + 1 / - 1 at its first base and behind its last (weight 0) or + q / - q (weight nh), or an entry counted
//            and then kept in an arena (weight em, which runs the add twice: a wave places its rows' entries by one atomic).  A pooled
//            CIGAR of more than COV_SMALL_OPS ops is walked by the wave, 64 ops a step, the positions by a wave scan: there every
//            covering op is an interval of its own.  records[t] gets one atomic per distinct transcript of the wave, the counters
//            one per wave
//   apply    k_cov_apply (weight em) turns the kept entries into events once the quantifier's posteriors exist
//   depth    every interval lies inside its transcript, so the plain inclusive scan of diff is the depth and returns to 0 at every
//            transcript's end: tile sums, their scan (launch_scan), and the tiles scanned again with their offsets
//   summary  a wave per transcript of up to COV_WAVE_LEN bases, a block per longer one
//   runs     run heads counted per tile, the counts scanned, and the runs written: the lane of a run's first base stores
//            (transcript, start), the lane of its last base (end, depth) -- the k-th last base belongs to the k-th head, and the
//            heads in front of a base say which one that is
// Everything is integer: the atomics change no result, whatever order they arrive in.
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "cigar_inl.h"
#include "coverage_kernels.h"
#include "scan_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
typedef uint32_t cv_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t cv_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void keep_entry(uint4 *arena, uint64_t cap, uint64_t slot, uint64_t w0, uint32_t len, uint32_t name) {
  if (slot < cap) arena[slot] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), len, name);
}
// Where a row's clamped, non-empty intervals [at, at + len) of the B bases go.  Only the mode's own fields are ever read
template <int MODE>
struct CovSink {
  void *diff; uint64_t q;                               // COV_ADD_UNIT (32-bit words), COV_ADD_NH (64-bit words and the row's q)
  uint4 *arena; uint64_t cap, slot; uint32_t name;      // COV_ADD_KEEP: slot = the row's first
  uint32_t n;                                           // COV_ADD_COUNT, COV_ADD_KEEP: entries of the row so far
  __device__ __forceinline__ void put(uint64_t at, uint64_t len) {
    if constexpr (MODE == COV_ADD_UNIT) { uint32_t *d = (uint32_t *)diff + at; atomicAdd(d, 1u); atomicAdd(d + len, 0xffffffffu); }
    if constexpr (MODE == COV_ADD_NH) { unsigned long long *d = (unsigned long long *)diff + at; atomicAdd(d, (unsigned long long)q); atomicAdd(d + len, (unsigned long long)(0ull - q)); }
    if constexpr (MODE == COV_ADD_KEEP) keep_entry(arena, cap, slot + n, at | (n ? 0ull : COV_KEEP_FIRST), (uint32_t)len, name);
    n++;
  }
  // the end of a counted row's walk: one without an entry leaves the entry of length 0.  Returns the row's entries
  __device__ __forceinline__ uint32_t end(uint32_t tid) {
    if (MODE == COV_ADD_KEEP && n == 0u) keep_entry(arena, cap, slot, (uint64_t)tid, 0u, name);
    return n ? n : 1u;
  }
};
// [s, e) of a transcript of len bases <- its part inside [0, len); the rest is counted as clipped.  False when nothing is left
__device__ __forceinline__ bool clamp(uint64_t len, uint64_t &s, uint64_t &e, uint64_t &clipped) {
  const uint64_t cs = s < len ? s : len, ce = e < len ? e : len;
  clipped += (e - s) - (ce - cs);
  s = cs; e = ce;
  return ce > cs;
}
// the interval [s, e) of the transcript whose first base is base: what is left of it ends at most at base + len, the first base of
// the next transcript or the word behind the last
template <int MODE>
__device__ __forceinline__ void cover(CovSink<MODE> &k, uint64_t base, uint64_t len, uint64_t s, uint64_t e, uint64_t &clipped) {
  if (clamp(len, s, e, clipped)) k.put(base + s, e - s);
}
// a lane's walk: the position and the interval not yet written ([cs, ce), empty when they are equal)
struct Walk { uint64_t p, cs, ce; };
template <int MODE>
__device__ __forceinline__ void walk_op(CovSink<MODE> &k, uint64_t base, uint64_t len, Walk &w, uint32_t op, uint64_t &clipped) {
  const uint64_t n = op >> 4;
  if (cigar_covers(op)) {
    if (w.ce > w.cs && w.ce == w.p) w.ce += n;
    else { if (w.ce > w.cs) cover(k, base, len, w.cs, w.ce, clipped); w.cs = w.p; w.ce = w.p + n; }
    w.p += n;
  } else if (cigar_skips(op)) w.p += n;
}
// the add-order name of row r, from the add's offsets; false where they do not give one (offsets that descend)
__device__ __forceinline__ bool name_of(const CovAddWArgs &W, uint64_t r, uint32_t &name) {
  const NameWindow &N = W.names;
  const uint32_t a0 = N.group_off[0], a1 = N.group_off[N.n_groups];
  if (a1 <= a0) return false;
  const auto ro = [&](uint32_t a) { return N.row_off[(int64_t)a - N.ro_bias]; };
  uint32_t lo = a0, hi = a1 - 1u;   // the last alignment of [a0, a1) whose rows begin at or in front of r
  while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (ro(mid) <= r) lo = mid; else hi = mid - 1u; }
  if (!(ro(lo) <= r && r < ro(lo + 1u))) return false;
  int64_t glo = 0, ghi = N.n_groups - 1;   // the last name whose alignments begin at or in front of it
  while (glo < ghi) { const int64_t mid = (glo + ghi + 1) >> 1; if (N.group_off[mid] <= lo) glo = mid; else ghi = mid - 1; }
  if (!(N.group_off[glo] <= lo && lo < N.group_off[glo + 1])) return false;
  name = (uint32_t)(W.name_base + (uint64_t)glo);
  return true;
}
}  // namespace

template <int MODE>
__global__ void __launch_bounds__(256) k_cov_add(CovAddWArgs W) {
  constexpr bool NH = MODE == COV_ADD_NH, KEEP = MODE == COV_ADD_KEEP, NAMED = MODE == COV_ADD_COUNT || MODE == COV_ADD_KEEP;
  const CovAddArgs &A = W.A;
  const uint64_t r = A.r_first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t counted = 0, skipped = 0, tid = 0, wide_n = 0, n_ops = 0, entries = 0;
  bool bad_pool = false, bad_tid = false, bad_nh = false, bad_names = false, walks = false;
  uint64_t clipped = 0, base = 0, len = 0, pos = 0, cref = 0;
  CovSink<MODE> k{A.diff, 0ull, W.arena, W.arena_cap, 0ull, 0u, 0u};   // of the lane's row
  if (r < A.r_last) {
    // the rows are read once here: non-temporal, as the projection's other consumers take them
    const cv_u4 m = __builtin_nontemporal_load((const cv_u4 *)A.a + ((int64_t)r - A.bias));
    if (A.primary_only && !(m.z & BR_ROW_PRIMARY)) skipped = 1;
    else if ((int64_t)m.x >= A.n_tx) { skipped = 1; bad_tid = true; }   // nothing of it is looked up
    else if (NH && m.w == 0u) { skipped = 1; bad_nh = true; }   // no weight to give it
    else if (NAMED && !name_of(W, r, k.name)) { skipped = 1; bad_names = true; }
    else {
      n_ops = BR_ROW_NCIGAR(m.z);
      cref = __builtin_nontemporal_load(A.cigar + ((int64_t)r - A.bias));
      tid = m.x; pos = m.y;
      base = A.off[tid]; len = A.off[tid + 1] - base;
      if constexpr (NH) k.q = ((1ull << 32) + (uint64_t)(m.w >> 1)) / (uint64_t)m.w;
      if (n_ops > 2u && !pool_holds(A.n_pool_words, cref, n_ops)) bad_pool = true;
      else walks = true;
    }
  }
  if constexpr (KEEP) {   // the wave's rows, one after the other in the arena: the count pass left every row's entries
    const uint64_t mine = walks ? (uint64_t)W.row_entries[r - A.r_first] : 0ull;
    const uint64_t incl = wave_scan(mine);
    uint64_t first = 0;
    if (lane == 63 && incl) first = atomicAdd(A.counters + CV_KEPT, (unsigned long long)incl);
    k.slot = __shfl(first, 63) + incl - mine;
  }
  if (walks) {
    counted = 1;
    if (n_ops <= COV_SMALL_OPS) {
      Walk w{pos, 0, 0};
      if (n_ops <= 2u) {
        if (n_ops >= 1u) walk_op(k, base, len, w, (uint32_t)cref, clipped);
        if (n_ops == 2u) walk_op(k, base, len, w, (uint32_t)(cref >> 32), clipped);
      } else {
        for (uint32_t i = 0; i < n_ops; i++) walk_op(k, base, len, w, A.pool[cref + i], clipped);
      }
      if (w.ce > w.cs) cover(k, base, len, w.cs, w.ce, clipped);
      if constexpr (NAMED) entries = k.end(tid);
    } else wide_n = n_ops;
  }
  // the long CIGARs, one after the other: 64 ops a step, an op's position from the wave's scan of the reference bases in front of
  // it.  Every covering op of positive length is an interval of its own here; its place among the row's entries is the emitting
  // lanes in front of it
  wave_turns(wide_n != 0u, [&](int src) {
    const uint64_t off = __shfl(cref, src), w_base = __shfl(base, src), w_len = __shfl(len, src);
    const uint32_t n = (uint32_t)__shfl((int)wide_n, src);
    CovSink<MODE> wk = k;   // row src's
    if constexpr (NH) wk.q = __shfl(k.q, src);
    if constexpr (KEEP) wk.slot = __shfl(k.slot, src);
    if constexpr (NAMED) wk.name = (uint32_t)__shfl((int)k.name, src);
    uint64_t p = __shfl(pos, src);
    uint32_t done = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
      const uint32_t i = k0 + (uint32_t)lane;
      const uint32_t op = i < n ? A.pool[off + i] : 4u;   // (past the end: a soft clip of no bases)
      const uint64_t adv = cigar_ref_len(op), inc = wave_scan(adv);
      uint64_t s = p + inc - adv, e = p + inc;
      const bool emit = cigar_covers(op) && (op >> 4) && clamp(w_len, s, e, clipped);
      if constexpr (NAMED) {
        const uint64_t bal = __ballot(emit);
        wk.n = done + (uint32_t)__popcll((unsigned long long)(bal & ((1ull << lane) - 1ull)));
        done += (uint32_t)__popcll((unsigned long long)bal);
      }
      if (emit) wk.put(w_base + s, e - s);
      p += __shfl(inc, 63);
    }
    if constexpr (NAMED) { wk.n = done; if (lane == src) entries = wk.end(tid); }
  });
  const bool any_bad_pool = __ballot(bad_pool) != 0;
  if constexpr (MODE == COV_ADD_COUNT) {   // nothing is counted yet: the keep pass does that
    if (r < A.r_last) W.row_entries[r - A.r_first] = entries;
    const uint64_t sum = wave_sum((uint64_t)entries);
    const bool any_bad_names = __ballot(bad_names) != 0;
    if (lane == 0) {
      if (sum) atomicAdd(A.counters + CV_ADD_ENTRIES, (unsigned long long)sum);
      if (any_bad_pool) A.counters[CV_BAD_POOL] = 1;
      if (any_bad_names) A.counters[CV_BAD_NAMES] = 1;
    }
    return;
  }
  // records (and, weight nh, weight_sum): one atomic each per distinct transcript among the wave's counted rows
  uint64_t live = __ballot(counted != 0u);
  while (live) {
    const int src = __ffsll((unsigned long long)live) - 1;
    const uint32_t t = (uint32_t)__shfl((int)tid, src);
    const bool in = counted != 0u && tid == t;
    const uint64_t same = __ballot(in);
    uint64_t qs = 0;
    if constexpr (NH) qs = wave_sum(in ? k.q : 0ull);
    if (lane == src) {
      atomicAdd(A.records + t, (unsigned long long)__popcll((unsigned long long)same));
      if constexpr (NH) atomicAdd(W.weight_sum + t, (unsigned long long)qs);
    }
    live &= ~same;
  }
  counted = wave_sum(counted); skipped = wave_sum(skipped); clipped = wave_sum(clipped);
  const bool any_bad_tid = __ballot(bad_tid) != 0;
  if (lane == 0) {
    if (counted) atomicAdd(A.counters + CV_COUNTED, (unsigned long long)counted);
    if (skipped) atomicAdd(A.counters + CV_SKIPPED, (unsigned long long)skipped);
    if (clipped) atomicAdd(A.counters + CV_CLIPPED, (unsigned long long)clipped);
    if (any_bad_pool) A.counters[CV_BAD_POOL] = 1;
    if (any_bad_tid) A.counters[CV_BAD_TID] = 1;
  }
  if constexpr (NH) { if (__ballot(bad_nh) && lane == 0) A.counters[CV_BAD_NH] = 1; }
  if constexpr (NAMED) { if (__ballot(bad_names) && lane == 0) A.counters[CV_BAD_NAMES] = 1; }
}

namespace {
// the transcript that owns base i (i < off[n_tx]): the last t of [lo, hi] with off[t] <= i -- off[t + 1] > i then, so transcripts
// without bases own nothing
__device__ __forceinline__ int64_t tx_of(const uint64_t *off, int64_t lo, int64_t hi, uint64_t i) {
  while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (off[mid] <= i) lo = mid; else hi = mid - 1; }
  return lo;
}
}  // namespace

// a lane per kept entry: name -> class -> the transcript's entry among the class's labels -> q, and the row's two events.  Nothing
// read from a table becomes an address before it was compared with that table's size; what fails is counted, not applied
__global__ void __launch_bounds__(256) k_cov_apply(CovApplyArgs P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad_name = false, bad_class = false, bad_label = false, bad_entry = false;
  if (i < P.n) {
    const uint4 e = P.arena[i];
    const uint64_t w0 = (uint64_t)e.x | ((uint64_t)e.y << 32), at = w0 & ~COV_KEEP_FIRST, len = e.z;
    const bool first = (w0 & COV_KEEP_FIRST) != 0ull || len == 0ull;
    int64_t t = -1;
    if (len == 0ull) { if (at < (uint64_t)P.n_tx) t = (int64_t)at; else bad_entry = true; }
    else if (at >= P.n_bases || len > P.n_bases - at) bad_entry = true;
    else {
      t = tx_of(P.off, 0, P.n_tx - 1, at);
      if (at + len > P.off[t + 1]) { bad_entry = true; t = -1; }
    }
    if (t >= 0) {
      if ((uint64_t)e.w >= P.n_names) bad_name = true;
      else {
        const uint64_t cls = P.name_cls[e.w];
        if (cls >= P.n_cls) bad_class = true;   // (a name without rows among them)
        else {
          const uint64_t b = P.label_off[cls], z = P.label_off[cls + 1];
          if (b > z || z > P.n_lab) bad_class = true;
          else {
            uint64_t lo = b, hi = z;   // the first label of [b, z) that is >= t
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if ((int64_t)P.labels[mid] < t) lo = mid + 1; else hi = mid; }
            if (lo >= z || (int64_t)P.labels[lo] != t) bad_label = true;
            else {
              const double qd = rint(P.post[lo] * 4294967296.0);
              if (!(qd >= 0.0 && qd <= 4294967296.0)) bad_label = true;   // (no posterior at all)
              else {
                const unsigned long long q = (unsigned long long)qd;
                if (len) { atomicAdd(P.diff + at, q); atomicAdd(P.diff + at + len, 0ull - q); }
                if (first) atomicAdd(P.weight_sum + t, q);
              }
            }
          }
        }
      }
    }
  }
  const uint64_t bn = __ballot(bad_name), bc = __ballot(bad_class), bl = __ballot(bad_label), be = __ballot(bad_entry);
  if ((threadIdx.x & 63) == 0) {
    if (bn) atomicAdd(P.counters + CV_BAD_NAME, (unsigned long long)__popcll((unsigned long long)bn));
    if (bc) atomicAdd(P.counters + CV_BAD_CLASS, (unsigned long long)__popcll((unsigned long long)bc));
    if (bl) atomicAdd(P.counters + CV_BAD_LABEL, (unsigned long long)__popcll((unsigned long long)bl));
    if (be) atomicAdd(P.counters + CV_BAD_ENTRY, (unsigned long long)__popcll((unsigned long long)be));
  }
}

// ---- the depth pipeline, over words W ------------------------------------------------------------------------------------------------
namespace {
// four consecutive entries from d[i] on (i a multiple of 4) as 16-byte accesses, 0 for those at or past n
template <typename W>
struct Four { W v[4]; };
template <typename W>
__device__ __forceinline__ Four<W> load4(const W *d, int64_t i, int64_t n) {
  constexpr int V = 16 / sizeof(W);   // words per 16 bytes
  typedef W vec_t __attribute__((ext_vector_type(V)));
  Four<W> r = {{0, 0, 0, 0}};
  if (i + 4 <= n) {
#pragma unroll
    for (int k = 0; k < 4; k += V) {
      const vec_t a = *(const vec_t *)(d + i + k);
#pragma unroll
      for (int j = 0; j < V; j++) r.v[k + j] = a[j];
    }
    return r;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) if (i + k < n) r.v[k] = d[i + k];
  return r;
}
template <typename W>
__device__ __forceinline__ void store4(W *d, int64_t i, int64_t n, const Four<W> &r) {
  constexpr int V = 16 / sizeof(W);
  typedef W vec_t __attribute__((ext_vector_type(V)));
  if (i + 4 <= n) {
#pragma unroll
    for (int k = 0; k < 4; k += V) {
      vec_t a;
#pragma unroll
      for (int j = 0; j < V; j++) a[j] = r.v[k + j];
      *(vec_t *)(d + i + k) = a;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) if (i + k < n) d[i + k] = r.v[k];
}
// the first entry of lane `tid` in chunk j (of 1024 entries) of the tile that starts at t0
__device__ __forceinline__ int64_t chunk_at(int64_t t0, int j) { return t0 + (int64_t)j * 1024 + (int64_t)threadIdx.x * 4; }
}  // namespace

template <typename W>
__global__ void __launch_bounds__(256) k_cov_tile_sum(const W *d, int64_t n, uint64_t *tile_sum) {
  __shared__ W sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  W s = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) { const Four<W> v = load4(d, chunk_at(t0, j), n); s += v.v[0] + v.v[1] + v.v[2] + v.v[3]; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = (uint64_t)(W)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// tile_pre: the exclusive scan of the tile sums (64-bit sums of W words: their low words are the sums modulo 2^32)
template <typename W>
__global__ void __launch_bounds__(256) k_cov_tile_apply(W *d, int64_t n, const uint64_t *tile_pre) {
  __shared__ W sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  W carry = (W)tile_pre[blockIdx.x];
  for (int j = 0; j < 4; j++) {
    const int64_t i = chunk_at(t0, j);
    Four<W> v = load4(d, i, n);
    v.v[1] += v.v[0]; v.v[2] += v.v[1]; v.v[3] += v.v[2];
    W total;
    const W add = carry + block_excl_scan_256(v.v[3], sh, total);   // (the lanes' sums in front of this one's four)
    v.v[0] += add; v.v[1] += add; v.v[2] += add; v.v[3] += add;
    store4(d, i, n, v);
    carry += total;
  }
}

namespace {
// A transcript's summary so far.  The sum of 32-bit depths is one 64-bit sum (lo); 64-bit depths are summed as their high and their
// low words.  N counts the non-zero entries: 32 bits are enough for a lane of the wave kernel
template <typename W, typename N>
struct CovSum {
  uint64_t hi, lo; N nz; W mx;
  __device__ __forceinline__ void add(W v) {
    if constexpr (sizeof(W) == 8) { hi += v >> 32; lo += v & 0xffffffffull; } else lo += v;
    nz += v != 0; mx = v > mx ? v : mx;
  }
  __device__ __forceinline__ void merge(const CovSum &o) { hi += o.hi; lo += o.lo; nz += o.nz; mx = o.mx > mx ? o.mx : mx; }
  __device__ __forceinline__ void wave() {
    if constexpr (sizeof(W) == 8) hi = wave_sum(hi);
    lo = wave_sum(lo); nz = wave_sum(nz); mx = wave_max(mx);
  }
  __device__ __forceinline__ void store(int64_t t, uint64_t *aligned, uint64_t *aligned_lo, uint64_t *covered, W *max_depth) const {
    if constexpr (sizeof(W) == 8) { aligned[t] = hi; aligned_lo[t] = lo; } else aligned[t] = lo;
    covered[t] = nz; max_depth[t] = mx;
  }
};
}  // namespace

template <typename W>
__global__ void __launch_bounds__(256) k_cov_summary_wave(const W *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned, uint64_t *aligned_lo,
                                                          uint64_t *covered, W *max_depth) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tx) return;
  const uint64_t b = off[t], e = off[t + 1];
  if (e - b > (uint64_t)COV_WAVE_LEN) return;   // (k_cov_summary_long's)
  CovSum<W, uint32_t> s = {0, 0, 0, 0};
  for (uint64_t i = b + (threadIdx.x & 63); i < e; i += 64) s.add(depth[i]);
  s.wave();
  if ((threadIdx.x & 63) == 0) s.store(t, aligned, aligned_lo, covered, max_depth);
}

template <typename W>
__global__ void __launch_bounds__(256) k_cov_summary_long(const W *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned, uint64_t *aligned_lo,
                                                          uint64_t *covered, W *max_depth) {
  __shared__ CovSum<W, uint64_t> sh[4];
  for (int64_t t = blockIdx.x; t < n_tx; t += gridDim.x) {   // (everything that branches here is the same in the whole block)
    const uint64_t b = off[t], e = off[t + 1];
    if (e - b <= (uint64_t)COV_WAVE_LEN) continue;
    CovSum<W, uint64_t> s = {0, 0, 0, 0};
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) s.add(depth[i]);
    s.wave();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < 4; k++) s.merge(sh[k]);
      s.store(t, aligned, aligned_lo, covered, max_depth);
    }
    __syncthreads();
  }
}

namespace {
// the transcripts of a tile's first and last base, found once a block: the lanes search between them
__device__ __forceinline__ void tile_span(const uint64_t *off, int64_t n_tx, int64_t t0, int64_t n, int64_t *sh_t) {
  if (threadIdx.x == 0) {
    const int64_t last = (t0 + COV_TILE < n ? t0 + COV_TILE : n) - 1;
    sh_t[0] = tx_of(off, 0, n_tx - 1, (uint64_t)t0);
    sh_t[1] = tx_of(off, sh_t[0], n_tx - 1, (uint64_t)last);
  }
  __syncthreads();
}
// a lane's four bases from i0 on (i0 < n): bit k of heads / tails = base i0 + k starts / ends a run; tx[k] and sb[k] = its
// transcript and that transcript's first base
template <typename W>
struct Quad { W d[4]; uint32_t heads, tails; uint32_t tx[4]; uint64_t sb[4]; };
template <typename W>
__device__ __forceinline__ Quad<W> quad_at(const W *depth, int64_t n, const uint64_t *off, const int64_t *sh_t, int64_t i0) {
  Quad<W> q;
  const Four<W> v = load4(depth, i0, n);
  q.d[0] = v.v[0]; q.d[1] = v.v[1]; q.d[2] = v.v[2]; q.d[3] = v.v[3];
  const W prev = i0 > 0 ? depth[i0 - 1] : 0, next = i0 + 4 < n ? depth[i0 + 4] : 0;
  q.heads = q.tails = 0;
  int64_t t = tx_of(off, sh_t[0], sh_t[1], (uint64_t)i0);
  uint64_t sb = off[t], nb = off[t + 1];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint64_t i = (uint64_t)i0 + (uint64_t)k;
    q.tx[k] = (uint32_t)t; q.sb[k] = sb;
    if ((int64_t)i >= n) continue;
    if (i >= nb) { do { t++; nb = off[t + 1]; } while (i >= nb); sb = off[t]; }   // (i < n = off[n_tx]: it ends)
    q.tx[k] = (uint32_t)t; q.sb[k] = sb;
    const W cur = q.d[k], before = k ? q.d[k - 1] : prev, behind = k < 3 ? q.d[k + 1] : next;
    if (cur != 0 && (i == sb || cur != before)) q.heads |= 1u << k;
    if (cur != 0 && (i + 1 == nb || cur != behind)) q.tails |= 1u << k;
  }
  return q;
}
}  // namespace

template <typename W>
__global__ void __launch_bounds__(256) k_cov_count(const W *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt) {
  __shared__ int64_t sh_t[2];
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  tile_span(off, n_tx, t0, n, sh_t);
  uint32_t cnt = 0;
  for (int j = 0; j < 4; j++) {
    const int64_t i0 = chunk_at(t0, j);
    if (i0 < n) cnt += (uint32_t)__popc(quad_at(depth, n, off, sh_t, i0).heads);
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint64_t)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// the head's lane stores (transcript, start), the lane of the run's last base (end, depth): a 32-bit depth in the run's fourth word,
// a 64-bit one in run_depth and 0 in that word
template <typename W>
__global__ void __launch_bounds__(256) k_cov_runs(const W *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *run4,
                                                  uint64_t *run_depth) {
  __shared__ int64_t sh_t[2];
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  tile_span(off, n_tx, t0, n, sh_t);
  uint64_t carry = tile_pre[blockIdx.x];   // heads in front of the chunk
  cv_u2 *out = (cv_u2 *)run4;
  for (int j = 0; j < 4; j++) {
    const int64_t i0 = chunk_at(t0, j);
    Quad<W> q;
    q.heads = q.tails = 0;
    if (i0 < n) q = quad_at(depth, n, off, sh_t, i0);
    uint32_t total;
    uint64_t h = carry + block_excl_scan_256((uint32_t)__popc(q.heads), sh, total);   // heads in front of base i0
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool head = (q.heads >> k) & 1u, tail = (q.tails >> k) & 1u;
      const uint64_t i = (uint64_t)i0 + (uint64_t)k;
      if (head) { const cv_u2 w = {q.tx[k], (uint32_t)(i - q.sb[k])}; out[2 * h] = w; }
      if (tail) {   // a last base that is no head ends the run of the head in front of it
        const uint64_t run = head ? h : h - 1;
        const cv_u2 w = {(uint32_t)(i + 1 - q.sb[k]), sizeof(W) == 4 ? (uint32_t)q.d[k] : 0u};
        out[2 * run + 1] = w;
        if constexpr (sizeof(W) == 8) run_depth[run] = q.d[k];
      }
      h += head ? 1u : 0u;
    }
    carry += total;
  }
}

namespace {
unsigned cov_tiles(int64_t n) { return (unsigned)((n + COV_TILE - 1) / COV_TILE); }
}  // namespace

void launch_cov_add(hipStream_t st, const CovAddWArgs &W, int mode) {
  const uint64_t n = W.A.r_last - W.A.r_first;
  if (!n) return;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (mode == COV_ADD_UNIT) hipLaunchKernelGGL(k_cov_add<COV_ADD_UNIT>, grid, dim3(256), 0, st, W);
  else if (mode == COV_ADD_NH) hipLaunchKernelGGL(k_cov_add<COV_ADD_NH>, grid, dim3(256), 0, st, W);
  else if (mode == COV_ADD_COUNT) hipLaunchKernelGGL(k_cov_add<COV_ADD_COUNT>, grid, dim3(256), 0, st, W);
  else hipLaunchKernelGGL(k_cov_add<COV_ADD_KEEP>, grid, dim3(256), 0, st, W);
}
void launch_cov_apply(hipStream_t st, const CovApplyArgs &P) {
  if (P.n) hipLaunchKernelGGL(k_cov_apply, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, st, P);
}
template <typename W>
void launch_cov_scan(hipStream_t st, W *depth, int64_t n, uint64_t *tile_sum, uint64_t *scan_tmp) {
  if (n <= 0) return;
  const unsigned tiles = cov_tiles(n);
  hipLaunchKernelGGL(k_cov_tile_sum<W>, dim3(tiles), dim3(256), 0, st, (const W *)depth, n, tile_sum);
  launch_scan(st, tile_sum, (int64_t)tiles, scan_tmp);
  hipLaunchKernelGGL(k_cov_tile_apply<W>, dim3(tiles), dim3(256), 0, st, depth, n, (const uint64_t *)tile_sum);
}
template <typename W>
void launch_cov_summary(hipStream_t st, const W *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned, uint64_t *aligned_lo,
                        uint64_t *covered, W *max_depth) {
  if (n_tx <= 0) return;
  hipLaunchKernelGGL(k_cov_summary_wave<W>, dim3((unsigned)((n_tx + 3) / 4)), dim3(256), 0, st, depth, off, n_tx, aligned, aligned_lo, covered, max_depth);
  const unsigned grid = (unsigned)(n_tx < (int64_t)COV_LONG_GRID ? n_tx : (int64_t)COV_LONG_GRID);
  hipLaunchKernelGGL(k_cov_summary_long<W>, dim3(grid), dim3(256), 0, st, depth, off, n_tx, aligned, aligned_lo, covered, max_depth);
}
template <typename W>
void launch_cov_count(hipStream_t st, const W *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt) {
  if (n > 0) hipLaunchKernelGGL(k_cov_count<W>, dim3(cov_tiles(n)), dim3(256), 0, st, depth, n, off, n_tx, tile_cnt);
}
template <typename W>
void launch_cov_runs(hipStream_t st, const W *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *run4,
                     uint64_t *run_depth) {
  if (n > 0) hipLaunchKernelGGL(k_cov_runs<W>, dim3(cov_tiles(n)), dim3(256), 0, st, depth, n, off, n_tx, tile_pre, run4, run_depth);
}
#define COV_PIPELINE(W)                                                                                                                              \
  template void launch_cov_scan<W>(hipStream_t, W *, int64_t, uint64_t *, uint64_t *);                                                              \
  template void launch_cov_summary<W>(hipStream_t, const W *, const uint64_t *, int64_t, uint64_t *, uint64_t *, uint64_t *, W *);                  \
  template void launch_cov_count<W>(hipStream_t, const W *, int64_t, const uint64_t *, int64_t, uint64_t *);                                        \
  template void launch_cov_runs<W>(hipStream_t, const W *, int64_t, const uint64_t *, int64_t, const uint64_t *, uint4 *, uint64_t *);
COV_PIPELINE(uint32_t)
COV_PIPELINE(uint64_t)
#undef COV_PIPELINE

}  // namespace br
