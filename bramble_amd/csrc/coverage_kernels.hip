// Kernels of br_coverage (coverage.cpp holds the pipeline's description; the definitions are in bramble_amd.h).
//
//   add      k_cov_add: a lane per row.  It walks the row's rewritten CIGAR in 64-bit arithmetic, merges covering ops that touch
//            (10M 2I 5M is one interval), clamps every interval to its transcript and leaves two events per interval in diff: + 1
//            at its first base, - 1 (mod 2^32) behind its last.  A pooled CIGAR of more than COV_SMALL_OPS ops is walked by the
//            wave, 64 ops a step, the positions by a wave scan.  records[t] gets one atomic per distinct transcript of the wave,
//            the counters one per wave
//   depth    every interval lies inside its transcript, so the plain inclusive scan of diff modulo 2^32 is the depth and returns
//            to 0 at every transcript's end: tile sums, their scan (launch_scan), and the tiles scanned again with their offsets
//   summary  a wave per transcript of up to COV_WAVE_LEN bases, a block per longer one
//   runs     run heads counted per tile, the counts scanned, and the runs written: the lane of a run's first base stores
//            (transcript, start), the lane of its last base (end, depth) -- the k-th last base belongs to the k-th head, and the
//            heads in front of a base say which one that is
// Everything is integer: the atomics change no result, whatever order they arrive in.
//
// The weighted modes (below the 32-bit kernels, which they leave as they were): k_cov_add_w, the same walk with another end for an
// interval -- + q / - q in 64-bit words (weight nh), or an entry counted and then kept in an arena (weight em) --; k_cov_apply,
// which turns the kept entries into events once the quantifier's posteriors exist; and the scan, summary, count and run kernels
// over uint64 words modulo 2^64.
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "coverage_kernels.h"
#include "scan_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
typedef uint32_t cv_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t cv_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bool op_covers(uint32_t w) { return (0x181u >> (w & 15u)) & 1u; }   // M = X (0, 7, 8)
__device__ __forceinline__ bool op_skips(uint32_t w) { return (0x00cu >> (w & 15u)) & 1u; }    // D N (2, 3)
// the interval [s, e) of a transcript of len bases whose first is diff[base]: the part inside [0, len) leaves its two events (the
// second at most at base + len, the first base of the next transcript or the word behind the last), the rest is counted as clipped
__device__ __forceinline__ void cover(uint32_t *diff, uint64_t base, uint64_t len, uint64_t s, uint64_t e, uint64_t &clipped) {
  const uint64_t cs = s < len ? s : len, ce = e < len ? e : len;
  clipped += (e - s) - (ce - cs);
  if (ce > cs) { atomicAdd(diff + base + cs, 1u); atomicAdd(diff + base + ce, 0xffffffffu); }
}
// a lane's walk: the position and the interval not yet written ([cs, ce), empty when they are equal)
struct Walk { uint64_t p, cs, ce; };
__device__ __forceinline__ void walk_op(uint32_t *diff, uint64_t base, uint64_t len, Walk &w, uint32_t op, uint64_t &clipped) {
  const uint64_t n = op >> 4;
  if (op_covers(op)) {
    if (w.ce > w.cs && w.ce == w.p) w.ce += n;
    else { if (w.ce > w.cs) cover(diff, base, len, w.cs, w.ce, clipped); w.cs = w.p; w.ce = w.p + n; }
    w.p += n;
  } else if (op_skips(op)) w.p += n;
}
__device__ __forceinline__ void walk_end(uint32_t *diff, uint64_t base, uint64_t len, const Walk &w, uint64_t &clipped) {
  if (w.ce > w.cs) cover(diff, base, len, w.cs, w.ce, clipped);
}
__device__ __forceinline__ bool in_pool(const CovAddArgs &A, uint64_t off, uint32_t n) { return off <= A.n_pool_words && (uint64_t)n <= A.n_pool_words - off; }
}  // namespace

__global__ void __launch_bounds__(256) k_cov_add(CovAddArgs A) {
  const uint64_t r = A.r_first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t counted = 0, skipped = 0, tid = 0, wide_n = 0;
  bool bad_pool = false, bad_tid = false;
  uint64_t clipped = 0, base = 0, len = 0, wide_off = 0, pos = 0;
  if (r < A.r_last) {
    // the rows are read once here: non-temporal, as the projection's other consumers take them
    const cv_u4 m = __builtin_nontemporal_load((const cv_u4 *)A.a + ((int64_t)r - A.bias));
    if (A.primary_only && !(m.z & BR_ROW_PRIMARY)) skipped = 1;
    else if ((int64_t)m.x >= A.n_tx) { skipped = 1; bad_tid = true; }   // nothing of it is looked up
    else {
      const uint32_t n = BR_ROW_NCIGAR(m.z);
      const uint64_t c = __builtin_nontemporal_load(A.cigar + ((int64_t)r - A.bias));
      tid = m.x; pos = m.y;
      base = A.off[tid]; len = A.off[tid + 1] - base;
      Walk w{pos, 0, 0};
      if (n <= 2u) {
        if (n >= 1u) walk_op(A.diff, base, len, w, (uint32_t)c, clipped);
        if (n == 2u) walk_op(A.diff, base, len, w, (uint32_t)(c >> 32), clipped);
        walk_end(A.diff, base, len, w, clipped);
        counted = 1;
      } else if (!in_pool(A, c, n)) bad_pool = true;
      else if (n <= COV_SMALL_OPS) {
        for (uint32_t k = 0; k < n; k++) walk_op(A.diff, base, len, w, A.pool[c + k], clipped);
        walk_end(A.diff, base, len, w, clipped);
        counted = 1;
      } else { wide_off = c; wide_n = n; counted = 1; }
    }
  }
  // the long CIGARs, one after the other: 64 ops a step, an op's position from the wave's scan of the reference bases in front of it
  uint64_t todo = __ballot(wide_n != 0u);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t off = __shfl(wide_off, src), w_base = __shfl(base, src), w_len = __shfl(len, src);
    const uint32_t n = (uint32_t)__shfl((int)wide_n, src);
    uint64_t p = __shfl(pos, src);
    for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
      const uint32_t k = k0 + (uint32_t)lane;
      const uint32_t op = k < n ? A.pool[off + k] : 4u;   // (past the end: a soft clip of no bases)
      const uint64_t bases = op >> 4, adv = op_covers(op) || op_skips(op) ? bases : 0ull;
      const uint64_t inc = wave_scan(adv);
      if (op_covers(op) && bases) cover(A.diff, w_base, w_len, p + inc - adv, p + inc, clipped);
      p += __shfl(inc, 63);
    }
  }
  // records: one atomic per distinct transcript among the wave's counted rows
  uint64_t live = __ballot(counted != 0u);
  while (live) {
    const int src = __ffsll((unsigned long long)live) - 1;
    const uint32_t t = (uint32_t)__shfl((int)tid, src);
    const uint64_t same = __ballot(counted != 0u && tid == t);
    if (lane == src) atomicAdd(A.records + t, (unsigned long long)__popcll((unsigned long long)same));
    live &= ~same;
  }
  counted = wave_sum(counted); skipped = wave_sum(skipped); clipped = wave_sum(clipped);
  const bool any_bad_pool = __ballot(bad_pool) != 0, any_bad_tid = __ballot(bad_tid) != 0;
  if (lane == 0) {
    if (counted) atomicAdd(A.counters + CV_COUNTED, (unsigned long long)counted);
    if (skipped) atomicAdd(A.counters + CV_SKIPPED, (unsigned long long)skipped);
    if (clipped) atomicAdd(A.counters + CV_CLIPPED, (unsigned long long)clipped);
    if (any_bad_pool) A.counters[CV_BAD_POOL] = 1;
    if (any_bad_tid) A.counters[CV_BAD_TID] = 1;
  }
}

namespace {
// four consecutive entries from d[i] on (i a multiple of 4), 0 for those at or past n
__device__ __forceinline__ cv_u4 load4(const uint32_t *d, int64_t i, int64_t n) {
  if (i + 4 <= n) return *(const cv_u4 *)(d + i);
  cv_u4 v = {0u, 0u, 0u, 0u};
  if (i < n) v.x = d[i];
  if (i + 1 < n) v.y = d[i + 1];
  if (i + 2 < n) v.z = d[i + 2];
  return v;
}
__device__ __forceinline__ void store4(uint32_t *d, int64_t i, int64_t n, cv_u4 v) {
  if (i + 4 <= n) { *(cv_u4 *)(d + i) = v; return; }
  if (i < n) d[i] = v.x;
  if (i + 1 < n) d[i + 1] = v.y;
  if (i + 2 < n) d[i + 2] = v.z;
}
// the first entry of lane `tid` in chunk j (of 1024 entries) of the tile that starts at t0
__device__ __forceinline__ int64_t chunk_at(int64_t t0, int j) { return t0 + (int64_t)j * 1024 + (int64_t)threadIdx.x * 4; }
}  // namespace

__global__ void __launch_bounds__(256) k_cov_tile_sum(const uint32_t *d, int64_t n, uint64_t *tile_sum) {
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) { const cv_u4 v = load4(d, chunk_at(t0, j), n); s += v.x + v.y + v.z + v.w; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = (uint64_t)(uint32_t)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// tile_pre: the exclusive scan of the tile sums (64-bit sums of 32-bit words: their low words are the sums modulo 2^32)
__global__ void __launch_bounds__(256) k_cov_tile_apply(uint32_t *d, int64_t n, const uint64_t *tile_pre) {
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  uint32_t carry = (uint32_t)tile_pre[blockIdx.x];
  for (int j = 0; j < 4; j++) {
    const int64_t i = chunk_at(t0, j);
    cv_u4 v = load4(d, i, n);
    v.y += v.x; v.z += v.y; v.w += v.z;
    uint32_t total;
    const uint32_t add = carry + block_excl_scan_256(v.w, sh, total);   // (the lanes' sums in front of this one's four)
    v.x += add; v.y += add; v.z += add; v.w += add;
    store4(d, i, n, v);
    carry += total;
  }
}

__global__ void __launch_bounds__(256) k_cov_summary_wave(const uint32_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned,
                                                          uint64_t *covered, uint32_t *max_depth) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tx) return;
  const uint64_t b = off[t], e = off[t + 1];
  if (e - b > (uint64_t)COV_WAVE_LEN) return;   // (k_cov_summary_long's)
  uint64_t sum = 0;
  uint32_t nz = 0, mx = 0;
  for (uint64_t i = b + (threadIdx.x & 63); i < e; i += 64) { const uint32_t v = depth[i]; sum += v; nz += v != 0u; mx = v > mx ? v : mx; }
  sum = wave_sum(sum); nz = wave_sum(nz); mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { aligned[t] = sum; covered[t] = nz; max_depth[t] = mx; }
}

__global__ void __launch_bounds__(256) k_cov_summary_long(const uint32_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned,
                                                          uint64_t *covered, uint32_t *max_depth) {
  __shared__ uint64_t sh_sum[4], sh_nz[4];
  __shared__ uint32_t sh_mx[4];
  for (int64_t t = blockIdx.x; t < n_tx; t += gridDim.x) {   // (everything that branches here is the same in the whole block)
    const uint64_t b = off[t], e = off[t + 1];
    if (e - b <= (uint64_t)COV_WAVE_LEN) continue;
    uint64_t sum = 0, nz = 0;
    uint32_t mx = 0;
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) { const uint32_t v = depth[i]; sum += v; nz += v != 0u; mx = v > mx ? v : mx; }
    sum = wave_sum(sum); nz = wave_sum(nz); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { sh_sum[threadIdx.x >> 6] = sum; sh_nz[threadIdx.x >> 6] = nz; sh_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t m = sh_mx[0];
      for (int k = 1; k < 4; k++) m = sh_mx[k] > m ? sh_mx[k] : m;
      aligned[t] = sh_sum[0] + sh_sum[1] + sh_sum[2] + sh_sum[3]; covered[t] = sh_nz[0] + sh_nz[1] + sh_nz[2] + sh_nz[3]; max_depth[t] = m;
    }
    __syncthreads();
  }
}

namespace {
// the transcript that owns base i (i < off[n_tx]): the last t of [lo, hi] with off[t] <= i -- off[t + 1] > i then, so transcripts
// without bases own nothing
__device__ __forceinline__ int64_t tx_of(const uint64_t *off, int64_t lo, int64_t hi, uint64_t i) {
  while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (off[mid] <= i) lo = mid; else hi = mid - 1; }
  return lo;
}
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
struct Quad { uint32_t d[4]; uint32_t heads, tails; uint32_t tx[4]; uint64_t sb[4]; };
__device__ __forceinline__ Quad quad_at(const uint32_t *depth, int64_t n, const uint64_t *off, const int64_t *sh_t, int64_t i0) {
  Quad q;
  const cv_u4 v = load4(depth, i0, n);
  q.d[0] = v.x; q.d[1] = v.y; q.d[2] = v.z; q.d[3] = v.w;
  const uint32_t prev = i0 > 0 ? depth[i0 - 1] : 0u, next = i0 + 4 < n ? depth[i0 + 4] : 0u;
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
    const uint32_t cur = q.d[k], before = k ? q.d[k - 1] : prev, behind = k < 3 ? q.d[k + 1] : next;
    if (cur != 0u && (i == sb || cur != before)) q.heads |= 1u << k;
    if (cur != 0u && (i + 1 == nb || cur != behind)) q.tails |= 1u << k;
  }
  return q;
}
}  // namespace

__global__ void __launch_bounds__(256) k_cov_count(const uint32_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt) {
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

__global__ void __launch_bounds__(256) k_cov_runs(const uint32_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre,
                                                  uint4 *runs) {
  __shared__ int64_t sh_t[2];
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  tile_span(off, n_tx, t0, n, sh_t);
  uint64_t carry = tile_pre[blockIdx.x];   // heads in front of the chunk
  cv_u2 *out = (cv_u2 *)runs;
  for (int j = 0; j < 4; j++) {
    const int64_t i0 = chunk_at(t0, j);
    Quad q;
    q.heads = q.tails = 0;
    if (i0 < n) q = quad_at(depth, n, off, sh_t, i0);
    uint32_t total;
    uint64_t h = carry + block_excl_scan_256((uint32_t)__popc(q.heads), sh, total);   // heads in front of base i0
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool head = (q.heads >> k) & 1u, tail = (q.tails >> k) & 1u;
      const uint64_t i = (uint64_t)i0 + (uint64_t)k;
      if (head) { const cv_u2 w = {q.tx[k], (uint32_t)(i - q.sb[k])}; out[2 * h] = w; }
      // a last base that is no head ends the run of the head in front of it
      if (tail) { const cv_u2 w = {(uint32_t)(i + 1 - q.sb[k]), q.d[k]}; out[2 * (head ? h : h - 1) + 1] = w; }
      h += head ? 1u : 0u;
    }
    carry += total;
  }
}

// ---- the weighted modes ---------------------------------------------------------------------------------------------------------------
// k_cov_add_w is k_cov_add with another end for a clamped interval: weight nh leaves + q / - q (mod 2^64) in the 64-bit diff;
// weight em, whose q is not known yet, runs it twice -- a pass that only counts a row's entries, and, once the host has made room,
// a pass that keeps them: a wave places its rows' entries by one atomic.  The walk, the paths and the counters are k_cov_add's.
namespace {
__device__ __forceinline__ void keep_entry(uint4 *arena, uint64_t cap, uint64_t slot, uint64_t w0, uint32_t len, uint32_t name) {
  if (slot < cap) arena[slot] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), len, name);
}
template <int MODE>
struct CovSink {
  unsigned long long *diff; uint64_t q;                 // COV_ADD_NH
  uint4 *arena; uint64_t cap, slot; uint32_t name;      // COV_ADD_KEEP: slot = the row's first
  uint32_t n;                                           // entries of the row so far
  __device__ __forceinline__ void put(uint64_t at, uint64_t len) {
    if (MODE == COV_ADD_NH) { atomicAdd(diff + at, (unsigned long long)q); atomicAdd(diff + at + len, (unsigned long long)(0ull - q)); }
    if (MODE == COV_ADD_KEEP) keep_entry(arena, cap, slot + n, at | (n ? 0ull : COV_KEEP_FIRST), (uint32_t)len, name);
    n++;
  }
};
template <int MODE>
__device__ __forceinline__ void cover_w(CovSink<MODE> &k, uint64_t base, uint64_t len, uint64_t s, uint64_t e, uint64_t &clipped) {
  const uint64_t cs = s < len ? s : len, ce = e < len ? e : len;
  clipped += (e - s) - (ce - cs);
  if (ce > cs) k.put(base + cs, ce - cs);
}
template <int MODE>
__device__ __forceinline__ void walk_op_w(CovSink<MODE> &k, uint64_t base, uint64_t len, Walk &w, uint32_t op, uint64_t &clipped) {
  const uint64_t n = op >> 4;
  if (op_covers(op)) {
    if (w.ce > w.cs && w.ce == w.p) w.ce += n;
    else { if (w.ce > w.cs) cover_w(k, base, len, w.cs, w.ce, clipped); w.cs = w.p; w.ce = w.p + n; }
    w.p += n;
  } else if (op_skips(op)) w.p += n;
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
__global__ void __launch_bounds__(256) k_cov_add_w(CovAddWArgs W) {
  const CovAddArgs &A = W.A;
  const uint64_t r = A.r_first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t counted = 0, skipped = 0, tid = 0, wide_n = 0, n_ops = 0, entries = 0, name = 0;
  bool bad_pool = false, bad_tid = false, bad_nh = false, bad_names = false, walks = false;
  uint64_t clipped = 0, base = 0, len = 0, wide_off = 0, pos = 0, q = 0, cref = 0, slot = 0;
  if (r < A.r_last) {
    const cv_u4 m = __builtin_nontemporal_load((const cv_u4 *)A.a + ((int64_t)r - A.bias));
    if (A.primary_only && !(m.z & BR_ROW_PRIMARY)) skipped = 1;
    else if ((int64_t)m.x >= A.n_tx) { skipped = 1; bad_tid = true; }
    else if (MODE == COV_ADD_NH && m.w == 0u) { skipped = 1; bad_nh = true; }   // no weight to give it
    else if (MODE != COV_ADD_NH && !name_of(W, r, name)) { skipped = 1; bad_names = true; }
    else {
      n_ops = BR_ROW_NCIGAR(m.z);
      cref = __builtin_nontemporal_load(A.cigar + ((int64_t)r - A.bias));
      tid = m.x; pos = m.y;
      base = A.off[tid]; len = A.off[tid + 1] - base;
      if (MODE == COV_ADD_NH) q = ((1ull << 32) + (uint64_t)(m.w >> 1)) / (uint64_t)m.w;
      if (n_ops > 2u && !in_pool(A, cref, n_ops)) bad_pool = true;
      else walks = true;
    }
  }
  if (MODE == COV_ADD_KEEP) {   // the wave's rows, one after the other in the arena: the count pass left every row's entries
    const uint64_t mine = walks ? (uint64_t)W.row_entries[r - A.r_first] : 0ull;
    const uint64_t incl = wave_scan(mine);
    uint64_t first = 0;
    if (lane == 63 && incl) first = atomicAdd(A.counters + CV_KEPT, (unsigned long long)incl);
    slot = __shfl(first, 63) + incl - mine;
  }
  if (walks) {
    counted = 1;
    if (n_ops <= COV_SMALL_OPS) {
      CovSink<MODE> k{W.diff, q, W.arena, W.arena_cap, slot, name, 0u};
      Walk w{pos, 0, 0};
      if (n_ops <= 2u) {
        if (n_ops >= 1u) walk_op_w(k, base, len, w, (uint32_t)cref, clipped);
        if (n_ops == 2u) walk_op_w(k, base, len, w, (uint32_t)(cref >> 32), clipped);
      } else {
        for (uint32_t i = 0; i < n_ops; i++) walk_op_w(k, base, len, w, A.pool[cref + i], clipped);
      }
      if (w.ce > w.cs) cover_w(k, base, len, w.cs, w.ce, clipped);
      if (MODE == COV_ADD_KEEP && k.n == 0u) keep_entry(W.arena, W.arena_cap, slot, (uint64_t)tid, 0u, name);
      entries = k.n ? k.n : 1u;
    } else { wide_off = cref; wide_n = n_ops; }
  }
  // the long CIGARs by the wave, as in k_cov_add: every covering op is an interval of its own here
  uint64_t todo = __ballot(wide_n != 0u);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t off = __shfl(wide_off, src), w_base = __shfl(base, src), w_len = __shfl(len, src), w_q = __shfl(q, src), w_slot = __shfl(slot, src);
    const uint32_t n = (uint32_t)__shfl((int)wide_n, src), w_name = (uint32_t)__shfl((int)name, src), w_tid = (uint32_t)__shfl((int)tid, src);
    uint64_t p = __shfl(pos, src);
    uint32_t done = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
      const uint32_t i = k0 + (uint32_t)lane;
      const uint32_t op = i < n ? A.pool[off + i] : 4u;
      const uint64_t bases = op >> 4, adv = op_covers(op) || op_skips(op) ? bases : 0ull;
      const uint64_t inc = wave_scan(adv);
      uint64_t cs = 0, ce = 0;
      if (op_covers(op) && bases) {
        const uint64_t s = p + inc - adv, e = p + inc;
        cs = s < w_len ? s : w_len; ce = e < w_len ? e : w_len;
        clipped += (e - s) - (ce - cs);
      }
      const bool emit = ce > cs;
      if (MODE == COV_ADD_NH) {
        if (emit) { atomicAdd(W.diff + w_base + cs, (unsigned long long)w_q); atomicAdd(W.diff + w_base + ce, (unsigned long long)(0ull - w_q)); }
      } else {
        const uint64_t bal = __ballot(emit);
        if (MODE == COV_ADD_KEEP && emit) {
          const uint32_t at = done + (uint32_t)__popcll((unsigned long long)(bal & ((1ull << lane) - 1ull)));
          keep_entry(W.arena, W.arena_cap, w_slot + at, (w_base + cs) | (at ? 0ull : COV_KEEP_FIRST), (uint32_t)(ce - cs), w_name);
        }
        done += (uint32_t)__popcll((unsigned long long)bal);
      }
      p += __shfl(inc, 63);
    }
    if (MODE != COV_ADD_NH) {
      if (done == 0u) { if (MODE == COV_ADD_KEEP && lane == src) keep_entry(W.arena, W.arena_cap, w_slot, (uint64_t)w_tid, 0u, w_name); done = 1u; }
      if (lane == src) entries = done;
    }
  }
  const bool any_bad_pool = __ballot(bad_pool) != 0, any_bad_names = __ballot(bad_names) != 0;
  if (MODE == COV_ADD_COUNT) {   // nothing is counted yet: the keep pass does that
    if (r < A.r_last) W.row_entries[r - A.r_first] = entries;
    const uint64_t sum = wave_sum((uint64_t)entries);
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
    if (MODE == COV_ADD_NH) qs = wave_sum(in ? q : 0ull);
    if (lane == src) {
      atomicAdd(A.records + t, (unsigned long long)__popcll((unsigned long long)same));
      if (MODE == COV_ADD_NH) atomicAdd(W.weight_sum + t, (unsigned long long)qs);
    }
    live &= ~same;
  }
  counted = wave_sum(counted); skipped = wave_sum(skipped); clipped = wave_sum(clipped);
  const bool any_bad_tid = __ballot(bad_tid) != 0, any_bad_nh = __ballot(bad_nh) != 0;
  if (lane == 0) {
    if (counted) atomicAdd(A.counters + CV_COUNTED, (unsigned long long)counted);
    if (skipped) atomicAdd(A.counters + CV_SKIPPED, (unsigned long long)skipped);
    if (clipped) atomicAdd(A.counters + CV_CLIPPED, (unsigned long long)clipped);
    if (any_bad_pool) A.counters[CV_BAD_POOL] = 1;
    if (any_bad_tid) A.counters[CV_BAD_TID] = 1;
    if (any_bad_nh) A.counters[CV_BAD_NH] = 1;
    if (any_bad_names) A.counters[CV_BAD_NAMES] = 1;
  }
}

namespace {
typedef uint64_t cv_q2 __attribute__((ext_vector_type(2)));
struct Q4 { uint64_t v[4]; };
// four consecutive 64-bit entries from d[i] on (i a multiple of 4), 0 for those at or past n
__device__ __forceinline__ Q4 load4q(const uint64_t *d, int64_t i, int64_t n) {
  Q4 r = {{0ull, 0ull, 0ull, 0ull}};
  if (i + 4 <= n) {
    const cv_q2 a = *(const cv_q2 *)(d + i), b = *(const cv_q2 *)(d + i + 2);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = b.x; r.v[3] = b.y;
    return r;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) if (i + k < n) r.v[k] = d[i + k];
  return r;
}
__device__ __forceinline__ void store4q(uint64_t *d, int64_t i, int64_t n, const Q4 &r) {
  if (i + 4 <= n) {
    const cv_q2 a = {r.v[0], r.v[1]}, b = {r.v[2], r.v[3]};
    *(cv_q2 *)(d + i) = a; *(cv_q2 *)(d + i + 2) = b;
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) if (i + k < n) d[i + k] = r.v[k];
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

__global__ void __launch_bounds__(256) k_cov_tile_sum64(const uint64_t *d, int64_t n, uint64_t *tile_sum) {
  __shared__ uint64_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  uint64_t s = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) { const Q4 v = load4q(d, chunk_at(t0, j), n); s += v.v[0] + v.v[1] + v.v[2] + v.v[3]; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// tile_pre: the exclusive scan of the tile sums, modulo 2^64 like everything here
__global__ void __launch_bounds__(256) k_cov_tile_apply64(uint64_t *d, int64_t n, const uint64_t *tile_pre) {
  __shared__ uint64_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  uint64_t carry = tile_pre[blockIdx.x];
  for (int j = 0; j < 4; j++) {
    const int64_t i = chunk_at(t0, j);
    Q4 v = load4q(d, i, n);
    v.v[1] += v.v[0]; v.v[2] += v.v[1]; v.v[3] += v.v[2];
    uint64_t total;
    const uint64_t add = carry + block_excl_scan_256(v.v[3], sh, total);
    v.v[0] += add; v.v[1] += add; v.v[2] += add; v.v[3] += add;
    store4q(d, i, n, v);
    carry += total;
  }
}

__global__ void __launch_bounds__(256) k_cov_summary_wave64(const uint64_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned_hi,
                                                            uint64_t *aligned_lo, uint64_t *covered, uint64_t *max_depth) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tx) return;
  const uint64_t b = off[t], e = off[t + 1];
  if (e - b > (uint64_t)COV_WAVE_LEN) return;   // (k_cov_summary_long64's)
  uint64_t hi = 0, lo = 0, nz = 0, mx = 0;
  for (uint64_t i = b + (threadIdx.x & 63); i < e; i += 64) { const uint64_t v = depth[i]; hi += v >> 32; lo += v & 0xffffffffull; nz += v != 0ull; mx = v > mx ? v : mx; }
  hi = wave_sum(hi); lo = wave_sum(lo); nz = wave_sum(nz); mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { aligned_hi[t] = hi; aligned_lo[t] = lo; covered[t] = nz; max_depth[t] = mx; }
}

__global__ void __launch_bounds__(256) k_cov_summary_long64(const uint64_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned_hi,
                                                            uint64_t *aligned_lo, uint64_t *covered, uint64_t *max_depth) {
  __shared__ uint64_t sh_hi[4], sh_lo[4], sh_nz[4], sh_mx[4];
  for (int64_t t = blockIdx.x; t < n_tx; t += gridDim.x) {   // (everything that branches here is the same in the whole block)
    const uint64_t b = off[t], e = off[t + 1];
    if (e - b <= (uint64_t)COV_WAVE_LEN) continue;
    uint64_t hi = 0, lo = 0, nz = 0, mx = 0;
    for (uint64_t i = b + threadIdx.x; i < e; i += 256) { const uint64_t v = depth[i]; hi += v >> 32; lo += v & 0xffffffffull; nz += v != 0ull; mx = v > mx ? v : mx; }
    hi = wave_sum(hi); lo = wave_sum(lo); nz = wave_sum(nz); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { sh_hi[threadIdx.x >> 6] = hi; sh_lo[threadIdx.x >> 6] = lo; sh_nz[threadIdx.x >> 6] = nz; sh_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t m = sh_mx[0];
      for (int k = 1; k < 4; k++) m = sh_mx[k] > m ? sh_mx[k] : m;
      aligned_hi[t] = sh_hi[0] + sh_hi[1] + sh_hi[2] + sh_hi[3]; aligned_lo[t] = sh_lo[0] + sh_lo[1] + sh_lo[2] + sh_lo[3];
      covered[t] = sh_nz[0] + sh_nz[1] + sh_nz[2] + sh_nz[3]; max_depth[t] = m;
    }
    __syncthreads();
  }
}

namespace {
// quad_at over 64-bit depths
struct Quad64 { uint64_t d[4]; uint32_t heads, tails; uint32_t tx[4]; uint64_t sb[4]; };
__device__ __forceinline__ Quad64 quad_at64(const uint64_t *depth, int64_t n, const uint64_t *off, const int64_t *sh_t, int64_t i0) {
  Quad64 q;
  const Q4 v = load4q(depth, i0, n);
  q.d[0] = v.v[0]; q.d[1] = v.v[1]; q.d[2] = v.v[2]; q.d[3] = v.v[3];
  const uint64_t prev = i0 > 0 ? depth[i0 - 1] : 0ull, next = i0 + 4 < n ? depth[i0 + 4] : 0ull;
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
    const uint64_t cur = q.d[k], before = k ? q.d[k - 1] : prev, behind = k < 3 ? q.d[k + 1] : next;
    if (cur != 0ull && (i == sb || cur != before)) q.heads |= 1u << k;
    if (cur != 0ull && (i + 1 == nb || cur != behind)) q.tails |= 1u << k;
  }
  return q;
}
}  // namespace

__global__ void __launch_bounds__(256) k_cov_count64(const uint64_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt) {
  __shared__ int64_t sh_t[2];
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  tile_span(off, n_tx, t0, n, sh_t);
  uint32_t cnt = 0;
  for (int j = 0; j < 4; j++) {
    const int64_t i0 = chunk_at(t0, j);
    if (i0 < n) cnt += (uint32_t)__popc(quad_at64(depth, n, off, sh_t, i0).heads);
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint64_t)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// the head's lane stores (transcript, start), the lane of the run's last base (end, 0) and the depth
__global__ void __launch_bounds__(256) k_cov_runs64(const uint64_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre,
                                                    uint4 *run4, uint64_t *run_depth) {
  __shared__ int64_t sh_t[2];
  __shared__ uint32_t sh[4];
  const int64_t t0 = (int64_t)blockIdx.x * COV_TILE;
  tile_span(off, n_tx, t0, n, sh_t);
  uint64_t carry = tile_pre[blockIdx.x];   // heads in front of the chunk
  cv_u2 *out = (cv_u2 *)run4;
  for (int j = 0; j < 4; j++) {
    const int64_t i0 = chunk_at(t0, j);
    Quad64 q;
    q.heads = q.tails = 0;
    if (i0 < n) q = quad_at64(depth, n, off, sh_t, i0);
    uint32_t total;
    uint64_t h = carry + block_excl_scan_256((uint32_t)__popc(q.heads), sh, total);   // heads in front of base i0
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool head = (q.heads >> k) & 1u, tail = (q.tails >> k) & 1u;
      const uint64_t i = (uint64_t)i0 + (uint64_t)k;
      if (head) { const cv_u2 w = {q.tx[k], (uint32_t)(i - q.sb[k])}; out[2 * h] = w; }
      if (tail) { const uint64_t run = head ? h : h - 1; const cv_u2 w = {(uint32_t)(i + 1 - q.sb[k]), 0u}; out[2 * run + 1] = w; run_depth[run] = q.d[k]; }
      h += head ? 1u : 0u;
    }
    carry += total;
  }
}

namespace {
unsigned cov_tiles(int64_t n) { return (unsigned)((n + COV_TILE - 1) / COV_TILE); }
}  // namespace

void launch_cov_add_w(hipStream_t st, const CovAddWArgs &W, int mode) {
  const uint64_t n = W.A.r_last - W.A.r_first;
  if (!n) return;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (mode == COV_ADD_NH) hipLaunchKernelGGL(k_cov_add_w<COV_ADD_NH>, grid, dim3(256), 0, st, W);
  else if (mode == COV_ADD_COUNT) hipLaunchKernelGGL(k_cov_add_w<COV_ADD_COUNT>, grid, dim3(256), 0, st, W);
  else hipLaunchKernelGGL(k_cov_add_w<COV_ADD_KEEP>, grid, dim3(256), 0, st, W);
}
void launch_cov_apply(hipStream_t st, const CovApplyArgs &P) {
  if (P.n) hipLaunchKernelGGL(k_cov_apply, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, st, P);
}
void launch_cov_scan64(hipStream_t st, uint64_t *depth, int64_t n, uint64_t *tile_sum, uint64_t *scan_tmp) {
  if (n <= 0) return;
  const unsigned tiles = cov_tiles(n);
  hipLaunchKernelGGL(k_cov_tile_sum64, dim3(tiles), dim3(256), 0, st, (const uint64_t *)depth, n, tile_sum);
  launch_scan(st, tile_sum, (int64_t)tiles, scan_tmp);
  hipLaunchKernelGGL(k_cov_tile_apply64, dim3(tiles), dim3(256), 0, st, depth, n, (const uint64_t *)tile_sum);
}
void launch_cov_summary64(hipStream_t st, const uint64_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned_hi, uint64_t *aligned_lo,
                          uint64_t *covered, uint64_t *max_depth) {
  if (n_tx <= 0) return;
  hipLaunchKernelGGL(k_cov_summary_wave64, dim3((unsigned)((n_tx + 3) / 4)), dim3(256), 0, st, depth, off, n_tx, aligned_hi, aligned_lo, covered, max_depth);
  const unsigned grid = (unsigned)(n_tx < (int64_t)COV_LONG_GRID ? n_tx : (int64_t)COV_LONG_GRID);
  hipLaunchKernelGGL(k_cov_summary_long64, dim3(grid), dim3(256), 0, st, depth, off, n_tx, aligned_hi, aligned_lo, covered, max_depth);
}
void launch_cov_count64(hipStream_t st, const uint64_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt) {
  if (n > 0) hipLaunchKernelGGL(k_cov_count64, dim3(cov_tiles(n)), dim3(256), 0, st, depth, n, off, n_tx, tile_cnt);
}
void launch_cov_runs64(hipStream_t st, const uint64_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *run4,
                       uint64_t *run_depth) {
  if (n > 0) hipLaunchKernelGGL(k_cov_runs64, dim3(cov_tiles(n)), dim3(256), 0, st, depth, n, off, n_tx, tile_pre, run4, run_depth);
}

void launch_cov_add(hipStream_t st, const CovAddArgs &A) {
  const uint64_t n = A.r_last - A.r_first;
  if (n) hipLaunchKernelGGL(k_cov_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
}
void launch_cov_scan(hipStream_t st, uint32_t *depth, int64_t n, uint64_t *tile_sum, uint64_t *scan_tmp) {
  if (n <= 0) return;
  const unsigned tiles = cov_tiles(n);
  hipLaunchKernelGGL(k_cov_tile_sum, dim3(tiles), dim3(256), 0, st, (const uint32_t *)depth, n, tile_sum);
  launch_scan(st, tile_sum, (int64_t)tiles, scan_tmp);
  hipLaunchKernelGGL(k_cov_tile_apply, dim3(tiles), dim3(256), 0, st, depth, n, (const uint64_t *)tile_sum);
}
void launch_cov_summary(hipStream_t st, const uint32_t *depth, const uint64_t *off, int64_t n_tx, uint64_t *aligned, uint64_t *covered,
                        uint32_t *max_depth) {
  if (n_tx <= 0) return;
  hipLaunchKernelGGL(k_cov_summary_wave, dim3((unsigned)((n_tx + 3) / 4)), dim3(256), 0, st, depth, off, n_tx, aligned, covered, max_depth);
  const unsigned grid = (unsigned)(n_tx < (int64_t)COV_LONG_GRID ? n_tx : (int64_t)COV_LONG_GRID);
  hipLaunchKernelGGL(k_cov_summary_long, dim3(grid), dim3(256), 0, st, depth, off, n_tx, aligned, covered, max_depth);
}
void launch_cov_count(hipStream_t st, const uint32_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, uint64_t *tile_cnt) {
  if (n > 0) hipLaunchKernelGGL(k_cov_count, dim3(cov_tiles(n)), dim3(256), 0, st, depth, n, off, n_tx, tile_cnt);
}
void launch_cov_runs(hipStream_t st, const uint32_t *depth, int64_t n, const uint64_t *off, int64_t n_tx, const uint64_t *tile_pre, uint4 *runs) {
  if (n > 0) hipLaunchKernelGGL(k_cov_runs, dim3(cov_tiles(n)), dim3(256), 0, st, depth, n, off, n_tx, tile_pre, runs);
}

}  // namespace br
