// The posterior of every projected record and the rewritten record stream on the device (host side: assign.cpp, which holds the
// pipeline's description; the definitions -- p, m, w, the draw, the rewritten record -- are in bramble_amd.h, br_assign).
//
//   add      k_as_add: a lane per row: the note (name by the search of k_cov_add, transcript, FIRST / PAIRED) and the record's
//            offset in the arena; k_as_place: every record belongs to a placement that lies inside its name
//   finish   k_as_p (the bounds-checked look-up of k_cov_apply) -> k_as_m (a lane per record over its name's records; the names
//            above AS_M_LANE_MAX records are listed) -> k_as_m_big (a wave per listed name) -> k_as_w -> k_as_draw (mode sample:
//            the first record's lane walks its name's placements in order; the sums are sequential by definition) -> k_as_rank;
//            then, with records, k_as_select over the scanned ranks
//   next     k_as_cut, k_as_write: AS_WRITE_LANES lanes per kept record
//
// All floating-point work is float64, one operation at a time (the unit is built with -ffp-contract=off); the counters are
// integer atomics, one per wave.
#include <hip/hip_runtime.h>

#include "../../include/bramble_amd.h"
#include "assign_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
// the add-order name of row r, from the add's offsets (name_of of coverage_kernels.hip); false where they do not give one
__device__ __forceinline__ bool as_name_of(const AsAddArgs &A, uint64_t r, uint32_t &name) {
  const NameWindow &N = A.names;
  const uint32_t a0 = N.group_off[0], a1 = N.group_off[N.n_groups];
  if (a1 <= a0) return false;
  const auto ro = [&](uint32_t a) { return N.row_off[(int64_t)a - N.ro_bias]; };
  uint32_t lo = a0, hi = a1 - 1u;   // the last alignment of [a0, a1) whose rows begin at or in front of r
  while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1u) / 2u; if (ro(mid) <= r) lo = mid; else hi = mid - 1u; }
  if (!(ro(lo) <= r && r < ro(lo + 1u))) return false;
  int64_t glo = 0, ghi = N.n_groups - 1;   // the last name whose alignments begin at or in front of it
  while (glo < ghi) { const int64_t mid = (glo + ghi + 1) >> 1; if (N.group_off[mid] <= lo) glo = mid; else ghi = mid - 1; }
  if (!(N.group_off[glo] <= lo && lo < N.group_off[glo + 1])) return false;
  name = (uint32_t)(A.name_base + (uint64_t)glo);
  return true;
}
// the first record of [lo, hi) whose name is >= g (hi when none): the names ascend with the records
__device__ __forceinline__ uint64_t name_bound(const uint4 *note, uint64_t lo, uint64_t hi, uint64_t g) {
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if ((uint64_t)note[mid].x < g) lo = mid + 1; else hi = mid; }
  return lo;
}
// Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1): the first two output words as one 64-bit number (the generator
// of the bootstrap, quant_kernels.hip, whose counters have c3 = 0)
__device__ __forceinline__ uint64_t philox4_u64(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (uint64_t)c0 | ((uint64_t)c1 << 32);
}
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }
}  // namespace

// ---- add -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_as_add(AsAddArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, n = A.names.r_last - A.names.r_first;
  bool bad_name = false, bad_off = false;
  if (i < n) {
    const uint64_t r = A.names.r_first + i;
    const uint4 m = A.a[(int64_t)r - A.a_bias];
    uint32_t name = 0xffffffffu;
    if (!as_name_of(A, r, name)) { bad_name = true; name = 0xffffffffu; }
    const uint32_t bits = ((m.z & BR_ROW_FIRST) ? AS_FIRST : 0u) | ((m.z & BR_ROW_PAIRED) ? AS_PAIRED : 0u);
    A.note[A.n0 + i] = make_uint4(name, m.x, bits, 0u);
    if (A.recs.rec_off) {
      const uint64_t *ro = A.recs.rec_off - A.recs.rec_bias;
      const uint64_t first = ro[A.names.r_first], at = ro[r], next = ro[r + 1];
      if (at < first || next < at) bad_off = true;
      A.off[A.n0 + i] = A.arena_base + (at - first);
      if (i == n - 1) A.off[A.n0 + n] = A.arena_base + (next - first);
    }
  }
  count_lanes(bad_name, A.counters + AS_BAD_NAMES);
  count_lanes(bad_off, A.counters + AS_BAD_OFF);
}

// the notes of the add are written: a FIRST | PAIRED record's mate is the next record, inside the name, PAIRED and not FIRST; a
// record that is not FIRST is such a mate
__global__ void __launch_bounds__(256) k_as_place(const uint4 *note, uint64_t n, unsigned long long *counters) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const uint4 me = note[i];
    if (me.z & AS_FIRST) {
      if (me.z & AS_PAIRED) {
        if (i + 1 >= n) bad = true;
        else { const uint4 nx = note[i + 1]; bad = nx.x != me.x || !(nx.z & AS_PAIRED) || (nx.z & AS_FIRST); }
      }
    } else {
      if (!(me.z & AS_PAIRED) || i == 0) bad = true;
      else { const uint4 pv = note[i - 1]; bad = pv.x != me.x || (pv.z & (AS_FIRST | AS_PAIRED)) != (AS_FIRST | AS_PAIRED); }
    }
  }
  count_lanes(bad, counters + AS_BAD_PLACE);
}

// ---- finish --------------------------------------------------------------------------------------------------------------------
// p(r): name -> class -> the transcript's entry among the class's labels -> the posterior.  Nothing read from a table becomes an
// address before it was compared with that table's size; what fails is counted and gets p = 0
__global__ void __launch_bounds__(256) k_as_p(AsFinishArgs F) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad_name = false, bad_class = false, bad_label = false, bad_post = false;
  if (r < F.n) {
    const uint4 e = F.note[r];
    double p = 0.0;
    if ((uint64_t)e.x >= F.n_names) bad_name = true;
    else {
      const uint64_t cls = F.name_cls[e.x];
      if (cls >= F.n_cls) bad_class = true;
      else {
        const uint64_t b = F.label_off[cls], z = F.label_off[cls + 1];
        if (b > z || z > F.n_lab) bad_class = true;
        else {
          uint64_t lo = b, hi = z;   // the first label of [b, z) that is >= t
          while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (F.labels[mid] < e.y) lo = mid + 1; else hi = mid; }
          if (lo >= z || F.labels[lo] != e.y) bad_label = true;
          else {
            const double q = F.post[lo];
            if (!(q >= 0.0 && q <= 1.0)) bad_post = true; else p = q;
          }
        }
      }
    }
    F.p[r] = p;
  }
  count_lanes(bad_name, F.counters + AS_BAD_NAME);
  count_lanes(bad_class, F.counters + AS_BAD_CLASS);
  count_lanes(bad_label, F.counters + AS_BAD_LABEL);
  count_lanes(bad_post, F.counters + AS_BAD_POST);
}

// m(r) for the names of up to AS_M_LANE_MAX records; the first record of a longer name puts it on the list
__global__ void __launch_bounds__(256) k_as_m(AsFinishArgs F) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool head = false;
  if (r < F.n) {
    const uint4 me = F.note[r];
    const uint64_t b = name_bound(F.note, 0, r, me.x), e = name_bound(F.note, r + 1, F.n, (uint64_t)me.x + 1);
    head = r == b;
    if (e - b <= AS_M_LANE_MAX) {
      uint32_t c = 0;
      for (uint64_t j = b; j < e; j++) c += F.note[j].y == me.y;
      F.m[r] = c;
    } else if (head) {
      const unsigned long long k = atomicAdd(F.counters + AS_N_BIG, 1ull);
      F.big[k] = (uint32_t)b;   // (at most n / (AS_M_LANE_MAX + 1) such names)
    }
  }
  count_lanes(head, F.counters + AS_N_NAMED);
}

// a wave per listed name: record after record, the lanes count its transcript among the name's records
__global__ void __launch_bounds__(256) k_as_m_big(AsFinishArgs F) {
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= F.counters[AS_N_BIG]) return;   // (the same in every lane of the wave)
  const uint64_t b = F.big[k];
  const uint64_t g = F.note[b].x, e = name_bound(F.note, b + 1, F.n, g + 1);
  for (uint64_t i = b; i < e; i++) {
    const uint32_t t = F.note[i].y;
    uint32_t c = 0;
    for (uint64_t j = b + lane; j < e; j += 64) c += F.note[j].y == t;
    c = wave_sum(c);
    if (lane == 0) F.m[i] = c;
  }
}

// w of the record's placement: the leader's term first, then the mate's
__global__ void __launch_bounds__(256) k_as_w(AsFinishArgs F) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= F.n) return;
  const uint32_t bits = F.note[r].z;
  const uint64_t lead = (bits & AS_FIRST) || r == 0 ? r : r - 1;
  double w = F.p[lead] / (double)F.m[lead];
  if ((bits & AS_PAIRED) && lead + 1 < F.n) w = w + F.p[lead + 1] / (double)F.m[lead + 1];
  F.w[r] = w;
  if (F.mode == 0) F.kept[r] = 1;
}

// mode sample: the lane of a name's first record draws the name's placement and writes kept for all of its records
__global__ void __launch_bounds__(256) k_as_draw(AsFinishArgs F) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= F.n) return;
  const uint32_t g = F.note[r].x;
  if (r > 0 && F.note[r - 1].x == g) return;
  const uint64_t e = name_bound(F.note, r + 1, F.n, (uint64_t)g + 1);
  double W = 0.0;
  for (uint64_t j = r; j < e; j++) if (F.note[j].z & AS_FIRST) W = W + F.w[j];
  const uint64_t u = philox4_u64(g, 0u, 0u, 1u, F.k0, F.k1);   // (name < 2^32: the counter's second word is 0)
  const double U = (double)(u >> 11) * 0x1p-53, target = U * W;
  uint64_t pick = e, last_pos = e, first = e;
  double cum = 0.0;
  for (uint64_t j = r; j < e; j++) {
    if (!(F.note[j].z & AS_FIRST)) continue;
    const double wj = F.w[j];
    if (first == e) first = j;
    if (wj > 0.0) last_pos = j;
    cum = cum + wj;
    if (cum > target) { pick = j; break; }
  }
  if (pick == e) pick = last_pos != e ? last_pos : first;   // (first == e: no placement at all -- the add refuses such a name)
  const bool pair = pick < e && (F.note[pick].z & AS_PAIRED);
  for (uint64_t j = r; j < e; j++) F.kept[j] = j == pick || (pair && j == pick + 1);
}

__global__ void __launch_bounds__(256) k_as_rank(const uint8_t *kept, uint64_t n, uint64_t *rank) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n) rank[r] = kept[r];
}

__global__ void __launch_bounds__(256) k_as_select(const uint8_t *kept, const uint64_t *rank, const uint64_t *off, uint64_t n, uint32_t *sel, uint64_t *out_len) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n || !kept[r]) return;
  const uint64_t k = rank[r];
  sel[k] = (uint32_t)r;
  out_len[k] = off[r + 1] - off[r] + AS_TAG_BYTES;
}

// ---- next ----------------------------------------------------------------------------------------------------------------------
__global__ void k_as_cut(const uint64_t *out_off, uint64_t n_out, uint64_t cur, uint64_t max_bytes, uint64_t *res) {
  const uint64_t base = out_off[cur];
  uint64_t lo = cur + 1, hi = n_out;   // the largest e with out_off[e] - base <= max_bytes
  while (lo < hi) { const uint64_t mid = (lo + hi + 1) >> 1; if (out_off[mid] - base <= max_bytes) lo = mid; else hi = mid - 1; }
  res[0] = lo; res[1] = out_off[lo] - base;
}

namespace {
// bytes [at, at + n) of a rewritten record (n <= 4) become (old & keep) | put, little-endian
struct AsPatch { uint32_t at, n, keep, put; };
// v holds the bytes [p, p + nb) of the record (nb <= 8, byte p lowest): the patch's part of them
__device__ __forceinline__ uint64_t as_apply(uint64_t v, uint64_t p, uint32_t nb, const AsPatch &q) {
  if (q.n == 0u || (uint64_t)q.at >= p + nb || (uint64_t)q.at + q.n <= p) return v;
  const uint64_t span = q.n >= 4u ? 0xffffffffull : (1ull << (8u * q.n)) - 1ull;
  uint64_t clear = span & ~(uint64_t)q.keep, set = (uint64_t)q.put & span;
  if ((uint64_t)q.at >= p) { const uint32_t sh = (uint32_t)((uint64_t)q.at - p) * 8u; clear <<= sh; set <<= sh; }
  else { const uint32_t sh = (uint32_t)(p - (uint64_t)q.at) * 8u; clear >>= sh; set >>= sh; }
  return (v & ~clear) | set;
}
// Where the encoder's NH:i and HI:i entries begin in the record s of len bytes ([block_size] first): they are the aux area's last
// entries -- NH, (AS for long reads,) HI -- in front of a CG:B,I spill, which only a record with the placeholder CIGAR
// <l_seq>S<n>N has and which the walk over the aux area finds.  false: the record does not end that way
__device__ __forceinline__ bool as_find_nh_hi(const uint8_t *s, uint64_t len, uint32_t &nh_at, uint32_t &hi_at) {
  if (len < 36 || len > 0xffffffffull) return false;
  const uint64_t l_name = s[12], n_cig = ld16(s + 16), l_seq = ld32(s + 20);
  const uint64_t aux = 36 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq;
  if (aux > len) return false;
  uint64_t tail = len;
  if (n_cig == 2) {
    const uint32_t c0 = ld32(s + 36 + l_name), c1 = ld32(s + 40 + l_name);
    if ((c0 & 15u) == 4u && (uint64_t)(c0 >> 4) == l_seq && (c1 & 15u) == 3u) {
      for (uint64_t p = aux; p + 3 <= len;) {
        const uint8_t ty = s[p + 2];
        if (s[p] == 'C' && s[p + 1] == 'G' && ty == 'B' && p + 8 <= len && s[p + 3] == 'I') { tail = p; break; }
        uint64_t sz;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') { uint64_t q = p + 3; while (q < len && s[q]) q++; sz = q - (p + 3) + 1; }
        else if (ty == 'B' && p + 8 <= len) {
          const uint8_t sub = s[p + 3];
          const uint64_t each = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : 4;
          sz = 5 + each * (uint64_t)ld32(s + p + 4);
        } else break;
        p += 3 + sz;
      }
    }
  }
  if (tail < aux + 14) return false;
  const auto is = [&](uint64_t at, char a, char b) { return s[at] == (uint8_t)a && s[at + 1] == (uint8_t)b && s[at + 2] == (uint8_t)'i'; };
  if (!is(tail - 7, 'H', 'I')) return false;
  if (is(tail - 14, 'N', 'H')) nh_at = (uint32_t)(tail - 14);
  else if (tail >= aux + 21 && is(tail - 14, 'A', 'S') && is(tail - 21, 'N', 'H')) nh_at = (uint32_t)(tail - 21);
  else return false;
  hi_at = (uint32_t)(tail - 7);
  return true;
}
}  // namespace

// AS_WRITE_LANES lanes per kept record, grid-stride.  Source and destination have any alignment (they differ by a multiple of 7
// plus the skipped records): the destination's aligned 8-byte words are built from two aligned, non-temporal source words (the
// arena is read once), the head in front of the first aligned word and the tail -- the record's last bytes and the seven of the
// tag -- go byte by byte.  The patches (block_size; mode sample: MAPQ, the flag's high byte, the values of NH and HI) are applied
// to the words in registers, so every byte of the destination is stored once
__global__ void __launch_bounds__(256) k_as_write(AsWriteArgs W) {
  constexpr uint32_t G = AS_WRITE_LANES;
  const uint32_t lane = threadIdx.x & (G - 1);
  const uint64_t groups = (uint64_t)gridDim.x * (256 / G);
  const uint64_t base = W.out_off[W.cur];
  for (uint64_t j = W.cur + (uint64_t)blockIdx.x * (256 / G) + threadIdx.x / G; j < W.e; j += groups) {
    const uint64_t r = W.sel[j];
    const uint64_t d = W.out_off[j] - base, len = W.off[r + 1] - W.off[r], total = len + AS_TAG_BYTES;
    const uint8_t *s = W.arena + W.off[r];
    uint8_t *t = W.dst + d;
    const uint32_t zw = __float_as_uint((float)W.w[r]);
    AsPatch P[5] = {};
    if (len >= 4) P[0] = AsPatch{0u, 4u, 0u, ld32(s) + AS_TAG_BYTES};
    if (W.mode == 1) {
      uint32_t nh_at = 0, hi_at = 0;
      if (as_find_nh_hi(s, len, nh_at, hi_at)) {
        P[1] = AsPatch{13u, 1u, 0u, W.mapq};        // MAPQ
        P[2] = AsPatch{19u, 1u, 0xfeu, 0u};         // flag bit 0x100
        P[3] = AsPatch{nh_at + 3u, 4u, 0u, 1u};
        P[4] = AsPatch{hi_at + 3u, 4u, 0u, 1u};
      } else if (lane == 0) atomicAdd(W.counters + AS_BAD_REC, 1ull);
    }
    const auto patched = [&](uint64_t v, uint64_t p, uint32_t nb) {
#pragma unroll
      for (int k = 0; k < 5; k++) v = as_apply(v, p, nb, P[k]);
      return v;
    };
    uint64_t head = (8 - ((uintptr_t)t & 7)) & 7;
    if (head > len) head = len;
    if (lane < head) t[lane] = (uint8_t)patched(s[lane], lane, 1);
    const uint64_t words = (len - head) >> 3;
    const uint8_t *sb = s + head;
    const uint32_t sh = (uint32_t)((uintptr_t)sb & 7) * 8;
    const uint64_t *sa = (const uint64_t *)((uintptr_t)sb & ~(uintptr_t)7);
    uint64_t *ta = (uint64_t *)(t + head);
    for (uint64_t w = lane; w < words; w += G) {
      uint64_t v = __builtin_nontemporal_load(sa + w);
      if (sh) v = v >> sh | __builtin_nontemporal_load(sa + w + 1) << (64 - sh);
      ta[w] = patched(v, head + (w << 3), 8);
    }
    const uint64_t k = head + (words << 3) + lane;   // the tail: below 8 bytes of the record and the tag's 7
    if (k < len) t[k] = (uint8_t)patched(s[k], k, 1);
    else if (k < total) {
      const uint64_t q = k - len;
      t[k] = q == 0 ? (uint8_t)'Z' : q == 1 ? (uint8_t)'W' : q == 2 ? (uint8_t)'f' : (uint8_t)(zw >> (8 * (q - 3)));
    }
    if (lane == 0) { W.row_off[j - W.cur] = d; if (j == W.e - 1) W.row_off[W.e - W.cur] = d + total; }
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
static dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_as_add(hipStream_t st, const AsAddArgs &A) {
  const uint64_t n = A.names.r_last - A.names.r_first;
  if (!n) return;
  hipLaunchKernelGGL(k_as_add, grid_for(n), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_as_place, grid_for(n), dim3(256), 0, st, (const uint4 *)(A.note + A.n0), n, A.counters);
}

void launch_as_finish(hipStream_t st, const AsFinishArgs &F) {
  if (!F.n) return;
  hipLaunchKernelGGL(k_as_p, grid_for(F.n), dim3(256), 0, st, F);
  hipLaunchKernelGGL(k_as_m, grid_for(F.n), dim3(256), 0, st, F);
  const uint64_t big_cap = F.n / (AS_M_LANE_MAX + 1) + 1;
  hipLaunchKernelGGL(k_as_m_big, dim3((unsigned)((big_cap + 3) / 4)), dim3(256), 0, st, F);
  hipLaunchKernelGGL(k_as_w, grid_for(F.n), dim3(256), 0, st, F);
  if (F.mode == 1) hipLaunchKernelGGL(k_as_draw, grid_for(F.n), dim3(256), 0, st, F);
  hipLaunchKernelGGL(k_as_rank, grid_for(F.n), dim3(256), 0, st, (const uint8_t *)F.kept, F.n, F.rank);
}

void launch_as_select(hipStream_t st, const uint8_t *kept, const uint64_t *rank, const uint64_t *off, uint64_t n, uint32_t *sel, uint64_t *out_len) {
  if (n) hipLaunchKernelGGL(k_as_select, grid_for(n), dim3(256), 0, st, kept, rank, off, n, sel, out_len);
}

void launch_as_cut(hipStream_t st, const uint64_t *out_off, uint64_t n_out, uint64_t cur, uint64_t max_bytes, uint64_t *res) {
  hipLaunchKernelGGL(k_as_cut, dim3(1), dim3(1), 0, st, out_off, n_out, cur, max_bytes, res);
}

void launch_as_write(hipStream_t st, const AsWriteArgs &W) {
  const uint64_t n = W.e - W.cur;
  if (!n) return;
  const uint64_t blocks = (n + 256 / AS_WRITE_LANES - 1) / (256 / AS_WRITE_LANES);
  hipLaunchKernelGGL(k_as_write, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, W);
}

}  // namespace br
