// Direct rows: pairing before the emit pass, packed rows written by the emit pass (included by project_kernels.hip).
//
// The two-pass path materialises every surviving (alignment, transcript) match in a 28-byte match table, decides
// pairing on that table, writes a 16-byte record per emitted row and gathers the packed row from both -- 13 GB
// written per 10 M pairs for a 3.5 GB result.  Nothing in process_mate_pair (src/mates.cpp:150-261) needs more than
// the two mates' sets of transcript ids, and the count pass already leaves those (survivor mask + slab rows).  So:
//   k_pair_mask   intersects the mates' survivor sets, keeps a FILTERED mask per alignment and the tid rank of every
//                 kept survivor among the kept (= which record of the leader it becomes: mates.cpp:204-231 walks the
//                 common transcripts in ascending tid order),
//   k_scan5       places the kept matches (work-list position, CIGAR arena slots, rows) in one pass,
//   k_group_desc  NH / HI / primary per read name (src/core.cpp:237-332; all scores tie in these presets),
//   k_emit_rows   one lane per kept match: candidate row -> (walk, merge) -> the 24-byte packed row, in place.
// Presets with the similarity filter (scores decide the primary record) and -S keep the match-table path.
// DirectArgs / PF_* : kernels.h.

#define WAVE_SYNC()                                                \
  do {                                                             \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");         \
    __builtin_amdgcn_wave_barrier();                               \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");         \
  } while (0)

// ---------------------------------------------------------------------------
// k_name_seed: one lane per read name.  get_rand (src/core.cpp:214-218) seeds mt19937_64 with std::hash(name) and
// draws once: 156 dependent 64-bit multiplies that depend on nothing but the name.  The draw's raw 64-bit output is
// kept; the (cheap) reduction to the number of tied units happens in k_group_desc.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_name_seed(DirectArgs D) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= D.n_groups) return;
  const uint32_t a0 = D.group_off[g];
  const uint32_t no = D.name_off[a0];
  Mt64Lazy gen;
  gen.seed(hash_bytes(D.names + no, D.name_off[a0 + 1] - no));
  D.rnd0[g] = gen();
}
// uniform_int_distribution(0, n - 1) on the stored first output; the rejection branch (probability n / 2^64) replays
// the whole generator
__device__ __forceinline__ uint32_t pick_from(uint64_t z0, const uint8_t *name, uint64_t len, uint32_t n) {
  uint64_t hi, lo;
  mul64wide(z0, (uint64_t)n, hi, lo);
  if (lo < (uint64_t)n) {
    const uint64_t thr = (0 - (uint64_t)n) % (uint64_t)n;
    if (lo < thr) return primary_pick(name, len, n);
  }
  return (uint32_t)hi;
}

// ---------------------------------------------------------------------------
// k_pair_mask: a wave per 64 consecutive alignments.
//   role of alignment i (src/core.cpp:384-415 + mates.cpp:153,157,204-245, as k_pair):
//     no survivors                      -> nothing
//     no mutual mate                    -> SOLO: every survivor kept (unpaired emission): the filtered mask is the mask
//     mate without survivors            -> the leader (lower index) is SOLO, the other one emits nothing
//     both with survivors               -> PAIR: kept = transcripts common to both; none common and one transcript
//                                          each -> both kept (a pair on different transcripts); else nothing
// Only PAIRs need transcript ids.  Nearly all of them are settled in registers, as the AND of two 64-bit tid masks (pair_window,
// BM); for the others every lane of a PAIR walks its own mask and stages its survivors' tids (slab rows
// under the set bits) in LDS, a list rounded up to four slots so that lists are read four tids at a time.  The
// intersection is done once per pair, from the ACTIVE side (the leader; or a mate whose leader sits outside the wave's
// window, which then stages a copy of the leader's list next to its own): one lane per active entry scans the partner's
// list, and a hit sets the entry's bit in its own filtered mask and the partner entry's bit in the partner's.  The
// rank of a kept survivor among the kept (= its record) is left to the emit pass, which has the tids at hand.
// A window whose lists exceed the staging area is put on a list for k_pair_mask_wide (the same code, 8192 slots).
// Alignments with > 64 candidate rows (no mask) and their partners are left to k_pair_big.
// ---------------------------------------------------------------------------
#define PM_CAP 768
#define PM_CAP_WIDE 8192   // 64 lists of 64 + 64 copies of outside partners
template <int CAP>
struct PmSh {
  uint32_t tid[CAP] __attribute__((aligned(16)));
  uint8_t bit[CAP], own4[CAP / 4];
  unsigned long long fmask[64];
  uint16_t poff[64];               // where the partner's list starts
  uint8_t pcnt[64], plane[64], same[64], one[64];
};
enum { PR_DEAD = 0, PR_SOLO = 1, PR_PAIR = 2 };

__device__ __forceinline__ uint32_t row_of_bit(uint32_t b, uint32_t lo0, uint32_t lo1, uint32_t n0) { return b < n0 ? lo0 + b : lo1 + (b - n0); }

// eight survivors of a mask at a time: their tids (eight gathers in flight) into slots o..o+7, padding = a tid no transcript
// has; a list takes its length rounded up to four slots
__device__ __forceinline__ void stage_list(const uint32_t *__restrict__ s_tid, uint64_t mm, uint32_t lo0, uint32_t lo1, uint32_t n0,
                                           uint32_t *tid, uint8_t *bit, uint8_t *own4, uint32_t o, uint8_t owner) {
  while (mm) {
    uint32_t b[8], t[8]; bool ok[8];
#pragma unroll
    for (int u = 0; u < 8; u++) { ok[u] = mm != 0; b[u] = ok[u] ? (uint32_t)__builtin_ctzll(mm) : b[0]; mm &= mm - 1; }
#pragma unroll
    for (int u = 0; u < 8; u++) t[u] = s_tid[row_of_bit(b[u], lo0, lo1, n0)];
    *(uint4 *)&tid[o] = make_uint4(t[0], ok[1] ? t[1] : 0xffffffffu, ok[2] ? t[2] : 0xffffffffu, ok[3] ? t[3] : 0xffffffffu);
    *(uint32_t *)&bit[o] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    own4[o >> 2] = owner;
    if (ok[4]) {
      *(uint4 *)&tid[o + 4] = make_uint4(t[4], ok[5] ? t[5] : 0xffffffffu, ok[6] ? t[6] : 0xffffffffu, ok[7] ? t[7] : 0xffffffffu);
      *(uint32_t *)&bit[o + 4] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      own4[(o >> 2) + 1] = owner;
    }
    o += 8;
  }
}

// the next eight survivors of a mask (mm != 0), as stage_list walks them: their tids, eight gathers in flight, and their mask bits,
// a byte each in pb; past the list's end the round's first survivor again, which changes no minimum, maximum or OR.
// c0 / c1: what turns a bit below / from n0 into its slab row (row_of_bit: lo0, lo1 - n0)
__device__ __forceinline__ void tids8(const uint32_t *__restrict__ s_tid, uint64_t &mm, uint32_t c0, uint32_t c1, uint32_t n0,
                                      uint2 &pb, uint32_t (&t)[8]) {
  uint32_t b[8];
#pragma unroll
  for (int u = 0; u < 8; u++) { b[u] = mm ? (uint32_t)__builtin_ctzll(mm) : b[0]; mm &= mm - 1; }
#pragma unroll
  for (int u = 0; u < 8; u++) t[u] = s_tid[b[u] + (b[u] < n0 ? c0 : c1)];
  pb = make_uint2(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24));
}
// a round's tids into the list's tid mask: bit (tid - lo) per survivor, lo = the smallest tid so far -- a round that lowers lo
// moves the mask up.  A list that spans more than 64 tids loses bits here; its hi - lo says so, and the span rule sends it away.
__device__ __forceinline__ void fold8(const uint32_t (&t)[8], uint32_t &lo, uint32_t &hi, uint64_t &tm) {
  uint32_t rlo = t[0], rhi = t[0];
#pragma unroll
  for (int u = 1; u < 8; u++) { rlo = min(rlo, t[u]); rhi = max(rhi, t[u]); }
  const uint32_t nlo = min(lo, rlo), sh = lo - nlo;
  tm = sh > 63u ? 0ull : tm << sh;
  lo = nlo; hi = max(hi, rhi);
#pragma unroll
  for (int u = 0; u < 8; u++) tm |= 1ull << ((t[u] - lo) & 63u);
}

// of a round's survivors (tids t, mask bits pb) the mask bits of those whose tid bit, relative to base, is in common
__device__ __forceinline__ uint64_t keep8(uint2 pb, const uint32_t (&t)[8], uint64_t common, uint32_t base) {
  uint64_t f = 0;
#pragma unroll
  for (int u = 0; u < 8; u++) f |= ((common >> ((t[u] - base) & 63u)) & 1ull) << (((u < 4 ? pb.x : pb.y) >> (8 * (u & 3))) & 63u);
  return f;
}

// the tid word of alignment i (DirectArgs::kt): none -- the emit pass ranks its kept survivors by the loop
__device__ __forceinline__ void kt_none(const DirectArgs &D, uint32_t i) { if (D.kt) D.kt[i] = make_uint4(0u, 0u, KT_NONE, 0u); }

// one window of 64 alignments starting at w0; false: its lists do not fit CAP slots (nothing of the list path's PAIRs was written)
// Lanes 1..62 own their alignments; lanes 0 and 63 are the neighbours on either side, loaded and staged like the others so
// that a pair that straddles two waves' ranges (mates are neighbours as a rule) finds its partner inside the window; they
// write nothing.  Partners further apart than that are copied next to the lane that needs them.
// BM (br_ctx_set_param "pair_bitmask"): a pair whose partner is inside the window and whose two lists together span at most 64
// tids -- transcripts are numbered in location order, so that is nearly every pair -- never reaches the lists: each lane
// folds its tids into a 64-bit mask relative to the pair's smallest tid, and the intersection is one AND.  What the rule turns
// away takes the list path below, with the same results: how transcripts are numbered decides the speed and nothing else.
// The tid word (D.kt, null with "emit_rank_tids" 0): a pair on the mask path with a common transcript keeps exactly the common
// tids on both sides, so {common, base} IS the sorted list of an alignment's kept tids, and the emit lanes take a record's
// rank from it with one population count instead of gathering the kept survivors' tids again.  Every place that writes fm[i]
// writes kt[i] too -- the word, or the marker KT_NONE -- so no emit lane ever meets a word of an earlier call.
template <int CAP, bool BM>
__device__ __forceinline__ bool pair_window(const DirectArgs &D, PmSh<CAP> &S, int64_t w0, int lane) {
  const int64_t i64 = w0 + lane;
  const bool valid = i64 >= 0 && i64 < D.n_aln;
  const bool owner = valid && lane >= 1 && lane <= 62;
  const uint32_t i = (uint32_t)i64;
  uint32_t nm = 0, g = 0; uint64_t mk = 0; uint4 rg = make_uint4(0, 0, 0, 0); int32_t m = -1;
  if (valid) { nm = D.n_matches[i]; mk = D.mask[i]; rg = D.ranges[i]; m = D.mate_idx[i]; g = D.aln_group[i]; }
  const uint32_t n0 = rg.y - rg.x;
  const bool big = nm != 0 && (n0 + (rg.w - rg.z)) > 64u;
  // the partner: a mutual mate pointer inside the same read name
  const bool has_m = valid && m >= 0 && (int64_t)m < D.n_aln && (uint32_t)m != i;
  const int ml = has_m ? (int)((int64_t)m - w0) : -1;
  const bool m_in = ml >= 0 && ml < 64;
  const int src = m_in ? ml : lane;
  uint32_t g_m = __shfl(g, src), nm_m = __shfl(nm, src), big_m = __shfl((uint32_t)big, src);
  int32_t m_m = __shfl(m, src);
  uint64_t mk_p = 0; uint4 rg_p = make_uint4(0, 0, 0, 0);   // a partner outside the window
  if (has_m && !m_in && owner) {
    g_m = D.aln_group[m]; m_m = D.mate_idx[m]; nm_m = D.n_matches[m]; mk_p = D.mask[m]; rg_p = D.ranges[m];
    big_m = (nm_m != 0 && ((rg_p.y - rg_p.x) + (rg_p.w - rg_p.z)) > 64u) ? 1u : 0u;
  }
  const bool mutual = has_m && g_m == g && m_m == (int32_t)i;
  const bool leader = !mutual || i < (uint32_t)m;
  int role = PR_DEAD;
  if (nm) { if (!mutual) role = PR_SOLO; else if (nm_m == 0) role = leader ? PR_SOLO : PR_DEAD; else role = PR_PAIR; }
  const bool defer = role != PR_DEAD && (big || (role == PR_PAIR && big_m));   // k_pair_big's
  const uint32_t cnt = (uint32_t)__popcll(mk);   // (= nm for an alignment with a mask)
  if (owner && !defer && role != PR_PAIR) {
    const bool solo = role == PR_SOLO;
    D.fm[i] = solo ? make_uint2((uint32_t)mk, (uint32_t)(mk >> 32)) : make_uint2(0, 0);
    D.n_kept[i] = solo ? cnt : 0u; D.n_rows[i] = solo ? cnt : 0u; D.pflag[i] = 0;
    kt_none(D, i);
  }
  // (a neighbour lane takes part only for a partner inside the window)
  bool pair = role == PR_PAIR && !defer && (owner || m_in);
  if (!__ballot(pair && owner)) return true;
  uint64_t on_list = 0;   // (BM) the owners the list path resolves
  if (BM) {
    const bool mp = pair && m_in;   // (the partner's lane reaches the same verdicts: every test here is symmetric)
    uint32_t t0[8], t1[8], lo = 0xffffffffu, hi = 0;
    uint2 pb0, pb1, pb;
    const uint32_t c0 = rg.x, c1 = rg.z - n0;
    uint64_t tm = 0, mm = mp ? mk : 0;
    // The kernel runs at full occupancy and waits: what it costs is the number of dependent round trips a wave makes.  So the
    // first two rounds of eight (97 % of the bench's lists are within them) are asked for together, the second one skipped
    // wave-uniformly when no lane has that many, and their 16 tids stay in registers for the pass over the survivors below.
    // (A third round in the same trip takes 65 VGPRs.)  The rounds leave their mask bits packed a byte each (pb): the pass over
    // the survivors reads them with one bit-field extract where finding them again costs eight 64-bit operations each, and the
    // kernel, once it waits less, is bound by what it issues.
    const bool any2 = __ballot(mp && cnt > 8u) != 0;
    if (mm) tids8(D.s_tid, mm, c0, c1, n0, pb0, t0);
    if (any2 && mm) tids8(D.s_tid, mm, c0, c1, n0, pb1, t1);
    if (mp) fold8(t0, lo, hi, tm);
    if (mp && cnt > 8u) fold8(t1, lo, hi, tm);
    while (mm) { uint32_t t[8]; tids8(D.s_tid, mm, c0, c1, n0, pb, t); fold8(t, lo, hi, tm); }
    const uint32_t lo_p = __shfl(lo, src), hi_p = __shfl(hi, src), cnt_p = __shfl(cnt, src);
    const uint32_t base = min(lo, lo_p);
    const bool fits = mp && max(hi, hi_p) - base <= 63u;   // the span rule
    const uint64_t tmb = fits ? tm << (lo - base) : 0ull;
    const uint64_t common = tmb & __shfl((unsigned long long)tmb, src);
    if (fits) {
      uint64_t fmask = mk;   // every survivor is common: the usual case
      if (common == 0) fmask = (cnt == 1u && cnt_p == 1u) ? mk : 0ull;   // a pair on different transcripts, or nothing
      else if (common != tmb) {   // the survivors whose tid bit is common: the first 16 from registers, the others gathered again (L1 hits)
        fmask = keep8(pb0, t0, common, base);
        if (cnt > 8u) fmask |= keep8(pb1, t1, common, base);
        if (cnt > 16u) {
          mm = mk;
          for (int u = 0; u < 16; u++) mm &= mm - 1;
          while (mm) { uint32_t t[8]; tids8(D.s_tid, mm, c0, c1, n0, pb, t); fmask |= keep8(pb, t, common, base); }
        }
      }
      if (owner) {
        const uint32_t nk = (uint32_t)__popcll(fmask);
        const bool paired = nk != 0;
        D.fm[i] = make_uint2((uint32_t)fmask, (uint32_t)(fmask >> 32));
        D.n_kept[i] = nk;
        D.n_rows[i] = leader ? 2u * nk : 0u;
        D.pflag[i] = (uint8_t)((paired ? PF_PAIRED : 0u) | ((paired && common != 0) ? PF_SAME : 0u) | ((paired && !leader) ? PF_MATE : 0u));
        // the kept survivors' tids are exactly the common ones: the emit pass ranks a survivor by counting common's bits below its own
        if (D.kt) D.kt[i] = make_uint4((uint32_t)common, (uint32_t)(common >> 32), common ? base : KT_NONE, 0u);
      }
    }
    // the list path: what the span rule turned away, and partners outside the window
    pair = pair && !fits;
    on_list = __ballot(pair && owner);
    if (!on_list) return true;
  }
  const bool active = pair && (leader || !m_in);
  const uint32_t cnt4 = (cnt + 3u) & ~3u;
  const uint32_t ext = (active && !m_in) ? (uint32_t)__popcll(mk_p) : 0u;
  const uint32_t nA = active ? cnt4 : 0u, nP = (pair && !active ? cnt4 : 0u) + ((ext + 3u) & ~3u);
  // (the two scans share their shuffles' waits; two wave_scan calls cost k_pair_mask two SGPRs)
  uint32_t incA = nA, incP = nP;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t ua = __shfl_up(incA, d), up = __shfl_up(incP, d); if (lane >= d) { incA += ua; incP += up; } }
  const uint32_t TA = __shfl(incA, 63), TP = __shfl(incP, 63);
  if (TA + TP > (uint32_t)CAP) return false;
  const uint32_t o_own = active ? incA - nA : TA + incP - nP;   // this lane's own list
  const uint32_t o_ext = TA + incP - nP;                         // (active lanes only: the copy of an outside partner)
  const uint32_t p_off = __shfl(o_own, src), p_cnt = __shfl(cnt, src);
  if (pair) {
    S.poff[lane] = (uint16_t)(m_in ? p_off : o_ext); S.pcnt[lane] = (uint8_t)(m_in ? p_cnt : ext);
    S.plane[lane] = (uint8_t)(m_in ? ml : 0xff); S.one[lane] = (cnt == 1u && (m_in ? p_cnt : ext) == 1u) ? 1 : 0;
  }
  S.fmask[lane] = 0; S.same[lane] = 0;
  if (pair) {
    stage_list(D.s_tid, mk, rg.x, rg.z, n0, S.tid, S.bit, S.own4, o_own, (uint8_t)lane);
    if (ext) stage_list(D.s_tid, mk_p, rg_p.x, rg_p.z, rg_p.y - rg_p.x, S.tid, S.bit, S.own4, o_ext, 0xff);
  }
  WAVE_SYNC();
  for (uint32_t e = lane; e < TA; e += 64) {   // the active lists
    const uint32_t t = S.tid[e];
    if (t == 0xffffffffu) continue;   // padding
    const uint32_t l = S.own4[e >> 2];
    const uint32_t p0 = S.poff[l], pe = p0 + S.pcnt[l];
    uint32_t y = 0xffffffffu;          // the partner's entry with the same tid (tids of a list are distinct)
    for (uint32_t x = p0; x < pe; x += 4) {
      const uint4 v = *(const uint4 *)&S.tid[x];
      y = v.x == t ? x : v.y == t ? x + 1 : v.z == t ? x + 2 : v.w == t ? x + 3 : y;
    }
    const bool found = y != 0xffffffffu;
    if (!found && !S.one[l]) continue;
    const uint32_t pl = S.plane[l];
    atomicOr(&S.fmask[l], 1ull << S.bit[e]);
    if (pl != 0xffu) atomicOr(&S.fmask[pl], 1ull << S.bit[found ? y : p0]);
    if (found) { S.same[l] = 1; if (pl != 0xffu) S.same[pl] = 1; }
  }
  WAVE_SYNC();
  if (pair && owner) {
    const uint64_t fmask = S.fmask[lane];
    const uint32_t nk = (uint32_t)__popcll(fmask);
    const bool paired = nk != 0;
    D.fm[i] = make_uint2((uint32_t)fmask, (uint32_t)(fmask >> 32));
    D.n_kept[i] = nk;
    D.n_rows[i] = leader ? 2u * nk : 0u;
    D.pflag[i] = (uint8_t)((paired ? PF_PAIRED : 0u) | ((paired && S.same[lane]) ? PF_SAME : 0u) | ((paired && !leader) ? PF_MATE : 0u));
    kt_none(D, i);
  }
  // br_ctx_direct_diag: the alignments the lists resolved, one atomic per wave that has any, spread like k_group_desc's
  if (BM && lane == 0)
    atomicAdd((unsigned long long *)&D.counters[GD_SLOT0 + (size_t)((uint64_t)(w0 + 1) / 62u & (GD_SLOTS - 1)) * GD_SLOT_STRIDE + PM_SLOT_WORD],
              (unsigned long long)__popcll(on_list));
  return true;
}

template <bool BM>
__global__ void __launch_bounds__(256) k_pair_mask(DirectArgs D) {
  __shared__ PmSh<PM_CAP> sh_all[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wi = (int64_t)blockIdx.x * 4 + wv;   // window: alignments 62 * wi .. 62 * wi + 61 (+ a neighbour on either side)
  const int64_t w0 = wi * 62 - 1;
  if (w0 + 1 >= D.n_aln) return;   // the whole wave
  if (!pair_window<PM_CAP, BM>(D, sh_all[wv], w0, lane) && lane == 0) D.pm_list[atomicAdd(D.pm_n, 1u)] = (uint32_t)wi;
}
template <bool BM>
__global__ void __launch_bounds__(64) k_pair_mask_wide(DirectArgs D) {
  __shared__ PmSh<PM_CAP_WIDE> sh;
  const uint32_t n_work = *D.pm_n;
  for (uint32_t q = blockIdx.x; q < n_work; q += gridDim.x) {
    (void)pair_window<PM_CAP_WIDE, BM>(D, sh, (int64_t)D.pm_list[q] * 62 - 1, (int)threadIdx.x);
    WAVE_SYNC();
  }
}

// The packed row of a kept match (what k_rows made of r_rec + the match record): E = the alignment's descriptor
// {PF_* | (primary rank + 1) << 8, NH, first record, -}, c = the match's rank among the alignment's kept ones.
__device__ __forceinline__ void write_row(const DirectArgs &D, const uint4 E, uint32_t a, uint32_t c, uint32_t tid, uint32_t pos,
                                          uint32_t n_out, bool minus, uint64_t cig_ref, uint32_t junc, uint32_t refc) {
  const uint32_t fl = E.x & 0xffu, prim = E.x >> 8;
  const uint32_t stride = (fl & PF_PAIRED) ? 2u : 1u;
  const uint64_t r = (uint64_t)E.z + (uint64_t)stride * c;
  if (n_out > RM_NCIG) D.counters[3] = 1;
  const uint32_t meta = (n_out & RM_NCIG) | (minus ? RM_MINUS : 0u) | ((fl & PF_PAIRED) ? RM_PAIRED : 0u) | ((fl & PF_SAME) ? RM_SAME : 0u) |
                        ((fl & PF_MATE) ? 0u : RM_FIRST) | (prim == c + 1u ? RM_PRIMARY : 0u);
  // the rows are the step's result: written once, read by nobody before the step ends -- streaming stores, so that they do
  // not push the index rows and the emit pass's own inputs out of L2 (k_emit_rows<1> 1.32 -> 1.22 ms, <2> 1.81 -> 1.72)
  typedef uint32_t nt4 __attribute__((ext_vector_type(4)));
  typedef uint32_t nt2 __attribute__((ext_vector_type(2)));
  const nt4 va = {tid, pos, meta, E.y};
  const nt2 vc = {(uint32_t)cig_ref, (uint32_t)(cig_ref >> 32)};
  __builtin_nontemporal_store(va, (nt4 *)(D.r_a + r));
  __builtin_nontemporal_store(vc, (nt2 *)(D.r_c + r));
  if (D.r_x) { const nt4 vx = {a, junc, refc, D.hi0[a] + stride * c}; __builtin_nontemporal_store(vx, (nt4 *)(D.r_x + r)); }
}


// ---------------------------------------------------------------------------
// Alignments with more than 64 candidate rows (big_list; a few per thousand at dense loci).  k_big<0> walks the
// candidates once more and leaves the survivors' tids in the side arena, k_pair_big does k_pair_mask's work on those
// lists (and for a partner with a mask), k_big<1> emits the kept ones.
// ---------------------------------------------------------------------------
// Side arena of a big alignment with nb survivors, in 8-byte units: X = {tid, rank | ~0u} per survivor, then K = the kept
// tids, compact (k_pair_big's scratch).  Both are padded to whole 128-byte lines, so that no line is shared between
// two alignments: what one wave writes and reads back is never in another line's stale copy of some L1.
__device__ __forceinline__ unsigned long long side_need(uint32_t nb) {
  const unsigned long long x = ((unsigned long long)nb + 15ull) & ~15ull, k = (((unsigned long long)nb + 1ull) / 2ull + 15ull) & ~15ull;
  return x + k;
}
template <int EM>
__global__ void __launch_bounds__(64) k_big(ProjectArgs A, DirectArgs D) {
  __shared__ uint32_t sh_cig[EM ? 64 * LDS_SLOT : 1];
  __shared__ uint16_t sh_mops[EM ? 256 : 1];
  const int lane = threadIdx.x;
  if (EM) {
    for (int t = lane; t < 256; t += 64) sh_mops[t] = (uint16_t)((merge_action(t >> 4, t & 15u) << 8) | merge_ops(t >> 4, t & 15u));
    WAVE_SYNC();
  }
  const DevIndex &ix = A.ix;
  const DevCfg &cfg = A.cfg;
  const uint32_t n_work = *D.n_big;
  for (uint32_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    if (D.side_used[1]) {   // the arena ran out: the host grows it and repeats
      if (EM) return;
      // no walk and no write from here on, but the need of every entry this block has left still counts (it depends on
      // n_matches alone), so that side_used[0] ends as the exact total and the repeat's arena holds it: lane l adds up the
      // entries w + (l + 64 k) * gridDim.x, one atomic per wave
      unsigned long long need = 0;
      for (uint64_t v = (uint64_t)w + (uint64_t)lane * gridDim.x; v < n_work; v += 64ull * gridDim.x) need += side_need(D.n_matches[D.big_list[v]]);
      need = wave_sum(need);
      if (lane == 0 && need) atomicAdd(D.side_used, need);
      return;
    }
    const uint32_t a = D.big_list[w];
    const uint32_t nm = D.n_matches[a];
    if (EM && D.n_kept[a] == 0) continue;
    const uint4 hd = A.head[a], hd2 = A.head2[a], rg = A.ranges[a];
    const uint32_t n_seg = hd.z, rid = hd.w >> 2;
    if (n_seg == 0 || nm == 0) continue;
    const uint2 q0 = make_uint2(hd.x, hd.y);
    const int st0 = (n_seg == 1) ? ST_ONLY : ST_FIRST;
    const uint32_t sb[2] = {ix.slab_off[2 * rid], ix.slab_off[2 * rid + 1]}, se[2] = {ix.slab_off[2 * rid + 1], ix.slab_off[2 * rid + 2]};
    const uint32_t n0 = rg.y - rg.x, n_items = n0 + (rg.w - rg.z);
    unsigned long long off = 0;
    uint4 E = make_uint4(0, 0, 0, 0);
    if (!EM) {
      const unsigned long long need = side_need(nm);
      if (lane == 0) off = atomicAdd(D.side_used, need);
      off = ((unsigned long long)__shfl((uint32_t)(off >> 32), 0) << 32) | __shfl((uint32_t)off, 0);
      if (off + need > D.side_cap) { if (lane == 0) D.side_used[1] = 1; continue; }
      if (lane == 0) D.fm[a] = make_uint2((uint32_t)off, (uint32_t)(off >> 32));
    } else {
      const uint2 f = D.fm[a];
      off = (unsigned long long)f.x | ((unsigned long long)f.y << 32);
      { const uint2 gd = D.gd[a], dp = D.dpos[a]; E = make_uint4(gd.x, gd.y, dp.x, dp.y); }
    }
    const uint32_t c0 = A.cigar_off[a];
    ReadCtx rd;
    rd.n_seg = n_seg; rd.seg = A.seg + (size_t)c0 + (size_t)a; rd.real = A.cigar + c0; rd.n_real = A.cigar_off[a + 1] - c0; rd.q12 = hd2;
    uint32_t seen = 0;
    for (uint32_t base = 0; base < n_items; base += 64) {
      const uint32_t item = base + (uint32_t)lane;
      bool alive = false;
      int s = 0; uint32_t gs = 0, gend = 0, nxt = 0, nxe = 0;
      uint4 pay = make_uint4(0xffffffffu, 0, 0, 0);
      Hit h0; CandOut p1; const uint4 *Ex = nullptr; uint32_t i0 = 0;
      p1.alive = false; p1.fwpos = 0; p1.rcpos = 0; p1.n_seg = 0; p1.n_gex = 0; p1.i_lastm = 0; p1.last_right_ins = 0; p1.last_right_gap = 0;
      h0.pos = 0; h0.left_ins = h0.right_ins = h0.left_gap = h0.right_gap = 0;
      if (item < n_items) {
        s = item < n0 ? 0 : 1;
        const uint32_t row = s == 0 ? rg.x + item : rg.z + (item - n0);
        const uint4 r_a = ix.s_row[2 * (size_t)row], r_b = ix.s_row[2 * (size_t)row + 1];
        gs = r_a.x; gend = r_a.y; nxt = r_a.z; nxe = r_b.w; pay = make_uint4(r_b.x, r_b.y, r_a.w, r_b.z);
        if (gend > q0.x && gs < q0.y && classify(s == 1, st0, q0.x, q0.y, gs, gend, pay.z, cfg, h0)) {
          Ex = ix.tx_ex + pay.w; i0 = pay.y & 0x7fffffffu;
          bool superseded = false;   // first-exon duplicate tid: the last passing row wins (src/evaluate.cpp:218-224)
          if (nxt < q0.y) {
            for (uint32_t q = i0 + 1;; q++) {
              const uint4 e = Ex[q];
              if (e.x >= q0.y) break;
              Hit hx;
              if (e.y > q0.x && classify(s == 1, st0, q0.x, q0.y, e.x, e.y, e.z, cfg, hx)) { superseded = true; break; }
            }
          }
          if (!superseded) {
            if (n_seg == 1) { p1.alive = true; p1.fwpos = h0.pos; p1.rcpos = h0.pos; p1.n_seg = 1; p1.n_gex = 1; p1.i_lastm = i0; p1.last_right_ins = h0.right_ins; p1.last_right_gap = h0.right_gap; }
            else p1 = walk_pass1(ix, cfg, rd, Ex, s == 1, sb[s], se[s], i0, make_uint4(gs, gend, pay.z, 0), make_uint2(nxt, nxe), q0, h0);
            alive = p1.alive;
          }
        }
      }
      const uint64_t bm = __ballot(alive);
      const uint32_t k = seen + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      seen += (uint32_t)__popcll(bm);
      if (!alive || k >= nm) continue;
      if (!EM) { D.side[off + k] = make_uint2(pay.x, 0u); continue; }
      const uint32_t c = D.side[off + k].y;
      if (c == 0xffffffffu) continue;   // dropped by the pairing
      const uint32_t ideal_cap = 4u * n_seg + 2u, cap = rd.n_real + 2u * ideal_cap;
      const uint64_t slot_off = D.cig_base[a] + (uint64_t)c * cap;
      uint32_t *slot = A.cig_arena + slot_off;
      uint32_t *lds = &sh_cig[(EM ? lane : 0) * LDS_SLOT];
      const bool ideal_lds = ideal_cap <= LDS_IDEAL;
      uint32_t *ideal = ideal_lds ? lds : slot + rd.n_real + ideal_cap;
      Acc acc; IdealSink sk;
      sk.init(ideal);
      walk_pass2(ix, cfg, rd, Ex, s == 1, sb[s], se[s], i0, q0, make_uint4(gs, gend, pay.z, 0), make_uint2(nxt, nxe), h0, p1, acc, sk, no_clip(), no_clip());
      const uint32_t n_ideal = sk.finish();
      const bool out_lds = ideal_lds && (rd.n_real + n_ideal <= LDS_SLOT - LDS_IDEAL);
      uint32_t *outp = out_lds ? lds + LDS_IDEAL : slot;
      RealCig rc; rc.fetch(rd.real, rd.n_real);
      const uint32_t n_out = merge_cigars(rc, rd.n_real, ideal, n_ideal, outp, sh_mops);
      uint64_t cig_ref = slot_off;
      if (n_out <= 2) cig_ref = (uint64_t)(n_out > 0 ? outp[0] : 0u) | ((uint64_t)(n_out > 1 ? outp[1] : 0u) << 32);
      else if (out_lds) for (uint32_t q = 0; q < n_out; q++) slot[q] = outp[q];
      write_row(D, E, a, c, pay.x, (s == 0) ? p1.fwpos : p1.rcpos, n_out, s == 1, cig_ref, (uint32_t)acc.junc_hits, (uint32_t)acc.ref_consumed);
    }
  }
}

// k_pair_big: a wave per big_list entry b.  X = b's survivors in the side arena, Y = its partner's (side arena, or the
// <= 64 tids under its mask, staged in LDS).  Writes b's outputs, and the partner's when the partner has a mask (a big
// partner is its own entry).
__global__ void __launch_bounds__(64) k_pair_big(DirectArgs D) {
  __shared__ uint32_t sh_y[64];
  __shared__ unsigned long long sh_f[2];
  const int lane = threadIdx.x;
  const uint32_t n_work = *D.n_big;
  for (uint32_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    if (D.side_used[1]) return;
    const uint32_t b = D.big_list[w];
    const uint32_t nb = D.n_matches[b];
    const int32_t m = D.mate_idx[b];
    const uint2 fb = D.fm[b];
    uint2 *X = D.side + ((unsigned long long)fb.x | ((unsigned long long)fb.y << 32));
    bool mutual = false; uint32_t np = 0; bool p_big = false; uint4 rp = make_uint4(0, 0, 0, 0);
    if (m >= 0 && (int64_t)m < D.n_aln && (uint32_t)m != b) {
      mutual = D.aln_group[m] == D.aln_group[b] && D.mate_idx[m] == (int32_t)b;
      if (mutual) { np = D.n_matches[m]; rp = D.ranges[m]; p_big = np != 0 && ((rp.y - rp.x) + (rp.w - rp.z)) > 64u; }
    }
    const bool leader = !mutual || b < (uint32_t)m;
    int role = PR_DEAD;
    if (nb) { if (!mutual) role = PR_SOLO; else if (np == 0) role = leader ? PR_SOLO : PR_DEAD; else role = PR_PAIR; }
    if (role == PR_DEAD) continue;   // (k_pair_mask wrote its zeros)
    const uint2 *Y = nullptr;
    uint64_t pmask = 0;
    uint32_t y_tid = 0, y_bit = 0;
    __builtin_amdgcn_wave_barrier();
    if (role == PR_PAIR) {
      if (p_big) { const uint2 fp = D.fm[m]; Y = D.side + ((unsigned long long)fp.x | ((unsigned long long)fp.y << 32)); }
      else {
        pmask = D.mask[m];
        if ((uint32_t)lane < np) {
          y_bit = kth_set_bit64(pmask, (uint32_t)lane);
          y_tid = D.s_tid[row_of_bit(y_bit, rp.x, rp.z, rp.y - rp.x)];
        }
        sh_y[lane] = y_tid;
      }
    }
    if (lane < 2) sh_f[lane] = 0;
    WAVE_SYNC();
    const bool one_each = nb == 1u && np == 1u;
    // 1. kept?  X[e].y: 0 kept, ~0u dropped; the kept tids go to K, compact (a round's kept ones by ballot rank)
    uint32_t *K = (uint32_t *)(X + (((unsigned long long)nb + 15ull) & ~15ull));
    bool any_found = false;
    uint32_t nk = 0;
    for (uint32_t e0 = 0; e0 < nb; e0 += 64) {
      const uint32_t e = e0 + lane;
      bool keep = false;
      uint32_t t = 0;
      if (e < nb) {
        keep = true;
        t = X[e].x;
        if (role == PR_PAIR) {
          bool found = false;
          if (Y) { for (uint32_t j = 0; j < np; j++) found |= Y[j].x == t; }
          else { for (uint32_t j = 0; j < np; j++) found |= sh_y[j] == t; }
          keep = found || one_each;
          any_found |= found;
        }
        X[e].y = keep ? 0u : 0xffffffffu;
      }
      const uint64_t km = __ballot(keep);
      if (keep) K[nk + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))] = t;
      nk += (uint32_t)__popcll(km);
    }
    const bool same = __ballot(any_found) != 0;
    WAVE_SYNC();   // K is complete (its lines were never read before: private to this alignment, see side_need)
    // 2. rank among the kept; a lane reads back only its own flag
    for (uint32_t e = lane; e < nb; e += 64) {
      if (X[e].y == 0xffffffffu) continue;
      const uint32_t t = X[e].x;
      uint32_t c = 0;
      for (uint32_t x = 0; x < nk; x++) c += K[x] < t ? 1u : 0u;
      X[e].y = c;
    }
    const bool paired = role == PR_PAIR && nk != 0;
    if (lane == 0) {
      D.n_kept[b] = nk;
      D.n_rows[b] = leader ? (paired ? 2u * nk : nk) : 0u;
      D.pflag[b] = (uint8_t)(PF_BIG | (paired ? PF_PAIRED : 0u) | ((paired && same) ? PF_SAME : 0u) | ((paired && !leader) ? PF_MATE : 0u));
    }
    // the partner with a mask: lane k holds the tid under its k-th set bit
    if (role == PR_PAIR && !p_big) {
      bool keep = false;
      if ((uint32_t)lane < np) {
        bool found = false;
        for (uint32_t x = 0; x < nb; x++) found |= X[x].x == y_tid;
        keep = found || one_each;
      }
      const uint64_t km = __ballot(keep);
      if (keep) {
        atomicOr(&sh_f[0], 1ull << y_bit);
      }
      WAVE_SYNC();
      if (lane == 0) {
        const uint64_t fmask = sh_f[0];
        const uint32_t nkp = (uint32_t)__popcll(km);
        const bool pp = nkp != 0;
        D.fm[m] = make_uint2((uint32_t)fmask, (uint32_t)(fmask >> 32));
        D.n_kept[m] = nkp;
        D.n_rows[m] = leader ? 0u : (pp ? 2u * nkp : 0u);   // the partner leads when b does not
        D.pflag[m] = (uint8_t)((pp ? PF_PAIRED : 0u) | ((pp && same) ? PF_SAME : 0u) | ((pp && leader) ? PF_MATE : 0u));
        kt_none(D, (uint32_t)m);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------
// k_scan5: per alignment (kept, kept x CIGAR slot capacity, kept of the simple class, records of a leader, survivors)
// -> class-list position (u32), arena base (u64), row offset (u64) + the five totals.
// ---------------------------------------------------------------------------
struct Scan5 { uint64_t v[5]; };
template <bool RAW>   // RAW: the survivors too (their total only: the tile pass)
__device__ __forceinline__ void scan5_load(const DirectArgs &D, int64_t base, Scan5 v[SCAN_ITEMS]) {
  uint32_t nk[SCAN_ITEMS], cf[SCAN_ITEMS], nr[SCAN_ITEMS], nm[SCAN_ITEMS];
  load8(D.n_kept, base, D.n_aln, nk); load8(D.fast_flag, base, D.n_aln, cf); load8(D.n_rows, base, D.n_aln, nr);
  if (RAW) load8(D.n_matches, base, D.n_aln, nm);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    v[k].v[0] = nk[k]; v[k].v[1] = (uint64_t)nk[k] * (uint64_t)(cf[k] & 0x7fffffffu); v[k].v[2] = (cf[k] >> 31) ? nk[k] : 0;
    v[k].v[3] = nr[k]; v[k].v[4] = RAW ? nm[k] : 0u;
  }
}
__global__ void __launch_bounds__(256) k_scan5_tiles(DirectArgs D, uint64_t *tile_sums, int64_t n_tiles) {
  __shared__ uint64_t sh[4][5];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint64_t sum[5] = {0, 0, 0, 0, 0};
  Scan5 v[SCAN_ITEMS];
  scan5_load<true>(D, base, v);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++)
#pragma unroll
    for (int c = 0; c < 5; c++) sum[c] += v[k].v[c];
  // sums only (no prefixes here): wave reductions, one barrier
#pragma unroll
  for (int c = 0; c < 5; c++)
    sum[c] = wave_sum(sum[c]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 5; c++) sh[threadIdx.x >> 6][c] = sum[c];
  }
  __syncthreads();
  if (threadIdx.x < 5) tile_sums[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}
// One block per quantity, SCAN5_TOP_ITEMS tile sums per thread and round.  Alone, the 10 206 sums of a quantity of the bench
// step take 13 us with 8 sums per thread (58 VGPRs), 15 with 16, 22 with 32 (155 VGPRs) and 18 with 64; on the step's path
// the kernel takes 0.12 ms whatever the shape.  Not for want of wave slots (with k_group_desc at 1 792 blocks, a slot per
// SIMD free, it took as long): k_group_desc keeps 8 192 waves of scattered loads and stores in flight on the second stream,
// and every dependent round trip of the one-block scan queues behind them in the memory system (DESIGN 10.1, row 26).
constexpr int SCAN5_TOP_ITEMS = 8;
__global__ void __launch_bounds__(256) k_scan5_top(uint64_t *tile_sums, int64_t n_tiles, uint64_t *total_out) {
  __shared__ uint64_t sh[4];
  scan_top_rounds<1, SCAN5_TOP_ITEMS>(tile_sums + (int64_t)blockIdx.x * n_tiles, n_tiles, total_out + blockIdx.x, sh);
}
__global__ void __launch_bounds__(256) k_scan5_apply(DirectArgs D, const uint64_t *tile_sums, int64_t n_tiles, const uint64_t *totals) {
  __shared__ uint64_t sh[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  Scan5 v[SCAN_ITEMS];
  uint64_t sum[4] = {0, 0, 0, 0};
  scan5_load<false>(D, base, v);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++)
#pragma unroll
    for (int c = 0; c < 4; c++) sum[c] += v[k].v[c];
  uint64_t ex[4];
#pragma unroll
  for (int c = 0; c < 4; c++) { uint64_t tot; ex[c] = block_excl_scan_256(sum[c], sh, tot) + tile_sums[(int64_t)c * n_tiles + blockIdx.x]; }
  const uint32_t n_simple = (uint32_t)totals[2];   // the general class follows the simple one in the work list
  uint32_t o0[SCAN_ITEMS]; uint64_t o1[SCAN_ITEMS], o3[SCAN_ITEMS];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; k++) {
    o0[k] = v[k].v[2] ? (uint32_t)ex[2] : n_simple + (uint32_t)(ex[0] - ex[2]);
    o1[k] = ex[1]; o3[k] = ex[3];
#pragma unroll
    for (int c = 0; c < 4; c++) ex[c] += v[k].v[c];
  }
  store8(D.cls_pos, base, D.n_aln, o0); store8(D.cig_base, base, D.n_aln, o1); store8(D.row_off, base, D.n_aln, o3);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) { D.cig_base[D.n_aln] = ex[1]; D.row_off[D.n_aln] = ex[3]; }
}

// ---------------------------------------------------------------------------
// k_group_desc: one lane per read name.  NH = records of the name (flush, src/core.cpp:250-258), HI = 1-based rank among
// them (:309-325); every emitted unit ties for primary (no similarity filter: all scores 0.0), so the choice is
// get_rand(units, hash(name)) (:283-303) -- the unit's leader and its rank there.  Leaves descriptor words .x (PF_* |
// (primary rank + 1) << 8) and .y (NH) and the first HI of every emitting alignment; the counters of
// src/bramble.cpp:729-736.
// ---------------------------------------------------------------------------
// (A read name's alignments are neighbours, so a name of at most four -- a pair, as a rule -- takes its rows, flags,
// survivor counts and mate indices with one vector load each right behind group_off, all in flight together, and a mate
// inside the group is looked up in those registers: two dependent round trips per name instead of five.  The name itself
// is only read when the draw's rejection branch needs it.)
struct __attribute__((packed, aligned(4))) GD4 { uint32_t a, b, c, d; };
__global__ void __launch_bounds__(256) k_group_desc(DirectArgs D) {
  // The side arena ran out: k_pair_big left the outputs of the > 64-candidate alignments (and of their partners) unwritten,
  // so rows, flags and mate links are not to be trusted -- a stale PF_PAIRED on an unpaired alignment sends the mate write
  // to gd[-1].  The host grows the arena and repeats; nothing here is used.
  if (D.side_used[1]) return;
  unsigned long long uniq = 0, dropped = 0;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < D.n_groups; g += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t a0 = D.group_off[g], a1 = D.group_off[g + 1];
    const uint32_t na = a1 - a0;
    uint32_t total = 0, units = 0, any = 0;
    uint32_t r4[4] = {0, 0, 0, 0}, f4[4] = {0, 0, 0, 0};
    int32_t mi4[4] = {-1, -1, -1, -1};
    const bool small = na <= 4u;
    // (the vector loads may reach three elements past the last alignment: the context's arrays have that room; the caller's
    // mate_idx is read element by element)
    if (small) {
      const GD4 rr = *(const GD4 *)(D.n_rows + a0), mm = *(const GD4 *)(D.n_matches + a0);
      typedef uint32_t u32u1 __attribute__((aligned(1)));
      const uint32_t ff = *(const u32u1 *)(D.pflag + a0);
#pragma unroll
      for (int k = 0; k < 4; k++) mi4[k] = (uint32_t)k < na ? D.mate_idx[a0 + (uint32_t)k] : -1;
      r4[0] = rr.a; r4[1] = rr.b; r4[2] = rr.c; r4[3] = rr.d;
      uint32_t m4[4] = {mm.a, mm.b, mm.c, mm.d};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        f4[k] = (ff >> (8 * k)) & 0xffu;
        if ((uint32_t)k >= na) { r4[k] = 0; m4[k] = 0; f4[k] = 0; }
        total += r4[k]; units += (f4[k] & PF_PAIRED) ? r4[k] / 2 : r4[k]; any |= m4[k];
      }
    } else {
      for (uint32_t i = a0; i < a1; i++) { const uint32_t r = D.n_rows[i]; total += r; units += (D.pflag[i] & PF_PAIRED) ? r / 2 : r; any |= D.n_matches[i]; }
    }
    uniq += total == 1u ? 1 : 0;
    dropped += any ? 0 : 1;
    if (total == 0) continue;
    if (total > RR_HI) D.counters[3] = 1;   // HI does not fit its 28 bits
    const bool have_prim = D.names != nullptr;
    uint32_t idx = 0;
    if (have_prim && units > 1) {
      // uniform_int_distribution(0, units - 1) on the stored first output; the rejection branch (probability units / 2^64)
      // replays the whole generator from the name
      uint64_t hi, lo;
      mul64wide(D.rnd0[g], (uint64_t)units, hi, lo);
      idx = (uint32_t)hi;
      if (lo < (uint64_t)units) {
        const uint64_t thr = (0 - (uint64_t)units) % (uint64_t)units;
        if (lo < thr) { const uint32_t no = D.name_off[a0]; idx = primary_pick(D.names + no, D.name_off[a0 + 1] - no, units); }
      }
    }
    uint32_t run = 0;
    if (small) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t i = a0 + (uint32_t)k, r = r4[k];   // (0 from the group's end on)
        if (r) {
        const uint32_t pf = f4[k];
        const bool paired = (pf & PF_PAIRED) != 0;
        const uint32_t u = paired ? r / 2 : r;
        uint32_t prim = 0;
        if (have_prim && idx != 0xffffffffu) { if (idx < u) { prim = idx + 1u; idx = 0xffffffffu; } else idx -= u; }
        D.gd[i] = make_uint2(pf | (prim << 8), total);
        D.hi0[i] = run + 1u;
        if (paired) {
          const uint32_t m = (uint32_t)mi4[k], mk = m - a0;
          const uint32_t pfm = mk < na ? (mk == 0 ? f4[0] : mk == 1 ? f4[1] : mk == 2 ? f4[2] : f4[3]) : (uint32_t)D.pflag[m];
          D.gd[m] = make_uint2(pfm | (prim << 8), total);
          D.hi0[m] = run + 2u;
        }
        run += r;
        }
      }
    } else {
      for (uint32_t i = a0; i < a1; i++) {
        const uint32_t r = D.n_rows[i];
        if (!r) continue;
        const uint32_t pf = D.pflag[i];
        const bool paired = (pf & PF_PAIRED) != 0;
        const uint32_t u = paired ? r / 2 : r;
        uint32_t prim = 0;
        if (have_prim && idx != 0xffffffffu) { if (idx < u) { prim = idx + 1u; idx = 0xffffffffu; } else idx -= u; }
        D.gd[i] = make_uint2(pf | (prim << 8), total);
        D.hi0[i] = run + 1u;
        if (paired) {
          const uint32_t m = (uint32_t)D.mate_idx[i];
          D.gd[m] = make_uint2((uint32_t)D.pflag[m] | (prim << 8), total);
          D.hi0[m] = run + 2u;
        }
        run += r;
      }
    }
  }
  // the two counters: one pair of atomics per block, spread over GD_SLOTS cache lines (16 384 atomics of 8 192 waves on one
  // address queue up in one L2 channel -- and every load of the kernels beside that needs that channel queues with them);
  // the host adds the slots up
  __shared__ unsigned long long sh_c[4][2];
  uniq = wave_sum(uniq); dropped = wave_sum(dropped);
  if ((threadIdx.x & 63) == 0) { sh_c[threadIdx.x >> 6][0] = uniq; sh_c[threadIdx.x >> 6][1] = dropped; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long u = sh_c[0][0] + sh_c[1][0] + sh_c[2][0] + sh_c[3][0], dr = sh_c[0][1] + sh_c[1][1] + sh_c[2][1] + sh_c[3][1];
    uint64_t *slot = D.counters + GD_SLOT0 + (size_t)(blockIdx.x & (GD_SLOTS - 1)) * GD_SLOT_STRIDE;
    if (u) atomicAdd((unsigned long long *)&slot[0], u);
    if (dr) atomicAdd((unsigned long long *)&slot[1], dr);
  }
}

// ---------------------------------------------------------------------------
// k_expand_rows: the emit work list over the KEPT matches (class-partitioned, as k_expand) and the second half of
// every emitting alignment's descriptor: .z = its first record (the leader's row offset, + 1 for the mate: a pair's
// records alternate), .w = where its entries start in the work list.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_expand_rows(DirectArgs D) {
  __shared__ uint32_t sh_pre[4][64], sh_v[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (D.m_aln_cap && D.tot[TOT_MATCHES] > D.m_aln_cap) return;   // launched ahead with the last call's list: too small this time (the host launches again)
  if (D.side_used[1]) return;   // the side arena ran out: counts and class positions are not to be trusted (see k_group_desc)
  uint32_t nk = 0, pos = 0, v = 0;
  bool fast = false;
  if (a < D.n_aln) nk = D.n_kept[a];
  if (nk) {
    fast = D.fast_flag[a] >> 31;
    pos = D.cls_pos[a];
    const uint32_t y = D.pflag[a];   // (not the descriptor's first half: k_group_desc may still be writing it on the second stream)
    const bool is_mate = (y & PF_MATE) != 0;
    const uint32_t leader = is_mate ? (uint32_t)D.mate_idx[a] : (uint32_t)a;
    D.dpos[a] = make_uint2((uint32_t)D.row_off[leader] + (is_mate ? 1u : 0u), pos);
    v = (y & PF_BIG) ? 0xffffffffu : (uint32_t)a;
  }
  sh_v[wv][lane] = v;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const uint32_t mine = (nk && fast == (c == 0)) ? nk : 0u;
    const uint64_t have = __ballot(mine != 0u);
    if (!have) continue;                       // the same for the whole wave
    // (written out, not wave_scan: through the helper this kernel took 8 more SGPRs and a VGPR, for a reason not found, and it is on the step's path)
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(inc, d); if (lane >= d) inc += up; }
    const uint32_t total = __shfl(inc, 63), first = __shfl(pos, (int)__builtin_ctzll(have));
    __builtin_amdgcn_wave_barrier();
    sh_pre[wv][lane] = inc - mine;
    WAVE_SYNC();
    for (uint32_t e = lane; e < total; e += 64) {
      int l = 0;
#pragma unroll
      for (int st = 32; st; st >>= 1) if (sh_pre[wv][l + st] <= e) l += st;
      D.m_aln[first + e] = sh_v[wv][l];
    }
  }
}

// ---------------------------------------------------------------------------
// k_emit_rows<CLS>: one lane per kept match (work-list entry).  Entry -> alignment -> its k-th kept survivor (k-th set
// bit of the filtered mask) and that survivor's tid rank c among the kept (from the alignment's tid word, DirectArgs::kt, where
// k_pair_mask left one: the bits of the common tids below the lane's own; else the rank loop over s_tid, as k_emit_dense) ->
// candidate row -> ideal CIGAR, merge -> the packed row at first record + stride * c.  CLS as k_emit_dense: 1 = the simple
// prefix (one read exon from a single M op, and the light two-exon class the count pass adds to it: "M N M" with exact
// inner junctions, a closed form as well), 2 = the rest.
// ---------------------------------------------------------------------------
// (CLS 2 at five waves per SIMD: 91 VGPRs and no scratch.  At six, the most its LDS allows, the budget is 80 VGPRs and ten
// of them went to 44 bytes of scratch per lane: 0.80-0.87 ms against 0.73-0.74 now that the class holds only heavy entries.)
//
// PRE = 1 (CLS 2 only; "emit_general_preset", launch_emit_rows): the general class of the short-read preset, where the count pass's
// PRE = 1 applies -- no long-read rules and no small-exon rescue, as constants, so pass 1 of the walk, the slab search of the
// INS_EXON rule and the skipped-exon rule are not in its code.  Its CIGAR scratch is typed: a lane whose ideal and rewritten
// CIGAR fit its LDS slot (lds_ideal_fits / lds_out_fits: reads of up to five exons) builds and merges them through LDS
// pointers (ds_read / ds_write) and touches the arena only to copy a result of three or more ops out.  The lanes that do not
// fit run the generic (flat) code behind that; a wave without one skips it.  <2, 0> is the kernel of every other preset and
// the A/B switch's other side.  (0.77 -> 0.55 ms at the bench step, all of it from the typed scratch: the constants alone,
// six waves per SIMD at 80 VGPRs, cig_base loaded early and the result's first words kept in registers changed nothing or
// cost time, DESIGN 10.1 rows 43-47.)
template <int CLS, int PRE = 0>
__global__ void __launch_bounds__(256, CLS == 1 ? 8 : 5) k_emit_rows(ProjectArgs A, DirectArgs D, int64_t first, int64_t n_end) {
  static_assert(PRE == 0 || CLS == 2, "the preset instantiation is the general class's");
  __shared__ uint32_t sh_cig[CLS == 1 ? 1 : 256 * LDS_SLOT];
  __shared__ uint16_t sh_mops[CLS == 1 ? 1 : 256];
  if (CLS != 1) {
    sh_mops[threadIdx.x] = (uint16_t)((merge_action(threadIdx.x >> 4, threadIdx.x & 15u) << 8) | merge_ops(threadIdx.x >> 4, threadIdx.x & 15u));
    __syncthreads();
  }
  const int64_t e64 = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e64 >= n_end) return;
  const DevIndex &ix = A.ix;
  DevCfg cfg_pre = A.cfg;
  if (PRE) { cfg_pre.long_reads = 0; cfg_pre.ignore_small_exons = 0; cfg_pre.max_error_exon = 0; }
  const DevCfg &cfg = PRE ? cfg_pre : A.cfg;
  // (the work-list entry and the alignment's records are read once: streaming loads, so that they do not displace the index
  // rows the gathers below come back to -- k_emit_rows<2> 1.84 -> 1.79 ms)
  typedef uint32_t ntl4 __attribute__((ext_vector_type(4)));
  typedef uint32_t ntl2 __attribute__((ext_vector_type(2)));
  const uint32_t a = __builtin_nontemporal_load(D.m_aln + e64);
  if (a == 0xffffffffu) return;   // a big alignment's entry: k_big<1>
  const ntl4 hd_ = __builtin_nontemporal_load((const ntl4 *)(A.head + a)), rg_ = __builtin_nontemporal_load((const ntl4 *)(A.ranges + a));
  const ntl2 f_ = __builtin_nontemporal_load((const ntl2 *)(D.fm + a)), gd_ = __builtin_nontemporal_load((const ntl2 *)(D.gd + a)), dp_ = __builtin_nontemporal_load((const ntl2 *)(D.dpos + a));
  const uint4 hd = make_uint4(hd_.x, hd_.y, hd_.z, hd_.w), rg = make_uint4(rg_.x, rg_.y, rg_.z, rg_.w);
  const uint2 f = make_uint2(f_.x, f_.y), gd = make_uint2(gd_.x, gd_.y), dp = make_uint2(dp_.x, dp_.y);
  ntl4 kt = {0u, 0u, KT_NONE, 0u};   // the alignment's tid word (null array: "emit_rank_tids" 0, every lane ranks by the loop)
  if (D.kt) kt = __builtin_nontemporal_load((const ntl4 *)(D.kt + a));
  const uint4 E = make_uint4(gd.x, gd.y, dp.x, dp.y);   // the emit descriptor: {PF_* | (primary rank + 1) << 8, NH, first record, work-list position}
  const uint32_t is_fast = CLS == 1;
  uint4 hd2 = make_uint4(0, 0, 0, 0);
  uint32_t c0 = 0, c1 = 0;
  RealCig rc;
  if (CLS != 1) { hd2 = A.head2[a]; c0 = A.cigar_off[a]; c1 = A.cigar_off[a + 1]; }
  else if (hd.z == 2) hd2 = A.head2[a];   // the light two-exon class: read exon 1 (in flight with the row load below)
  const uint32_t n_seg = hd.z, rid = hd.w >> 2;
  const uint2 q0 = make_uint2(hd.x, hd.y);
  const int st0 = (n_seg == 1) ? ST_ONLY : ST_FIRST;
  const uint32_t n0 = rg.y - rg.x;
  if (CLS != 1) rc.fetch(A.cigar + c0, c1 - c0);   // in flight with the row load below
  const uint32_t k = (uint32_t)e64 - E.w;
  const uint64_t fmask = (uint64_t)f.x | ((uint64_t)f.y << 32);
  const uint32_t item = kth_set_bit64(fmask, k);
  const int s = item < n0 ? 0 : 1;
  const uint32_t row = s == 0 ? rg.x + item : rg.z + (item - n0);
  const uint4 r_a = ix.s_row[2 * (size_t)row], r_b = ix.s_row[2 * (size_t)row + 1];
  const uint32_t gs = r_a.x, gend = r_a.y;
  const uint4 pay = make_uint4(r_b.x, r_b.y, r_a.w, r_b.z);
  uint32_t c = 0;   // rank by tid among the kept: its record among the alignment's
  // With a tid word (k_pair_mask's mask path: nearly every pair) the kept tids are the bits of `common` relative to `base`, and
  // the rank is the number of bits below the lane's own; a single kept survivor has rank 0.  What is left -- SOLO alignments
  // with several survivors, list-path pairs, partners of big alignments -- gathers the kept survivors' tids, and a wave
  // without such a lane skips that.
  const bool has_word = kt.z != KT_NONE;
  const bool by_loop = !has_word && (fmask & (fmask - 1)) != 0;
  if (has_word) c = (uint32_t)__popcll(((uint64_t)kt.x | ((uint64_t)kt.y << 32)) & ((1ull << ((pay.x - kt.z) & 63u)) - 1ull));
  if (__ballot(by_loop)) {
    for (uint64_t m2 = by_loop ? fmask : 0ull; m2;) {   // eight loads in flight per step: unconditional (spent slots re-read the lane's own row)
      uint32_t t8[8]; bool ok[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        ok[u] = m2 != 0;
        const uint32_t b = ok[u] ? (uint32_t)(__ffsll((long long)m2) - 1) : item;
        m2 &= m2 - 1;
        t8[u] = ix.s_tid[b < n0 ? rg.x + b : rg.z + (b - n0)];
      }
#pragma unroll
      for (int u = 0; u < 8; u++) c += (ok[u] && t8[u] < pay.x) ? 1u : 0u;
    }
  }
  Hit h0;
  classify(s == 1, st0, q0.x, q0.y, gs, gend, pay.z, cfg, h0);
  if (is_fast) {
    // one read exon from a single M op: the rewritten CIGAR is [S left_ins] M [S right_ins] (see k_emit_dense)
    const uint32_t os = q0.x > gs ? q0.x : gs, oe = q0.y < gend ? q0.y : gend;
    uint32_t ml = oe - os, pos = h0.pos, r_ins = h0.right_ins, junc_in = 0;
    bool r_exact = h0.right_ins == 0 && h0.right_gap == 0;
    if (n_seg == 2) {
      // The light two-exon class ("M N M", every kept survivor's inner junction the annotated one: the count pass's mark).
      // walk_pass2 under `plain` for it: the second read exon hits exactly the exon after the candidate's (status LAST),
      // build_match adds (ml0)M then (ml1)M -- one op in the ideal sink -- and two junction hits for the inner sides; the
      // merge with "aM bN cM" drops the N, so the rewritten CIGAR is [S left_ins] (ml0 + ml1)M [S right_ins of the
      // second hit].  pos: the first hit's on '+', acc.last_pos (the second hit's) on '-'.
      const uint2 q1 = make_uint2(hd2.x, hd2.y);
      const uint4 e1 = next_row(make_uint4(gs, gend, pay.z, 0), make_uint2(r_a.z, r_b.w), s == 1);
      Hit hh;
      classify(s == 1, ST_LAST, q1.x, q1.y, e1.x, e1.y, e1.z, cfg, hh);
      ml += (q1.y < e1.y ? q1.y : e1.y) - q1.x;
      pos = s == 0 ? h0.pos : hh.pos;
      r_ins = hh.right_ins; r_exact = hh.right_ins == 0 && hh.right_gap == 0;
      junc_in = 2;
    }
    uint32_t w0, w1 = 0, w2 = 0, n_out;
    if (h0.left_ins) { w0 = CIG_GEN(h0.left_ins, OP_S); w1 = CIG_GEN(ml, OP_M); n_out = 2; if (r_ins) { w2 = CIG_GEN(r_ins, OP_S); n_out = 3; } }
    else { w0 = CIG_GEN(ml, OP_M); n_out = 1; if (r_ins) { w1 = CIG_GEN(r_ins, OP_S); n_out = 2; } }
    const uint32_t junc = junc_in + ((h0.left_ins == 0 && h0.left_gap == 0) ? 1u : 0u) + (r_exact ? 1u : 0u);
    uint64_t cref = (uint64_t)w0 | ((uint64_t)w1 << 32);
    if (n_out == 3) {
      // the alignment's own slot capacity (k_segment / the count pass): n_cigar + 2 * (4 * n_seg + 2)
      cref = D.cig_base[a] + (uint64_t)c * (n_seg == 2 ? 3u + 2u * 10u : 1u + 2u * 6u);
      uint32_t *slot = A.cig_arena + cref;
      slot[0] = w0; slot[1] = w1; slot[2] = w2;
    }
    write_row(D, E, a, c, pay.x, pos, n_out, s == 1, cref, junc, ml);
    return;
  }
  if (CLS == 1) return;
  ReadCtx rd;
  rd.n_seg = n_seg; rd.seg = A.seg + (size_t)c0 + (size_t)a; rd.real = A.cigar + c0; rd.n_real = c1 - c0; rd.q12 = hd2;
  const uint4 *Ex = ix.tx_ex + pay.w;
  const uint32_t i0 = pay.y & 0x7fffffffu;
  CandOut p1;
  bool plain = false;
  uint32_t sb = 0, se = 0;   // (the slab's bounds: the INS_EXON rule's search only)
  if (!PRE) { sb = ix.slab_off[2 * rid + s]; se = ix.slab_off[2 * rid + s + 1]; }
  if (n_seg == 1) { p1.alive = true; p1.fwpos = h0.pos; p1.rcpos = h0.pos; p1.n_seg = 1; p1.n_gex = 1; p1.i_lastm = i0; p1.last_right_ins = h0.right_ins; p1.last_right_gap = h0.right_gap; }
  else if (PRE || (!cfg.long_reads && !cfg.ignore_small_exons)) {
    // short-read presets without --max-error-exon: pass 1's counts are the read's exon count (see k_emit_dense)
    plain = true;
    p1.alive = true; p1.fwpos = h0.pos; p1.rcpos = h0.pos; p1.n_seg = n_seg; p1.n_gex = n_seg; p1.i_lastm = i0;
    p1.last_right_ins = 0; p1.last_right_gap = 0;
  }
  else p1 = walk_pass1(ix, cfg, rd, Ex, s == 1, sb, se, i0, make_uint4(gs, gend, pay.z, 0), make_uint2(r_a.z, r_b.w), q0, h0);
  const uint32_t ideal_cap = 4u * n_seg + 2u;
  const uint32_t cap = rd.n_real + 2u * ideal_cap;
  const uint64_t slot_off = D.cig_base[a] + (uint64_t)c * cap;
  uint32_t *slot = A.cig_arena + slot_off;
  if constexpr (PRE != 0) {
    lds_u32 *lds = (lds_u32 *)&sh_cig[threadIdx.x * LDS_SLOT];
    lds_cu16 *mops = (lds_cu16 *)&sh_mops[0];
    Acc acc;
    uint32_t n_out = 0, n_ideal = 0;
    uint2 w01 = make_uint2(0, 0);   // the result's first two words
    const bool t_ideal = lds_ideal_fits(n_seg);
    bool done = false;
    if (t_ideal) {
      IdealSinkT<lds_u32 *> sk;
      sk.init(lds);
      walk_pass2(ix, cfg, rd, Ex, s == 1, sb, se, i0, q0, make_uint4(gs, gend, pay.z, 0), make_uint2(r_a.z, r_b.w), h0, p1, acc, sk, no_clip(), no_clip());
      n_ideal = sk.finish();
      if (lds_out_fits(rd.n_real, n_ideal)) {
        lds_u32 *outp = lds + n_ideal;
        n_out = merge_cigars_t(rc, rd.n_real, lds, n_ideal, outp, mops);
        w01 = make_uint2(n_out > 0 ? outp[0] : 0u, n_out > 1 ? outp[1] : 0u);   // (ds_read: a wait on LDS alone)
        for (uint32_t q = 0; n_out > 2 && q < n_out; q++) slot[q] = outp[q];   // (the arena copy: the result)
        done = true;
      }
      // (else the output goes to the arena and the ideal CIGAR stays where it is: the generic merge below reads it through a
      // flat pointer)
    }
    if (__ballot(!done)) {
      if (!done) {
        uint32_t *ideal = t_ideal ? (uint32_t *)lds : slot + rd.n_real + ideal_cap;
        if (!t_ideal) {
          IdealSink sk;
          sk.init(ideal);
          walk_pass2(ix, cfg, rd, Ex, s == 1, sb, se, i0, q0, make_uint4(gs, gend, pay.z, 0), make_uint2(r_a.z, r_b.w), h0, p1, acc, sk, no_clip(), no_clip());
          n_ideal = sk.finish();
        }
        n_out = merge_cigars(rc, rd.n_real, ideal, n_ideal, slot, (const uint16_t *)mops);
        w01 = make_uint2(n_out > 0 ? slot[0] : 0u, n_out > 1 ? slot[1] : 0u);
      }
    }
    uint64_t cig_ref = slot_off;
    if (n_out <= 2) cig_ref = (uint64_t)(n_out > 0 ? w01.x : 0u) | ((uint64_t)(n_out > 1 ? w01.y : 0u) << 32);
    write_row(D, E, a, c, pay.x, (s == 0) ? p1.fwpos : (plain ? acc.last_pos : p1.rcpos), n_out, s == 1, cig_ref,
              (uint32_t)acc.junc_hits, (uint32_t)acc.ref_consumed);
    return;
  }
  uint32_t *lds = &sh_cig[(CLS == 1 ? 0 : threadIdx.x) * LDS_SLOT];
  const bool ideal_lds = ideal_cap <= LDS_IDEAL;
  uint32_t *ideal = ideal_lds ? lds : slot + rd.n_real + ideal_cap;
  Acc acc; IdealSink sk;
  sk.init(ideal);
  walk_pass2(ix, cfg, rd, Ex, s == 1, sb, se, i0, q0, make_uint4(gs, gend, pay.z, 0), make_uint2(r_a.z, r_b.w), h0, p1, acc, sk, no_clip(), no_clip());
  const uint32_t n_ideal = sk.finish();
  const bool out_lds = ideal_lds && (rd.n_real + n_ideal <= LDS_SLOT - LDS_IDEAL);
  uint32_t *outp = out_lds ? lds + LDS_IDEAL : slot;
  const uint32_t n_out = merge_cigars(rc, rd.n_real, ideal, n_ideal, outp, sh_mops);
  uint64_t cig_ref = slot_off;
  if (n_out <= 2) cig_ref = (uint64_t)(n_out > 0 ? outp[0] : 0u) | ((uint64_t)(n_out > 1 ? outp[1] : 0u) << 32);
  else if (out_lds) for (uint32_t q = 0; q < n_out; q++) slot[q] = outp[q];
  write_row(D, E, a, c, pay.x, (s == 0) ? p1.fwpos : (plain ? acc.last_pos : p1.rcpos), n_out, s == 1, cig_ref,
            (uint32_t)acc.junc_hits, (uint32_t)acc.ref_consumed);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static inline int grid_for_d(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

void launch_name_seed(hipStream_t st, const DirectArgs &D) {
  if (D.n_groups > 0 && D.names) hipLaunchKernelGGL(k_name_seed, dim3(grid_for_d(D.n_groups, 256)), dim3(256), 0, st, D);
}
template <bool BM>
static void launch_pair_mask_t(hipStream_t st, const DirectArgs &D, int wide_blocks) {
  hipLaunchKernelGGL((k_pair_mask<BM>), dim3(grid_for_d(D.n_aln, 4 * 62)), dim3(256), 0, st, D);   // a wave per 62 alignments
  hipLaunchKernelGGL((k_pair_mask_wide<BM>), dim3(wide_blocks), dim3(64), 0, st, D);   // the windows the first kernel listed (dense loci)
}
void launch_pair_mask(hipStream_t st, const DirectArgs &D, int wide_blocks, bool bitmask) {
  if (D.n_aln <= 0) return;
  if (bitmask) launch_pair_mask_t<true>(st, D, wide_blocks); else launch_pair_mask_t<false>(st, D, wide_blocks);
}
void launch_big_collect(hipStream_t st, const ProjectArgs &A, const DirectArgs &D, int n_blocks) {
  if (D.n_aln > 0 && A.ix.n_rows != 0) hipLaunchKernelGGL((k_big<0>), dim3(n_blocks), dim3(64), 0, st, A, D);
}
void launch_pair_big(hipStream_t st, const DirectArgs &D, int n_blocks) {
  if (D.n_aln > 0) hipLaunchKernelGGL(k_pair_big, dim3(n_blocks), dim3(64), 0, st, D);
}
void launch_big_emit(hipStream_t st, const ProjectArgs &A, const DirectArgs &D, int n_blocks) {
  if (D.n_aln > 0 && A.ix.n_rows != 0) hipLaunchKernelGGL((k_big<1>), dim3(n_blocks), dim3(64), 0, st, A, D);
}
void launch_scan5(hipStream_t st, const DirectArgs &D, uint64_t *tile_sums, uint64_t *total_out5) {
  int64_t tiles = scan_tiles_for(D.n_aln);
  if (tiles < 1) tiles = 1;
  hipLaunchKernelGGL(k_scan5_tiles, dim3((unsigned)tiles), dim3(256), 0, st, D, tile_sums, tiles);
  hipLaunchKernelGGL(k_scan5_top, dim3(5), dim3(256), 0, st, tile_sums, tiles, total_out5);
  hipLaunchKernelGGL(k_scan5_apply, dim3((unsigned)tiles), dim3(256), 0, st, D, (const uint64_t *)tile_sums, tiles, (const uint64_t *)total_out5);
}
void launch_group_desc(hipStream_t st, const DirectArgs &D) {
  if (D.n_groups > 0) hipLaunchKernelGGL(k_group_desc, dim3(std::min(grid_for_d(D.n_groups, 256), 2048)), dim3(256), 0, st, D);   // (grid-stride: one counter atomic per wave at the end)
}
void launch_expand_rows(hipStream_t st, const DirectArgs &D) {
  if (D.n_aln > 0) hipLaunchKernelGGL(k_expand_rows, dim3(grid_for_d(D.n_aln, 256)), dim3(256), 0, st, D);
}
// part 1: the work list's simple prefix [0, n_simple), 2: the rest
// preset ("emit_general_preset"): part 2 runs k_emit_rows<2, 1> where its constants hold -- the count pass's PRE = 1 (launch_count_g)
// on the direct-rows route, which the similarity filter and -S never take -- and k_emit_rows<2, 0> otherwise
static inline bool emit_general_preset_applies(const DevCfg &cfg, bool preset) {
  return preset && !cfg.long_reads && !cfg.ignore_small_exons && !cfg.filter_by_similarity && !cfg.use_fasta;
}
void launch_emit_rows(hipStream_t st, const ProjectArgs &A, const DirectArgs &D, int64_t n_kept, int64_t n_simple, int part, bool preset) {
  if (A.n_aln <= 0 || n_kept <= 0) return;
  if (part == 1) { if (n_simple > 0) hipLaunchKernelGGL((k_emit_rows<1>), dim3(grid_for_d(n_simple, 256)), dim3(256), 0, st, A, D, (int64_t)0, n_simple); }
  else if (n_kept > n_simple) {
    const dim3 g(grid_for_d(n_kept - n_simple, 256)), b(256);
    if (emit_general_preset_applies(A.cfg, preset)) hipLaunchKernelGGL((k_emit_rows<2, 1>), g, b, 0, st, A, D, n_simple, n_kept);
    else hipLaunchKernelGGL((k_emit_rows<2, 0>), g, b, 0, st, A, D, n_simple, n_kept);
  }
}
