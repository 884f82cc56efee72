// -S soft-clip rescue for long reads (rows a9/a10 of SURVEY.md 8a).  Included by
// project_kernels.hip (shares its per-lane building blocks).
//
//   k_project_fa<MODE>   wave per alignment; MODE 0 counts the rescue problems of
//                        every pass-1 survivor, 1 writes their descriptors and the
//                        2-bit-coded query / target sequences, 2 counts matches with
//                        the rescue results applied, 3 emits them.
//   The DP itself (ksw_extz2, traceback, build_left/right_clip_segment) is ksw_kernels.hip.
//
// No reference test exercises this path and ksw2.h is not in the reference tree.  What pins it instead:
//   the DP        an independent full-matrix checker (tests/ksw2_gotoh.c, tests/golden/ksw2_cases.json; k_ksw / k_ksw_dp /
//                 k_ksw_trace are compared with both through br_ctx_ksw_pairs in tests/test_ksw2_pinned.py), and behind it
//                 clip_segment on left- and right-side problems against build_left / build_right_clip_segment restated in
//                 tests/rescue_ref.py (the same test, br_ctx_ksw_pairs with sides and segments);
//   the front end every decision below -- the 5-base rule, max >= 10, the gap / overhang gating, no neighbour exon, the cap at
//                 the shared sequence's length, its source record, the target window over short exons and its trim, N and
//                 lower case in the exon pool, both sides of one candidate, more rows than G and than 64, rcpos -- one
//                 hand-built read each (tests/rescue_cases.py), rows against tests/rescue_ref.py's frozen answers
//                 (tests/golden/rescue_expect.json) and the oracle, br_ctx_rescue_stats against its problem / rescued counts,
//                 on every route and through the BAM-record entry (tests/test_gpu_rescue_cases.py).

__device__ __forceinline__ uint8_t base_code(uint8_t c) {
  switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
               case 'T': case 't': return 3; default: return 4; }
}

// What one candidate needs from the rescue stage.
struct FaCand {
  bool alive;            // pass-1 survivor
  bool wantL, wantR;
  uint32_t qlenL, tlenL, qlenR, tlenR;
};

// Length of the target window of a rescue: neighbour exons are added until they
// cover the query (collect_left/right_exons, src/evaluate.cpp:333-365,513-546), then
// trimmed to qlen + 40 (:374-375,630).
__device__ __forceinline__ uint32_t target_len(const uint4 *E, uint32_t i_from, bool leftwards, uint32_t qlen) {
  uint32_t acc = 0;
  if (leftwards) { for (uint32_t i = i_from; acc < qlen; i--) { acc += E[i].y - E[i].x; if (i == 0) break; } }
  else { for (uint32_t i = i_from; acc < qlen && E[i].x != 0xffffffffu; i++) acc += E[i].y - E[i].x; }
  uint32_t cap = qlen + 40u;
  return acc < cap ? acc : cap;
}

// G lanes per alignment (a long read has a handful of candidate rows: with a whole wave per alignment most lanes idled);
// every ballot / shuffle below is confined to the group.
template <int MODE, int G>
__global__ void __launch_bounds__(256) k_project_fa(ProjectArgs A, FaArgs F) {
  const int gl = threadIdx.x & (G - 1);
  const int gbase = (threadIdx.x & 63) & ~(G - 1);
  const uint64_t gmask = (G == 64) ? ~0ull : ((1ull << G) - 1ull);
  auto gballot = [&](bool x) -> uint64_t { return (__ballot(x) >> gbase) & gmask; };
  const int64_t groups_total = (int64_t)gridDim.x * (blockDim.x / G);
  const int64_t gid = (int64_t)blockIdx.x * (blockDim.x / G) + threadIdx.x / G;
  const DevIndex &ix = A.ix;
  const DevCfg &cfg = A.cfg;

  for (int64_t a = gid; a < A.n_aln; a += groups_total) {
    uint4 hd = A.head[a];
    uint32_t n_seg = hd.z;
    if (n_seg == 0) {
      if (gl == 0) {
        if (MODE == 0) { F.n_prob[a] = 0; F.seq_bytes[a] = 0; A.ranges[a] = make_uint4(0, 0, 0, 0); }
        if (MODE == 2) { A.n_matches[a] = 0; F.ideal_cap[a] = 0; }
      }
      continue;
    }
    if (MODE == 3 && A.n_matches[a] == 0) continue;
    if (MODE == 3) { const uint4 rg3 = A.ranges[a]; if ((rg3.y - rg3.x) + (rg3.w - rg3.z) <= 64u) continue; }   // k_emit_dense<.., FA> emits those
    uint2 q0 = make_uint2(hd.x, hd.y);
    uint32_t smode = hd.w & 3u, rid = hd.w >> 2;
    int st0 = (n_seg == 1) ? ST_ONLY : ST_FIRST;
    uint32_t sb[2], se[2];
    sb[0] = ix.slab_off[2 * rid]; se[0] = ix.slab_off[2 * rid + 1]; se[1] = ix.slab_off[2 * rid + 2]; sb[1] = se[0];
    uint32_t lo[2] = {0, 0}, hi[2] = {0, 0};
    if (MODE != 0) { uint4 rg = A.ranges[a]; lo[0] = rg.x; hi[0] = rg.y; lo[1] = rg.z; hi[1] = rg.w; }
    else {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        lo[s] = hi[s] = sb[s];
        if (!((smode >> s) & 1u) || sb[s] == se[s]) continue;
        uint32_t bo = ix.bin_off[rid], nb = ix.bin_off[rid + 1] - bo - 1;
        uint32_t bh = q0.y >> ix.bin_shift, bl = q0.x >> ix.bin_shift;
        bh = bh < nb - 1 ? bh : nb - 1; bl = bl < nb - 1 ? bl : nb - 1;
        const uint4 th0 = ix.t_bin[bo + bh], th1 = ix.t_bin[bo + bh + 1], tl0 = ix.t_bin[bo + bl], tl1 = ix.t_bin[bo + bl + 1];
        uint32_t ha = s ? th0.w : th0.y, hb = s ? th1.w : th1.y, la = s ? tl0.z : tl0.x, lb = s ? tl1.z : tl1.x;
        uint32_t ch = 0, cl = 0;
        for (uint32_t r0 = ha; r0 < hb; r0 += G) { uint32_t r = r0 + gl; ch += (uint32_t)__popcll(gballot(r < hb && ix.s_start[r] < q0.y)); }
        for (uint32_t r0 = la; r0 < lb; r0 += G) { uint32_t r = r0 + gl; cl += (uint32_t)__popcll(gballot(r < lb && ix.s_pmax[r] <= q0.x)); }
        hi[s] = ha + ch; lo[s] = la + cl < hi[s] ? la + cl : hi[s];
      }
      if (gl == 0) A.ranges[a] = make_uint4(lo[0], hi[0], lo[1], hi[1]);
    }
    uint32_t n0 = hi[0] - lo[0], n1 = hi[1] - lo[1], n_items = n0 + n1;

    uint32_t c0 = A.cigar_off[a];
    ReadCtx rd;
    rd.n_seg = n_seg; rd.seg = A.seg + (size_t)c0 + (size_t)a; rd.real = A.cigar + c0; rd.n_real = A.cigar_off[a + 1] - c0;
    rd.q12 = A.head2[a];
    AlnMeta mt = A.meta[a];
    int32_t src = F.seq_src[a];
    uint32_t seq_len = 0;
    if (src >= 0) seq_len = F.seq_off[src + 1] - F.seq_off[src];
    uint32_t p_base = (MODE >= 1) ? F.prob_off[a] : 0;        // first problem of this alignment
    uint64_t s_base = (MODE == 1) ? F.seqarena_off[a] : 0;    // its first sequence byte
    uint32_t moff = 0; uint64_t cbase = 0; uint32_t cap = 0, ideal_cap = 0;
    if (MODE == 3) { moff = A.match_off[a]; cbase = A.cig_base[a]; ideal_cap = F.ideal_cap[a]; cap = rd.n_real + 2u * ideal_cap; }

    uint32_t tot_prob = 0; uint32_t tot_bytes = 0, total = 0, max_ops = 0, aux_n = 0;
    uint64_t m_alive = 0, m_wl = 0, m_wr = 0;   // MODE 2, at most 64 candidate rows: survivors and rescue wishes by candidate index
    const int n_sweeps = (MODE == 3) ? 2 : 1;
    for (int sweep = 0; sweep < n_sweeps; sweep++) {
      uint32_t run_prob = 0; uint64_t run_bytes = 0;
      for (uint32_t base = 0; base < n_items; base += G) {
        uint32_t item = base + (uint32_t)gl;
        bool valid = item < n_items;
        int s = 0; uint32_t row = 0, gs = 0, gend = 0, nxt = 0;
        uint4 pay = make_uint4(0xffffffffu, 0, 0, 0);
        Hit h0; CandOut p1; const uint4 *E = nullptr; uint32_t i0 = 0;
        FaCand fc; fc.alive = false; fc.wantL = fc.wantR = false; fc.qlenL = fc.tlenL = fc.qlenR = fc.tlenR = 0;
        p1.alive = false; p1.fwpos = p1.rcpos = p1.n_seg = p1.n_gex = p1.i_lastm = p1.last_right_ins = p1.last_right_gap = 0;
        h0.pos = h0.left_ins = h0.right_ins = h0.left_gap = h0.right_gap = 0;
        if (valid) {
          s = item < n0 ? 0 : 1;
          row = s == 0 ? lo[0] + item : lo[1] + (item - n0);
          const uint4 r_a = ix.s_row[2 * (size_t)row], r_b = ix.s_row[2 * (size_t)row + 1];
          gs = r_a.x; gend = r_a.y; nxt = r_a.z; pay = make_uint4(r_b.x, r_b.y, r_a.w, r_b.z);
          if (gend > q0.x && classify(s == 1, st0, q0.x, q0.y, gs, gend, pay.z, cfg, h0)) {
            E = ix.tx_ex + pay.w; i0 = pay.y & 0x7fffffffu;
            bool superseded = false;
            if (nxt < q0.y) {
              for (uint32_t i = i0 + 1;; i++) {
                uint4 e = E[i];
                if (e.x >= q0.y) break;
                Hit hx;
                if (e.y > q0.x && classify(s == 1, st0, q0.x, q0.y, e.x, e.y, e.z, cfg, hx)) { superseded = true; break; }
              }
            }
            if (!superseded) {
              p1 = walk_pass1(ix, cfg, rd, E, s == 1, sb[s], se[s], i0, make_uint4(gs, gend, pay.z, 0), make_uint2(0, 0), q0, h0);
              fc.alive = p1.alive;
            }
          }
        }
        if (fc.alive) {
          // left_clip_rescue / right_clip_rescue preconditions (src/evaluate.cpp:946-963,459,608)
          if (mt.n_left_clip >= 5 && h0.left_gap == 0) {
            uint32_t tot = mt.n_left_clip + h0.left_ins; if (tot > seq_len) tot = seq_len;
            if (tot > 0 && i0 > 0) { fc.wantL = true; fc.qlenL = tot; fc.tlenL = target_len(E, i0 - 1, true, tot); }
          }
          if (mt.n_right_clip >= 5 && p1.last_right_gap == 0) {
            uint32_t tot = p1.last_right_ins + mt.n_right_clip; if (tot > seq_len) tot = seq_len;
            if (tot > 0 && E[p1.i_lastm + 1].x != 0xffffffffu) { fc.wantR = true; fc.qlenR = tot; fc.tlenR = target_len(E, p1.i_lastm + 1, false, tot); }
          }
        }
        // problem index: item-major, left before right
        uint64_t bl = gballot(fc.wantL), br = gballot(fc.wantR);
        uint64_t lower = (1ull << gl) - 1ull;
        uint32_t pidxL = run_prob + (uint32_t)__popcll(bl & lower) + (uint32_t)__popcll(br & lower);
        uint32_t pidxR = pidxL + (fc.wantL ? 1u : 0u);
        uint32_t my_bytes = (fc.wantL ? fc.qlenL + fc.tlenL : 0u) + (fc.wantR ? fc.qlenR + fc.tlenR : 0u);
        // exclusive prefix of my_bytes over the wave
        const uint32_t incl = wave_scan<uint32_t, G>(my_bytes);
        uint32_t chunk_bytes = __shfl(incl, G - 1, G);
        uint64_t my_off = run_bytes + (incl - my_bytes);
        run_prob += (uint32_t)__popcll(bl) + (uint32_t)__popcll(br);
        run_bytes += chunk_bytes;

        if (MODE == 0) continue;
        if (MODE == 1) {
          // descriptors; k_fa_fill writes the coded sequences (a group of lanes per problem instead of byte loops here)
          if (fc.wantL) {
            KswProb pr; pr.qlen = fc.qlenL; pr.tlen = fc.tlenL; pr.side = 0; pr.t_has_n = 0; pr.seq_off = s_base + my_off;
            F.probs[p_base + pidxL] = pr;
            FaSrc sr; sr.aln = (uint32_t)a; sr.e_base = pay.w; sr.i_from = i0 - 1; sr.pad = 0;
            F.srcs[p_base + pidxL] = sr;
          }
          if (fc.wantR) {
            KswProb pr; pr.qlen = fc.qlenR; pr.tlen = fc.tlenR; pr.side = 1; pr.t_has_n = 0;
            pr.seq_off = s_base + my_off + (fc.wantL ? fc.qlenL + fc.tlenL : 0u);
            F.probs[p_base + pidxR] = pr;
            FaSrc sr; sr.aln = (uint32_t)a; sr.e_base = pay.w; sr.i_from = p1.i_lastm + 1; sr.pad = 0;
            F.srcs[p_base + pidxR] = sr;
          }
          continue;
        }
        // MODE 2 / 3: apply the rescue results
        ClipSide L = no_clip(), R = no_clip();
        if (fc.wantL) {
          KswRes rs = F.results[p_base + pidxL];
          if (rs.ok) { L.ok = true; L.ops = F.clip_ops + (F.probs[p_base + pidxL].seq_off + p_base + pidxL); L.n_ops = rs.n_ops; L.score = rs.score; L.refc = (uint32_t)rs.refc; }
        }
        if (fc.wantR) {
          KswRes rs = F.results[p_base + pidxR];
          if (rs.ok) { R.ok = true; R.ops = F.clip_ops + (F.probs[p_base + pidxR].seq_off + p_base + pidxR); R.n_ops = rs.n_ops; R.score = rs.score; R.refc = (uint32_t)rs.refc; }
        }
        bool alive = fc.alive;
        Acc acc; IdealSink sk; double score = 0.0;
        if (alive) {
          apply_clips(p1, s == 1, pay.z, E[p1.i_lastm].z, L, R);
          sk.init(nullptr);
          walk_pass2(ix, cfg, rd, E, s == 1, sb[s], se[s], i0, q0, make_uint4(gs, gend, pay.z, 0), make_uint2(0, 0), h0, p1, acc, sk, L, R);
          alive = similarity(cfg, acc, score);
        }
        uint64_t m = gballot(alive);
        if (MODE == 2) {
          if (base < 64u) { m_alive |= m << base; m_wl |= bl << base; m_wr |= br << base; }
          total += (uint32_t)__popcll(m);
          uint32_t ops = alive ? (L.n_ops + R.n_ops) : 0u;
          ops = wave_max<uint32_t, G>(ops);
          max_ops = max_ops > ops ? max_ops : ops;
          continue;
        }
        // MODE 3: sweep 0 lists the survivors' tids, sweep 1 ranks and emits
        if (sweep == 0) {
          if (alive) A.m_aux[moff + aux_n + (uint32_t)__popcll(m & lower)] = pay.x;
          aux_n += (uint32_t)__popcll(m);
        } else if (alive) {
          uint32_t rank = 0;
          for (uint32_t k = 0; k < aux_n; k++) rank += (A.m_aux[moff + k] < pay.x) ? 1u : 0u;
          uint32_t *slot = A.cig_arena + cbase + (uint64_t)rank * cap;
          uint32_t *ideal = slot + rd.n_real + ideal_cap;
          sk.init(ideal);
          walk_pass2(ix, cfg, rd, E, s == 1, sb[s], se[s], i0, q0, make_uint4(gs, gend, pay.z, 0), make_uint2(0, 0), h0, p1, acc, sk, L, R);
          uint32_t n_ideal = sk.finish();
          RealCig rc; rc.fetch(rd.real, rd.n_real);
          uint32_t n_out = merge_cigars(rc, rd.n_real, ideal, n_ideal, slot);
          uint64_t cig_ref = cbase + (uint64_t)rank * cap;
          if (n_out <= 2) cig_ref = (uint64_t)(n_out > 0 ? slot[0] : 0u) | ((uint64_t)(n_out > 1 ? slot[1] : 0u) << 32);
          uint32_t mi = moff + rank;
          A.m_tid[mi] = pay.x;
          A.m_p[mi] = make_uint2((s == 0) ? p1.fwpos : p1.rcpos, n_out | ((uint32_t)s << 31));
          A.m_x[mi] = make_uint2((uint32_t)acc.junc_hits, (uint32_t)acc.ref_consumed);
          unsigned long long sb64 = (unsigned long long)__double_as_longlong(score);
          A.m_b[mi] = make_uint4((uint32_t)acc.clip_score, 0u, (uint32_t)sb64, (uint32_t)(sb64 >> 32));
          A.m_cigoff[mi] = cig_ref;
        }
      }
      tot_prob = run_prob; tot_bytes = (uint32_t)run_bytes;
      if (MODE == 3 && sweep == 0) __threadfence_block();
    }
    if (gl == 0) {
      if (MODE == 0) { F.n_prob[a] = tot_prob; F.seq_bytes[a] = tot_bytes; }
      if (MODE == 2) { A.n_matches[a] = total; A.mask[a] = m_alive; F.want_l[a] = m_wl; F.want_r[a] = m_wr; F.ideal_cap[a] = 4u * n_seg + 2u + max_ops; }
    }
  }
}

// k_fa_fill: 16 lanes per rescue problem write its 0..4-coded query (the clipped bases + overhang, reversed for a left
// clip: align_reversed, src/evaluate.cpp:368-395) and target (neighbour exon sequences, collect_left/right_exons
// :333-365,513-546, trimmed to tlen) into the sequence arena, and note whether the target holds an N.
__global__ void __launch_bounds__(256) k_fa_fill(const uint4 *tx_ex, const uint8_t *seq_pool, FaArgs F, int64_t n_prob) {
  constexpr int FG = 16;
  const int gl = threadIdx.x & (FG - 1);
  const int64_t groups_total = (int64_t)gridDim.x * (blockDim.x / FG);
  for (int64_t p = (int64_t)blockIdx.x * (blockDim.x / FG) + threadIdx.x / FG; p < n_prob; p += groups_total) {
    const KswProb pr = F.probs[p];
    const FaSrc sr = F.srcs[p];
    const int32_t src = F.seq_src[sr.aln];
    const uint32_t s0 = F.seq_off[src], seq_len = F.seq_off[src + 1] - s0;
    const uint8_t *seq = F.seqs + s0;
    uint8_t *qd = F.seq_arena + pr.seq_off, *td = qd + pr.qlen;
    const bool left = pr.side == 0;
    for (uint32_t j = (uint32_t)gl; j < pr.qlen; j += FG) qd[j] = base_code(left ? seq[pr.qlen - 1 - j] : seq[seq_len - pr.qlen + j]);
    const uint4 *E = tx_ex + sr.e_base;
    uint32_t t = 0, has_n = 0;
    for (uint32_t i = sr.i_from; t < pr.tlen;) {
      const uint4 e = E[i];
      if (!left && e.x == 0xffffffffu) break;
      const uint32_t len = e.y - e.x, take = len < pr.tlen - t ? len : pr.tlen - t;
      const uint8_t *sq = seq_pool + e.w;
      for (uint32_t b = (uint32_t)gl; b < take; b += FG) { const uint8_t cd = base_code(left ? sq[len - 1 - b] : sq[b]); has_n |= cd >> 2; td[t + b] = cd; }
      t += take;
      if (left) { if (i == 0) break; i--; } else i++;
    }
    has_n = wave_or<uint32_t, FG>(has_n);
    if (gl == 0 && has_n) F.probs[p].t_has_n = 1;
  }
}
