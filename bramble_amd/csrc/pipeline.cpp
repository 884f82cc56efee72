// run_device: the HIP projection pipeline over a device-resident batch (small / speculative, direct rows, match table,
// -S), the -S rescue DP, and what is derived from the last call's rows (detail column, wide view, counters).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"

// the side stream for kernels that can run beside the main one (a shape's tracebacks beside the next shape's DP; the
// few-block emit kernel of the > 64-candidate alignments beside the work-list kernels), with the events of every SideWork;
// it and the second one (side2_stream) are of normal priority (0)
int ensure_side_stream(br_ctx *c) {
  if (c->side_stream) return BR_OK;
  HIPCHK(hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, 0));
  for (auto &p : c->side_ev) for (auto &e : p) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return BR_OK;
}

// The -S rescue DP over n_prob problems.  Problems whose target fits a register array go
// through the streamed kernels piece by piece (a piece = a range of problems whose direction tape fits the budget):
// k_ksw_bin -> [host reads the bin sizes] -> k_ksw_plan -> k_ksw_dp per bin -> k_ksw over the leftovers -> k_ksw_trace.
int run_ksw(br_ctx *c, hipStream_t st, const KswRun &R) {
  if (R.n_prob <= 0) return BR_OK;
  const uint64_t n_all = (uint64_t)R.n_prob;
  const uint64_t qmax = std::max<uint64_t>(R.qmax, 1), tmax = std::max<uint64_t>(R.tmax, 1);
  KswArgs K{};
  K.n_prob = R.n_prob; K.probs = R.probs; K.results = R.results; K.seq_arena = R.seq_arena; K.clip_ops = R.clip_ops;
  K.stats = R.stats;
  K.raw_out = R.raw_out; K.raw_n = R.raw_n; K.max_out = R.max_out; K.raw_cap = R.raw_cap;
  // the general kernel: per-wave scratch = direction matrix + raw traceback ops + (large targets) u / v / x / y, sized by the
  // longest query / target it will see.  16 GB are set aside; one outlier (a 100 kb soft clip) may take more: then a single
  // wave runs, as long as its matrix fits in 60 % of the free HBM
  auto general = [&](uint64_t n_work, uint64_t q_hi, uint64_t t_hi, const uint32_t *list, const uint32_t *n_list) -> int {
    q_hi = std::max<uint64_t>(q_hi, 1); t_hi = std::max<uint64_t>(t_hi, 1);
    K.tmax = (uint32_t)t_hi;
    K.pmat_bytes = (size_t)(((q_hi + t_hi) * t_hi + 15) & ~15ull);
    K.raw_words = (size_t)((q_hi + t_hi + 4 + 3) & ~3ull);
    K.scratch_per_wave = K.pmat_bytes + K.raw_words * 4 + ((4 * t_hi + 15) & ~15ull);
    const uint64_t budget = 16ull << 30;
    uint64_t waves = std::min<uint64_t>({(uint64_t)c->n_cu * 16, budget / K.scratch_per_wave, n_work});
    if (waves == 0) {
      size_t free_b = 0, total_b = 0;
      HIPCHK(hipMemGetInfo(&free_b, &total_b));
      if ((double)K.scratch_per_wave > 0.6 * (double)(free_b + c->fa_scratch.cap)) return BR_ERR_CAPACITY;
      waves = 1;
    }
    RC(c->fa_scratch.ensure((size_t)waves * K.scratch_per_wave));
    K.scratch = c->fa_scratch.as<uint8_t>(); K.list = list; K.n_list = n_list; K.n_waves = (int64_t)waves;
    launch_ksw(st, K, (int)((waves + 3) / 4));
    return BR_OK;
  };
  memset(c->ksw_diag, 0, sizeof(c->ksw_diag));
  c->rb->ksw_left_after = 0;
  if (!c->ksw_fast) return general(n_all, qmax, tmax, nullptr, nullptr);

  RC(c->ksw_raw.ensure((size_t)(R.seq_total + n_all + 1) * 4));
  RC(c->ksw_cnt.ensure(128));
  RC(ensure_side_stream(c));
  uint32_t *h_cnt = c->rb->ksw_bins;
  const uint64_t tape_budget = (uint64_t)c->ksw_tape_mb << 20;
  // groups of a bin = what is resident at once (one wave of blocks: every group runs from the first cycle)
  uint32_t max_groups[KSW_N_BINS];
  for (int b = 0; b < KSW_N_BINS; b++) {
    if (!c->ksw_groups[b]) c->ksw_groups[b] = ksw_dp_resident_groups(b, c->n_cu);
    max_groups[b] = c->ksw_groups[b];
  }
  std::vector<std::pair<uint64_t, uint64_t>> todo;   // [p0, p1)
  todo.emplace_back(0, n_all);
  while (!todo.empty()) {
    const uint64_t p0 = todo.back().first, p1 = todo.back().second, n = p1 - p0;
    todo.pop_back();
    RC(c->ksw_desc.ensure((size_t)n * sizeof(KswDesc) * KSW_N_BINS));
    RC(c->ksw_dp.ensure((size_t)n * sizeof(KswDp)));
    RC(c->ksw_left.ensure((size_t)n * 4));
    KswFastArgs A{};
    A.p0 = (int64_t)p0; A.n = (int64_t)n; A.probs = R.probs; A.results = R.results; A.seq_arena = R.seq_arena;
    A.clip_ops = R.clip_ops; A.raw_ops = c->ksw_raw.as<uint32_t>();
    for (int b = 0; b < KSW_N_BINS; b++) A.desc[b] = c->ksw_desc.as<KswDesc>() + (size_t)b * n;
    A.counters = c->ksw_cnt.as<uint32_t>(); A.leftover = c->ksw_left.as<uint32_t>(); A.dp = c->ksw_dp.as<KswDp>();
    A.stats = R.stats; A.raw_out = R.raw_out; A.raw_n = R.raw_n; A.max_out = R.max_out; A.raw_cap = R.raw_cap;
    HIPCHK(hipMemsetAsync(c->ksw_cnt.p, 0, 128, st));
    launch_ksw_bin(st, A);
    HIPCHK(hipMemcpyAsync(h_cnt, c->ksw_cnt.p, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t *h_rows = (const uint64_t *)(h_cnt + 8);
    // tape: a row = one step of a wave (512 or 1024 B); a bin's waves run (tape rows of its problems) / (groups per wave) steps when
    // its groups stay equally busy (they share one queue), 15 % on top, and every wave rounds up to chunks and drains
    uint64_t tape_bytes = 0, tape_fixed = 0; uint32_t n_groups_total = 0;   // tape_fixed: what every wave rounds up and drains, whatever the piece holds
    for (int b = 0; b < KSW_N_BINS; b++) {
      A.n_bin[b] = h_cnt[b];
      A.n_groups[b] = std::min<uint32_t>(max_groups[b], (h_cnt[b] + 7u) / 8u);   // a group takes its problems eight at a time
      n_groups_total += A.n_groups[b];
      const uint64_t gpw = 64u / (uint64_t)KSW_BIN_G(b), waves = (A.n_groups[b] + gpw - 1) / gpw;
      const uint64_t fixed = waves * (1ull * KSW_CHUNK_ROWS + KSW_BIN_W(b) + 64);
      const uint64_t rows = h_rows[b] / gpw + h_rows[b] / gpw / 7 + fixed;
      if (A.n_bin[b]) { tape_bytes += rows * (uint64_t)KSW_BIN_ROWBYTES(b); tape_fixed += fixed * (uint64_t)KSW_BIN_ROWBYTES(b); }
    }
    if (tape_bytes > tape_budget && n >= 2048) {
      // as few pieces as fit: the part of the tape that scales with the problems over what a piece has left for it (halves
      // when the fixed part alone nearly fills the budget); a piece that still does not fit is cut again
      uint64_t k = 2;
      if (tape_budget > tape_fixed + tape_fixed / 4) k = ((tape_bytes - tape_fixed) + (tape_budget - tape_fixed) - 1) / (tape_budget - tape_fixed);
      k = std::min<uint64_t>(std::max<uint64_t>(k, 2), std::min<uint64_t>(64, n / 1024));
      for (uint64_t i = k; i-- > 0;) todo.emplace_back(p0 + n * i / k, p0 + n * (i + 1) / k);
      continue;
    }
    const uint32_t n_left = h_cnt[KSW_N_BINS];
    SideWork traces(c, st, c->side_stream);
    c->ksw_diag[0]++;
    for (int b = 0; b < KSW_N_BINS; b++) c->ksw_diag[1 + b] += h_cnt[b];
    c->ksw_diag[5] += n_left; c->ksw_diag[6] = std::max<uint64_t>(c->ksw_diag[6], tape_bytes);
    for (int b = 0; b < KSW_N_BINS; b++) c->ksw_diag[8 + b] += h_rows[b];
    if (n_groups_total) {
      RC(c->ksw_tape.ensure((size_t)tape_bytes + 256));
      A.tape = c->ksw_tape.as<uint8_t>(); A.tape_cap = tape_bytes / 100 * (uint64_t)c->ksw_tape_pct;
      // a shape's tracebacks (one lane per problem, waiting on tape lines) run on the side stream beside the next shape's
      // DP kernel (issue-bound, one wave of registers to spare per SIMD)
      for (int b = KSW_N_BINS - 1; b >= 0; b--) {     // widest shape first: the exposed last traceback is the smallest shape's
        if (!A.n_bin[b]) continue;
        launch_ksw_dp(st, A, b);
        RC(traces.fork());
        launch_ksw_trace(c->side_stream, A, b);
      }
      RC(traces.done());
    }
    // what the arrays do not take: targets beyond the widest array, and (never seen outside tests) groups whose tape ran out
    // (problems a wave hands back when the tape runs out come from the arrays: at most KSW_MAX_SPAN bases)
    RC(general(n_left ? n_left : 64, std::max<uint64_t>(h_cnt[5], KSW_MAX_SPAN), std::max<uint64_t>(h_cnt[6], KSW_BIN_W(KSW_N_BINS - 1)), A.leftover, A.counters + KSW_N_BINS));
    if (n_groups_total) RC(traces.join());   // the tape and the result arrays are free again
    // leftovers after the DP (those of the last piece; read by br_ctx_ksw_diag once the stream has been synchronised)
    HIPCHK(hipMemcpyAsync(&c->rb->ksw_left_after, A.counters + KSW_N_BINS, 4, hipMemcpyDeviceToHost, st));
  }
  return BR_OK;
}

// ---- what the three pipelines share: the segment stage, the tables and arguments of the count pass, its launch, the match
// table's arguments and emit pass, pairing's arguments, the row tables, the row tail and the end of a call ----
// a1/a2/a6: CIGAR -> read exons (X: what the small route has the kernel do on the side)
static int segment_stage(br_ctx *c, hipStream_t st, const DevCfg &dc, const br_device_batch *b, Prof &pf, const SegExtra *X = nullptr) {
  RC(pf.begin(BR_K_SEGMENT));
  launch_segment(st, b->n_aln, b->ref_id, b->ref_start, b->flags, b->xs, b->ts, b->cigar_off, b->cigar, dc, c->ix->n_refs,
                 c->seg.as<uint2>(), c->meta.as<AlnMeta>(), c->head.as<uint4>(), c->head2.as<uint4>(), c->fast_flag.as<uint32_t>(), X);
  RC(pf.end());
  return BR_OK;
}

static int ensure_count_tables(br_ctx *c, const br_device_batch *b) {
  const int64_t n = b->n_aln;
  RC(c->seg.ensure((size_t)(b->n_cigar_words + n) * sizeof(uint2)));
  RC(c->meta.ensure((size_t)n * sizeof(AlnMeta))); RC(c->head.ensure((size_t)n * sizeof(uint4))); RC(c->head2.ensure((size_t)n * sizeof(uint4)));
  RC(c->fast_flag.ensure((size_t)n * 4)); RC(c->ranges.ensure((size_t)n * sizeof(uint4))); RC(c->mask.ensure((size_t)n * 8));
  RC(c->cig_base.ensure((size_t)(n + 1) * 8)); RC(c->big_list.ensure((size_t)n * 4)); RC(ensure_totals(c));
  return BR_OK;
}

// (n_matches is sized by the caller)
static ProjectArgs count_args(br_ctx *c, const DevCfg &dc, const br_device_batch *b) {
  ProjectArgs A{};
  A.ix = c->ix->dev; A.cfg = dc; A.n_aln = b->n_aln; A.ref_id = b->ref_id; A.cigar_off = b->cigar_off; A.cigar = b->cigar;
  A.seg = c->seg.as<uint2>(); A.meta = c->meta.as<AlnMeta>(); A.head = c->head.as<uint4>(); A.head2 = c->head2.as<uint4>();
  A.fast_flag = c->fast_flag.as<uint32_t>(); A.n_matches = c->n_matches.as<uint32_t>();
  A.ranges = c->ranges.as<uint4>(); A.mask = c->mask.as<uint64_t>(); A.big_list = c->big_list.as<uint32_t>();
  return A;
}

// what the split count pass reads and writes (A's other fields are the emit pass's)
static CountArgs count_view(const ProjectArgs &A) {
  CountArgs C{};
  const DevIndex &ix = A.ix;
  C.slab_off = ix.slab_off; C.bin_off = ix.bin_off; C.s_start = ix.s_start; C.s_pmax = ix.s_pmax;
  C.t_bin = ix.t_bin; C.s_row = ix.s_row; C.tx_ex = ix.tx_ex; C.n_refs = ix.n_refs; C.bin_shift = ix.bin_shift;
  C.max_clip = A.cfg.max_clip; C.max_junc_ins = A.cfg.max_junc_ins; C.max_junc_gap = A.cfg.max_junc_gap;
  C.max_error_exon = A.cfg.max_error_exon; C.ignore_small_exons = A.cfg.ignore_small_exons; C.long_reads = A.cfg.long_reads;
  C.n_aln = (uint32_t)A.n_aln;   // (br_batch_prepare: < 2^31; the work lists hold 32-bit alignment numbers)
  C.head = A.head; C.head2 = A.head2; C.cigar_off = A.cigar_off; C.seg = A.seg;
  C.n_matches = A.n_matches; C.mask = A.mask; C.ranges = A.ranges;
  C.walk_list = A.walk_list; C.n_walk = A.n_walk; C.big_list = A.big_list; C.n_big = A.n_big;
  return C;
}

// the count pass: one kernel with the exon walk inline, or (split: presets without the similarity filter) the main kernel
// without it and a second one for the alignments it put on A.walk_list.  light (direct rows): the main kernel moves the
// light two-exon alignments into the simple class (fast_flag)
static int count_pass(br_ctx *c, hipStream_t st, const ProjectArgs &A, Prof &pf, bool split, bool light = false) {
  const int n_blocks = c->n_cu * c->blocks_per_cu;
  if (!split || A.ix.n_rows == 0) {   // (an empty annotation: launch_project zeroes the counts)
    RC(pf.begin(BR_K_COUNT));
    launch_project(st, A, false, c->group_lanes, n_blocks);
    RC(pf.end());
    return BR_OK;
  }
  CountArgs C = count_view(A);
  if (light) C.light_flag = const_cast<uint32_t *>(A.fast_flag);
  RC(pf.begin(BR_K_COUNT));
  launch_count(st, C, c->group_lanes, n_blocks, 1);
  RC(pf.end());
  RC(pf.begin(BR_K_COUNT_WALK));
  launch_count(st, C, c->group_lanes, n_blocks, 2);
  RC(pf.end());
  return BR_OK;
}

// what the three-value scan reads (matches per alignment; CIGAR sizes from the exon heads; the simple class)
static ScanArgs scan3_args(br_ctx *c, const br_device_batch *b) {
  ScanArgs S{};
  S.n = b->n_aln; S.src32 = c->n_matches.as<uint32_t>(); S.cigar_off = b->cigar_off;
  S.tile_sums = c->tile_sums.as<uint64_t>(); S.fast_flag = c->fast_flag.as<uint32_t>();
  return S;
}

// the match table's emit pass over a work list of n_list entries: without the similarity filter, its simple prefix (one
// read exon from a single M op, n_simple entries) and the rest as two launches; with it, the whole list in one
static int emit_match_table(hipStream_t st, const ProjectArgs &A, Prof &pf, int64_t n_list, int64_t n_simple) {
  if (!A.cfg.filter_by_similarity) {
    RC(pf.begin(BR_K_EMIT_SIMPLE));
    launch_emit_dense(st, A, n_list, n_simple, 1);
    RC(pf.end());
    RC(pf.begin(BR_K_EMIT));
    launch_emit_dense(st, A, n_list, n_simple, 2);
    RC(pf.end());
  } else {
    RC(pf.begin(BR_K_EMIT));
    launch_emit_dense(st, A, n_list, -1, 0);
    RC(pf.end());
  }
  return BR_OK;
}

// the match table for n_m matches and the CIGAR arena for n_c words (0: as earlier calls left them), and A pointed at them
static int match_tables(br_ctx *c, ProjectArgs &A, uint64_t n_m, uint64_t n_c) {
  if (n_m) {
    RC(c->m_tid.ensure(n_m * 4)); RC(c->m_aux.ensure(n_m * 4)); RC(c->m_p.ensure(n_m * sizeof(uint2))); RC(c->m_x.ensure(n_m * sizeof(uint2)));
    RC(c->m_b.ensure(n_m * sizeof(uint4))); RC(c->m_cigoff.ensure(n_m * 8)); RC(c->m_aln.ensure(n_m * 4));
    RC(c->cig_arena.ensure(n_c * 4));
  }
  A.m_aln = c->m_aln.as<uint32_t>(); A.m_tid = c->m_tid.as<uint32_t>(); A.m_aux = c->m_aux.as<uint32_t>(); A.m_p = c->m_p.as<uint2>();
  A.m_x = c->m_x.as<uint2>(); A.m_b = c->m_b.as<uint4>(); A.m_cigoff = c->m_cigoff.as<uint64_t>(); A.cig_arena = c->cig_arena.as<uint32_t>();
  return BR_OK;
}

// the dense-locus kernel (alignments with > 64 candidate rows: a few long-running blocks) on the side stream beside the
// emit classes of the work list; expand: the work list is written first, beside it too
static int emit_beside_dense(br_ctx *c, hipStream_t st, const ProjectArgs &A, Prof &pf, int64_t n_list, int64_t n_simple, bool expand) {
  RC(ensure_side_stream(c));
  SideWork dense(c, st, c->side_stream);
  RC(dense.fork());
  RC(pf.begin(BR_K_EMIT_AUX, c->side_stream));
  launch_project(c->side_stream, A, true, 64, c->n_cu);
  RC(pf.end());
  RC(dense.done());
  if (expand) {
    RC(pf.begin(BR_K_EXPAND));
    launch_expand(st, A);
    RC(pf.end());
  }
  RC(emit_match_table(st, A, pf, n_list, n_simple));
  return dense.join();
}

// a16/a17: what pairing reads (the match table of A) and writes (per-alignment record counts and offsets, pair bits); the
// per-alignment tables are sized here, the counters are the context's block
static int pair_args(br_ctx *c, const DevCfg &dc, const br_device_batch *b, const ProjectArgs &A, PairArgs &P) {
  const int64_t n = b->n_aln;
  RC(c->pmask.ensure((size_t)n * 8)); RC(c->pbit.ensure((size_t)n));
  P = PairArgs{};
  P.n_groups = b->n_groups; P.n_aln = n; P.long_reads = dc.long_reads; P.group_off = b->group_off; P.mate_idx = b->mate_idx;
  P.aln_group = c->aln_group.as<uint32_t>();
  P.match_off = c->match_off.as<uint32_t>(); P.n_matches = c->n_matches.as<uint32_t>(); P.m_tid = A.m_tid; P.m_p = A.m_p; P.m_x = A.m_x; P.m_b = A.m_b;
  P.m_cigoff = A.m_cigoff;
  P.n_rows = c->n_rows.as<uint32_t>(); P.row_off = c->row_off.as<uint64_t>(); P.counters = c->counters_d.as<uint64_t>();
  P.pmask = c->pmask.as<uint64_t>(); P.pbit = c->pbit.as<uint8_t>();
  return BR_OK;
}

// k_pair<false>, and its record counts scanned into row_off and TOT_ROWS (wait_busy: a packed download of the previous call
// may still be reading row_off / the row tables, br_project_staged)
static int pair_count(br_ctx *c, hipStream_t st, const PairArgs &P, Prof &pf, bool wait_busy) {
  RC(pf.begin(BR_K_PAIR_COUNT));
  launch_pair(st, P, false);
  RC(pf.end());
  if (wait_busy) HIPCHK(hipStreamWaitEvent(st, c->rows_busy, 0));
  RC(pf.begin(BR_K_SCAN));
  launch_scan(st, P.n_rows, P.n_aln, c->tile_sums.as<uint64_t>(), c->row_off.p, true, c->totals.as<uint64_t>() + TOT_ROWS);
  RC(pf.end());
  return BR_OK;
}

// the row tables for n_rows records (grow: sized here -- a buffer that a queued packed download still reads must not be
// reallocated under it), and P pointed at them.  The clip score / similarity score columns exist only when the preset
// filters by similarity (long reads): else all zero
static int row_tables(br_ctx *c, PairArgs &P, uint64_t n_rows, bool aux_cols, bool grow) {
  if (grow) {
    const size_t nr = (size_t)std::max<uint64_t>(n_rows, 1);
    if (c->rows_busy_set && (c->pk_a.cap < nr * sizeof(uint4) || (aux_cols && (c->pk_sim.cap < nr * 8 || c->pk_clip.cap < nr * 4))))
      HIPCHK(hipEventSynchronize(c->rows_busy));
    RC(c->r_rec.ensure(nr * sizeof(uint4)));
    RC(c->pk_a.ensure(nr * sizeof(uint4))); RC(c->pk_c.ensure(nr * sizeof(uint2)));
    if (aux_cols) { RC(c->pk_sim.ensure(nr * 8)); RC(c->pk_clip.ensure(nr * 4)); }
  }
  P.n_rows_total = (int64_t)n_rows; P.r_rec = c->r_rec.as<uint4>();
  P.r_a = c->pk_a.as<uint4>(); P.r_c = c->pk_c.as<uint2>(); P.r_x = nullptr;
  P.r_sim = aux_cols ? c->pk_sim.as<double>() : nullptr; P.r_clip = aux_cols ? c->pk_clip.as<int32_t>() : nullptr;
  return BR_OK;
}

// The row tail: k_pair<true> -> k_primary -> k_rows.  Presets without scores: the primary choice (ALU: the mt19937_64
// seeding chain) needs row_off and the pair bits only, so it runs before the records exist -- on the side stream beside the
// emit pass of k_pair when `side` -- and leaves its pick for k_rows; with scores it follows the emit pass.  have_rows: false
// when the host knows that there are none (the kernels that need records are not launched).  host_cap: the caller wants
// the few rows of a small call on the host (br_project_group) -- the row kernel writes the packed rows and their detail
// column straight into pinned host memory of that many records: no download, no second wait
static int row_tail(br_ctx *c, hipStream_t st, const br_device_batch *b, PairArgs &P, Prof &pf, bool aux_cols, bool side,
                    bool have_rows, uint64_t host_cap) {
  c->rows_at_host = false;
  if (host_cap) {
    RC(c->g_a.resize(host_cap)); RC(c->g_c.resize(host_cap)); RC(c->g_x.resize(host_cap));
    if (aux_cols) RC(c->g_sim.resize(host_cap));
    P.r_a = c->g_a.p; P.r_c = c->g_c.p; P.r_x = c->g_x.p;
    if (aux_cols) P.r_sim = c->g_sim.p;
    c->rows_at_host = true;
  }
  const uint8_t *names = (b->names && b->name_off) ? b->names : nullptr;
  if (side) RC(ensure_side_stream(c));
  SideWork choice(c, st, c->side_stream);
  if (!aux_cols) {
    RC(c->pick.ensure((size_t)std::max<int64_t>(b->n_groups, 1) * 8)); P.pick = c->pick.as<uint64_t>();
    if (side) RC(choice.fork());
    RC(pf.begin(BR_K_PRIMARY, side ? c->side_stream : st));
    launch_primary(side ? c->side_stream : st, P, b->name_off, names, false);   // + per-group counters
    RC(pf.end());
    if (side) RC(choice.done());
  }
  if (have_rows) {
    RC(pf.begin(BR_K_PAIR_EMIT));
    launch_pair(st, P, true);
    RC(pf.end());
  }
  if (!aux_cols) { if (side) RC(choice.join()); }
  else {
    RC(pf.begin(BR_K_PRIMARY));
    launch_primary(st, P, b->name_off, names, true);   // + per-group counters
    RC(pf.end());
  }
  if (have_rows) {
    RC(pf.begin(BR_K_ROWS));
    launch_rows(st, P, aux_cols);
    RC(pf.end());
  }
  return BR_OK;
}

// the counts of a finished call (rb->counters: unique reads, dropped reads) and what the context keeps of it; P: the row
// tables of the match-table routes (the direct route passes its own)
static void finish_call(br_ctx *c, const DevCfg &dc, const br_device_batch *b, br_device_rows *out, uint64_t n_matches,
                        uint64_t n_rows, uint64_t n_pool, bool aux_cols, const PairArgs *P = nullptr) {
  out->n_matches = (int64_t)n_matches; out->n_rows = (int64_t)n_rows; out->n_pool_words = (int64_t)n_pool;
  out->total_complete = n_rows; out->total_unique = c->rb->counters[1]; out->dropped_reads = c->rb->counters[2];
  out->pool = c->cig_arena.as<uint32_t>(); out->row_off = c->row_off.as<uint64_t>();
  c->counters[6] = n_matches;
  c->last_n_rows = (int64_t)n_rows; c->last_n_aln = b->n_aln; c->last_n_pool = (int64_t)n_pool;
  c->last_aux_cols = aux_cols; c->wide_valid = false; c->detail_valid = false; c->last_l_qseq = b->l_qseq; c->last_long_reads = dc.long_reads;
  c->last_direct = false;   // (run_device_direct says otherwise after this)
  if (P) {
    out->a = (const br_row_a *)P->r_a; out->cigar = (const uint64_t *)P->r_c; out->x = (const br_row_x *)P->r_x;   // (null: br_device_rows_detail)
    out->similarity_score = P->r_sim; out->clip_score = P->r_clip;
  }
}

// Small batches (a read-name group, the 64 groups a bramble-cli worker holds, the 100 k alignments of a reference bundle):
// the ordinary pipeline stops three times for the host to read a total and size the next tables, and launches about
// twenty kernels -- for 10 k alignments that is 0.3 ms of which the kernels are a fraction.  Here the tables are sized from
// upper bounds (32 matches per alignment and the CIGAR room that goes with them), the scan totals stay on the device
// (ProjectArgs::tot: the kernels that need a count read it there, and do nothing when a total is beyond its table), the
// split kernels run in their single-launch forms, everything goes down ONE stream, and the host waits once, at the end.
// A batch that does not fit the bounds (a dense locus) comes back as BR_RETRY_ORDINARY and takes the ordinary path.
// LARGE batches take the same route when the context has projected a batch before (`big`): the tables are what earlier calls
// left behind (grown with a quarter of headroom), the launch grids of the two emit classes and of the row kernel come from
// the LAST call's counts scaled to this batch's size (+15 %), the kernels keep their split, two-stream forms -- and the
// host, instead of stopping three times, checks once at the end that nothing outgrew its table or its grid.  A batch that
// did is redone the ordinary way, which also grows the tables.
static int run_device_small(br_ctx *c, const DevCfg &dc, const br_device_batch *b, hipStream_t st, br_device_rows *out, Prof &pf,
                            bool keep_events, bool big) {
  const int64_t n = b->n_aln, ng = b->n_groups;
  const bool aux_cols = dc.filter_by_similarity != 0;
  uint64_t cap_m = 32ull * (uint64_t)n + 8192;
  const uint64_t per = 9ull * (uint64_t)std::min<int32_t>(std::max<int32_t>(b->max_n_cigar, 4), 64) + 12ull;   // n_real + 2 (4 n_seg + 2) <= 9 n_cigar + 12
  uint64_t cap_c = std::min<uint64_t>(cap_m * per, 1ull << 28);
  uint64_t cap_r = cap_m, cover_m = cap_m, cover_s = cap_m, cover_g = cap_m, cover_r = cap_m;   // tables' capacities; what the emit / row grids cover (all matches, simple class, general class, records)
  if (big) {
    const double f = 1.15 * (double)n / (double)std::max<int64_t>(c->hist_n, 1);
    cover_m = (uint64_t)(f * (double)c->hist[0]) + 4096; cover_s = (uint64_t)(f * (double)c->hist[2]) + 4096; cover_r = (uint64_t)(f * (double)c->hist[3]) + 4096;
    cover_g = (uint64_t)(f * (double)(c->hist[0] - std::min(c->hist[0], c->hist[2]))) + 4096;
    const uint64_t need_c = (uint64_t)(f * (double)c->hist[1]) + 4096;
    cap_m = std::min<uint64_t>({c->m_tid.cap / 4, c->m_aux.cap / 4, c->m_p.cap / 8, c->m_x.cap / 8, c->m_b.cap / 16, c->m_cigoff.cap / 8, c->m_aln.cap / 4});
    cap_c = c->cig_arena.cap / 4;
    cap_r = std::min<uint64_t>({c->r_rec.cap / 16, c->pk_a.cap / 16, c->pk_c.cap / 8});
    if (aux_cols) cap_r = std::min<uint64_t>({cap_r, c->pk_sim.cap / 8, c->pk_clip.cap / 4});
    if (cover_m > cap_m || need_c > cap_c || cover_r > cap_r) return BR_RETRY_ORDINARY;   // the tables have to grow: the ordinary path does that
  }
  const int64_t tiles = std::max<int64_t>(scan_tiles_for(std::max<int64_t>(n, ng) + 1), 1);
  RC(ensure_count_tables(c, b));
  RC(c->n_matches.ensure((size_t)n * 4)); RC(c->fast_pre.ensure((size_t)(n + 1) * 4)); RC(c->match_off.ensure((size_t)(n + 1) * 4));
  RC(c->tile_sums.ensure((size_t)tiles * 8 * 3)); RC(c->counters_d.ensure(GD_COUNTER_WORDS * 8)); RC(c->n_big.ensure(16));
  // a queued packed download of the last call (br_project_staged) may still read the row tables: small batches wait for it here;
  // large ones keep the overlap -- their tables are not reallocated (checked above) -- and make the row scan wait instead
  const bool rows_busy_wait = c->rows_busy_set && big && c->row_off.cap >= (size_t)(n + 1) * 8;
  if (c->rows_busy_set && !rows_busy_wait) HIPCHK(hipEventSynchronize(c->rows_busy));
  RC(c->n_rows.ensure((size_t)n * 4)); RC(c->row_off.ensure((size_t)(n + 1) * 8)); RC(c->aln_group.ensure((size_t)n * 4));
  if (big) RC(c->walk_list.ensure((size_t)n * 4));
  uint64_t *d_tot = c->totals.as<uint64_t>();

  // (the per-batch counters sit behind the totals: one download brings both home; k_segment zeroes them and the two
  // work-list counters, and labels the alignments with their read-name groups)
  uint64_t *d_cnt = d_tot + TOT_SMALL_CNT;
  SegExtra X{};
  X.group_off = b->group_off; X.aln_group = c->aln_group.as<uint32_t>(); X.n_groups = ng;
  X.zero_a = (uint64_t *)c->n_big.p; X.n_zero_a = 1; X.zero_b = d_cnt; X.n_zero_b = 4;
  RC(segment_stage(c, st, dc, b, pf, &X));
  ProjectArgs A = count_args(c, dc, b);
  A.fast_pre = c->fast_pre.as<uint32_t>(); A.match_off = c->match_off.as<uint32_t>(); A.cig_base = c->cig_base.as<uint64_t>();
  A.n_big = c->n_big.as<uint32_t>();
  RC(match_tables(c, A, big ? 0 : cap_m, cap_c));   // (big: checked above)
  A.tot = d_tot; A.lim_m = cap_m; A.lim_c = cap_c;
  const bool split = big && !dc.filter_by_similarity;   // (small: one kernel, the exon walk inline)
  if (split) { A.walk_list = c->walk_list.as<uint32_t>(); A.n_walk = c->n_big.as<uint32_t>() + 1; }
  RC(count_pass(c, st, A, pf, split));
  ScanArgs S = scan3_args(c, b);
  RC(pf.begin(BR_K_SCAN));
  const bool expanded = launch_scan3(st, S, c->match_off.as<uint32_t>(), c->cig_base.as<uint64_t>(), c->fast_pre.as<uint32_t>(), d_tot + TOT_MATCHES, &A);
  RC(pf.end());
  if (!expanded) {
    RC(pf.begin(BR_K_EXPAND));
    launch_expand(st, A);
    RC(pf.end());
  }
  if (!big) {
    RC(pf.begin(BR_K_EMIT));
    launch_emit_dense(st, A, (int64_t)cover_m, -1, 0);          // one launch over the whole list; the kernel stops at TOT_MATCHES
    launch_project(st, A, true, 64, std::min(c->n_cu, 64));     // alignments with > 64 candidate rows (reads *n_big)
    RC(pf.end());
  } else {
    // as the ordinary path, over the grids of the predictions: cover_s + cover_g entries of the two classes, or cover_m of the whole list
    RC(emit_beside_dense(c, st, A, pf, (int64_t)(dc.filter_by_similarity ? cover_m : cover_s + cover_g), (int64_t)cover_s, false));
  }

  PairArgs P;
  RC(pair_args(c, dc, b, A, P));
  P.counters = d_cnt; P.tot = d_tot; P.lim_m = cap_m; P.lim_c = cap_c; P.lim_r = std::min(cap_r, cover_r);
  RC(pair_count(c, st, P, pf, rows_busy_wait));
  // (small: the row tables of the upper bound, lim_r = cap_m; big: the ones earlier calls left, checked above; the record
  // count stays on the device: every launch of the tail is made)
  RC(row_tables(c, P, P.lim_r, aux_cols, !big));
  RC(row_tail(c, st, b, P, pf, aux_cols, big, true, c->rows_to_host ? cap_m : 0));
  ReadBack *rb = c->rb;
  HIPCHK(hipMemcpyAsync(rb->small, d_tot, sizeof(rb->small), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < 4; k++) { rb->scan[k] = rb->small[k]; rb->counters[k] = rb->small[TOT_SMALL_CNT + k]; }
  const uint64_t n_matches = rb->scan[TOT_MATCHES], n_cig_arena = rb->scan[TOT_ARENA], n_simple = rb->scan[TOT_SIMPLE], n_rows = rb->scan[TOT_ROWS];
  // nothing was written past a table or left out by a grid: the kernels checked the same totals and did nothing then
  if (n_matches > cap_m || n_cig_arena > cap_c || n_rows > P.lim_r) return BR_RETRY_ORDINARY;
  if (big && (!dc.filter_by_similarity ? (n_simple > cover_s || n_matches - n_simple > cover_g) : n_matches > cover_m)) return BR_RETRY_ORDINARY;
  c->hist_simf = dc.filter_by_similarity != 0;
  c->hist_n = n; c->hist[0] = n_matches; c->hist[1] = n_cig_arena; c->hist[2] = n_simple; c->hist[3] = n_rows;
  if (!keep_events) RC(pf.collect());
  if (rb->counters[3]) return BR_ERR_UNSUPPORTED;  // a rewritten CIGAR with more than 2^24 - 1 ops
  finish_call(c, dc, b, out, n_matches, n_rows, n_cig_arena, aux_cols, &P);
  return BR_OK;
}

// Direct rows: presets without the similarity filter and without -S (every short-read preset; long reads with the filter
// switched off).  segment -> count -> [k_pair_mask || k_big<0> + k_pair_big] -> k_scan5 (one host wait: sizes) ->
// k_expand_rows -> k_emit_rows (|| k_big<1>): the packed rows are written once, by the lane that computes the match; the
// match table, the per-record r_rec, k_pair<true> and k_rows do not exist on this path.  On the side streams: the name
// seeds of the primary tie-break (beside k_pair_mask), the big alignments' pairing (beside k_pair_mask), k_group_desc
// (beside the scan), k_big<1> (beside the emit kernels).
static int run_device_direct(br_ctx *c, const DevCfg &dc, const br_device_batch *b, hipStream_t st, br_device_rows *out, Prof &pf,
                             bool keep_events) {
  const br_index *ix = c->ix;
  const int64_t n = b->n_aln, ng = b->n_groups;
  const int64_t tiles = std::max<int64_t>(scan_tiles_for(std::max<int64_t>(n, ng) + 1), 1);
  RC(ensure_count_tables(c, b));
  RC(c->n_matches.ensure((size_t)n * 4 + 16));   // (+ 16: k_group_desc reads four elements at a time)
  RC(c->tile_sums.ensure((size_t)tiles * 8 * 5));   // (k_scan5: five sums per tile)
  // every small counter of the step in one block, zeroed by one fill at the start: [0, GD_COUNTER_WORDS) the four counters + k_group_desc's
  // slots, then the side arena's two words, then n_big | n_walk | pm_n | -
  RC(c->counters_d.ensure((GD_COUNTER_WORDS + 4) * 8));
  uint64_t *const dz = c->counters_d.as<uint64_t>();
  uint32_t *const dz_nbig = (uint32_t *)(dz + GD_COUNTER_WORDS + 2);
  RC(c->walk_list.ensure((size_t)n * 4));
  RC(c->aln_group.ensure((size_t)n * 4)); RC(c->n_rows.ensure((size_t)n * 4 + 16)); RC(c->pbit.ensure((size_t)n + 16));
  RC(c->d_fm.ensure((size_t)n * sizeof(uint2) + (size_t)(n / 62 + 2) * 4));   // + the window list of k_pair_mask
  RC(c->d_nkept.ensure((size_t)n * 4)); RC(c->d_desc.ensure((size_t)n * sizeof(uint4)));
  if (c->emit_rank_tids) RC(c->d_kt.ensure((size_t)n * sizeof(uint4)));   // the tid words of k_pair_mask ("emit_rank_tids", read at every launch)
  RC(c->d_hi0.ensure((size_t)n * 4)); RC(c->d_clspos.ensure((size_t)n * 4)); RC(c->d_rnd.ensure((size_t)std::max<int64_t>(ng, 1) * 8));
  if (c->d_side_cap == 0) c->d_side_cap = std::max<uint64_t>((uint64_t)n / 4, 1u << 20);
  RC(c->d_side.ensure((size_t)c->d_side_cap * sizeof(uint2)));
  // (a buffer that a queued packed download still reads must not be reallocated under it)
  if (c->rows_busy_set && c->row_off.cap < (size_t)(n + 1) * 8) HIPCHK(hipEventSynchronize(c->rows_busy));
  RC(c->row_off.ensure((size_t)(n + 1) * 8));
  RC(ensure_side_stream(c));
  if (!c->side2_stream) HIPCHK(hipStreamCreateWithPriority(&c->side2_stream, hipStreamNonBlocking, 0));
  hipStream_t ax = c->side_stream, ax2 = c->side2_stream;
  uint64_t *d_tot = c->totals.as<uint64_t>();
  ReadBack *rb = c->rb;

  ProjectArgs A = count_args(c, dc, b);
  A.n_big = dz_nbig; A.walk_list = c->walk_list.as<uint32_t>(); A.n_walk = dz_nbig + 1;
  const bool have_names = b->names && b->name_off;
  DirectArgs D{};
  D.n_aln = n; D.n_groups = ng; D.group_off = b->group_off; D.aln_group = c->aln_group.as<uint32_t>(); D.mate_idx = b->mate_idx;
  D.n_matches = c->n_matches.as<uint32_t>(); D.mask = c->mask.as<uint64_t>(); D.ranges = c->ranges.as<uint4>();
  D.fast_flag = c->fast_flag.as<uint32_t>(); D.s_tid = ix->dev.s_tid; D.big_list = A.big_list; D.n_big = A.n_big;
  D.fm = c->d_fm.as<uint2>(); D.pm_list = (uint32_t *)(c->d_fm.as<uint2>() + n); D.pm_n = dz_nbig + 2; D.n_kept = c->d_nkept.as<uint32_t>(); D.n_rows = c->n_rows.as<uint32_t>(); D.pflag = c->pbit.as<uint8_t>();
  D.kt = c->emit_rank_tids ? c->d_kt.as<uint4>() : nullptr;
  D.side = c->d_side.as<uint2>(); D.side_cap = c->d_side_cap; D.side_used = (unsigned long long *)(dz + GD_COUNTER_WORDS);
  D.cls_pos = c->d_clspos.as<uint32_t>(); D.cig_base = c->cig_base.as<uint64_t>(); D.row_off = c->row_off.as<uint64_t>();
  D.name_off = have_names ? b->name_off : nullptr; D.names = have_names ? b->names : nullptr; D.rnd0 = c->d_rnd.as<uint64_t>();
  D.gd = c->d_desc.as<uint2>(); D.dpos = c->d_desc.as<uint2>() + n; D.hi0 = c->d_hi0.as<uint32_t>(); D.counters = c->counters_d.as<uint64_t>(); D.tot = d_tot;

  // the pieces beside the main chain: the name seeds (second side stream), the big alignments' pairing, k_group_desc, k_big<1>
  SideWork seeds(c, st, ax2), pair_big(c, st, ax), group_desc(c, st, ax), big_emit(c, st, ax);
  HIPCHK(hipMemsetAsync(dz, 0, (GD_COUNTER_WORDS + 4) * 8, st));
  RC(pair_big.fork());   // (the side stream behind the fill; every attempt below forks again)
  // a3-a8, a11-a14 (survival only): the count pass
  RC(segment_stage(c, st, dc, b, pf));
  RC(pf.begin(BR_K_GROUP_IDS));
  launch_group_ids(st, ng, b->group_off, c->aln_group.as<uint32_t>());
  RC(pf.end());
  RC(count_pass(c, st, A, pf, true, true));
  // a packed download of the previous call may still be reading row_off / the row tables (br_project_staged)
  if (c->rows_busy_set) { HIPCHK(hipStreamWaitEvent(st, c->rows_busy, 0)); }
  // a16 (src/mates.cpp:150-261) on the survivor sets, then placement
  const int big_blocks = c->n_cu * 4;
  uint64_t kept = 0, arena = 0, n_simple = 0, n_rows = 0, n_raw = 0;
  bool expanded_ahead = false;
  // second side stream: the name seeds need nothing but the names, and their 156 dependent multiplies per read name are pure ALU work:
  // beside k_pair_mask, which waits on memory or for its turn to issue most of the time
  if (have_names) {
    RC(seeds.fork());
    RC(pf.begin(BR_K_NAME_SEED, ax2));
    launch_name_seed(ax2, D);
    RC(pf.end());
    RC(seeds.done());
  }
  for (int attempt = 0;; attempt++) {
    if (attempt) {   // (the first attempt's counters were zeroed with everything else at the start)
      HIPCHK(hipMemsetAsync(dz, 0, (GD_COUNTER_WORDS + 2) * 8, st));
      HIPCHK(hipMemsetAsync(D.pm_n, 0, 4, st));
    }
    RC(pair_big.fork());
    RC(pf.begin(BR_K_PAIR_BIG, ax));
    launch_big_collect(ax, A, D, big_blocks);
    launch_pair_big(ax, D, big_blocks);
    RC(pf.end());
    RC(pair_big.done());
    RC(pf.begin(BR_K_PAIR_MASK));
    launch_pair_mask(st, D, c->n_cu * 2, c->pair_bitmask);
    RC(pf.end());
    RC(pair_big.join());
    // NH / HI / primary per read name on the side stream beside the scan
    RC(group_desc.fork());
    if (have_names) RC(seeds.join_on(ax));
    RC(pf.begin(BR_K_GROUP_DESC, ax));
    launch_group_desc(ax, D);
    RC(pf.end());
    RC(group_desc.done());
    RC(pf.begin(BR_K_SCAN));
    launch_scan5(st, D, c->tile_sums.as<uint64_t>(), d_tot);
    RC(pf.end());
    // the work list goes out at once, into the list the last call left (it checks the total against that room on the
    // device): it runs while the host waits for the totals, wakes up and sizes the row tables
    expanded_ahead = false;
    if (c->m_aln.cap >= 4) {
      D.m_aln = c->m_aln.as<uint32_t>(); D.m_aln_cap = c->m_aln.cap / 4;
      RC(pf.begin(BR_K_EXPAND_ROWS));
      launch_expand_rows(st, D);
      RC(pf.end());
      expanded_ahead = true;
    }
    HIPCHK(hipMemcpyAsync(rb->scan, d_tot, sizeof(rb->scan), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rb->side, dz + GD_COUNTER_WORDS, sizeof(rb->side), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->d_side_attempts = attempt + 1;
    if (rb->side[1]) {   // the side arena of the > 64-candidate alignments ran out: grow it to the exact total k_big<0> counted
      // (every entry adds its need, also after the overflow) plus a margin for the calls to come, repeat: the repeat fits
      if (attempt >= 3) return BR_ERR_CAPACITY;   // (a guard: the second attempt always fits)
      RC(group_desc.wait_host());
      c->d_side_cap = rb->side[0] + rb->side[0] / 4 + 4096;
      RC(c->d_side.ensure((size_t)c->d_side_cap * sizeof(uint2)));
      D.side = c->d_side.as<uint2>(); D.side_cap = c->d_side_cap;
      continue;
    }
    kept = rb->scan[TOT_MATCHES]; arena = rb->scan[TOT_ARENA]; n_simple = rb->scan[TOT_SIMPLE]; n_rows = rb->scan[TOT_ROWS]; n_raw = rb->scan[TOT_RAW];
    break;
  }
  if (n_raw >= 0xffffffffull || kept >= 0xffffffffull) return BR_ERR_CAPACITY;
  if (kept != n_rows) return BR_ERR_HIP;   // (every kept match is one record: the pairing kernels disagree with themselves)

  const size_t nr = (size_t)std::max<uint64_t>(n_rows, 1);
  if (c->rows_busy_set && (c->pk_a.cap < nr * sizeof(uint4) || c->pk_c.cap < nr * sizeof(uint2))) HIPCHK(hipEventSynchronize(c->rows_busy));
  RC(c->pk_a.ensure(nr * sizeof(uint4))); RC(c->pk_c.ensure(nr * sizeof(uint2)));
  if (expanded_ahead && kept > D.m_aln_cap) expanded_ahead = false;   // (the kernel saw the same and did nothing)
  RC(c->m_aln.ensure(nr * 4)); RC(c->cig_arena.ensure((size_t)std::max<uint64_t>(arena, 1) * 4));
  const bool with_x = c->want_x;
  if (with_x) {
    if (c->rows_busy_set && c->pk_x.cap < nr * sizeof(uint4)) HIPCHK(hipEventSynchronize(c->rows_busy));
    RC(c->pk_x.ensure(nr * sizeof(uint4)));
  }
  A.cig_arena = c->cig_arena.as<uint32_t>();
  D.m_aln = c->m_aln.as<uint32_t>(); D.r_a = c->pk_a.as<uint4>(); D.r_c = c->pk_c.as<uint2>(); D.r_x = with_x ? c->pk_x.as<uint4>() : nullptr;
  D.m_aln_cap = 0;
  if (kept) {
    if (!expanded_ahead) {
      RC(pf.begin(BR_K_EXPAND_ROWS));
      launch_expand_rows(st, D);
      RC(pf.end());
    }
    RC(group_desc.join());   // the descriptors' first halves
    RC(big_emit.fork());
    RC(pf.begin(BR_K_BIG_EMIT, ax));
    launch_big_emit(ax, A, D, big_blocks);
    RC(pf.end());
    RC(big_emit.done());
    RC(pf.begin(BR_K_EMIT_ROWS_SIMPLE));
    launch_emit_rows(st, A, D, (int64_t)kept, (int64_t)n_simple, 1);
    RC(pf.end());
    RC(pf.begin(BR_K_EMIT_ROWS));
    launch_emit_rows(st, A, D, (int64_t)kept, (int64_t)n_simple, 2, c->emit_general_preset != 0);
    RC(pf.end());
    RC(big_emit.join());
  } else {
    RC(group_desc.join());
  }
  HIPCHK(hipMemcpyAsync(rb->direct_cnt, c->counters_d.p, sizeof(rb->direct_cnt), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (!keep_events) RC(pf.collect());
  for (int k = 0; k < 4; k++) rb->counters[k] = rb->direct_cnt[k];
  for (int k = 0; k < GD_SLOTS; k++) { rb->counters[1] += rb->direct_cnt[GD_SLOT0 + k * GD_SLOT_STRIDE]; rb->counters[2] += rb->direct_cnt[GD_SLOT0 + k * GD_SLOT_STRIDE + 1]; }
  if (rb->counters[3]) return BR_ERR_UNSUPPORTED;  // a rewritten CIGAR with more than 2^24 - 1 ops, or NH beyond 28 bits
  c->hist_n = 0;   // (nothing a later speculative launch of the match-table path could be sized from)
  finish_call(c, dc, b, out, n_raw, n_rows, arena, false);
  out->a = (const br_row_a *)c->pk_a.p; out->cigar = (const uint64_t *)c->pk_c.p; out->x = with_x ? (const br_row_x *)c->pk_x.p : nullptr;
  out->similarity_score = nullptr; out->clip_score = nullptr;
  c->detail_valid = with_x;
  c->last_direct = true; c->dA = A; c->dD = D; c->d_kept = (int64_t)kept; c->d_simple = (int64_t)n_simple;
  return BR_OK;
}

// The match-table path: segment -> count -> scan (host wait: sizes) -> k_expand -> k_emit_dense (|| k_project<64,true>)
// -> k_pair -> scan (host wait: sizes) -> k_pair<true> -> k_primary -> k_rows.  The -S rescue plans, runs and applies its
// DP between the count and the scan.
static int run_match_table(br_ctx *c, const DevCfg &dc, const br_device_batch *b, hipStream_t st, br_device_rows *out, Prof &pf,
                           bool keep_events) {
  const bool fa_mode = dc.use_fasta && dc.long_reads;
  const int64_t n = b->n_aln, ng = b->n_groups;
  const int64_t tiles = std::max<int64_t>(scan_tiles_for(std::max<int64_t>(n, ng) + 1), 1);
  RC(ensure_count_tables(c, b));
  RC(c->n_matches.ensure((size_t)n * 4)); RC(c->fast_pre.ensure((size_t)(n + 1) * 4)); RC(c->match_off.ensure((size_t)(n + 1) * 4));
  RC(c->tile_sums.ensure((size_t)tiles * 8 * 3)); RC(c->counters_d.ensure(4 * 8));
  RC(c->n_big.ensure(16)); RC(c->walk_list.ensure((size_t)n * 4));
  uint64_t *d_tot = c->totals.as<uint64_t>();
  ReadBack *rb = c->rb;

  RC(segment_stage(c, st, dc, b, pf));
  ProjectArgs A = count_args(c, dc, b);
  A.fast_pre = c->fast_pre.as<uint32_t>(); A.match_off = c->match_off.as<uint32_t>(); A.cig_base = c->cig_base.as<uint64_t>();
  HIPCHK(hipMemsetAsync(c->n_big.p, 0, 8, st));
  A.n_big = c->n_big.as<uint32_t>(); A.walk_list = c->walk_list.as<uint32_t>(); A.n_walk = c->n_big.as<uint32_t>() + 1;
  const int n_blocks = c->n_cu * c->blocks_per_cu;
  ScanArgs S = scan3_args(c, b);
  FaArgs F{};
  if (!fa_mode) {
    RC(count_pass(c, st, A, pf, !dc.filter_by_similarity));
    RC(pf.begin(BR_K_SCAN));
    launch_scan3(st, S, c->match_off.as<uint32_t>(), c->cig_base.as<uint64_t>(), c->fast_pre.as<uint32_t>(), d_tot + TOT_MATCHES);
    RC(pf.end());
  } else {
    // rescue planning -> ksw2 DP -> count with the rescue results
    RC(c->fa_n_prob.ensure((size_t)n * 4)); RC(c->fa_seq_bytes.ensure((size_t)n * 4));
    RC(c->fa_prob_off.ensure((size_t)(n + 1) * 4)); RC(c->fa_seqarena_off.ensure((size_t)(n + 1) * 8));
    RC(c->fa_ideal_cap.ensure((size_t)n * 4)); RC(c->fa_want.ensure((size_t)n * 16));
    F.seq_src = b->seq_src; F.seq_off = b->seq_off; F.seqs = b->seqs;
    F.n_prob = c->fa_n_prob.as<uint32_t>(); F.seq_bytes = c->fa_seq_bytes.as<uint32_t>();
    F.prob_off = c->fa_prob_off.as<uint32_t>(); F.seqarena_off = c->fa_seqarena_off.as<uint64_t>();
    F.ideal_cap = c->fa_ideal_cap.as<uint32_t>(); F.want_l = c->fa_want.as<uint64_t>(); F.want_r = F.want_l + n;
    RC(pf.begin(BR_K_COUNT));
    launch_project_fa(st, A, F, 0, n_blocks);
    RC(pf.end());
    RC(pf.begin(BR_K_SCAN));
    launch_scan(st, F.n_prob, n, c->tile_sums.as<uint64_t>(), c->fa_prob_off.p, false, d_tot + TOT_RESCUE_PROB);
    launch_scan(st, F.seq_bytes, n, c->tile_sums.as<uint64_t>(), c->fa_seqarena_off.p, true, d_tot + TOT_RESCUE_SEQ);
    RC(pf.end());
    HIPCHK(hipMemcpyAsync(rb->rescue_n, d_tot + TOT_RESCUE_PROB, sizeof(rb->rescue_n), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t n_prob = rb->rescue_n[0], seq_total = rb->rescue_n[1];
    RC(c->fa_stats.ensure(16));
    HIPCHK(hipMemsetAsync(c->fa_stats.p, 0, 16, st));
    c->rescue_stats[0] = n_prob; c->rescue_stats[1] = 0; c->rescue_stats[2] = 0; c->rescue_stats[3] = seq_total;
    if (n_prob >= 0xffffffffull) return BR_ERR_CAPACITY;
    RC(c->fa_probs.ensure(std::max<size_t>(n_prob, 1) * ksw_prob_bytes()));
    RC(c->fa_results.ensure(std::max<size_t>(n_prob, 1) * ksw_res_bytes()));
    RC(c->fa_seq_arena.ensure((size_t)seq_total + 1024));   // the streamed DP reads whole dwords past a problem's last base
    RC(c->fa_clip_ops.ensure((std::max<size_t>(seq_total + n_prob, 1)) * 4));
    RC(c->fa_srcs.ensure(std::max<size_t>(n_prob, 1) * sizeof(FaSrc)));
    F.probs = (KswProb *)c->fa_probs.p; F.results = (KswRes *)c->fa_results.p; F.srcs = c->fa_srcs.as<FaSrc>();
    F.seq_arena = c->fa_seq_arena.as<uint8_t>(); F.clip_ops = c->fa_clip_ops.as<uint32_t>();
    if (n_prob) {
      RC(pf.begin(BR_K_COUNT));
      launch_project_fa(st, A, F, 1, n_blocks);
      launch_fa_fill(st, A, F, (int64_t)n_prob);
      RC(pf.end());
      uint64_t qmax = (uint64_t)std::max(b->max_soft_clip, 0) + std::max(dc.max_clip, dc.max_junc_ins);
      KswRun R{};
      R.n_prob = (int64_t)n_prob; R.probs = F.probs; R.results = F.results; R.seq_arena = F.seq_arena; R.clip_ops = F.clip_ops;
      R.seq_total = seq_total; R.qmax = qmax; R.tmax = qmax + 40; R.stats = c->fa_stats.as<uint64_t>();
      RC(pf.begin(BR_K_KSW));
      RC(run_ksw(c, st, R));
      RC(pf.end());
      HIPCHK(hipMemcpyAsync(rb->rescue_stats, c->fa_stats.p, sizeof(rb->rescue_stats), hipMemcpyDeviceToHost, st));
    }
    RC(pf.begin(BR_K_COUNT));
    launch_project_fa(st, A, F, 2, n_blocks);
    RC(pf.end());
    S.ideal_cap = F.ideal_cap;
    RC(pf.begin(BR_K_SCAN));
    launch_scan3(st, S, c->match_off.as<uint32_t>(), c->cig_base.as<uint64_t>(), c->fast_pre.as<uint32_t>(), d_tot + TOT_MATCHES);
    RC(pf.end());
  }
  HIPCHK(hipMemcpyAsync(rb->scan, d_tot, 3 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t n_matches = rb->scan[TOT_MATCHES], n_cig_arena = rb->scan[TOT_ARENA];
  const int64_t n_simple = fa_mode ? -1 : (int64_t)rb->scan[TOT_SIMPLE];  // matches of the single-M class (first in the emit list)
  if (n_matches >= 0xffffffffull) return BR_ERR_CAPACITY;

  RC(match_tables(c, A, std::max<uint64_t>(n_matches, 1), std::max<uint64_t>(n_cig_arena, 1)));
  if (n_matches) {
    if (fa_mode) {
      // the work list + one lane per match for alignments with at most 64 candidate rows, k_project_fa<3> for the others
      RC(pf.begin(BR_K_EXPAND));
      launch_expand(st, A);
      RC(pf.end());
      RC(pf.begin(BR_K_EMIT));
      launch_project_fa(st, A, F, 3, n_blocks);
      launch_emit_dense_fa(st, A, F, (int64_t)n_matches);
      RC(pf.end());
    } else {
      RC(emit_beside_dense(c, st, A, pf, (int64_t)n_matches, n_simple, true));
    }
  }

  // a16/a17: pairing + NH -> the packed row table
  // (a buffer that a queued packed download still reads must not be reallocated under it)
  if (c->rows_busy_set && c->row_off.cap < (size_t)(n + 1) * 8) HIPCHK(hipEventSynchronize(c->rows_busy));
  RC(c->n_rows.ensure((size_t)n * 4)); RC(c->row_off.ensure((size_t)(n + 1) * 8)); RC(c->aln_group.ensure((size_t)n * 4));
  RC(pf.begin(BR_K_GROUP_IDS));
  launch_group_ids(st, ng, b->group_off, c->aln_group.as<uint32_t>());
  RC(pf.end());
  HIPCHK(hipMemsetAsync(c->counters_d.p, 0, 4 * 8, st));
  PairArgs P;
  RC(pair_args(c, dc, b, A, P));
  RC(pair_count(c, st, P, pf, c->rows_busy_set));
  HIPCHK(hipMemcpyAsync(&rb->scan[TOT_ROWS], d_tot + TOT_ROWS, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t n_rows = rb->scan[TOT_ROWS];

  const bool aux_cols = dc.filter_by_similarity != 0;
  RC(row_tables(c, P, n_rows, aux_cols, true));
  RC(row_tail(c, st, b, P, pf, aux_cols, true, n_rows != 0, 0));
  HIPCHK(hipMemcpyAsync(rb->counters, c->counters_d.p, sizeof(rb->counters), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (!keep_events) RC(pf.collect());
  if (rb->counters[3]) return BR_ERR_UNSUPPORTED;  // a rewritten CIGAR with more than 2^24 - 1 ops
  if (fa_mode && c->rescue_stats[0]) { c->rescue_stats[1] = rb->rescue_stats[0]; c->rescue_stats[2] = rb->rescue_stats[1]; }

  // what a later large batch is predicted from (run_device_small, big)
  c->hist_n = n; c->hist[0] = n_matches; c->hist[1] = n_cig_arena; c->hist[2] = n_simple >= 0 ? (uint64_t)n_simple : 0; c->hist[3] = n_rows;
  c->hist_simf = dc.filter_by_similarity != 0;
  if (fa_mode) c->hist_n = 0;
  finish_call(c, dc, b, out, n_matches, n_rows, n_cig_arena, aux_cols, &P);
  return BR_OK;
}

// The HIP pipeline over a device-resident batch: small and speculative batches (run_device_small), direct rows
// (run_device_direct), or the match table (run_match_table: presets with the similarity filter, -S, direct_rows = 0).
static int run_device_paths(br_ctx *c, const br_config *cfg, const br_device_batch *b, hipStream_t st, br_device_rows *out, bool keep_events) {
  const br_index *ix = c->ix;
  memset(out, 0, sizeof(*out));
  DevCfg dc;
  RC(make_devcfg(cfg, dc));
  // -S only changes long-read runs (src/evaluate.cpp:916-919,939)
  const bool fa_mode = dc.use_fasta && dc.long_reads;
  if (fa_mode && (!ix->has_seq || !b->seq_src || !b->seq_off || !b->seqs)) return BR_ERR_INVALID_ARG;
  const int64_t n = b->n_aln, ng = b->n_groups;
  if (n < 0 || ng < 0 || n >= 0x7fffffffll || b->n_cigar_words >= 0xffffffffll - n) return BR_ERR_CAPACITY;
  HIPCHK(hipSetDevice(ix->device));
  Prof pf{c, st};
  if (!keep_events) c->events_used = 0;
  out->total_processed = (uint64_t)n;
  c->last_n_rows = 0; c->last_n_aln = n; c->last_n_pool = 0; c->wide_valid = false; c->last_aux_cols = false; c->last_direct = false;
  c->last_l_qseq = b->l_qseq; c->last_long_reads = dc.long_reads;
  if (n == 0) { pf.collect(); return BR_OK; }
  if (!fa_mode && c->small_batch && ix->dev.n_rows != 0) {
    // small batches always; large ones when an earlier call left tables and counts to predict from (same preset class)
    const bool small = n <= c->small_n;
    // (up to speculate_n alignments: at 20 M alignments the three waits are 2 % of the step and the 15 % of empty blocks in
    // the predicted grids cost as much, profiles/r03/ab_speculate.log; at 0.1-1 M alignments the step gets 6-13 % shorter)
    const bool big = !small && n <= c->speculate_n && c->speculate && c->hist_n > 0 && c->hist_simf == (dc.filter_by_similarity != 0);
    if (small || big) {
      const int rc = run_device_small(c, dc, b, st, out, pf, keep_events, big);
      if (rc != BR_RETRY_ORDINARY) return rc;
      if (!keep_events) c->events_used = 0;
    }
  }

  if (!fa_mode && !dc.filter_by_similarity && c->direct_rows) return run_device_direct(c, dc, b, st, out, pf, keep_events);
  return run_match_table(c, dc, b, st, out, pf, keep_events);
}

int run_device(br_ctx *c, const br_config *cfg, const br_device_batch *b, hipStream_t st, br_device_rows *out, bool keep_events) {
  c->forget_last_call(st);   // (a bundle call notes its records once they are encoded)
  RC(run_device_paths(c, cfg, b, st, out, keep_events));
  if (out->row_off) { c->last_rows = *out; c->last_group_off = b->group_off; c->last_n_groups = b->n_groups; }   // (no rows table: an empty batch)
  return BR_OK;
}

// br_row_x of the last call's rows, derived on first request (k_rows_detail)
int ensure_detail(br_ctx *c, hipStream_t st) {
  if (c->detail_valid) return BR_OK;
  const size_t nr = (size_t)std::max<int64_t>(c->last_n_rows, 1);
  if (c->rows_busy_set && c->pk_x.cap < nr * sizeof(uint4)) HIPCHK(hipEventSynchronize(c->rows_busy));   // a download may still read it
  RC(c->pk_x.ensure(nr * sizeof(uint4)));
  if (c->last_direct) {
    // direct rows keep no match table to gather from: the emit kernels run once more and write the detail column next to
    // the rows (the last call's batch and the context's tables are still in place: nothing has run since)
    if (c->last_n_rows > 0) {
      DirectArgs D = c->dD;
      D.r_x = c->pk_x.as<uint4>();
      launch_emit_rows(st, c->dA, D, c->d_kept, c->d_simple, 1);
      launch_emit_rows(st, c->dA, D, c->d_kept, c->d_simple, 2, c->emit_general_preset != 0);
      launch_big_emit(st, c->dA, D, c->n_cu * 4);
    }
    c->detail_valid = true;
    return BR_OK;
  }
  if (c->last_n_rows > 0) {
    PairArgs P{};
    P.n_rows_total = c->last_n_rows; P.r_rec = c->r_rec.as<uint4>(); P.m_x = c->m_x.as<uint2>(); P.r_x = c->pk_x.as<uint4>();
    launch_rows_detail(st, P);
  }
  c->detail_valid = true;
  return BR_OK;
}

extern "C" int br_device_rows_detail(br_ctx *c, void *stream, const br_row_x **x) {
  if (!c || !x) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  RC(ensure_detail(c, (hipStream_t)stream));
  *x = (const br_row_x *)c->pk_x.p;
  return BR_OK;
}

// The wide view of the last call's rows: one device array per field (what tests, debuggers and the host-row entry
// points read).  Everything is derived from the packed table; nothing here is on the projection's own path.
int expand_rows(br_ctx *c, hipStream_t st, br_device_wide_rows *out) {
  memset(out, 0, sizeof(*out));
  HIPCHK(hipSetDevice(c->ix->device));
  const uint64_t n_rows = (uint64_t)c->last_n_rows;
  const size_t nr = (size_t)std::max<uint64_t>(n_rows, 1);
  RC(c->r_input.ensure(nr * 4)); RC(c->r_nh.ensure(nr * 4)); RC(c->r_hi.ensure(nr * 4));
  RC(c->r_mapq.ensure(nr * 4)); RC(c->r_group.ensure(nr * 4));
  RC(c->r_mate_tid.ensure(nr * 4)); RC(c->r_mate_pos.ensure(nr * 4)); RC(c->r_isize.ensure(nr * 4));
  RC(c->r_tid.ensure(nr * 4)); RC(c->r_pos.ensure(nr * 4)); RC(c->r_ncig.ensure(nr * 4)); RC(c->r_strand.ensure(nr));
  RC(c->r_sim.ensure(nr * 8)); RC(c->r_clip.ensure(nr * 4)); RC(c->r_junc.ensure(nr * 4)); RC(c->r_refc.ensure(nr * 4));
  RC(c->r_cigoff.ensure((nr + 1) * 8));
  RC(c->r_paired.ensure(nr)); RC(c->r_same.ensure(nr)); RC(c->r_first.ensure(nr)); RC(c->r_primary.ensure(nr));
  uint64_t n_out_words = 0;
  if (n_rows) {
    WideArgs W{};
    W.n_rows = (int64_t)n_rows; W.n_aln = c->last_n_aln; W.long_reads = c->last_long_reads;
    RC(ensure_detail(c, st));
    W.r_a = c->pk_a.as<uint4>(); W.r_c = c->pk_c.as<uint2>(); W.r_x = c->pk_x.as<uint4>();
    W.r_sim = c->last_aux_cols ? c->pk_sim.as<double>() : nullptr; W.r_clip = c->last_aux_cols ? c->pk_clip.as<int32_t>() : nullptr;
    W.pool = c->cig_arena.as<uint32_t>(); W.aln_group = c->aln_group.as<uint32_t>(); W.l_qseq = c->last_l_qseq;
    W.w_input = c->r_input.as<int32_t>(); W.w_nh = c->r_nh.as<uint32_t>(); W.w_hi = c->r_hi.as<uint32_t>();
    W.w_mapq = c->r_mapq.as<uint32_t>(); W.w_group = c->r_group.as<uint32_t>(); W.w_mate_tid = c->r_mate_tid.as<int32_t>();
    W.w_mate_pos = c->r_mate_pos.as<int32_t>(); W.w_isize = c->r_isize.as<int32_t>(); W.w_tid = c->r_tid.as<uint32_t>();
    W.w_pos = c->r_pos.as<uint32_t>(); W.w_ncig = c->r_ncig.as<uint32_t>(); W.w_strand = c->r_strand.as<int8_t>();
    W.w_sim = c->r_sim.as<double>(); W.w_clip = c->r_clip.as<int32_t>(); W.w_junc = c->r_junc.as<int32_t>();
    W.w_refc = c->r_refc.as<int32_t>(); W.w_paired = c->r_paired.as<uint8_t>(); W.w_same = c->r_same.as<uint8_t>();
    W.w_first = c->r_first.as<uint8_t>(); W.w_primary = c->r_primary.as<uint8_t>();
    launch_wide_fields(st, W);
    RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for((int64_t)n_rows + 1), 1) * 8 * 3));
    RC(ensure_totals(c));
    uint64_t *d_tot = c->totals.as<uint64_t>();
    launch_scan(st, c->r_ncig.as<uint32_t>(), (int64_t)n_rows, c->tile_sums.as<uint64_t>(), c->r_cigoff.p, true, d_tot + TOT_WIDE_CIGAR);
    HIPCHK(hipMemcpyAsync(&c->rb->wide_cigar, d_tot + TOT_WIDE_CIGAR, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    n_out_words = c->rb->wide_cigar;
    RC(c->cigar_out.ensure((size_t)std::max<uint64_t>(n_out_words, 1) * 4));
    W.w_cigoff = c->r_cigoff.as<uint64_t>(); W.w_cigar = c->cigar_out.as<uint32_t>();
    launch_wide_cigars(st, W, (int64_t)n_out_words);
  } else {
    HIPCHK(hipMemsetAsync(c->r_cigoff.p, 0, 8, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  c->wide_valid = true;
  out->n_rows = (int64_t)n_rows; out->n_cigar_words = (int64_t)n_out_words;
  out->input_index = c->r_input.as<int32_t>(); out->transcript_id = c->r_tid.as<uint32_t>();
  out->pos = c->r_pos.as<uint32_t>(); out->strand = c->r_strand.as<int8_t>();
  out->cigar_off = c->r_cigoff.as<uint64_t>(); out->cigar = c->cigar_out.as<uint32_t>();
  out->similarity_score = c->r_sim.as<double>(); out->clip_score = c->r_clip.as<int32_t>();
  out->junc_hits = c->r_junc.as<int32_t>(); out->aligned_len = c->r_refc.as<int32_t>();
  out->nh = c->r_nh.as<uint32_t>(); out->hi = c->r_hi.as<uint32_t>(); out->mapq = c->r_mapq.as<uint32_t>();
  out->is_paired = c->r_paired.as<uint8_t>(); out->same_transcript_as_mate = c->r_same.as<uint8_t>();
  out->is_first = c->r_first.as<uint8_t>();
  out->mate_transcript_id = c->r_mate_tid.as<int32_t>(); out->mate_pos = c->r_mate_pos.as<int32_t>();
  out->insert_size = c->r_isize.as<int32_t>(); out->group = c->r_group.as<uint32_t>();
  out->is_primary = c->r_primary.as<uint8_t>();
  return BR_OK;
}

// Exact counters of the algorithmic-bytes formula for the batch the context
// projected last (its exon / match tables are still resident).
extern "C" int br_ctx_collect_counters(br_ctx *c, const br_device_batch *b, void *stream) {
  if (!c || !b) return BR_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->ix->device));
  if (c->last_direct) {
    // The formula's B_out counts the rewritten CIGAR words of every MATCH (the evaluator's output, before pairing), and
    // only the match table holds those: this diagnostic projects the batch once more through the match-table path, with the
    // configuration of the last call (never timed; the row tables are then that projection's)
    const DevCfg dc = c->dA.cfg;
    Prof pf{c, st};
    c->events_used = 0;
    br_device_rows tmp;
    memset(&tmp, 0, sizeof(tmp));
    // (that projection overwrites the row tables and may move the CIGAR arena: what br_quant_add_last / br_coverage_add_last
    // read is its table from here on, not the direct-rows call's description of buffers that no longer hold it)
    c->last_rows = br_device_rows{}; c->last_group_off = nullptr; c->last_n_groups = 0; c->last_stream = st;
    RC(run_match_table(c, dc, b, st, &tmp, pf, false));
    tmp.total_processed = (uint64_t)b->n_aln;
    if (tmp.row_off) { c->last_rows = tmp; c->last_group_off = b->group_off; c->last_n_groups = b->n_groups; }
  }
  DevBuf stats; RC(stats.ensure(8 * 8));   // (freed on the way out)
  HIPCHK(hipMemsetAsync(stats.p, 0, 8 * 8, st));
  StatsArgs T{};
  T.ix = c->ix->dev; T.n_aln = b->n_aln; T.ref_id = b->ref_id; T.cigar_off = b->cigar_off;
  T.seg = c->seg.as<uint2>(); T.head = c->head.as<uint4>(); T.head2 = c->head2.as<uint4>(); T.out = stats.as<uint64_t>();
  int64_t nm = (int64_t)c->counters[6];
  launch_stats(st, T, nm ? c->m_p.as<uint2>() : nullptr, c->match_off.as<uint32_t>(), c->n_matches.as<uint32_t>());
  uint64_t h[8];
  HIPCHK(hipMemcpyAsync(h, stats.p, 8 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t n = (uint64_t)b->n_aln;
  c->counters[3] = h[3]; c->counters[4] = h[4]; c->counters[5] = h[5]; c->counters[7] = h[7];
  c->counters[0] = 24ull * n + 4ull * h[3];
  c->counters[1] = h[1];
  c->counters[2] = 4ull * n + 24ull * (uint64_t)nm + 4ull * h[7];
  return BR_OK;
}

// Diagnostic of the last call, which must have been a direct-rows call: read back from what that call left on the device
// (its counter block, the pairing flags), nothing recomputed.
extern "C" int br_ctx_direct_diag(br_ctx *c, uint64_t out[8], uint8_t *pflags) {
  if (!c || !out || !c->last_direct) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  const DirectArgs &D = c->dD;
  uint64_t used = 0;
  uint32_t nb[3] = {0, 0, 0};   // n_big | n_walk | pm_n
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&used, D.side_used, 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nb, D.n_big, 12, hipMemcpyDeviceToHost));
  if (pflags && D.n_aln > 0) HIPCHK(hipMemcpy(pflags, D.pflag, (size_t)D.n_aln, hipMemcpyDeviceToHost));
  memset(out, 0, 8 * sizeof(uint64_t));
  out[0] = nb[0]; out[1] = (uint64_t)c->d_side_attempts; out[2] = used; out[3] = D.side_cap; out[4] = nb[2];
  uint64_t slots[GD_COUNTER_WORDS];
  HIPCHK(hipMemcpy(slots, D.counters, sizeof(slots), hipMemcpyDeviceToHost));
  for (int k = 0; k < GD_SLOTS; k++) out[6] += slots[GD_SLOT0 + k * GD_SLOT_STRIDE + PM_SLOT_WORD];
  if (D.n_aln > 0) {   // work-list entries of the light two-exon class: kept matches of simple-class alignments with two read exons
    const size_t n = (size_t)D.n_aln;
    std::vector<uint32_t> ff(n), nk(n);
    std::vector<uint4> hd(n);
    std::vector<uint8_t> pf(n);
    HIPCHK(hipMemcpy(ff.data(), D.fast_flag, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nk.data(), D.n_kept, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hd.data(), c->head.p, n * sizeof(uint4), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pf.data(), D.pflag, n, hipMemcpyDeviceToHost));
    uint64_t light = 0;
    for (size_t a = 0; a < n; a++)
      if ((ff[a] >> 31) && hd[a].z == 2 && !(pf[a] & PF_BIG)) light += nk[a];
    out[5] = light;
  }
  return BR_OK;
}

// Diagnostic: the tid words the last direct-rows call's pairing left (DirectArgs::kt), one per alignment.  A call made with
// "emit_rank_tids" 0 has none: every alignment reads as "no word".
extern "C" int br_ctx_direct_tidwords(br_ctx *c, uint64_t *common, uint32_t *base) {
  if (!c || !common || !base || !c->last_direct) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  const DirectArgs &D = c->dD;
  const size_t n = D.n_aln > 0 ? (size_t)D.n_aln : 0;
  std::vector<uint4> w(n, make_uint4(0u, 0u, KT_NONE, 0u));
  HIPCHK(hipDeviceSynchronize());
  if (D.kt && n) HIPCHK(hipMemcpy(w.data(), D.kt, n * sizeof(uint4), hipMemcpyDeviceToHost));
  for (size_t a = 0; a < n; a++) { common[a] = (uint64_t)w[a].x | ((uint64_t)w[a].y << 32); base[a] = w[a].z; }
  return BR_OK;
}

extern "C" int br_project_batch_device(br_ctx *c, const br_config *cfg, const br_device_batch *b, void *stream,
                                       br_device_rows *out) {
  if (!c || !cfg || !b || !out) return BR_ERR_INVALID_ARG;
  return run_device(c, cfg, b, (hipStream_t)stream, out);
}

extern "C" int br_device_rows_expand(br_ctx *c, void *stream, br_device_wide_rows *out) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  return expand_rows(c, (hipStream_t)stream, out);
}
