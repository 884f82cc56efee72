// Host batches: flat staging and the packed rows home (br_project_staged), the wide host rows, the per-group entry points
// and the -S DP diagnostic.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"

// ---------------------------------------------------------------------------
// host-batch entry: upload, run, download, finalise primary flags
// ---------------------------------------------------------------------------
template <typename T>
static int h2d(DevBuf &buf, const T *src, size_t n, hipStream_t st) {
  RC(buf.ensure(std::max<size_t>(n, 1) * sizeof(T)));
  if (n) HIPCHK(hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
  return BR_OK;
}
template <typename T>
static int d2h(PinnedVec<T> &dst, const void *src, size_t n, hipStream_t st) {
  RC(dst.resize(n));
  if (n) HIPCHK(hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, st));
  return BR_OK;
}

// ---- flat batches: staging, the input contract on the device, packed rows home ----
static int ensure_streams(br_ctx *c) {
  // The runtime keeps a small pool of hardware queues per stream priority and lets streams of one priority share them once
  // there are more streams than queues: two streams on one queue run one after the other.  The context's kernel streams
  // (run, side, side2, the caller's) are of normal priority; the upload stream takes the high pool and the download stream the
  // low one, so that neither transfer ever queues behind the other or behind a kernel stream (a context that had already
  // created its side streams -- a device-resident call first -- found its uploads and downloads serialised: 80 ms per
  // PCIe-inclusive step where 60 is the wire, profiles/pcie_phases.py)
  int prio_low = 0, prio_high = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
  if (!c->copy_stream) HIPCHK(hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, prio_high));
  if (!c->run_stream) HIPCHK(hipStreamCreateWithFlags(&c->run_stream, hipStreamNonBlocking));
  if (!c->d2h_stream) HIPCHK(hipStreamCreateWithPriority(&c->d2h_stream, hipStreamNonBlocking, prio_low));
  if (!c->rows_busy) HIPCHK(hipEventCreateWithFlags(&c->rows_busy, hipEventDisableTiming));
  if (!c->alt.busy) HIPCHK(hipEventCreateWithFlags(&c->alt.busy, hipEventDisableTiming));
  return BR_OK;
}

extern "C" int br_batch_stage(br_ctx *c, const br_batch *b, int slot) {
  if (!c || !b || slot < 0 || slot > 1) return BR_ERR_INVALID_ARG;
  const int64_t n = b->n_aln;
  if (n < 0 || n >= 0x7fffffffll) return BR_ERR_CAPACITY;
  if (n && (!b->ref_id || !b->ref_start || !b->flags || !b->xs || !b->ts || !b->cigar_off || !b->name_off || !b->mate_ref_id ||
            !b->mate_start)) return BR_ERR_INVALID_ARG;
  const uint64_t n_words = n ? b->cigar_off[n] : 0, n_name = n ? b->name_off[n] : 0;
  const bool has_seq = b->seq_off && b->seqs;
  const uint64_t n_seq = (n && has_seq) ? b->seq_off[n] : 0;
  if (n_words >= 0xfffffff0ull - (uint64_t)n || n_name >= 0xfffffff0ull || n_seq >= 0xfffffff0ull) return BR_ERR_CAPACITY;
  if ((n_words && !b->cigar) || (n_name && !b->names)) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  RC(ensure_streams(c));
  br_ctx::InSlot &S = c->in_slot[slot];
  if (!S.ready) HIPCHK(hipEventCreateWithFlags(&S.ready, hipEventDisableTiming));
  if (!S.rows_home) HIPCHK(hipEventCreateWithFlags(&S.rows_home, hipEventDisableTiming));
  hipStream_t cs = c->copy_stream;
  S.n = n; S.n_words = n_words; S.n_name = n_name; S.n_seq = n_seq; S.has_seq = has_seq; S.staged = true;
  const size_t nn = (size_t)n;
  RC(h2d(S.ref_id, b->ref_id, nn, cs)); RC(h2d(S.ref_start, b->ref_start, nn, cs)); RC(h2d(S.flags, b->flags, nn, cs));
  RC(h2d(S.xs, b->xs, nn, cs)); RC(h2d(S.ts, b->ts, nn, cs));
  RC(h2d(S.mate_ref, b->mate_ref_id, nn, cs)); RC(h2d(S.mate_start, b->mate_start, nn, cs));
  RC(S.cigar_off64.ensure((nn + 1) * 8)); RC(S.name_off64.ensure((nn + 1) * 8));
  if (n) {
    HIPCHK(hipMemcpyAsync(S.cigar_off64.p, b->cigar_off, (nn + 1) * 8, hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(S.name_off64.p, b->name_off, (nn + 1) * 8, hipMemcpyHostToDevice, cs));
  } else {
    HIPCHK(hipMemsetAsync(S.cigar_off64.p, 0, 8, cs)); HIPCHK(hipMemsetAsync(S.name_off64.p, 0, 8, cs));
  }
  RC(h2d(S.cigar, b->cigar, (size_t)n_words, cs)); RC(h2d(S.names, (const uint8_t *)b->names, (size_t)n_name, cs));
  RC(S.lqseq.ensure(std::max<size_t>(nn, 1) * 4));
  if (b->l_qseq) { if (n) HIPCHK(hipMemcpyAsync(S.lqseq.p, b->l_qseq, nn * 4, hipMemcpyHostToDevice, cs)); }
  else HIPCHK(hipMemsetAsync(S.lqseq.p, 0, std::max<size_t>(nn, 1) * 4, cs));
  if (has_seq) {
    RC(S.seq_off64.ensure((nn + 1) * 8));
    if (n) HIPCHK(hipMemcpyAsync(S.seq_off64.p, b->seq_off, (nn + 1) * 8, hipMemcpyHostToDevice, cs));
    else HIPCHK(hipMemsetAsync(S.seq_off64.p, 0, 8, cs));
    RC(h2d(S.seqs, (const uint8_t *)b->seqs, (size_t)n_seq, cs));
  }
  HIPCHK(hipEventRecord(S.ready, cs));
  return BR_OK;
}

// The staged slot's input contract on the device (what br_batch_prepare / br_batch_seq_source compute on the host:
// read-name groups src/core.cpp:347-380, mate index src/bramble.cpp:272-311, the group's shared sequence
// src/core.cpp:353-378) and the device batch over it.
static int prep_staged(br_ctx *c, const br_config *cfg, br_ctx::InSlot &S, hipStream_t st, br_device_batch *db) {
  memset(db, 0, sizeof(*db));
  const int64_t n = S.n;
  const size_t nn = (size_t)n;
  HIPCHK(hipStreamWaitEvent(st, S.ready, 0));
  db->n_aln = n;
  if (n == 0) return BR_OK;
  RC(S.cigar_off.ensure((nn + 1) * 4)); RC(S.name_off.ensure((nn + 1) * 4)); RC(S.isnew.ensure(nn * 4));
  RC(S.group_pre.ensure((nn + 1) * 4)); RC(S.mate_idx.ensure(nn * 4));
  if (S.has_seq) { RC(S.seq_off.ensure((nn + 1) * 4)); RC(S.seq_src.ensure(nn * 4)); }
  RC(c->p_small.ensure(64)); RC(c->p_big.ensure((nn / 96 + 2) * 4));
  RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for(n + 1), 1) * 8 * 3));
  RC(ensure_totals(c));
  HIPCHK(hipMemsetAsync(c->p_small.p, 0, 64, st));
  SoaArgs A{};
  A.n = n; A.cigar_off64 = S.cigar_off64.as<uint64_t>(); A.name_off64 = S.name_off64.as<uint64_t>();
  A.seq_off64 = S.has_seq ? S.seq_off64.as<uint64_t>() : nullptr;
  A.cigar_off = S.cigar_off.as<uint32_t>(); A.name_off = S.name_off.as<uint32_t>(); A.seq_off = S.has_seq ? S.seq_off.as<uint32_t>() : nullptr;
  A.names = S.names.as<uint8_t>(); A.cigar = S.cigar.as<uint32_t>(); A.isnew = S.isnew.as<uint32_t>(); A.maxima = c->p_small.as<uint32_t>();
  launch_soa_fields(st, A);
  uint64_t *d_tot = c->totals.as<uint64_t>();
  launch_scan(st, A.isnew, n, c->tile_sums.as<uint64_t>(), S.group_pre.p, false, d_tot + TOT_HOST_GROUPS);
  HIPCHK(hipMemcpyAsync(&c->rb->host_groups, d_tot + TOT_HOST_GROUPS, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&c->rb->host_max, c->p_small.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t ng = c->rb->host_groups;
  const uint32_t max_nc = (uint32_t)(c->rb->host_max & 0xffffffffu), max_clip = (uint32_t)(c->rb->host_max >> 32);
  RC(S.group_off.ensure(((size_t)ng + 1) * 4));
  ParseArgs P{};
  P.n = n; P.n_groups = (int64_t)ng; P.isnew = A.isnew; P.group_pre = S.group_pre.as<uint32_t>(); P.group_off = S.group_off.as<uint32_t>();
  P.flags = S.flags.as<uint16_t>(); P.ref_id = S.ref_id.as<int32_t>(); P.ref_start = S.ref_start.as<int32_t>();
  P.mate_ref_id = S.mate_ref.as<int32_t>(); P.mate_start = S.mate_start.as<int32_t>(); P.mate_idx = S.mate_idx.as<int32_t>();
  P.n_big_groups = c->p_small.as<uint32_t>() + 2; P.big_groups = c->p_big.as<uint32_t>();
  launch_group_off(st, P);
  launch_mates(st, P);
  db->n_groups = (int64_t)ng; db->ref_id = P.ref_id; db->ref_start = P.ref_start; db->flags = P.flags;
  db->xs = S.xs.as<int8_t>(); db->ts = S.ts.as<int8_t>(); db->cigar_off = A.cigar_off; db->cigar = A.cigar;
  db->mate_idx = P.mate_idx; db->group_off = P.group_off; db->l_qseq = S.lqseq.as<int32_t>();
  db->n_cigar_words = (int64_t)S.n_words; db->max_n_cigar = (int32_t)max_nc;
  db->name_off = A.name_off; db->names = A.names;
  if (cfg->use_fasta && (cfg->lr || cfg->lr_hq)) {
    if (!S.has_seq) return BR_ERR_INVALID_ARG;
    P.seq_off = A.seq_off; P.seq_src = S.seq_src.as<int32_t>();
    launch_seq_src(st, P);
    db->seq_off = A.seq_off; db->seqs = S.seqs.as<uint8_t>(); db->seq_src = P.seq_src; db->max_soft_clip = (int32_t)max_clip;
  }
  return BR_OK;
}

extern "C" int br_project_staged(br_ctx *c, const br_config *cfg, int slot, br_host_rows *out) {
  if (!c || !cfg || !out || slot < 0 || slot > 1) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  br_ctx::InSlot &S = c->in_slot[slot];
  if (!S.staged) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  RC(ensure_streams(c));
  if (S.rows_pending) { HIPCHK(hipEventSynchronize(S.rows_home)); S.rows_pending = false; }  // the slot's pinned arrays are rewritten below
  hipStream_t st = c->run_stream;
  // the other set of row tables: what the last call's download reads stays untouched (rows_busy follows its set)
  std::swap(c->pk_a, c->alt.pk_a); std::swap(c->pk_x, c->alt.pk_x); std::swap(c->pk_sim, c->alt.pk_sim); std::swap(c->pk_clip, c->alt.pk_clip);
  std::swap(c->pk_ch, c->alt.pk_ch); std::swap(c->pool, c->alt.pool); std::swap(c->row_off, c->alt.row_off);
  std::swap(c->rows_busy, c->alt.busy); std::swap(c->rows_busy_set, c->alt.busy_set);
  c->detail_valid = false; c->wide_valid = false; c->last_direct = false;   // (they describe the other set)
  br_device_batch db;
  RC(prep_staged(c, cfg, S, st, &db));
  S.staged = false;
  br_device_rows pr;
  { WantDetail wd(c, c->host_detail != 0); RC(run_device(c, cfg, &db, st, &pr)); }   // returns with the stream drained
  const size_t nr = (size_t)pr.n_rows, nn = (size_t)S.n;
  // the long (> 2 op) rewritten CIGARs sit in the sparse arena: a dense copy for the host (sizes -> scan -> copy)
  size_t np = 0;
  if (nr) {
    RC(c->pool_sizes.ensure(nr * 4)); RC(c->pool_off.ensure((nr + 1) * 8)); RC(c->pk_ch.ensure(nr * sizeof(uint2)));
    RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for((int64_t)nr + 1), 1) * 8 * 3));
    PoolArgs Q{};
    Q.n_rows = (int64_t)nr; Q.r_a = c->pk_a.as<uint4>(); Q.r_c = c->pk_c.as<uint2>(); Q.arena = c->cig_arena.as<uint32_t>();
    Q.sizes = c->pool_sizes.as<uint32_t>(); Q.off = c->pool_off.as<uint64_t>(); Q.c_out = c->pk_ch.as<uint2>();
    if (c->host_detail) RC(ensure_detail(c, st));
    launch_pool_sizes(st, Q);
    launch_scan(st, Q.sizes, (int64_t)nr, c->tile_sums.as<uint64_t>(), c->pool_off.p, true, c->totals.as<uint64_t>() + TOT_HOST_POOL);
    HIPCHK(hipMemcpyAsync(&c->rb->host_pool, c->totals.as<uint64_t>() + TOT_HOST_POOL, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    np = (size_t)c->rb->host_pool;
    RC(c->pool.ensure(std::max<size_t>(np, 1) * 4));
    Q.pool = c->pool.as<uint32_t>();
    launch_pool_copy(st, Q, np > 8 * nr);
    HIPCHK(hipStreamSynchronize(st));
  }
  hipStream_t ds = c->d2h_stream;
  RC(d2h(S.h_a, pr.a, nr, ds)); RC(d2h(S.h_c, c->pk_ch.p, nr, ds)); RC(d2h(S.h_pool, c->pool.p, np, ds));
  RC(S.h_row_off.resize(nn + 1));
  if (nn) HIPCHK(hipMemcpyAsync(S.h_row_off.data(), pr.row_off, (nn + 1) * 8, hipMemcpyDeviceToHost, ds));
  else S.h_row_off.p[0] = 0;
  RC(d2h(S.h_mate, db.mate_idx, nn, ds));
  if (c->host_detail) RC(d2h(S.h_x, c->pk_x.p, nr, ds));
  if (pr.similarity_score) { RC(d2h(S.h_sim, pr.similarity_score, nr, ds)); RC(d2h(S.h_clip, pr.clip_score, nr, ds)); }
  HIPCHK(hipEventRecord(S.rows_home, ds));
  HIPCHK(hipEventRecord(c->rows_busy, ds));
  c->rows_busy_set = true; S.rows_pending = true;
  out->n_rows = pr.n_rows; out->n_aln = S.n; out->n_groups = db.n_groups; out->n_pool_words = (int64_t)np;
  out->a = (const br_row_a *)S.h_a.data(); out->cigar = S.h_c.data(); out->pool = S.h_pool.data();
  out->row_off = S.h_row_off.data(); out->mate_idx = S.h_mate.data();
  out->x = c->host_detail ? (const br_row_x *)S.h_x.data() : nullptr;
  out->similarity_score = pr.similarity_score ? S.h_sim.data() : nullptr;
  out->clip_score = pr.similarity_score ? S.h_clip.data() : nullptr;
  out->total_complete = pr.total_complete; out->total_unique = pr.total_unique;
  out->dropped_reads = pr.dropped_reads; out->total_processed = pr.total_processed;
  return BR_OK;
}

extern "C" int br_host_rows_wait(br_ctx *c, int slot) {
  if (!c || slot < 0 || slot > 1) return BR_ERR_INVALID_ARG;
  br_ctx::InSlot &S = c->in_slot[slot];
  if (S.rows_pending) { HIPCHK(hipEventSynchronize(S.rows_home)); S.rows_pending = false; }
  return BR_OK;
}

extern "C" int br_project_batch_packed(br_ctx *c, const br_config *cfg, const br_batch *b, br_host_rows *out) {
  if (!c || !cfg || !b || !out) return BR_ERR_INVALID_ARG;
  RC(br_batch_stage(c, b, 0));
  RC(br_project_staged(c, cfg, 0, out));
  return br_host_rows_wait(c, 0);
}

// The wide host rows (ABI version 1 layout): the same staging and device-side input contract, then the wide view
// derived on the device and downloaded array by array.
extern "C" int br_project_batch(br_ctx *c, const br_config *cfg, const br_batch *b, br_rows *out) {
  if (!c || !cfg || !b || !out) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  RC(br_batch_stage(c, b, 0));
  br_ctx::InSlot &S = c->in_slot[0];
  hipStream_t st = c->run_stream;
  br_device_batch db;
  RC(prep_staged(c, cfg, S, st, &db));
  S.staged = false;
  br_device_rows pr;
  { WantDetail wd(c, true); RC(run_device(c, cfg, &db, st, &pr)); }
  br_device_wide_rows dr;
  RC(expand_rows(c, st, &dr));

  size_t nr = (size_t)dr.n_rows;
  RC(d2h(c->h_input, dr.input_index, nr, st)); RC(d2h(c->h_tid, dr.transcript_id, nr, st));
  RC(d2h(c->h_pos, dr.pos, nr, st)); RC(d2h(c->h_strand, dr.strand, nr, st));
  RC(d2h(c->h_cigoff, dr.cigar_off, nr ? nr + 1 : 0, st)); RC(d2h(c->h_cigar, dr.cigar, (size_t)dr.n_cigar_words, st));
  RC(d2h(c->h_sim, dr.similarity_score, nr, st)); RC(d2h(c->h_clip, dr.clip_score, nr, st));
  RC(d2h(c->h_junc, dr.junc_hits, nr, st)); RC(d2h(c->h_refc, dr.aligned_len, nr, st));
  RC(d2h(c->h_nh, dr.nh, nr, st)); RC(d2h(c->h_hi, dr.hi, nr, st)); RC(d2h(c->h_mapq, dr.mapq, nr, st));
  RC(d2h(c->h_paired, dr.is_paired, nr, st)); RC(d2h(c->h_same, dr.same_transcript_as_mate, nr, st));
  RC(d2h(c->h_first, dr.is_first, nr, st)); RC(d2h(c->h_mate_tid, dr.mate_transcript_id, nr, st));
  RC(d2h(c->h_mate_pos, dr.mate_pos, nr, st)); RC(d2h(c->h_isize, dr.insert_size, nr, st));
  RC(d2h(c->h_group, dr.group, nr, st)); RC(d2h(c->h_primary, dr.is_primary, nr, st));
  HIPCHK(hipStreamSynchronize(st));
  if (nr == 0) { RC(c->h_cigoff.resize(1)); c->h_cigoff.p[0] = 0; }

  out->n_rows = (int64_t)nr;
  out->input_index = c->h_input.data(); out->transcript_id = c->h_tid.data(); out->pos = c->h_pos.data();
  out->strand = c->h_strand.data(); out->cigar_off = c->h_cigoff.data(); out->cigar = c->h_cigar.data();
  out->similarity_score = c->h_sim.data(); out->clip_score = c->h_clip.data(); out->junc_hits = c->h_junc.data();
  out->aligned_len = c->h_refc.data(); out->nh = c->h_nh.data(); out->hi = c->h_hi.data(); out->mapq = c->h_mapq.data();
  out->is_primary = c->h_primary.data(); out->is_paired = c->h_paired.data();
  out->same_transcript_as_mate = c->h_same.data(); out->is_first = c->h_first.data();
  out->mate_transcript_id = c->h_mate_tid.data(); out->mate_pos = c->h_mate_pos.data();
  out->insert_size = c->h_isize.data(); out->group = c->h_group.data();
  out->total_complete = pr.total_complete; out->total_unique = pr.total_unique;
  out->dropped_reads = pr.dropped_reads; out->total_processed = pr.total_processed;
  return BR_OK;
}

extern "C" uint32_t br_row_mapq(uint32_t nh, int long_reads);
static int project_groups_lean(br_ctx *c, const br_config *cfg, const br_batch &b, const std::vector<uint64_t> &kept,
                               const std::vector<char> &read_strand, const br_projected **out, size_t *n_out) {
  const size_t n = (size_t)b.n_aln;
  const uint64_t n_words = b.cigar_off[n], n_name = b.name_off[n], n_seq = b.seq_off ? b.seq_off[n] : 0;
  if (n_words >= 0x7fffffffull || n_name >= 0x7fffffffull || n_seq >= 0x7fffffffull) return BR_RETRY_ORDINARY;
  HIPCHK(hipSetDevice(c->ix->device));
  RC(ensure_streams(c));
  hipStream_t st = c->run_stream;
  // the contract on the host (src/core.cpp:347-380, src/bramble.cpp:272-311, src/core.cpp:353-378)
  std::vector<int32_t> mate_idx(n), seq_src;
  std::vector<uint32_t> group_off(n + 1);
  int64_t ng = 0;
  RC(br_batch_prepare(&b, mate_idx.data(), group_off.data(), &ng));
  if (b.seq_off) { seq_src.resize(n); RC(br_batch_seq_source(&b, group_off.data(), ng, seq_src.data())); }
  // one packed upload: every array at a 16-byte aligned offset
  size_t at = 0;
  auto place = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15) & ~(size_t)15; return o; };
  const size_t o_ref = place(4 * n), o_start = place(4 * n), o_flags = place(2 * n), o_xs = place(n), o_ts = place(n),
               o_coff = place(4 * (n + 1)), o_cig = place(4 * (size_t)n_words), o_mate = place(4 * n), o_goff = place(4 * ((size_t)ng + 1)),
               o_lq = place(4 * n), o_noff = place(4 * (n + 1)), o_names = place((size_t)n_name),
               o_soff = place(b.seq_off ? 4 * (n + 1) : 0), o_seqs = place((size_t)n_seq), o_ssrc = place(b.seq_off ? 4 * n : 0);
  RC(c->g_host.resize(at + 16));
  RC(c->g_dev.ensure(at + 16));
  uint8_t *h = c->g_host.data();
  memcpy(h + o_ref, b.ref_id, 4 * n); memcpy(h + o_start, b.ref_start, 4 * n); memcpy(h + o_flags, b.flags, 2 * n);
  memcpy(h + o_xs, b.xs, n); memcpy(h + o_ts, b.ts, n);
  int32_t max_nc = 0, max_clip = 0;
  for (size_t i = 0; i <= n; i++) { ((uint32_t *)(h + o_coff))[i] = (uint32_t)b.cigar_off[i]; ((uint32_t *)(h + o_noff))[i] = (uint32_t)b.name_off[i]; }
  for (size_t i = 0; i < n; i++) {
    const uint64_t c0 = b.cigar_off[i], c1 = b.cigar_off[i + 1];
    max_nc = std::max<int32_t>(max_nc, (int32_t)(c1 - c0));
    if (c1 > c0) {   // leading / trailing soft clips (sizing of the rescue buffers), as k_soa_fields
      uint32_t w = b.cigar[c0];
      if ((w & 0xfu) == 5u && c1 - c0 > 1) w = b.cigar[c0 + 1];
      if ((w & 0xfu) == 4u) max_clip = std::max<int32_t>(max_clip, (int32_t)(w >> 4));
      w = b.cigar[c1 - 1];
      if ((w & 0xfu) == 5u && c1 - c0 > 1) w = b.cigar[c1 - 2];
      if ((w & 0xfu) == 4u) max_clip = std::max<int32_t>(max_clip, (int32_t)(w >> 4));
    }
  }
  memcpy(h + o_cig, b.cigar, 4 * (size_t)n_words); memcpy(h + o_mate, mate_idx.data(), 4 * n);
  memcpy(h + o_goff, group_off.data(), 4 * ((size_t)ng + 1));
  if (b.l_qseq) memcpy(h + o_lq, b.l_qseq, 4 * n); else memset(h + o_lq, 0, 4 * n);
  memcpy(h + o_names, b.names, (size_t)n_name);
  if (b.seq_off) {
    for (size_t i = 0; i <= n; i++) ((uint32_t *)(h + o_soff))[i] = (uint32_t)b.seq_off[i];
    memcpy(h + o_seqs, b.seqs, (size_t)n_seq); memcpy(h + o_ssrc, seq_src.data(), 4 * n);
  }
  HIPCHK(hipMemcpyAsync(c->g_dev.p, h, at, hipMemcpyHostToDevice, st));
  const uint8_t *d = c->g_dev.as<uint8_t>();
  br_device_batch db{};
  db.n_aln = (int64_t)n; db.n_groups = ng;
  db.ref_id = (const int32_t *)(d + o_ref); db.ref_start = (const int32_t *)(d + o_start); db.flags = (const uint16_t *)(d + o_flags);
  db.xs = (const int8_t *)(d + o_xs); db.ts = (const int8_t *)(d + o_ts); db.cigar_off = (const uint32_t *)(d + o_coff);
  db.cigar = (const uint32_t *)(d + o_cig); db.mate_idx = (const int32_t *)(d + o_mate); db.group_off = (const uint32_t *)(d + o_goff);
  db.l_qseq = (const int32_t *)(d + o_lq); db.name_off = (const uint32_t *)(d + o_noff); db.names = d + o_names;
  db.n_cigar_words = (int64_t)n_words; db.max_n_cigar = max_nc;
  if (b.seq_off) { db.seq_off = (const uint32_t *)(d + o_soff); db.seqs = d + o_seqs; db.seq_src = (const int32_t *)(d + o_ssrc); db.max_soft_clip = max_clip; }
  br_device_rows pr;
  c->rows_to_host = true;
  int rrc;
  { WantDetail wd(c, true); rrc = run_device(c, cfg, &db, st, &pr); }   // returns with the stream drained
  c->rows_to_host = false;
  RC(rrc);
  const size_t nr = (size_t)pr.n_rows, np = (size_t)pr.n_pool_words;
  if (np > (1u << 20)) return BR_RETRY_ORDINARY;   // a CIGAR arena of more than 4 MB: the dense pool of the batch path
  bool pool_home = false;
  if (!c->rows_at_host) {   // the call went down the ordinary pipeline (-S, or a dense locus): fetch the rows
    RC(ensure_detail(c, st));
    RC(d2h(c->g_a, pr.a, nr, st)); RC(d2h(c->g_c, pr.cigar, nr, st)); RC(d2h(c->g_x, c->pk_x.p, nr, st));
    if (pr.similarity_score) RC(d2h(c->g_sim, pr.similarity_score, nr, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  else c->last_n_rows = 0;   // the context's device row tables were not written: nothing for br_device_rows_expand / br_bam_encode_device to find
  c->rows_at_host = false;
  size_t n_cig_words = 0;
  for (size_t r = 0; r < nr; r++) n_cig_words += c->g_a.p[r].z & RM_NCIG;
  RC(c->g_cig.resize(n_cig_words + 1));
  c->h_proj.resize(nr);
  size_t cw = 0;
  const int long_reads = (cfg->lr || cfg->lr_hq) ? 1 : 0;
  for (size_t r = 0; r < nr; r++) {
    const uint4 a = c->g_a.p[r], x = c->g_x.p[r];
    const uint2 cr = c->g_c.p[r];
    const uint32_t meta = a.z, nc = meta & RM_NCIG;
    br_projected &p = c->h_proj[r];
    p.transcript_id = a.x; p.transcript_start = a.y;
    p.aligned_len = (uint32_t)std::max<int32_t>((int32_t)x.z, 0);
    uint64_t e = (uint64_t)p.transcript_start + p.aligned_len;  // saturating add, then saturating sub 1
    if (e > 0xffffffffull) e = 0xffffffffull;
    p.transcript_end = e ? (uint32_t)(e - 1) : 0;
    uint32_t *cg = c->g_cig.p + cw;
    if (nc <= 2) { if (nc > 0) cg[0] = cr.x; if (nc > 1) cg[1] = cr.y; }
    else {
      if (!pool_home) {   // the arena's used part, once, when a record has more than two ops
        RC(d2h(c->g_pool, pr.pool, np, st));
        HIPCHK(hipStreamSynchronize(st));
        pool_home = true;
      }
      const uint64_t off = ((uint64_t)cr.y << 32) | cr.x;
      if (off + nc > np) return BR_ERR_HIP;
      memcpy(cg, c->g_pool.p + off, 4 * (size_t)nc);
    }
    cw += nc;
    uint32_t qa = 0;
    for (uint32_t k = 0; k < nc; k++) {
      const uint32_t op = cg[k] & 0xf;
      if (op == OP_M || op == OP_EQ || op == OP_X || op == OP_I || op == OP_MATCH_OVR || op == OP_INS_OVR) qa += cg[k] >> 4;
    }
    p.query_aligned_len = qa;
    const size_t bi = (size_t)x.x;
    p.transcript_strand = (meta & RM_MINUS) ? '-' : '+';
    p.is_reverse = p.transcript_strand != read_strand[bi];   // api.rs:453 <- evaluate.rs:1062 (see project_groups_impl)
    p.similarity_score = pr.similarity_score ? c->g_sim.p[r] : 0.0;
    p.nh = a.w; p.hi = x.w; p.is_primary = (meta & RM_PRIMARY) ? 1 : 0;
    p.same_transcript_as_mate = (meta & RM_SAME) ? 1 : 0; p.is_paired_out = (meta & RM_PAIRED) ? 1 : 0;
    int32_t isize = 0;   // set_mate_info (src/bam.cpp:531-588): the pair's other record is the adjacent row
    if ((meta & RM_PAIRED) && (meta & RM_SAME)) {
      const uint4 o = c->g_a.p[(meta & RM_FIRST) ? r + 1 : r - 1];
      const int32_t my_pos = (int32_t)a.y, mate_pos = (int32_t)o.y, lq = b.l_qseq ? b.l_qseq[bi] : 0;
      isize = (my_pos <= mate_pos) ? (mate_pos + lq) - my_pos : -((my_pos + lq) - mate_pos);
    }
    p.insert_size = isize; p.input_index = kept[bi];
    p.mapq = br_row_mapq(a.w, long_reads); p.cigar = cg; p.n_cigar = nc;
  }
  *out = c->h_proj.data(); *n_out = nr;
  return BR_OK;
}

// project_group_with (bramble-rs/src/api.rs:285-464), AoS in/out.  Shape and field meanings are the Rust library's;
// the values are the C++ path's: mates pair up by the C++ rule (name + position hash, src/bramble.cpp:272-311
// = k_mates), not by find_mate_pairs' mutual pointers (groups.rs:126-190), and hit_index is carried for layout parity
// only -- neither the C++ reader nor find_mate_pairs reads it.
// single_name: one call = one query name (br_project_group); else any number of name-collated groups (br_project_groups).
static int project_groups_impl(br_ctx *c, const br_config *cfg, const br_alignment *alns, size_t n, bool single_name,
                               const br_projected **out, size_t *n_out) {
  if (!c || !cfg || (!alns && n) || !out || !n_out) return BR_ERR_INVALID_ARG;
  *out = nullptr; *n_out = 0;
  std::vector<int32_t> ref_id, ref_start, mate_ref, mate_start, lq;
  std::vector<uint16_t> flags; std::vector<int8_t> xs, ts;
  std::vector<uint64_t> coff(1, 0), noff(1, 0), soff(1, 0);
  std::vector<uint32_t> cig; std::string names, seqs;
  std::vector<uint64_t> kept;          // batch position -> caller's index (alignments with ref_id < 0 are skipped, api.rs:316-318)
  std::vector<char> read_strand;       // infer_strand (api.rs:470-489) per kept alignment
  const char *name0 = n ? (alns[0].query_name ? alns[0].query_name : "") : "";
  bool any_seq = false;
  for (size_t i = 0; i < n; i++) {
    const br_alignment &a = alns[i];
    const char *nm = a.query_name ? a.query_name : "";
    // one call = one query name (GenomicAlignment::query_name: "shared by all alignments in the group", api.rs:74-75)
    if (single_name && strcmp(nm, name0) != 0) return BR_ERR_INVALID_ARG;
    if (a.ref_start < 0 || a.ref_start > 0x7fffffffll || a.mate_ref_start < 0 || a.mate_ref_start > 0x7fffffffll) return BR_ERR_INVALID_ARG;
    if ((a.n_cigar && !a.cigar) || (a.sequence_len && !a.sequence)) return BR_ERR_INVALID_ARG;
    if (a.ref_id < 0) continue;        // api.rs:316-318
    kept.push_back(i);
    ref_id.push_back(a.ref_id); ref_start.push_back((int32_t)a.ref_start);
    uint16_t f = 0;
    if (a.is_paired) { f |= 0x1; if (a.mate_is_unmapped) f |= 0x8; f |= a.is_first_in_pair ? 0x40 : 0x80; }
    if (a.is_reverse) f |= 0x10;
    flags.push_back(f); xs.push_back((int8_t)a.xs_strand); ts.push_back((int8_t)a.ts_strand);
    char rs = '.';
    if (a.xs_strand == '+' || a.xs_strand == '-') rs = a.xs_strand;
    else if (a.ts_strand == '+' || a.ts_strand == '-') rs = a.is_reverse ? (a.ts_strand == '+' ? '-' : '+') : a.ts_strand;
    read_strand.push_back(rs);
    mate_ref.push_back(a.mate_ref_id); mate_start.push_back((int32_t)a.mate_ref_start);
    cig.insert(cig.end(), a.cigar, a.cigar + a.n_cigar); coff.push_back(cig.size());
    names += nm; noff.push_back(names.size());
    // sequence: Option<Vec<u8>> (api.rs:91-95); the clip rescue shares the first one of the group (api.rs:308-312, src/core.cpp:353-378)
    if (a.sequence && a.sequence_len) { seqs.append(a.sequence, a.sequence_len); any_seq = true; }
    soff.push_back(seqs.size());
    lq.push_back((int32_t)(a.read_len ? a.read_len : a.sequence_len));   // api.rs:345-349
  }
  const size_t nk = kept.size();
  if (nk == 0) { c->h_proj.clear(); *out = c->h_proj.data(); return BR_OK; }   // api.rs:392-394
  br_batch b{};
  b.n_aln = (int64_t)nk; b.ref_id = ref_id.data(); b.ref_start = ref_start.data(); b.flags = flags.data();
  b.xs = xs.data(); b.ts = ts.data(); b.cigar_off = coff.data(); b.cigar = cig.data();
  b.mate_ref_id = mate_ref.data(); b.mate_start = mate_start.data(); b.name_off = noff.data();
  b.names = names.data(); b.l_qseq = lq.data();
  if (any_seq) { b.seq_off = soff.data(); b.seqs = seqs.data(); }
  else if (cfg->use_fasta && (cfg->lr || cfg->lr_hq)) { seqs.assign(1, 'N'); b.seq_off = soff.data(); b.seqs = seqs.data(); }  // no sequence: nothing to rescue
  // The lean way (a call that carries a name group or a few dozen of them): the input contract -- read-name groups, mate
  // index, the group's shared sequence -- on the host (a few alignments), ONE upload of everything, the device path
  // (without host round trips at this size), the packed rows and the CIGAR words they point at back in a handful of small
  // copies, and the record fields put together here.  The staged batch path (a dozen uploads, the contract on the device,
  // the wide row view, twenty-one downloads) is built for bundles; it stays the route for large calls.
  if (nk <= 8192) {
    int rc = project_groups_lean(c, cfg, b, kept, read_strand, out, n_out);
    if (rc != BR_RETRY_ORDINARY) return rc;
  }
  br_rows rows;
  RC(br_project_batch(c, cfg, &b, &rows));
  c->h_proj.resize((size_t)rows.n_rows);
  for (int64_t r = 0; r < rows.n_rows; r++) {
    br_projected &p = c->h_proj[(size_t)r];
    p.transcript_id = rows.transcript_id[r];
    p.transcript_start = rows.pos[r];
    p.aligned_len = (uint32_t)std::max(rows.aligned_len[r], 0);
    uint64_t e = (uint64_t)p.transcript_start + p.aligned_len;  // saturating add, then saturating sub 1
    if (e > 0xffffffffull) e = 0xffffffffull;
    p.transcript_end = e ? (uint32_t)(e - 1) : 0;
    const uint32_t *cg = rows.cigar + rows.cigar_off[r];
    uint32_t nc = (uint32_t)(rows.cigar_off[r + 1] - rows.cigar_off[r]);
    uint32_t qa = 0;
    for (uint32_t k = 0; k < nc; k++) {
      uint32_t op = cg[k] & 0xf;
      if (op == OP_M || op == OP_EQ || op == OP_X || op == OP_I || op == OP_MATCH_OVR || op == OP_INS_OVR) qa += cg[k] >> 4;
    }
    p.query_aligned_len = qa;
    const size_t bi = (size_t)rows.input_index[r];
    // api.rs:453 <- evaluate.rs:1062: the transcript's strand differs from the read's INFERRED strand ('.' for a read
    // without XS / ts: then true on either strand).  The C++ AlignInfo::is_reverse is never assigned (include/evaluate.h:157);
    // what the C++ path acts on is the transcript strand (src/bam.cpp:549-553): transcript_strand below.
    p.transcript_strand = (char)rows.strand[r];
    p.is_reverse = p.transcript_strand != read_strand[bi];
    p.similarity_score = rows.similarity_score[r];
    p.nh = rows.nh[r]; p.hi = rows.hi[r]; p.is_primary = rows.is_primary[r];
    p.same_transcript_as_mate = rows.same_transcript_as_mate[r]; p.is_paired_out = rows.is_paired[r];
    p.insert_size = rows.insert_size[r]; p.input_index = kept[bi];
    p.mapq = rows.mapq[r]; p.cigar = cg; p.n_cigar = nc;
  }
  *out = c->h_proj.data(); *n_out = c->h_proj.size();
  return BR_OK;
}

extern "C" int br_project_group(br_ctx *c, const br_config *cfg, const br_alignment *alns, size_t n,
                                const br_projected **out, size_t *n_out) {
  return project_groups_impl(c, cfg, alns, n, true, out, n_out);
}

// Many read-name groups per call (name-collated: each query name one contiguous run of `alns`): what a caller that holds
// batches of groups (bramble-cli batches 64, bramble-cli/src/pipeline.rs:29) should use -- one trip through the device
// pipeline instead of one per group.  NH / HI / primary are per query name, as in the per-group call.
extern "C" int br_project_groups(br_ctx *c, const br_config *cfg, const br_alignment *alns, size_t n,
                                 const br_projected **out, size_t *n_out) {
  return project_groups_impl(c, cfg, alns, n, false, out, n_out);
}

// Diagnostic: the -S rescue DP alone.  Runs k_ksw on n (target, query) pairs and returns, per pair, whether the rescue is
// accepted, the maximum, and the raw traceback CIGAR (forward order, BAM-packed M / I / D).  side (optional; null = all
// right): 0 = a left-side problem, whose strings the caller passes already reversed (align_reversed, src/evaluate.cpp:368-395),
// 1 = a right-side one.  refc / n_seg / seg (optional, all or none): what clip_segment made of the traceback -- KswRes.refc,
// KswRes.n_ops and the override ops read back from clip_ops[seq_off + p], seg[p * cigar_cap ...].
extern "C" int br_ctx_ksw_pairs(br_ctx *c, int64_t n, const char *const *tseq, const char *const *qseq, int32_t *ok,
                                int32_t *max, uint32_t *n_cigar, uint32_t *cigar, uint32_t cigar_cap, const uint8_t *side,
                                int32_t *refc, uint32_t *n_seg, uint32_t *seg) {
  if (!c || n < 0 || (n && (!tseq || !qseq || !ok || !max || !n_cigar || !cigar)) || !cigar_cap) return BR_ERR_INVALID_ARG;
  if ((refc || n_seg || seg) && !(refc && n_seg && seg)) return BR_ERR_INVALID_ARG;
  if (n == 0) return BR_OK;
  if (side) for (int64_t p = 0; p < n; p++) if (side[p] > 1) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  hipStream_t st = nullptr;
  struct HProb { uint32_t qlen, tlen, side, pad; uint64_t seq_off; };
  if (ksw_prob_bytes() != sizeof(HProb)) return BR_ERR_UNSUPPORTED;
  std::vector<HProb> probs((size_t)n);
  std::vector<uint8_t> arena;
  auto code = [](char ch) -> uint8_t { switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; } };
  uint64_t qmax = 0, tmaxv = 0;
  for (int64_t p = 0; p < n; p++) {
    size_t ql = strlen(qseq[p]), tl = strlen(tseq[p]);
    probs[(size_t)p] = HProb{(uint32_t)ql, (uint32_t)tl, side ? (uint32_t)side[p] : 1u, 0u, (uint64_t)arena.size()};
    for (size_t k = 0; k < ql; k++) arena.push_back(code(qseq[p][k]));
    for (size_t k = 0; k < tl; k++) { uint8_t cd = code(tseq[p][k]); probs[(size_t)p].pad |= cd >> 2; arena.push_back(cd); }
    qmax = std::max<uint64_t>(qmax, ql); tmaxv = std::max<uint64_t>(tmaxv, tl);
  }
  DevBuf d_probs, d_res, d_arena, d_ops, d_raw, d_rawn, d_max;
  int rc = BR_OK;
  struct HRes { int32_t ok, score, refc; uint32_t n_ops; };
  std::vector<HRes> res((size_t)n);
  std::vector<uint32_t> ops(seg ? arena.size() + (size_t)n + 1 : 0);
  do {
    if ((rc = d_probs.ensure((size_t)n * sizeof(HProb))) || (rc = d_res.ensure((size_t)n * ksw_res_bytes())) ||
        (rc = d_arena.ensure(arena.size() + 1024)) || (rc = d_ops.ensure((arena.size() + (size_t)n + 1) * 4)) ||
        (rc = d_raw.ensure((size_t)n * cigar_cap * 4)) || (rc = d_rawn.ensure((size_t)n * 4)) || (rc = d_max.ensure((size_t)n * 4))) break;
    KswRun R{};
    R.n_prob = n; R.probs = (const KswProb *)d_probs.p; R.results = (KswRes *)d_res.p; R.seq_arena = d_arena.as<uint8_t>();
    R.clip_ops = d_ops.as<uint32_t>(); R.seq_total = arena.size(); R.qmax = qmax; R.tmax = tmaxv; R.stats = nullptr;
    R.raw_out = d_raw.as<uint32_t>(); R.raw_n = d_rawn.as<uint32_t>(); R.max_out = d_max.as<int32_t>(); R.raw_cap = cigar_cap;
    if (hipMemsetAsync(d_max.p, 0, (size_t)n * 4, st) != hipSuccess || hipMemsetAsync(d_rawn.p, 0, (size_t)n * 4, st) != hipSuccess ||
        hipMemcpyAsync(d_probs.p, probs.data(), (size_t)n * sizeof(HProb), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_arena.p, arena.data(), arena.size(), hipMemcpyHostToDevice, st) != hipSuccess) { rc = BR_ERR_HIP; break; }
    if ((rc = run_ksw(c, st, R))) break;
    if (hipMemcpyAsync(res.data(), d_res.p, (size_t)n * sizeof(HRes), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(max, d_max.p, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(n_cigar, d_rawn.p, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(cigar, d_raw.p, (size_t)n * cigar_cap * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (seg && hipMemcpyAsync(ops.data(), d_ops.p, ops.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess) { rc = BR_ERR_HIP; break; }
    for (int64_t p = 0; p < n; p++) ok[p] = res[(size_t)p].ok;
    if (seg) for (int64_t p = 0; p < n; p++) {
      const HRes &r = res[(size_t)p];
      refc[p] = r.ok ? r.refc : 0; n_seg[p] = r.ok ? r.n_ops : 0;
      // a problem's ops lie in the qlen + tlen + 1 words from clip_ops[seq_off + p] on
      const uint32_t room = probs[(size_t)p].qlen + probs[(size_t)p].tlen + 1, take = std::min(std::min(n_seg[p], room), cigar_cap);
      memcpy(seg + (size_t)p * cigar_cap, ops.data() + probs[(size_t)p].seq_off + (size_t)p, (size_t)take * 4);
    }
  } while (0);
  return rc;
}
