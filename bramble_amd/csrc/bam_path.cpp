// BAM records in, BAM records out: the record encoder, the bundle entry points (staged, resident, nowait) and BGZF deflate
// on the device.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.h"

// aux_done: k_bam_scan already ran over these records with the same configuration
// (br_project_bam_device); keep_events: append to the running event list instead of restarting it; group_off / n_groups: the
// bundle's read-name groups (br_project_bam_device), for the unprojected records ("keep_unprojected"), else NULL
static int bam_encode_impl(br_ctx *c, const br_config *cfg, const br_device_records *recs, hipStream_t st,
                           br_device_bam *out, bool aux_done, bool keep_events, const uint32_t *group_off = nullptr, int64_t n_groups = 0) {
  memset(out, 0, sizeof(*out));
  if (recs->n_aln != c->last_n_aln) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  int64_t nr = c->last_n_rows, n = recs->n_aln;
  out->n_rows = nr;
  Prof pf{c, st};
  if (!keep_events) c->events_used = 0;
  BamArgs B{};
  B.n_aln = n; B.n_rows = nr; B.long_reads = (cfg->lr || cfg->lr_hq) ? 1 : 0;
  B.blob = recs->blob; B.rec_off = recs->rec_off; B.rec_len = recs->rec_len;
  RC(c->bam_aux.ensure(std::max<size_t>((size_t)n, 1) * sizeof(BamAux)));
  RC(c->bam_base.ensure(std::max<size_t>((size_t)n, 1) * 4));
  RC(c->bam_len.ensure(std::max<size_t>((size_t)nr, 1) * 4)); RC(c->bam_off.ensure(((size_t)nr + 1) * 8));
  B.aux = (BamAux *)c->bam_aux.p; B.base_len = c->bam_base.as<uint32_t>();
  RC(c->bam_end.ensure(BLOB_END_SLOTS * BLOB_END_STRIDE * 8)); B.blob_end = c->bam_end.as<uint64_t>();
  B.r_a = c->pk_a.as<uint4>(); B.r_c = c->pk_c.as<uint2>(); B.r_rec = c->r_rec.as<uint4>();
  if (c->last_direct) {   // no r_rec on the direct path: the detail column carries the input alignment and HI
    RC(ensure_detail(c, st));
    B.r_rec = c->pk_x.as<uint4>(); B.rec_x = 1;
  }
  B.r_sim = c->last_aux_cols ? c->pk_sim.as<double>() : nullptr; B.r_clip = c->last_aux_cols ? c->pk_clip.as<int32_t>() : nullptr;
  B.pool = c->cig_arena.as<uint32_t>(); B.l_qseq = c->last_l_qseq;
  B.out_len = c->bam_len.as<uint32_t>(); B.out_off = c->bam_off.as<uint64_t>();
  RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for(nr + 1), 1) * 8 * 3));
  RC(ensure_totals(c));
  uint64_t *d_tot = c->totals.as<uint64_t>();
  B.too_long = d_tot + TOT_BAM_LONG;
  HIPCHK(hipMemsetAsync(B.too_long, 0, 8, st));
  RC(pf.begin(BR_K_BAM));
  if (!aux_done) { HIPCHK(hipMemsetAsync(B.blob_end, 0, BLOB_END_SLOTS * BLOB_END_STRIDE * 8, st)); launch_bam_scan(st, B); }
  launch_bam_size(st, B);
  RC(pf.end());
  RC(pf.begin(BR_K_SCAN));
  launch_scan(st, B.out_len, nr, c->tile_sums.as<uint64_t>(), c->bam_off.p, true, d_tot + TOT_BAM_BYTES);
  RC(pf.end());
  // the records without an output row: measured here, so that their totals come home with the encoder's size
  const bool unproj = group_off && c->un.keep;
  UnprojArgs U{};
  if (unproj) RC(unproj_measure(c, st, pf, B, group_off, n_groups, U));
  HIPCHK(hipMemcpyAsync(c->rb->bam, d_tot + TOT_BAM_LONG, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // (bam[0], "a spilled CIGAR spans 2^28 reference bases or more", is set by the encoder: checked after it)
  uint64_t total = nr ? c->rb->bam[1] : 0;
  RC(c->bam_out.ensure(std::max<size_t>(total, 16)));
  B.out = c->bam_out.as<uint8_t>();
  RC(pf.begin(BR_K_BAM));
  launch_bam_encode(st, B, c->bam_lanes);
  RC(pf.end());
  if (unproj) RC(unproj_gather(c, st, pf, U));   // complete at the synchronise below: the caller may release the input then
  HIPCHK(hipMemcpyAsync(c->rb->bam, d_tot + TOT_BAM_LONG, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (nr && c->rb->bam[0]) { pf.collect(); return BR_ERR_UNSUPPORTED; }  // bam_write1 refuses such a record too
  RC(pf.collect());
  if (unproj) unproj_commit(c, U);
  out->data = c->bam_out.as<uint8_t>(); out->n_bytes = total; out->row_off = c->bam_off.as<uint64_t>();
  return BR_OK;
}

extern "C" int br_bam_encode_device(br_ctx *c, const br_config *cfg, const br_device_records *recs, void *stream,
                                    br_device_bam *out) {
  if (!c || !cfg || !recs || !out) return BR_ERR_INVALID_ARG;
  return bam_encode_impl(c, cfg, recs, (hipStream_t)stream, out, false, false);
}

// ---------------------------------------------------------------------------
// BAM bundle entry: records -> input tables -> projection -> records
// ---------------------------------------------------------------------------
extern "C" int br_project_bam_device(br_ctx *c, const br_config *cfg, const br_device_records *recs,
                                     const int32_t *ref_map, int32_t n_ref_map, void *stream,
                                     br_device_rows *rows_out, br_device_bam *out) {
  if (!c || !cfg || !recs || !out || n_ref_map < 0 || (n_ref_map && !ref_map)) return BR_ERR_INVALID_ARG;
  if (recs->n_aln && (!recs->blob || !recs->rec_off)) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  br_device_rows local_rows;
  br_device_rows *rows = rows_out ? rows_out : &local_rows;
  memset(rows, 0, sizeof(*rows));
  hipStream_t st = (hipStream_t)stream;
  const br_index *ix = c->ix;
  DevCfg dc;
  RC(make_devcfg(cfg, dc));
  const bool fa_mode = dc.use_fasta && dc.long_reads;
  int64_t n = recs->n_aln;
  if (n < 0 || n >= 0x7fffffffll) return BR_ERR_CAPACITY;
  HIPCHK(hipSetDevice(ix->device));
  c->last_n_aln = n; c->last_n_rows = 0;
  c->events_used = 0;
  Prof pf{c, st};
  if (n == 0) { c->forget_last_call(st); pf.collect(); return BR_OK; }

  size_t nn = (size_t)n;
  RC(c->b_ref_id.ensure(nn * 4)); RC(c->b_ref_start.ensure(nn * 4)); RC(c->b_flags.ensure(nn * 2));
  RC(c->b_xs.ensure(nn)); RC(c->b_ts.ensure(nn)); RC(c->b_lqseq.ensure(nn * 4));
  RC(c->b_cigar_off.ensure((nn + 1) * 4)); RC(c->b_name_off.ensure((nn + 1) * 4)); RC(c->b_mate_idx.ensure(nn * 4));
  RC(c->p_ncig.ensure(nn * 4)); RC(c->p_name_len.ensure(nn * 4)); RC(c->p_isnew.ensure(nn * 4));
  RC(c->p_group_pre.ensure((nn + 1) * 4)); RC(c->p_small.ensure(64)); RC(c->p_big.ensure((nn / 96 + 2) * 4));
  RC(c->p_ref_map.ensure(std::max<size_t>((size_t)n_ref_map, 1) * 4));
  RC(c->bam_aux.ensure(nn * sizeof(BamAux)));
  RC(c->bam_base.ensure(nn * 4));
  RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for(n + 1), 1) * 8 * 3));
  RC(ensure_totals(c));
  if (n_ref_map) HIPCHK(hipMemcpyAsync(c->p_ref_map.p, ref_map, (size_t)n_ref_map * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->p_small.p, 0, 64, st));  // [0] max n_cigar, [1] max soft clip, [2] big-group count

  ParseArgs P{};
  P.n = n; P.blob = recs->blob; P.rec_off = recs->rec_off; P.rec_len = recs->rec_len;
  P.ref_map = c->p_ref_map.as<int32_t>(); P.n_ref_map = n_ref_map;
  P.ref_id = c->b_ref_id.as<int32_t>(); P.ref_start = c->b_ref_start.as<int32_t>(); P.l_qseq = c->b_lqseq.as<int32_t>();
  P.flags = c->b_flags.as<uint16_t>(); P.ncig = c->p_ncig.as<uint32_t>(); P.name_len = c->p_name_len.as<uint32_t>();
  P.isnew = c->p_isnew.as<uint32_t>(); P.maxima = c->p_small.as<uint32_t>(); P.n_big_groups = c->p_small.as<uint32_t>() + 2;
  P.big_groups = c->p_big.as<uint32_t>(); P.group_pre = c->p_group_pre.as<uint32_t>();
  P.cigar_off = c->b_cigar_off.as<uint32_t>(); P.name_off = c->b_name_off.as<uint32_t>(); P.mate_idx = c->b_mate_idx.as<int32_t>();

  BamArgs B{};
  B.n_aln = n; B.long_reads = dc.long_reads ? 1 : 0; B.blob = recs->blob; B.rec_off = recs->rec_off; B.rec_len = recs->rec_len;
  B.aux = (BamAux *)c->bam_aux.p; B.base_len = c->bam_base.as<uint32_t>(); B.xs_out = c->b_xs.as<int8_t>(); B.ts_out = c->b_ts.as<int8_t>();
  RC(c->bam_end.ensure(BLOB_END_SLOTS * BLOB_END_STRIDE * 8)); B.blob_end = c->bam_end.as<uint64_t>();
  HIPCHK(hipMemsetAsync(B.blob_end, 0, BLOB_END_SLOTS * BLOB_END_STRIDE * 8, st));

  // the aux walk of the records (one lane per record, latency-bound) on the side stream beside the reader side
  // (k_rec_fields .. k_mates, the same kind of kernel over the same records): joined below, in front of the projection
  RC(ensure_side_stream(c));
  SideWork aux_walk(c, st, c->side_stream);
  RC(aux_walk.fork());
  RC(pf.begin(BR_K_BAM, c->side_stream));
  launch_bam_scan(c->side_stream, B);
  RC(pf.end());
  RC(aux_walk.done());
  RC(pf.begin(BR_K_PARSE));
  launch_rec_fields(st, P);
  RC(pf.end());
  uint64_t *d_tot = c->totals.as<uint64_t>();
  uint64_t *const ts = c->tile_sums.as<uint64_t>();
  RC(pf.begin(BR_K_SCAN));
  launch_scan(st, P.ncig, n, ts, c->b_cigar_off.p, false, d_tot + TOT_PARSE_CIGAR);
  launch_scan(st, P.name_len, n, ts, c->b_name_off.p, false, d_tot + TOT_PARSE_NAMES);
  launch_scan(st, P.isnew, n, ts, c->p_group_pre.p, false, d_tot + TOT_PARSE_GROUPS);
  RC(pf.end());
  HIPCHK(hipMemcpyAsync(c->rb->parse_n, d_tot + TOT_PARSE_CIGAR, 3 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&c->rb->parse_max, c->p_small.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t n_words = c->rb->parse_n[0], name_bytes = c->rb->parse_n[1], ng = c->rb->parse_n[2];
  uint32_t max_nc = (uint32_t)(c->rb->parse_max & 0xffffffffu), max_clip = (uint32_t)(c->rb->parse_max >> 32);
  if (n_words >= 0xffffffffull - (uint64_t)n || name_bytes >= 0xfffffff0ull) { pf.collect(); return BR_ERR_CAPACITY; }
  RC(c->b_cigar.ensure(std::max<size_t>((size_t)n_words, 1) * 4)); RC(c->b_names.ensure(std::max<size_t>((size_t)name_bytes, 1)));
  RC(c->b_group_off.ensure(((size_t)ng + 1) * 4));
  P.n_groups = (int64_t)ng; P.group_off = c->b_group_off.as<uint32_t>();
  P.cigar = c->b_cigar.as<uint32_t>(); P.names = c->b_names.as<uint8_t>();
  RC(pf.begin(BR_K_PARSE));
  launch_group_off(st, P);
  launch_rec_copy(st, P);
  launch_mates(st, P);
  RC(pf.end());
  RC(aux_walk.join());   // k_bam_scan: XS / ts characters, the aux table

  br_device_batch db{};
  if (fa_mode) {
    RC(c->b_seq_src.ensure(nn * 4)); RC(c->p_seq_len.ensure(nn * 4)); RC(c->b_seq_off.ensure((nn + 1) * 4));
    P.seq_src = c->b_seq_src.as<int32_t>(); P.seq_len = c->p_seq_len.as<uint32_t>(); P.seq_off = c->b_seq_off.as<uint32_t>();
    RC(pf.begin(BR_K_PARSE));
    launch_seq_src(st, P);
    RC(pf.end());
    RC(pf.begin(BR_K_SCAN));
    launch_scan(st, P.seq_len, n, ts, c->b_seq_off.p, false, d_tot + TOT_PARSE_SEQ);
    RC(pf.end());
    HIPCHK(hipMemcpyAsync(&c->rb->parse_seq, d_tot + TOT_PARSE_SEQ, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t sbytes = c->rb->parse_seq;
    if (sbytes >= 0xfffffff0ull) { pf.collect(); return BR_ERR_CAPACITY; }
    RC(c->b_seqs.ensure(std::max<size_t>((size_t)sbytes, 1)));
    P.seqs = c->b_seqs.as<uint8_t>();
    RC(pf.begin(BR_K_PARSE));
    launch_seq_ascii(st, P);
    RC(pf.end());
    db.seq_off = P.seq_off; db.seqs = P.seqs; db.seq_src = P.seq_src; db.max_soft_clip = (int32_t)max_clip;
  }
  db.n_aln = n; db.n_groups = (int64_t)ng; db.ref_id = P.ref_id; db.ref_start = P.ref_start; db.flags = P.flags;
  db.xs = c->b_xs.as<int8_t>(); db.ts = c->b_ts.as<int8_t>(); db.cigar_off = P.cigar_off; db.cigar = P.cigar;
  db.mate_idx = P.mate_idx; db.group_off = P.group_off; db.l_qseq = P.l_qseq;
  db.n_cigar_words = (int64_t)n_words; db.max_n_cigar = (int32_t)max_nc;
  db.name_off = P.name_off; db.names = P.names;
  { WantDetail wd(c, true); RC(run_device(c, cfg, &db, st, rows, true)); }   // the encoder reads input alignment and HI of every row
  RC(bam_encode_impl(c, cfg, recs, st, out, true, true, P.group_off, (int64_t)ng));
  return BR_OK;
}

// ---------------------------------------------------------------------------
// BGZF deflate on the device
// ---------------------------------------------------------------------------
static int deflate_device_impl(br_ctx *c, const uint8_t *src, uint64_t n, hipStream_t st, const uint8_t **out, uint64_t *out_bytes,
                               bool keep_events) {
  *out = nullptr; *out_bytes = 0;
  Prof pf{c, st};
  if (!keep_events) c->events_used = 0;
  if (n == 0) { if (!keep_events) pf.collect(); return BR_OK; }
  if (!c->z_tabs_ready) {
    // CRC-32 (reflected 0xEDB88320) byte table and the operator that appends DEFLATE_CRC_CHUNK zero bytes to a
    // register (zlib's crc32_combine does the same with squared matrices; here the length is fixed)
    std::vector<uint32_t> t(256 + 1024);
    for (uint32_t i = 0; i < 256; i++) { uint32_t v = i; for (int k = 0; k < 8; k++) v = (v & 1u) ? 0xEDB88320u ^ (v >> 1) : v >> 1; t[i] = v; }
    uint32_t col[32];
    for (int b = 0; b < 32; b++) { uint32_t v = 1u << b; for (uint32_t k = 0; k < DEFLATE_CRC_CHUNK; k++) v = (v >> 8) ^ t[v & 0xffu]; col[b] = v; }
    for (int byte = 0; byte < 4; byte++)
      for (uint32_t x = 0; x < 256; x++) { uint32_t v = 0; for (int b = 0; b < 8; b++) if (x & (1u << b)) v ^= col[8 * byte + b]; t[256 + 256 * byte + x] = v; }
    RC(c->z_tabs.ensure(t.size() * 4));
    HIPCHK(hipMemcpyAsync(c->z_tabs.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    c->z_tabs_ready = true;
  }
  uint64_t nb = (n + DEFLATE_PAYLOAD - 1) / DEFLATE_PAYLOAD;
  RC(c->z_slots.ensure((size_t)nb * DEFLATE_SLOT)); RC(c->z_sizes.ensure((size_t)nb * 4)); RC(c->z_off.ensure(((size_t)nb + 1) * 8));
  RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for((int64_t)nb + 1), 1) * 8 * 3));
  RC(ensure_totals(c));
  uint64_t *d_tot = c->totals.as<uint64_t>();
  DeflateArgs A{};
  A.src = src; A.n_bytes = n; A.n_blocks = nb; A.slots = c->z_slots.as<uint8_t>(); A.sizes = c->z_sizes.as<uint32_t>();
  A.crc_tab = c->z_tabs.as<uint32_t>(); A.crc_shift = c->z_tabs.as<uint32_t>() + 256;
  int dyn_waves = 0;
  if (c->deflate_dynamic) {  // persistent waves: as many as the chip holds (6 workgroups of 4 waves per CU by their LDS), a token list each
    uint64_t want = (uint64_t)c->n_cu * 24;
    if (c->deflate_waves > 0) want = std::min<uint64_t>(want, ((uint64_t)c->deflate_waves + 3) / 4 * 4);   // fewer waves, more blocks each
    dyn_waves = (int)std::min<uint64_t>((nb + 3) / 4 * 4, want / 4 * 4);
    if (dyn_waves < 4) dyn_waves = 4;
    RC(c->z_tokens.ensure((size_t)dyn_waves * DEFLATE_PAYLOAD * 4 + 64));
#ifdef DEFLATE_PROFILE
    HIPCHK(hipMemsetAsync(c->z_tokens.as<uint8_t>() + (size_t)dyn_waves * DEFLATE_PAYLOAD * 4, 0, 64, st));
#endif
    A.tokens = c->z_tokens.as<uint32_t>();
    A.queue = (uint32_t *)(d_tot + TOT_DEFLATE_QUEUE);
    HIPCHK(hipMemsetAsync(A.queue, 0, 8, st));
  }
  RC(pf.begin(BR_K_CODEC));
  launch_deflate(st, A, dyn_waves);
  RC(pf.end());
#ifdef DEFLATE_PROFILE
  if (dyn_waves) {
    uint64_t pt[8];
    HIPCHK(hipMemcpyAsync(pt, c->z_tokens.as<uint8_t>() + (size_t)dyn_waves * DEFLATE_PAYLOAD * 4, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double tot = 0; for (int k = 0; k < 8; k++) tot += (double)pt[k];
    static const char *nm[8] = {"clear", "parse_step", "tokens+hist", "code build", "header", "replay", "crc+frame", "claim"};
    for (int k = 0; k < 8; k++) fprintf(stderr, "[deflate profile] %-12s %5.1f %%\n", nm[k], 100.0 * (double)pt[k] / tot);
  }
#endif
  RC(pf.begin(BR_K_SCAN));
  launch_scan(st, A.sizes, (int64_t)nb, c->tile_sums.as<uint64_t>(), c->z_off.p, true, d_tot + TOT_DEFLATE);
  RC(pf.end());
  HIPCHK(hipMemcpyAsync(&c->rb->deflate_total, d_tot + TOT_DEFLATE, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t total = c->rb->deflate_total;
  DevBuf &dense = c->z_dense_which ? c->z_dense_alt : c->z_dense;
  RC(dense.ensure((size_t)total + 16));
  RC(pf.begin(BR_K_CODEC));
  launch_bgzf_compact(st, A, c->z_off.as<uint64_t>(), dense.as<uint8_t>());
  RC(pf.end());
  if (!keep_events) { HIPCHK(hipStreamSynchronize(st)); RC(pf.collect()); }
  *out = dense.as<uint8_t>(); *out_bytes = total;
  return BR_OK;
}

extern "C" int br_bgzf_deflate_device(br_ctx *c, const uint8_t *src, uint64_t n, void *stream, const uint8_t **out,
                                      uint64_t *out_bytes) {
  if (!c || (!src && n) || !out || !out_bytes) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  return deflate_device_impl(c, src, n, (hipStream_t)stream, out, out_bytes, false);
}

extern "C" int br_bam_bundle_stage(br_ctx *c, const br_bam_bundle *bb, int slot) {
  if (!c || !bb || slot < 0 || slot > 2) return BR_ERR_INVALID_ARG;
  int64_t n = bb->n_records;
  if (n < 0 || (n && (!bb->blob || !bb->rec_off || !bb->rec_len))) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  br_ctx::StageSlot &S = c->stage[slot];
  if (!c->copy_stream) { int pl = 0, ph = 0; HIPCHK(hipDeviceGetStreamPriorityRange(&pl, &ph)); HIPCHK(hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, ph)); }   // (see ensure_streams)
  if (!S.ready) HIPCHK(hipEventCreateWithFlags(&S.ready, hipEventDisableTiming));
  S.n = n;
  if (n) {
    // upload only the span the records cover
    uint64_t lo = bb->rec_off[0], hi = bb->rec_off[n - 1] + bb->rec_len[n - 1];
    if (hi > bb->n_bytes || lo > hi) return BR_ERR_INVALID_ARG;
    RC(S.blob.ensure((size_t)(hi - lo) + 16)); RC(S.off.ensure((size_t)n * 8)); RC(S.len.ensure((size_t)n * 4));
    S.h_off.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) S.h_off[(size_t)i] = bb->rec_off[i] - lo;
    HIPCHK(hipMemcpyAsync(S.blob.p, bb->blob + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(hipMemcpyAsync(S.off.p, S.h_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(hipMemcpyAsync(S.len.p, bb->rec_len, (size_t)n * 4, hipMemcpyHostToDevice, c->copy_stream));
  }
  HIPCHK(hipEventRecord(S.ready, c->copy_stream));
  return BR_OK;
}

// a record stream in HBM -> its bytes (or its BGZF blocks, or its SAM lines) in one of the two pinned host buffers.  note: the
// BRAMBLE_AMD_TIMING line's front (what came before the stream), or NULL
static int device_bam_home(br_ctx *c, br_device_bam db, int out_mode, bool nowait, const char *note, br_host_bam *out) {
  static const bool timing = getenv("BRAMBLE_AMD_TIMING") != nullptr;
  auto tnow = []() { return std::chrono::steady_clock::now(); };
  auto tms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  hipStream_t st = nullptr;
  auto t2 = tnow();
  int hs = c->h_bam_next; c->h_bam_next ^= 1;
  if (c->home_pending[hs]) { HIPCHK(hipEventSynchronize(c->ev_home[hs])); c->home_pending[hs] = false; }   // (a caller that never asked)
  const bool later = nowait && out_mode && db.n_bytes;
  if (out_mode == 1 && db.n_bytes) {
    c->z_dense_which = hs;
    const uint8_t *z = nullptr; uint64_t zn = 0;
    RC(deflate_device_impl(c, db.data, db.n_bytes, st, &z, &zn, false));
    db.data = z; db.n_bytes = zn;
  } else if (out_mode == BR_OUT_SAM_TEXT && db.n_bytes) {   // the lines, where the BGZF blocks would be made (sam_writer.cpp)
    c->sf_which = hs;
    const uint8_t *t = nullptr; uint64_t tn = 0;
    RC(sam_format_impl(c, &db, st, &t, &tn));
    db.data = t; db.n_bytes = tn;
  }
  auto t3 = tnow();
  if (db.n_bytes > c->h_bam_cap[hs]) {
    c->h_bam[hs] = nullptr; c->h_bam_cap[hs] = 0;
    size_t want = (size_t)db.n_bytes + (size_t)db.n_bytes / 4 + 4096;
    RC(c->h_bam_mem[hs].alloc(want));
    c->h_bam[hs] = c->h_bam_mem[hs].p; c->h_bam_cap[hs] = c->h_bam_mem[hs].cap;
  }
  if (later) {
    // everything on `st` is complete (the deflate step ends with the block sizes on the host, the SAM step with its text made): the copy goes to a stream of its
    // own and the caller asks for it with br_host_bam_wait, so the next bundle's kernels start without the 4 ms of PCIe in front
    if (!c->down_stream) HIPCHK(hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
    if (!c->ev_home[hs]) HIPCHK(hipEventCreateWithFlags(&c->ev_home[hs], hipEventDisableTiming));
    HIPCHK(hipMemcpyAsync(c->h_bam[hs], db.data, (size_t)db.n_bytes, hipMemcpyDeviceToHost, c->down_stream));
    HIPCHK(hipEventRecord(c->ev_home[hs], c->down_stream));
    c->home_pending[hs] = true;
  } else {
    if (db.n_bytes) HIPCHK(hipMemcpyAsync(c->h_bam[hs], db.data, (size_t)db.n_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (timing && note) fprintf(stderr, "%s, deflate / format %.1f ms, download of %.0f MB %.1f ms\n", note, tms(t2, t3), (double)db.n_bytes / 1e6, tms(t3, tnow()));
  out->data = c->h_bam[hs]; out->n_bytes = db.n_bytes; out->n_rows = db.n_rows;
  return BR_OK;
}

// records in HBM -> projected records (or their BGZF blocks, or their SAM lines) in pinned host memory, or left in HBM
// (BR_OUT_RESIDENT): the part the staged and the resident entry points share.  out_mode: br_bam_bundle.bgzf_on_device
static int project_bam_tail(br_ctx *c, const br_config *cfg, const br_device_records *dr, const int32_t *ref_map, int32_t n_ref_map,
                            int out_mode, bool nowait, double wait_ms, br_host_bam *out) {
  static const bool timing = getenv("BRAMBLE_AMD_TIMING") != nullptr;
  hipStream_t st = nullptr;
  auto t1 = std::chrono::steady_clock::now();
  br_device_rows rows; br_device_bam db;
  c->last_bam = br_device_bam{};
  RC(br_project_bam_device(c, cfg, dr, ref_map, n_ref_map, st, &rows, &db));
  char note[160]; note[0] = 0;
  if (timing) snprintf(note, sizeof note, "[bundle] %lld records: upload wait %.1f ms, records -> records %.1f ms", (long long)dr->n_aln, wait_ms,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  c->last_bam = db;   // in every output mode: the buffer lives until the context's next call (br_sorter and br_assign take it from there)
  if (out_mode == BR_OUT_RESIDENT) { out->n_rows = db.n_rows; if (timing) fprintf(stderr, "%s, kept in HBM\n", note); }
  else RC(device_bam_home(c, db, out_mode, nowait, note, out));
  out->total_complete = rows.total_complete; out->total_unique = rows.total_unique;
  out->dropped_reads = rows.dropped_reads; out->total_processed = rows.total_processed;
  return BR_OK;
}

extern "C" int br_ctx_last_device_bam(const br_ctx *c, br_device_bam *out) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  *out = c->last_bam;
  return BR_OK;
}

extern "C" int br_device_bam_download(br_ctx *c, const br_device_bam *in, int out_mode, int nowait, br_host_bam *out) {
  if (!c || !in || !out || (in->n_bytes && (!in->data || !in->row_off)) || (out_mode != 0 && out_mode != 1 && out_mode != BR_OUT_SAM_TEXT)) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  HIPCHK(hipSetDevice(c->ix->device));
  return device_bam_home(c, *in, out_mode, nowait != 0, nullptr, out);
}

// bgzf_on_device: BR_OUT_SAM_TEXT, or BGZF blocks for any other value than 0 (as before there was a third output)
static int out_mode_of(int v) { return v == BR_OUT_SAM_TEXT || v == BR_OUT_RESIDENT ? v : v != 0 ? 1 : 0; }

static int project_bam_staged_impl(br_ctx *c, const br_config *cfg, const br_bam_bundle *bb, int slot, br_host_bam *out, bool nowait) {
  if (!c || !cfg || !bb || !out || slot < 0 || slot > 2) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  br_ctx::StageSlot &S = c->stage[slot];
  if (!S.ready || S.n != bb->n_records) return BR_ERR_INVALID_ARG;   // not staged (or another bundle was)
  HIPCHK(hipSetDevice(c->ix->device));
  int64_t n = S.n;
  out->total_processed = (uint64_t)n;
  auto t0 = std::chrono::steady_clock::now();
  HIPCHK(hipEventSynchronize(S.ready));
  const double wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (n == 0) { c->forget_last_call(nullptr); return BR_OK; }   // a bundle without records: a call that leaves nothing behind
  br_device_records dr{S.blob.as<uint8_t>(), S.off.as<uint64_t>(), n, S.len.as<uint32_t>()};
  return project_bam_tail(c, cfg, &dr, bb->ref_map, bb->n_ref_map, out_mode_of(bb->bgzf_on_device), nowait, wait_ms, out);
}

extern "C" int br_project_bam_resident(br_ctx *c, const br_config *cfg, const br_device_records *recs, const int32_t *ref_map, int32_t n_ref_map,
                                       int bgzf_on_device, int nowait, br_host_bam *out) {
  if (!c || !cfg || !recs || !out || recs->n_aln < 0 || (recs->n_aln && (!recs->blob || !recs->rec_off))) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  HIPCHK(hipSetDevice(c->ix->device));
  out->total_processed = (uint64_t)recs->n_aln;
  if (recs->n_aln == 0) { c->forget_last_call(nullptr); return BR_OK; }
  return project_bam_tail(c, cfg, recs, ref_map, n_ref_map, out_mode_of(bgzf_on_device), nowait != 0, 0.0, out);
}

extern "C" int br_project_bam_staged(br_ctx *c, const br_config *cfg, const br_bam_bundle *bb, int slot, br_host_bam *out) {
  return project_bam_staged_impl(c, cfg, bb, slot, out, false);
}
extern "C" int br_project_bam_staged_nowait(br_ctx *c, const br_config *cfg, const br_bam_bundle *bb, int slot, br_host_bam *out) {
  return project_bam_staged_impl(c, cfg, bb, slot, out, true);
}
extern "C" int br_host_bam_wait(br_ctx *c, const br_host_bam *hb) {
  if (!c || !hb) return BR_ERR_INVALID_ARG;
  for (int k = 0; k < 2; k++)
    if (hb->data && hb->data == c->h_bam[k] && c->home_pending[k]) {
      HIPCHK(hipSetDevice(c->ix->device));
      HIPCHK(hipEventSynchronize(c->ev_home[k]));
      c->home_pending[k] = false;
    }
  return BR_OK;
}

extern "C" int br_project_bam_bundle(br_ctx *c, const br_config *cfg, const br_bam_bundle *bb, br_host_bam *out) {
  if (!c || !cfg || !bb || !out) return BR_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  RC(br_bam_bundle_stage(c, bb, 0));
  return br_project_bam_staged(c, cfg, bb, 0, out);
}
