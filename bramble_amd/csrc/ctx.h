// Internal to libbramble_amd.so: the index and context types, and the functions the host units share.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cassert>
#include <string>
#include <vector>

#include "../../include/bramble_amd.h"
#include "device_types.h"
#include "devmem.h"
#include "kernels.h"
#include "unprojected_kernels.h"

using namespace br;

struct br_index {
  int device = -1;
  std::vector<std::string> names;
  std::vector<uint32_t> lengths;
  uint32_t n_refs = 0;
  bool has_seq = false;
  // host copies of the flattened tables
  std::vector<uint32_t> slab_off, s_start, s_pmax, s_tid, tx_first, bin_off;
  std::vector<uint4> t_bin;
  std::vector<uint4> s_row, tx_ex;
  std::vector<uint8_t> seq_pool;
  // device copies
  void *d_slab_off = nullptr, *d_s_start = nullptr, *d_s_pmax = nullptr, *d_bin_off = nullptr, *d_t_bin = nullptr, *d_s_tid = nullptr,
       *d_s_row = nullptr, *d_tx_ex = nullptr, *d_tx_first = nullptr, *d_seq_pool = nullptr;
  size_t device_bytes = 0;
  DevIndex dev{};
};

struct KEvent { int which; hipEvent_t a, b; };

// The pinned read-back page (br_ctx::rb, one hipHostMalloc): every word a device-to-host copy brings home, named for what
// it holds and grouped by owner.  No member has two owners; words that one copy fetches together are one array.
struct ReadBack {
  // the projection (pipeline.cpp)
  uint64_t scan[5];                       // TOT_MATCHES .. TOT_RAW as the scans left them (the row scan: scan[TOT_ROWS] alone)
  uint64_t counters[4];                   // PairArgs::counters of the call: -, unique reads, dropped reads, a field overflowed its width
  uint64_t small[TOT_SMALL_CNT + 4];      // run_device_small: the totals up to its counter block, one copy at the end
  uint64_t direct_cnt[GD_COUNTER_WORDS];  // run_device_direct: the four counters + k_group_desc's slots
  uint64_t side[2];                       //   its side arena: entries asked for, overflowed
  uint64_t wide_cigar;                    // expand_rows: CIGAR words of the wide view
  // the -S rescue
  uint64_t rescue_n[2];                 // problems, sequence bytes (TOT_RESCUE_PROB, TOT_RESCUE_SEQ)
  uint64_t rescue_stats[2];               // DP cells, accepted rescues
  uint32_t ksw_bins[16];                  // run_ksw: k_ksw_bin's counters of a piece (problems per bin, leftovers, maxima, tape rows)
  uint64_t ksw_left_after;                // leftovers of the last piece after the DP (br_ctx_ksw_diag out[7]; low 32 bits)
  // BAM in and out (bam_path.cpp)
  uint64_t parse_n[3];                  // CIGAR words, name bytes, read-name groups (TOT_PARSE_CIGAR ..)
  uint64_t parse_seq;                     // sequence bytes (-S)
  uint64_t parse_max;                     // max n_cigar | max soft clip << 32
  uint64_t bam[2];                        // the encoder: a record it cannot write, the records' bytes (TOT_BAM_LONG, TOT_BAM_BYTES)
  uint64_t deflate_total;                 // compressed bytes of a BGZF call
  uint64_t unproj[UNPROJ_SMALL_N];        // the unprojected records of a call: bytes, records, names without / with some record projected
  // flat batches (host_rows.cpp)
  uint64_t host_groups, host_max, host_pool;   // read-name groups, max n_cigar | max soft clip << 32, dense pool words
  // SAM text out (sam_writer.cpp)
  uint64_t sam_bad, sam_bytes;            // the first record the text cannot say (~0: none), the text's bytes
};

// The input records of the bundle calls that got no output record, kept in HBM until drawn (unprojected.cpp).
struct Unprojected {
  int keep = 0;                 // "keep_unprojected": 0 off, 1 scope record, 2 scope name
  uint64_t first_cap = 0;       // "unprojected_cap": the arena's first capacity in bytes (a test hook)
  ColBuf arena, off;            // [block_size][record]... in input order; off: n + 1 offsets, the last one = used
  ColBuf old_arena, old_off;    // what a growing call replaced: freed behind that call's last synchronise
  uint64_t used = 0; int64_t n = 0, cur = 0;   // arena bytes and records held; the next record br_ctx_unprojected_next hands out
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};     // br_ctx_unprojected_stats [0..5]
  uint64_t live = 0, peak = 0;  // device bytes of the arenas now / at most
  DevBuf flag, len, one, out_off, rank, small, piece_rows;   // a call's tables; the row_off of the last piece
  void drop(ColBuf &b) { live -= b.cap; b.release(); }
};

struct br_ctx {
  const br_index *ix = nullptr;
  Unprojected un;
  int group_lanes = 8;
  int bam_lanes = 0;   // 0: k_bam_tasks (a wave per 32 rows); 4..64: k_bam_encode<G>, G lanes per row
  int blocks_per_cu = 8;
  int split_spoil = 0;   // test hook: k_split_spoil plants wrong segment guesses (tests/test_gpu_split.py)
  int n_cu = 256;
  bool profiling = false;
  std::vector<KEvent> events; size_t events_used = 0;
  double k_ms[BR_K_NUM] = {0}; int32_t k_launches[BR_K_NUM] = {0};
  double k_ms_sum[BR_K_NUM] = {0}; int64_t k_launches_sum[BR_K_NUM] = {0};   // over the calls since profiling was switched on (br_ctx_kernel_ms_sum)
  uint64_t counters[8] = {0};
  uint64_t rescue_stats[4] = {0};  // problems, DP cells, accepted rescues, coded sequence bytes
  // device scratch
  DevBuf seg, meta, head, head2, fast_flag, fast_pre, n_matches, ranges, mask, match_off, cig_base, tile_sums, totals, counters_d;
  DevBuf m_tid, m_aux, m_p, m_x, m_b, m_cigoff, cig_arena, big_list, n_big, m_aln;
  DevBuf bam_aux, bam_base, bam_len, bam_off, bam_out, bam_end;
  struct StageSlot { DevBuf blob, off, len; hipEvent_t ready = nullptr; std::vector<uint64_t> h_off; int64_t n = 0; };
  StageSlot stage[3];              // br_bam_bundle_stage: uploads of the next bundles overlap the current projection
  hipStream_t copy_stream = nullptr;
  // flat (br_batch) staging: two input slots, uploads on copy_stream; packed rows go back on d2h_stream into the
  // slot's pinned arrays while the next batch is being projected on run_stream
  struct InSlot {
    DevBuf ref_id, ref_start, flags, xs, ts, cigar_off64, cigar, mate_ref, mate_start, name_off64, names, lqseq, seq_off64, seqs;
    DevBuf cigar_off, name_off, seq_off, mate_idx, group_off, seq_src, isnew, group_pre;
    hipEvent_t ready = nullptr, rows_home = nullptr;
    int64_t n = -1; uint64_t n_words = 0, n_name = 0, n_seq = 0; bool has_seq = false, staged = false, rows_pending = false;
    PinnedVec<uint4> h_a; PinnedVec<uint64_t> h_c, h_row_off; PinnedVec<uint32_t> h_pool; PinnedVec<uint4> h_x;
    PinnedVec<int32_t> h_mate, h_clip; PinnedVec<double> h_sim;
  };
  InSlot in_slot[2];
  hipStream_t run_stream = nullptr, d2h_stream = nullptr;
  hipEvent_t rows_busy = nullptr;   // recorded after the last packed download of the CURRENT row-table set was queued: the kernels that write the set wait for it
  bool rows_busy_set = false;
  // br_project_staged alternates between two sets of the tables a packed download reads (rows, detail, scores, dense CIGAR
  // references + pool, row_off): batch k's kernels write one set while batch k - 1's rows are still crossing PCIe out of the
  // other -- with one set the projection of batch k stood still behind the count pass until the wire was idle
  struct RowSetAlt { DevBuf pk_a, pk_x, pk_sim, pk_clip, pk_ch, pool, row_off; hipEvent_t busy = nullptr; bool busy_set = false; } alt;
  int host_detail = 0;              // br_host_rows carries the x (detail) array
  DevBuf z_slots, z_sizes, z_off, z_dense, z_dense_alt, z_tabs, z_tokens;
  DevBuf inf_out, inf_blocks, inf_tabs, inf_cnt; bool inf_tabs_ready = false;   // br_bgzf_inflate_device
  DevBuf sp_entry, sp_entry2, sp_exit, sp_nmap, sp_nunm, sp_ended, sp_redo, sp_pre, sp_small, sp_off, sp_len;   // br_bam_split_device
  // SAM text out (sam_writer.cpp): the reference names of RNAME / RNEXT, line lengths -> offsets, the long-record list, and two
  // text buffers that alternate like z_dense / z_dense_alt
  DevBuf sf_names, sf_name_off, sf_len, sf_long, sf_small, sf_tmp, sf_text[2];
  int32_t sf_n_names = 0;
  int sf_which = 0;
  int z_dense_which = 0;           // br_project_bam_staged_nowait: the packed blocks of call j are still on their way home while call j + 1 packs its own
  hipStream_t down_stream = nullptr; hipEvent_t ev_home[2] = {nullptr, nullptr}; std::atomic<bool> home_pending[2] = {{false}, {false}};
  int deflate_dynamic = 1;
  int deflate_waves = 0;     // "deflate_waves": a cap on k_deflate_dynamic's persistent waves (rounded up to 4), 0: as many as the chip holds; a test hook that makes one wave take many blocks
  int64_t speculate_n = 4194304;
  int speculate = 1;         // large batches are launched from the last call's counts, checked once at the end (run_device_small, big)
  int64_t hist_n = 0; uint64_t hist[4] = {0, 0, 0, 0}; bool hist_simf = false;   // the last call: alignments; matches, arena words, simple-class matches, records
  int small_batch = 1;       // batches of at most small_n alignments run without a host round trip before the final one (run_device_small)
  int64_t small_n = 65536;
  DevBuf walk_list, pmask, pbit, pick;
  // direct rows (run_device_direct): presets without the similarity filter and without -S pair on the count pass's survivor
  // sets before anything is emitted, and the emit kernels write the packed rows themselves
  int direct_rows = 1;       // "direct_rows" / BRAMBLE_AMD_DIRECT_ROWS=0: the match-table path (k_emit_dense -> k_pair -> k_rows), the A/B switch
  int pair_bitmask = 1;      // "pair_bitmask": k_pair_mask intersects mates' survivor sets as 64-bit tid masks where their tids span at most 64 (0: lists only, the A/B switch)
  int emit_rank_tids = 1;    // "emit_rank_tids": k_pair_mask leaves a pair's common tids as a word per alignment and the emit kernels rank by counting its bits (0: the rank loop only, the A/B switch)
  int emit_general_preset = 1;   // "emit_general_preset": the short-read preset emits its general class with k_emit_rows<2, 1> (preset as constants, typed LDS CIGAR scratch; 0: k_emit_rows<2, 0> as every other preset, the A/B switch)
  DevBuf d_fm, d_nkept, d_desc, d_hi0, d_clspos, d_rnd, d_side, d_sidectr, d_kt;
  uint64_t d_side_cap = 0;   // (br_ctx_set_param "side_cap": the first capacity, a test hook)
  int d_side_attempts = 0;   // side-arena attempts of the last direct-rows call (br_ctx_direct_diag)
  bool last_direct = false;  // the last call's rows came from the direct path: the detail column is re-emitted on request, not gathered
  bool want_x = false;       // the caller of run_device needs the detail column (input alignment, HI: the BAM encoder) with the rows
  ProjectArgs dA{}; DirectArgs dD{}; int64_t d_kept = 0, d_simple = 0;
  // packed row table (the product of the row stage) and what its kernels need
  DevBuf r_rec, pk_a, pk_c, pk_x, pk_sim, pk_clip;
  DevBuf pool, pool_sizes, pool_off, pk_ch;   // dense long-CIGAR pool + rewritten references for host downloads
  bool last_aux_cols = false;           // the last call's rows carry similarity / clip scores
  bool wide_valid = false;              // the wide view below matches the last call's rows
  bool detail_valid = false;            // pk_x (br_row_x) has been derived for the last call's rows
  const int32_t *last_l_qseq = nullptr; // the last batch's l_qseq (device; insert sizes of the wide view / the encoder)
  int32_t last_long_reads = 0;
  int64_t last_n_pool = 0;
  bool z_tabs_ready = false;
  DevBuf p_ncig, p_name_len, p_isnew, p_group_pre, p_small, p_big, p_seq_len, p_ref_map;
  uint8_t *h_bam[2] = {nullptr, nullptr}; size_t h_bam_cap[2] = {0, 0}; int h_bam_next = 0;  // pinned download buffers of br_project_bam_bundle (alternating)
  BigPinned h_bam_mem[2];
  int64_t last_n_rows = 0, last_n_aln = 0;
  br_device_bam last_bam{};   // the last bundle call's projected records in HBM, in every output mode (br_ctx_last_device_bam); a flat batch call has none
  // the last projection call's rows, read-name groups and stream, whichever entry point made it (br_quant_add_last); valid like the rows
  br_device_rows last_rows{}; const uint32_t *last_group_off = nullptr; int64_t last_n_groups = 0; hipStream_t last_stream = nullptr;
  // a projection call begins: what the call before it left is no longer the last call's.  Every entry point says so before it can
  // return, a call without alignments or records too: br_*_add_last after an empty bundle adds nothing, not the bundle before it again
  void forget_last_call(hipStream_t st) {
    last_rows = br_device_rows{}; last_group_off = nullptr; last_n_groups = 0; last_stream = st; last_bam = br_device_bam{};
  }
  DevBuf fa_stats, fa_n_prob, fa_seq_bytes, fa_prob_off, fa_seqarena_off, fa_probs, fa_results, fa_seq_arena, fa_clip_ops,
      fa_ideal_cap, fa_scratch, fa_srcs, fa_want, b_seq_off, b_seqs, b_seq_src;
  // the streamed -S DP (ksw_kernels.hip): per-bin descriptors, per-problem DP results, leftovers, counters, group
  // rows / offsets, the direction tape, raw traceback ops
  DevBuf ksw_desc, ksw_dp, ksw_left, ksw_cnt, ksw_group, ksw_tape, ksw_raw;
  int ksw_fast = 1;            // 0: every problem through the general kernel k_ksw
  // the side stream (ensure_side_stream) for kernels that run beside the main chain, a second one (ensure_side2_stream: the
  // name seeds of the direct path beside k_pair_mask), and the event pairs a SideWork in scope holds (side_live of them)
  hipStream_t side_stream = nullptr, side2_stream = nullptr;
  static constexpr int SIDE_EV = 8;
  hipEvent_t side_ev[SIDE_EV][2] = {}; int side_live = 0;
  uint32_t ksw_groups[KSW_N_BINS] = {0};
  int64_t ksw_tape_mb = 49152; // HBM set aside for the direction tape; larger batches go through in pieces
  int ksw_tape_pct = 100;      // test hook: the share of the computed tape the DP kernels may use (the rest of the problems goes to k_ksw)
  uint64_t ksw_diag[16] = {0};  // last call: pieces, problems per bin [4], leftovers before the DP, tape bytes (largest piece), spare, tape rows per bin [4]
  DevBuf n_rows, row_off, aln_group;
  // wide view of the rows (br_device_rows_expand): one array per field
  DevBuf r_input, r_nh, r_hi, r_mapq, r_group, r_mate_tid, r_mate_pos,
      r_isize, r_tid, r_pos, r_ncig, r_strand, r_sim, r_clip, r_junc, r_refc, r_cigoff, cigar_out;
  DevBuf r_paired, r_same, r_first, r_primary;
  DevBuf b_name_off, b_names;
  // device staging of host batches (br_project_batch)
  DevBuf b_ref_id, b_ref_start, b_flags, b_xs, b_ts, b_cigar_off, b_cigar, b_mate_idx, b_group_off, b_lqseq;
  ReadBack *rb = nullptr;        // pinned
  // host result storage (br_project_batch / br_project_group)
  // pinned: the row download runs at PCIe speed instead of through the pageable bounce path
  PinnedVec<int32_t> h_input, h_clip, h_junc, h_refc, h_mate_tid, h_mate_pos, h_isize;
  PinnedVec<uint32_t> h_tid, h_pos, h_nh, h_hi, h_mapq, h_group, h_cigar;
  PinnedVec<int8_t> h_strand;
  PinnedVec<uint64_t> h_cigoff;
  PinnedVec<double> h_sim;
  PinnedVec<uint8_t> h_primary, h_paired, h_same, h_first;
  std::vector<br_projected> h_proj;
  // br_project_group(s): one packed upload of the call's alignments, and the packed rows / their CIGAR words back
  PinnedVec<uint8_t> g_host; DevBuf g_dev;
  PinnedVec<uint4> g_a, g_x; PinnedVec<uint2> g_c; PinnedVec<uint32_t> g_pool, g_cig; PinnedVec<double> g_sim;
  bool rows_to_host = false, rows_at_host = false;   // br_project_group(s): the small path's row kernel writes g_a / g_c / g_x / g_sim (pinned host memory) itself
};

struct Prof {
  br_ctx *c; hipStream_t st;
  hipStream_t cur = nullptr;   // stream of the open begin / end pair
  int begin(int which, hipStream_t on = nullptr) {
    cur = on ? on : st;
    if (!c->profiling) return BR_OK;
    if (c->events_used == c->events.size()) {
      KEvent e; e.which = which;
      HIPCHK(hipEventCreate(&e.a)); HIPCHK(hipEventCreate(&e.b));
      c->events.push_back(e);
    }
    c->events[c->events_used].which = which;
    HIPCHK(hipEventRecord(c->events[c->events_used].a, cur));
    return BR_OK;
  }
  int end() {
    if (!c->profiling) return BR_OK;
    HIPCHK(hipEventRecord(c->events[c->events_used].b, cur));
    c->events_used++;
    return BR_OK;
  }
  int collect() {
    for (int k = 0; k < BR_K_NUM; k++) { c->k_ms[k] = 0; c->k_launches[k] = 0; }
    if (!c->profiling) return BR_OK;
    for (size_t i = 0; i < c->events_used; i++) {
      float ms = 0;
      // (the call has waited for its streams already: as a rule the events are complete and one query each is all it takes)
      if (hipEventElapsedTime(&ms, c->events[i].a, c->events[i].b) != hipSuccess) {
        (void)hipGetLastError();
        HIPCHK(hipEventSynchronize(c->events[i].b));
        HIPCHK(hipEventElapsedTime(&ms, c->events[i].a, c->events[i].b));
      }
      c->k_ms[c->events[i].which] += ms; c->k_launches[c->events[i].which]++;
      c->k_ms_sum[c->events[i].which] += ms; c->k_launches_sum[c->events[i].which]++;
    }
    c->events_used = 0;
    return BR_OK;
  }
};

// One piece of work on a side stream beside the main chain: fork (the side stream waits for what the main one has queued),
// the work, done (recorded behind it), join (the main stream waits for it).  Leaving the scope finishes what is open, so no
// return leaves side-stream kernels over the context's tables with nothing on the caller's stream ordered behind them.  A
// fork after a join starts over.  The events are the context's: a pair per SideWork in scope.
struct SideWork {
  br_ctx *c; hipStream_t main, side; hipEvent_t *ev;
  enum { IDLE, FORKED, DONE } state = IDLE;
  SideWork(br_ctx *c_, hipStream_t main_, hipStream_t side_) : c(c_), main(main_), side(side_), ev(c_->side_ev[c_->side_live++]) { assert(c->side_live <= br_ctx::SIDE_EV); }
  SideWork(const SideWork &) = delete;
  ~SideWork() { if (state == FORKED) (void)done(); if (state == DONE) (void)join(); c->side_live--; }
  int fork() { HIPCHK(hipEventRecord(ev[0], main)); HIPCHK(hipStreamWaitEvent(side, ev[0], 0)); state = FORKED; return BR_OK; }
  int done() { HIPCHK(hipEventRecord(ev[1], side)); state = DONE; return BR_OK; }
  int join() { return join_on(main); }
  int join_on(hipStream_t other) { state = IDLE; HIPCHK(hipStreamWaitEvent(other, ev[1], 0)); return BR_OK; }   // (another side stream takes the result)
  int wait_host() { state = IDLE; HIPCHK(hipEventSynchronize(ev[1])); return BR_OK; }   // (the host reallocates what the work reads)
};

// the device totals (kernels.h: TOT_*)
inline int ensure_totals(br_ctx *c) { return c->totals.ensure(TOT_N * 8); }

// the next run_device call should leave the detail column (input alignment, junc_hits, aligned_len, HI) next to the rows:
// the direct path then writes it in the emit pass instead of emitting a second time on request
struct WantDetail { br_ctx *c; bool old; WantDetail(br_ctx *c_, bool v) : c(c_), old(c_->want_x) { c->want_x = v; } ~WantDetail() { c->want_x = old; } };

// run_device_small / project_groups_lean: the call does not fit the short way; take the ordinary one
#define BR_RETRY_ORDINARY 1000

// one run of the -S rescue DP (run_ksw)
struct KswRun {
  int64_t n_prob; const KswProb *probs; KswRes *results; const uint8_t *seq_arena; uint32_t *clip_ops;
  uint64_t seq_total, qmax, tmax; uint64_t *stats;
  uint32_t *raw_out, *raw_n; int32_t *max_out; uint32_t raw_cap;
};

int check_device(int device);
int make_devcfg(const br_config *c, DevCfg &d);
int ensure_side_stream(br_ctx *c);
int run_ksw(br_ctx *c, hipStream_t st, const KswRun &R);
// keep_events: append to the running event list instead of restarting it
int run_device(br_ctx *c, const br_config *cfg, const br_device_batch *b, hipStream_t st, br_device_rows *out,
               bool keep_events = false);
int ensure_detail(br_ctx *c, hipStream_t st);
int expand_rows(br_ctx *c, hipStream_t st, br_device_wide_rows *out);
int sam_format_impl(br_ctx *c, const br_device_bam *in, hipStream_t st, const uint8_t **text, uint64_t *n_bytes);
// The unprojected records of a bundle call (unprojected.cpp), in three steps around the encoder's two waits: the kernels up to
// the scans and the copy of their totals into rb->unproj, queued in front of the wait for the encoder's size; the gather into
// the arena, queued beside the encoder once those totals are home; the bookkeeping behind the call's last synchronise.
int unproj_measure(br_ctx *c, hipStream_t st, Prof &pf, const BamArgs &B, const uint32_t *group_off, int64_t n_groups, UnprojArgs &U);
int unproj_gather(br_ctx *c, hipStream_t st, Prof &pf, UnprojArgs &U);
void unproj_commit(br_ctx *c, const UnprojArgs &U);
