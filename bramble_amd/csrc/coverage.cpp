// br_coverage: the depth of coverage along every transcript, from the rows of a whole run, in one device's HBM
// (coverage_kernels.hip; the definitions are in bramble_amd.h).
//
//   new      off[t] = the bases of the transcripts in front of t (a scan on the host: T numbers); diff, B + 1 words, and the
//            per-transcript record counts, zeroed
//   add      a lane per row: the row's covered intervals, clamped to the transcript, leave + 1 / - 1 in diff (integer atomics)
//   finish   diff -> depth by an in-place inclusive scan modulo 2^32; sum, non-zero count and maximum per transcript; run heads
//            counted per tile of 4096 bases, the counts scanned, the runs written
//
// Device memory (B bases, T transcripts, R runs; to the byte, every table has one entry more than its items):
//   from new on    4 (B + 1) (diff, then the depth) + 16 (T + 1) (offsets, records) + 64 bytes of counters
//   a host add     adds 24 a row of the add and 4 a pool word while it runs (24 and 4 more for the entry behind them)
//   finish         adds 8 a tile of 4096 bases (the tile sums, then the tile counts; freed again), 20 (T + 1) (the summary) and
//                  16 (R + 1)
//
// The weighted modes ("weight" = 1: 1 / NH, 2: the EM's posteriors; bramble_amd.h) keep the pipeline and change the word: a depth is
// 64 bits, one unit 2^32, and a row leaves + q / - q.  Weight nh knows q at the add.  Weight em does not: its add keeps, per
// clamped non-empty interval, 16 bytes (first base, length, name) in an arena -- a pass that counts a row's entries, room made on
// the host, a pass that writes them -- and br_coverage_finish_em applies them with the quantifier's posteriors (quant_view.h)
// before the scan.  The kernels are the same ones in every mode: the add is instantiated per way of ending an interval (the unit
// mode's instance holds nothing of the others: no q, no names, no entries), the scan, the summary, the run count and the run writer
// per depth word, and coverage_finish below is one routine for both words.
//
// Device memory in a weighted mode (E kept entries: the intervals, and one for every counted row without one):
//   from "weight" on  8 (B + 1) (diff, then the depth) + 24 (T + 1) (offsets, records, weight_sum) + 128 bytes of counters (what
//                     new made is freed first: the peak keeps its 4 (B + 1))
//   a host add        as above; weight em adds 8 an alignment and 4 a name of the add (the offsets, one entry more each)
//   weight em, add    adds 4 (rows of the add + 1) while it runs (the rows' entry counts) and holds the arena, 16 bytes an entry: an
//                     add that needs more room makes max(E + 1, 3/2 of the old room) entries, the old arena beside the new while
//                     copying; add_names of device tables holds 16 bytes for the span of its rows
//   finish            finish_em frees the arena after the apply; then 8 a tile of 4096 bases (freed again), 32 (T + 1) (the summary:
//                     aligned_hi, aligned_lo, covered, max_depth) and 24 (R + 1) (16 for transcript, start, end; 8 for the depth)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "accum.h"
#include "coverage_kernels.h"
#include "coverage_view.h"
#include "ctx.h"
#include "name_window.h"
#include "quant_kernels.h"
#include "quant_view.h"
#include "scan_kernels.h"

using namespace br;

struct br_coverage : Accum {
  int64_t n_tx = 0;
  std::vector<uint64_t> off;   // n_tx + 1
  int64_t n_bases = 0;
  int primary_only = 0;
  bool added = false, finished = false, broken = false;   // broken: an add met a table it could not trust
  uint64_t rows = 0;           // rows of all adds, counted or skipped
  int64_t n_runs = 0;
  uint64_t counters[CV_WORDS_W] = {};
  double add_s = 0, finish_s = 0;
  ColBuf d_off, diff, records, small, aligned, covered, max_depth, runs;
  // the weighted modes: 0 unit, 1 nh, 2 em
  int weight = 0;
  int64_t n_names = 0;         // names of all add_names (weight em)
  uint64_t kept = 0;           // entries in the arena
  ColBuf weight_sum, aligned_lo, run_depth, arena;
  BigwigState *bigwig = nullptr;   // br_coverage_bigwig's image (bigwig.cpp), through coverage_view
  size_t counter_words() const { return weight ? (size_t)CV_WORDS_W : (size_t)CV_WORDS; }
};

// the hook of bigwig.cpp (coverage_view.h): what a finished object holds
int br::coverage_view(br_coverage *c, CoverageView *v) {
  if (!c || c->broken || !c->finished) return BR_ERR_INVALID_ARG;
  *v = CoverageView{c, c->weight, c->n_tx, c->n_runs, &c->off, c->d_off.as<uint64_t>(), c->diff.p, c->runs.as<uint4>(),
                    c->weight ? c->run_depth.as<uint64_t>() : nullptr, &c->bigwig};
  return BR_OK;
}

extern "C" void br_coverage_free(br_coverage *c) {
  if (!c) return;
  bigwig_state_free(c, c->bigwig);
  c->close();
  delete c;
}

extern "C" int br_coverage_new(int device, int64_t n_transcripts, const int64_t *lengths, br_coverage **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  if (n_transcripts < 0 || n_transcripts >= (1ll << 32) || (n_transcripts && !lengths)) return BR_ERR_INVALID_ARG;
  for (int64_t t = 0; t < n_transcripts; t++) if (lengths[t] > 0xffffffffll) return BR_ERR_INVALID_ARG;   // (start and end are 32-bit)
  br_coverage *c = new br_coverage();
  c->n_tx = n_transcripts;
  c->off.assign((size_t)n_transcripts + 1, 0);
  for (int64_t t = 0; t < n_transcripts; t++) c->off[(size_t)t + 1] = c->off[(size_t)t] + (uint64_t)std::max<int64_t>(lengths[t], 0);
  c->n_bases = (int64_t)c->off[(size_t)n_transcripts];
  const size_t t1 = (size_t)n_transcripts + 1, b1 = (size_t)c->n_bases + 1;
  int rc = c->open(device);
  if (!rc) rc = c->alloc(c->small, CV_WORDS * 8);
  if (!rc) rc = c->alloc(c->d_off, t1 * 8);
  if (!rc) rc = c->alloc(c->records, t1 * 8);
  if (!rc) rc = c->alloc(c->diff, b1 * 4);
  if (!rc && (hipMemsetAsync(c->small.p, 0, CV_WORDS * 8, c->st) != hipSuccess || hipMemsetAsync(c->records.p, 0, t1 * 8, c->st) != hipSuccess ||
              hipMemsetAsync(c->diff.p, 0, b1 * 4, c->st) != hipSuccess ||
              hipMemcpyAsync(c->d_off.p, c->off.data(), t1 * 8, hipMemcpyHostToDevice, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess))
    rc = BR_ERR_HIP;
  if (rc) { br_coverage_free(c); return rc; }
  *out = c;
  return BR_OK;
}

// diff, the counters and weight_sum for the mode: what the object held of them goes first
static int coverage_set_weight(br_coverage *c, int weight) {
  if (weight == c->weight) return BR_OK;
  if (weight == 2 && (uint64_t)c->n_bases >= COV_KEEP_MAX_BASES) return BR_ERR_CAPACITY;   // (a kept entry holds 40 bits of it)
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  HIPCHK(hipStreamSynchronize(st));
  c->drop(c->diff); c->drop(c->small); c->drop(c->weight_sum);
  c->weight = weight;
  c->broken = true;   // until the tables are there
  const size_t t1 = (size_t)c->n_tx + 1, b1 = (size_t)c->n_bases + 1, word = weight ? 8 : 4;
  RC(c->alloc(c->small, c->counter_words() * 8)); RC(c->alloc(c->diff, b1 * word));
  if (weight) RC(c->alloc(c->weight_sum, t1 * 8));
  HIPCHK(hipMemsetAsync(c->small.p, 0, c->counter_words() * 8, st)); HIPCHK(hipMemsetAsync(c->diff.p, 0, b1 * word, st));
  if (weight) HIPCHK(hipMemsetAsync(c->weight_sum.p, 0, t1 * 8, st));
  HIPCHK(hipStreamSynchronize(st));
  c->broken = false;
  return BR_OK;
}

extern "C" int br_coverage_set_param(br_coverage *c, const char *name, int64_t value) {
  if (!c || !name || c->broken || c->finished || c->added) return BR_ERR_INVALID_ARG;   // (what the adds counted depends on it)
  if (!strcmp(name, "primary_only")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->primary_only = (int)value; return BR_OK; }
  if (!strcmp(name, "weight")) { if (value < 0 || value > 2) return BR_ERR_INVALID_ARG; return coverage_set_weight(c, (int)value); }
  return BR_ERR_INVALID_ARG;
}

// the rows [r0, r1) through the kernel; A: a, cigar, bias, pool and n_pool_words are set
static int coverage_add_rows(br_coverage *c, CovAddArgs A, uint64_t r0, uint64_t r1) {
  hipStream_t st = c->st;
  A.r_first = r0; A.r_last = r1;
  A.n_tx = c->n_tx; A.off = c->d_off.as<uint64_t>(); A.primary_only = (uint32_t)c->primary_only;
  A.records = c->records.as<unsigned long long>(); A.counters = c->small.as<unsigned long long>();
  A.diff = c->diff.p;
  CovAddWArgs W{};
  W.A = A; W.weight_sum = c->weight_sum.as<unsigned long long>();   // (weight nh: the row's q into 64-bit words, and into weight_sum)
  launch_cov_add(st, W, c->weight ? COV_ADD_NH : COV_ADD_UNIT);
  HIPCHK(hipMemcpyAsync(c->counters, c->small.p, c->counter_words() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's rows may be reused now
  c->rows += r1 - r0;
  if (c->counters[CV_BAD_POOL]) { c->broken = true; return BR_ERR_INVALID_ARG; }   // a CIGAR reference that leaves the pool
  return BR_OK;
}

// weight em: the rows of the names W holds (a, cigar, bias, pool, n_pool_words and names are set) into the
// arena.  The first pass counts and changes nothing else, so an add it refuses has added nothing
static int coverage_keep_rows(br_coverage *c, CovAddWArgs W) {
  hipStream_t st = c->st;
  CovAddArgs &A = W.A;
  const uint64_t r0 = W.names.r_first, r1 = W.names.r_last;
  A.r_first = r0; A.r_last = r1;
  A.n_tx = c->n_tx; A.off = c->d_off.as<uint64_t>(); A.primary_only = (uint32_t)c->primary_only;
  A.records = c->records.as<unsigned long long>(); A.counters = c->small.as<unsigned long long>();
  W.name_base = (uint64_t)c->n_names;
  ColBuf entries;
  DropGuard dropper{c, {&entries}};
  RC(c->alloc(entries, (size_t)(r1 - r0 + 1) * 4));
  W.row_entries = entries.as<uint32_t>();
  HIPCHK(hipMemsetAsync(c->small.as<uint64_t>() + CV_ADD_ENTRIES, 0, 8, st));
  launch_cov_add(st, W, COV_ADD_COUNT);
  uint64_t seen[CV_WORDS_W];
  HIPCHK(hipMemcpyAsync(seen, c->small.p, sizeof(seen), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (seen[CV_BAD_POOL]) { c->broken = true; return BR_ERR_INVALID_ARG; }
  if (seen[CV_BAD_NAMES]) {   // offsets that descend somewhere: nothing was added
    HIPCHK(hipMemsetAsync(c->small.as<uint64_t>() + CV_BAD_NAMES, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    return BR_ERR_INVALID_ARG;
  }
  const size_t need = (size_t)(c->kept + seen[CV_ADD_ENTRIES]) + 1;
  if (need * 16 > c->arena.cap) RC(c->alloc(c->arena, std::max(need, (size_t)(c->arena.cap / 16) * 3 / 2) * 16, true));
  W.arena = c->arena.as<uint4>(); W.arena_cap = c->arena.cap / 16;
  launch_cov_add(st, W, COV_ADD_KEEP);
  HIPCHK(hipMemcpyAsync(c->counters, c->small.p, CV_WORDS_W * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's rows may be reused now
  if (c->counters[CV_KEPT] != c->kept + seen[CV_ADD_ENTRIES]) { c->broken = true; return BR_ERR_HIP; }   // (the two passes disagree)
  c->kept = c->counters[CV_KEPT];
  c->rows += r1 - r0; c->n_names += W.names.n_groups;
  return BR_OK;
}

static int coverage_add_host(br_coverage *c, const br_device_rows &rows, uint64_t r0, uint64_t r1) {
  RowWindow w;
  DropGuard dropper{c, {&w.a, &w.cigar, &w.pool}};
  RC(c->upload_rows(rows, r0, r1, true, w));
  CovAddArgs A{};
  A.a = w.a.as<uint4>(); A.cigar = w.cigar.as<uint64_t>(); A.bias = w.bias; A.pool = w.pool.as<uint32_t>(); A.n_pool_words = w.n_pool_words;
  return coverage_add_rows(c, A, r0, r1);   // (it waits for the stream: the uploads are done when the host arrays go)
}

static int coverage_add_device(br_coverage *c, const br_device_rows &rows, uint64_t r0, uint64_t r1, hipStream_t caller) {
  RC(c->after(caller));   // after whatever made the rows
  CovAddArgs A{};
  A.a = (const uint4 *)rows.a; A.cigar = rows.cigar; A.pool = rows.pool; A.n_pool_words = (uint64_t)rows.n_pool_words;
  return coverage_add_rows(c, A, r0, r1);
}

extern "C" int br_coverage_add_rows(br_coverage *c, const br_device_rows *rows, int64_t r0, int64_t r1, int on_device, void *stream) {
  if (!c || !rows || c->broken || c->finished || c->weight == 2) return BR_ERR_INVALID_ARG;   // (weight em: br_coverage_add_names)
  if (r0 < 0 || r1 < r0 || rows->n_rows < 0 || r1 > rows->n_rows || rows->n_pool_words < 0) { c->broken = true; return BR_ERR_INVALID_ARG; }
  if (r1 > r0 && (!rows->a || !rows->cigar || (rows->n_pool_words && !rows->pool))) return BR_ERR_INVALID_ARG;
  if (c->rows + (uint64_t)(r1 - r0) >= (1ull << 32)) return BR_ERR_CAPACITY;   // (the depth is 32-bit)
  c->added = true;
  if (r1 == r0) return BR_OK;
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  return on_device ? coverage_add_device(c, *rows, (uint64_t)r0, (uint64_t)r1, (hipStream_t)stream) : coverage_add_host(c, *rows, (uint64_t)r0, (uint64_t)r1);
}

extern "C" int br_coverage_add_names(br_coverage *c, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups, int on_device,
                                     void *stream) {
  if (!c || !rows || n_groups < 0 || c->broken || c->finished || (n_groups && (!rows->row_off || !group_off))) return BR_ERR_INVALID_ARG;
  if (rows->n_rows < 0 || rows->n_pool_words < 0) return BR_ERR_INVALID_ARG;
  if (n_groups == 0) { c->added = true; return BR_OK; }
  HIPCHK(hipSetDevice(c->device));
  uint64_t span[2] = {0, 0};
  {   // the object has no slot for the span of device tables: two words of the call's.  (None of these refusals sets `broken`:
      // nothing was read that an add could have counted)
    ColBuf d_span;
    DropGuard dropper{c, {&d_span}};
    if (on_device) RC(c->alloc(d_span, 16));
    RC(names_span(c, rows->row_off, (uint64_t)rows->n_rows, group_off, n_groups, on_device != 0, (hipStream_t)stream, d_span.as<uint64_t>(), span));
  }
  if (c->weight != 2) return br_coverage_add_rows(c, rows, (int64_t)span[0], (int64_t)span[1], on_device, stream);
  if (span[1] > span[0] && (!rows->a || !rows->cigar || (rows->n_pool_words && !rows->pool))) return BR_ERR_INVALID_ARG;
  if (c->rows + (span[1] - span[0]) >= (1ull << 32) || (uint64_t)c->n_names + (uint64_t)n_groups >= (1ull << 32)) return BR_ERR_CAPACITY;
  c->added = true;
  ScopeTimer timer(&c->add_s);
  if (span[1] == span[0]) { c->n_names += n_groups; return BR_OK; }   // names without rows
  RowWindow w;   // host tables: the rows' window and the names'
  ColBuf d_ro, d_go;
  DropGuard dropper{c, {&w.a, &w.cigar, &w.pool, &d_ro, &d_go}};
  CovAddWArgs W{};
  if (on_device) {   // (after whatever made the rows: the span's wait saw to it)
    W.A.a = (const uint4 *)rows->a; W.A.cigar = rows->cigar; W.A.pool = rows->pool; W.A.n_pool_words = (uint64_t)rows->n_pool_words;
    W.names = device_names(rows->row_off, group_off, n_groups, span);
  } else {
    RC(c->upload_rows(*rows, span[0], span[1], true, w));
    RC(upload_names(c, rows->row_off, group_off, n_groups, span, d_ro, d_go, &W.names));
    W.A.a = w.a.as<uint4>(); W.A.cigar = w.cigar.as<uint64_t>(); W.A.bias = w.bias; W.A.pool = w.pool.as<uint32_t>(); W.A.n_pool_words = w.n_pool_words;
  }
  return coverage_keep_rows(c, W);
}

extern "C" int br_coverage_add_last(br_coverage *c, br_ctx *ctx) {
  if (!c || !ctx || !ctx->ix || ctx->ix->device != c->device || c->broken || c->finished) return BR_ERR_INVALID_ARG;
  if (c->weight == 2) {
    if (ctx->last_n_groups == 0) { c->added = true; return BR_OK; }   // a call without names
    return br_coverage_add_names(c, &ctx->last_rows, ctx->last_group_off, ctx->last_n_groups, 1, ctx->last_stream);
  }
  if (!ctx->last_rows.row_off || ctx->last_rows.n_rows == 0) { c->added = true; return BR_OK; }   // a call without rows
  return br_coverage_add_rows(c, &ctx->last_rows, 0, ctx->last_rows.n_rows, 1, ctx->last_stream);
}

// diff (it holds every row's events by now) -> depth, summary and runs, over the mode's depth word
template <typename W>
static int coverage_finish(br_coverage *c) {
  constexpr bool wide = sizeof(W) == 8;
  hipStream_t st = c->st;
  const int64_t B = c->n_bases, T = c->n_tx;
  const size_t t1 = (size_t)T + 1;
  const int64_t tiles = (B + COV_TILE - 1) / COV_TILE;
  ColBuf tile, tmp;
  DropGuard dropper{c, {&tile, &tmp}};
  RC(c->alloc(c->aligned, t1 * 8));
  if (wide) RC(c->alloc(c->aligned_lo, t1 * 8));
  RC(c->alloc(c->covered, t1 * 8)); RC(c->alloc(c->max_depth, t1 * sizeof(W)));
  RC(c->alloc(tile, (size_t)(tiles + 2) * 8)); RC(c->alloc(tmp, scan_scratch_bytes(tiles)));
  HIPCHK(hipMemsetAsync(c->aligned.p, 0, t1 * 8, st));
  if (wide) HIPCHK(hipMemsetAsync(c->aligned_lo.p, 0, t1 * 8, st));
  HIPCHK(hipMemsetAsync(c->covered.p, 0, t1 * 8, st)); HIPCHK(hipMemsetAsync(c->max_depth.p, 0, t1 * sizeof(W), st));
  W *depth = c->diff.as<W>();
  const uint64_t *off = c->d_off.as<uint64_t>();
  launch_cov_scan(st, depth, B, tile.as<uint64_t>(), tmp.as<uint64_t>());
  if (B > 0) launch_cov_summary(st, (const W *)depth, off, T, c->aligned.as<uint64_t>(), c->aligned_lo.as<uint64_t>(), c->covered.as<uint64_t>(), c->max_depth.as<W>());
  uint64_t R = 0;
  if (B > 0) {
    launch_cov_count(st, (const W *)depth, B, off, T, tile.as<uint64_t>());
    launch_scan(st, tile.as<uint64_t>(), tiles, tmp.as<uint64_t>());   // tile counts -> the first run of every tile; [tiles] = R
    HIPCHK(hipMemcpyAsync(&R, tile.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (R > (uint64_t)B) return BR_ERR_HIP;
  RC(c->alloc(c->runs, (size_t)(R + 1) * 16));
  if (wide) RC(c->alloc(c->run_depth, (size_t)(R + 1) * 8));
  if (R) launch_cov_runs(st, (const W *)depth, B, off, T, tile.as<uint64_t>(), c->runs.as<uint4>(), c->run_depth.as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  c->n_runs = (int64_t)R;
  return BR_OK;
}

// weight em: the kept entries into diff, by the quantifier's posteriors
static int coverage_apply(br_coverage *c, const QuantView &v) {
  hipStream_t st = c->st;
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + CV_BAD_NAME, 0, 4 * 8, st));   // CV_BAD_NAME .. CV_BAD_ENTRY
  CovApplyArgs P{};
  P.arena = c->arena.as<uint4>(); P.n = c->kept;
  P.off = c->d_off.as<uint64_t>(); P.n_tx = c->n_tx; P.n_bases = (uint64_t)c->n_bases;
  P.name_cls = v.name_cls; P.n_names = (uint64_t)v.n_names;
  P.label_off = v.label_off; P.labels = v.labels; P.n_cls = (uint64_t)v.n_cls; P.n_lab = (uint64_t)v.n_lab; P.post = v.post;
  P.diff = c->diff.as<unsigned long long>(); P.weight_sum = c->weight_sum.as<unsigned long long>(); P.counters = c->small.as<unsigned long long>();
  launch_cov_apply(st, P);
  HIPCHK(hipMemcpyAsync(c->counters, c->small.p, CV_WORDS_W * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->drop(c->arena);
  return BR_OK;
}

extern "C" int br_coverage_finish_em(br_coverage *c, br_quant *q, int64_t *n_runs) {
  if (!c || !q || c->broken || c->finished || c->weight != 2) return BR_ERR_INVALID_ARG;
  if (c->counters[CV_BAD_TID]) return BR_ERR_INVALID_ARG;
  QuantView v{};
  if (quant_view(q, &v) != BR_OK) return BR_ERR_INVALID_ARG;   // before br_quant_em, or without "keep_names"
  if (v.device != c->device || v.n_names != c->n_names) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  int rc = coverage_apply(c, v);
  // an entry that names nothing of the quantifier's: counted by the apply, never looked up
  if (!rc && (c->counters[CV_BAD_NAME] || c->counters[CV_BAD_CLASS] || c->counters[CV_BAD_LABEL] || c->counters[CV_BAD_ENTRY])) rc = BR_ERR_INVALID_ARG;
  if (!rc) rc = coverage_finish<uint64_t>(c);
  if (rc) { c->broken = true; return rc; }   // (diff holds part of the events, or half a depth)
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_runs) *n_runs = c->n_runs;
  return BR_OK;
}

extern "C" int br_coverage_finish(br_coverage *c, int64_t *n_runs) {
  if (!c || c->broken || c->finished || c->weight == 2) return BR_ERR_INVALID_ARG;   // (weight em: br_coverage_finish_em)
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  // a transcript id the object has no transcript for, or (weight nh) a row without a weight: nh == 0
  if (c->counters[CV_BAD_TID] || (c->weight == 1 && c->counters[CV_BAD_NH])) return BR_ERR_INVALID_ARG;
  const int rc = c->weight ? coverage_finish<uint64_t>(c) : coverage_finish<uint32_t>(c);
  if (rc) { c->broken = true; return rc; }   // (diff may be half a depth by now)
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_runs) *n_runs = c->n_runs;
  return BR_OK;
}

extern "C" int br_coverage_runs(br_coverage *c, int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
  if (!c || c->broken || !c->finished || c->weight || first < 0 || n < 0 || first > c->n_runs || n > c->n_runs - first) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  constexpr int64_t PAGE = 1 << 20;
  std::vector<uint32_t> page((size_t)std::min(n, PAGE) * 4);
  for (int64_t done = 0; done < n; done += PAGE) {
    const int64_t m = std::min(PAGE, n - done);
    HIPCHK(hipMemcpyAsync(page.data(), c->runs.as<uint4>() + first + done, (size_t)m * 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int64_t k = 0; k < m; k++) {
      const uint32_t *r = page.data() + 4 * k;
      if (tid) tid[done + k] = r[0];
      if (start) start[done + k] = r[1];
      if (end) end[done + k] = r[2];
      if (depth) depth[done + k] = r[3];
    }
  }
  return BR_OK;
}

extern "C" int br_coverage_depth(br_coverage *c, int64_t tid, uint32_t *depth) {
  if (!c || c->broken || !c->finished || c->weight || tid < 0 || tid >= c->n_tx) return BR_ERR_INVALID_ARG;
  const uint64_t b = c->off[(size_t)tid], len = c->off[(size_t)tid + 1] - b;
  if (!depth || !len) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(depth, c->diff.as<uint32_t>() + b, (size_t)len * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_coverage_summary(br_coverage *c, uint64_t *records, uint64_t *aligned_bases, uint64_t *covered_bases, uint32_t *max_depth) {
  if (!c || c->broken || !c->finished || c->weight) return BR_ERR_INVALID_ARG;
  const size_t T = (size_t)c->n_tx;
  if (!T) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  if (records) HIPCHK(hipMemcpyAsync(records, c->records.p, T * 8, hipMemcpyDeviceToHost, st));
  if (aligned_bases) HIPCHK(hipMemcpyAsync(aligned_bases, c->aligned.p, T * 8, hipMemcpyDeviceToHost, st));
  if (covered_bases) HIPCHK(hipMemcpyAsync(covered_bases, c->covered.p, T * 8, hipMemcpyDeviceToHost, st));
  if (max_depth) HIPCHK(hipMemcpyAsync(max_depth, c->max_depth.p, T * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

// ---- the getters of the weighted modes ---------------------------------------------------------------------------------------------
extern "C" int br_coverage_runs64(br_coverage *c, int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint64_t *depth) {
  if (!c || c->broken || !c->finished || !c->weight || first < 0 || n < 0 || first > c->n_runs || n > c->n_runs - first) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (depth && n) HIPCHK(hipMemcpyAsync(depth, c->run_depth.as<uint64_t>() + first, (size_t)n * 8, hipMemcpyDeviceToHost, c->st));
  constexpr int64_t PAGE = 1 << 20;
  std::vector<uint32_t> page((size_t)std::min(n, PAGE) * 4);
  for (int64_t done = 0; done < n; done += PAGE) {
    const int64_t m = std::min(PAGE, n - done);
    HIPCHK(hipMemcpyAsync(page.data(), c->runs.as<uint4>() + first + done, (size_t)m * 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int64_t k = 0; k < m; k++) {
      const uint32_t *r = page.data() + 4 * k;
      if (tid) tid[done + k] = r[0];
      if (start) start[done + k] = r[1];
      if (end) end[done + k] = r[2];
    }
  }
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_coverage_depth64(br_coverage *c, int64_t tid, uint64_t *depth) {
  if (!c || c->broken || !c->finished || !c->weight || tid < 0 || tid >= c->n_tx) return BR_ERR_INVALID_ARG;
  const uint64_t b = c->off[(size_t)tid], len = c->off[(size_t)tid + 1] - b;
  if (!depth || !len) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(depth, c->diff.as<uint64_t>() + b, (size_t)len * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_coverage_summary64(br_coverage *c, uint64_t *records, uint64_t *weight_sum, uint64_t *aligned_hi, uint64_t *aligned_lo,
                                     uint64_t *covered_bases, uint64_t *max_depth) {
  if (!c || c->broken || !c->finished || !c->weight) return BR_ERR_INVALID_ARG;
  const size_t T = (size_t)c->n_tx;
  if (!T) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const struct { uint64_t *to; const ColBuf *from; } cols[] = {{records, &c->records}, {weight_sum, &c->weight_sum}, {aligned_hi, &c->aligned},
                                                               {aligned_lo, &c->aligned_lo}, {covered_bases, &c->covered}, {max_depth, &c->max_depth}};
  for (const auto &col : cols) if (col.to) HIPCHK(hipMemcpyAsync(col.to, col.from->p, T * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

extern "C" int br_coverage_stats(const br_coverage *c, uint64_t *rows_counted, uint64_t *rows_skipped, uint64_t *clipped_bases,
                                 uint64_t *held_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds) {
  if (!c || c->broken) return BR_ERR_INVALID_ARG;
  if (rows_counted) *rows_counted = c->counters[CV_COUNTED];
  if (rows_skipped) *rows_skipped = c->counters[CV_SKIPPED];
  if (clipped_bases) *clipped_bases = c->counters[CV_CLIPPED];
  if (held_bytes) *held_bytes = c->live;
  if (peak_bytes) *peak_bytes = c->peak;
  if (add_seconds) *add_seconds = c->add_s;
  if (finish_seconds) *finish_seconds = c->finish_s;
  return BR_OK;
}
