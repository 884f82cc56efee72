// br_assign: the EM's posterior on every projected record of a run, and the record stream rewritten with it -- every record with
// ZW:f (mode tag), or one drawn placement per read name (mode sample) -- in one device's HBM (assign_kernels.hip; the definitions
// are in bramble_amd.h).
//
//   add      a note per record (the add-order name, the transcript, the FIRST / PAIRED bits) and, with records, their bytes
//            appended to the arena with one copy and the add-order offsets; the placements are checked here, so an add that is
//            refused has added nothing
//   finish   with the quantifier's tables (quant_view.h): p by the bounds-checked look-up, m, w per placement, the draw per
//            name (mode sample) or kept = 1, the kept records ranked by the shared scan; with records: the kept records' list
//            and the offsets of their rewritten forms, scanned
//   next     the cut at max_bytes (a search in the scanned offsets), then the kept records [cur, e) rewritten into one of two
//            alternating piece buffers: the rewritten stream never exists whole, so finish adds no second copy of the run
//
// Device memory (n records, R arena bytes = the sum of 4 + block_size, K kept records; every table has one entry more than its
// items): the adds hold R + 64 (the arena grows by half, the old one beside the new while copying) + 16 n (the notes) + 8 n (the
// offsets; not without records); a host add holds 16 bytes a row, 8 an alignment, 4 a name and 8 a record of the add while it
// runs.  finish adds 8 n (w) + n (kept) for good and, while it runs, 8 n (p) + 4 n (m) + 4 a 65 records (the long names) + 8 n
// (the ranks) + the scan's scratch; with records 4 K (the list) + 8 K (the rewritten offsets) stay.  next holds two piece buffers
// of the largest piece's bytes + 16 and 8 bytes a record of theirs.  128 bytes of counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "accum.h"
#include "assign_kernels.h"
#include "ctx.h"
#include "name_window.h"
#include "quant_kernels.h"
#include "quant_view.h"
#include "scan_kernels.h"

using namespace br;

struct br_assign : Accum {
  int mode = 0, long_reads = 0;
  uint64_t seed = 0, max_bytes = 0;   // max_bytes: 0: no cap on the arena but the device's memory
  int with_recs = -1;                 // -1: no add yet; 0: values only; 1: with records
  bool finished = false, dead = false;
  uint64_t n = 0, n_names = 0, used = 0;   // records, names, arena bytes of all adds
  uint64_t n_out = 0, n_named = 0, cur = 0;
  uint64_t counters[AS_WORDS] = {};
  double add_s = 0, finish_s = 0, next_s = 0;
  ColBuf small, arena, note, off, w, kept, sel, out_off;
  ColBuf buf[2], rows[2];
  int which = 0;
};

extern "C" void br_assign_free(br_assign *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_assign_new(int device, br_assign **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  br_assign *c = new br_assign();
  const int rc = c->open(device, c->small, AS_WORDS);
  if (rc) { br_assign_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_assign_set_param(br_assign *c, const char *name, int64_t value) {
  if (!c || !name || c->dead || c->finished || c->with_recs >= 0) return BR_ERR_INVALID_ARG;   // (before the first add)
  if (!strcmp(name, "mode")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->mode = (int)value; return BR_OK; }
  if (!strcmp(name, "seed")) { c->seed = (uint64_t)value; return BR_OK; }
  if (!strcmp(name, "long_reads")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->long_reads = (int)value; return BR_OK; }
  if (!strcmp(name, "max_bytes")) { if (value < 0) return BR_ERR_INVALID_ARG; c->max_bytes = (uint64_t)value; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

// room for m more records of `bytes` arena bytes
static int assign_reserve(br_assign *c, uint64_t m, uint64_t bytes, bool recs) {
  if (c->n + m >= (1ull << 32)) return BR_ERR_CAPACITY;   // (the list of the kept records is 32-bit)
  const size_t rn = (size_t)(c->n + m) + 1;
  if (rn * 16 > c->note.cap) RC(c->alloc(c->note, std::max(rn, (size_t)(c->note.cap / 16) * 3 / 2) * 16, true));
  if (!recs) return BR_OK;
  RC(c->grow_arena(c->arena, c->used, bytes, c->max_bytes));
  if (rn * 8 > c->off.cap) RC(c->alloc(c->off, std::max(rn, (size_t)(c->off.cap / 8) * 3 / 2) * 8, true));
  return BR_OK;
}

// the rows of the names A holds (a, a_bias, names and, with records, recs are set; data: the records' bytes from the first row's
// record on, `bytes` of them, in host or device memory).  Nothing is counted before the kernels have accepted the add
static int assign_add_rows(br_assign *c, AsAddArgs A, const uint8_t *data, uint64_t bytes, bool on_device) {
  hipStream_t st = c->st;
  const uint64_t m = A.names.r_last - A.names.r_first;
  const bool recs = A.recs.rec_off != nullptr;
  RC(assign_reserve(c, m, bytes, recs));
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + AS_BAD_NAMES, 0, 16, st)); HIPCHK(hipMemsetAsync(small + AS_BAD_OFF, 0, 8, st));
  A.name_base = c->n_names; A.arena_base = c->used;
  A.note = c->note.as<uint4>(); A.off = c->off.as<uint64_t>(); A.n0 = c->n; A.counters = c->small.as<unsigned long long>();
  if (recs && bytes) HIPCHK(hipMemcpyAsync(c->arena.as<uint8_t>() + c->used, data, (size_t)bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  launch_as_add(st, A);
  uint64_t seen[AS_WORDS];
  HIPCHK(hipMemcpyAsync(seen, small, sizeof(seen), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's tables may be reused now
  if (seen[AS_BAD_NAMES] || seen[AS_BAD_PLACE] || seen[AS_BAD_OFF]) return BR_ERR_INVALID_ARG;   // nothing was added
  c->n += m; c->used += recs ? bytes : 0;
  return BR_OK;
}

extern "C" int br_assign_add(br_assign *c, const br_device_bam *recs, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups,
                             int on_device, void *stream) {
  if (!c || !rows || n_groups < 0 || c->dead || c->finished || (n_groups && (!rows->row_off || !group_off))) return BR_ERR_INVALID_ARG;
  if (rows->n_rows < 0 || (c->with_recs >= 0 && c->with_recs != (recs ? 1 : 0))) return BR_ERR_INVALID_ARG;   // records on every add or on none
  if (recs && (recs->n_rows != rows->n_rows || (recs->n_rows && (!recs->data || !recs->row_off)))) return BR_ERR_INVALID_ARG;
  if (n_groups == 0) { c->with_recs = recs ? 1 : 0; return BR_OK; }
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  uint64_t span[2] = {0, 0};
  RC(names_span(c, rows->row_off, (uint64_t)rows->n_rows, group_off, n_groups, on_device != 0, (hipStream_t)stream, c->small.as<uint64_t>() + AS_CUT, span));
  if (span[1] > span[0] && !rows->a) return BR_ERR_INVALID_ARG;   // (the only table of the rows that is read)
  if (c->n_names + (uint64_t)n_groups >= (1ull << 32)) return BR_ERR_CAPACITY;
  if (span[1] > span[0]) {   // an empty span adds nothing; its names still count
    RowWindow w;
    ColBuf d_ro, d_go, d_rec;
    DropGuard dropper{c, {&w.a, &w.cigar, &w.pool, &d_ro, &d_go, &d_rec}};
    AsAddArgs A{};
    const uint8_t *data = nullptr; uint64_t bytes = 0;
    // the records are optional: without them recs.rec_off stays NULL (after whatever made them: the span's wait saw to it)
    if (recs) RC(record_window(c, *recs, span[0], span[1], on_device != 0, d_rec, &A.recs, &data, &bytes));
    if (on_device) { A.a = (const uint4 *)rows->a; A.names = device_names(rows->row_off, group_off, n_groups, span); }
    else {
      RC(c->upload_rows(*rows, span[0], span[1], false, w));
      RC(upload_names(c, rows->row_off, group_off, n_groups, span, d_ro, d_go, &A.names));
      A.a = w.a.as<uint4>(); A.a_bias = w.bias;
    }
    RC(assign_add_rows(c, A, data, bytes, on_device != 0));   // (it waits for the stream: the uploads are done when the host arrays go)
  }
  c->n_names += (uint64_t)n_groups;
  c->with_recs = recs ? 1 : 0;   // (an add that was refused decides nothing)
  return BR_OK;
}

extern "C" int br_assign_add_last(br_assign *c, br_ctx *ctx) {
  if (!c || !ctx || !ctx->ix || ctx->ix->device != c->device || c->dead || c->finished) return BR_ERR_INVALID_ARG;
  if (ctx->last_n_groups == 0) return BR_OK;   // a call without names
  br_device_bam recs; bool flat;
  last_call_records(ctx, &recs, &flat);
  // a flat batch call left rows and no records: only an object without records takes it (one without adds becomes that)
  if (flat && c->with_recs == 1) return BR_ERR_INVALID_ARG;
  return br_assign_add(c, flat || c->with_recs == 0 ? nullptr : &recs, &ctx->last_rows, ctx->last_group_off, ctx->last_n_groups, 1, ctx->last_stream);
}

static int assign_finish(br_assign *c, const QuantView &v) {
  hipStream_t st = c->st;
  const uint64_t n = c->n;
  const size_t n1 = (size_t)n + 1;
  ColBuf p, m, big, rank, tmp;
  DropGuard dropper{c, {&p, &m, &big, &rank, &tmp}};
  RC(c->alloc(c->w, n1 * 8)); RC(c->alloc(c->kept, n1));
  RC(c->alloc(p, n1 * 8)); RC(c->alloc(m, n1 * 4)); RC(c->alloc(big, (size_t)(n / (AS_M_LANE_MAX + 1) + 1) * 4));
  RC(c->alloc(rank, n1 * 8)); RC(c->alloc(tmp, scan_scratch_bytes((int64_t)n1)));
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + AS_BAD_NAME, 0, 6 * 8, st));   // AS_BAD_NAME .. AS_N_NAMED
  HIPCHK(hipMemsetAsync(c->kept.p, 0, n1, st));
  AsFinishArgs F{};
  F.note = c->note.as<uint4>(); F.n = n;
  F.name_cls = v.name_cls; F.n_names = (uint64_t)v.n_names;
  F.label_off = v.label_off; F.labels = v.labels; F.n_cls = (uint64_t)v.n_cls; F.n_lab = (uint64_t)v.n_lab; F.post = v.post;
  F.p = p.as<double>(); F.m = m.as<uint32_t>(); F.big = big.as<uint32_t>(); F.w = c->w.as<double>(); F.kept = c->kept.as<uint8_t>();
  F.rank = rank.as<uint64_t>();
  F.mode = c->mode; F.k0 = (uint32_t)c->seed; F.k1 = (uint32_t)(c->seed >> 32);
  F.counters = c->small.as<unsigned long long>();
  launch_as_finish(st, F);
  uint64_t K = 0;
  if (n) {
    launch_scan(st, rank.as<uint64_t>(), (int64_t)n, tmp.as<uint64_t>());
    HIPCHK(hipMemcpyAsync(&K, rank.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipMemcpyAsync(c->counters, small, AS_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // what names nothing of the quantifier's was counted by the look-up, never looked up
  if (c->counters[AS_BAD_NAME] || c->counters[AS_BAD_CLASS] || c->counters[AS_BAD_LABEL] || c->counters[AS_BAD_POST]) return BR_ERR_INVALID_ARG;
  if (K > n) return BR_ERR_HIP;
  c->n_out = K; c->n_named = c->counters[AS_N_NAMED];
  if (c->with_recs == 1 && K) {
    RC(c->alloc(c->sel, (size_t)(K + 1) * 4)); RC(c->alloc(c->out_off, (size_t)(K + 1) * 8));
    launch_as_select(st, c->kept.as<uint8_t>(), rank.as<uint64_t>(), c->off.as<uint64_t>(), n, c->sel.as<uint32_t>(), c->out_off.as<uint64_t>());
    launch_scan(st, c->out_off.as<uint64_t>(), (int64_t)K, tmp.as<uint64_t>());
    HIPCHK(hipStreamSynchronize(st));
  }
  return BR_OK;
}

extern "C" int br_assign_finish(br_assign *c, br_quant *q, int64_t *n_records_out, int64_t *n_names_with_records) {
  if (!c || !q || c->dead || c->finished) return BR_ERR_INVALID_ARG;
  QuantView v{};
  if (quant_view(q, &v) != BR_OK) return BR_ERR_INVALID_ARG;   // before br_quant_em, or without "keep_names"
  if (v.device != c->device || (uint64_t)v.n_names != c->n_names) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  const int rc = assign_finish(c, v);
  if (rc) { c->dead = true; return rc; }
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_records_out) *n_records_out = (int64_t)c->n_out;
  if (n_names_with_records) *n_names_with_records = (int64_t)c->n_named;
  return BR_OK;
}

extern "C" int br_assign_values(br_assign *c, int64_t first, int64_t n, double *w, float *zw, uint8_t *kept) {
  if (!c || c->dead || !c->finished || !in_range(c->n, first, n)) return BR_ERR_INVALID_ARG;
  if (n == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> tmp;
  double *wd = w;
  if (!wd && zw) { tmp.resize((size_t)n); wd = tmp.data(); }
  if (wd) HIPCHK(hipMemcpyAsync(wd, c->w.as<double>() + first, (size_t)n * 8, hipMemcpyDeviceToHost, c->st));
  if (kept) HIPCHK(hipMemcpyAsync(kept, c->kept.as<uint8_t>() + first, (size_t)n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (zw) for (int64_t i = 0; i < n; i++) zw[i] = (float)wd[i];   // (round to nearest even, as the write kernel's conversion)
  return BR_OK;
}

extern "C" int br_assign_next(br_assign *c, uint64_t max_bytes, br_device_bam *piece) {
  if (!c || !piece || c->dead || !c->finished || c->with_recs != 1) return BR_ERR_INVALID_ARG;
  memset(piece, 0, sizeof(*piece));
  if (c->cur >= c->n_out) return BR_OK;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  uint64_t *small = c->small.as<uint64_t>();
  launch_as_cut(st, c->out_off.as<uint64_t>(), c->n_out, c->cur, max_bytes, small + AS_CUT);
  uint64_t cut[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(cut, small + AS_CUT, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t e = cut[0];
  if (e <= c->cur || e > c->n_out) return BR_ERR_HIP;
  const int wh = c->which; c->which ^= 1;
  RC(c->alloc(c->buf[wh], (size_t)cut[1] + 16)); RC(c->alloc(c->rows[wh], (size_t)(e - c->cur + 1) * 8));
  AsWriteArgs W{};
  W.arena = c->arena.as<uint8_t>(); W.off = c->off.as<uint64_t>(); W.sel = c->sel.as<uint32_t>(); W.out_off = c->out_off.as<uint64_t>();
  W.w = c->w.as<double>(); W.cur = c->cur; W.e = e; W.dst = c->buf[wh].as<uint8_t>(); W.row_off = c->rows[wh].as<uint64_t>();
  W.mode = c->mode; W.mapq = br_row_mapq(1, c->long_reads); W.counters = c->small.as<unsigned long long>();
  launch_as_write(st, W);
  uint64_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, small + AS_BAD_REC, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad) { c->dead = true; return BR_ERR_INVALID_ARG; }   // a kept record that is no record of the encoder's
  piece->data = c->buf[wh].as<uint8_t>(); piece->n_bytes = cut[1]; piece->row_off = c->rows[wh].as<uint64_t>(); piece->n_rows = (int64_t)(e - c->cur);
  c->cur = e;
  c->next_s += timer.seconds();
  return BR_OK;
}

extern "C" int br_assign_stats(const br_assign *c, uint64_t *held, uint64_t *peak, double *add_s, double *finish_s, double *next_s, uint64_t *bad) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (held) *held = c->live;
  if (peak) *peak = c->peak;
  if (add_s) *add_s = c->add_s;
  if (finish_s) *finish_s = c->finish_s;
  if (next_s) *next_s = c->next_s;
  if (bad) { bad[0] = c->counters[AS_BAD_NAME]; bad[1] = c->counters[AS_BAD_CLASS]; bad[2] = c->counters[AS_BAD_LABEL]; bad[3] = c->counters[AS_BAD_POST]; }
  return BR_OK;
}
