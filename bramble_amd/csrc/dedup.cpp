// br_dedup: UMI-aware duplicate removal by read name over a whole run, in one device's HBM (dedup_kernels.hip; the definitions are in
// bramble_amd.h).
//
//   add      per row its entry (t, five, f) from the rewritten CIGAR and the record's flag word; per name the UMI of its first
//            record, its entries in order in the entry arena and their hash; with "keep_records" the records' bytes appended to the
//            arena with one copy and their offsets.  The offsets and the pooled CIGARs are checked here, so an add that is refused
//            has added nothing
//   finish   the names with rows sorted by (hash & mask), cut into position groups by comparing the signatures themselves and, where
//            unlike ones share a key, put in order and cut again (the quantifier's kernels: a signature is a list of words to them);
//            within the groups a stable sort by (length, UMI) gives the nodes and their counts, a stable sort of the nodes by count
//            the node order; the edges of every group by all pairs of its nodes, tile by tile, counted, scanned and stored; labels
//            swept to their fixed point, at most (largest group's nodes) sweeps; the molecules' sizes, the histogram and per name
//            rep, dup, group_first.  With records: the list of the records handed out and their scanned lengths
//   next     the cut at max_bytes (a search in the scanned lengths), then the records [cur, e) gathered into one of two alternating
//            piece buffers
//
// Device memory (N names, R rows, D nodes, E edges, B record bytes; every table has one entry more than its items): the adds hold
// 53 N (UMI 32, length 1, arena offset 8, signature length 4, hash 8) + 16 R (the entries) and, while one runs, 16 a row of the add
// (the entries in row order) + 4 a name of the add (the list of long names); a host add also its tables (16 + 8 bytes a row, the
// pool, 8 an alignment, 4 a name, 8 a record and the records' bytes).  With "keep_records" B + 64 (the arena grows by half, the old
// one beside the new while copying) + 8 R.  finish keeps 9 N (rep, group_first, dup) + 8 (hist_max + 1) and, with records, 1 R
// (the record's verdict) + 12 a record handed out; while it runs 4 N (the name's group) + 32 a name with rows (two key / index pairs,
// the heads) + the sorts' histograms and scratch, then 105 D (UMI 32, length 1, count, first name, group and place 4 each, two
// labels 8, the edge offsets 8, cursor 4, molecule size 4, the nodes' begins 8, two key / index pairs 24) + 24 a group + 4 E.  next holds two piece buffers of the largest piece's bytes
// + 16 and 8 bytes a record of theirs.  128 bytes of counters.
// With a br_whitelist set (br_dedup_set_whitelist, "cell_source" != 0) finish first resolves the cell barcodes in place against it
// (whitelist.h): 1 N of status and the resolve's own tables, all gone before the groups are made.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "accum.h"
#include "assign_kernels.h"
#include "barcode_sort.h"
#include "ctx.h"
#include "dedup_kernels.h"
#include "name_window.h"
#include "quant_kernels.h"
#include "scan_kernels.h"
#include "whitelist.h"

using namespace br;

struct br_dedup : Accum {
  int method = 1, umi_source = 0, cell_source = 0, keep_records = 0, mark = 0, hash_bits = 64;
  uint32_t umi_sep = '_', umi_tag = 'R' | 'X' << 8, cell_tag = 'C' | 'B' << 8, hist_max = 1000;
  uint64_t max_bytes = 0;   // 0: no cap on the arena but the device's memory
  bool added = false, finished = false, dead = false;
  uint64_t n = 0, rows = 0, used = 0;   // names, rows, arena bytes of all adds
  uint64_t n_with_rows = 0, n_no_umi = 0, n_too_long = 0, n_bad_aux = 0;
  uint64_t n_groups = 0, n_nodes = 0, n_edges = 0, sweeps = 0, max_nodes = 0, collisions = 0, n_mols = 0;
  uint64_t n_out = 0, cur = 0;
  double add_s = 0, finish_s = 0;
  const br_whitelist *wl = nullptr;   // set: finish resolves the cell barcodes against it first ("correct": wl_correct)
  int wl_correct = 1;
  WlResolved wl_res;
  ColBuf status;
  ColBuf small, umi, ulen, cb, cblen, noff, nk, hash, ent, arena, rec_at;
  ColBuf rep, gfirst, dup, hist, rdup, sel, out_off;
  ColBuf buf[2], prow[2];
  int which = 0;
};

extern "C" void br_dedup_free(br_dedup *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_dedup_new(int device, br_dedup **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  br_dedup *c = new br_dedup();
  const int rc = c->open(device, c->small, DD_WORDS);
  if (rc) { br_dedup_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_dedup_set_param(br_dedup *c, const char *name, int64_t value) {
  if (!c || !name || c->dead || c->finished) return BR_ERR_INVALID_ARG;
  if (!strcmp(name, "hash_bits")) { if (value < 1 || value > 64) return BR_ERR_INVALID_ARG; c->hash_bits = (int)value; return BR_OK; }
  if (c->added) return BR_ERR_INVALID_ARG;   // (the others before the first add)
  const bool flag = value == 0 || value == 1;
  if (!strcmp(name, "method")) { if (!flag) return BR_ERR_INVALID_ARG; c->method = (int)value; return BR_OK; }
  if (!strcmp(name, "umi_source")) { if (!flag) return BR_ERR_INVALID_ARG; c->umi_source = (int)value; return BR_OK; }
  if (!strcmp(name, "umi_sep")) { if (value < 0 || value > 255) return BR_ERR_INVALID_ARG; c->umi_sep = (uint32_t)value; return BR_OK; }
  if (!strcmp(name, "cell_source")) { if (value < 0 || value > 2) return BR_ERR_INVALID_ARG; c->cell_source = (int)value; return BR_OK; }
  if (!strcmp(name, "cell_tag")) { if (value < 0 || value > 65535) return BR_ERR_INVALID_ARG; c->cell_tag = (uint32_t)value; return BR_OK; }
  if (!strcmp(name, "umi_tag")) { if (value < 0 || value > 65535) return BR_ERR_INVALID_ARG; c->umi_tag = (uint32_t)value; return BR_OK; }
  if (!strcmp(name, "keep_records")) { if (!flag) return BR_ERR_INVALID_ARG; c->keep_records = (int)value; return BR_OK; }
  if (!strcmp(name, "mark")) { if (!flag) return BR_ERR_INVALID_ARG; c->mark = (int)value; return BR_OK; }
  if (!strcmp(name, "max_bytes")) { if (value < 0) return BR_ERR_INVALID_ARG; c->max_bytes = (uint64_t)value; return BR_OK; }
  if (!strcmp(name, "hist_max")) { if (value < 1 || value > 65535) return BR_ERR_INVALID_ARG; c->hist_max = (uint32_t)value; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

// b holds `items` + 1 items of `each` bytes, with what it held; it grows by half
static int dedup_grow(br_dedup *c, ColBuf &b, uint64_t items, size_t each) {
  const size_t want = (size_t)(items + 1) * each;
  if (want <= b.cap) return BR_OK;
  return c->alloc(b, std::max(want, b.cap + b.cap / 2), true);
}

// room for ng more names of m rows and `bytes` record bytes
static int dedup_reserve(br_dedup *c, uint64_t ng, uint64_t m, uint64_t bytes) {
  if (c->n + ng >= (1ull << 32) || c->rows + m >= (1ull << 32)) return BR_ERR_CAPACITY;
  const uint64_t N = c->n + ng, R = c->rows + m;
  RC(dedup_grow(c, c->umi, N, 32)); RC(dedup_grow(c, c->ulen, N, 1)); RC(dedup_grow(c, c->noff, N, 8)); RC(dedup_grow(c, c->nk, N, 4));
  RC(dedup_grow(c, c->hash, N, 8)); RC(dedup_grow(c, c->ent, R, 16));
  if (c->cell_source) { RC(dedup_grow(c, c->cb, N, 32)); RC(dedup_grow(c, c->cblen, N, 1)); }
  if (!c->keep_records) return BR_OK;
  RC(c->grow_arena(c->arena, c->used, bytes, c->max_bytes));
  return dedup_grow(c, c->rec_at, R, 8);
}

// the names of one add, their tables on the device (A: the rows' tables, a_bias, names and recs but for recs.data are set).  data: the
// records' bytes from the first row's record on, `bytes` of them, in host or device memory.  Nothing is counted before the kernels
// have accepted the add
static int dedup_add_names(br_dedup *c, DdAddArgs A, const uint8_t *data, uint64_t bytes, bool on_device) {
  hipStream_t st = c->st;
  const uint64_t ng = (uint64_t)A.names.n_groups, m = A.names.r_last - A.names.r_first;
  RC(dedup_reserve(c, ng, m, bytes));
  ColBuf raw, big, window;
  DropGuard dropper{c, {&raw, &big, &window}};
  RC(c->alloc(raw, (size_t)(m + 1) * 16)); RC(c->alloc(big, (size_t)(ng + 1) * 4));
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + DD_BAD, 0, 5 * 8, st));   // DD_BAD .. DD_BAD_AUX
  if (c->keep_records) {   // one copy into the arena; the kernels read the records where they stay
    if (bytes) HIPCHK(hipMemcpyAsync(c->arena.as<uint8_t>() + c->used, data, (size_t)bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    A.recs.data = c->arena.as<uint8_t>() + c->used;
    A.rec_at = c->rec_at.as<uint64_t>() + c->rows; A.arena_base = c->used;
  } else if (on_device) A.recs.data = data;
  else {
    RC(c->alloc(window, (size_t)bytes + ARENA_SLACK));
    if (bytes) HIPCHK(hipMemcpyAsync(window.p, data, (size_t)bytes, hipMemcpyHostToDevice, st));
    A.recs.data = window.as<uint8_t>();
  }
  A.umi_source = c->umi_source; A.umi_sep = c->umi_sep; A.umi_tag = c->umi_tag;
  A.cell_source = c->cell_source; A.cell_tag = c->cell_tag;
  if (c->cell_source) { A.cb = c->cb.as<uint64_t>() + 4 * c->n; A.cblen = c->cblen.as<uint8_t>() + c->n; }
  A.raw = raw.as<uint4>(); A.ent = c->ent.as<uint32_t>(); A.row_base = c->rows;
  A.noff = c->noff.as<uint64_t>() + c->n; A.nk = c->nk.as<uint32_t>() + c->n; A.hash = c->hash.as<uint64_t>() + c->n;
  A.umi = c->umi.as<uint64_t>() + 4 * c->n; A.ulen = c->ulen.as<uint8_t>() + c->n;
  A.big = big.as<uint32_t>(); A.counters = c->small.as<unsigned long long>();
  launch_dd_add(st, A);
  uint64_t seen[5];
  HIPCHK(hipMemcpyAsync(seen, small + DD_BAD, sizeof(seen), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's tables may be reused now
  if (seen[DD_BAD]) return BR_ERR_INVALID_ARG;   // nothing was added
  c->n += ng; c->rows += m; c->used += c->keep_records ? bytes : 0;
  c->n_no_umi += seen[DD_NO_UMI]; c->n_too_long += seen[DD_TOO_LONG]; c->n_bad_aux += seen[DD_BAD_AUX];
  return BR_OK;
}

static int dedup_add_host(br_dedup *c, const br_device_bam &recs, const br_device_rows &rows, const uint32_t *group_off, int64_t ng, const uint64_t span[2]) {
  RowWindow w;
  ColBuf d_ro, d_go, d_rec;
  DropGuard dropper{c, {&w.a, &w.cigar, &w.pool, &d_ro, &d_go, &d_rec}};
  DdAddArgs A{};
  const uint8_t *data; uint64_t bytes;
  RC(record_window(c, recs, span[0], span[1], false, d_rec, &A.recs, &data, &bytes));
  RC(c->upload_rows(rows, span[0], span[1], true, w));
  RC(upload_names(c, rows.row_off, group_off, ng, span, d_ro, d_go, &A.names));
  A.a = w.a.as<uint4>(); A.cigar = w.cigar.as<uint64_t>(); A.a_bias = w.bias; A.pool = w.pool.as<uint32_t>(); A.n_pool_words = w.n_pool_words;
  return dedup_add_names(c, A, data, bytes, false);   // (it waits for the stream: the uploads are done when the host arrays go)
}

static int dedup_add_device(br_dedup *c, const br_device_bam &recs, const br_device_rows &rows, const uint32_t *group_off, int64_t ng, const uint64_t span[2]) {
  ColBuf none;
  DdAddArgs A{};
  const uint8_t *data; uint64_t bytes;
  RC(record_window(c, recs, span[0], span[1], true, none, &A.recs, &data, &bytes));
  A.names = device_names(rows.row_off, group_off, ng, span);
  A.a = (const uint4 *)rows.a; A.cigar = rows.cigar; A.pool = rows.pool; A.n_pool_words = (uint64_t)rows.n_pool_words;
  return dedup_add_names(c, A, data, bytes, true);
}

extern "C" int br_dedup_add(br_dedup *c, const br_device_bam *recs, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups,
                            int on_device, void *stream) {
  if (!c || !recs || !rows || n_groups < 0 || c->dead || c->finished || (n_groups && (!rows->row_off || !group_off))) return BR_ERR_INVALID_ARG;
  if (rows->n_rows < 0 || rows->n_pool_words < 0 || (rows->n_pool_words && !rows->pool) || recs->n_rows != rows->n_rows) return BR_ERR_INVALID_ARG;
  if (recs->n_rows && (!recs->data || !recs->row_off || !rows->a || !rows->cigar)) return BR_ERR_INVALID_ARG;
  if (n_groups == 0) { c->added = true; return BR_OK; }
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  uint64_t span[2] = {0, 0};
  RC(names_span(c, rows->row_off, (uint64_t)rows->n_rows, group_off, n_groups, on_device != 0, (hipStream_t)stream, c->small.as<uint64_t>() + DD_SPAN, span));
  RC(on_device ? dedup_add_device(c, *recs, *rows, group_off, n_groups, span) : dedup_add_host(c, *recs, *rows, group_off, n_groups, span));
  c->added = true;   // (an add that was refused decides nothing)
  return BR_OK;
}

extern "C" int br_dedup_add_last(br_dedup *c, br_ctx *ctx) {
  if (!c || !ctx || !ctx->ix || ctx->ix->device != c->device || c->dead || c->finished) return BR_ERR_INVALID_ARG;
  if (ctx->last_n_groups == 0) return BR_OK;   // a call without names
  br_device_bam recs; bool flat;
  last_call_records(ctx, &recs, &flat);
  if (flat) return BR_ERR_INVALID_ARG;   // a flat batch call left no records
  return br_dedup_add(c, &recs, &ctx->last_rows, ctx->last_group_off, ctx->last_n_groups, 1, ctx->last_stream);
}

static int dedup_finish(br_dedup *c) {
  hipStream_t st = c->st;
  const int64_t N = (int64_t)c->n;
  uint64_t *small = c->small.as<uint64_t>();
  const size_t n1 = (size_t)N + 1;
  RC(c->alloc(c->rep, n1 * 4)); RC(c->alloc(c->gfirst, n1 * 4)); RC(c->alloc(c->dup, n1)); RC(c->alloc(c->hist, (size_t)(c->hist_max + 1) * 8));
  HIPCHK(hipMemsetAsync(c->rep.p, 0xff, n1 * 4, st)); HIPCHK(hipMemsetAsync(c->gfirst.p, 0xff, n1 * 4, st));
  HIPCHK(hipMemsetAsync(c->dup.p, 0, n1, st)); HIPCHK(hipMemsetAsync(c->hist.p, 0, (size_t)(c->hist_max + 1) * 8, st));
  HIPCHK(hipMemsetAsync(small + DD_COLL, 0, (DD_WORDS - DD_COLL) * 8, st));
  HIPCHK(hipStreamSynchronize(st));
  if (N == 0) return BR_OK;
  ColBuf tmp, name_gid, head, mark, gbeg;
  SortBufs s;
  DropGuard bufs{c, {&tmp, &name_gid, &head, &mark, &gbeg, &s.key[0], &s.key[1], &s.idx[0], &s.idx[1]}};
  // the names with rows
  uint64_t M = 0;
  {
    ColBuf pos;
    DropGuard dropper{c, {&pos}};
    RC(c->alloc(pos, n1 * 8));
    launch_q_flag(st, c->nk.as<uint32_t>(), N, pos.as<uint64_t>());
    RC(c->scan_total(pos, N, tmp, &M));
    c->n_with_rows = M;
    if (M == 0) return BR_OK;
    RC(s.make(c, (size_t)M));
    const uint64_t mask = c->hash_bits >= 64 ? ~0ull : (1ull << c->hash_bits) - 1;
    launch_q_compact(st, c->nk.as<uint32_t>(), c->hash.as<uint64_t>(), pos.as<uint64_t>(), N, mask, s.key[0].as<uint64_t>(), s.idx[0].as<uint32_t>());
    HIPCHK(hipStreamSynchronize(st));
  }
  const int64_t n = (int64_t)M;
  RC(sort_pairs(c, s, n, tmp, small + DD_BITS));
  // position groups: the heads compare the signatures; a run of equal keys that holds different ones is put in order and cut again
  const uint32_t *ent = c->ent.as<uint32_t>();
  const uint64_t *noff = c->noff.as<uint64_t>();
  const uint32_t *nk = c->nk.as<uint32_t>();
  RC(c->alloc(head, (size_t)(n + 1) * 8));
  auto heads = [&](uint32_t *mk, uint64_t *n_coll) -> int {
    HIPCHK(hipMemsetAsync(small + DD_COLL, 0, 8, st));
    launch_q_heads(st, ent, noff, nk, s.key[0].as<uint64_t>(), s.idx[0].as<uint32_t>(), n, head.as<uint64_t>(), (unsigned long long *)(small + DD_COLL), mk);
    HIPCHK(hipMemcpyAsync(n_coll, small + DD_COLL, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return BR_OK;
  };
  uint64_t n_coll = 0;
  RC(heads(nullptr, &n_coll));
  c->collisions = n_coll;
  if (n_coll) {
    RC(c->alloc(mark, (size_t)n * 4));
    HIPCHK(hipMemsetAsync(mark.p, 0, (size_t)n * 4, st));
    RC(heads(mark.as<uint32_t>(), &n_coll));
    launch_q_resolve(st, ent, noff, nk, s.key[0].as<uint64_t>(), s.idx[0].as<uint32_t>(), n, mark.as<uint32_t>(), s.key[1].as<uint64_t>(), s.idx[1].as<uint32_t>());
    std::swap(s.key[0], s.key[1]); std::swap(s.idx[0], s.idx[1]);
    RC(heads(nullptr, &n_coll));
  }
  uint64_t G = 0;
  RC(c->scan_total(head, n, tmp, &G));   // head -> group ids (exclusive), head[n] = G
  if (G == 0 || G > M) return BR_ERR_HIP;
  c->n_groups = G;
  RC(c->alloc(gbeg, (size_t)(G + 1) * 8)); RC(c->alloc(name_gid, n1 * 4));
  launch_col_gbeg(st, head.as<uint64_t>(), n, gbeg.as<uint64_t>());
  launch_dd_groups(st, head.as<uint64_t>(), gbeg.as<uint64_t>(), s.idx[0].as<uint32_t>(), n, c->gfirst.as<uint32_t>(), name_gid.as<uint32_t>());
  const uint64_t *umi = c->umi.as<uint64_t>();
  const uint8_t *ulen = c->ulen.as<uint8_t>();
  // the field sorts below are by (group, length, bytes), every sort stable, so equal items' names ascend
  if (c->cell_source) {   // per cell: a group of equal signatures is cut where the barcode changes, by the barcodes themselves
    RC(sort_by_barcode(c, s, c->cb.as<uint64_t>(), c->cblen.as<uint8_t>(), name_gid.as<uint32_t>(), n, tmp, small + DD_BITS));
    // (names without a barcode share the empty one: an empty field is no head of its own)
    launch_bc_heads(st, s.idx[0].as<uint32_t>(), c->cb.as<uint64_t>(), c->cblen.as<uint8_t>(), name_gid.as<uint32_t>(), 0, n, head.as<uint64_t>());
    RC(c->scan_total(head, n, tmp, &G));
    if (G < c->n_groups || G > M) return BR_ERR_HIP;
    c->n_groups = G;
    RC(c->alloc(gbeg, (size_t)(G + 1) * 8));
    launch_col_gbeg(st, head.as<uint64_t>(), n, gbeg.as<uint64_t>());
    launch_dd_groups(st, head.as<uint64_t>(), gbeg.as<uint64_t>(), s.idx[0].as<uint32_t>(), n, c->gfirst.as<uint32_t>(), name_gid.as<uint32_t>());
  }
  // within the groups by (length, UMI), so the names of a node ascend
  RC(sort_by_barcode(c, s, umi, ulen, name_gid.as<uint32_t>(), n, tmp, small + DD_BITS));
  // nodes: a name without a UMI is a node of its own
  launch_bc_heads(st, s.idx[0].as<uint32_t>(), umi, ulen, name_gid.as<uint32_t>(), 1, n, head.as<uint64_t>());
  uint64_t D = 0;
  RC(c->scan_total(head, n, tmp, &D));
  if (D < G || D > M) return BR_ERR_HIP;
  c->n_nodes = D;
  const size_t d1 = (size_t)D + 1;
  ColBuf nbeg, o_umi, o_len, o_cnt, o_first, o_gid, inv, gn0, work, eoff, cursor, esrc, label[2], msize;
  SortBufs ns;
  DropGuard node_bufs{c, {&nbeg, &o_umi, &o_len, &o_cnt, &o_first, &o_gid, &inv, &gn0, &work, &eoff, &cursor, &esrc, &label[0], &label[1], &msize,
                          &ns.key[0], &ns.key[1], &ns.idx[0], &ns.idx[1]}};
  RC(c->alloc(nbeg, d1 * 8));
  launch_col_gbeg(st, head.as<uint64_t>(), n, nbeg.as<uint64_t>());
  RC(ns.make(c, (size_t)D));
  launch_dd_node_key(st, nbeg.as<uint64_t>(), s.idx[0].as<uint32_t>(), name_gid.as<uint32_t>(), (int64_t)D, ns.key[0].as<uint64_t>(), ns.idx[0].as<uint32_t>());
  RC(sort_pairs(c, ns, (int64_t)D, tmp, small + DD_BITS));
  RC(c->alloc(o_umi, d1 * 32)); RC(c->alloc(o_len, d1)); RC(c->alloc(o_cnt, d1 * 4)); RC(c->alloc(o_first, d1 * 4)); RC(c->alloc(o_gid, d1 * 4));
  RC(c->alloc(inv, d1 * 4)); RC(c->alloc(gn0, (size_t)(G + 1) * 8)); RC(c->alloc(work, (size_t)(G + 1) * 8));
  RC(c->alloc(eoff, d1 * 8)); RC(c->alloc(cursor, d1 * 4)); RC(c->alloc(label[0], d1 * 4)); RC(c->alloc(label[1], d1 * 4)); RC(c->alloc(msize, d1 * 4));
  HIPCHK(hipMemsetAsync(eoff.p, 0, d1 * 8, st)); HIPCHK(hipMemsetAsync(cursor.p, 0, d1 * 4, st)); HIPCHK(hipMemsetAsync(msize.p, 0, d1 * 4, st));
  DdNodes Nd{};
  Nd.n_nodes = (int64_t)D; Nd.n_groups = (int64_t)G;
  Nd.umi = o_umi.as<uint64_t>(); Nd.len = o_len.as<uint8_t>(); Nd.cnt = o_cnt.as<uint32_t>(); Nd.first = o_first.as<uint32_t>(); Nd.gid = o_gid.as<uint32_t>();
  Nd.inv = inv.as<uint32_t>(); Nd.gn0 = gn0.as<uint64_t>(); Nd.work = work.as<uint64_t>(); Nd.indeg = eoff.as<uint64_t>(); Nd.cursor = cursor.as<uint32_t>();
  Nd.label[0] = label[0].as<uint32_t>(); Nd.label[1] = label[1].as<uint32_t>(); Nd.msize = msize.as<uint32_t>();
  Nd.counters = c->small.as<unsigned long long>();
  launch_dd_nodes(st, Nd, ns.idx[0].as<uint32_t>(), nbeg.as<uint64_t>(), s.idx[0].as<uint32_t>(), umi, ulen, name_gid.as<uint32_t>());
  RC(c->alloc(tmp, scan_tmp_bytes((int64_t)std::max(G, D))));
  launch_scan(st, work.as<uint64_t>(), (int64_t)G, tmp.as<uint64_t>());
  uint64_t got[2] = {0, 0};   // the tile pairs, the largest group's nodes: the scan's total and a counter come back in one wait
  HIPCHK(hipMemcpyAsync(&got[0], work.as<uint64_t>() + G, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&got[1], small + DD_MAXM, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->max_nodes = got[1];
  if (got[1] == 0 || got[1] > D) return BR_ERR_HIP;
  launch_dd_label_init(st, Nd.label[0], (int64_t)D);
  int lab = 0;
  if (c->method == 1 && got[0]) {
    launch_dd_edges(st, Nd, nullptr, got[0], false);
    uint64_t E = 0;
    RC(c->scan_total(eoff, (int64_t)D, tmp, &E));
    c->n_edges = E;
    if (E) {
      RC(c->alloc(esrc, (size_t)(E + 1) * 4));
      Nd.esrc = esrc.as<uint32_t>();
      launch_dd_edges(st, Nd, eoff.as<uint64_t>(), got[0], true);
      // labels to their fixed point: a label travels one edge a sweep, so the largest group's node count bounds the sweeps
      uint64_t changed = 1;
      for (uint64_t sweep = 0; sweep < c->max_nodes && changed; sweep++) {
        HIPCHK(hipMemsetAsync(small + DD_CHANGED, 0, 8, st));
        launch_dd_sweep(st, Nd, eoff.as<uint64_t>(), Nd.label[lab], Nd.label[lab ^ 1]);
        HIPCHK(hipMemcpyAsync(&changed, small + DD_CHANGED, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        lab ^= 1;
        c->sweeps++;
      }
      if (changed) return BR_ERR_HIP;   // (no fixed point within the bound: a kernel's fault, never the input's)
    }
  }
  launch_dd_molecules(st, Nd, Nd.label[lab], c->hist.as<uint64_t>(), c->hist_max);
  launch_dd_verdict(st, Nd, Nd.label[lab], head.as<uint64_t>(), s.idx[0].as<uint32_t>(), n, c->rep.as<uint32_t>(), c->dup.as<uint8_t>());
  HIPCHK(hipMemcpyAsync(&c->n_mols, small + DD_MOLS, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->n_mols == 0 || c->n_mols > D) return BR_ERR_HIP;
  return BR_OK;
}

// the records that will be handed out: their list and scanned lengths
static int dedup_records(br_dedup *c) {
  if (!c->keep_records || !c->rows) return BR_OK;
  hipStream_t st = c->st;
  const uint64_t R = c->rows;
  ColBuf rank, tmp;
  DropGuard dropper{c, {&rank, &tmp}};
  RC(c->alloc(c->rdup, (size_t)R + 1)); RC(c->alloc(rank, (size_t)(R + 1) * 8)); RC(c->alloc(tmp, scan_scratch_bytes((int64_t)R + 1)));
  launch_dd_keep(st, c->noff.as<uint64_t>(), (int64_t)c->n, c->dup.as<uint8_t>(), R, c->mark, rank.as<uint64_t>(), c->rdup.as<uint8_t>());
  launch_scan(st, rank.as<uint64_t>(), (int64_t)R, tmp.as<uint64_t>());   // (not scan_total: the scratch here is the scan's own, smaller size)
  uint64_t K = 0;
  HIPCHK(hipMemcpyAsync(&K, rank.as<uint64_t>() + R, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (K > R) return BR_ERR_HIP;
  c->n_out = K;
  if (!K) return BR_OK;
  RC(c->alloc(c->sel, (size_t)(K + 1) * 4)); RC(c->alloc(c->out_off, (size_t)(K + 1) * 8));
  launch_dd_select(st, rank.as<uint64_t>(), c->rec_at.as<uint64_t>(), R, c->sel.as<uint32_t>(), c->out_off.as<uint64_t>());
  launch_scan(st, c->out_off.as<uint64_t>(), (int64_t)K, tmp.as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

extern "C" int br_dedup_finish(br_dedup *c, int64_t *n_names, int64_t *n_molecules, int64_t *n_duplicates) {
  if (!c || c->dead || c->finished) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  int rc = BR_OK;
  if (c->wl) {   // the observed cell barcodes become whitelist entries, or the empty barcode
    rc = c->alloc(c->status, (size_t)c->n + 1);
    if (!rc) rc = wl_resolve(c, c->wl, c->wl_correct, c->cb.as<uint64_t>(), c->cblen.as<uint8_t>(), (int64_t)c->n, c->status.as<uint8_t>(), nullptr, &c->wl_res);
    c->drop(c->status);
  }
  if (!rc) rc = dedup_finish(c);
  if (!rc) rc = dedup_records(c);
  if (rc) { c->dead = true; return rc; }
  c->drop(c->ent); c->drop(c->hash); c->drop(c->nk); c->drop(c->noff);   // the names are molecules now
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_names) *n_names = (int64_t)c->n;
  if (n_molecules) *n_molecules = (int64_t)c->n_mols;
  if (n_duplicates) *n_duplicates = (int64_t)(c->n_with_rows - c->n_mols);
  return BR_OK;
}

extern "C" int br_dedup_set_whitelist(br_dedup *c, const br_whitelist *wl, int correct) {
  if (!c || !wl || c->dead || c->finished || !c->cell_source || correct < 0 || correct > 2 || wl_device(wl) != c->device) return BR_ERR_INVALID_ARG;
  c->wl = wl; c->wl_correct = correct;
  return BR_OK;
}

extern "C" int br_dedup_whitelist_stats(const br_dedup *c, uint64_t out[8]) {
  return c && c->wl ? wl_stats(c->wl_res, c->wl_correct, out) : BR_ERR_INVALID_ARG;
}

extern "C" int br_dedup_umis(br_dedup *c, int64_t first, int64_t n, uint8_t *umi, uint8_t *len) {
  if (!c || c->dead || !in_range(c->n, first, n)) return BR_ERR_INVALID_ARG;
  return c->fetch_fields(c->umi, c->ulen, first, n, umi, len);
}

extern "C" int br_dedup_result(br_dedup *c, int64_t first, int64_t n, uint32_t *rep, uint32_t *group_first, uint8_t *dup) {
  if (!c || c->dead || !c->finished || !in_range(c->n, first, n)) return BR_ERR_INVALID_ARG;
  if (n == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  if (rep) HIPCHK(hipMemcpyAsync(rep, c->rep.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (group_first) HIPCHK(hipMemcpyAsync(group_first, c->gfirst.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (dup) HIPCHK(hipMemcpyAsync(dup, c->dup.as<uint8_t>() + first, (size_t)n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_dedup_hist(br_dedup *c, uint64_t *hist) {
  if (!c || c->dead || !c->finished) return BR_ERR_INVALID_ARG;
  if (!hist) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(hist, c->hist.p, (size_t)(c->hist_max + 1) * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_dedup_flags(br_dedup *c, const uint8_t **dup_device, int64_t *n) {
  if (!c || c->dead || !c->finished) return BR_ERR_INVALID_ARG;
  if (dup_device) *dup_device = c->dup.as<uint8_t>();
  if (n) *n = (int64_t)c->n;
  return BR_OK;
}

extern "C" int br_dedup_next(br_dedup *c, uint64_t max_bytes, br_device_bam *piece) {
  if (!c || !piece || c->dead || !c->finished || !c->keep_records) return BR_ERR_INVALID_ARG;
  memset(piece, 0, sizeof(*piece));
  if (c->cur >= c->n_out) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  uint64_t *small = c->small.as<uint64_t>();
  launch_as_cut(st, c->out_off.as<uint64_t>(), c->n_out, c->cur, max_bytes, small + DD_CUT);
  uint64_t cut[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(cut, small + DD_CUT, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t e = cut[0];
  if (e <= c->cur || e > c->n_out) return BR_ERR_HIP;
  const int wh = c->which; c->which ^= 1;
  RC(c->alloc(c->buf[wh], (size_t)cut[1] + 16)); RC(c->alloc(c->prow[wh], (size_t)(e - c->cur + 1) * 8));
  launch_dd_write(st, c->arena.as<uint8_t>(), c->rec_at.as<uint64_t>(), c->sel.as<uint32_t>(), c->out_off.as<uint64_t>(), c->rdup.as<uint8_t>(), c->cur, e,
                  c->buf[wh].as<uint8_t>(), c->prow[wh].as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  piece->data = c->buf[wh].as<uint8_t>(); piece->n_bytes = cut[1]; piece->row_off = c->prow[wh].as<uint64_t>(); piece->n_rows = (int64_t)(e - c->cur);
  c->cur = e;
  return BR_OK;
}

extern "C" int br_dedup_stats(const br_dedup *c, uint64_t out[16]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  const uint64_t v[16] = {c->n, c->n_with_rows, c->n_no_umi, c->n_too_long, c->n_bad_aux, c->n_groups, c->n_nodes, c->n_edges, c->sweeps, c->max_nodes,
                          c->collisions, c->live, c->peak, (uint64_t)(c->add_s * 1e6), (uint64_t)(c->finish_s * 1e6), c->n_out};
  memcpy(out, v, sizeof(v));
  return BR_OK;
}
