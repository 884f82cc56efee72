// br_cells: cell x feature count matrices over a whole run, in one device's HBM (cells_kernels.hip; the definitions are in
// bramble_amd.h).
//
//   add      per name the cell barcode of its first record (barcode_inl.h); the offsets are checked here, so an add that is refused
//            has added nothing.  Nothing else of a record is kept
//   finish   with a br_whitelist set (br_cells_set_whitelist): first the barcodes resolved in place against it (whitelist.h: status
//            per name, a name without a match has no barcode any more; its tables are gone before the rest begins).  Then it
//            reads the quantifier's classes (quant_view.h: name_cls and the label tables; no EM is asked for).  The names that count
//            -- a barcode and a class -- sorted by (length, barcode) into cells; (cell << 32 | class) sorted and run-length encoded
//            into entries; the classes' feature lists by the quantifier's (class, gene) arena routine; entries x features expanded
//            into (cell << 32 | feature) pairs, whose stable sort gives every pair its slot and, as it stands, the per-slot lists of
//            entries; the cells routed by size; one launch for the values; the matrix without the slots that ended at 0 ("unique")
//
// Device memory (N names, M names that count, K cells, E entries, P pairs, S slots, Z matrix entries, C classes, L labels; every
// table has one entry more than its items): the adds hold 33 N (barcode 32, length 1).  finish keeps 4 N (the name's cell) + 69 K
// (barcode 32, length 1, matrix offset 8, names, unique, multi 8 each, features 4, iterations 4) + 12 Z (feature 4, value 8);
// while it runs 24 M (two key / index pairs) + 8 N (flags, then heads), 20 E (cell, class, n_e 4 each, pair offset 8) + 8 E (begins),
// the feature arena 24 L (two key / index pairs) + 8 L (flags) + 4 L + 12 C, 36 P (two key / index pairs 24, entry 4, slot 4, entry
// in slot order 4) + 8 P (flags), 28 S (feature 4, begin 8, theta 8, flag 8), 16 K (first entry, first slot) + 8 K (the route lists)
// and, where a cell takes the HBM route, 8 (S + E) of scratch.  128 bytes of counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "accum.h"
#include "barcode_inl.h"
#include "barcode_sort.h"
#include "cellcall.h"
#include "cellcall_kernels.h"
#include "cells_kernels.h"
#include "ctx.h"
#include "name_window.h"
#include "quant_kernels.h"
#include "quant_view.h"
#include "scan_kernels.h"
#include "whitelist.h"

using namespace br;

struct br_cells : Accum {
  int barcode_source = 0, mode = 0, hash_bits = 64;
  uint32_t barcode_sep = '_', barcode_tag = 'C' | 'B' << 8, lds_bytes = CL_LDS_MAX;
  int64_t max_iters = 10000;
  double tolerance = 1e-2;
  bool added = false, finished = false, dead = false;
  uint64_t n = 0;
  uint64_t n_no_barcode = 0, n_too_long = 0, n_bad_aux = 0;
  uint64_t n_counted = 0, n_cells = 0, n_entries = 0, n_pairs = 0, n_slots = 0, n_matrix = 0, n_wave = 0, n_block = 0, n_hbm = 0;
  double add_s = 0, finish_s = 0, em_s = 0;
  const br_whitelist *wl = nullptr;   // set: finish resolves the barcodes against it first ("correct": wl_correct)
  int wl_correct = 1;
  WlResolved wl_res;
  ColBuf small, cb, cblen, status;
  ColBuf name_cell, cell_cb, cell_len, m_off, m_feat, m_val, c_names, c_unique, c_multi, c_feat, c_iters;
  // "call_counts": the "unique" counts as integers (u_off, u_feat alias the matrix's in mode 0: empty here), then what br_cells_call left
  int call_counts = 0;
  bool called = false;
  uint64_t n_u = 0, n_called = 0, n_called_entries = 0;
  ColBuf u_off, u_feat, u_cnt, f_off, f_cells, f_feat, f_val;
};

extern "C" void br_cells_free(br_cells *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_cells_new(int device, br_cells **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  br_cells *c = new br_cells();
  const int rc = c->open(device, c->small, CL_WORDS);
  if (rc) { br_cells_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_cells_set_param(br_cells *c, const char *name, int64_t value) {
  if (!c || !name || c->dead || c->finished || c->added) return BR_ERR_INVALID_ARG;
  if (!strcmp(name, "barcode_source")) { if (value < 0 || value > 1) return BR_ERR_INVALID_ARG; c->barcode_source = (int)value; return BR_OK; }
  if (!strcmp(name, "barcode_sep")) { if (value < 0 || value > 255) return BR_ERR_INVALID_ARG; c->barcode_sep = (uint32_t)value; return BR_OK; }
  if (!strcmp(name, "barcode_tag")) { if (value < 0 || value > 65535) return BR_ERR_INVALID_ARG; c->barcode_tag = (uint32_t)value; return BR_OK; }
  if (!strcmp(name, "mode")) { if (value < 0 || value > 2) return BR_ERR_INVALID_ARG; c->mode = (int)value; return BR_OK; }
  if (!strcmp(name, "max_iters")) { if (value < 1 || value > 0xffffffffll) return BR_ERR_INVALID_ARG; c->max_iters = value; return BR_OK; }
  if (!strcmp(name, "hash_bits")) { if (value < 1 || value > 64) return BR_ERR_INVALID_ARG; c->hash_bits = (int)value; return BR_OK; }
  if (!strcmp(name, "call_counts")) { if (value < 0 || value > 1) return BR_ERR_INVALID_ARG; c->call_counts = (int)value; return BR_OK; }
  if (!strcmp(name, "lds_bytes")) { if (value < 0 || value > (int64_t)CL_LDS_MAX) return BR_ERR_INVALID_ARG; c->lds_bytes = (uint32_t)value; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

extern "C" int br_cells_set_whitelist(br_cells *c, const br_whitelist *wl, int correct) {
  if (!c || !wl || c->dead || c->finished || correct < 0 || correct > 2 || wl_device(wl) != c->device) return BR_ERR_INVALID_ARG;
  c->wl = wl; c->wl_correct = correct;
  return BR_OK;
}

extern "C" int br_cells_set_tolerance(br_cells *c, double tolerance) {
  if (!c || c->dead || c->finished || c->added || !(tolerance >= 0)) return BR_ERR_INVALID_ARG;
  c->tolerance = tolerance;
  return BR_OK;
}

// the names of one add, their tables on the device (A: names and recs but for recs.data are set).  data: the records' bytes from the
// first row's record on, in host or device memory
static int cells_add_names(br_cells *c, ClAddArgs A, const uint8_t *data, uint64_t bytes, bool on_device) {
  hipStream_t st = c->st;
  const uint64_t ng = (uint64_t)A.names.n_groups;
  if (c->n + ng >= (1ull << 32)) return BR_ERR_CAPACITY;
  for (ColBuf *b : {&c->cb, &c->cblen}) {
    const size_t want = (size_t)(c->n + ng + 1) * (b == &c->cb ? 32 : 1);
    if (want > b->cap) RC(c->alloc(*b, std::max(want, b->cap + b->cap / 2), true));
  }
  ColBuf window;
  DropGuard dropper{c, {&window}};
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + CL_BAD, 0, 4 * 8, st));   // CL_BAD .. CL_BAD_AUX
  if (on_device) A.recs.data = data;   // nothing of a record is kept: the kernels read them where they are,
  else {                               // or from a window that goes with the add
    RC(c->alloc(window, (size_t)bytes + 64));
    if (bytes) HIPCHK(hipMemcpyAsync(window.p, data, (size_t)bytes, hipMemcpyHostToDevice, st));
    A.recs.data = window.as<uint8_t>();
  }
  A.where = c->barcode_source == 0 ? BC_NAME_PREV : BC_TAG; A.sep = c->barcode_sep; A.tag = c->barcode_tag;
  A.cb = c->cb.as<uint64_t>() + 4 * c->n; A.cblen = c->cblen.as<uint8_t>() + c->n;
  A.counters = c->small.as<unsigned long long>();
  launch_cl_add(st, A);
  uint64_t seen[4];
  HIPCHK(hipMemcpyAsync(seen, small + CL_BAD, sizeof(seen), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's tables may be reused now
  if (seen[CL_BAD]) return BR_ERR_INVALID_ARG;   // nothing was added
  c->n += ng;
  c->n_no_barcode += seen[CL_NO_BC]; c->n_too_long += seen[CL_TOO_LONG]; c->n_bad_aux += seen[CL_BAD_AUX];
  return BR_OK;
}

extern "C" int br_cells_add(br_cells *c, const br_device_bam *recs, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups,
                            int on_device, void *stream) {
  if (!c || !recs || !rows || n_groups < 0 || c->dead || c->finished || (n_groups && (!rows->row_off || !group_off))) return BR_ERR_INVALID_ARG;
  if (rows->n_rows < 0 || recs->n_rows != rows->n_rows) return BR_ERR_INVALID_ARG;
  if (recs->n_rows && (!recs->data || !recs->row_off)) return BR_ERR_INVALID_ARG;
  if (n_groups == 0) { c->added = true; return BR_OK; }
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  uint64_t span[2] = {0, 0};
  RC(names_span(c, rows->row_off, (uint64_t)rows->n_rows, group_off, n_groups, on_device != 0, (hipStream_t)stream, c->small.as<uint64_t>() + CL_SPAN, span));
  ColBuf d_ro, d_go, d_rec;   // (host tables only; the rows themselves are not looked at)
  DropGuard dropper{c, {&d_ro, &d_go, &d_rec}};
  ClAddArgs A{};
  const uint8_t *data; uint64_t bytes;
  RC(record_window(c, *recs, span[0], span[1], on_device != 0, d_rec, &A.recs, &data, &bytes));
  if (on_device) A.names = device_names(rows->row_off, group_off, n_groups, span);
  else RC(upload_names(c, rows->row_off, group_off, n_groups, span, d_ro, d_go, &A.names));
  RC(cells_add_names(c, A, data, bytes, on_device != 0));   // (it waits for the stream)
  c->added = true;   // (an add that was refused decides nothing)
  return BR_OK;
}

extern "C" int br_cells_add_last(br_cells *c, br_ctx *ctx) {
  if (!c || !ctx || !ctx->ix || ctx->ix->device != c->device || c->dead || c->finished) return BR_ERR_INVALID_ARG;
  if (ctx->last_n_groups == 0) return BR_OK;   // a call without names
  br_device_bam recs; bool flat;
  last_call_records(ctx, &recs, &flat);
  if (flat) return BR_ERR_INVALID_ARG;   // a flat batch call left no records
  return br_cells_add(c, &recs, &ctx->last_rows, ctx->last_group_off, ctx->last_n_groups, 1, ctx->last_stream);
}

// the radix sort of (key[0], idx[0]) over the digits in which the keys differ (barcode_sort.h)
static int cells_sort(br_cells *c, SortBufs &s, int64_t n, ColBuf &tmp) { return sort_pairs(c, s, n, tmp, c->small.as<uint64_t>() + CL_BITS); }

static int cells_finish(br_cells *c, const QuantClassView &V, const uint32_t *tx_feature) {
  hipStream_t st = c->st;
  const int64_t N = (int64_t)c->n, C = V.n_cls, L = V.n_lab;
  const size_t n1 = (size_t)N + 1;
  uint64_t *small = c->small.as<uint64_t>();
  RC(c->alloc(c->name_cell, n1 * 4));
  HIPCHK(hipMemsetAsync(c->name_cell.p, 0xff, n1 * 4, st));
  RC(c->alloc(c->m_off, 8));
  HIPCHK(hipMemsetAsync(c->m_off.p, 0, 8, st));
  HIPCHK(hipStreamSynchronize(st));
  if (N == 0 || C == 0 || L == 0) return BR_OK;
  ColBuf tmp, flag;
  SortBufs s;
  DropGuard bufs{c, {&tmp, &flag, &s.key[0], &s.key[1], &s.idx[0], &s.idx[1]}};
  // the names that count
  uint64_t M = 0;
  RC(c->alloc(flag, n1 * 8));
  launch_cl_flag(st, c->cblen.as<uint8_t>(), V.name_cls, N, flag.as<uint64_t>());
  RC(c->scan_total(flag, N, tmp, &M));
  c->n_counted = M;
  if (M == 0) return BR_OK;
  if (M > (uint64_t)N) return BR_ERR_HIP;
  const int64_t n = (int64_t)M;
  RC(s.make(c, (size_t)M));
  launch_bc_compact(st, flag.as<uint64_t>(), N, s.idx[0].as<uint32_t>());
  // cells: by (length, bytes), least significant word first, every sort stable
  const uint64_t *cb = c->cb.as<uint64_t>();
  const uint8_t *cblen = c->cblen.as<uint8_t>();
  RC(sort_by_barcode(c, s, cb, cblen, nullptr, n, tmp, small + CL_BITS));
  uint64_t K = 0;
  RC(c->alloc(flag, ((size_t)M + 1) * 8));
  launch_bc_heads(st, s.idx[0].as<uint32_t>(), cb, cblen, nullptr, 0, n, flag.as<uint64_t>());
  RC(c->scan_total(flag, n, tmp, &K));
  if (K == 0 || K > M) return BR_ERR_HIP;
  const size_t k1 = (size_t)K + 1;
  RC(c->alloc(c->cell_cb, k1 * 32)); RC(c->alloc(c->cell_len, k1));
  launch_cl_cells(st, flag.as<uint64_t>(), s.idx[0].as<uint32_t>(), n, cb, cblen, V.name_cls, c->name_cell.as<uint32_t>(), c->cell_cb.as<uint64_t>(),
                  c->cell_len.as<uint8_t>(), s.key[0].as<uint64_t>());
  // entries: the runs of the sorted (cell, class) keys
  RC(cells_sort(c, s, n, tmp));
  launch_qg_flag(st, s.key[0].as<uint64_t>(), n, flag.as<uint64_t>());
  uint64_t E = 0;
  RC(c->scan_total(flag, n, tmp, &E));
  if (E < K || E > M) return BR_ERR_HIP;
  const size_t e1 = (size_t)E + 1;
  ColBuf ebeg, e_cell, e_cls, e_n, pair_off, cell_eoff, cell_soff, d_txf, glab, goff, gk;
  DropGuard ent_bufs{c, {&ebeg, &e_cell, &e_cls, &e_n, &pair_off, &cell_eoff, &cell_soff, &d_txf, &glab, &goff, &gk}};
  // the classes' feature lists: the quantifier's (class, gene) arena routine
  {
    SortBufs ls;
    ColBuf pos;
    DropGuard dropper{c, {&ls.key[0], &ls.key[1], &ls.idx[0], &ls.idx[1], &pos}};
    const size_t l1 = (size_t)L + 1, c1 = (size_t)C + 1;
    RC(c->alloc(d_txf, ((size_t)V.n_tx + 1) * 4));
    HIPCHK(hipMemcpyAsync(d_txf.p, tx_feature, (size_t)V.n_tx * 4, hipMemcpyHostToDevice, st));
    RC(ls.make(c, (size_t)L));
    launch_qg_key(st, V.label_off, V.labels, d_txf.as<uint32_t>(), C, L, ls.key[0].as<uint64_t>(), ls.idx[0].as<uint32_t>());
    RC(cells_sort(c, ls, L, tmp));
    RC(c->alloc(pos, l1 * 8));
    launch_qg_flag(st, ls.key[0].as<uint64_t>(), L, pos.as<uint64_t>());
    uint64_t LE = 0;
    RC(c->scan_total(pos, L, tmp, &LE));
    if (LE == 0 || LE > (uint64_t)L) return BR_ERR_HIP;
    RC(c->alloc(glab, ((size_t)LE + 1) * 4)); RC(c->alloc(goff, c1 * 8)); RC(c->alloc(gk, c1 * 4));
    launch_qg_arena(st, ls.key[0].as<uint64_t>(), pos.as<uint64_t>(), V.label_off, L, C, glab.as<uint32_t>(), goff.as<uint64_t>(), gk.as<uint32_t>());
    HIPCHK(hipStreamSynchronize(st));
  }
  RC(c->alloc(ebeg, e1 * 8)); RC(c->alloc(e_cell, e1 * 4)); RC(c->alloc(e_cls, e1 * 4)); RC(c->alloc(e_n, e1 * 4)); RC(c->alloc(pair_off, e1 * 8));
  RC(c->alloc(cell_eoff, k1 * 8)); RC(c->alloc(cell_soff, k1 * 8));
  launch_col_gbeg(st, flag.as<uint64_t>(), n, ebeg.as<uint64_t>());
  launch_cl_entries(st, s.key[0].as<uint64_t>(), ebeg.as<uint64_t>(), (int64_t)E, (int64_t)K, gk.as<uint32_t>(), e_cell.as<uint32_t>(), e_cls.as<uint32_t>(),
                    e_n.as<uint32_t>(), pair_off.as<uint64_t>(), cell_eoff.as<uint64_t>());
  uint64_t P = 0;
  RC(c->scan_total(pair_off, (int64_t)E, tmp, &P));
  if (P < E) return BR_ERR_HIP;   // (every class has a label, so every entry a feature)
  if (P >= (1ull << 32)) return BR_ERR_CAPACITY;
  c->drop(ebeg);
  for (int k = 0; k < 2; k++) { c->drop(s.key[k]); c->drop(s.idx[k]); }
  // pairs, slots and the per-slot lists
  const size_t p1 = (size_t)P + 1;
  ColBuf p_ent, pslot, t_ent, sbeg, s_feat, val;
  DropGuard pair_bufs{c, {&p_ent, &pslot, &t_ent, &sbeg, &s_feat, &val}};
  RC(s.make(c, (size_t)P)); RC(c->alloc(p_ent, p1 * 4)); RC(c->alloc(pslot, p1 * 4)); RC(c->alloc(t_ent, p1 * 4));
  launch_cl_pairs(st, (int64_t)E, e_cell.as<uint32_t>(), e_cls.as<uint32_t>(), pair_off.as<uint64_t>(), glab.as<uint32_t>(), goff.as<uint64_t>(),
                  s.key[0].as<uint64_t>(), s.idx[0].as<uint32_t>(), p_ent.as<uint32_t>());
  RC(cells_sort(c, s, (int64_t)P, tmp));
  RC(c->alloc(flag, p1 * 8));
  launch_qg_flag(st, s.key[0].as<uint64_t>(), (int64_t)P, flag.as<uint64_t>());
  uint64_t S = 0;
  RC(c->scan_total(flag, (int64_t)P, tmp, &S));
  if (S < K || S > P) return BR_ERR_HIP;
  const size_t s1 = (size_t)S + 1;
  RC(c->alloc(sbeg, s1 * 8)); RC(c->alloc(s_feat, s1 * 4)); RC(c->alloc(val, s1 * 8));
  launch_col_gbeg(st, flag.as<uint64_t>(), (int64_t)P, sbeg.as<uint64_t>());
  launch_cl_transpose(st, s.idx[0].as<uint32_t>(), flag.as<uint64_t>(), (int64_t)P, p_ent.as<uint32_t>(), pslot.as<uint32_t>(), t_ent.as<uint32_t>());
  launch_cl_slots(st, s.key[0].as<uint64_t>(), sbeg.as<uint64_t>(), (int64_t)S, (int64_t)K, s_feat.as<uint32_t>(), cell_soff.as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < 2; k++) { c->drop(s.key[k]); c->drop(s.idx[k]); }
  c->drop(p_ent); c->drop(glab); c->drop(goff); c->drop(gk); c->drop(d_txf);
  // the values
  ClTables T{};
  T.n_cells = (int64_t)K; T.cell_eoff = cell_eoff.as<uint64_t>(); T.cell_soff = cell_soff.as<uint64_t>(); T.pair_off = pair_off.as<uint64_t>();
  T.sbeg = sbeg.as<uint64_t>(); T.e_n = e_n.as<uint32_t>(); T.pslot = pslot.as<uint32_t>(); T.t_ent = t_ent.as<uint32_t>();
  RC(c->alloc(c->c_iters, k1 * 4));
  HIPCHK(hipMemsetAsync(c->c_iters.p, 0, k1 * 4, st));
  if (c->mode == 0) launch_cl_unique(st, T, (int64_t)S, val.as<double>());
  else {
    ColBuf lists, scratch;
    DropGuard dropper{c, {&lists, &scratch}};
    RC(c->alloc(lists, 2 * k1 * 4));
    HIPCHK(hipMemsetAsync(small + CL_NWAVE, 0, 4 * 8, st));   // CL_NWAVE .. CL_NEED
    uint32_t *wave_list = lists.as<uint32_t>(), *blk_list = wave_list + k1;
    launch_cl_route(st, T, c->lds_bytes, wave_list, blk_list, c->small.as<unsigned long long>());
    uint64_t got[4];
    HIPCHK(hipMemcpyAsync(got, small + CL_NWAVE, sizeof(got), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (got[0] + got[1] != K || got[2] > got[1] || got[3] > c->lds_bytes) return BR_ERR_HIP;
    c->n_wave = got[0]; c->n_hbm = got[2]; c->n_block = got[1] - got[2];
    if (c->n_hbm) RC(c->alloc(scratch, (size_t)(S + E + 1) * 8));
    ClEmArgs A{};
    A.T = T; A.wave_list = wave_list; A.blk_list = blk_list; A.n_wave = (uint32_t)got[0]; A.n_blk = (uint32_t)got[1];
    A.lds_bytes = c->lds_bytes; A.lds = (uint32_t)got[3];
    A.max_iters = c->mode == 1 ? 1u : (uint32_t)c->max_iters; A.tolerance = c->mode == 1 ? 0.0 : c->tolerance;
    A.n_slots = (int64_t)S; A.theta = val.as<double>(); A.scratch = scratch.as<double>(); A.n_iters = c->c_iters.as<uint32_t>();
    const ScopeTimer em_timer;
    launch_cl_em(st, A);
    HIPCHK(hipStreamSynchronize(st));
    c->em_s = em_timer.seconds();
  }
  // the matrix and the cells' numbers
  RC(c->alloc(c->c_names, k1 * 8)); RC(c->alloc(c->c_unique, k1 * 8)); RC(c->alloc(c->c_multi, k1 * 8)); RC(c->alloc(c->c_feat, k1 * 4));
  launch_cl_cell_stats(st, T, c->c_names.as<uint64_t>(), c->c_unique.as<uint64_t>(), c->c_multi.as<uint64_t>());
  RC(c->alloc(flag, s1 * 8));
  launch_cl_keep(st, val.as<double>(), (int64_t)S, c->mode == 0, flag.as<uint64_t>());
  uint64_t Z = 0;
  RC(c->scan_total(flag, (int64_t)S, tmp, &Z));
  if (Z > S) return BR_ERR_HIP;
  RC(c->alloc(c->m_off, k1 * 8)); RC(c->alloc(c->m_feat, ((size_t)Z + 1) * 4)); RC(c->alloc(c->m_val, ((size_t)Z + 1) * 8));
  launch_cl_matrix(st, T, flag.as<uint64_t>(), (int64_t)S, s_feat.as<uint32_t>(), val.as<double>(), c->m_off.as<uint64_t>(), c->m_feat.as<uint32_t>(),
                   c->m_val.as<double>(), c->c_feat.as<uint32_t>());
  HIPCHK(hipStreamSynchronize(st));
  if (c->call_counts) {   // the counts the cells are called on: "unique"'s values without the slots at 0, whatever the mode
    uint64_t U = Z;
    const double *from = c->m_val.as<double>();
    ColBuf uval, nf;
    DropGuard dropper{c, {&uval, &nf}};
    if (c->mode != 0) {
      RC(c->alloc(nf, k1 * 4));
      launch_cl_unique(st, T, (int64_t)S, val.as<double>());   // (the mode's values are in the matrix by now)
      launch_cl_keep(st, val.as<double>(), (int64_t)S, 1, flag.as<uint64_t>());
      RC(c->scan_total(flag, (int64_t)S, tmp, &U));
      if (U > S) return BR_ERR_HIP;
      RC(c->alloc(c->u_off, k1 * 8)); RC(c->alloc(c->u_feat, ((size_t)U + 1) * 4));
      RC(c->alloc(uval, ((size_t)U + 1) * 8));
      launch_cl_matrix(st, T, flag.as<uint64_t>(), (int64_t)S, s_feat.as<uint32_t>(), val.as<double>(), c->u_off.as<uint64_t>(), c->u_feat.as<uint32_t>(),
                       uval.as<double>(), nf.as<uint32_t>());
      from = uval.as<double>();
    }
    RC(c->alloc(c->u_cnt, ((size_t)U + 1) * 4));
    launch_cc_counts(st, from, U, c->u_cnt.as<uint32_t>());
    HIPCHK(hipStreamSynchronize(st));
    c->n_u = U;
  }
  c->n_cells = K; c->n_entries = E; c->n_pairs = P; c->n_slots = S; c->n_matrix = Z;
  return BR_OK;
}

extern "C" int br_cells_finish(br_cells *c, br_quant *quant, const uint32_t *tx_feature, int64_t n_features, int64_t *n_cells, int64_t *n_entries) {
  if (!c || !quant || c->dead || c->finished || n_features < 0 || n_features >= (1ll << 32)) return BR_ERR_INVALID_ARG;
  QuantClassView V{};
  if (quant_class_view(quant, &V) != BR_OK || V.device != c->device || (uint64_t)V.n_names != c->n) return BR_ERR_INVALID_ARG;
  if (V.n_tx > 0 && !tx_feature) return BR_ERR_INVALID_ARG;
  for (int64_t t = 0; t < V.n_tx; t++) if ((int64_t)tx_feature[t] >= n_features) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  int rc = BR_OK;
  if (c->wl) {   // the observed barcodes become whitelist entries, or nothing
    rc = c->alloc(c->status, (size_t)c->n + 1);
    if (!rc) rc = wl_resolve(c, c->wl, c->wl_correct, c->cb.as<uint64_t>(), c->cblen.as<uint8_t>(), (int64_t)c->n, c->status.as<uint8_t>(), nullptr, &c->wl_res);
  }
  if (!rc) rc = cells_finish(c, V, tx_feature);
  if (rc) { c->dead = true; return rc; }
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_cells) *n_cells = (int64_t)c->n_cells;
  if (n_entries) *n_entries = (int64_t)c->n_matrix;
  return BR_OK;
}

extern "C" int br_cells_barcodes(br_cells *c, int64_t first, int64_t n, uint8_t *cb, uint8_t *len) {
  if (!c || c->dead || !in_range(c->n, first, n)) return BR_ERR_INVALID_ARG;
  return c->fetch_fields(c->cb, c->cblen, first, n, cb, len);
}

extern "C" int br_cells_cell_barcodes(br_cells *c, int64_t first, int64_t n, uint8_t *cb, uint8_t *len) {
  if (!c || c->dead || !c->finished || !in_range(c->n_cells, first, n)) return BR_ERR_INVALID_ARG;
  return c->fetch_fields(c->cell_cb, c->cell_len, first, n, cb, len);
}

extern "C" int br_cells_name_cells(br_cells *c, int64_t first, int64_t n, uint32_t *cell) {
  if (!c || c->dead || !c->finished || !in_range(c->n, first, n)) return BR_ERR_INVALID_ARG;
  if (n == 0 || !cell) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(cell, c->name_cell.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_cells_name_status(br_cells *c, int64_t first, int64_t n, uint8_t *status) {
  if (!c || c->dead || !c->finished || !c->wl || !in_range(c->n, first, n)) return BR_ERR_INVALID_ARG;
  if (n == 0 || !status) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(status, c->status.as<uint8_t>() + first, (size_t)n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_cells_whitelist_stats(const br_cells *c, uint64_t out[8]) {
  return c && c->wl ? wl_stats(c->wl_res, c->wl_correct, out) : BR_ERR_INVALID_ARG;
}

extern "C" int br_cells_matrix(br_cells *c, int64_t first_cell, int64_t n, uint64_t *cell_off, uint32_t *feature, double *value) {
  if (!c || c->dead || !c->finished || !in_range(c->n_cells, first_cell, n) || !cell_off) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  HIPCHK(hipMemcpyAsync(cell_off, c->m_off.as<uint64_t>() + first_cell, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t z0 = cell_off[0], z = cell_off[n] - z0;
  if (z && feature) HIPCHK(hipMemcpyAsync(feature, c->m_feat.as<uint32_t>() + z0, (size_t)z * 4, hipMemcpyDeviceToHost, st));
  if (z && value) HIPCHK(hipMemcpyAsync(value, c->m_val.as<double>() + z0, (size_t)z * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t k = 0; k <= n; k++) cell_off[k] -= z0;
  return BR_OK;
}

extern "C" int br_cells_call(br_cells *c, br_cellcall *cc, int64_t n_features) {
  if (!c || c->dead || !c->finished || !c->call_counts || c->called || !cc_fresh(cc, c->device)) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const bool own = c->mode != 0;
  RC(cc_run(cc, (int64_t)c->n_cells, n_features, (own ? c->u_off : c->m_off).as<uint64_t>(), (own ? c->u_feat : c->m_feat).as<uint32_t>(),
            c->u_cnt.as<uint32_t>(), c->n_u));
  // the matrix's rows of the called cells
  int64_t K = 0;
  uint64_t n_called = 0;
  const uint8_t *status = cc_status(cc, &K, &n_called);
  if (!status || (uint64_t)K != c->n_cells) return BR_ERR_HIP;
  const size_t k1 = (size_t)K + 1;
  ColBuf flag, len, tmp;
  DropGuard bufs{c, {&flag, &len, &tmp}};
  RC(c->alloc(flag, k1 * 8)); RC(c->alloc(len, k1 * 8));
  HIPCHK(hipMemsetAsync(flag.p, 0, k1 * 8, st));
  HIPCHK(hipMemsetAsync(len.p, 0, k1 * 8, st));
  launch_cc_called(st, status, c->m_off.as<uint64_t>(), K, flag.as<uint64_t>(), len.as<uint64_t>());
  uint64_t got = 0, Zc = 0;
  RC(c->scan_total(flag, K, tmp, &got));
  RC(c->scan_total(len, K, tmp, &Zc));
  if (got != n_called || Zc > c->n_matrix) return BR_ERR_HIP;
  RC(c->alloc(c->f_off, ((size_t)got + 1) * 8)); RC(c->alloc(c->f_cells, ((size_t)got + 1) * 4));
  RC(c->alloc(c->f_feat, ((size_t)Zc + 1) * 4)); RC(c->alloc(c->f_val, ((size_t)Zc + 1) * 8));
  launch_cc_rows(st, status, flag.as<uint64_t>(), len.as<uint64_t>(), K, c->m_off.as<uint64_t>(), c->m_feat.as<uint32_t>(), c->m_val.as<double>(),
                 c->f_cells.as<uint32_t>(), c->f_off.as<uint64_t>(), c->f_feat.as<uint32_t>(), c->f_val.as<double>());
  HIPCHK(hipMemcpyAsync(c->f_off.as<uint64_t>() + got, &Zc, 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  c->n_called = got; c->n_called_entries = Zc; c->called = true;
  return BR_OK;
}

extern "C" int br_cells_matrix_called(br_cells *c, int64_t first, int64_t n, uint32_t *cells, uint64_t *cell_off, uint32_t *feature, double *value) {
  if (!c || c->dead || !c->called || !in_range(c->n_called, first, n) || !cell_off) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  HIPCHK(hipMemcpyAsync(cell_off, c->f_off.as<uint64_t>() + first, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
  if (n && cells) HIPCHK(hipMemcpyAsync(cells, c->f_cells.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t z0 = cell_off[0], z = cell_off[n] - z0;
  if (z && feature) HIPCHK(hipMemcpyAsync(feature, c->f_feat.as<uint32_t>() + z0, (size_t)z * 4, hipMemcpyDeviceToHost, st));
  if (z && value) HIPCHK(hipMemcpyAsync(value, c->f_val.as<double>() + z0, (size_t)z * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t k = 0; k <= n; k++) cell_off[k] -= z0;
  return BR_OK;
}

extern "C" int br_cells_cell_stats(br_cells *c, int64_t first, int64_t n, uint64_t *names, uint64_t *unique, uint64_t *multi, uint32_t *n_features,
                                   uint32_t *n_iters) {
  if (!c || c->dead || !c->finished || !in_range(c->n_cells, first, n)) return BR_ERR_INVALID_ARG;
  if (n == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  if (names) HIPCHK(hipMemcpyAsync(names, c->c_names.as<uint64_t>() + first, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (unique) HIPCHK(hipMemcpyAsync(unique, c->c_unique.as<uint64_t>() + first, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (multi) HIPCHK(hipMemcpyAsync(multi, c->c_multi.as<uint64_t>() + first, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (n_features) HIPCHK(hipMemcpyAsync(n_features, c->c_feat.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (n_iters) HIPCHK(hipMemcpyAsync(n_iters, c->c_iters.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

extern "C" int br_cells_stats(const br_cells *c, uint64_t out[16]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  const uint64_t v[16] = {c->n, c->n_counted, c->n_no_barcode, c->n_too_long, c->n_bad_aux, c->n_cells, c->n_entries, c->n_pairs, c->n_slots, c->n_matrix,
                          c->n_wave, c->n_block, c->n_hbm, (uint64_t)(c->add_s * 1e6), (uint64_t)(c->finish_s * 1e6), (uint64_t)(c->em_s * 1e6)};
  memcpy(out, v, sizeof(v));
  return BR_OK;
}
