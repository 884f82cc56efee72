// br_sorter: the projected records of a whole run in one device's HBM, handed out in coordinate order, and the BAI index of
// that order (sort_kernels.hip).
//
//   add      the rows of a br_device_bam ([block_size][record], contiguous) are appended to one arena with one copy; the
//            add-order offset table off (n + 1 entries, the last one the arena's end) grows with it
//   finish   key ((u32)refID << 32 | (u32)(pos + 1) << 1 | reverse strand; the CIGAR walk leaves each record's end) -> stable LSD
//            radix sort of (key, add index), the digits that are constant over all keys skipped -> the sizes of the records in
//            sorted order, scanned: s_off, the offset of every record in the sorted stream
//   next     the cut at max_bytes (a search in s_off), then a gather of the records [cur, e) into one of two buffers
//   index    per record: the BGZF block that holds its first byte (a search in the caller's block table) -> virtual offset, bin,
//            the largest end per reference; a stable radix sort of (refID << 32 | bin, sorted index); bin heads and chunk heads
//            (a chunk = consecutive records of the file in one bin), scanned; per reference the counts and the byte position of
//            its section; atomicMin of the virtual offsets into the 16 kb windows; the file image, written in place
//
// Device memory (n records, R arena bytes = sum of 4 + block_size): add holds R + 8 n (and, while the arena grows, the old arena
// beside the new one); finish adds keys 2 x 8 n, indices 2 x 4 n, ends 4 n, s_off 8 n and the radix histograms (2 KiB a tile of
// 2048), so its peak is R + 44 n; afterwards R + 32 n stay (off, the sorted keys, the order, ends, s_off), plus the two gather
// buffers of next (max_bytes each, and 8 bytes a record of theirs).  index holds 64 n more while it runs (virtual offsets 8 n,
// (refID, bin) keys 2 x 8 n, their indices 2 x 4 n, three scanned columns -- unmapped flags, bin heads, chunk heads -- 3 x 8 n, the
// bins' first chunks 8 n; all freed when it returns),
// 80 bytes a reference, 8 bytes a window and the image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/bramble_amd.h"
#include "accum.h"
#include "collate_kernels.h"
#include "scan_kernels.h"
#include "sort_kernels.h"

using namespace br;

struct br_sorter : Accum {
  uint64_t max_bytes = 0;     // 0: no cap but the device's memory
  bool finished = false;
  int64_t n = 0, cur = 0;
  uint64_t used = 0;            // arena bytes in use
  double add_s = 0, finish_s = 0, next_s = 0;
  ColBuf arena, off;                 // add order
  ColBuf key, order, ends, s_off;    // after finish: sorted keys, add index of every sorted record, ends (add order), stream offsets
  ColBuf buf[2], rows[2];            // next: two gather buffers alternate
  int which = 0;
  ColBuf tmp, small;
};

extern "C" void br_sorter_free(br_sorter *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_sorter_new(int device, br_sorter **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  br_sorter *c = new br_sorter();
  int rc = c->open(device);
  if (!rc) rc = c->alloc(c->small, 64);
  if (rc) { br_sorter_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_sorter_set_param(br_sorter *c, const char *name, int64_t value) {
  if (!c || !name || c->n || c->finished) return BR_ERR_INVALID_ARG;
  if (!strcmp(name, "max_bytes")) { if (value < 0) return BR_ERR_INVALID_ARG; c->max_bytes = (uint64_t)value; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

// room for m more records of `bytes` arena bytes (the arena keeps 64 bytes behind its end: the gather reads whole words)
static int sort_reserve(br_sorter *c, int64_t m, uint64_t bytes) {
  if ((uint64_t)(c->n + m) >= (1ull << 32)) return BR_ERR_CAPACITY;   // (32-bit radix indices)
  const uint64_t need = c->used + bytes;
  if (c->max_bytes && need > c->max_bytes) return BR_ERR_CAPACITY;
  if (need + 64 > c->arena.cap) {
    uint64_t want = std::max<uint64_t>(need + 64, c->arena.cap + c->arena.cap / 2);
    if (c->max_bytes) want = std::min<uint64_t>(want, c->max_bytes + 64);
    RC(c->alloc(c->arena, (size_t)want, true));
  }
  const size_t rn = (size_t)(c->n + m) + 1;
  if (rn * 8 > c->off.cap) RC(c->alloc(c->off, std::max(rn, (size_t)(c->off.cap / 8) * 3 / 2) * 8, true));
  return BR_OK;
}

static int sort_add_device(br_sorter *c, const br_device_bam *r, hipStream_t caller) {
  const int64_t m = r->n_rows;
  hipStream_t st = c->st;
  RC(c->after(caller));   // after whatever made the rows
  uint64_t ends[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&ends[0], r->row_off, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&ends[1], r->row_off + m, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ends[1] < ends[0] || ends[1] > r->n_bytes) return BR_ERR_INVALID_ARG;
  const uint64_t total = ends[1] - ends[0];
  RC(sort_reserve(c, m, total));
  if (total) HIPCHK(hipMemcpyAsync(c->arena.as<uint8_t>() + c->used, r->data + ends[0], (size_t)total, hipMemcpyDeviceToDevice, st));
  uint32_t *bad = (uint32_t *)(c->small.as<uint64_t>() + 6), h_bad = 0;
  HIPCHK(hipMemsetAsync(bad, 0, 4, st));
  launch_sort_offs(st, r->row_off, m, c->used, c->off.as<uint64_t>() + c->n, bad);
  HIPCHK(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's rows may be reused now
  if (h_bad) return BR_ERR_INVALID_ARG;   // row_off descends somewhere: nothing was added
  c->used += total; c->n += m;
  return BR_OK;
}

static int sort_add_host(br_sorter *c, const br_device_bam *r) {
  const int64_t m = r->n_rows;
  const uint64_t lo = r->row_off[0], hi = r->row_off[m];
  if (hi < lo || hi > r->n_bytes) return BR_ERR_INVALID_ARG;
  std::vector<uint64_t> off((size_t)m + 1);
  for (int64_t i = 0; i <= m; i++) {
    if (r->row_off[i] < lo || r->row_off[i] > hi || (i && r->row_off[i] < r->row_off[i - 1])) return BR_ERR_INVALID_ARG;
    off[(size_t)i] = c->used + (r->row_off[i] - lo);
  }
  RC(sort_reserve(c, m, hi - lo));
  hipStream_t st = c->st;
  if (hi > lo) HIPCHK(hipMemcpyAsync(c->arena.as<uint8_t>() + c->used, r->data + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->off.as<uint64_t>() + c->n, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  c->used += hi - lo; c->n += m;
  return BR_OK;
}

extern "C" int br_sorter_add(br_sorter *c, const br_device_bam *recs, int on_device, void *stream) {
  if (!c || !recs || recs->n_rows < 0 || (recs->n_rows && (!recs->data || !recs->row_off)) || c->finished) return BR_ERR_INVALID_ARG;
  if (recs->n_rows == 0) return BR_OK;
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  return on_device ? sort_add_device(c, recs, (hipStream_t)stream) : sort_add_host(c, recs);
}

static int sort_finish(br_sorter *c) {
  hipStream_t st = c->st;
  const int64_t n = c->n;
  const size_t n1 = (size_t)n + 1;
  ColBuf key[2], idx[2];
  DropGuard dropper{c, {&key[0], &key[1], &idx[0], &idx[1]}};   // (what finish keeps is swapped out of them)
  RC(c->alloc(key[0], n1 * 8)); RC(c->alloc(key[1], n1 * 8)); RC(c->alloc(idx[0], n1 * 4)); RC(c->alloc(idx[1], n1 * 4));
  RC(c->alloc(c->ends, n1 * 4)); RC(c->alloc(c->tmp, scan_tmp_bytes(n)));
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + 6, 0, 8, st));
  launch_sort_key(st, c->arena.as<uint8_t>(), c->off.as<uint64_t>(), n, key[0].as<uint64_t>(), idx[0].as<uint32_t>(), c->ends.as<uint32_t>(),
                  c->tmp.as<uint64_t>(), small, (uint32_t *)(small + 6));
  uint64_t bits[2] = {0, 0};
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(bits, small, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&bad, small + 6, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad) return BR_ERR_INVALID_ARG;   // a pos that is no BAM position
  int cur = 0;
  RC(c->radix_sort(key, idx, n, bits, c->tmp, &cur));
  RC(c->alloc(c->s_off, n1 * 8));
  launch_sort_lens(st, c->off.as<uint64_t>(), idx[cur].as<uint32_t>(), n, c->s_off.as<uint64_t>());
  launch_scan(st, c->s_off.as<uint64_t>(), n, c->tmp.as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  std::swap(c->key, key[cur]); std::swap(c->order, idx[cur]);
  return BR_OK;
}

extern "C" int br_sorter_finish(br_sorter *c, int64_t *n_records) {
  if (!c || c->finished) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  if (c->n) RC(sort_finish(c));
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_records) *n_records = c->n;
  return BR_OK;
}

extern "C" int br_sorter_next(br_sorter *c, uint64_t max_bytes, br_device_bam *piece) {
  if (!c || !piece || !c->finished) return BR_ERR_INVALID_ARG;
  memset(piece, 0, sizeof(*piece));
  if (c->cur >= c->n) return BR_OK;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  uint64_t *res = c->small.as<uint64_t>() + 4;
  launch_sort_cut(st, c->s_off.as<uint64_t>(), c->n, c->cur, max_bytes, res);
  uint64_t cut[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(cut, res, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t e = (int64_t)cut[0];
  if (e <= c->cur || e > c->n) return BR_ERR_HIP;
  const int w = c->which; c->which ^= 1;
  RC(c->alloc(c->buf[w], (size_t)cut[1] + 16)); RC(c->alloc(c->rows[w], (size_t)(e - c->cur + 1) * 8));
  launch_sort_gather(st, c->arena.as<uint8_t>(), c->off.as<uint64_t>(), c->order.as<uint32_t>(), c->s_off.as<uint64_t>(), c->cur, e,
                     c->buf[w].as<uint8_t>(), c->rows[w].as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  piece->data = c->buf[w].as<uint8_t>(); piece->n_bytes = cut[1]; piece->row_off = c->rows[w].as<uint64_t>(); piece->n_rows = e - c->cur;
  c->cur = e;
  c->next_s += timer.seconds();
  return BR_OK;
}

extern "C" int br_sorter_order(const br_sorter *c, int64_t *order) {
  if (!c || !c->finished || (!order && c->n)) return BR_ERR_INVALID_ARG;
  if (!c->n) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint32_t> o((size_t)c->n);
  HIPCHK(hipMemcpyAsync(o.data(), c->order.p, o.size() * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (size_t i = 0; i < o.size(); i++) order[i] = o[i];
  return BR_OK;
}

extern "C" int br_sorter_stats(const br_sorter *c, uint64_t *arena_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds,
                               double *next_seconds) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (arena_bytes) *arena_bytes = c->used;
  if (peak_bytes) *peak_bytes = c->peak;
  if (add_seconds) *add_seconds = c->add_s;
  if (finish_seconds) *finish_seconds = c->finish_s;
  if (next_seconds) *next_seconds = c->next_s;
  return BR_OK;
}

// ---- the index -------------------------------------------------------------------------------------------------------------
static int sort_index_device(br_sorter *c, int32_t n_ref, const br_bgzf_span *blocks, int64_t n_blocks, uint64_t eof_coffset, uint8_t **bai,
                             uint64_t *n_bytes) {
  hipStream_t st = c->st;
  const int64_t n = c->n;
  const size_t n1 = (size_t)n + 1, nr1 = (size_t)n_ref + 1;
  ColBuf blk, vo, key2[2], idx2[2], um, bh, ch, binc0, refmax, ref, lin_off, ref_pos, lin, out;
  // (whatever the outcome, the tables go when the call returns)
  DropGuard dropper{c, {&blk, &vo, &key2[0], &key2[1], &idx2[0], &idx2[1], &um, &bh, &ch, &binc0, &refmax, &ref, &lin_off, &ref_pos, &lin, &out}};
  RC(c->alloc(blk, (size_t)n_blocks * 16)); RC(c->alloc(vo, n1 * 8));
  RC(c->alloc(key2[0], n1 * 8)); RC(c->alloc(key2[1], n1 * 8)); RC(c->alloc(idx2[0], n1 * 4)); RC(c->alloc(idx2[1], n1 * 4));
  RC(c->alloc(um, n1 * 8)); RC(c->alloc(bh, (n1 + 1) * 8)); RC(c->alloc(ch, (n1 + 1) * 8)); RC(c->alloc(binc0, (n1 + 1) * 8));
  RC(c->alloc(refmax, nr1 * 4)); RC(c->alloc(ref, nr1 * sizeof(BaiRef))); RC(c->alloc(lin_off, nr1 * 8)); RC(c->alloc(ref_pos, nr1 * 8));
  RC(c->alloc(c->tmp, std::max(scan_tmp_bytes(n), scan_scratch_bytes(n_ref))));
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemcpyAsync(blk.p, blocks, (size_t)n_blocks * 16, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(small, 0, 32, st));
  HIPCHK(hipMemsetAsync(refmax.p, 0, nr1 * 4, st));
  HIPCHK(hipMemsetAsync(lin_off.p, 0, nr1 * 8, st)); HIPCHK(hipMemsetAsync(ref_pos.p, 0, nr1 * 8, st));
  BaiArgs A{};
  A.n = n; A.n_ref = n_ref; A.key = c->key.as<uint64_t>(); A.idx = c->order.as<uint32_t>(); A.ends = c->ends.as<uint32_t>(); A.s_off = c->s_off.as<uint64_t>();
  A.blk = blk.as<uint64_t>(); A.n_blk = n_blocks; A.eof_coffset = eof_coffset;
  A.vo = vo.as<uint64_t>(); A.key2[0] = key2[0].as<uint64_t>(); A.key2[1] = key2[1].as<uint64_t>(); A.idx2[0] = idx2[0].as<uint32_t>(); A.idx2[1] = idx2[1].as<uint32_t>();
  A.um = um.as<uint64_t>(); A.bh = bh.as<uint64_t>(); A.ch = ch.as<uint64_t>(); A.binc0 = binc0.as<uint64_t>(); A.refmax = refmax.as<uint32_t>();
  A.ref = ref.as<BaiRef>(); A.lin_off = lin_off.as<uint64_t>(); A.ref_pos = ref_pos.as<uint64_t>(); A.part = c->tmp.as<uint64_t>(); A.small = small;
  launch_bai_rec(st, A);
  uint64_t sm[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(sm, small, 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (sm[3] & (BAI_ERR_BLOCKS | BAI_ERR_REF)) return BR_ERR_INVALID_ARG;   // a record outside the block table, or a refID >= n_ref
  if (sm[3] & BAI_ERR_RANGE) return BR_ERR_UNSUPPORTED;                     // an end beyond 2^29: the binning scheme's reach
  RC(c->radix_sort(key2, idx2, n, sm, c->tmp, &A.cur));
  launch_scan(st, A.um, n, c->tmp.as<uint64_t>());
  launch_bai_heads(st, A);
  launch_scan(st, A.bh, n, c->tmp.as<uint64_t>());
  launch_scan(st, A.ch, n, c->tmp.as<uint64_t>());
  launch_bai_binc0(st, A);
  launch_bai_refs(st, A);
  if (n_ref > 0) { launch_scan(st, A.lin_off, n_ref, c->tmp.as<uint64_t>()); launch_scan(st, A.ref_pos, n_ref, c->tmp.as<uint64_t>()); }
  uint64_t tot[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&tot[0], A.lin_off + n_ref, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot[1], A.ref_pos + n_ref, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t total = 8 + tot[1] + 8;
  RC(c->alloc(lin, (size_t)(tot[0] + 1) * 8)); RC(c->alloc(out, (size_t)total));
  HIPCHK(hipMemsetAsync(lin.p, 0xff, (size_t)(tot[0] + 1) * 8, st));
  A.lin = lin.as<uint64_t>(); A.out = out.as<uint8_t>();
  launch_bai_lin(st, A);
  launch_bai_write(st, A);
  uint8_t *h = (uint8_t *)malloc((size_t)total);
  if (!h) return BR_ERR_CAPACITY;
  if (hipMemcpyAsync(h, out.p, (size_t)total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { free(h); return BR_ERR_HIP; }
  *bai = h; *n_bytes = total;
  return BR_OK;
}

extern "C" int br_sorter_index(br_sorter *c, int32_t n_ref, const br_bgzf_span *blocks, int64_t n_blocks, uint64_t eof_coffset, uint8_t **bai,
                               uint64_t *n_bytes) {
  if (!c || !c->finished || n_ref < 0 || n_blocks < 0 || (n_blocks && !blocks) || !bai || !n_bytes) return BR_ERR_INVALID_ARG;
  *bai = nullptr; *n_bytes = 0;
  if (c->n && (n_blocks == 0 || blocks[0].uoffset != 0)) return BR_ERR_INVALID_ARG;
  for (int64_t b = 1; b < n_blocks; b++) if (blocks[b].uoffset < blocks[b - 1].uoffset || blocks[b].coffset <= blocks[b - 1].coffset) return BR_ERR_INVALID_ARG;
  if (c->n == 0) {   // no record: every reference is empty
    const size_t total = 8 + (size_t)n_ref * 8 + 8;
    uint8_t *h = (uint8_t *)calloc(total, 1);
    if (!h) return BR_ERR_CAPACITY;
    memcpy(h, "BAI\1", 4); memcpy(h + 4, &n_ref, 4);
    *bai = h; *n_bytes = total;
    return BR_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  return sort_index_device(c, n_ref, blocks, n_blocks, eof_coffset, bai, n_bytes);
}
