// The reader side on the device: BGZF block scan, inflate, record split, br_bam_reader (whole-buffer and piece-wise) and
// the host record split.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "ctx.h"

// ---------------------------------------------------------------------------
// BGZF inflate on the device
// ---------------------------------------------------------------------------
static_assert(sizeof(br_bgzf_block) == sizeof(InflateBlock), "br_bgzf_block is the kernel's block descriptor");

extern "C" int br_bgzf_scan(const uint8_t *data, uint64_t n_bytes, int64_t cap, br_bgzf_block *blocks, int64_t *n_blocks,
                            uint64_t *consumed, uint64_t *out_bytes) {
  if ((!data && n_bytes) || !blocks || !n_blocks || !consumed || !out_bytes || cap < 0) return BR_ERR_INVALID_ARG;
  uint64_t p = 0, total = 0; int64_t n = 0;
  while (n < cap && p + 18 <= n_bytes) {
    const uint8_t *h = data + p;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return BR_ERR_INVALID_ARG;   // not a BGZF block
    const uint32_t xlen = h[10] | ((uint32_t)h[11] << 8);
    if (p + 12 + xlen > n_bytes) break;
    int64_t bsize = -1;
    for (uint32_t q = 0; q + 4 <= xlen;) {
      const uint8_t *x = h + 12 + q;
      const uint32_t slen = x[2] | ((uint32_t)x[3] << 8);
      if (x[0] == 'B' && x[1] == 'C' && slen == 2 && q + 6 <= xlen) bsize = (x[4] | (x[5] << 8)) + 1;
      q += 4 + slen;
    }
    if (bsize < (int64_t)(12 + xlen + 8)) return BR_ERR_INVALID_ARG;            // no BC subfield
    if (p + (uint64_t)bsize > n_bytes) break;                                     // partial block: next call
    const uint8_t *t = h + bsize - 8;
    const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24), ulen = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    if (ulen > 65536) return BR_ERR_INVALID_ARG;
    if (ulen) {   // (empty blocks -- the EOF marker -- are stepped over)
      br_bgzf_block &b = blocks[n++];
      b.src_off = p + 12 + xlen; b.dst_off = total; b.clen = (uint32_t)(bsize - 12 - xlen - 8); b.ulen = ulen; b.crc = crc; b.pad = 0;
      total += ulen;
    }
    p += (uint64_t)bsize;
  }
  *n_blocks = n; *consumed = p; *out_bytes = total;
  return BR_OK;
}

// dst_ext: where the inflated bytes go (room for every block's dst_off + ulen), or null: the context's own buffer
static int inflate_impl(br_ctx *c, const uint8_t *src, uint64_t n_src, const br_bgzf_block *blocks, int64_t n_blocks, hipStream_t st,
                        uint8_t *dst_ext, const uint8_t **out, uint64_t *out_bytes) {
  *out = nullptr; *out_bytes = 0;
  if (n_blocks == 0) return BR_OK;
  uint64_t total = 0;
  for (int64_t i = 0; i < n_blocks; i++) {
    const br_bgzf_block &b = blocks[i];
    if (b.ulen > 65536 || b.src_off + b.clen + 8 > n_src) return BR_ERR_INVALID_ARG;   // (+ 8: the block's CRC32 / ISIZE trailer lies inside the buffer)
    total = std::max<uint64_t>(total, b.dst_off + b.ulen);
  }
  if (!c->inf_tabs_ready) {
    // slice-by-4 tables of the reflected CRC-32 and the operator that appends INFLATE_CRC_CHUNK zero bytes (see deflate_device_impl)
    std::vector<uint32_t> t(1024 + 1024);
    for (uint32_t i = 0; i < 256; i++) { uint32_t v = i; for (int k = 0; k < 8; k++) v = (v & 1u) ? 0xEDB88320u ^ (v >> 1) : v >> 1; t[i] = v; }
    for (int k = 1; k < 4; k++) for (uint32_t i = 0; i < 256; i++) { const uint32_t p = t[256 * (k - 1) + i]; t[256 * k + i] = (p >> 8) ^ t[p & 0xffu]; }
    uint32_t col[32];
    for (int b = 0; b < 32; b++) { uint32_t v = 1u << b; for (uint32_t k = 0; k < INFLATE_CRC_CHUNK; k++) v = (v >> 8) ^ t[v & 0xffu]; col[b] = v; }
    for (int byte = 0; byte < 4; byte++)
      for (uint32_t x = 0; x < 256; x++) { uint32_t v = 0; for (int b = 0; b < 8; b++) if (x & (1u << b)) v ^= col[8 * byte + b]; t[1024 + 256 * byte + x] = v; }
    RC(c->inf_tabs.ensure(t.size() * 4));
    HIPCHK(hipMemcpyAsync(c->inf_tabs.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    c->inf_tabs_ready = true;
  }
  if (!dst_ext) RC(c->inf_out.ensure((size_t)total + 16));
  RC(c->inf_blocks.ensure((size_t)n_blocks * sizeof(InflateBlock))); RC(c->inf_cnt.ensure(16));
  HIPCHK(hipMemcpyAsync(c->inf_blocks.p, blocks, (size_t)n_blocks * sizeof(InflateBlock), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->inf_cnt.p, 0, 16, st));
  InflateArgs A{};
  A.src = src; A.n_src = n_src; A.dst = dst_ext ? dst_ext : c->inf_out.as<uint8_t>(); A.blocks = (const InflateBlock *)c->inf_blocks.p; A.n_blocks = (uint64_t)n_blocks;
  A.queue = c->inf_cnt.as<uint32_t>(); A.n_bad = c->inf_cnt.as<uint32_t>() + 1;
  A.crc_tab4 = c->inf_tabs.as<uint32_t>(); A.crc_shift = c->inf_tabs.as<uint32_t>() + 1024;
  const int waves = (int)std::min<uint64_t>(((uint64_t)n_blocks + 3) / 4 * 4, (uint64_t)c->n_cu * 20);   // five workgroups of four waves per CU (their LDS and registers)
  Prof pf{c, st};
  c->events_used = 0;
  RC(pf.begin(BR_K_CODEC));
  launch_inflate(st, A, waves);
  RC(pf.end());
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, A.n_bad, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  RC(pf.collect());
  if (bad) return BR_ERR_INVALID_ARG;   // a block that does not inflate to its ISIZE bytes with its CRC32
  *out = A.dst; *out_bytes = total;
  return BR_OK;
}

extern "C" int br_bgzf_inflate_device(br_ctx *c, const uint8_t *src, uint64_t n_src, const br_bgzf_block *blocks, int64_t n_blocks,
                                      void *stream, const uint8_t **out, uint64_t *out_bytes) {
  if (!c || (!src && n_src) || (!blocks && n_blocks) || n_blocks < 0 || !out || !out_bytes) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  return inflate_impl(c, src, n_src, blocks, n_blocks, (hipStream_t)stream, nullptr, out, out_bytes);
}

// br_bam_split on the device (split_kernels.hip): data = an inflated BAM alignment section in HBM that starts at a record
static int split_impl(br_ctx *c, const uint8_t *data, uint64_t n_bytes, int32_t n_ref, hipStream_t st, br_device_records *recs,
                      int64_t *n_unmapped, uint64_t *consumed, SplitArgs *S_out) {
  memset(recs, 0, sizeof(*recs));
  recs->blob = data; *consumed = 0;
  if (n_unmapped) *n_unmapped = 0;
  if (S_out) *S_out = SplitArgs{};
  if (n_bytes == 0) return BR_OK;
  const int64_t n_seg = (int64_t)((n_bytes + SPLIT_SEG_BYTES - 1) / SPLIT_SEG_BYTES);
  const size_t ns = (size_t)n_seg;
  RC(c->sp_entry.ensure(ns * 8)); RC(c->sp_entry2.ensure(ns * 8)); RC(c->sp_exit.ensure(ns * 8)); RC(c->sp_nmap.ensure(ns * 4));
  RC(c->sp_nunm.ensure(ns * 4)); RC(c->sp_ended.ensure(ns * 4)); RC(c->sp_redo.ensure(ns * 4)); RC(c->sp_pre.ensure((ns + 1) * 8));
  RC(c->sp_small.ensure(64));   // flags[2] (u32) | totals[2] (u64) at +16 | mapped total (u64) at +32
  RC(c->tile_sums.ensure((size_t)std::max<int64_t>(scan_tiles_for(n_seg + 1), 1) * 8 * 3));
  HIPCHK(hipMemsetAsync(c->sp_small.p, 0, 64, st));
  SplitArgs S{};
  S.data = data; S.n_bytes = n_bytes; S.n_ref = n_ref; S.seg_bytes = SPLIT_SEG_BYTES; S.n_seg = n_seg;
  S.entry = c->sp_entry.as<uint64_t>(); S.entry_next = c->sp_entry2.as<uint64_t>(); S.exit_ = c->sp_exit.as<uint64_t>();
  S.n_map = c->sp_nmap.as<uint32_t>(); S.n_unm = c->sp_nunm.as<uint32_t>(); S.ended = c->sp_ended.as<uint32_t>();
  S.flags = c->sp_small.as<uint32_t>(); S.totals = (uint64_t *)(c->sp_small.as<uint8_t>() + 16);
  uint32_t *redo = c->sp_redo.as<uint32_t>();
  launch_split_guess(st, S);
  if (c->split_spoil > 0) launch_split_spoil(st, S, c->split_spoil);   // test hook (br_ctx_set_param "split_spoil"): wrong guesses on purpose
  launch_split_walk(st, S, nullptr);
  for (int pass = 0;; pass++) {
    // every guess against where the chain of the segments in front arrives; the segments that were wrong walk again
    HIPCHK(hipMemsetAsync(S.flags + 1, 0, 4, st));
    launch_split_check(st, S, redo);
    uint32_t changed = 0;
    HIPCHK(hipMemcpyAsync(&changed, S.flags + 1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::swap(S.entry, S.entry_next);
    static const bool split_debug = getenv("BRAMBLE_AMD_SPLIT_DEBUG") != nullptr;
    if (split_debug && (pass < 12 || !changed)) fprintf(stderr, "[split] pass %d: %u of %lld segments took another entry\n", pass, changed, (long long)n_seg);
    if (!changed) break;
    if (pass > n_seg + 2) return BR_ERR_INVALID_ARG;   // (cannot happen: every pass settles at least the first wrong segment)
    launch_split_walk(st, S, redo);
  }
  launch_scan(st, S.n_map, n_seg, c->tile_sums.as<uint64_t>(), c->sp_pre.p, true, (uint64_t *)(c->sp_small.as<uint8_t>() + 32));
  uint64_t n_mapped = 0;
  HIPCHK(hipMemcpyAsync(&n_mapped, c->sp_small.as<uint8_t>() + 32, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  RC(c->sp_off.ensure(std::max<size_t>((size_t)n_mapped, 1) * 8)); RC(c->sp_len.ensure(std::max<size_t>((size_t)n_mapped, 1) * 4));
  S.map_pre = c->sp_pre.as<uint64_t>(); S.rec_off = c->sp_off.as<uint64_t>(); S.rec_len = c->sp_len.as<uint32_t>();
  launch_split_emit(st, S);
  launch_split_totals(st, S);
  struct { uint32_t flags[4]; uint64_t totals[2]; } h;
  HIPCHK(hipMemcpyAsync(&h, c->sp_small.p, 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (h.flags[0] & 1u) return BR_ERR_INVALID_ARG;      // a record whose fixed fields overrun its block_size (as br_bam_split)
  recs->rec_off = S.rec_off; recs->rec_len = S.rec_len; recs->n_aln = (int64_t)n_mapped;
  if (n_unmapped) *n_unmapped = (int64_t)h.totals[0];
  *consumed = h.totals[1];
  if (S_out) *S_out = S;
  return BR_OK;
}

extern "C" int br_bam_split_device(br_ctx *c, const uint8_t *data, uint64_t n_bytes, int32_t n_ref, void *stream, br_device_records *recs,
                                   int64_t *n_unmapped, uint64_t *consumed) {
  if (!c || (!data && n_bytes) || !recs || !consumed || n_ref < 0) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->ix->device));
  return split_impl(c, data, n_bytes, n_ref, (hipStream_t)stream, recs, n_unmapped, consumed, nullptr);
}

// ---------------------------------------------------------------------------
// br_bam_reader: BGZF bytes of a BAM file in, bundles of device-resident records of whole read-name groups out.  What the host
// reader of the command line does with sixteen inflate threads and a serial chain walk (inflate -> br_bam_split -> cut at a
// read-name change -> upload), done where the records are needed: the compressed bytes go up as they are, k_inflate and
// k_split_* make records of them, and the bytes behind the last complete name group wait in HBM for the next piece.
// It needs no index (the command line runs it beside the guide parsing and the index build).
// ---------------------------------------------------------------------------
struct br_bam_reader {
  br_index shell;                  // carries the device for the private context below; never used for projection
  br_ctx *c = nullptr;
  int32_t n_ref = 0;
  uint64_t skip = 0;               // inflated bytes still to skip (the BAM header in front of the first record)
  int64_t max_blocks = 3072;       // BGZF blocks per piece (about 200 MB inflated)
  hipStream_t st = nullptr;
  struct Chunk { DevBuf data, off, len; int64_t id = -1; bool out = false; };   // out: handed to the caller, not yet released
  std::vector<std::unique_ptr<Chunk>> chunks;
  std::mutex m;
  Chunk *carry_from = nullptr; uint64_t carry_off = 0, carry_len = 0;
  DevBuf comp, small;
  // piece-wise reading (br_bam_piece_*): two upload slots, filled on a copy stream of their own beside the processing of the
  // piece before
  struct PieceSlot { DevBuf comp; hipEvent_t up = nullptr; int64_t b0 = -1, b1x = -1; uint64_t src0 = 0, n_src = 0; };
  PieceSlot pslot[2];
  hipStream_t copy_st = nullptr;
  // the way up: PIN_THREADS host threads copy the mapped file's bytes into pinned buffers of their own (two each) and
  // queue the transfers from there -- a transfer straight from the pageable mapping goes through the driver's one staging
  // thread at a fifth of the wire's rate
  static constexpr int PIN_THREADS = 4, PIN_SLOTS = 2;
  static constexpr size_t PIN_BYTES = 4u << 20;
  struct PinBuf { uint8_t *p = nullptr; hipEvent_t done = nullptr; bool used = false; };
  PinBuf pin[PIN_THREADS][PIN_SLOTS];
  std::mutex up_m;                 // one upload at a time (the pinned buffers; a piece that asks for more blocks uploads from the processing thread)
  double t_upload = 0;
  std::vector<br_bgzf_block> pblocks;
  double t_proc = 0;
  std::vector<br_bgzf_block> blocks;
  int64_t next_id = 0;
  bool finished = false;
  double t_scan = 0, t_up = 0, t_inflate = 0, t_split = 0, t_cut = 0;   // BRAMBLE_AMD_TIMING
};

extern "C" int br_bam_reader_new(int device, int32_t n_ref, uint64_t header_bytes, br_bam_reader **out) {
  if (!out || n_ref < 0) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  int rc = check_device(device);
  if (rc) return rc;
  auto r = std::make_unique<br_bam_reader>();
  r->shell.device = device; r->n_ref = n_ref; r->skip = header_bytes;
  RC(br_ctx_new(&r->shell, &r->c));
  // the lowest priority the device offers: once the projection has started, its kernels go first (what the reader makes is
  // needed a few bundles later; what the runner makes is what the writer waits for)
  int prio_low = 0, prio_high = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
  HIPCHK(hipStreamCreateWithPriority(&r->st, hipStreamNonBlocking, prio_low));
  *out = r.release();
  return BR_OK;
}

extern "C" int br_bam_reader_set_piece_blocks(br_bam_reader *r, int64_t blocks) {
  if (!r || blocks < 1 || blocks > (1 << 20)) return BR_ERR_INVALID_ARG;
  r->max_blocks = blocks;
  return BR_OK;
}

extern "C" void br_bam_reader_free(br_bam_reader *r) {
  if (!r) return;
  (void)hipSetDevice(r->shell.device);   // (the buffers are freed on this device when the reader goes)
  for (auto &ps : r->pslot) if (ps.up) (void)hipEventDestroy(ps.up);
  for (auto &row : r->pin) for (auto &pb : row) { if (pb.used && pb.done) (void)hipEventSynchronize(pb.done); if (pb.p) (void)hipHostFree(pb.p); if (pb.done) (void)hipEventDestroy(pb.done); }
  if (r->copy_st) (void)hipStreamDestroy(r->copy_st);
  if (r->st) (void)hipStreamDestroy(r->st);
  if (r->c) br_ctx_free(r->c);
  delete r;
}

extern "C" int br_bam_reader_release(br_bam_reader *r, int64_t id) {
  if (!r) return BR_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> l(r->m);
  for (auto &ch : r->chunks) if (ch->id == id) { ch->out = false; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

extern "C" int br_bam_reader_next(br_bam_reader *r, const uint8_t *data, uint64_t n_bytes, int last, uint64_t *consumed,
                                  br_device_records *bundle, int64_t *id, int64_t *n_unmapped) {
  if (!r || (!data && n_bytes) || !consumed || !bundle || !id || !n_unmapped) return BR_ERR_INVALID_ARG;
  memset(bundle, 0, sizeof(*bundle));
  *consumed = 0; *id = -1; *n_unmapped = 0;
  if (r->finished) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(r->shell.device));
  hipStream_t st = r->st;
  auto tnow = []() { return std::chrono::steady_clock::now(); };
  auto tsec = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
  auto tp = tnow();
  // the complete blocks of this piece
  r->blocks.resize((size_t)r->max_blocks);
  int64_t nb = 0; uint64_t used = 0, total = 0;
  RC(br_bgzf_scan(data, n_bytes, r->max_blocks, r->blocks.data(), &nb, &used, &total));
  r->t_scan += tsec(tp); tp = tnow();
  *consumed = used;
  const bool at_end = last && used == n_bytes;       // nothing of the file is left behind this piece
  if (last && nb < r->max_blocks && used != n_bytes) return BR_ERR_INVALID_ARG;   // a truncated block at the end of the file
  if (nb == 0 && !at_end) return BR_OK;              // (only empty blocks so far)
  // a chunk to hold: what the last piece left over + this piece's bytes
  br_bam_reader::Chunk *ch = nullptr;
  {
    std::lock_guard<std::mutex> l(r->m);
    for (auto &x : r->chunks) if (!x->out && x.get() != r->carry_from) { ch = x.get(); break; }
    if (!ch) { r->chunks.push_back(std::make_unique<br_bam_reader::Chunk>()); ch = r->chunks.back().get(); }
  }
  RC(ch->data.ensure((size_t)(r->carry_len + total) + 64));
  if (r->carry_len) HIPCHK(hipMemcpyAsync(ch->data.p, r->carry_from->data.as<uint8_t>() + r->carry_off, (size_t)r->carry_len, hipMemcpyDeviceToDevice, st));
  if (nb) {
    RC(r->comp.ensure((size_t)used + 64));
    HIPCHK(hipMemcpyAsync(r->comp.p, data, (size_t)used, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    r->t_up += tsec(tp); tp = tnow();
    const uint8_t *o = nullptr; uint64_t ob = 0;
    RC(inflate_impl(r->c, r->comp.as<uint8_t>(), used, r->blocks.data(), nb, st, ch->data.as<uint8_t>() + r->carry_len, &o, &ob));
    r->t_inflate += tsec(tp); tp = tnow();
  }
  uint64_t have = r->carry_len + total, start = 0;
  if (r->skip) { start = std::min<uint64_t>(r->skip, have); r->skip -= start; }   // (the header never leaves a carry: nothing is split before it ends)
  const uint8_t *base = ch->data.as<uint8_t>() + start;
  const uint64_t nbytes = have - start;
  br_device_records recs; int64_t unm_all = 0; uint64_t used_bytes = 0; SplitArgs S{};
  RC(split_impl(r->c, base, nbytes, r->n_ref, st, &recs, &unm_all, &used_bytes, &S));
  r->t_split += tsec(tp); tp = tnow();
  const int64_t n = recs.n_aln;
  // the cut: everything in front of the last read-name group (it may go on in the next piece); at the end of the file, all
  int64_t n_take = n; uint64_t cut = used_bytes;
  RC(r->small.ensure(64));
  if (!at_end && n > 0) {
    HIPCHK(hipMemsetAsync(r->small.p, 0, 16, st));
    launch_last_group(st, base, recs.rec_off, n, (unsigned long long *)r->small.p);
    uint64_t g = 0;
    HIPCHK(hipMemcpyAsync(&g, r->small.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    n_take = (int64_t)g;
    uint64_t off_g = 0;
    HIPCHK(hipMemcpyAsync(&off_g, recs.rec_off + n_take, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    cut = off_g - 4;
  }
  if (at_end && used_bytes != nbytes) return BR_ERR_INVALID_ARG;   // a truncated record at the end of the file
  // unmapped records in front of the cut (the ones behind it are met again with the next piece)
  int64_t unm = unm_all;
  if (cut != used_bytes && S.n_seg) {
    HIPCHK(hipMemsetAsync(r->small.as<uint8_t>() + 16, 0, 8, st));
    launch_unmapped_before(st, S, cut, (unsigned long long *)(r->small.as<uint8_t>() + 16));
    uint64_t u = 0;
    HIPCHK(hipMemcpyAsync(&u, r->small.as<uint8_t>() + 16, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unm = (int64_t)u;
  }
  // the bundle's tables live with the chunk (the context's are overwritten by the next piece)
  if (n_take) {
    RC(ch->off.ensure((size_t)n_take * 8)); RC(ch->len.ensure((size_t)n_take * 4));
    HIPCHK(hipMemcpyAsync(ch->off.p, recs.rec_off, (size_t)n_take * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(ch->len.p, recs.rec_len, (size_t)n_take * 4, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  {
    std::lock_guard<std::mutex> l(r->m);
    ch->id = r->next_id++; ch->out = true;
    r->carry_from = ch; r->carry_off = start + cut; r->carry_len = nbytes - cut;
  }
  r->t_cut += tsec(tp);
  if (at_end) {
    r->finished = true;
    if (getenv("BRAMBLE_AMD_TIMING")) fprintf(stderr, "[reader] block scan %.2fs, upload of the compressed bytes %.2fs, inflate %.2fs, record split %.2fs, cuts + tables %.2fs\n", r->t_scan, r->t_up, r->t_inflate, r->t_split, r->t_cut);
  }
  bundle->blob = base; bundle->rec_off = ch->off.as<uint64_t>(); bundle->rec_len = ch->len.as<uint32_t>(); bundle->n_aln = n_take;
  *id = ch->id; *n_unmapped = unm;
  return BR_OK;
}

// ---------------------------------------------------------------------------
// Piece-wise device reader.  The caller holds the whole file's block table (br_bgzf_scan over the mapping) and hands out
// pieces [b0, b1) of it -- to one reader in order, or to several readers on several devices: a piece needs nothing from
// its neighbours (see split_kernels.hip: the cut rule).  br_bam_piece_upload may run on another thread than
// br_bam_piece_process, one piece ahead (two slots).
// ---------------------------------------------------------------------------
extern "C" int br_bam_piece_upload(br_bam_reader *r, int slot, const uint8_t *file, uint64_t file_bytes, const br_bgzf_block *blocks,
                                   int64_t n_blocks, int64_t b0, int64_t b1x) {
  if (!r || slot < 0 || slot > 1 || !file || !blocks || b0 < 0 || b1x <= b0 || b1x > n_blocks) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(r->shell.device));
  if (!r->copy_st) HIPCHK(hipStreamCreateWithFlags(&r->copy_st, hipStreamNonBlocking));
  br_bam_reader::PieceSlot &P = r->pslot[slot];
  if (!P.up) HIPCHK(hipEventCreateWithFlags(&P.up, hipEventDisableTiming));
  const uint64_t src0 = blocks[b0].src_off, src1 = blocks[b1x - 1].src_off + blocks[b1x - 1].clen + 8;
  if (src1 > file_bytes || src1 <= src0) return BR_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> up_lock(r->up_m);
  RC(P.comp.ensure((size_t)(src1 - src0) + 64));
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t n = src1 - src0;
  const uint64_t n_chunks = (n + br_bam_reader::PIN_BYTES - 1) / br_bam_reader::PIN_BYTES;
  for (auto &row : r->pin) for (auto &pb : row) {
    if (!pb.p) { HIPCHK(hipHostMalloc((void **)&pb.p, br_bam_reader::PIN_BYTES, hipHostMallocDefault)); HIPCHK(hipEventCreateWithFlags(&pb.done, hipEventDisableTiming)); }
  }
  std::atomic<int> failed{0};
  auto work = [&](int w) {
    if (hipSetDevice(r->shell.device) != hipSuccess) { failed = 1; return; }
    int j = 0;
    for (uint64_t k = (uint64_t)w; k < n_chunks && !failed; k += br_bam_reader::PIN_THREADS, j ^= 1) {
      br_bam_reader::PinBuf &pb = r->pin[w][j];
      if (pb.used && hipEventSynchronize(pb.done) != hipSuccess) { failed = 1; return; }   // its last transfer (this call's or an earlier one's)
      const uint64_t off = k * br_bam_reader::PIN_BYTES, len = std::min<uint64_t>(br_bam_reader::PIN_BYTES, n - off);
      memcpy(pb.p, file + src0 + off, (size_t)len);
      if (hipMemcpyAsync(P.comp.as<uint8_t>() + off, pb.p, (size_t)len, hipMemcpyHostToDevice, r->copy_st) != hipSuccess ||
          hipEventRecord(pb.done, r->copy_st) != hipSuccess) { failed = 1; return; }
      pb.used = true;
    }
  };
  {
    std::vector<std::thread> th;
    const int nt = (int)std::min<uint64_t>(br_bam_reader::PIN_THREADS, n_chunks);
    for (int w = 1; w < nt; w++) th.emplace_back(work, w);
    work(0);
    for (auto &t : th) t.join();
  }
  if (failed) return BR_ERR_HIP;
  HIPCHK(hipEventRecord(P.up, r->copy_st));   // (everything queued above; br_bam_piece_process waits for it on its own stream)
  r->t_upload += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  P.b0 = b0; P.b1x = b1x; P.src0 = src0; P.n_src = src1 - src0;
  return BR_OK;
}

// Inflates the slot's blocks [b0, b1x) (b1x >= b1: the piece's own blocks and a few of the next piece's, for the END cut),
// splits them into records and returns the piece's bundle.
//   start_rel >= 0: the piece's first record starts that many inflated bytes behind the start of block b0 (the BAM header's
//                   size for the first piece; the END of the piece in front otherwise);  -1: guess it
//   info->start_rel / end_rel: where the bundle starts (behind block b0) and ends (behind block b1); end_rel of piece k is
//                   the start_rel of piece k + 1 -- a guessing reader's start_rel must equal its neighbour's end_rel, or the
//                   piece is to be processed again with that value
// Returns BR_PIECE_MORE (1) when the END cut lies beyond block b1x: upload more blocks and call again.
extern "C" int br_bam_piece_process(br_bam_reader *r, int slot, const br_bgzf_block *blocks, int64_t n_blocks, int64_t b1,
                                    int64_t start_rel, br_device_records *bundle, int64_t *id, br_piece_info *info) {
  if (!r || slot < 0 || slot > 1 || !blocks || !bundle || !id || !info) return BR_ERR_INVALID_ARG;
  br_bam_reader::PieceSlot &P = r->pslot[slot];
  const int64_t b0 = P.b0, b1x = P.b1x;
  if (b0 < 0 || b1 <= b0 || b1 > b1x || b1x > n_blocks) return BR_ERR_INVALID_ARG;
  memset(bundle, 0, sizeof(*bundle)); memset(info, 0, sizeof(*info));
  *id = -1;
  HIPCHK(hipSetDevice(r->shell.device));
  hipStream_t st = r->st;
  auto tp = std::chrono::steady_clock::now();
  const bool file_ends = b1x == n_blocks, last_piece = b1 == n_blocks;
  const uint64_t dst0 = blocks[b0].dst_off;
  const uint64_t total = blocks[b1x - 1].dst_off + blocks[b1x - 1].ulen - dst0;
  const uint64_t bound = last_piece ? total : blocks[b1].dst_off - dst0;   // where the next piece's first block starts
  r->pblocks.assign(blocks + b0, blocks + b1x);
  for (auto &b : r->pblocks) { b.src_off -= P.src0; b.dst_off -= dst0; }
  br_bam_reader::Chunk *ch = nullptr;
  {
    std::lock_guard<std::mutex> l(r->m);
    for (auto &x : r->chunks) if (!x->out) { ch = x.get(); break; }
    if (!ch) { r->chunks.push_back(std::make_unique<br_bam_reader::Chunk>()); ch = r->chunks.back().get(); }
  }
  RC(ch->data.ensure((size_t)total + 64));
  HIPCHK(hipStreamWaitEvent(st, P.up, 0));
  const uint8_t *o = nullptr; uint64_t ob = 0;
  RC(inflate_impl(r->c, P.comp.as<uint8_t>(), P.n_src, r->pblocks.data(), b1x - b0, st, ch->data.as<uint8_t>(), &o, &ob));
  RC(r->small.ensure(64));
  unsigned long long *cut = (unsigned long long *)r->small.p;
  uint64_t start = 0;
  const int guess = start_rel < 0 ? 1 : 0;
  if (guess) {   // the first offset that starts a run of records
    SplitArgs G{}; G.data = ch->data.as<uint8_t>(); G.n_bytes = total; G.n_ref = r->n_ref;
    launch_first_record(st, G, total, cut);
    unsigned long long e = 0;
    HIPCHK(hipMemcpyAsync(&e, cut, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (e == ~0ull) { if (file_ends) e = total; else return 1; }   // no record starts in here (one long record): more blocks
    start = e;
  } else {
    if ((uint64_t)start_rel > total) return file_ends ? BR_ERR_INVALID_ARG : 1;
    start = (uint64_t)start_rel;
  }
  const uint8_t *base = ch->data.as<uint8_t>() + start;
  const uint64_t nbytes = total - start;
  br_device_records recs; int64_t unm_all = 0; uint64_t used_bytes = 0; SplitArgs S{};
  RC(split_impl(r->c, base, nbytes, r->n_ref, st, &recs, &unm_all, &used_bytes, &S));
  if (file_ends && used_bytes != nbytes) return BR_ERR_INVALID_ARG;   // a truncated record at the end of the file
  const int64_t n = recs.n_aln;
  // the two cuts (see split_kernels.hip), their offsets, the unmapped records between: one read-back
  const unsigned long long init[5] = {guess ? (unsigned long long)n : 0ull, ~0ull, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(cut, init, sizeof(init), hipMemcpyHostToDevice, st));
  const uint64_t bound_rel = bound > start ? bound - start : 0;   // (relative to base)
  launch_piece_cut(st, S, recs.rec_off, n, last_piece ? ~0ull : bound_rel, used_bytes, guess, cut);
  unsigned long long h[5];
  HIPCHK(hipMemcpyAsync(h, cut, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int64_t iS = (int64_t)std::min<unsigned long long>(h[0], (unsigned long long)n), iE = n;
  if (!last_piece) {
    if (h[1] == ~0ull) { if (!file_ends) return 1; }   // the group at the boundary goes on past the data: more blocks (or the file ends: all of it)
    else iE = (int64_t)h[1];
  }
  if (iS > iE) iS = iE;   // (a read-name group that covers the whole piece and more: the piece in front takes it all)
  const uint64_t off_S = h[2], off_E = std::max<uint64_t>(h[3], h[2]);
  const int64_t n_take = iE - iS;
  if (n_take) {
    RC(ch->off.ensure((size_t)n_take * 8)); RC(ch->len.ensure((size_t)n_take * 4));
    HIPCHK(hipMemcpyAsync(ch->off.p, recs.rec_off + iS, (size_t)n_take * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(ch->len.p, recs.rec_len + iS, (size_t)n_take * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  { std::lock_guard<std::mutex> l(r->m); ch->id = r->next_id++; ch->out = true; }
  bundle->blob = base; bundle->rec_off = ch->off.as<uint64_t>(); bundle->rec_len = ch->len.as<uint32_t>(); bundle->n_aln = n_take;
  *id = ch->id;
  info->start_rel = start + off_S;
  info->end_rel = start + off_E >= bound ? start + off_E - bound : 0;
  info->n_unmapped = (int64_t)h[4];
  info->guessed = guess; info->at_end = last_piece ? 1 : 0;
  r->t_proc += std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
  return BR_OK;
}
extern "C" double br_bam_reader_seconds(const br_bam_reader *r) { return r ? r->t_proc : 0.0; }
extern "C" double br_bam_reader_upload_seconds(const br_bam_reader *r) { return r ? r->t_upload : 0.0; }

extern "C" int br_bam_split(const uint8_t *data, uint64_t n_bytes, int64_t cap, uint64_t *rec_off, uint32_t *rec_len,
                            int64_t *n_records, int64_t *n_unmapped, uint64_t *consumed) {
  if ((!data && n_bytes) || !rec_off || !rec_len || !n_records || !consumed || cap < 0) return BR_ERR_INVALID_ARG;
  uint64_t p = 0; int64_t n = 0, un = 0;
  while (n < cap && p + 4 <= n_bytes) {
    uint32_t bs; memcpy(&bs, data + p, 4);
    if (bs < 32) return BR_ERR_INVALID_ARG;
    if (p + 4 + (uint64_t)bs > n_bytes) break;  // partial record: next call
    const uint8_t *r = data + p + 4;
    uint32_t l_qname = r[8]; uint16_t ncig, flag; int32_t l_seq;
    memcpy(&ncig, r + 12, 2); memcpy(&flag, r + 14, 2); memcpy(&l_seq, r + 16, 4);
    uint64_t ls = l_seq > 0 ? (uint64_t)l_seq : 0;
    if (32ull + l_qname + 4ull * ncig + (ls + 1) / 2 + ls > bs || l_qname == 0) return BR_ERR_INVALID_ARG;
    if (flag & 0x4) un++;
    else { rec_off[n] = p + 4; rec_len[n] = bs; n++; }
    p += 4 + (uint64_t)bs;
  }
  *n_records = n; if (n_unmapped) *n_unmapped = un; *consumed = p;
  return BR_OK;
}
