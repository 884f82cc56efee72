// The unprojected records: every input record of a bundle call (br_project_bam_device and the entry points above it) that
// no emitted row came from, kept byte for byte in the context's HBM until the caller draws them (unprojected_kernels.hip).
//
//   measure  (in front of the wait for the encoder's size) mark: a flag per input alignment from the detail column the
//            encoder reads; names: flagged alignments per read-name group -> the two name counters, and in scope name the
//            flags of every group that has one; sizes: 4 + block_size and 1 per unprojected record, two scans -> offsets and
//            ranks; the totals ride home with the encoder's own read-back
//   gather   (beside the encoder) the arena and its offset table take the new records.  The arena grows by half, the old
//            one beside the new while its bytes are copied; the old one is freed behind the call's last synchronise, so a
//            growing call waits for nothing either
//   commit   (behind that synchronise) the counters
//   next     the arena is the stream in input order already: a piece is a slice of it (k_sort_cut finds the cut) and its
//            offsets rebased (k_sort_offs)
//
// Device memory: the held bytes + 8 bytes a record (+ the same again while growing); per call 17 bytes an input alignment.
#include <algorithm>
#include <cstring>

#include "ctx.h"
#include "scan_kernels.h"
#include "sort_kernels.h"

// b holds at least `bytes`, with what it held: the new buffer is made beside the old one, which moves to `old` (to be freed
// once the stream is through with the copy).  Memory that is not there is BR_ERR_CAPACITY
static int unproj_grow(Unprojected &u, ColBuf &b, ColBuf &old, size_t bytes, size_t keep_bytes, hipStream_t st) {
  if (bytes <= b.cap) return BR_OK;
  void *q = nullptr;
  const hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? BR_ERR_CAPACITY : BR_ERR_HIP; }
  u.live += bytes; u.peak = std::max(u.peak, u.live);
  if (b.p && keep_bytes) {
    if (hipMemcpyAsync(q, b.p, keep_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) { (void)hipFree(q); u.live -= bytes; return BR_ERR_HIP; }
  }
  if (old.p) u.drop(old);   // (left by a call that failed: hipFree waits for the device)
  std::swap(old, b);
  b.p = q; b.cap = bytes;
  return BR_OK;
}

int unproj_measure(br_ctx *c, hipStream_t st, Prof &pf, const BamArgs &B, const uint32_t *group_off, int64_t n_groups, UnprojArgs &U) {
  Unprojected &u = c->un;
  const size_t n = (size_t)B.n_aln;
  if (u.old_arena.p) u.drop(u.old_arena);
  if (u.old_off.p) u.drop(u.old_off);
  RC(u.flag.ensure(n)); RC(u.len.ensure(n * 4)); RC(u.one.ensure(n * 4)); RC(u.out_off.ensure((n + 1) * 8)); RC(u.rank.ensure((n + 1) * 4));
  RC(u.small.ensure(UNPROJ_SMALL_N * 8));
  U = UnprojArgs{};
  U.n_aln = B.n_aln; U.n_rows = B.n_rows; U.n_groups = n_groups;
  U.blob = B.blob; U.rec_off = B.rec_off; U.rec_len = B.rec_len; U.r_rec = B.r_rec; U.rec_x = B.rec_x;
  U.group_off = group_off; U.scope = u.keep;
  U.flag = u.flag.as<uint8_t>(); U.small = u.small.as<uint64_t>(); U.len = u.len.as<uint32_t>(); U.one = u.one.as<uint32_t>();
  U.out_off = u.out_off.as<uint64_t>(); U.rank = u.rank.as<uint32_t>();
  HIPCHK(hipMemsetAsync(U.flag, 0, n, st));
  HIPCHK(hipMemsetAsync(U.small, 0, UNPROJ_SMALL_N * 8, st));
  RC(pf.begin(BR_K_BAM));
  launch_unproj_mark(st, U);
  launch_unproj_names(st, U);
  launch_unproj_size(st, U);
  RC(pf.end());
  RC(pf.begin(BR_K_SCAN));   // (tile_sums holds a scan of n_aln + 1 items: br_project_bam_device sized it)
  launch_scan(st, U.len, B.n_aln, c->tile_sums.as<uint64_t>(), u.out_off.p, true, U.small + UNPROJ_BYTES);
  launch_scan(st, U.one, B.n_aln, c->tile_sums.as<uint64_t>(), u.rank.p, false, U.small + UNPROJ_RECORDS);
  RC(pf.end());
  HIPCHK(hipMemcpyAsync(c->rb->unproj, U.small, UNPROJ_SMALL_N * 8, hipMemcpyDeviceToHost, st));
  return BR_OK;
}

int unproj_gather(br_ctx *c, hipStream_t st, Prof &pf, UnprojArgs &U) {
  Unprojected &u = c->un;
  U.new_bytes = c->rb->unproj[UNPROJ_BYTES]; U.n_new = c->rb->unproj[UNPROJ_RECORDS];
  if (U.n_new == 0) return BR_OK;
  const uint64_t need = u.used + U.new_bytes + 64;
  if (need > u.arena.cap)
    RC(unproj_grow(u, u.arena, u.old_arena, (size_t)std::max<uint64_t>({need, u.arena.cap + u.arena.cap / 2, u.arena.cap ? 0 : u.first_cap}), (size_t)u.used, st));
  const size_t rows = (size_t)u.n + (size_t)U.n_new + 1;
  if (rows * 8 > u.off.cap) RC(unproj_grow(u, u.off, u.old_off, std::max(rows, (size_t)(u.off.cap / 8) * 3 / 2) * 8, ((size_t)u.n + 1) * 8, st));
  U.arena = u.arena.as<uint8_t>(); U.arena_base = u.used; U.off = u.off.as<uint64_t>() + u.n;
  // 200-byte records are 25 destination words: 16 lanes each; the long reads' kilobytes take a wave
  const uint64_t mean = U.new_bytes / U.n_new;
  RC(pf.begin(BR_K_BAM));
  launch_unproj_gather(st, U, mean >= 4096 ? 64 : mean >= 512 ? 32 : 16, c->n_cu);
  RC(pf.end());
  return BR_OK;
}

void unproj_commit(br_ctx *c, const UnprojArgs &U) {
  Unprojected &u = c->un;
  if (u.old_arena.p) u.drop(u.old_arena);
  if (u.old_off.p) u.drop(u.old_off);
  u.used += U.new_bytes; u.n += (int64_t)U.n_new;
  u.stats[0] += (uint64_t)U.n_aln; u.stats[1] += U.n_new; u.stats[2] += U.new_bytes;
  u.stats[3] += (uint64_t)U.n_groups; u.stats[4] += c->rb->unproj[UNPROJ_NAMES_NONE]; u.stats[5] += c->rb->unproj[UNPROJ_NAMES_PART];
}

extern "C" int br_ctx_unprojected_stats(const br_ctx *c, uint64_t out[8]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  memcpy(out, c->un.stats, sizeof(c->un.stats));
  out[6] = c->un.live; out[7] = c->un.peak;
  return BR_OK;
}

extern "C" int br_ctx_unprojected_next(br_ctx *c, uint64_t max_bytes, br_device_bam *piece) {
  if (!c || !piece) return BR_ERR_INVALID_ARG;
  memset(piece, 0, sizeof(*piece));
  Unprojected &u = c->un;
  if (u.cur >= u.n) return BR_OK;
  HIPCHK(hipSetDevice(c->ix->device));
  hipStream_t st = nullptr;
  RC(u.small.ensure(UNPROJ_SMALL_N * 8));
  uint64_t *res = u.small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(res + 2, 0, 8, st));
  launch_sort_cut(st, u.off.as<uint64_t>(), u.n, u.cur, max_bytes, res);
  uint64_t cut[2] = {0, 0}, begin = 0;
  HIPCHK(hipMemcpyAsync(cut, res, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&begin, u.off.as<uint64_t>() + u.cur, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t e = (int64_t)cut[0];
  if (e <= u.cur || e > u.n || begin + cut[1] > u.used) return BR_ERR_HIP;
  const int64_t m = e - u.cur;
  RC(u.piece_rows.ensure((size_t)(m + 1) * 8));
  launch_sort_offs(st, u.off.as<uint64_t>() + u.cur, m, 0, u.piece_rows.as<uint64_t>(), (uint32_t *)(res + 2));
  HIPCHK(hipStreamSynchronize(st));
  piece->data = u.arena.as<uint8_t>() + begin; piece->n_bytes = cut[1]; piece->row_off = u.piece_rows.as<uint64_t>(); piece->n_rows = m;
  u.cur = e;
  return BR_OK;
}

extern "C" int br_ctx_unprojected_reset(br_ctx *c) {
  if (!c) return BR_ERR_INVALID_ARG;
  Unprojected &u = c->un;
  if (u.arena.p || u.off.p || u.old_arena.p || u.old_off.p) {
    HIPCHK(hipSetDevice(c->ix->device));
    u.drop(u.arena); u.drop(u.off); u.drop(u.old_arena); u.drop(u.old_off);
  }
  u.used = 0; u.n = 0; u.cur = 0; u.live = 0; u.peak = 0;
  memset(u.stats, 0, sizeof(u.stats));
  return BR_OK;
}
