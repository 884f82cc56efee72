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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "accum.h"
#include "coverage_kernels.h"
#include "ctx.h"
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
  uint64_t counters[CV_WORDS] = {};
  double add_s = 0, finish_s = 0;
  ColBuf d_off, diff, records, small, aligned, covered, max_depth, runs;
};

extern "C" void br_coverage_free(br_coverage *c) {
  if (!c) return;
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

extern "C" int br_coverage_set_param(br_coverage *c, const char *name, int64_t value) {
  if (!c || !name || c->broken || c->finished || c->added) return BR_ERR_INVALID_ARG;   // (what the adds counted depends on it)
  if (!strcmp(name, "primary_only")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->primary_only = (int)value; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

// the rows [r0, r1) through the kernel; A: a, cigar, bias, pool and n_pool_words are set
static int coverage_add_rows(br_coverage *c, CovAddArgs A, uint64_t r0, uint64_t r1) {
  hipStream_t st = c->st;
  A.r_first = r0; A.r_last = r1;
  A.n_tx = c->n_tx; A.off = c->d_off.as<uint64_t>(); A.primary_only = (uint32_t)c->primary_only;
  A.diff = c->diff.as<uint32_t>(); A.records = c->records.as<unsigned long long>(); A.counters = c->small.as<unsigned long long>();
  launch_cov_add(st, A);
  HIPCHK(hipMemcpyAsync(c->counters, c->small.p, CV_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's rows may be reused now
  c->rows += r1 - r0;
  if (c->counters[CV_BAD_POOL]) { c->broken = true; return BR_ERR_INVALID_ARG; }   // a CIGAR reference that leaves the pool
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
  if (!c || !rows || c->broken || c->finished) return BR_ERR_INVALID_ARG;
  if (r0 < 0 || r1 < r0 || rows->n_rows < 0 || r1 > rows->n_rows || rows->n_pool_words < 0) { c->broken = true; return BR_ERR_INVALID_ARG; }
  if (r1 > r0 && (!rows->a || !rows->cigar || (rows->n_pool_words && !rows->pool))) return BR_ERR_INVALID_ARG;
  if (c->rows + (uint64_t)(r1 - r0) >= (1ull << 32)) return BR_ERR_CAPACITY;   // (the depth is 32-bit)
  c->added = true;
  if (r1 == r0) return BR_OK;
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  return on_device ? coverage_add_device(c, *rows, (uint64_t)r0, (uint64_t)r1, (hipStream_t)stream) : coverage_add_host(c, *rows, (uint64_t)r0, (uint64_t)r1);
}

extern "C" int br_coverage_add_last(br_coverage *c, br_ctx *ctx) {
  if (!c || !ctx || !ctx->ix || ctx->ix->device != c->device || c->broken || c->finished) return BR_ERR_INVALID_ARG;
  if (!ctx->last_rows.row_off || ctx->last_rows.n_rows == 0) { c->added = true; return BR_OK; }   // a call without rows
  return br_coverage_add_rows(c, &ctx->last_rows, 0, ctx->last_rows.n_rows, 1, ctx->last_stream);
}

static int coverage_finish(br_coverage *c) {
  hipStream_t st = c->st;
  const int64_t B = c->n_bases, T = c->n_tx;
  if (c->counters[CV_BAD_TID]) return BR_ERR_INVALID_ARG;   // a transcript id the object has no transcript for
  const size_t t1 = (size_t)T + 1;
  const int64_t tiles = (B + COV_TILE - 1) / COV_TILE;
  ColBuf tile, tmp;
  DropGuard dropper{c, {&tile, &tmp}};
  RC(c->alloc(c->aligned, t1 * 8)); RC(c->alloc(c->covered, t1 * 8)); RC(c->alloc(c->max_depth, t1 * 4));
  RC(c->alloc(tile, (size_t)(tiles + 2) * 8)); RC(c->alloc(tmp, scan_scratch_bytes(tiles)));
  HIPCHK(hipMemsetAsync(c->aligned.p, 0, t1 * 8, st)); HIPCHK(hipMemsetAsync(c->covered.p, 0, t1 * 8, st));
  HIPCHK(hipMemsetAsync(c->max_depth.p, 0, t1 * 4, st));
  uint32_t *depth = c->diff.as<uint32_t>();
  const uint64_t *off = c->d_off.as<uint64_t>();
  launch_cov_scan(st, depth, B, tile.as<uint64_t>(), tmp.as<uint64_t>());
  if (B > 0) launch_cov_summary(st, depth, off, T, c->aligned.as<uint64_t>(), c->covered.as<uint64_t>(), c->max_depth.as<uint32_t>());
  uint64_t R = 0;
  if (B > 0) {
    launch_cov_count(st, depth, B, off, T, tile.as<uint64_t>());
    launch_scan(st, tile.as<uint64_t>(), tiles, tmp.as<uint64_t>());   // tile counts -> the first run of every tile; [tiles] = R
    HIPCHK(hipMemcpyAsync(&R, tile.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (R > (uint64_t)B) return BR_ERR_HIP;
  RC(c->alloc(c->runs, (size_t)(R + 1) * 16));
  if (R) launch_cov_runs(st, depth, B, off, T, tile.as<uint64_t>(), c->runs.as<uint4>());
  HIPCHK(hipStreamSynchronize(st));
  c->n_runs = (int64_t)R;
  return BR_OK;
}

extern "C" int br_coverage_finish(br_coverage *c, int64_t *n_runs) {
  if (!c || c->broken || c->finished) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  const int rc = coverage_finish(c);
  if (rc) { if (rc != BR_ERR_INVALID_ARG) c->broken = true; return rc; }   // (diff may be half a depth by now)
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_runs) *n_runs = c->n_runs;
  return BR_OK;
}

extern "C" int br_coverage_runs(br_coverage *c, int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
  if (!c || c->broken || !c->finished || first < 0 || n < 0 || first > c->n_runs || n > c->n_runs - first) return BR_ERR_INVALID_ARG;
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
  if (!c || c->broken || !c->finished || tid < 0 || tid >= c->n_tx) return BR_ERR_INVALID_ARG;
  const uint64_t b = c->off[(size_t)tid], len = c->off[(size_t)tid + 1] - b;
  if (!depth || !len) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(depth, c->diff.as<uint32_t>() + b, (size_t)len * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_coverage_summary(br_coverage *c, uint64_t *records, uint64_t *aligned_bases, uint64_t *covered_bases, uint32_t *max_depth) {
  if (!c || c->broken || !c->finished) return BR_ERR_INVALID_ARG;
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
