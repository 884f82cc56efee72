// br_coverage_bigwig: the bigWig of a finished br_coverage, built and compressed in the device's HBM (bigwig_kernels.hip; the
// layout and the definitions are in bramble_amd.h; the host's pieces -- name order, chromosome tree, headers -- in host/bigwig_file).
//
//   chromosomes  k_bw_run_first gives every transcript's runs; the host keeps the transcripts with runs, sorts their names (strcmp)
//                and scans their run, section and window counts: four numbers a chromosome go up
//   full data    k_bw_sections + k_bw_pack: the sections' bytes, dense, in (chromId, start) order; k_bw_zlib, one wave a section,
//                into slots; a scan of the sizes; k_bw_gather behind the section count.  Uncompressed: one copy
//   trees        k_bw_tree_reduce level by level (the bounds), k_bw_tree_nodes per level (root level first in the file); the 48-byte
//                header from the host with the root's bounds
//   zoom level   k_bw_zoom_windows over every window of the level (a record and a flag each), a scan of the flags,
//                k_bw_zoom_compact; blocks of S records through the same zlib / gather / tree path
//   total        k_bw_total's 256 partials, summed on the host in order
//   image        the parts lie in buffers of their own until the last size is known (the offsets are absolute); then the image is
//                made, the parts copied in and dropped
//
// Device memory (C chromosomes, R runs, N = ceil-sum of R / S sections, image I bytes; all of it in the object's account):
//   held         I, from the call's return until the next call or br_coverage_free
//   while it runs  8 (T + 2) (first runs; freed before the data), 28 (C + 1) (chromosome tables); per part of the file its bytes; for
//                the full data 24 N + 12 R + 8 (raw sections), 24 (N + 2) (offsets, bounds) and, compressed, the slots
//                (9/8 of the raw bytes + 32 N + 16) with 8 (N + 2) sizes and the scan's scratch; a tree adds 16 a node above the
//                leaves; a zoom level 40 a window (records and flags, freed after the compaction), 32 a record, 24 a block, and
//                its slots; at the end the image beside its parts: the peak is about 2 I + the largest of these
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "accum.h"
#include "bigwig_kernels.h"
#include "coverage_view.h"
#include "host/bigwig_file.h"
#include "scan_kernels.h"

using namespace br;

struct br::BigwigState {
  ColBuf image;
  uint64_t n_bytes = 0, n_chrom = 0, n_sections = 0, raw_bytes = 0, data_bytes = 0;
  int32_t zoom_levels = 0;
  uint64_t zoom_records[10] = {};
  double seconds = 0;
};

void br::bigwig_state_free(Accum *acc, BigwigState *s) {
  if (!s) return;
  acc->drop(s->image);
  delete s;
}

namespace {

struct Opts { uint32_t S = 1024, bs = 256, R0 = 32; int Z = 4; bool compress = true; };

bool read_opts(const br_bigwig_opts *o, Opts *out) {
  Opts v;
  if (o) {
    if (o->items_per_slot > 4096 || o->block_size == 1 || o->block_size > 4096 || o->zoom_levels < -1 || o->zoom_levels > 10) return false;
    if (o->compress != 0 && o->compress != 1 && o->compress != -1) return false;
    if (o->items_per_slot) v.S = o->items_per_slot;
    if (o->block_size) v.bs = o->block_size;
    if (o->zoom_levels) v.Z = o->zoom_levels < 0 ? 0 : o->zoom_levels;
    if (o->first_reduction) v.R0 = o->first_reduction;
    v.compress = o->compress >= 0;
  }
  for (int k = 0; k < v.Z; k++) if (((uint64_t)v.R0 << (2 * k)) >= (1ull << 31)) return false;
  *out = v;
  return true;
}

// the parts of the file in order, each in a buffer of its own until the image is made
struct Builder {
  Accum *a; hipStream_t st; Opts o;
  std::vector<ColBuf> parts; std::vector<uint64_t> part_bytes;
  std::vector<ColBuf *> temps;   // tables of the call: dropped with the builder
  uint64_t pos = 0;              // the file offset behind the last part
  uint64_t raw_bytes = 0, data_bytes = 0;
  ~Builder() { for (ColBuf &p : parts) a->drop(p); for (ColBuf *t : temps) a->drop(*t); }

  int part(uint64_t bytes, uint8_t **p) {
    parts.emplace_back(); part_bytes.push_back(bytes);
    RC(a->alloc(parts.back(), (size_t)bytes + 16));
    *p = parts.back().as<uint8_t>();
    pos += bytes;
    return BR_OK;
  }
  int up(void *dst, const void *src, size_t bytes) {   // small host tables: the copy is done when it returns
    if (!bytes) return BR_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); HIPCHK(hipStreamSynchronize(st));
    return BR_OK;
  }

  // The n payloads src[off[i] .. off[i + 1]) behind a count of count_bytes bytes, as the next part.  *where (n + 1 words): item i lies
  // where[i] bytes behind the count -- off itself, or the scanned stream sizes (then off is dropped here)
  int data_part(const uint8_t *src, ColBuf &off, uint64_t n, uint64_t raw_total, uint64_t count, int count_bytes, ColBuf *where) {
    uint8_t *p = nullptr;
    raw_bytes += raw_total;
    if (!o.compress) {
      RC(part((uint64_t)count_bytes + raw_total, &p));
      RC(up(p, &count, (size_t)count_bytes));
      if (raw_total) HIPCHK(hipMemcpyAsync(p + count_bytes, src, raw_total, hipMemcpyDeviceToDevice, st));
      data_bytes += raw_total;
      *where = std::move(off);
      return BR_OK;
    }
    ColBuf slots, tmp;
    DropGuard dropper{a, {&slots, &tmp}};
    RC(a->alloc(*where, (size_t)(n + 2) * 8)); RC(a->alloc(slots, (size_t)bw_slot_off(raw_total, n) + 16)); RC(a->alloc(tmp, scan_scratch_bytes((int64_t)n + 1)));
    HIPCHK(hipMemsetAsync(where->p, 0, (size_t)(n + 2) * 8, st));
    uint64_t total = 0;
    if (n) {
      launch_bw_zlib(st, src, off.as<uint64_t>(), n, 0, slots.as<uint8_t>(), where->as<uint64_t>());
      launch_scan(st, where->as<uint64_t>(), (int64_t)n, tmp.as<uint64_t>());
      HIPCHK(hipMemcpyAsync(&total, where->as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    RC(part((uint64_t)count_bytes + total, &p));
    RC(up(p, &count, (size_t)count_bytes));
    launch_bw_gather(st, slots.as<uint8_t>(), off.as<uint64_t>(), where->as<uint64_t>(), n, p + count_bytes);
    HIPCHK(hipStreamSynchronize(st));
    data_bytes += total;
    a->drop(off);
    return BR_OK;
  }

  // the R-tree over n items (bounds lo / hi, item i at data_base + where[i]) as the next part; the indexed data ends where it begins
  int rtree(const uint64_t *lo, const uint64_t *hi, uint64_t n, const uint64_t *where, uint64_t data_base) {
    const uint64_t tree_off = pos;
    const brbw::TreeShape t = brbw::tree_shape(n, o.bs);
    uint8_t *p = nullptr;
    RC(part(brbw::RTREE_HEADER + t.bytes(32, 24), &p));
    uint64_t upper = 1;   // the bounds of the levels above the items, then the root's own
    for (size_t l = 1; l < t.items.size(); l++) upper += t.items[l];
    ColBuf bounds;
    DropGuard dropper{a, {&bounds}};
    RC(a->alloc(bounds, (size_t)upper * 16 + 16));
    HIPCHK(hipMemsetAsync(bounds.p, 0, (size_t)upper * 16 + 16, st));
    uint64_t *blo = bounds.as<uint64_t>(), *bhi = blo + upper;
    const uint64_t *llo = lo, *lhi = hi;
    uint64_t at = 0;
    for (size_t l = 0; l < t.items.size(); l++) {
      BwNodeArgs N{};
      N.lo = llo; N.hi = lhi; N.n = t.items[l]; N.bs = t.bs; N.leaf = l == 0; N.pos = where; N.data_base = data_base;
      if (l) { N.child_off = tree_off + brbw::RTREE_HEADER + t.bytes_above(l - 1, 32, 24); N.child_size = 4 + (uint64_t)t.bs * (l == 1 ? 32 : 24); }
      N.n_nodes = t.nodes(l); N.out = p + brbw::RTREE_HEADER + t.bytes_above(l, 32, 24);
      launch_bw_tree_nodes(st, N);
      launch_bw_tree_reduce(st, llo, lhi, t.items[l], t.bs, blo + at, bhi + at);   // the next level's items; the last: the root's bounds
      llo = blo + at; lhi = bhi + at; at += t.nodes(l);
    }
    uint64_t root[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&root[0], llo, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(&root[1], lhi, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const std::vector<uint8_t> head = brbw::rtree_header(t.bs, n, root[0], root[1], tree_off);
    return up(p, head.data(), head.size());
  }
};

}  // namespace

extern "C" int br_coverage_bigwig(br_coverage *c, const char *const *names, const br_bigwig_opts *opts, uint64_t *n_bytes) {
  CoverageView v{};
  ColBuf d_tid, d_run0, d_cum, d_sec0, d_win0;   // (in front of the builder, which drops them)
  Builder b{};
  RC(coverage_view(c, &v));
  if (!read_opts(opts, &b.o)) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  Accum *a = v.acc;
  hipStream_t st = a->st;
  b.a = a; b.st = st;
  const Opts &o = b.o;
  HIPCHK(hipSetDevice(a->device));
  const int64_t T = v.n_tx;
  const uint64_t R = (uint64_t)v.n_runs;

  // ---- the chromosomes: the transcripts with runs, in the order of their names
  std::vector<uint64_t> first((size_t)T + 1, 0);
  {
    ColBuf d_first;
    DropGuard dropper{a, {&d_first}};
    RC(a->alloc(d_first, (size_t)(T + 2) * 8));
    launch_bw_run_first(st, v.runs, R, T, d_first.as<uint64_t>());
    HIPCHK(hipMemcpyAsync(first.data(), d_first.p, (size_t)(T + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  std::vector<uint32_t> with_runs;
  std::vector<const char *> nm;
  for (int64_t t = 0; t < T; t++) if (first[(size_t)t + 1] > first[(size_t)t]) {
    if (!names) return BR_ERR_INVALID_ARG;
    with_runs.push_back((uint32_t)t); nm.push_back(names[t]);
  }
  std::vector<uint32_t> order;
  uint32_t key_size = 0;
  if (!brbw::name_order(nm, &order, &key_size, nullptr)) return BR_ERR_INVALID_ARG;
  const uint64_t C = with_runs.size();
  std::vector<uint32_t> tid(C + 1, 0), sizes(C);
  std::vector<const char *> sorted(C);
  std::vector<uint64_t> run0(C + 1, 0), cum(C + 1, 0), sec0(C + 1, 0), win0(C + 1, 0);
  for (uint64_t k = 0; k < C; k++) {
    const uint32_t t = with_runs[order[k]];
    const uint64_t n = first[t + 1] - first[t];
    tid[k] = t; sorted[k] = nm[order[k]]; sizes[k] = (uint32_t)((*v.off)[t + 1] - (*v.off)[t]);
    run0[k] = first[t]; cum[k + 1] = cum[k] + n; sec0[k + 1] = sec0[k] + (n + o.S - 1) / o.S;
  }
  const uint64_t N = sec0[C];

  // (from here on the call makes things: the image of an earlier call goes first)
  BigwigState *&state = *v.state;
  bigwig_state_free(a, state);
  state = nullptr;
  BigwigState *s = new BigwigState();
  struct Undo { BigwigState *s; Accum *a; ~Undo() { bigwig_state_free(a, s); } } undo{s, a};

  b.temps ={&d_tid, &d_run0, &d_cum, &d_sec0, &d_win0};
  RC(a->alloc(d_tid, (C + 1) * 4)); RC(a->alloc(d_run0, (C + 1) * 8)); RC(a->alloc(d_cum, (C + 1) * 8)); RC(a->alloc(d_sec0, (C + 1) * 8));
  RC(a->alloc(d_win0, (C + 1) * 8));
  RC(b.up(d_tid.p, tid.data(), (C + 1) * 4)); RC(b.up(d_run0.p, run0.data(), (C + 1) * 8)); RC(b.up(d_cum.p, cum.data(), (C + 1) * 8));
  RC(b.up(d_sec0.p, sec0.data(), (C + 1) * 8));

  const uint64_t head_bytes = brbw::HEADER_BYTES + brbw::ZOOM_HEADER_BYTES * (uint64_t)o.Z + brbw::SUMMARY_BYTES;
  const std::vector<uint8_t> ctree = brbw::chrom_tree(sorted, sizes, key_size, o.bs, head_bytes);
  b.pos = head_bytes + ctree.size();

  // ---- the full data and its index
  const uint64_t data_off = b.pos;
  uint64_t index_off = 0;
  {
    ColBuf raw, raw_off, lo, hi, where;
    DropGuard dropper{a, {&raw, &raw_off, &lo, &hi, &where}};
    const uint64_t raw_total = 24 * N + 12 * R;
    RC(a->alloc(raw, (size_t)raw_total + 8)); RC(a->alloc(raw_off, (size_t)(N + 2) * 8)); RC(a->alloc(lo, (size_t)(N + 1) * 8)); RC(a->alloc(hi, (size_t)(N + 1) * 8));
    HIPCHK(hipMemsetAsync(raw_off.p, 0, (size_t)(N + 2) * 8, st));
    BwPackArgs P{};
    P.runs = v.runs; P.run_depth = v.run_depth; P.n_runs = R; P.n_sec = N; P.n_chrom = C; P.S = o.S;
    P.run0 = d_run0.as<uint64_t>(); P.cum = d_cum.as<uint64_t>(); P.sec0 = d_sec0.as<uint64_t>();
    P.raw = raw.as<uint8_t>(); P.raw_off = raw_off.as<uint64_t>(); P.lo = lo.as<uint64_t>(); P.hi = hi.as<uint64_t>();
    launch_bw_sections(st, P);
    launch_bw_pack(st, P);
    RC(b.data_part(raw.as<uint8_t>(), raw_off, N, raw_total, N, 8, &where));
    index_off = b.pos;
    RC(b.rtree(lo.as<uint64_t>(), hi.as<uint64_t>(), N, where.as<uint64_t>(), data_off + 8));
  }

  // ---- the zoom levels
  std::vector<brbw::ZoomHeader> zooms;
  for (int k = 0; k < o.Z; k++) {
    const uint32_t Rk = o.R0 << (2 * k);
    for (uint64_t i = 0; i < C; i++) win0[i + 1] = win0[i] + ((uint64_t)sizes[i] + Rk - 1) / Rk;
    const uint64_t W = win0[C];
    int G = 1;
    while (G < 64 && (uint32_t)(4 * G) < Rk) G *= 2;   // a lane takes about four bases of a small window
    if (W * (uint64_t)G / 256 >= (1ull << 31)) return BR_ERR_CAPACITY;
    RC(b.up(d_win0.p, win0.data(), (C + 1) * 8));
    ColBuf zrec, boff, lo, hi, where;
    DropGuard dropper{a, {&zrec, &boff, &lo, &hi, &where}};
    uint64_t n_rec = 0;
    {
      ColBuf rec, flag, tmp;
      DropGuard dropper2{a, {&rec, &flag, &tmp}};
      RC(a->alloc(rec, (size_t)(W + 1) * 32)); RC(a->alloc(flag, (size_t)(W + 2) * 8)); RC(a->alloc(tmp, scan_scratch_bytes((int64_t)W + 1)));
      HIPCHK(hipMemsetAsync(flag.p, 0, (size_t)(W + 2) * 8, st));
      BwZoomArgs Z{};
      Z.depth = v.depth; Z.wide = v.weight != 0; Z.off = v.d_off; Z.tid = d_tid.as<uint32_t>(); Z.win0 = d_win0.as<uint64_t>();
      Z.n_chrom = C; Z.n_win = W; Z.R = Rk; Z.G = G; Z.rec = rec.as<uint4>(); Z.flag = flag.as<uint64_t>();
      launch_bw_zoom_windows(st, Z);
      if (W) {
        launch_scan(st, flag.as<uint64_t>(), (int64_t)W, tmp.as<uint64_t>());
        HIPCHK(hipMemcpyAsync(&n_rec, flag.as<uint64_t>() + W, 8, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipStreamSynchronize(st));
      if (n_rec > 0xffffffffull) return BR_ERR_CAPACITY;   // (recordCount is 32-bit)
      RC(a->alloc(zrec, (size_t)(n_rec + 1) * 32));
      launch_bw_zoom_compact(st, rec.as<uint4>(), flag.as<uint64_t>(), W, zrec.as<uint4>());
      HIPCHK(hipStreamSynchronize(st));
    }
    const uint64_t n_blocks = (n_rec + o.S - 1) / o.S;
    RC(a->alloc(boff, (size_t)(n_blocks + 2) * 8)); RC(a->alloc(lo, (size_t)(n_blocks + 1) * 8)); RC(a->alloc(hi, (size_t)(n_blocks + 1) * 8));
    launch_bw_zoom_blocks(st, zrec.as<uint4>(), n_rec, o.S, n_blocks, boff.as<uint64_t>(), lo.as<uint64_t>(), hi.as<uint64_t>());
    brbw::ZoomHeader zh{Rk, b.pos, 0};
    RC(b.data_part(zrec.as<uint8_t>(), boff, n_blocks, 32 * n_rec, n_rec, 4, &where));
    zh.index_off = b.pos;
    RC(b.rtree(lo.as<uint64_t>(), hi.as<uint64_t>(), n_blocks, where.as<uint64_t>(), zh.data_off + 4));
    zooms.push_back(zh);
    s->zoom_records[k] = n_rec;
  }

  // ---- the total summary, the head of the file, the image
  brbw::Summary total{0, 0, 0, 0, 0};
  if (R) {
    ColBuf partial;
    DropGuard dropper{a, {&partial}};
    std::vector<uint64_t> h(5 * BW_TOTAL_BLOCKS);
    RC(a->alloc(partial, h.size() * 8));
    launch_bw_total(st, v.runs, v.run_depth, R, partial.as<uint64_t>());
    HIPCHK(hipMemcpyAsync(h.data(), partial.p, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t mn = ~0ull, mx = 0;
    for (unsigned k = 0; k < BW_TOTAL_BLOCKS; k++) {
      double sum, sq;
      memcpy(&sum, &h[5 * k + 3], 8); memcpy(&sq, &h[5 * k + 4], 8);
      total.valid += h[5 * k]; mn = std::min(mn, h[5 * k + 1]); mx = std::max(mx, h[5 * k + 2]); total.sum += sum; total.sum_squares += sq;
    }
    const double unit = v.weight ? 1.0 / 4294967296.0 : 1.0;
    total.min_val = (double)mn * unit; total.max_val = (double)mx * unit;
  }
  const uint32_t ubuf = o.compress ? std::max<uint32_t>(24 + 12 * o.S, 32 * o.S) : 0;
  std::vector<uint8_t> head = brbw::file_head(zooms, head_bytes, data_off, index_off, ubuf, total);
  head.insert(head.end(), ctree.begin(), ctree.end());
  const uint32_t magic = brbw::BIGWIG_MAGIC;
  const uint64_t I = b.pos + 4;
  RC(a->alloc(s->image, (size_t)I));
  uint8_t *img = s->image.as<uint8_t>();
  RC(b.up(img, head.data(), head.size()));
  uint64_t at = head.size();
  for (size_t k = 0; k < b.parts.size(); k++) {
    if (b.part_bytes[k]) HIPCHK(hipMemcpyAsync(img + at, b.parts[k].p, b.part_bytes[k], hipMemcpyDeviceToDevice, st));
    at += b.part_bytes[k];
  }
  RC(b.up(img + at, &magic, 4));
  HIPCHK(hipStreamSynchronize(st));
  s->n_bytes = I; s->n_chrom = C; s->n_sections = N; s->raw_bytes = b.raw_bytes; s->data_bytes = b.data_bytes; s->zoom_levels = o.Z;
  s->seconds = timer.seconds();
  state = s; undo.s = nullptr;
  if (n_bytes) *n_bytes = I;
  return BR_OK;
}

extern "C" int br_coverage_bigwig_read(br_coverage *c, uint64_t off, uint64_t n, uint8_t *dst) {
  CoverageView v{};
  RC(coverage_view(c, &v));
  const BigwigState *s = *v.state;
  if (!s || off > s->n_bytes || n > s->n_bytes - off || (n && !dst)) return BR_ERR_INVALID_ARG;
  if (!n) return BR_OK;
  HIPCHK(hipSetDevice(v.acc->device));
  HIPCHK(hipMemcpyAsync(dst, s->image.as<uint8_t>() + off, (size_t)n, hipMemcpyDeviceToHost, v.acc->st));
  HIPCHK(hipStreamSynchronize(v.acc->st));
  return BR_OK;
}

extern "C" int br_coverage_bigwig_stats(const br_coverage *c, uint64_t *n_chromosomes, uint64_t *n_sections, int32_t *zoom_levels,
                                        uint64_t *zoom_records, uint64_t *raw_bytes, uint64_t *data_bytes, uint64_t *n_bytes, double *seconds) {
  CoverageView v{};
  RC(coverage_view(const_cast<br_coverage *>(c), &v));
  const BigwigState *s = *v.state;
  if (!s) return BR_ERR_INVALID_ARG;
  if (n_chromosomes) *n_chromosomes = s->n_chrom;
  if (n_sections) *n_sections = s->n_sections;
  if (zoom_levels) *zoom_levels = s->zoom_levels;
  if (zoom_records) for (int k = 0; k < 10; k++) zoom_records[k] = s->zoom_records[k];
  if (raw_bytes) *raw_bytes = s->raw_bytes;
  if (data_bytes) *data_bytes = s->data_bytes;
  if (n_bytes) *n_bytes = s->n_bytes;
  if (seconds) *seconds = s->seconds;
  return BR_OK;
}

extern "C" int br_zlib_sections_device(int device, const uint8_t *src, const uint64_t *off, int64_t n, int mode, uint8_t **out, uint64_t *out_off) {
  if (!out || !out_off || n < 0 || (n && !off) || (mode != 0 && mode != 1)) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  for (int64_t i = 0; i < n; i++) if (off[i + 1] < off[i] || off[i + 1] - off[i] > BW_MAX_PAYLOAD) return BR_ERR_INVALID_ARG;
  const uint64_t lo = n ? off[0] : 0, total = n ? off[n] - lo : 0;
  if (total && !src) return BR_ERR_INVALID_ARG;
  Accum a;
  RC(a.open(device));
  struct Close { Accum *a; ~Close() { a->close(); } } closer{&a};
  ColBuf d_src, d_off, slots, sizes, tmp, dense;
  DropGuard dropper{&a, {&d_src, &d_off, &slots, &sizes, &tmp, &dense}};
  std::vector<uint64_t> rel((size_t)n + 1, 0);
  for (int64_t i = 0; i <= n && n; i++) rel[(size_t)i] = off[i] - lo;
  RC(a.alloc(d_src, (size_t)total + 8)); RC(a.alloc(d_off, (size_t)(n + 2) * 8)); RC(a.alloc(slots, (size_t)bw_slot_off(total, (uint64_t)n) + 16));
  RC(a.alloc(sizes, (size_t)(n + 2) * 8)); RC(a.alloc(tmp, scan_scratch_bytes(n + 1)));
  hipStream_t st = a.st;
  if (total) HIPCHK(hipMemcpyAsync(d_src.p, src + lo, (size_t)total, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_off.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(sizes.p, 0, (size_t)(n + 2) * 8, st));
  std::vector<uint64_t> where((size_t)n + 1, 0);
  if (n) {
    launch_bw_zlib(st, d_src.as<uint8_t>(), d_off.as<uint64_t>(), (uint64_t)n, mode, slots.as<uint8_t>(), sizes.as<uint64_t>());
    launch_scan(st, sizes.as<uint64_t>(), n, tmp.as<uint64_t>());
    HIPCHK(hipMemcpyAsync(where.data(), sizes.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t bytes = where[(size_t)n];
  uint8_t *h = (uint8_t *)malloc((size_t)bytes + 1);
  if (!h) return BR_ERR_CAPACITY;
  if (bytes) {
    int rc = a.alloc(dense, (size_t)bytes);
    if (!rc) {
      launch_bw_gather(st, slots.as<uint8_t>(), d_off.as<uint64_t>(), sizes.as<uint64_t>(), (uint64_t)n, dense.as<uint8_t>());
      if (hipMemcpyAsync(h, dense.p, (size_t)bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = BR_ERR_HIP;
    }
    if (rc) { free(h); return rc; }
  }
  memcpy(out_off, where.data(), (size_t)(n + 1) * 8);
  *out = h;
  return BR_OK;
}
