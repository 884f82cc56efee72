// br_sam_reader: SAM text in (host memory), bundles of device-resident BAM records of whole read-name groups out -- the SAM
// counterpart of br_bam_reader (reader.cpp).  The reference reads SAM through htslib like BAM (GSamReader -> hts_open,
// gclib/GSam.h:371; BamIO::start, include/bramble.h:45): every line becomes the bam1_t that sam_parse1 builds.  Here the text
// goes up as it is and sam_kernels.hip makes the records where br_project_bam_resident needs them.
//
//   upload     br_sam_reader_upload, on a copy stream of its own into device text slot 0 / 1 (one chunk ahead of the parse when
//              the caller uploads from another thread): two pinned 8 MB buffers, the host fills one while the other crosses PCIe
//   line index k_sam_nl_count -> scan -> k_sam_nl_write
//   measure    k_sam_measure (fields, CIGAR, tags -> block_size, verdict, error), two scans (record index, byte offset)
//   emit       k_sam_emit into the chunk's own buffers; floats off the device's exact path are patched with strtod
//   cut        k_last_group (split_kernels.hip) on the records made: the last read-name group waits for the next call
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bramble_amd.h"
#include "devmem.h"
#include "kernels.h"
#include "sam_header.h"
#include "sam_kernels.h"

using namespace br;

namespace {

const char *sam_reason(int e) {
  switch (e) {
    case SAM_E_EMPTY: return "empty line";
    case SAM_E_FIELDS: return "fewer than 11 fields";
    case SAM_E_QNAME: return "QNAME is empty or longer than 254 characters";
    case SAM_E_FLAG: return "FLAG is not a number in 0..65535";
    case SAM_E_POS: return "POS is not a number in 0..2147483647";
    case SAM_E_MAPQ: return "MAPQ is not a number in 0..255";
    case SAM_E_CIGAR: return "malformed CIGAR (ops are <length><one of MIDNSHP=X>)";
    case SAM_E_PNEXT: return "PNEXT is not a number in 0..2147483647";
    case SAM_E_TLEN: return "TLEN is not a 32-bit number";
    case SAM_E_SEQ_CIGAR: return "SEQ length differs from the CIGAR's query length";
    case SAM_E_QUAL_SEQ: return "QUAL length differs from the SEQ length";
    case SAM_E_TAG: return "malformed tag";
    case SAM_E_TAG_RANGE: return "tag value out of range";
    case SAM_E_TOO_LONG: return "record too long for BAM";
    case SAM_E_FLOAT: return "malformed float tag value";
    default: return "malformed line";
  }
}

}  // namespace

struct br_sam_reader {
  int device = 0;
  hipStream_t st = nullptr;
  int32_t n_ref = 0;
  uint32_t h_mask = 0;
  DevBuf h_slot, name_off, names;
  DevBuf text[2], tile, tmp, lend, line, mapped, bytes, small, fix;
  uint64_t text_n[2] = {0, 0};
  hipStream_t up_st = nullptr;
  hipEvent_t up_done[2] = {nullptr, nullptr}, up_t[2] = {nullptr, nullptr};
  std::mutex stat_m;
  uint32_t fix_cap = 4096;
  struct Chunk { DevBuf blob, off, len, rline; int64_t id = -1; bool out = false; };
  std::vector<std::unique_ptr<Chunk>> chunks;
  std::mutex m;
  static constexpr size_t PIN_BYTES = 8u << 20;
  uint8_t *pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_used[2] = {false, false};
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // (unused), parse start, parse end
  uint64_t last_nl = 0;                              // lend entry of a last line without '\n' (source of an async copy)
  int64_t line_base = 0, next_id = 0, n_chunks = 0;
  uint64_t n_bytes_in = 0;
  double upload_s = 0, parse_s = 0;
  std::string err;
};

static int sam_check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return BR_ERR_NO_DEVICE; }
  return BR_OK;
}

extern "C" int br_sam_header_scan(const uint8_t *data, uint64_t n, uint64_t *header_bytes) {
  if ((!data && n) || !header_bytes) return BR_ERR_INVALID_ARG;
  uint64_t p = 0;
  while (p < n && data[p] == '@') {
    const uint8_t *q = (const uint8_t *)memchr(data + p, '\n', (size_t)(n - p));
    p = q ? (uint64_t)(q - data) + 1 : n;
  }
  *header_bytes = p;
  return BR_OK;
}

extern "C" void br_sam_reader_free(br_sam_reader *r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->st) (void)hipStreamSynchronize(r->st);
  if (r->up_st) (void)hipStreamSynchronize(r->up_st);
  for (int k = 0; k < 2; k++) { if (r->pin[k]) (void)hipHostFree(r->pin[k]); if (r->pin_ev[k]) (void)hipEventDestroy(r->pin_ev[k]); }
  for (auto &e : r->ev) if (e) (void)hipEventDestroy(e);
  for (int k = 0; k < 2; k++) { if (r->up_done[k]) (void)hipEventDestroy(r->up_done[k]); if (r->up_t[k]) (void)hipEventDestroy(r->up_t[k]); }
  if (r->up_st) (void)hipStreamDestroy(r->up_st);
  if (r->st) (void)hipStreamDestroy(r->st);
  delete r;
}

static int sam_reader_init(br_sam_reader *r, const char *header_text, uint64_t header_len) {
  std::vector<std::string> names;
  std::vector<uint32_t> lens;
  if (!sam_header_refs(header_text, (size_t)header_len, names, lens)) return BR_ERR_INVALID_ARG;
  r->n_ref = (int32_t)names.size();
  uint32_t sz = 2;
  while (sz < 2 * names.size() + 2) sz <<= 1;
  r->h_mask = sz - 1;
  std::vector<int32_t> slot(sz, -1);
  std::vector<uint64_t> off(names.size() + 1, 0);
  std::string blob;
  for (size_t i = 0; i < names.size(); i++) {
    off[i] = blob.size(); blob += names[i];
    uint64_t h = 1469598103934665603ull;   // FNV-1a, as ref_lookup in sam_kernels.hip
    for (unsigned char c : names[i]) { h ^= c; h *= 1099511628211ull; }
    bool dup = false;
    uint32_t k = (uint32_t)h & r->h_mask;
    for (; slot[k] >= 0; k = (k + 1) & r->h_mask) if (names[(size_t)slot[k]] == names[i]) { dup = true; break; }
    if (!dup) slot[k] = (int32_t)i;   // (a repeated name resolves to its first @SQ line)
  }
  off[names.size()] = blob.size();
  RC(r->h_slot.ensure(sz * 4)); RC(r->name_off.ensure(off.size() * 8)); RC(r->names.ensure(blob.size() + 1));
  HIPCHK(hipMemcpy(r->h_slot.p, slot.data(), sz * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r->name_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  if (!blob.empty()) HIPCHK(hipMemcpy(r->names.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
  HIPCHK(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&r->up_st, hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) {
    HIPCHK(hipEventCreateWithFlags(&r->up_done[k], hipEventDisableTiming));
    HIPCHK(hipEventCreate(&r->up_t[k]));
  }
  for (int k = 0; k < 2; k++) {
    HIPCHK(hipHostMalloc((void **)&r->pin[k], br_sam_reader::PIN_BYTES, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&r->pin_ev[k], hipEventDisableTiming));
  }
  for (auto &e : r->ev) HIPCHK(hipEventCreate(&e));
  RC(r->small.ensure(64));
  return BR_OK;
}

extern "C" int br_sam_reader_new(int device, const char *header_text, uint64_t header_len, br_sam_reader **out) {
  if (!out || (!header_text && header_len)) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  RC(sam_check_device(device));
  HIPCHK(hipSetDevice(device));
  br_sam_reader *r = new br_sam_reader();
  r->device = device;
  const int rc = sam_reader_init(r, header_text, header_len);
  if (rc) { br_sam_reader_free(r); return rc; }
  *out = r;
  return BR_OK;
}

extern "C" int br_sam_reader_release(br_sam_reader *r, int64_t id) {
  if (!r) return BR_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> l(r->m);
  for (auto &c : r->chunks) if (c->id == id) { c->out = false; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

extern "C" const char *br_sam_reader_error(const br_sam_reader *r) { return r ? r->err.c_str() : ""; }

extern "C" int br_sam_reader_stats(const br_sam_reader *r, double *upload_seconds, double *parse_seconds, int64_t *chunks,
                                   uint64_t *bytes, int64_t *lines) {
  if (!r) return BR_ERR_INVALID_ARG;
  if (upload_seconds) { std::lock_guard<std::mutex> l(const_cast<br_sam_reader *>(r)->stat_m); *upload_seconds = r->upload_s; }
  if (parse_seconds) *parse_seconds = r->parse_s;
  if (chunks) *chunks = r->n_chunks;
  if (bytes) *bytes = r->n_bytes_in;
  if (lines) *lines = r->line_base;
  return BR_OK;
}

constexpr uint64_t SAM_MAX_CHUNK = 1ull << 30;   // text per call (field offsets are 32-bit; HBM for the scratch arrays)

extern "C" int br_sam_reader_upload(br_sam_reader *r, int slot, const uint8_t *text, uint64_t n) {
  if (!r || slot < 0 || slot > 1 || (!text && n)) return BR_ERR_INVALID_ARG;
  n = std::min(n, SAM_MAX_CHUNK);
  HIPCHK(hipSetDevice(r->device));
  hipStream_t st = r->up_st;
  RC(r->text[slot].ensure(n + 16));
  HIPCHK(hipEventRecord(r->up_t[0], st));
  // two pinned buffers: the host fills one while the other one's bytes cross PCIe
  for (uint64_t o = 0, k = 0; o < n; o += br_sam_reader::PIN_BYTES, k++) {
    const int s = (int)(k & 1);
    const size_t len = (size_t)std::min<uint64_t>(br_sam_reader::PIN_BYTES, n - o);
    if (r->pin_used[s]) HIPCHK(hipEventSynchronize(r->pin_ev[s]));
    memcpy(r->pin[s], text + o, len);
    HIPCHK(hipMemcpyAsync(r->text[slot].as<uint8_t>() + o, r->pin[s], len, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(r->pin_ev[s], st));
    r->pin_used[s] = true;
  }
  HIPCHK(hipEventRecord(r->up_t[1], st));
  HIPCHK(hipEventRecord(r->up_done[slot], st));
  HIPCHK(hipEventSynchronize(r->up_t[1]));
  float ms = 0;
  if (hipEventElapsedTime(&ms, r->up_t[0], r->up_t[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
  std::lock_guard<std::mutex> l(r->stat_m);
  r->upload_s += 1e-3 * ms;
  r->text_n[slot] = n;
  return BR_OK;
}

static int sam_next(br_sam_reader *r, int slot, const uint8_t *text, uint64_t n, int last, uint64_t *consumed, br_device_records *bundle,
                    int64_t *id, int64_t *n_unmapped, int64_t *bad_line) {
  hipStream_t st = r->st;
  HIPCHK(hipSetDevice(r->device));
  {
    std::lock_guard<std::mutex> l(r->stat_m);
    if (r->text_n[slot] != n) return BR_ERR_INVALID_ARG;   // the slot does not hold these bytes
  }
  HIPCHK(hipStreamWaitEvent(st, r->up_done[slot], 0));
  HIPCHK(hipEventRecord(r->ev[1], st));
  const uint8_t *d_text = r->text[slot].as<uint8_t>();
  // line index
  const uint64_t tiles = (n + SAM_NL_TILE - 1) / SAM_NL_TILE;
  RC(r->tile.ensure((tiles + 1) * 8));
  RC(r->tmp.ensure(scan_scratch_bytes((int64_t)std::max<uint64_t>(tiles, n / 64))));   // (the line scans below: as a rule no second allocation)
  launch_sam_nl_count(st, d_text, n, r->tile.as<uint64_t>());
  launch_scan(st, r->tile.as<uint64_t>(), (int64_t)tiles, r->tmp.as<uint64_t>());
  uint64_t n_nl = 0;
  HIPCHK(hipMemcpyAsync(&n_nl, r->tile.as<uint64_t>() + tiles, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const bool tail_line = last && text[n - 1] != '\n';   // the file's last line may lack its '\n'
  const int64_t n_lines = (int64_t)n_nl + (tail_line ? 1 : 0);
  if (n_lines == 0) { *consumed = 0; return BR_OK; }
  RC(r->lend.ensure((size_t)(n_lines + 1) * 8));
  launch_sam_nl_write(st, d_text, n, r->tile.as<uint64_t>(), r->lend.as<uint64_t>());
  if (tail_line) { r->last_nl = n; HIPCHK(hipMemcpyAsync(r->lend.as<uint64_t>() + n_nl, &r->last_nl, 8, hipMemcpyHostToDevice, st)); }
  // measure
  const size_t nl1 = (size_t)n_lines + 1;
  RC(r->line.ensure(nl1 * sizeof(SamLine))); RC(r->mapped.ensure(nl1 * 8)); RC(r->bytes.ensure(nl1 * 8));
  RC(r->tmp.ensure(scan_scratch_bytes((int64_t)n_lines)));
  RC(r->fix.ensure((size_t)r->fix_cap * sizeof(SamFix)));
  unsigned long long *first_bad = (unsigned long long *)r->small.p;
  uint32_t *n_fix = (uint32_t *)(r->small.as<uint8_t>() + 8);
  HIPCHK(hipMemsetAsync(r->small.p, 0xff, 8, st));
  HIPCHK(hipMemsetAsync(n_fix, 0, 4, st));
  SamArgs A{};
  A.text = d_text; A.n_bytes = n; A.lend = r->lend.as<uint64_t>(); A.n_lines = n_lines; A.line = r->line.as<SamLine>();
  A.mapped = r->mapped.as<uint64_t>(); A.bytes = r->bytes.as<uint64_t>(); A.first_bad = first_bad;
  A.h_slot = r->h_slot.as<int32_t>(); A.h_mask = r->h_mask; A.name_off = r->name_off.as<uint64_t>(); A.names = r->names.as<uint8_t>();
  A.n_ref = r->n_ref;
  launch_sam_measure(st, A);
  launch_scan(st, A.mapped, n_lines, r->tmp.as<uint64_t>());
  launch_scan(st, A.bytes, n_lines, r->tmp.as<uint64_t>());
  uint64_t h3[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(&h3[0], first_bad, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&h3[1], A.mapped + n_lines, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&h3[2], A.bytes + n_lines, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (h3[0] != ~0ull) {
    const int64_t bl = (int64_t)(h3[0] >> 8);
    *bad_line = r->line_base + bl + 1;
    r->err = sam_reason((int)(h3[0] & 0xff));
    return BR_ERR_INVALID_ARG;
  }
  const int64_t n_mapped = (int64_t)h3[1];
  const uint64_t total = h3[2];
  // the chunk that holds this call's records until br_sam_reader_release
  br_sam_reader::Chunk *ch = nullptr;
  {
    std::lock_guard<std::mutex> l(r->m);
    for (auto &c : r->chunks) if (!c->out) { ch = c.get(); break; }
    if (!ch) { r->chunks.push_back(std::make_unique<br_sam_reader::Chunk>()); ch = r->chunks.back().get(); }
  }
  RC(ch->blob.ensure(total + 64)); RC(ch->off.ensure((size_t)n_mapped * 8 + 8));
  RC(ch->len.ensure((size_t)n_mapped * 4 + 4)); RC(ch->rline.ensure((size_t)n_mapped * 4 + 4));
  A.blob = ch->blob.as<uint8_t>(); A.rec_off = ch->off.as<uint64_t>(); A.rec_len = ch->len.as<uint32_t>(); A.rec_line = ch->rline.as<uint32_t>();
  A.n_fix = n_fix;
  uint32_t nf = 0;
  for (int pass = 0; pass < 2; pass++) {
    A.fix = r->fix.as<SamFix>(); A.fix_cap = r->fix_cap;
    if (n_mapped) launch_sam_emit(st, A);
    HIPCHK(hipMemcpyAsync(&nf, n_fix, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nf <= r->fix_cap) break;
    r->fix_cap = nf;   // more floats off the fast path than the list holds: a longer list, and the records once more
    RC(r->fix.ensure((size_t)r->fix_cap * sizeof(SamFix)));
    HIPCHK(hipMemsetAsync(n_fix, 0, 4, st));
  }
  HIPCHK(hipEventRecord(r->ev[2], st));
  // floats the device could not convert exactly: (float)strtod(text), as sam_parse1 does
  if (nf) {
    std::vector<SamFix> fx(nf);
    HIPCHK(hipMemcpyAsync(fx.data(), r->fix.p, nf * sizeof(SamFix), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<float> val(nf);
    int64_t bad = -1;
    for (uint32_t k = 0; k < nf; k++) {
      std::string s((const char *)text + fx[k].text, fx[k].text_len);
      char *e = nullptr;
      const double d = strtod(s.c_str(), &e);
      if (e != s.c_str() + s.size()) { if (bad < 0 || (int64_t)fx[k].line < bad) bad = fx[k].line; continue; }
      val[k] = (float)d;
    }
    if (bad >= 0) { *bad_line = r->line_base + bad + 1; r->err = sam_reason(SAM_E_FLOAT); return BR_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < nf; k++) HIPCHK(hipMemcpyAsync(A.blob + fx[k].dst, &val[k], 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  // the cut: everything in front of the last read-name group, unless the text ends with the file
  int64_t n_take = n_mapped, cut_line = n_lines;
  uint64_t used = n;
  if (!last) {
    if (n_mapped > 0) {
      HIPCHK(hipMemsetAsync(r->small.as<uint8_t>() + 16, 0, 8, st));
      launch_last_group(st, A.blob, A.rec_off, n_mapped, (unsigned long long *)(r->small.as<uint8_t>() + 16));
      uint64_t g = 0;
      HIPCHK(hipMemcpyAsync(&g, r->small.as<uint8_t>() + 16, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      uint32_t gl = 0;
      HIPCHK(hipMemcpyAsync(&gl, A.rec_line + g, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      n_take = (int64_t)g; cut_line = gl;
      uint64_t prev_end = 0;
      if (gl) { HIPCHK(hipMemcpyAsync(&prev_end, A.lend + gl - 1, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); }
      used = gl ? prev_end + 1 : 0;
    } else {   // only unmapped lines: all complete ones are done with
      n_take = 0; cut_line = n_lines;
      const uint8_t *q = (const uint8_t *)memrchr(text, '\n', (size_t)n);
      used = q ? (uint64_t)(q - text) + 1 : 0;
    }
  }
  float ms_parse = 0;
  if (hipEventElapsedTime(&ms_parse, r->ev[1], r->ev[2]) == hipSuccess) r->parse_s += 1e-3 * ms_parse;
  (void)hipGetLastError();
  r->n_chunks++; r->n_bytes_in += used;
  r->line_base += cut_line;
  {
    std::lock_guard<std::mutex> l(r->m);
    ch->id = r->next_id++; ch->out = true;
  }
  bundle->blob = A.blob; bundle->rec_off = A.rec_off; bundle->rec_len = A.rec_len; bundle->n_aln = n_take;
  *id = ch->id;
  *n_unmapped = cut_line - n_take;
  *consumed = used;
  return BR_OK;
}

extern "C" int br_sam_reader_next_staged(br_sam_reader *r, int slot, const uint8_t *text, uint64_t n_bytes, int last, uint64_t *consumed,
                                         br_device_records *bundle, int64_t *id, int64_t *n_unmapped, int64_t *bad_line) {
  if (!r || slot < 0 || slot > 1 || (!text && n_bytes) || !consumed || !bundle || !id || !n_unmapped || !bad_line) return BR_ERR_INVALID_ARG;
  memset(bundle, 0, sizeof(*bundle));
  *consumed = 0; *id = -1; *n_unmapped = 0; *bad_line = 0;
  r->err.clear();
  if (n_bytes > SAM_MAX_CHUNK) { n_bytes = SAM_MAX_CHUNK; last = 0; }
  if (n_bytes == 0) return BR_OK;
  return sam_next(r, slot, text, n_bytes, last, consumed, bundle, id, n_unmapped, bad_line);
}

extern "C" int br_sam_reader_next(br_sam_reader *r, const uint8_t *text, uint64_t n_bytes, int last, uint64_t *consumed,
                                  br_device_records *bundle, int64_t *id, int64_t *n_unmapped, int64_t *bad_line) {
  if (!r || (!text && n_bytes)) return BR_ERR_INVALID_ARG;
  RC(br_sam_reader_upload(r, 0, text, n_bytes));
  return br_sam_reader_next_staged(r, 0, text, n_bytes, last, consumed, bundle, id, n_unmapped, bad_line);
}
