// The SAM text input of the command line (told apart from BGZF by its first bytes, as htslib's hts_open does): a feeder
// thread cuts the text (the mapped file, or what a pipe delivers) into chunks of about --bundle-size records at read-name
// changes and deals them to one br_sam_reader per device, which makes the BAM records on the device; the projection and the
// writer are the BAM path's.
#include <errno.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../sam_header.h"
#include "cli_input.h"

namespace brcli {
namespace {
// the SAM text: the mapped file, or a pipe read as it comes
struct SamText {
  const uint8_t *map = nullptr; size_t map_size = 0;
  int fd = -1; bool own_fd = false, eof = false, read_failed = false;
  brio::ByteBuf pbuf;            // pipe: bytes read, not yet handed out
  uint64_t header_bytes = 0, header_lines = 0;
  ~SamText() { if (map) munmap((void *)map, map_size); if (own_fd && fd >= 0) close(fd); }
  size_t read_more(size_t want) {   // appends up to `want` bytes of the pipe; 0 at its end
    size_t got = 0;
    while (got < want && !eof) {
      const size_t old = pbuf.size();
      pbuf.resize(old + (want - got));
      ssize_t k = read(fd, pbuf.data() + old, want - got);
      pbuf.resize(old + (k > 0 ? (size_t)k : 0));
      if (k < 0 && errno == EINTR) continue;
      if (k < 0) read_failed = true;   // (a read error is not the end of the input: the run fails)
      if (k <= 0) { eof = true; break; }
      got += (size_t)k;
    }
    return got;
  }
  // stream_fd >= 0: a stream the sniffing has begun to read (peek = its first bytes); else the regular file at path
  bool open(const std::string &path, int stream_fd, const std::string &peek, BamHeader &h, std::string &err) {
    if (stream_fd >= 0) { fd = stream_fd; own_fd = fd != 0; }
    else { fd = ::open(path.c_str(), O_RDONLY); own_fd = true; if (fd < 0) { err = "cannot open " + path; return false; } }
    struct stat sb;
    if (stream_fd < 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
      void *m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m != MAP_FAILED) { map = (const uint8_t *)m; map_size = (size_t)sb.st_size; madvise(m, map_size, MADV_SEQUENTIAL); }
    }
    const uint8_t *d; uint64_t n;
    if (map) { d = map; n = map_size; (void)br_sam_header_scan(d, n, &header_bytes); }
    else {
      pbuf.resize(peek.size()); memcpy(pbuf.data(), peek.data(), peek.size());
      for (;;) {   // until a line that is not a header line has begun, or the stream ends
        (void)br_sam_header_scan(pbuf.data(), pbuf.size(), &header_bytes);
        if (header_bytes < pbuf.size() || eof) break;
        read_more(1u << 20);
      }
      if (read_failed) { err = "read error"; return false; }
      d = pbuf.data(); n = pbuf.size();
    }
    h.text.assign((const char *)d, (size_t)header_bytes);
    for (uint64_t i = 0; i < header_bytes; i++) header_lines += d[i] == '\n';
    if (!br::sam_header_refs(h.text.data(), h.text.size(), h.ref_names, h.ref_lens)) { err = "@SQ line without SN:"; return false; }
    if (!map) pbuf.erase_front((size_t)header_bytes);
    return true;
  }
};

// the read name of the line at p (up to its first tab)
inline std::pair<const uint8_t *, size_t> line_name(const uint8_t *p, const uint8_t *end) {
  const uint8_t *t = (const uint8_t *)memchr(p, '\t', (size_t)(end - p));
  const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
  const uint8_t *e = t && (!nl || t < nl) ? t : nl ? nl : end;
  return {p, (size_t)(e - p)};
}
// Where the chunk that starts at `start` ends: at a read-name change near `target`.  Backwards from the last complete line in
// front of target to the first line of its name group; when that group began at `start` (one group longer than the target),
// forwards to the next name change.  nullptr: the text in [start, end) does not reach that change yet (at_eof: the end does).
const uint8_t *sam_cut(const uint8_t *start, const uint8_t *target, const uint8_t *end, bool at_eof) {
  auto same = [&](const uint8_t *a, const uint8_t *b) { auto x = line_name(a, end), y = line_name(b, end); return x.second == y.second && memcmp(x.first, y.first, x.second) == 0; };
  const uint8_t *nl = target > start ? (const uint8_t *)memrchr(start, '\n', (size_t)(target - start)) : nullptr;
  if (nl) {
    const uint8_t *pn = nl > start ? (const uint8_t *)memrchr(start, '\n', (size_t)(nl - start)) : nullptr;
    const uint8_t *L = pn ? pn + 1 : start;
    while (L > start) {
      const uint8_t *q = L - 1 > start ? (const uint8_t *)memrchr(start, '\n', (size_t)(L - 1 - start)) : nullptr;
      const uint8_t *P = q ? q + 1 : start;
      if (!same(P, L)) break;
      L = P;
    }
    if (L > start) return L;
  }
  for (const uint8_t *q = start;;) {   // forwards: the first line whose name differs from the first line's
    const uint8_t *e = (const uint8_t *)memchr(q, '\n', (size_t)(end - q));
    if (!e) return at_eof ? end : nullptr;
    q = e + 1;
    if (q >= end) return at_eof ? end : nullptr;
    if (!memchr(q, '\n', (size_t)(end - q)) && !at_eof) return nullptr;   // (a name is only known once its line is complete)
    if (!same(start, q)) return q;
  }
}
struct SamChunk { const uint8_t *data = nullptr; uint64_t n = 0; brio::ByteBuf own; int64_t line0 = -1; uint64_t seq = 0; };
// One SAM reader per device: its chunks (whole read-name groups, in file order k = d, d + N, ...) become device records.
// Two threads a device: the uploader (br_sam_reader_upload, one chunk ahead) and the processor (br_sam_reader_next_staged)
class SamInput : public DevInput {
 public:
  explicit SamInput(const Options &o) : DevInput(o) { for (size_t d = 0; d < o.devices.size(); d++) dev.emplace_back(new Dev()); }
  bool open(int stream_fd, const std::string &peek, std::string &err) { return sam.open(o.in_bam, stream_fd, peek, hdr, err); }
  bool start(Outbox &out_, std::string &) override {
    out = &out_;
    for (size_t d = 0; d < dev.size(); d++) { threads.emplace_back([this, d] { upload(d); }); threads.emplace_back([this, d] { process(d); }); }
    reader = std::thread([this] { feed(); });
    return true;
  }
  void report_timing() const override {
    double t_up = 0, t_parse = 0; uint64_t nb = 0;
    for (auto &D : dev) { double u = 0, p = 0; uint64_t b = 0; (void)br_sam_reader_stats(D->r, &u, &p, nullptr, &b, nullptr); t_up += u; t_parse += p; nb += b; }
    fprintf(stderr, "[bramble] SAM readers: %.3f GB of text, device upload %.3fs, device parse %.3fs (summed over devices); feeder thread %.2fs\n",
            1e-9 * (double)nb, t_up, t_parse, t_feeder);
  }
 private:
  // a device's SAM uploader puts chunk j into text slot j % 2 while its processor parses chunk j - 1 (two permits = two slots)
  struct Staged { std::unique_ptr<SamChunk> c; int slot; int rc; };
  struct Dev { Slot<SamChunk> q{2}; Slot<Staged> ready{2}; std::mutex m; std::condition_variable cv; int permits = 2; br_sam_reader *r = nullptr; };
  void wake() override { for (auto &D : dev) { std::lock_guard<std::mutex> l(D->m); D->cv.notify_all(); } }
  void free_readers() override { for (auto &D : dev) { if (D->r) br_sam_reader_free(D->r); D->r = nullptr; } }
  void upload(size_t d) {
    Dev &D = *dev[d];
    int rrc = cancel ? 0 : br_sam_reader_new(o.devices[d], hdr.text.data(), hdr.text.size(), &D.r);
    if (rrc) set_err(std::string("SAM reader: ") + br_strerror(rrc));
    for (int64_t j = 0;; j++) {
      auto c = D.q.take();
      if (!c) break;
      if (cancel || !D.r) continue;   // (drain)
      { std::unique_lock<std::mutex> l(D.m); D.cv.wait(l, [&] { return D.permits > 0 || cancel; }); if (cancel) continue; D.permits--; }
      auto st = std::make_unique<Staged>();
      st->slot = (int)(j & 1);
      st->rc = br_sam_reader_upload(D.r, st->slot, c->data, c->n);
      st->c = std::move(c);
      D.ready.put(std::move(st));
    }
    D.ready.finish();
  }
  void process(size_t d) {
    auto tr0 = now();
    Dev &D = *dev[d];
    for (;;) {
      auto st = D.ready.take();
      if (!st) break;
      auto give_back = [&]() { { std::lock_guard<std::mutex> l(D.m); D.permits++; } D.cv.notify_all(); };
      if (cancel) { give_back(); continue; }   // (drain)
      br_sam_reader *R = D.r;
      SamChunk *c = st->c.get();
      int64_t lines_before = 0;
      (void)br_sam_reader_stats(R, nullptr, nullptr, nullptr, nullptr, &lines_before);
      auto b = std::make_unique<DevBundle>([R](int64_t id) { (void)br_sam_reader_release(R, id); });
      uint64_t used = 0; int64_t un = 0, bad = 0;
      int rrc = st->rc ? st->rc : br_sam_reader_next_staged(R, st->slot, c->data, c->n, 1, &used, &b->recs, &b->id, &un, &bad);
      give_back();
      if (rrc) {
        if (rrc == BR_ERR_INVALID_ARG && bad > 0) {
          // the file's line number: header lines + lines in front of the chunk + the line inside it
          int64_t l0 = c->line0;
          if (l0 < 0) { l0 = (int64_t)sam.header_lines; for (const uint8_t *p = sam.map + sam.header_bytes; p < c->data; p++) l0 += *p == '\n'; }
          std::string m = std::to_string(l0 + (bad - lines_before)) + ": " + br_sam_reader_error(R);
          if (sam.header_bytes == 0) m += " (the input is not BGZF/BAM, and as SAM text it has no header)";
          set_err(m, true);
        } else set_err(std::string("SAM reader: ") + br_strerror(rrc));
        continue;
      }
      if (used != c->n) {   // (a chunk the reader could not take whole: one read-name group of more than 1 GiB of text)
        b->release();
        set_err("a read-name group spans more than the SAM reader can take at once (1 GiB of text)");
        continue;
      }
      b->seq = c->seq;
      hand_over(d, std::move(b), un);
    }
    processor_done(d, tr0);
  }
  // the feeder: chunks of about --bundle-size records, cut at read-name changes, dealt round-robin to the devices
  void feed() {
    auto tr0 = now();
    uint64_t k = 0;
    const bool mapped = sam.map != nullptr;
    if (!mapped && !sam.eof) sam.read_more(4u << 20);
    // bytes a record takes, from the first lines (the chunk size follows from --bundle-size)
    const uint8_t *s0 = mapped ? sam.map + sam.header_bytes : sam.pbuf.data();
    const uint64_t n0 = mapped ? sam.map_size - sam.header_bytes : sam.pbuf.size();
    uint64_t probe = std::min<uint64_t>(n0, 4u << 20), nl0 = 0;
    for (uint64_t i = 0; i < probe; i++) nl0 += s0[i] == '\n';
    const uint64_t per_line = nl0 ? probe / nl0 + 1 : 512;
    const uint64_t chunk_bytes = std::max<uint64_t>(1u << 20, std::min<uint64_t>((uint64_t)o.bundle_records * per_line, 768ull << 20));
    uint64_t off = 0;            // mapped: where the next chunk starts (behind the header)
    int64_t line0 = (int64_t)sam.header_lines;   // pipe: the file line of the next chunk's first line
    while (!cancel) {
      auto c = std::make_unique<SamChunk>();
      if (mapped) {
        const uint8_t *start = s0 + off, *end = s0 + n0;
        if (start >= end) break;
        const uint8_t *target = start + std::min<uint64_t>(chunk_bytes, (uint64_t)(end - start));
        const uint8_t *cut = target == end ? end : sam_cut(start, target, end, true);
        c->data = start; c->n = (uint64_t)(cut - start);
        off += c->n;
      } else {
        const uint8_t *cut = nullptr;
        for (uint64_t want = chunk_bytes;; want *= 2) {
          while (sam.pbuf.size() < want && !sam.eof) sam.read_more(std::min<uint64_t>(want - sam.pbuf.size(), 64u << 20));
          if (sam.pbuf.size() == 0) break;
          const uint8_t *start = sam.pbuf.data(), *end = start + sam.pbuf.size();
          const uint8_t *target = start + std::min<uint64_t>(want, sam.pbuf.size());
          cut = (target == end && sam.eof) ? end : sam_cut(start, target, end, sam.eof);
          if (cut) break;
        }
        if (!cut) break;
        const uint64_t n = (uint64_t)(cut - sam.pbuf.data());
        c->own.resize(n); memcpy(c->own.data(), sam.pbuf.data(), n);
        sam.pbuf.erase_front(n);
        c->data = c->own.data(); c->n = n; c->line0 = line0;
        for (uint64_t i = 0; i < n; i++) line0 += c->data[i] == '\n';
      }
      c->seq = k;
      dev[k % dev.size()]->q.put(std::move(c));
      k++;
    }
    if (sam.read_failed) set_err("read error");
    next_seq = k;
    for (auto &D : dev) D->q.finish();
    t_feeder = secs(tr0, now());
  }

  SamText sam;
  std::vector<std::unique_ptr<Dev>> dev;
  double t_feeder = 0;
};

}  // namespace

std::unique_ptr<Input> open_sam(const Options &o, int stream_fd, const std::string &peek, std::string &err) {
  std::unique_ptr<SamInput> in(new SamInput(o));
  std::string e;
  if (!in->open(stream_fd, peek, e)) { err = o.in_bam + ": " + e; return nullptr; }
  return in;
}

}  // namespace brcli
