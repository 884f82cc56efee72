// The BAM inputs of the command line and the factory that tells BAM from SAM.  Both BAM readers start from the open
// BgzfReader and the header in front of the records:
//
//   host reader    : one thread -- BGZF inflate (threaded) -> record boundaries -> bundles cut at a read-name change
//                    (process_reads, src/bramble.cpp:330-441; a bundle here is millions of records, the result does not
//                    depend on where a name-collated stream is cut); the workers stage them to their devices
//   device readers : the mapped file's bytes go to the GPUs as they are (br_bam_reader, piece-wise), see DevBamInput
#include <errno.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <future>

#include "cli_input.h"

namespace brcli {
namespace {
using brio::BgzfReader;
// the open file; buf[0, pos): its header, the records follow
struct BamFile { BgzfReader rd; brio::ByteBuf buf; size_t pos = 0; };
// consumes the header from the front of `buf` (reading more as needed); false on a malformed file
bool read_header(BgzfReader &rd, brio::ByteBuf &buf, size_t &pos, BamHeader &h, std::string &err) {
  auto need = [&](size_t n) -> bool {
    while (buf.size() - pos < n) { int64_t got = rd.read(buf, 1 << 20); if (got < 0) { err = rd.error(); return false; } if (got == 0) { err = "truncated BAM header"; return false; } }
    return true;
  };
  auto u32 = [&](size_t at) { uint32_t v; memcpy(&v, buf.data() + at, 4); return v; };
  if (!need(12)) return false;
  if (memcmp(buf.data() + pos, "BAM\1", 4) != 0) { err = "not a BAM file (bad magic): BGZF-compressed SAM (bgzipped SAM) is not supported, decompress it first"; return false; }
  uint32_t l_text = u32(pos + 4);
  if (!need(12 + (size_t)l_text)) return false;
  h.text.assign((const char *)buf.data() + pos + 8, l_text);
  while (!h.text.empty() && h.text.back() == '\0') h.text.pop_back();
  size_t p = pos + 8 + l_text;
  uint32_t n_ref = u32(p); p += 4;
  for (uint32_t r = 0; r < n_ref; r++) {
    if (!need(p - pos + 4)) return false;
    uint32_t l_name = u32(p); p += 4;
    if (!need(p - pos + l_name + 4)) return false;
    h.ref_names.emplace_back((const char *)buf.data() + p, l_name ? l_name - 1 : 0); p += l_name;
    h.ref_lens.push_back(u32(p)); p += 4;
  }
  pos = p;
  return true;
}
const uint8_t *rec_name(const brio::ByteBuf &b, uint64_t off, uint32_t &l) { l = b[off + 8]; return b.data() + off + 32; }
class HostBamInput : public Input {
 public:
  HostBamInput(const Options &o, std::unique_ptr<BamFile> f) : Input(o), f(std::move(f)) {}
  bool start(Outbox &, std::string &) override { reader = std::thread([this] { read(); }); return true; }
  Slot<Bundle> *host_queue() override { return &to_gpu; }
  void recycle(Bundle &b) override { auto spare = std::make_unique<brio::ByteBuf>(); spare->swap(b.blob); std::lock_guard<std::mutex> l(pool_m); pool.push_back(std::move(spare)); }
  void report_timing() const override { fprintf(stderr, "[bramble] reader thread: %.2fs in all, %.2fs reserving buffers, %.2fs waiting for a free queue slot\n", t_reader, t_reserve, t_put); }
 private:
  void drain() override { while (to_gpu.take()) {} }
  void read() {
    BgzfReader &rd = f->rd; brio::ByteBuf &buf = f->buf; size_t &pos = f->pos;
    buf.erase_front(pos); pos = 0;
    std::vector<uint64_t> off; std::vector<uint32_t> len;
    bool eof = false;
    size_t scanned = 0;  // bytes of buf already split into off/len
    // the next chunk inflates (threaded, into the reserved tail of buf) while this thread walks the records of the
    // previous one; `valid` is how far the walker may look
    size_t valid = buf.size();
    const size_t CHUNK = 64u << 20;
    std::future<int64_t> fut; bool inflight = false;
    size_t bundle_bytes = 0;   // size of the largest bundle cut so far: the next buffer is reserved whole instead of growing chunk by chunk
    uint64_t split_bytes = 0, split_recs = 0;   // running mean record length: tells whether the bytes at hand already hold the next cut
    auto tr0 = now();
    struct ReaderClock { double &t; std::chrono::steady_clock::time_point t0; ~ReaderClock() { t = secs(t0, now()); } } reader_clock{t_reader, tr0};
    auto launch = [&]() {
      auto tv0 = now();
      const size_t need = buf.size() + CHUNK + (1u << 20);
      if (need > buf.capacity()) {   // only the first bundles get here (later buffers are reserved whole): one move, from the mean record length
        size_t est = split_recs ? (size_t)std::min<uint64_t>((split_bytes / split_recs + 1) * ((uint64_t)o.bundle_records + 64), (uint64_t)1 << 30) : 0;
        buf.reserve(std::max(std::max(need, est + 2 * CHUNK), std::max(bundle_bytes + 2 * CHUNK, buf.capacity() + buf.capacity() / 2)));
      }
      t_reserve += secs(tv0, now());
      fut = std::async(std::launch::async, [&]() { return rd.read(buf, CHUNK); }); inflight = true;
    };
    auto land = [&]() -> bool {
      auto ti0 = now();
      int64_t got = fut.get(); inflight = false;
      t_inflate += secs(ti0, now());
      if (got < 0) { err = rd.error(); return false; }
      if (got == 0) eof = true;
      valid = buf.size();
      return true;
    };
    // do the bytes already inflated reach past the next cut?  Then they are split first and the next read starts in the NEXT
    // bundle's buffer (beside the copy of this one's tail) instead of landing behind the cut and being copied over with it.
    auto cut_expected = [&]() -> bool {
      if (!split_recs) return false;
      const uint64_t mean = split_bytes / split_recs + 1;
      return off.size() + (valid - scanned) / mean > (size_t)o.bundle_records + 64;
    };
    for (;;) {
      if (cancel) break;
      // split what is there; read more until a cut point exists
      int64_t cut = -1;
      size_t searched = std::max<size_t>((size_t)o.bundle_records, 1);  // records below this index cannot be a cut
      for (;;) {
        if (!eof && !inflight && !cut_expected()) launch();
        auto ts0 = now();
        for (;;) {
          // room for the records to come: from the mean record length (the worst case, 36 bytes a record, is a table six
          // times too large, value-initialised on every pass); a piece that fills its room is followed by another
          const size_t left = valid - scanned, worst = left / 36 + 1;
          size_t cap = split_recs ? std::min<size_t>(worst, (size_t)(left / (split_bytes / split_recs + 1)) * 5 / 4 + 4096) : worst;
          const size_t base = off.size();
          off.resize(base + cap); len.resize(base + cap);
          int64_t n = 0, un = 0; uint64_t used = 0;
          int r = br_bam_split(buf.data() + scanned, left, (int64_t)cap, off.data() + base, len.data() + base, &n, &un, &used);
          if (r) { if (inflight) (void)fut.get(); err = "malformed BAM record"; to_gpu.finish(); return; }
          for (int64_t i = 0; i < n; i++) off[base + (size_t)i] += scanned;
          off.resize(base + (size_t)n); len.resize(base + (size_t)n);
          totals.add(n, un);
          split_bytes += used; split_recs += (uint64_t)(n + un);
          scanned += used;
          if ((size_t)n < cap || used == 0) break;   // the bytes ran out (or end in a partial record), not the room
        }
        // cut: first record >= bundle_records whose name differs from its predecessor's
        for (size_t i = searched; i < off.size(); i++) {
          uint32_t la, lb; const uint8_t *a = rec_name(buf, off[i - 1], la), *b = rec_name(buf, off[i], lb);
          if (la != lb || memcmp(a, b, la) != 0) { cut = (int64_t)i; break; }
        }
        searched = std::max(searched, off.size());
        t_split += secs(ts0, now());
        if (cut >= 0) break;
        if (inflight) { if (!land()) { to_gpu.finish(); return; } continue; }
        if (!eof) { launch(); if (!land()) { to_gpu.finish(); return; } continue; }   // the estimate was short of the cut
        // end of stream, nothing in flight
        if (scanned != valid) { err = "truncated BAM record at end of file"; to_gpu.finish(); return; }
        break;
      }
      if (inflight && !land()) { to_gpu.finish(); return; }   // the buffer must be still before its tail moves
      size_t n_take = cut >= 0 ? (size_t)cut : off.size();
      if (n_take) {
        auto tc0 = now();
        auto b = std::make_unique<Bundle>();
        size_t byte_end = (n_take < off.size()) ? (size_t)off[n_take] - 4 : scanned;
        b->off.assign(off.begin(), off.begin() + (ptrdiff_t)n_take); b->len.assign(len.begin(), len.begin() + (ptrdiff_t)n_take);
        // the bundle takes the buffer; only the tail (records past the cut, < one read chunk) is copied over
        brio::ByteBuf tail;
        { std::lock_guard<std::mutex> l(pool_m); if (!pool.empty()) { tail.swap(*pool.back()); pool.pop_back(); } }
        bundle_bytes = std::max(bundle_bytes, byte_end);
        tail.clear(); tail.reserve(bundle_bytes + 2 * CHUNK);   // whole, while it is empty: growing it later moves the mapping
        const size_t tail_bytes = buf.size() - byte_end;
        tail.resize(tail_bytes);
        buf.resize(byte_end);
        b->blob.swap(buf);
        buf.swap(tail);
        valid = tail_bytes;
        scanned -= byte_end;
        off.erase(off.begin(), off.begin() + (ptrdiff_t)n_take); len.erase(len.begin(), len.begin() + (ptrdiff_t)n_take);   // (the tables keep their capacity)
        for (auto &x : off) x -= byte_end;
        // the next read lands behind the tail's place in the new buffer while the tail itself is still on its way there
        if (!eof && !cut_expected()) launch();
        if (tail_bytes) memcpy(buf.data(), b->blob.data() + byte_end, tail_bytes);   // (launch() may have moved the buffer; the read itself never does)
        t_copy += secs(tc0, now());
        b->seq = next_seq++;   // the writer restores this order whatever worker projects the bundle
        auto tp0 = now();
        to_gpu.put(std::move(b));
        t_put += secs(tp0, now());
      }
      if (cut < 0 && eof && !inflight) break;
    }
    if (inflight) (void)fut.get();
    to_gpu.finish();
  }

  std::unique_ptr<BamFile> f;
  Slot<Bundle> to_gpu{16};     // the reader runs ahead while the guides are parsed and the indexes are built (sixteen bundles: about 3 GB of records)
  std::mutex pool_m; std::vector<std::unique_ptr<brio::ByteBuf>> pool;   // consumed bundle buffers: their pages are already faulted in
  double t_reserve = 0, t_put = 0, t_reader = 0;
};

// Device readers (br_bam_reader, piece-wise): the mapped file's bytes go to the GPUs as they are; inflate, the record split
// and the cuts at read-name changes happen there, beside the guide parsing and the index build (they need neither), and the
// bundles stay in the HBM of the device that made them until its runner has projected them.  The file's BGZF blocks are cut
// into pieces of --bundle-size x 3 / 1000 blocks; piece k goes to device k mod N (reader k mod N inflates it, worker k mod N
// projects it, the writer puts the results back in piece order), so N devices read, project and deflate N pieces at a
// time -- nothing here is one host thread wide (the reference's one reader thread, src/bramble.cpp:329-435, feeds all its
// workers).  Every piece cuts itself off at read-name changes by a rule both neighbours can evaluate (include/bramble_amd.h,
// br_bam_piece_process); with one device the pieces follow each other and every start is known, with several a piece guesses
// where its first record starts and the guess is checked against what the piece in front found: a piece that guessed wrong is
// processed again with the true start before anything of it is used.
class DevBamInput : public DevInput {
 public:
  DevBamInput(const Options &o, std::unique_ptr<BamFile> f) : DevInput(o), f(std::move(f)), n_dev(o.devices.size()), readers(n_dev, nullptr) {
    for (size_t d = 0; d < n_dev; d++) ups.emplace_back(new UpState());
  }
  bool start(Outbox &out_, std::string &err) override {
    out = &out_;
    // the whole file's block table: it grows while the readers are already at work on its first pieces (a lazily committed
    // mapping of the worst-case size, so that the table never moves: a block is at least 28 bytes)
    blk.bytes = (size_t)(f->rd.mapped_size() / 28 + 16) * sizeof(br_bgzf_block);
    void *tab_mem = mmap(nullptr, blk.bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (tab_mem == MAP_FAILED) { err = "out of memory (block table)"; return false; }
    blk.p = (br_bgzf_block *)tab_mem;
    threads.emplace_back([this] { scan_blocks(); });
    for (size_t d = 0; d < n_dev; d++) { threads.emplace_back([this, d] { upload(d); }); threads.emplace_back([this, d] { process(d); }); }
    reader = std::thread([this] {   // (the work is on the threads above; this one only waits for the block table, for next_seq)
      std::unique_lock<std::mutex> l(piece_m); piece_cv.wait(l, [&] { return table_ready || cancel; });
      next_seq = (uint64_t)n_pieces;
    });
    return true;
  }
  void report_timing() const override {
    double t_in = 0, t_up = 0;
    for (auto r : readers) { t_in = std::max(t_in, br_bam_reader_seconds(r)); t_up = std::max(t_up, br_bam_reader_upload_seconds(r)); }
    const uint64_t fsize = f->rd.mapped_size();
    fprintf(stderr, "[bramble] device readers: the compressed bytes went up in %.2fs of the longest uploader (%.1f GB/s of the file's %.2f GB; pinned buffers filled by four threads)\n",
            t_up, t_up > 0 ? 1e-9 * (double)fsize / (double)n_dev / t_up : 0.0, 1e-9 * (double)fsize);
    fprintf(stderr, "[bramble] device readers: block table %.2fs; the longest processing thread %.2fs in all (inflate + record split + cuts: %.2fs; the rest: waiting for its uploads, its neighbour's cut, the runner's queue); %llu pieces, %llu processed again from the true start\n",
            t_block_scan, t_dev_reader, t_in, (unsigned long long)n_pieces, (unsigned long long)reprocessed.load());
  }
 private:
  // (each under its mutex: a thread that has just found its wait predicate false is blocked before the notification comes)
  void wake() override {
    { std::lock_guard<std::mutex> l(piece_m); } piece_cv.notify_all();
    for (auto &u : ups) { { std::lock_guard<std::mutex> l(u->m); } u->cv.notify_all(); }
  }
  void free_readers() override { for (auto &r : readers) { if (r) br_bam_reader_free(r); r = nullptr; } }
  // the block table: one walk over the block headers of the mapping (a cache line per block), published as it grows
  void scan_blocks() {
    const uint8_t *file = f->rd.mapped(); const uint64_t fsize = f->rd.mapped_size();
    auto t0 = now();
    int64_t nb = 0; uint64_t src_base = 0, dst_base = 0;
    int rc2 = 0;
    const int64_t step = std::max<int64_t>(256, std::min<int64_t>(piece_blocks, 4096));
    while (!rc2 && src_base < fsize && !cancel) {
      int64_t got = 0; uint64_t used = 0, total = 0;
      rc2 = br_bgzf_scan(file + src_base, fsize - src_base, step, blk.p + nb, &got, &used, &total);
      if (rc2) break;
      for (int64_t i = 0; i < got; i++) { blk.p[nb + i].src_off += src_base; blk.p[nb + i].dst_off += dst_base; }
      if (used == 0) { rc2 = BR_ERR_INVALID_ARG; break; }   // a truncated block at the end of the file
      src_base += used; dst_base += total; nb += got;
      { std::lock_guard<std::mutex> l(piece_m); n_blk = nb; const size_t np = (size_t)((nb + piece_blocks - 1) / piece_blocks); piece_end.resize(np, 0); piece_known.resize(np, 0); }
      piece_cv.notify_all();
    }
    t_block_scan = secs(t0, now());
    {
      std::lock_guard<std::mutex> l(piece_m);
      n_blk = nb; n_pieces = nb ? (nb + piece_blocks - 1) / piece_blocks : 0;
      piece_end.resize((size_t)n_pieces, 0); piece_known.resize((size_t)n_pieces, 0);
      table_ready = true; table_failed = rc2 != 0;
    }
    if (rc2) set_err(std::string("malformed or truncated BAM file (") + br_strerror(rc2) + ")");
    piece_cv.notify_all();
  }
  // blocks [b0, b1) of piece k and the `extra` blocks behind them; waits until the table has grown past them (or is whole).
  // false: no such piece (the table ended in front of it), or the run is being cancelled
  bool piece_range(int64_t k, int64_t extra, int64_t &b0, int64_t &b1, int64_t &b1x, int64_t &nb_now) {
    std::unique_lock<std::mutex> l(piece_m);
    const int64_t want = (k + 1) * piece_blocks + extra;
    piece_cv.wait(l, [&] { return n_blk > want || table_ready || cancel; });
    if (cancel || table_failed) return false;
    nb_now = n_blk;
    b0 = k * piece_blocks;
    if (b0 >= n_blk) return false;
    b1 = std::min(n_blk, b0 + piece_blocks); b1x = std::min(n_blk, b1 + extra);
    return true;
  }
  // uploader of device d: the compressed bytes of its pieces, one piece ahead of the processing
  void upload(size_t d) {
    UpState &U = *ups[d];
    int rrc = cancel ? 0 : br_bam_reader_new(o.devices[d], (int32_t)hdr.ref_names.size(), (uint64_t)f->pos, &readers[d]);
    if (rrc) set_err(std::string("device reader: ") + br_strerror(rrc));
    int64_t j = 0;
    for (int64_t k = (int64_t)d; !rrc && !cancel; k += (int64_t)n_dev, j++) {
      int64_t b0, b1, b1x, nb_now;
      if (!piece_range(k, 2, b0, b1, b1x, nb_now)) break;
      { std::unique_lock<std::mutex> l(U.m); U.cv.wait(l, [&] { return U.free_slots > 0 || cancel; }); if (cancel) break; U.free_slots--; }
      rrc = br_bam_piece_upload(readers[d], (int)(j & 1), f->rd.mapped(), f->rd.mapped_size(), blk.p, nb_now, b0, b1x);
      if (rrc) { set_err(std::string("device reader: ") + br_strerror(rrc)); break; }
      { std::lock_guard<std::mutex> l(U.m); U.ready.push_back(k); }
      U.cv.notify_all();
    }
    { std::lock_guard<std::mutex> l(U.m); U.done = true; }
    U.cv.notify_all();
  }
  // processor of device d: inflate, split and cut its pieces; check a guessed start against the piece in front
  void process(size_t d) {
    auto tr0 = now();
    UpState &U = *ups[d];
    for (int64_t j = 0;; j++) {
      int64_t k = -1;
      { std::unique_lock<std::mutex> l(U.m); U.cv.wait(l, [&] { return !U.ready.empty() || U.done || cancel; }); if (!U.ready.empty()) { k = U.ready.front(); U.ready.pop_front(); } }
      if (k < 0) break;
      const int slot = (int)(j & 1);
      br_bam_reader *R = readers[d];
      int64_t b0, b1, b1x, nb_now;
      if (!piece_range(k, 2, b0, b1, b1x, nb_now)) break;   // (the uploader has seen this range already: no waiting here)
      auto b = std::make_unique<DevBundle>([R](int64_t id) { (void)br_bam_reader_release(R, id); });
      br_piece_info info; memset(&info, 0, sizeof(info));
      // the start: the header's end (first piece), the end of the piece in front when this reader made it itself, else a guess
      int64_t start_rel = -1;
      if (k == 0) start_rel = (int64_t)f->pos;
      else if (n_dev == 1) { std::lock_guard<std::mutex> l(piece_m); start_rel = (int64_t)piece_end[(size_t)k - 1]; }
      int rrc = 0;
      int64_t extra = 2;
      for (int tries = 0;; tries++) {
        rrc = cancel ? BR_ERR_INVALID_ARG : br_bam_piece_process(R, slot, blk.p, nb_now, b1, start_rel, &b->recs, &b->id, &info);
        if (rrc == BR_PIECE_MORE && tries < 12) {   // the group at the piece's end goes on: more of the next piece's blocks
          extra *= 8;
          if (!piece_range(k, extra, b0, b1, b1x, nb_now)) { rrc = BR_ERR_INVALID_ARG; break; }
          rrc = br_bam_piece_upload(R, slot, f->rd.mapped(), f->rd.mapped_size(), blk.p, nb_now, b0, b1x);
          if (!rrc) continue;
        }
        if (rrc) break;
        if (start_rel >= 0) break;
        // a guessed start: what did the piece in front find?
        uint64_t want = 0;
        { std::unique_lock<std::mutex> l(piece_m); piece_cv.wait(l, [&] { return piece_known[(size_t)k - 1] || cancel; }); want = piece_end[(size_t)k - 1]; }
        if (cancel) { rrc = BR_ERR_INVALID_ARG; break; }
        if (piece_spoil > 0 && k % piece_spoil == 0) info.start_rel ^= 1u;   // test hook: treat the guess as wrong
        if (info.start_rel == want) break;
        b->release();    // the guess was wrong: once more, from the true start
        reprocessed++;
        start_rel = (int64_t)want;
      }
      if (rrc) { if (!cancel) set_err(rrc == BR_PIECE_MORE ? std::string("a read-name group spans more than the reader can hold") : rrc == BR_ERR_INVALID_ARG ? std::string("malformed or truncated BAM file (") + br_strerror(rrc) + ")" : std::string("device reader: ") + br_strerror(rrc)); break; }
      { std::lock_guard<std::mutex> l(piece_m); piece_end[(size_t)k] = info.end_rel; piece_known[(size_t)k] = 1; }
      piece_cv.notify_all();
      { std::lock_guard<std::mutex> l(U.m); U.free_slots++; }
      U.cv.notify_all();
      b->seq = (uint64_t)k;
      hand_over(d, std::move(b), info.n_unmapped);
    }
    processor_done(d, tr0);
  }

  std::unique_ptr<BamFile> f;
  const size_t n_dev;
  std::vector<br_bam_reader *> readers;
  struct BlockTable { br_bgzf_block *p = nullptr; size_t bytes = 0; ~BlockTable() { if (p) munmap(p, bytes); } } blk;
  int64_t n_blk = 0, n_pieces = 0;          // blocks known so far (under piece_m); pieces: known once the table is done
  const int64_t piece_blocks = std::max<int64_t>(1, std::min<int64_t>(o.bundle_records * 3 / 1000, 8192));
  std::mutex piece_m; std::condition_variable piece_cv;
  std::vector<uint64_t> piece_end; std::vector<char> piece_known;   // end_rel of every finished piece (the next one's true start)
  bool table_ready = false, table_failed = false;   // ready: the whole file has been walked
  std::atomic<uint64_t> reprocessed{0};
  const int64_t piece_spoil = getenv("BRAMBLE_AMD_PIECE_SPOIL") ? atoll(getenv("BRAMBLE_AMD_PIECE_SPOIL")) : 0;   // test hook (tests/test_gpu_cli.py): every k-th guessed start counts as wrong
  double t_block_scan = 0;
  // a device's uploader and processor: two piece slots, the pieces uploaded and not yet processed
  struct UpState { std::mutex m; std::condition_variable cv; int free_slots = 2; std::deque<int64_t> ready; bool done = false; };
  std::vector<std::unique_ptr<UpState>> ups;
};

// What the input holds, from its first bytes: 0 BGZF (BAM), 1 SAM text, -1 error.  A regular file is looked at with pread and
// reopened by its path (the readers map it); anything else -- standard input ("-"), a pipe or FIFO given by its path -- is read
// once: *stream_fd is the open descriptor the reader goes on with, and the bytes read to find out are kept in `peek` for it.
int sniff_input(const std::string &path, int *stream_fd, std::string &peek, std::string &err) {
  uint8_t h[18];
  size_t got = 0;
  *stream_fd = -1;
  int fd = 0;
  if (path != "-") {
    fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) { err = "cannot open " + path; return -1; }
    struct stat sb;
    if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) {
      const ssize_t k = pread(fd, h, sizeof h, 0);
      close(fd);
      if (k < 0) { err = "cannot read " + path; return -1; }
      got = (size_t)k;
      fd = -1;
    }
  }
  if (fd >= 0) {
    *stream_fd = fd;
    while (got < sizeof h) {
      const ssize_t k = read(fd, h + got, sizeof h - got);
      if (k < 0 && errno == EINTR) continue;
      if (k < 0) { err = "cannot read the input"; return -1; }
      if (k == 0) break;
      got += (size_t)k;
    }
    peek.assign((const char *)h, got);
  }
  if (got == 0) { err = "empty input"; return -1; }
  if (got >= 2 && h[0] == 0x1f && h[1] == 0x8b) {
    if (got >= 14 && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C') return 0;
    err = "gzip-compressed input is not supported (plain SAM, or BAM)";
    return -1;
  }
  return 1;
}

}  // namespace

std::unique_ptr<Input> open_input(const Options &o, std::string &err) {
  std::string peek, e;
  int stream_fd = -1;
  const int kind = sniff_input(o.in_bam, &stream_fd, peek, e);
  if (kind < 0) { if (stream_fd > 0) close(stream_fd); err = o.in_bam + ": " + e; return nullptr; }
  if (kind == 1) return open_sam(o, stream_fd, peek, err);
  auto f = std::make_unique<BamFile>();
  BamHeader hdr;
  if (!f->rd.open(o.in_bam.c_str(), o.threads, peek, stream_fd)) { err = f->rd.error(); return nullptr; }
  if (!read_header(f->rd, f->buf, f->pos, hdr, e)) { err = o.in_bam + ": " + e; return nullptr; }
  int dev_reader = o.device_reader;
  if (dev_reader < 0) if (const char *v = getenv("BRAMBLE_AMD_DEVICE_READER")) dev_reader = atoi(v) != 0;   // (A/B with one command line: the @PG line quotes it)
  const bool on_device = dev_reader != 0 && f->rd.mapped() && (dev_reader > 0 || f->rd.mapped_size() >= (1u << 20));
  std::unique_ptr<Input> in;
  if (on_device) in.reset(new DevBamInput(o, std::move(f)));
  else in.reset(new HostBamInput(o, std::move(f)));
  in->hdr = std::move(hdr);
  return in;
}

}  // namespace brcli
