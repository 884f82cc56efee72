// --unprojected FILE [--unprojected-scope record|name] (cli_output.h): the input records that got no output record, as a BAM
// under the input's header.  The library keeps them in worker 0's context while the bundles are projected ("keep_unprojected",
// set where the contexts are made); this consumer only remembers that context, reads the counters after the last bundle and,
// once the writer thread has joined and the context is idle, draws the records in pieces (br_ctx_unprojected_next ->
// br_device_bam_download) into a BGZF writer of its own.
#include "cli_output.h"

namespace brcli {
namespace {

class UnprojectedOut : public Consumer {
 public:
  explicit UnprojectedOut(const RunEnv &e) : Consumer(e, "unprojected records", "writing the unprojected records"), file(e.o.unprojected) {}
  ~UnprojectedOut() override { if (opened) { wr.abandon(); remove(file.tmp.c_str()); } }   // (a set-up error elsewhere: no settle came)
  // the file is begun here, in front of the run: a path that cannot be written fails before anything is projected
  bool open(std::string &err) {
    if (!wr.open(file.tmp.c_str(), env.o.threads, env.o.level)) { err = wr.error(); return false; }
    opened = true;
    const BamHeader &h = env.hdr;
    std::vector<uint8_t> b;
    auto p32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); };
    b.insert(b.end(), {'B', 'A', 'M', 1});
    p32((uint32_t)h.text.size()); b.insert(b.end(), h.text.begin(), h.text.end());
    p32((uint32_t)h.ref_names.size());
    for (size_t r = 0; r < h.ref_names.size(); r++) {
      p32((uint32_t)h.ref_names[r].size() + 1);
      b.insert(b.end(), h.ref_names[r].begin(), h.ref_names[r].end()); b.push_back(0);
      p32(r < h.ref_lens.size() ? h.ref_lens[r] : 0);
    }
    if (!wr.write(b.data(), b.size())) { err = wr.error(); return false; }
    return true;
  }
  int add(br_ctx *c) override { ctx = c; return BR_OK; }
  int finish() override { return ctx ? br_ctx_unprojected_stats(ctx, stats) : BR_OK; }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    int rc = 0;
    bool ok = true;
    while (ctx && ok) {
      br_device_bam piece;
      br_host_bam hb;
      if ((rc = br_ctx_unprojected_next(ctx, PIECE, &piece)) || piece.n_rows == 0) break;
      if ((rc = br_device_bam_download(ctx, &piece, env.o.device_deflate ? 1 : 0, 0, &hb))) break;
      ok = env.o.device_deflate ? wr.write_raw(hb.data, (size_t)hb.n_bytes) : wr.write(hb.data, (size_t)hb.n_bytes);
      written += (uint64_t)piece.n_rows;
    }
    if (rc) fprintf(stderr, "error: unprojected records on device %d: %s\n", env.device, br_strerror(rc));
    if (!rc && ok) ok = wr.close(); else wr.abandon();
    if (!ok) fprintf(stderr, "error: %s: %s\n", file.path.c_str(), wr.error().c_str());
    closed = true;
    return !rc && ok;
  }
  bool settle(bool failed) override {
    if (!closed) wr.abandon();
    opened = false;
    return file.settle(failed);
  }
  void report() const override {
    printf("[bramble] unprojected: %llu of %llu records written (%llu read names without a projected record, %llu partly projected; scope %s)\n",
           (unsigned long long)written, (unsigned long long)stats[0], (unsigned long long)stats[4], (unsigned long long)stats[5],
           env.o.unprojected_scope == 2 ? "name" : "record");
  }
 private:
  static constexpr uint64_t PIECE = 128ull << 20;   // record bytes per piece (one deflate call and one download)
  br_ctx *ctx = nullptr;
  SideFile file;
  brio::BgzfWriter wr;
  bool opened = false, closed = false;
  uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}, written = 0;
};

}  // namespace

std::unique_ptr<Consumer> open_unprojected(const RunEnv &env, std::string &err) {
  auto c = std::make_unique<UnprojectedOut>(env);
  if (!c->open(err)) return nullptr;
  return c;
}

}  // namespace brcli
