// --quant-bam FILE [--quant-bam-mode tag|sample] (cli_output.h): the projected records of the run with the EM's posterior on them,
// as a second BAM under the header the main output has without --sort.  Every bundle's rows, names and records go to a br_assign
// (br_assign_add_last: the records are copied inside HBM, the main output streams as before); after the last bundle it finishes
// with the --quant consumer's quantifier, which it met through Consumer::quantifier when the consumers were opened (quant's
// finish() runs first: open_consumers' order); once the writer thread has joined and the context is idle, the rewritten records
// are drawn in pieces (br_assign_next -> br_device_bam_download) into a BGZF writer of its own, as --unprojected writes its file.
#include "cli_output.h"

namespace brcli {
namespace {

class AssignOut : public Consumer {
 public:
  explicit AssignOut(const RunEnv &e) : Consumer(e, "posterior BAM", "the posterior BAM"), file(e.o.quant_bam) {}
  ~AssignOut() override {
    if (opened) { wr.abandon(); remove(file.tmp.c_str()); }   // (a set-up error elsewhere: no settle came)
    if (a) br_assign_free(a);
  }
  // the file is begun here, in front of the run: a path that cannot be written fails before anything is projected
  bool open(std::string &err) {
    if (!wr.open(file.tmp.c_str(), env.o.threads, env.o.level)) { err = wr.error(); return false; }
    opened = true;
    if (!wr.write(env.out_header.data(), env.out_header.size())) { err = wr.error(); return false; }
    const Options &o = env.o;
    int rc = br_assign_new(env.device, &a);
    if (!rc) rc = br_assign_set_param(a, "mode", o.quant_bam_mode);
    if (!rc) rc = br_assign_set_param(a, "seed", (int64_t)o.quant_seed);
    if (!rc) rc = br_assign_set_param(a, "long_reads", o.cfg.lr || o.cfg.lr_hq ? 1 : 0);
    if (rc) { err = std::string(name) + " on device " + std::to_string(env.device) + ": " + br_strerror(rc); return false; }
    return true;
  }
  bool meet(const std::vector<std::unique_ptr<Consumer>> &all) override {
    for (auto &other : all) if (br_quant *q = other->quantifier()) quant = q;
    return quant != nullptr;
  }
  int add(br_ctx *c) override {
    ctx = c;
    br_device_bam db;
    if (br_ctx_last_device_bam(c, &db) == BR_OK) n_in += db.n_rows;
    return br_assign_add_last(a, c);
  }
  int finish() override {
    const int rc = br_assign_finish(a, quant, &n_out, &n_names);
    (void)br_assign_stats(a, nullptr, nullptr, &t_add, &t_finish, nullptr, nullptr);
    return rc;
  }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    int rc = 0;
    bool ok = true;
    while (ctx && ok) {
      br_device_bam piece;
      br_host_bam hb;
      if ((rc = br_assign_next(a, PIECE, &piece)) || piece.n_rows == 0) break;
      if ((rc = br_device_bam_download(ctx, &piece, env.o.device_deflate ? 1 : 0, 0, &hb))) break;
      ok = env.o.device_deflate ? wr.write_raw(hb.data, (size_t)hb.n_bytes) : wr.write(hb.data, (size_t)hb.n_bytes);
      written += (uint64_t)piece.n_rows;
    }
    if (rc) fprintf(stderr, "error: posterior BAM on device %d: %s\n", env.device, br_strerror(rc));
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
    printf("[bramble] posterior BAM: %llu of %lld records written for %lld read names (mode %s; add %.2fs, weigh %.2fs)\n", (unsigned long long)written,
           (long long)n_in, (long long)n_names, env.o.quant_bam_mode ? "sample" : "tag", t_add, t_finish);
  }
 private:
  static constexpr uint64_t PIECE = 128ull << 20;   // record bytes per piece (one deflate call and one download)
  br_assign *a = nullptr;
  br_quant *quant = nullptr;   // the --quant consumer's, which outlives neither of the two
  br_ctx *ctx = nullptr;
  SideFile file;
  brio::BgzfWriter wr;
  bool opened = false, closed = false;
  int64_t n_in = 0, n_out = 0, n_names = 0;   // records of all bundles, records to write, names with records
  uint64_t written = 0;
  double t_add = 0, t_finish = 0;
};

}  // namespace

std::unique_ptr<Consumer> open_assign(const RunEnv &env, std::string &err) {
  auto c = std::make_unique<AssignOut>(env);
  if (!c->open(err)) return nullptr;
  return c;
}

}  // namespace brcli
