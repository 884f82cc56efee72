// --dedup unique|directional and its switches (cli_output.h): every bundle's rows, names and records go to a br_dedup
// (br_dedup_add_last; with --dedup-bam the records are copied inside HBM, the main output streams as before); after the last bundle
// it decides which read names are PCR copies.  Its finish() runs in front of the --quant consumer's (open_consumers' order), which
// met it through Consumer::duplicate_flags and drops the duplicate names before its classes are made: --quant then quantifies
// molecules.  --dedup-stats: the molecules' size histogram; --dedup-bam: once the writer thread has joined and the context is idle,
// the records without the duplicate names' (mode remove) or with 0x400 set on them (mode mark) are drawn in pieces (br_dedup_next ->
// br_device_bam_download) into a BGZF writer of its own, under the header the main output has without --sort, as --quant-bam writes
// its file.
#include "cli_output.h"

namespace brcli {
namespace {

class DedupOut : public Consumer {
 public:
  explicit DedupOut(const RunEnv &e) : Consumer(e, "duplicate removal", "duplicate removal"), stats(e.o.dedup_stats), file(e.o.dedup_bam) {}
  ~DedupOut() override {
    if (opened) { wr.abandon(); remove(file.tmp.c_str()); }   // (a set-up error elsewhere: no settle came)
    if (d) br_dedup_free(d);
  }
  // the BAM is begun here, in front of the run: a path that cannot be written fails before anything is projected
  bool open(std::string &err) {
    const Options &o = env.o;
    if (!file.path.empty()) {
      if (!wr.open(file.tmp.c_str(), o.threads, o.level)) { err = wr.error(); return false; }
      opened = true;
      if (!wr.write(env.out_header.data(), env.out_header.size())) { err = wr.error(); return false; }
    }
    int rc = br_dedup_new(env.device, &d);
    if (!rc) rc = br_dedup_set_param(d, "method", o.dedup);
    if (!rc) rc = br_dedup_set_param(d, "umi_source", o.dedup_umi);
    if (!rc) rc = br_dedup_set_param(d, "umi_sep", o.dedup_umi_sep);
    if (!rc) rc = br_dedup_set_param(d, "umi_tag", o.dedup_umi_tag);
    if (!rc && !o.cells.empty()) rc = br_dedup_set_param(d, "cell_source", 1 + o.cells_barcode);   // (--cells: duplicates per cell)
    if (!rc && !o.cells.empty()) rc = br_dedup_set_param(d, "cell_tag", o.cells_barcode_tag);
    if (!rc && !file.path.empty()) rc = br_dedup_set_param(d, "keep_records", 1);
    if (!rc && !file.path.empty()) rc = br_dedup_set_param(d, "mark", o.dedup_bam_mode);
    if (rc) { err = std::string(name) + " on device " + std::to_string(env.device) + ": " + br_strerror(rc); return false; }
    return true;
  }
  // --cells-whitelist: the per-cell groups are made from the barcodes the cells consumer's whitelist resolves
  bool meet(const std::vector<std::unique_ptr<Consumer>> &all) override {
    for (auto &other : all) {
      int correct = 0;
      if (const br_whitelist *wl = other->whitelist(&correct)) if (br_dedup_set_whitelist(d, wl, correct)) return false;
    }
    return true;
  }
  int add(br_ctx *c) override { ctx = c; return br_dedup_add_last(d, c); }
  int finish() override {
    int rc = br_dedup_finish(d, &n_names, &n_molecules, &n_duplicates);
    if (!rc && !stats.path.empty()) { hist.resize(HIST_MAX + 1); rc = br_dedup_hist(d, hist.data()); }
    (void)br_dedup_stats(d, st);
    return rc;
  }
  int duplicate_flags(const uint8_t **flags, int64_t *n) override { return br_dedup_flags(d, flags, n); }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    if (FILE *f = stats.open()) for (size_t s = 0; s < hist.size(); s++) if (hist[s]) fprintf(f, "%zu\t%llu\n", s, (unsigned long long)hist[s]);
    if (!stats.close()) return false;
    if (file.path.empty()) return true;
    int rc = 0;
    bool ok = true;
    while (ctx && ok) {
      br_device_bam piece;
      br_host_bam hb;
      if ((rc = br_dedup_next(d, PIECE, &piece)) || piece.n_rows == 0) break;
      if ((rc = br_device_bam_download(ctx, &piece, env.o.device_deflate ? 1 : 0, 0, &hb))) break;
      ok = env.o.device_deflate ? wr.write_raw(hb.data, (size_t)hb.n_bytes) : wr.write(hb.data, (size_t)hb.n_bytes);
    }
    if (rc) fprintf(stderr, "error: duplicate removal on device %d: %s\n", env.device, br_strerror(rc));
    if (!rc && ok) ok = wr.close(); else wr.abandon();
    if (!ok) fprintf(stderr, "error: %s: %s\n", file.path.c_str(), wr.error().c_str());
    closed = true;
    return !rc && ok;
  }
  bool settle(bool failed) override {
    if (opened && !closed) wr.abandon();
    opened = false;
    return settle_all({&stats, &file}, failed);
  }
  void report() const override {
    printf("[bramble] dedup: %lld molecules of %lld read names (%lld duplicates, %llu without UMI; %llu position groups; method %s; add %.2fs, finish %.2fs)\n",
           (long long)n_molecules, (long long)n_names, (long long)n_duplicates, (unsigned long long)st[2], (unsigned long long)st[5],
           env.o.dedup ? "directional" : "unique", (double)st[13] * 1e-6, (double)st[14] * 1e-6);
  }
 private:
  static constexpr uint64_t PIECE = 128ull << 20;   // record bytes per piece (one deflate call and one download)
  static constexpr size_t HIST_MAX = 1000;          // br_dedup's default "hist_max"
  br_dedup *d = nullptr;
  br_ctx *ctx = nullptr;
  SideFile stats, file;
  brio::BgzfWriter wr;
  bool opened = false, closed = false;
  int64_t n_names = 0, n_molecules = 0, n_duplicates = 0;
  uint64_t st[16] = {};
  std::vector<uint64_t> hist;
};

}  // namespace

std::unique_ptr<Consumer> open_dedup(const RunEnv &env, std::string &err) {
  auto c = std::make_unique<DedupOut>(env);
  if (!c->open(err)) return nullptr;
  return c;
}

}  // namespace brcli
