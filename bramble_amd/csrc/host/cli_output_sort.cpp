// --sort [--write-index] (cli_output.h): every bundle's records, left in HBM by the projection, go into a br_sorter; after the
// last bundle the writer draws the sorted pieces from it, and br_sorter_index builds <out>.bai from the blocks the writer noted.
#include "cli_output.h"

namespace brcli {
namespace {

class SortOut : public Consumer {
 public:
  explicit SortOut(const RunEnv &e) : Consumer(e, "sorter", "sorting"), bai(e.o.write_index ? e.o.out_bam + ".bai" : "") {}
  ~SortOut() override { if (s) br_sorter_free(s); }
  int open() { return br_sorter_new(env.device, &s); }
  bool keeps_records() const override { return true; }
  int add(br_ctx *ctx) override {   // (the runner sees the bundles in order)
    br_device_bam db;
    const int rc = br_ctx_last_device_bam(ctx, &db);
    return rc ? rc : br_sorter_add(s, &db, 1, nullptr);
  }
  int finish() override {
    const int rc = br_sorter_finish(s, &n_records);
    (void)br_sorter_stats(s, nullptr, nullptr, &t_add, &t_finish, nullptr);
    return rc;
  }
  int next_piece(uint64_t max_bytes, br_device_bam *piece) override { return br_sorter_next(s, max_bytes, piece); }
  bool write_files(brio::BgzfWriter &wr, const std::vector<br_bgzf_span> &spans) override {   // the index of the blocks just written
    if (bai.path.empty()) return true;
    uint8_t *buf = nullptr; uint64_t n = 0;
    const int rc = wr.flush() ? br_sorter_index(s, (int32_t)env.tx.n_sq, spans.data(), (int64_t)spans.size(), wr.bytes_out(), &buf, &n) : BR_ERR_INVALID_ARG;
    if (rc) { fprintf(stderr, "error: %s: index: %s\n", bai.path.c_str(), br_strerror(rc)); return false; }
    FILE *f = bai.open(true);
    const bool whole = f && fwrite(buf, 1, (size_t)n, f) == (size_t)n;   // (a short write leaves the stream's error flag up: close() says so)
    br_free_buffer(buf);
    return bai.close() && whole;
  }
  bool settle(bool failed) override { return bai.settle(failed); }
  void report() const override {
    printf("[bramble] sorted %lld records by coordinate on device %d (add %.2fs, sort %.2fs)%s\n", (long long)n_records, env.device, t_add, t_finish,
           bai.path.empty() ? "" : ", index written");
  }
 private:
  br_sorter *s = nullptr;
  SideFile bai;
  int64_t n_records = 0;
  double t_add = 0, t_finish = 0;
};

}  // namespace

std::unique_ptr<Consumer> open_sort(const RunEnv &env, std::string &err) { return open_as<SortOut>(env, err); }

}  // namespace brcli
