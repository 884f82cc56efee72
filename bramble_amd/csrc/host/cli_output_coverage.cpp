// --coverage / --coverage-summary (cli_output.h): every bundle's rows go to a br_coverage (br_coverage_add_last); after the last
// bundle: depth, summary and runs on the device; the per-transcript table comes home then, the runs in pages while the bedGraph
// is written.
#include "cli_output.h"

namespace brcli {
namespace {

class CoverageOut : public Consumer {
 public:
  explicit CoverageOut(const RunEnv &e) : Consumer(e, "coverage", "coverage"), bedgraph(e.o.coverage), summary(e.o.coverage_summary) {}
  ~CoverageOut() override { if (c) br_coverage_free(c); }
  int open() {
    int rc = br_coverage_new(env.device, (int64_t)env.tx.len.size(), env.tx.len.data(), &c);
    if (!rc && env.o.coverage_primary) rc = br_coverage_set_param(c, "primary_only", 1);
    return rc;
  }
  int add(br_ctx *ctx) override { return br_coverage_add_last(c, ctx); }
  int finish() override {
    const size_t nt = env.tx.len.size();
    int rc = br_coverage_finish(c, &n_runs);
    if (!rc) {
      records.resize(nt + 1); aligned.resize(nt + 1); covered.resize(nt + 1); max_depth.resize(nt + 1);
      rc = br_coverage_summary(c, records.data(), aligned.data(), covered.data(), max_depth.data());
    }
    (void)br_coverage_stats(c, nullptr, nullptr, nullptr, nullptr, nullptr, &t_add, &t_finish);
    return rc;
  }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    int rc = 0;
    if (FILE *f = bedgraph.open())
      rc = write_bedgraph(f, env.tx, n_runs, 1 << 20, [this](int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
        return br_coverage_runs(c, first, n, tid, start, end, depth);
      });
    if (rc) fprintf(stderr, "error: coverage on device %d: %s\n", env.device, br_strerror(rc));
    if (!bedgraph.close() || rc) return false;
    if (FILE *f = summary.open()) write_coverage_summary(f, env.tx, records, aligned, covered, max_depth);
    return summary.close();
  }
  bool settle(bool failed) override { return settle_all({&bedgraph, &summary}, failed); }
  void report() const override {
    uint64_t n = 0, a = 0, cv = 0, b = 0;
    for (size_t t = 0; t < env.tx.len.size(); t++) { n += records[t]; a += aligned[t]; cv += covered[t]; b += (uint64_t)std::max<int64_t>(env.tx.len[t], 0); }
    printf("[bramble] coverage: %llu records, %llu aligned bases on %llu of %llu bases in %lld runs (add %.2fs, finish %.2fs)\n", (unsigned long long)n,
           (unsigned long long)a, (unsigned long long)cv, (unsigned long long)b, (long long)n_runs, t_add, t_finish);
  }
 private:
  br_coverage *c = nullptr;
  SideFile bedgraph, summary;
  int64_t n_runs = 0;
  double t_add = 0, t_finish = 0;
  std::vector<uint64_t> records, aligned, covered;
  std::vector<uint32_t> max_depth;
};

}  // namespace

std::unique_ptr<Consumer> open_coverage(const RunEnv &env, std::string &err) { return open_as<CoverageOut>(env, err); }

}  // namespace brcli
