// --coverage / --coverage-summary (cli_output.h): every bundle's rows go to a br_coverage (br_coverage_add_last); after the last
// bundle: depth, summary and runs on the device; the per-transcript table comes home then, the runs in pages while the bedGraph
// is written.  --coverage-weight nh|em: the object's "weight" 1 / 2, the 64-bit getters and the weighted files; em keeps every bundle's
// rows by name and finishes with the --quant consumer's quantifier, which it met through Consumer::quantifier when the consumers
// were opened (quant's finish() runs first: open_consumers' order).  --coverage-bigwig: after the finish the track is built and
// compressed on the device (br_coverage_bigwig) and comes home in pieces of 64 MiB while the file is written.
#include "cli_output.h"

namespace brcli {
namespace {

class CoverageOut : public Consumer {
 public:
  explicit CoverageOut(const RunEnv &e) : Consumer(e, "coverage", "coverage"), bedgraph(e.o.coverage), summary(e.o.coverage_summary), bigwig(e.o.coverage_bigwig) {}
  ~CoverageOut() override { if (c) br_coverage_free(c); }
  int open() {
    int rc = br_coverage_new(env.device, (int64_t)env.tx.len.size(), env.tx.len.data(), &c);
    if (!rc && env.o.coverage_primary) rc = br_coverage_set_param(c, "primary_only", 1);
    if (!rc && weight) rc = br_coverage_set_param(c, "weight", weight);
    return rc;
  }
  bool meet(const std::vector<std::unique_ptr<Consumer>> &all) override {
    if (weight != 2) return true;
    for (auto &other : all) if (br_quant *q = other->quantifier()) quant = q;
    return quant != nullptr;
  }
  int add(br_ctx *ctx) override { return br_coverage_add_last(c, ctx); }
  int finish() override {
    const size_t nt = env.tx.len.size();
    int rc = weight == 2 ? br_coverage_finish_em(c, quant, &n_runs) : br_coverage_finish(c, &n_runs);
    if (!rc) {
      records.resize(nt + 1); aligned.resize(nt + 1); covered.resize(nt + 1); max_depth.resize(nt + 1);
      if (weight) {
        weight_sum.resize(nt + 1); aligned_lo.resize(nt + 1); max_depth64.resize(nt + 1);
        rc = br_coverage_summary64(c, records.data(), weight_sum.data(), aligned.data(), aligned_lo.data(), covered.data(), max_depth64.data());
      } else rc = br_coverage_summary(c, records.data(), aligned.data(), covered.data(), max_depth.data());
    }
    (void)br_coverage_stats(c, nullptr, nullptr, nullptr, nullptr, nullptr, &t_add, &t_finish);
    if (!rc && !bigwig.path.empty()) {
      br_bigwig_opts bo{};
      bo.zoom_levels = env.o.coverage_bigwig_zooms ? env.o.coverage_bigwig_zooms : -1;
      bo.compress = env.o.coverage_bigwig_uncompressed ? -1 : 1;
      rc = br_coverage_bigwig(c, env.tx.name.data(), &bo, &bw_bytes);
      if (!rc) rc = br_coverage_bigwig_stats(c, &bw_chroms, &bw_sections, &bw_zooms, bw_records, &bw_raw, &bw_data, nullptr, &bw_seconds);
    }
    return rc;
  }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    int rc = 0;
    if (FILE *f = bedgraph.open()) {
      if (weight)
        rc = write_bedgraph_weighted(f, env.tx, n_runs, 1 << 20, [this](int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint64_t *depth) {
          return br_coverage_runs64(c, first, n, tid, start, end, depth);
        });
      else
        rc = write_bedgraph(f, env.tx, n_runs, 1 << 20, [this](int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
          return br_coverage_runs(c, first, n, tid, start, end, depth);
        });
    }
    if (rc) fprintf(stderr, "error: coverage on device %d: %s\n", env.device, br_strerror(rc));
    if (!bedgraph.close() || rc) return false;
    if (FILE *f = summary.open()) {
      if (weight) write_coverage_summary_weighted(f, env.tx, records, weight_sum, aligned, aligned_lo, covered, max_depth64);
      else write_coverage_summary(f, env.tx, records, aligned, covered, max_depth);
    }
    if (!summary.close()) return false;
    if (FILE *f = bigwig.open(true)) {
      constexpr uint64_t PIECE = 64ull << 20;
      std::vector<uint8_t> piece((size_t)std::min<uint64_t>(bw_bytes, PIECE));
      for (uint64_t at = 0; at < bw_bytes && !rc; at += PIECE) {
        const uint64_t n = std::min<uint64_t>(PIECE, bw_bytes - at);
        rc = br_coverage_bigwig_read(c, at, n, piece.data());
        if (!rc && fwrite(piece.data(), 1, (size_t)n, f) != (size_t)n) break;   // (close() reports the stream's error)
      }
      if (rc) fprintf(stderr, "error: coverage on device %d: %s\n", env.device, br_strerror(rc));
    }
    return bigwig.close() && !rc;
  }
  bool settle(bool failed) override { return settle_all({&bedgraph, &summary, &bigwig}, failed); }
  void report_bigwig() const {
    if (bigwig.path.empty()) return;
    printf("[bramble] bigwig: %llu transcripts, %llu sections of %lld runs, %d zoom levels (", (unsigned long long)bw_chroms,
           (unsigned long long)bw_sections, (long long)n_runs, (int)bw_zooms);
    for (int k = 0; k < bw_zooms; k++) printf("%s%llu", k ? ", " : "", (unsigned long long)bw_records[k]);
    printf(" records), %llu -> %llu bytes (build %.2fs)\n", (unsigned long long)bw_raw, (unsigned long long)bw_data, bw_seconds);
  }
  void report() const override {
    if (weight) {   // the aligned bases are fixed point here: the whole units, then the 2^-32 fractions
      uint64_t n = 0, cv = 0, b = 0;
      double a = 0, ws = 0;
      for (size_t t = 0; t < env.tx.len.size(); t++) {
        n += records[t]; cv += covered[t]; b += (uint64_t)std::max<int64_t>(env.tx.len[t], 0);
        a += (double)aligned[t] + (double)aligned_lo[t] / 4294967296.0; ws += (double)weight_sum[t] / 4294967296.0;
      }
      printf("[bramble] coverage (weight %s): %llu records of weight %.2f, %.2f aligned bases on %llu of %llu bases in %lld runs (add %.2fs, finish %.2fs)\n",
             weight == 1 ? "nh" : "em", (unsigned long long)n, ws, a, (unsigned long long)cv, (unsigned long long)b, (long long)n_runs, t_add, t_finish);
      report_bigwig();
      return;
    }
    uint64_t n = 0, a = 0, cv = 0, b = 0;
    for (size_t t = 0; t < env.tx.len.size(); t++) { n += records[t]; a += aligned[t]; cv += covered[t]; b += (uint64_t)std::max<int64_t>(env.tx.len[t], 0); }
    printf("[bramble] coverage: %llu records, %llu aligned bases on %llu of %llu bases in %lld runs (add %.2fs, finish %.2fs)\n", (unsigned long long)n,
           (unsigned long long)a, (unsigned long long)cv, (unsigned long long)b, (long long)n_runs, t_add, t_finish);
    report_bigwig();
  }
 private:
  br_coverage *c = nullptr;
  const int weight = env.o.coverage_weight;   // br_coverage's "weight"
  br_quant *quant = nullptr;                  // weight em: the --quant consumer's, which outlives neither of the two
  SideFile bedgraph, summary, bigwig;
  uint64_t bw_bytes = 0, bw_chroms = 0, bw_sections = 0, bw_raw = 0, bw_data = 0, bw_records[10] = {};   // --coverage-bigwig: br_coverage_bigwig_stats
  int32_t bw_zooms = 0;
  double bw_seconds = 0;
  int64_t n_runs = 0;
  double t_add = 0, t_finish = 0;
  std::vector<uint64_t> records, aligned, covered;
  std::vector<uint32_t> max_depth;
  std::vector<uint64_t> weight_sum, aligned_lo, max_depth64;   // the weighted modes (aligned holds aligned_hi there)
};

}  // namespace

std::unique_ptr<Consumer> open_coverage(const RunEnv &env, std::string &err) { return open_as<CoverageOut>(env, err); }

}  // namespace brcli
