// --quant and its switches (cli_output.h): every bundle's rows go to a br_quant (br_quant_add_last; --quant-eff-length: the adds
// count the fragment lengths as well, "eff_len"); after the last bundle: classes, EM, and everything the three files need in one
// download each -- the table, --quant-classes, --quant-fld; with --quant-bootstraps the replicates run behind the EM
// (br_quant_bootstrap) and their summary joins the table, their values --quant-boot-out; with --quant-genes the gene tables are
// made last (br_quant_genes on the numbers env.tx gives the genes) and go to --quant-genes and --quant-gene-classes; --quant-vb
// turns the variational Bayes EM on ("vb") for all of them.  Beside --dedup the names that consumer has found to be duplicates are
// dropped in front of the classes (br_quant_drop_names with its flags, from where they lie in HBM): the file's numbers are molecules.
#include "cli_output.h"

namespace brcli {
namespace {

class QuantOut : public Consumer {
 public:
  explicit QuantOut(const RunEnv &e) : Consumer(e, "quantifier", "quantification"), table(e.o.quant), classes(e.o.quant_classes), fld(e.o.quant_fld), boot(e.o.quant_boot_out), genes(e.o.quant_genes), gene_classes(e.o.quant_gene_classes) {}
  ~QuantOut() override { if (q) br_quant_free(q); }
  int open() {
    const Options &o = env.o;
    int rc = br_quant_new(env.device, (int64_t)env.tx.len.size(), env.tx.len.data(), &q);
    const int norm = o.quant_length_norm >= 0 ? o.quant_length_norm : (o.cfg.lr || o.cfg.lr_hq) ? 0 : 1;   // (oarfish does not length-normalise long reads)
    if (!rc) rc = br_quant_set_param(q, "length_norm", norm);
    if (!rc && o.quant_eff_length) rc = br_quant_set_param(q, "eff_len", 1);
    if (!rc && o.quant_bootstraps) rc = br_quant_set_param(q, "bootstraps", o.quant_bootstraps);
    if (!rc && o.quant_bootstraps) rc = br_quant_set_param(q, "boot_seed", (int64_t)o.quant_seed);
    if (!rc && o.quant_vb) rc = br_quant_set_param(q, "vb", 1);
    if (!rc && o.quant_vb) rc = br_quant_set_vb_prior(q, o.quant_vb_prior);
    if (!rc && o.quant_vb_per_nt) rc = br_quant_set_param(q, "vb_per_nucleotide", 1);
    if (!rc && (o.coverage_weight == 2 || !o.quant_bam.empty() || !o.cells.empty())) rc = br_quant_set_param(q, "keep_names", 1);   // (the coverage, posterior-BAM and cells consumers join names to classes)
    return rc;
  }
  int add(br_ctx *ctx) override { return br_quant_add_last(q, ctx); }
  br_quant *quantifier() override { return q; }
  bool meet(const std::vector<std::unique_ptr<Consumer>> &all) override {
    for (auto &other : all) if (other->duplicate_flags(nullptr, nullptr) != BR_ERR_UNSUPPORTED) dedup = other.get();
    return dedup != nullptr || env.o.dedup < 0;
  }
  int finish() override {
    const size_t nt = env.tx.len.size();
    int rc = BR_OK;
    if (dedup) {   // (its finish() has run)
      const uint8_t *flags = nullptr; int64_t n = 0;
      rc = dedup->duplicate_flags(&flags, &n);
      if (!rc) rc = br_quant_drop_names(q, flags, n, 1, nullptr);
    }
    if (!rc) rc = br_quant_finish(q, &n_names, &n_classes);
    if (!rc) rc = br_quant_em(q, &n_iters, nullptr);
    if (!rc) {
      theta.resize(nt + 1); tpm.resize(nt + 1); unique.resize(nt + 1); ambig.resize(nt + 1);
      rc = br_quant_result(q, theta.data(), tpm.data(), unique.data(), ambig.data());
    }
    if (!rc && env.o.quant_eff_length) {
      eff.resize(nt + 1); hist.resize(FLD_MAX + 1);
      rc = br_quant_eff_lengths(q, eff.data());
      if (!rc) rc = br_quant_fld(q, hist.data(), &fld_obs, &fld_nofrag, &fld_oor);
    }
    if (const int n_boot = env.o.quant_bootstraps; !rc && n_boot) {
      rc = br_quant_bootstrap(q, nullptr);
      boot_mean.resize(nt + 1); boot_var.resize(nt + 1);
      if (!rc) rc = br_quant_boot_summary(q, boot_mean.data(), boot_var.data());
      if (!rc && !boot.path.empty()) {
        boot_theta.resize((size_t)n_boot * nt + 1);
        rc = br_quant_boot_theta(q, 0, n_boot, boot_theta.data());
      }
      if (!rc) rc = br_quant_boot_stats(q, &t_boot_sample, &t_boot_em, &boot_iters);
    }
    if (!rc && !classes.path.empty()) {
      int64_t n_labels = 0;
      rc = br_quant_stats(q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_labels);
      label_off.resize((size_t)n_classes + 1); counts.resize((size_t)n_classes + 1); labels.resize((size_t)n_labels + 1);
      if (!rc) rc = br_quant_classes(q, label_off.data(), labels.data(), counts.data(), nullptr);
    }
    if (!rc && !genes.path.empty()) {
      const size_t ng = env.tx.gene_name.size();
      rc = br_quant_genes(q, env.tx.gene_of.data(), (int64_t)ng, &n_gene_classes);
      g_len.resize(ng + 1); g_reads.resize(ng + 1); g_tpm.resize(ng + 1); g_unique.resize(ng + 1); g_ambig.resize(ng + 1); g_ntx.resize(ng + 1);
      if (env.o.quant_eff_length) g_eff.resize(ng + 1);
      if (!rc) rc = br_quant_gene_result(q, g_reads.data(), g_tpm.data(), g_len.data(), env.o.quant_eff_length ? g_eff.data() : nullptr, g_unique.data(),
                                         g_ambig.data(), g_ntx.data());
      if (!rc && env.o.quant_bootstraps) {
        g_boot_mean.resize(ng + 1); g_boot_var.resize(ng + 1);
        rc = br_quant_gene_boot_summary(q, g_boot_mean.data(), g_boot_var.data());
      }
      int64_t n_labels = 0;
      if (!rc) rc = br_quant_gene_stats(q, &t_genes, &n_labels, nullptr);
      if (!rc && !gene_classes.path.empty()) {
        g_label_off.resize((size_t)n_gene_classes + 1); g_counts.resize((size_t)n_gene_classes + 1); g_labels.resize((size_t)n_labels + 1);
        rc = br_quant_gene_classes(q, g_label_off.data(), g_labels.data(), g_counts.data(), nullptr);
      }
    }
    (void)br_quant_stats(q, nullptr, nullptr, &t_add, &t_finish, &t_em, nullptr, nullptr, nullptr);
    return rc;
  }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    const bool with_boot = env.o.quant_bootstraps > 0;
    if (FILE *f = table.open()) write_quant_table(f, env.tx, env.o.quant_eff_length ? &eff : nullptr, theta, tpm, unique, ambig, with_boot ? &boot_mean : nullptr,
                                                  with_boot ? &boot_var : nullptr);
    if (!table.close()) return false;
    if (FILE *f = classes.open()) write_quant_classes(f, env.tx, n_classes, label_off, labels, counts);
    if (!classes.close()) return false;
    if (FILE *f = fld.open()) write_fragment_lengths(f, hist);
    if (!fld.close()) return false;
    if (FILE *f = boot.open()) write_quant_bootstraps(f, env.tx, env.o.quant_bootstraps, boot_theta);
    if (!boot.close()) return false;
    if (FILE *f = genes.open()) write_quant_gene_table(f, env.tx, g_len, env.o.quant_eff_length ? &g_eff : nullptr, g_reads, g_tpm, g_unique, g_ambig, g_ntx,
                                                       with_boot ? &g_boot_mean : nullptr, with_boot ? &g_boot_var : nullptr);
    if (!genes.close()) return false;
    if (FILE *f = gene_classes.open()) write_quant_gene_classes(f, env.tx, n_gene_classes, g_label_off, g_labels, g_counts);
    return gene_classes.close();
  }
  bool settle(bool failed) override { return settle_all({&table, &classes, &fld, &boot, &genes, &gene_classes}, failed); }
  void report() const override {
    if (env.o.quant_eff_length) {
      double sum = 0;
      for (size_t k = 0; k < hist.size(); k++) sum += (double)k * (double)hist[k];
      printf("[bramble] fragment lengths: %llu observed, mean %.1f, %llu unique names without a pair, %llu out of range\n", (unsigned long long)fld_obs,
             fld_obs ? sum / (double)fld_obs : 0.0, (unsigned long long)fld_nofrag, (unsigned long long)fld_oor);
    }
    if (env.o.quant_bootstraps)
      printf("[bramble] bootstrapped %d replicates (seed %lld, %lld iterations in all, sampling %.2fs, EM %.2fs)\n", env.o.quant_bootstraps, env.o.quant_seed,
             (long long)boot_iters, t_boot_sample, t_boot_em);
    if (env.o.quant_vb) {
      size_t at_zero = 0;
      for (size_t t = 0; t < env.tx.len.size(); t++) at_zero += theta[t] <= 1e-8;
      printf("[bramble] variational Bayes: prior %g per %s, %zu transcripts at zero\n", env.o.quant_vb_prior, env.o.quant_vb_per_nt ? "nucleotide" : "transcript", at_zero);
    }
    if (!genes.path.empty()) printf("[bramble] gene level: %zu genes, %lld classes (%.2fs)\n", env.tx.gene_name.size(), (long long)n_gene_classes, t_genes);
    printf("[bramble] quantified %lld read names in %lld classes (%d iterations, add %.2fs, classes %.2fs, EM %.2fs)\n", (long long)n_names, (long long)n_classes,
           (int)n_iters, t_add, t_finish, t_em);
  }
 private:
  static constexpr size_t FLD_MAX = 1000;   // br_quant's default "fld_max"
  br_quant *q = nullptr;
  Consumer *dedup = nullptr;   // the --dedup consumer, which outlives neither of the two
  SideFile table, classes, fld, boot, genes, gene_classes;
  int64_t n_names = 0, n_classes = 0; int32_t n_iters = 0;
  double t_add = 0, t_finish = 0, t_em = 0;
  std::vector<double> theta, tpm, eff, boot_mean, boot_var, boot_theta;   // boot_*: --quant-bootstraps (boot_theta: one row a replicate)
  double t_boot_sample = 0, t_boot_em = 0; int64_t boot_iters = 0;
  std::vector<uint64_t> unique, ambig, label_off, counts, hist;   // hist, eff: --quant-eff-length
  std::vector<uint32_t> labels;
  uint64_t fld_obs = 0, fld_nofrag = 0, fld_oor = 0;
  // --quant-genes: per gene, and the gene classes
  int64_t n_gene_classes = 0; double t_genes = 0;
  std::vector<double> g_len, g_eff, g_reads, g_tpm, g_boot_mean, g_boot_var;
  std::vector<uint64_t> g_unique, g_ambig, g_label_off, g_counts;
  std::vector<uint32_t> g_ntx, g_labels;
};

}  // namespace

std::unique_ptr<Consumer> open_quant(const RunEnv &env, std::string &err) { return open_as<QuantOut>(env, err); }

}  // namespace brcli
