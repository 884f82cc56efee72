// --cells PREFIX and its switches (cli_output.h): every bundle's names and records go to a br_cells (br_cells_add_last), which keeps
// the cell barcode of every read name.  Its finish() runs behind the --quant consumer's (open_consumers' order), which it met through
// Consumer::quantifier: the quantifier's classes per name (with --dedup: without the names that consumer found to be duplicates, per
// cell) become the sparse cell x feature matrix on the device, the features being the genes env.tx numbers or the @SQ transcripts.
// Four files through SideFiles: PREFIXmatrix.mtx, PREFIXbarcodes.tsv, PREFIXfeatures.tsv, PREFIXcells.tsv.
// --cells-filter METHOD: the br_cells keeps its unique counts ("call_counts"), and after its finish a br_cellcall calls the cells on them
// (br_cells_call); three more files: PREFIXfiltered_matrix.mtx, PREFIXfiltered_barcodes.tsv, PREFIXcalls.tsv.
// --cells-whitelist FILE: the list is read (whitelist_file.h) and the run's one br_whitelist built here, in front of the run; the
// br_cells gets it, and the --dedup consumer takes it from here (Consumer::whitelist) for its br_dedup.
#include "cli_output.h"
#include "whitelist_file.h"

namespace brcli {
namespace {

class CellsOut : public Consumer {
 public:
  explicit CellsOut(const RunEnv &e)
      : Consumer(e, "cell matrix", "the cell matrix"), matrix(e.o.cells + "matrix.mtx"), barcodes(e.o.cells + "barcodes.tsv"),
        features(e.o.cells + "features.tsv"), table(e.o.cells + "cells.tsv"),
        f_matrix(e.o.cells_filter >= 0 ? e.o.cells + "filtered_matrix.mtx" : std::string()),
        f_barcodes(e.o.cells_filter >= 0 ? e.o.cells + "filtered_barcodes.tsv" : std::string()),
        calls(e.o.cells_filter >= 0 ? e.o.cells + "calls.tsv" : std::string()) {}
  ~CellsOut() override {
    if (probed) remove(matrix.tmp.c_str());   // (a set-up error elsewhere: no settle came)
    if (c) br_cells_free(c);
    if (call) br_cellcall_free(call);
    if (wl) br_whitelist_free(wl);
  }
  // PREFIX is tried here, in front of the run: a directory that is not there fails before anything is projected
  bool open(std::string &err) {
    const Options &o = env.o;
    FILE *f = fopen(matrix.tmp.c_str(), "w");
    if (!f) { err = "--cells: could not write " + matrix.tmp + " (the directory of the prefix must exist)"; return false; }
    fclose(f);
    probed = true;
    std::vector<uint8_t> wl_cb, wl_len;
    if (!o.cells_whitelist.empty() && !read_whitelist_file(o.cells_whitelist, wl_cb, wl_len, err)) return false;
    int rc = br_cells_new(env.device, &c);
    if (!rc && !wl_len.empty()) rc = br_whitelist_new(env.device, wl_cb.data(), wl_len.data(), (int64_t)wl_len.size(), 0, &wl);
    if (!rc && wl) rc = br_cells_set_whitelist(c, wl, o.cells_correct);
    if (!rc) rc = br_cells_set_param(c, "barcode_source", o.cells_barcode);
    if (!rc) rc = br_cells_set_param(c, "barcode_sep", o.dedup_umi_sep);
    if (!rc) rc = br_cells_set_param(c, "barcode_tag", o.cells_barcode_tag);
    if (!rc) rc = br_cells_set_param(c, "mode", o.cells_multi);
    if (!rc && o.cells_filter >= 0) {
      rc = br_cells_set_param(c, "call_counts", 1);
      if (!rc) rc = br_cellcall_new(env.device, &call);
      const std::pair<const char *, long long> ints[] = {{"method", o.cells_filter}, {"expected", o.cells_expected}, {"ind_min", o.cells_ed_lo},
                                                         {"ind_max", o.cells_ed_hi}, {"umi_min", o.cells_ed_umi_min}, {"cand_max", o.cells_ed_candidates},
                                                         {"sims", o.cells_ed_sims}, {"seed", o.quant_seed}};
      const std::pair<const char *, double> reals[] = {{"percentile", o.cells_percentile}, {"ratio", o.cells_ratio}, {"umi_frac", o.cells_ed_umi_frac},
                                                       {"fdr", o.cells_ed_fdr}};
      for (auto &p : ints) if (!rc) rc = br_cellcall_set_param(call, p.first, p.second);
      for (auto &p : reals) if (!rc) rc = br_cellcall_set_real(call, p.first, p.second);
    }
    if (rc) { err = std::string(name) + " on device " + std::to_string(env.device) + ": " + br_strerror(rc); return false; }
    return true;
  }
  int add(br_ctx *ctx) override { return br_cells_add_last(c, ctx); }
  const br_whitelist *whitelist(int *correct) override { *correct = env.o.cells_correct; return wl; }
  bool meet(const std::vector<std::unique_ptr<Consumer>> &all) override {
    for (auto &other : all) if (other->quantifier()) quant = other.get();
    return quant != nullptr;
  }
  int finish() override {
    const bool genes = env.o.cells_features == 0;
    const size_t nt = env.tx.len.size();
    std::vector<uint32_t> tx_feature(nt + 1, 0);   // (a transcript outside the @SQ list has no rows: its entry is never read)
    for (size_t t = 0; t < nt; t++) tx_feature[t] = genes ? env.tx.gene_of[t] : env.tx.sq_of[t] >= 0 ? (uint32_t)env.tx.sq_of[t] : 0u;
    n_features = genes ? env.tx.gene_name.size() : (size_t)env.tx.n_sq;
    int64_t n_cells = 0, n_entries = 0;
    int rc = br_cells_finish(c, quant->quantifier(), tx_feature.data(), (int64_t)n_features, &n_cells, &n_entries);   // (the quantifier's finish() has run)
    if (!rc) {
      const size_t k = (size_t)n_cells, z = (size_t)n_entries;
      cb.resize(32 * k + 1); len.resize(k); names.resize(k + 1); unique.resize(k + 1); multi.resize(k + 1); n_feat.resize(k + 1); iters.resize(k + 1);
      cell_off.resize(k + 1); feature.resize(z + 1); value.resize(z + 1);
      rc = br_cells_cell_barcodes(c, 0, n_cells, cb.data(), len.data());
      if (!rc) rc = br_cells_cell_stats(c, 0, n_cells, names.data(), unique.data(), multi.data(), n_feat.data(), iters.data());
      if (!rc) rc = br_cells_matrix(c, 0, n_cells, cell_off.data(), feature.data(), value.data());
      if (!rc && wl) {   // Corrected: the counted names of the cell whose status is 2
        const size_t n = (size_t)st_names();
        std::vector<uint8_t> status(n + 1);
        std::vector<uint32_t> cell(n + 1);
        rc = br_cells_name_status(c, 0, (int64_t)n, status.data());
        if (!rc) rc = br_cells_name_cells(c, 0, (int64_t)n, cell.data());
        corrected.assign(k + 1, 0);
        if (!rc) for (size_t i = 0; i < n; i++) if (status[i] == 2 && cell[i] < k) corrected[cell[i]]++;
      }
    }
    if (!rc && call) rc = call_cells((int64_t)n_cells);
    if (wl) { (void)br_cells_whitelist_stats(c, wst); (void)br_whitelist_stats(wl, lst); }
    (void)br_cells_stats(c, st);
    return rc;
  }
  bool write_files(brio::BgzfWriter &, const std::vector<br_bgzf_span> &) override {
    probed = false;   // (the matrix's own file takes the place of the trial)
    if (FILE *f = matrix.open()) write_cells_matrix(f, n_features, cell_off, feature, value, env.o.cells_multi == 0);
    if (!matrix.close()) return false;
    if (FILE *f = barcodes.open()) write_cells_table(f, cb, len, names, unique, multi, n_feat, iters, false);
    if (!barcodes.close()) return false;
    if (FILE *f = features.open()) write_cells_features(f, env.tx, env.o.cells_features == 0);
    if (!features.close()) return false;
    if (FILE *f = table.open()) write_cells_table(f, cb, len, names, unique, multi, n_feat, iters, true, wl ? &corrected : nullptr);
    if (!table.close()) return false;
    if (!call) return true;
    if (FILE *f = f_matrix.open()) write_cells_matrix(f, n_features, f_off, f_feature, f_value, env.o.cells_multi == 0);
    if (!f_matrix.close()) return false;
    if (FILE *f = f_barcodes.open()) write_cells_calls(f, cb, len, total, rank, status, cand_of, loglik, lower, pval, padj, true);
    if (!f_barcodes.close()) return false;
    if (FILE *f = calls.open()) write_cells_calls(f, cb, len, total, rank, status, cand_of, loglik, lower, pval, padj, false);
    return calls.close();
  }
  bool settle(bool failed) override { probed = false; return settle_all({&matrix, &barcodes, &features, &table, &f_matrix, &f_barcodes, &calls}, failed); }
  void report() const override {
    static const char *const multi_name[] = {"unique", "uniform", "em"};
    static const char *const correct_name[] = {"exact", "1mm", "1mm-multi"};
    if (wl)
      printf("[bramble] whitelist: %llu barcodes; %llu read names with a barcode: %llu exact, %llu corrected, %llu without match, %llu ambiguous (%llu distinct observed; correct %s; build %.2fs, resolve %.2fs)\n",
             (unsigned long long)lst[0], (unsigned long long)(wst[1] + wst[2] + wst[3] + wst[4]), (unsigned long long)wst[1], (unsigned long long)wst[2],
             (unsigned long long)wst[3], (unsigned long long)wst[4], (unsigned long long)wst[5], correct_name[env.o.cells_correct], (double)lst[4] * 1e-6,
             (double)wst[6] * 1e-6);
    static const char *const filter_name[] = {"topcells", "cr2.2", "emptydrops"};
    if (call)
      printf("[bramble] cell calling: %llu of %llu cells called (%llu simple, %llu by emptydrops of %llu candidates; threshold %llu; ambient %llu counts over %llu barcodes, %llu features; %llu sims; method %s; rank %.2fs, simulate %.2fs)\n",
             (unsigned long long)(cst[1] + cst[2]), (unsigned long long)cst[0], (unsigned long long)cst[1], (unsigned long long)cst[2],
             (unsigned long long)cst[11], (unsigned long long)cst[3], (unsigned long long)cst[6], (unsigned long long)cst[5], (unsigned long long)cst[7],
             (unsigned long long)(cst[14] ? cst[21] : 0), filter_name[env.o.cells_filter], (double)cst[16] * 1e-6, (double)cst[18] * 1e-6);
    printf("[bramble] cells: %llu cells, %llu of %llu read names counted (%llu without barcode; %llu matrix entries; features %s; multi %s; add %.2fs, finish %.2fs)\n",
           (unsigned long long)st[5], (unsigned long long)st[1], (unsigned long long)st[0], (unsigned long long)st[2], (unsigned long long)st[9],
           env.o.cells_features == 0 ? "gene" : "transcript", multi_name[env.o.cells_multi], (double)st[13] * 1e-6, (double)st[14] * 1e-6);
  }
 private:
  // --cells-filter: the calls, the candidates' numbers and the called cells' rows to the host
  int call_cells(int64_t n_cells) {
    int rc = br_cells_call(c, call, (int64_t)n_features);
    if (!rc) rc = br_cellcall_stats(call, cst);
    if (rc) return rc;
    const size_t k = (size_t)n_cells, m = (size_t)cst[11], called = (size_t)(cst[1] + cst[2]);
    status.resize(k + 1); rank.resize(k + 1); total.resize(k + 1); cand_of.assign(k + 1, 0xffffffffu);
    std::vector<uint32_t> cand(m + 1), cells(called + 1);
    loglik.resize(m + 1); lower.resize(m + 1); pval.resize(m + 1); padj.resize(m + 1);
    rc = br_cellcall_calls(call, 0, n_cells, status.data(), rank.data(), total.data());
    if (!rc) rc = br_cellcall_candidates(call, 0, (int64_t)m, cand.data(), loglik.data(), lower.data(), pval.data(), padj.data());
    for (size_t j = 0; !rc && j < m; j++) if (cand[j] < k) cand_of[cand[j]] = (uint32_t)j;
    f_off.resize(called + 1);
    if (!rc) rc = br_cells_matrix_called(c, 0, (int64_t)called, cells.data(), f_off.data(), nullptr, nullptr);
    if (rc) return rc;
    f_feature.resize((size_t)f_off[called] + 1); f_value.resize((size_t)f_off[called] + 1);
    return br_cells_matrix_called(c, 0, (int64_t)called, nullptr, f_off.data(), f_feature.data(), f_value.data());
  }
  uint64_t st_names() const { uint64_t v[16] = {}; (void)br_cells_stats(c, v); return v[0]; }
  br_cells *c = nullptr;
  br_whitelist *wl = nullptr;   // --cells-whitelist: the run's one
  uint64_t wst[8] = {}, lst[8] = {};
  std::vector<uint64_t> corrected;
  Consumer *quant = nullptr;   // the --quant consumer, which outlives neither of the two
  SideFile matrix, barcodes, features, table, f_matrix, f_barcodes, calls;
  br_cellcall *call = nullptr;   // --cells-filter: the caller, with its parameters from open() on
  uint64_t cst[32] = {};
  std::vector<uint8_t> status;
  std::vector<uint32_t> rank, cand_of, lower, f_feature;
  std::vector<uint64_t> total, f_off;
  std::vector<double> loglik, pval, padj, f_value;
  bool probed = false;
  size_t n_features = 0;
  uint64_t st[16] = {};
  std::vector<uint8_t> cb, len;
  std::vector<uint64_t> names, unique, multi, cell_off;
  std::vector<uint32_t> n_feat, iters, feature;
  std::vector<double> value;
};

}  // namespace

std::unique_ptr<Consumer> open_cells(const RunEnv &env, std::string &err) {
  auto c = std::make_unique<CellsOut>(env);
  if (!c->open(err)) return nullptr;
  return c;
}

}  // namespace brcli
