// SideFile and the text of the side files (cli_output_files.h).  No call into the library.
#include "cli_output_files.h"

#include <math.h>

#include <algorithm>
#include <string_view>
#include <unordered_map>

namespace brcli {

FILE *SideFile::open(bool binary) { return f_ = path.empty() ? nullptr : fopen(tmp.c_str(), binary ? "wb" : "w"); }

bool SideFile::close() {
  if (path.empty()) return true;
  bool ok = f_ && !ferror(f_);
  if (f_ && fclose(f_) != 0) ok = false;
  f_ = nullptr;
  if (!ok) fprintf(stderr, "error: could not write %s\n", tmp.c_str());
  return ok;
}

bool SideFile::settle(bool failed) {
  if (path.empty()) return true;
  const bool renamed = !failed && rename(tmp.c_str(), path.c_str()) == 0;
  if (!failed && !renamed) fprintf(stderr, "error: could not rename %s to %s\n", tmp.c_str(), path.c_str());
  if (!renamed) remove(tmp.c_str());
  return failed || renamed;
}

bool settle_all(std::initializer_list<SideFile *> files, bool failed) {
  for (SideFile *f : files) if (!f->settle(failed)) failed = true;
  return !failed;
}

void number_sq(TxTable &tx) {
  tx.sq_of.assign(tx.len.size(), -1);
  tx.n_sq = 0;
  for (size_t t = 0; t < tx.len.size(); t++) if (tx.len[t] > 0) tx.sq_of[t] = tx.n_sq++;
}

void number_genes(TxTable &tx) {
  std::unordered_map<std::string_view, uint32_t> number;
  tx.gene_of.assign(tx.gene.size(), 0);
  tx.gene_name.clear();
  for (int pass = 0; pass < 2; pass++)   // the @SQ transcripts first
    for (size_t t = 0; t < tx.gene.size(); t++) {
      if ((tx.len[t] > 0) != (pass == 0)) continue;
      auto it = number.emplace(tx.gene[t], (uint32_t)tx.gene_name.size());
      if (it.second) tx.gene_name.push_back(tx.gene[t]);
      tx.gene_of[t] = it.first->second;
    }
}

void write_cells_matrix(FILE *f, size_t n_features, const std::vector<uint64_t> &cell_off, const std::vector<uint32_t> &feature,
                        const std::vector<double> &value, bool integer) {
  const size_t n_cells = cell_off.empty() ? 0 : cell_off.size() - 1;
  fprintf(f, "%%%%MatrixMarket matrix coordinate %s general\n%%\n%zu %zu %llu\n", integer ? "integer" : "real", n_features, n_cells,
          (unsigned long long)(n_cells ? cell_off[n_cells] : 0));
  for (size_t k = 0; k < n_cells; k++)
    for (uint64_t z = cell_off[k]; z < cell_off[k + 1]; z++) {
      if (integer) fprintf(f, "%u %zu %llu\n", feature[z] + 1, k + 1, (unsigned long long)value[z]);
      else fprintf(f, "%u %zu %.10g\n", feature[z] + 1, k + 1, value[z]);
    }
}

void write_cells_features(FILE *f, const TxTable &tx, bool genes) {
  if (genes) for (const char *g : tx.gene_name) fprintf(f, "%s\t%s\tGene Expression\n", g, g);
  else for (size_t t = 0; t < tx.len.size(); t++) if (tx.len[t] > 0) fprintf(f, "%s\t%s\tGene Expression\n", tx.name[t], tx.name[t]);
}

// table: the whole line; else the barcode alone (barcodes.tsv)
void write_cells_table(FILE *f, const std::vector<uint8_t> &barcodes, const std::vector<uint8_t> &len, const std::vector<uint64_t> &names,
                       const std::vector<uint64_t> &unique, const std::vector<uint64_t> &multi, const std::vector<uint32_t> &features,
                       const std::vector<uint32_t> &iters, bool table, const std::vector<uint64_t> *corrected) {
  if (table) fprintf(f, corrected ? "Barcode\tNames\tUnique\tMulti\tFeatures\tIterations\tCorrected\n" : "Barcode\tNames\tUnique\tMulti\tFeatures\tIterations\n");
  for (size_t k = 0; k < len.size(); k++) {
    fwrite(barcodes.data() + 32 * k, 1, len[k], f);
    if (table) fprintf(f, "\t%llu\t%llu\t%llu\t%u\t%u", (unsigned long long)names[k], (unsigned long long)unique[k], (unsigned long long)multi[k], features[k], iters[k]);
    if (table && corrected) fprintf(f, "\t%llu", (unsigned long long)(*corrected)[k]);
    fputc('\n', f);
  }
}

void write_cells_calls(FILE *f, const std::vector<uint8_t> &barcodes, const std::vector<uint8_t> &len, const std::vector<uint64_t> &total,
                       const std::vector<uint32_t> &rank, const std::vector<uint8_t> &status, const std::vector<uint32_t> &cand_of,
                       const std::vector<double> &loglik, const std::vector<uint32_t> &lower, const std::vector<double> &pval,
                       const std::vector<double> &padj, bool only) {
  if (!only) fprintf(f, "Barcode\tTotal\tRank\tStatus\tLogLik\tLower\tPValue\tPAdj\n");
  for (size_t k = 0; k < len.size(); k++) {
    if (only && !status[k]) continue;
    fwrite(barcodes.data() + 32 * k, 1, len[k], f);
    if (!only) {
      fprintf(f, "\t%llu\t%u\t%u", (unsigned long long)total[k], rank[k], (unsigned)status[k]);
      const uint32_t j = cand_of[k];
      if (j == 0xffffffffu) fprintf(f, "\t.\t.\t.\t.");
      else fprintf(f, "\t%.17g\t%u\t%.17g\t%.17g", loglik[j], lower[j], pval[j], padj[j]);
    }
    fputc('\n', f);
  }
}

void write_quant_table(FILE *f, const TxTable &tx, const std::vector<double> *eff, const std::vector<double> &theta, const std::vector<double> &tpm,
                       const std::vector<uint64_t> &unique, const std::vector<uint64_t> &ambig, const std::vector<double> *boot_mean,
                       const std::vector<double> *boot_var) {
  const bool boot = boot_mean && boot_var;
  fprintf(f, eff ? "Name\tLength\tEffectiveLength\tNumReads\tTPM\tUniqueReads\tAmbigReads" : "Name\tLength\tNumReads\tTPM\tUniqueReads\tAmbigReads");
  fprintf(f, boot ? "\tBootMean\tBootSD\n" : "\n");
  for (size_t t = 0; t < tx.len.size(); t++) {
    if (tx.len[t] <= 0) continue;
    fprintf(f, "%s\t%lld", tx.name[t], (long long)tx.len[t]);
    if (eff) fprintf(f, "\t%.3f", (*eff)[t]);
    fprintf(f, "\t%.6f\t%.6f\t%llu\t%llu", theta[t], tpm[t], (unsigned long long)unique[t], (unsigned long long)ambig[t]);
    if (boot) fprintf(f, "\t%.6f\t%.6f", (*boot_mean)[t], sqrt((*boot_var)[t]));
    fputc('\n', f);
  }
}

void write_quant_bootstraps(FILE *f, const TxTable &tx, int n_boot, const std::vector<double> &theta) {
  const size_t n_tx = tx.len.size();
  fprintf(f, "Name");
  for (int b = 0; b < n_boot; b++) fprintf(f, "\t%d", b);
  fputc('\n', f);
  for (size_t t = 0; t < n_tx; t++) {
    if (tx.len[t] <= 0) continue;
    fprintf(f, "%s", tx.name[t]);
    for (int b = 0; b < n_boot; b++) fprintf(f, "\t%.6f", theta[(size_t)b * n_tx + t]);
    fputc('\n', f);
  }
}

void write_quant_classes(FILE *f, const TxTable &tx, int64_t n_classes, const std::vector<uint64_t> &label_off, const std::vector<uint32_t> &labels,
                         const std::vector<uint64_t> &counts) {
  fprintf(f, "%lld\n%lld\n", (long long)tx.n_sq, (long long)n_classes);
  for (size_t t = 0; t < tx.len.size(); t++) if (tx.len[t] > 0) fprintf(f, "%s\n", tx.name[t]);
  for (size_t c = 0; c < (size_t)n_classes; c++) {
    fprintf(f, "%llu", (unsigned long long)(label_off[c + 1] - label_off[c]));
    for (uint64_t e = label_off[c]; e < label_off[c + 1]; e++) fprintf(f, "\t%lld", (long long)tx.sq_of[labels[(size_t)e]]);
    fprintf(f, "\t%llu\n", (unsigned long long)counts[c]);
  }
}

void write_quant_gene_table(FILE *f, const TxTable &tx, const std::vector<double> &length, const std::vector<double> *eff, const std::vector<double> &num_reads,
                            const std::vector<double> &tpm, const std::vector<uint64_t> &unique, const std::vector<uint64_t> &ambig,
                            const std::vector<uint32_t> &n_transcripts, const std::vector<double> *boot_mean, const std::vector<double> *boot_var) {
  const bool boot = boot_mean && boot_var;
  fprintf(f, eff ? "Name\tLength\tEffectiveLength\tNumReads\tTPM\tUniqueReads\tAmbigReads\tNumTranscripts" : "Name\tLength\tNumReads\tTPM\tUniqueReads\tAmbigReads\tNumTranscripts");
  fprintf(f, boot ? "\tBootMean\tBootSD\n" : "\n");
  for (size_t g = 0; g < tx.gene_name.size(); g++) {
    fprintf(f, "%s\t%.3f", tx.gene_name[g], length[g]);
    if (eff) fprintf(f, "\t%.3f", (*eff)[g]);
    fprintf(f, "\t%.6f\t%.6f\t%llu\t%llu\t%u", num_reads[g], tpm[g], (unsigned long long)unique[g], (unsigned long long)ambig[g], n_transcripts[g]);
    if (boot) fprintf(f, "\t%.6f\t%.6f", (*boot_mean)[g], sqrt((*boot_var)[g]));
    fputc('\n', f);
  }
}

void write_quant_gene_classes(FILE *f, const TxTable &tx, int64_t n_classes, const std::vector<uint64_t> &label_off, const std::vector<uint32_t> &labels,
                              const std::vector<uint64_t> &counts) {
  fprintf(f, "%zu\n%lld\n", tx.gene_name.size(), (long long)n_classes);
  for (const char *g : tx.gene_name) fprintf(f, "%s\n", g);
  for (size_t c = 0; c < (size_t)n_classes; c++) {
    fprintf(f, "%llu", (unsigned long long)(label_off[c + 1] - label_off[c]));
    for (uint64_t e = label_off[c]; e < label_off[c + 1]; e++) fprintf(f, "\t%u", labels[(size_t)e]);
    fprintf(f, "\t%llu\n", (unsigned long long)counts[c]);
  }
}

void write_fragment_lengths(FILE *f, const std::vector<uint64_t> &hist) {
  fprintf(f, "FragmentLength\tCount\n");
  for (size_t k = 0; k < hist.size(); k++) fprintf(f, "%zu\t%llu\n", k, (unsigned long long)hist[k]);
}

int write_bedgraph(FILE *f, const TxTable &tx, int64_t n_runs, int64_t page, const RunPage &fetch) {
  std::vector<uint32_t> tid((size_t)std::min(n_runs, page) + 1), start(tid.size()), end(tid.size()), depth(tid.size());
  for (int64_t first = 0; first < n_runs; first += page) {
    const int64_t n = std::min(page, n_runs - first);
    if (const int rc = fetch(first, n, tid.data(), start.data(), end.data(), depth.data())) return rc;
    for (size_t k = 0; k < (size_t)n; k++) fprintf(f, "%s\t%u\t%u\t%u\n", tx.name[tid[k]], start[k], end[k], depth[k]);
  }
  return 0;
}

void write_coverage_summary(FILE *f, const TxTable &tx, const std::vector<uint64_t> &records, const std::vector<uint64_t> &aligned,
                            const std::vector<uint64_t> &covered, const std::vector<uint32_t> &max_depth) {
  fprintf(f, "Name\tLength\tRecords\tAlignedBases\tCoveredBases\tMaxDepth\tMeanDepth\tBreadth\n");
  for (size_t t = 0; t < tx.len.size(); t++)
    if (tx.len[t] > 0) fprintf(f, "%s\t%lld\t%llu\t%llu\t%llu\t%u\t%.6f\t%.6f\n", tx.name[t], (long long)tx.len[t], (unsigned long long)records[t],
                               (unsigned long long)aligned[t], (unsigned long long)covered[t], max_depth[t], (double)aligned[t] / (double)tx.len[t],
                               (double)covered[t] / (double)tx.len[t]);
}

int write_bedgraph_weighted(FILE *f, const TxTable &tx, int64_t n_runs, int64_t page, const RunPage64 &fetch) {
  std::vector<uint32_t> tid((size_t)std::min(n_runs, page) + 1), start(tid.size()), end(tid.size());
  std::vector<uint64_t> depth(tid.size());
  for (int64_t first = 0; first < n_runs; first += page) {
    const int64_t n = std::min(page, n_runs - first);
    if (const int rc = fetch(first, n, tid.data(), start.data(), end.data(), depth.data())) return rc;
    for (size_t k = 0; k < (size_t)n; k++) fprintf(f, "%s\t%u\t%u\t%.10g\n", tx.name[tid[k]], start[k], end[k], (double)depth[k] / 4294967296.0);
  }
  return 0;
}

void write_coverage_summary_weighted(FILE *f, const TxTable &tx, const std::vector<uint64_t> &records, const std::vector<uint64_t> &weight_sum,
                                     const std::vector<uint64_t> &aligned_hi, const std::vector<uint64_t> &aligned_lo,
                                     const std::vector<uint64_t> &covered, const std::vector<uint64_t> &max_depth) {
  fprintf(f, "Name\tLength\tRecords\tWeightedRecords\tAlignedBases\tCoveredBases\tMaxDepth\tMeanDepth\tBreadth\n");
  for (size_t t = 0; t < tx.len.size(); t++) {
    if (tx.len[t] <= 0) continue;
    const double aligned = (double)aligned_hi[t] + (double)aligned_lo[t] / 4294967296.0;
    fprintf(f, "%s\t%lld\t%llu\t%.6f\t%.6f\t%llu\t%.6f\t%.6f\t%.6f\n", tx.name[t], (long long)tx.len[t], (unsigned long long)records[t],
            (double)weight_sum[t] / 4294967296.0, aligned, (unsigned long long)covered[t], (double)max_depth[t] / 4294967296.0,
            aligned / (double)tx.len[t], (double)covered[t] / (double)tx.len[t]);
  }
}

}  // namespace brcli
