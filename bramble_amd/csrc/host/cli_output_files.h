// The files beside the main output (cli_output.h): how each goes to disk and what its text is.  Plain data and a FILE * only --
// nothing here knows the library, so cli_output_files.cpp builds and runs without it (tests/cli_output_probe.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

namespace brcli {

// A file written under a temporary name next to its target and renamed once the whole run has succeeded, like the main output: a
// failed run leaves neither.  An empty path: the file was not asked for, and every call does nothing.
class SideFile {
 public:
  explicit SideFile(const std::string &p) : path(p), tmp(p.empty() ? p : p + ".tmp-bramble") {}
  FILE *open(bool binary = false);   // nullptr: not asked for, or not opened -- close() says which
  bool close();                      // false: opening, a write or the close failed (said here)
  bool settle(bool failed);          // renames, or after a failure removes; false: the rename failed (said here, nothing is left)
  const std::string path, tmp;
 private:
  FILE *f_ = nullptr;
};
bool settle_all(std::initializer_list<SideFile *> files, bool failed);   // in this order; after a failed rename the rest is removed; false: one failed

// Every transcript of the index; the tables list those of length > 0 (the output's @SQ list), numbered in that order by sq_of
// --quant-genes: gene, every transcript's gene id (else empty); the genes are numbered in order of first appearance in @SQ order
// (those that only transcripts outside the @SQ list have come last): gene_of per transcript, gene_name per gene
struct TxTable {
  std::vector<const char *> name; std::vector<int64_t> len, sq_of; int64_t n_sq = 0;
  std::vector<const char *> gene, gene_name; std::vector<uint32_t> gene_of;
};
void number_sq(TxTable &tx);   // sq_of and n_sq from len
void number_genes(TxTable &tx);   // gene_of and gene_name from gene and len

// eff: the EffectiveLength column behind Length, nullptr without it; boot_mean and boot_var: the last columns BootMean and BootSD
// (the variance's square root), nullptr without them
void write_quant_table(FILE *f, const TxTable &tx, const std::vector<double> *eff, const std::vector<double> &theta, const std::vector<double> &tpm,
                       const std::vector<uint64_t> &unique, const std::vector<uint64_t> &ambig, const std::vector<double> *boot_mean = nullptr,
                       const std::vector<double> *boot_var = nullptr);
// the replicates' NumReads (theta: n_boot rows of one value per transcript): Name 0 1 ... n_boot - 1, a line per @SQ transcript
void write_quant_bootstraps(FILE *f, const TxTable &tx, int n_boot, const std::vector<double> &theta);
// salmon's eq_classes.txt: the counts, the names, then per class its size, its transcripts' @SQ numbers and its count
void write_quant_classes(FILE *f, const TxTable &tx, int64_t n_classes, const std::vector<uint64_t> &label_off, const std::vector<uint32_t> &labels,
                         const std::vector<uint64_t> &counts);
void write_fragment_lengths(FILE *f, const std::vector<uint64_t> &hist);
// --quant-genes: a line per gene, Name Length [EffectiveLength] NumReads TPM UniqueReads AmbigReads NumTranscripts [BootMean BootSD];
// eff, boot_mean and boot_var as in write_quant_table
void write_quant_gene_table(FILE *f, const TxTable &tx, const std::vector<double> &length, const std::vector<double> *eff, const std::vector<double> &num_reads,
                            const std::vector<double> &tpm, const std::vector<uint64_t> &unique, const std::vector<uint64_t> &ambig,
                            const std::vector<uint32_t> &n_transcripts, const std::vector<double> *boot_mean = nullptr, const std::vector<double> *boot_var = nullptr);
// write_quant_classes' layout with the genes' names and numbers
void write_quant_gene_classes(FILE *f, const TxTable &tx, int64_t n_classes, const std::vector<uint64_t> &label_off, const std::vector<uint32_t> &labels,
                              const std::vector<uint64_t> &counts);
// --cells: Matrix Market coordinate, features x cells, 1-based, by cell then feature (cell_off: CSR by cell); integer: the values as
// integers, else %.10g
void write_cells_matrix(FILE *f, size_t n_features, const std::vector<uint64_t> &cell_off, const std::vector<uint32_t> &feature,
                        const std::vector<double> &value, bool integer);
// id<TAB>name<TAB>Gene Expression, a line per feature (genes: tx.gene_name; else the @SQ transcripts)
void write_cells_features(FILE *f, const TxTable &tx, bool genes);
// table: Barcode Names Unique Multi Features Iterations, a line per cell under that header; else the barcode alone (barcodes.tsv).
// barcodes: n x 32 bytes with their lengths.  corrected (--cells-whitelist): a last column Corrected of the table
void write_cells_table(FILE *f, const std::vector<uint8_t> &barcodes, const std::vector<uint8_t> &len, const std::vector<uint64_t> &names,
                       const std::vector<uint64_t> &unique, const std::vector<uint64_t> &multi, const std::vector<uint32_t> &features,
                       const std::vector<uint32_t> &iters, bool table, const std::vector<uint64_t> *corrected = nullptr);
// --cells-filter: Barcode Total Rank Status LogLik Lower PValue PAdj, a line per cell in barcode order.  cand_of[k]: the cell's place among
// the candidates (their columns with %.17g), or 0xffffffff: a dot in each of the four; `only`: the barcodes of the cells with a status
// other than 0, nothing else (filtered_barcodes.tsv)
void write_cells_calls(FILE *f, const std::vector<uint8_t> &barcodes, const std::vector<uint8_t> &len, const std::vector<uint64_t> &total,
                       const std::vector<uint32_t> &rank, const std::vector<uint8_t> &status, const std::vector<uint32_t> &cand_of,
                       const std::vector<double> &loglik, const std::vector<uint32_t> &lower, const std::vector<double> &pval,
                       const std::vector<double> &padj, bool only);
// runs [first, first + n) into the four columns; not 0: an error, which ends the file there
using RunPage = std::function<int(int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth)>;
int write_bedgraph(FILE *f, const TxTable &tx, int64_t n_runs, int64_t page, const RunPage &fetch);   // the first error of fetch
void write_coverage_summary(FILE *f, const TxTable &tx, const std::vector<uint64_t> &records, const std::vector<uint64_t> &aligned,
                            const std::vector<uint64_t> &covered, const std::vector<uint32_t> &max_depth);
// --coverage-weight nh|em: the depth is fixed point, one unit 2^32, and printed as depth / 2^32 with %.10g
using RunPage64 = std::function<int(int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint64_t *depth)>;
int write_bedgraph_weighted(FILE *f, const TxTable &tx, int64_t n_runs, int64_t page, const RunPage64 &fetch);
// Name Length Records WeightedRecords AlignedBases CoveredBases MaxDepth MeanDepth Breadth; the fixed-point columns (weight_sum,
// aligned = aligned_hi + aligned_lo / 2^32, max_depth) and MeanDepth with %.6f
void write_coverage_summary_weighted(FILE *f, const TxTable &tx, const std::vector<uint64_t> &records, const std::vector<uint64_t> &weight_sum,
                                     const std::vector<uint64_t> &aligned_hi, const std::vector<uint64_t> &aligned_lo,
                                     const std::vector<uint64_t> &covered, const std::vector<uint64_t> &max_depth);

}  // namespace brcli
