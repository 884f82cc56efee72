// The bramble command line on top of the C ABI (scope table rows f-1 / f-3 / f-4): same flags as the
// reference's CLI11 front-end (src/bramble.cpp:443-485), same output header layout
// (src/bramble.cpp:513-623), same final report (src/bramble.cpp:727-736).
//
//   input         : bundles of records cut at read-name changes, from the host BAM reader, the device BAM readers or the SAM
//                   readers (cli_input.h: one source per format)
//   uploader      : br_bam_bundle_stage (host bundles: records to one of three device slots, own copy stream)
//   runner        : br_project_bam_staged_nowait / br_project_bam_resident (everything between the raw records on the device)
//   writer thread : BGZF deflate (threaded) -> output file; device-made BGZF blocks or SAM lines (-O sam) go out as they are
//   consumers     : what else takes something from every projected bundle -- --sort, --dedup, --quant, --coverage, --unprojected, --quant-bam (cli_output.h: one consumer
//                   per feature).  The runner hands each bundle to every consumer right after its projection call; after the last
//                   bundle each finishes on the device, writes its files under temporary names and prints its report line.  One of
//                   them may keep the records (--sort): then the projection leaves them in HBM (BR_OUT_RESIDENT), nothing of a
//                   bundle goes to the writer, and after the last bundle the consumer's pieces take the same way out
//                   (br_device_bam_download -> writer); the writer notes the blocks it writes for the consumer's index
#include <ctype.h>
#include <math.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include <future>
#include <unordered_map>

#include "cli_input.h"
#include "cli_output.h"

#define BRAMBLE_REF_VERSION "0.1.6"  // src/bramble.cpp:35

using namespace brcli;

namespace {
using brio::BgzfReader;
using brio::BgzfWriter;
void usage(FILE *f) {
  fprintf(f,
          "bramble (MI355X) usage:\n\n"
          "bramble <in.bam|in.sam|-> -G <annotation.gtf> -o <out.bam|out.sam|-> [-O bam|sam] [-p <cpus>] [-S <genome.fa>]\n"
          " [--help] [--version] [--quiet] [--fr] [--rf] [--lr] [--lr-hq] [--strict]\n"
          " [--max-soft-clip N] [--max-junction-insertion N] [--max-junction-deletion N]\n"
          " [--max-error-exon N] [--similarity-threshold X]\n"
          " [--device-deflate | --host-deflate | --compression-level 0-9] [--device-reader | --host-reader] [--bundle-size N]\n"
          "               [--device N | --devices a,b,...] [--collate] [--sort [--write-index]]\n"
          "               [--quant <quant.tsv> [--quant-classes <eq_classes.txt>] [--quant-length-norm | --quant-no-length-norm]\n"
          "                [--quant-eff-length [--quant-fld <fld.tsv>]]\n"
          "                [--quant-bootstraps B [--quant-seed S] [--quant-boot-out <bootstraps.tsv>]]\n"
          "                [--quant-vb [--quant-vb-prior P] [--quant-vb-per-nucleotide]]\n"
          "                [--quant-genes <genes.tsv> [--quant-gene-classes <gene_classes.txt>] [--quant-gene-map <tx2gene.tsv>]]]\n"
          "               [--coverage <cov.bedgraph>] [--coverage-summary <cov.tsv>] [--coverage-primary]\n"
          "               [--coverage-weight unit|nh|em]\n"
          "               [--coverage-bigwig <cov.bw> [--coverage-bigwig-zooms 0-10] [--coverage-bigwig-uncompressed]]\n"
          "               [--unprojected <unprojected.bam> [--unprojected-scope record|name]]\n"
          "               [--quant-bam <post.bam> [--quant-bam-mode tag|sample]]\n"
          "               [--dedup unique|directional [--dedup-umi name|tag] [--dedup-umi-sep C] [--dedup-umi-tag XY]\n"
          "                [--dedup-stats <sizes.tsv>] [--dedup-bam <dedup.bam> [--dedup-bam-mode remove|mark]]]\n"
          "               [--cells <prefix> [--cells-barcode name|tag] [--cells-barcode-tag XY] [--cells-features gene|transcript]\n"
          "                [--cells-multi unique|uniform|em] [--cells-whitelist <file> [--cells-correct exact|1mm|1mm-multi]]\n"
          "                [--cells-filter topcells|cr2.2|emptydrops [--cells-expected N] [--cells-filter-percentile P]\n"
          "                 [--cells-filter-ratio R] [--cells-ed-window LO,HI] [--cells-ed-umi-min N] [--cells-ed-umi-frac F]\n"
          "                 [--cells-ed-candidates N] [--cells-ed-fdr F] [--cells-ed-sims N]]]\n\n"
          "Project spliced genomic alignments into transcriptomic space.\n"
          "The output BGZF blocks are deflated on the GPU by default (per-block Huffman codes); --host-deflate or\n"
          "--compression-level N use the host codec (libdeflate / zlib, level 6 like the reference unless N is given).\n"
          "--devices 0,1,...: bundles are dealt to one worker per listed GPU (an index replica each, no exchange between them);\n"
          "the output keeps the input order.\n"
          "The input is BAM or SAM text (a file, or standard input as -), told apart by its bytes; SAM lines become BAM\n"
          "records on the GPU.  --device-reader / --host-reader choose how BAM is read and do not apply to SAM.\n"
          "BGZF-compressed SAM and plain gzip input are not supported.\n"
          "--collate: input in any order (e.g. coordinate-sorted); the whole input is read into one device's memory and grouped by read name before the first bundle is projected.\n"
          "-O, --output-fmt bam|sam: BAM (the default) or SAM text, formatted on the GPU (the header text, then one line per record,\n"
          "no BGZF framing); the format is never taken from the output's extension.  --compression-level, --host-deflate and\n"
          "--device-deflate apply to BAM only.\n"
          "--sort: the output is sorted by coordinate (transcript, position, forward strand first; ties keep the order of the unsorted\n"
          "output) and its header says @HD SO:coordinate; the projected records of the whole run are kept in one device's memory and\n"
          "sorted there.  --write-index: with --sort and BAM output to a file, also write <out>.bai, built on the GPU (device deflate only).\n"
          "A run with --sort prints one more line in front of the final report, which is unchanged: [bramble] sorted N records by coordinate ...\n"
          "--quant FILE: the projected records of the whole run are reduced, on one GPU, to equivalence classes (the set of transcripts a\n"
          "read name was projected to; both mates count) and per-transcript abundances are estimated from them by EM; FILE gets one line\n"
          "per @SQ transcript: Name, Length, NumReads, TPM, UniqueReads, AmbigReads.  --quant-classes FILE: the classes in the layout of\n"
          "salmon's eq_classes.txt.  Reads are weighted by 1 / transcript length in the short-read preset and not under --lr / --lr-hq;\n"
          "--quant-length-norm / --quant-no-length-norm say otherwise.  No bias model.  One more line\n"
          "in front of the final report: [bramble] quantified N read names in C classes ...\n"
          "--quant-bootstraps B (1 .. 10000): B bootstrap replicates on the GPU: the read names are resampled with replacement (a\n"
          "counter-based generator, Philox4x32-10 under --quant-seed S, default 0: the same seed gives the same replicates on every\n"
          "run) and the EM runs on each replicate's counts, sixteen replicates at a time; quant.tsv gains two last columns, BootMean and\n"
          "BootSD (the replicates' mean and sample standard deviation of NumReads).  --quant-boot-out FILE: one line per @SQ\n"
          "transcript, Name and the B replicates' NumReads, under the header Name 0 1 ... B-1.  One more line in front of the\n"
          "quantified line: [bramble] bootstrapped B replicates (seed S, I iterations in all, sampling X.XXs, EM Y.YYs)\n"
          "--quant-eff-length: the fragment lengths of the pairs that project to one transcript alone are counted on the GPU and reads\n"
          "are weighted by 1 / effective length (the transcript's length minus the mean of the observed fragment lengths that fit it,\n"
          "plus 1: salmon's and kallisto's convention); quant.tsv gains an EffectiveLength column behind Length.  It needs length\n"
          "normalisation: not with --quant-no-length-norm, and under --lr / --lr-hq only with --quant-length-norm.  --quant-fld FILE:\n"
          "the histogram, FragmentLength and Count for the lengths 0 .. 1000.  One more line in front of the quantified line:\n"
          "[bramble] fragment lengths: N observed, mean M.M, U unique names without a pair, R out of range\n"
          "--quant-vb: the variational Bayes EM (salmon's default estimator) in place of the maximum-likelihood EM, for the point estimate,\n"
          "the replicates and the posteriors of --coverage-weight em: a Dirichlet prior of P reads per transcript (--quant-vb-prior P,\n"
          "default 0.01, finite and >= 0) or, with --quant-vb-per-nucleotide, per nucleotide of its (effective) length, which needs\n"
          "length normalisation; isoforms without evidence of their own go to zero.  Transcripts the data cannot tell apart are\n"
          "split by rounding (the same on every run).  The files keep their columns.  One more line in front of the quantified line:\n"
          "[bramble] variational Bayes: prior P per transcript|nucleotide, N transcripts at zero\n"
          "--quant-genes FILE: the transcripts' results collapsed to genes on the GPU (the gene_id of the annotation): one line per gene,\n"
          "genes in order of first appearance in @SQ order: Name, Length (the TPM-weighted mean of its transcripts' lengths, their plain\n"
          "mean where the gene's TPM is 0), [EffectiveLength,] NumReads, TPM, UniqueReads and AmbigReads (of the read names' gene sets: a\n"
          "read that is ambiguous among isoforms of one gene is unique here), NumTranscripts, [BootMean, BootSD of the gene's NumReads over\n"
          "the replicates].  --quant-gene-classes FILE: the classes merged by gene set, in the layout of --quant-classes with gene names.\n"
          "--quant-gene-map FILE: transcript<TAB>gene lines (a tximport tx2gene table; # lines and empty lines are skipped, further\n"
          "columns ignored) that replace the annotation's gene ids; every @SQ transcript must be in it.  One more line in front of the\n"
          "quantified line: [bramble] gene level: G genes, C classes (X.XXs)\n"
          "--coverage FILE: the depth of coverage along every transcript, counted on one GPU from the projected records of the whole\n"
          "run, as a bedGraph (name, start, end, depth; 0-based, half-open, no header; @SQ order, then ascending start; depth > 0\n"
          "only, as bedtools genomecov -bg -split lists it).  M = X cover, D N do not; secondary records and both mates count, a base\n"
          "both mates cover twice.  --coverage-summary FILE: one line per @SQ transcript: Name, Length, Records, AlignedBases,\n"
          "CoveredBases, MaxDepth, MeanDepth, Breadth.  Either switch alone turns the feature on; --coverage-primary counts primary\n"
          "records only.  One more line in front of the final report: [bramble] coverage: N records, A aligned bases on C of B bases in R runs ...\n"
          "--coverage-weight unit|nh|em (default unit): what a record adds to the depth.  nh: 1 / NH of the record; em: the posterior\n"
          "of (read name, transcript) under the abundances --quant estimates (it needs --quant) -- the expected depth.  The depth is\n"
          "fixed point, 32 fractional bits: the bedGraph's depth is printed with %%.10g, and the summary has the columns Name, Length,\n"
          "Records, WeightedRecords, AlignedBases, CoveredBases, MaxDepth, MeanDepth, Breadth.  The report line becomes\n"
          "[bramble] coverage (weight nh|em): ...\n"
          "--coverage-bigwig FILE: the same depth as a bigWig track (UCSC's binary format, version 4), built and compressed on the GPU: no\n"
          "text, no sort | bedGraphToBigWig.  Alone or with --coverage / --coverage-summary, with every weight.  Only transcripts with\n"
          "coverage are in it, in the byte order of their names; one item per bedGraph line, the value a float (24 bits: unit depths\n"
          "above 16 777 216 lose their low bits).  --coverage-bigwig-zooms N (0 .. 10, default 4): zoom levels of 32, 128, 512, ...\n"
          "bases per summary.  --coverage-bigwig-uncompressed: plain sections in place of zlib streams.  One more line behind the\n"
          "coverage line: [bramble] bigwig: C transcripts, S sections of R runs, Z zoom levels (z0, z1, ... records), U -> B bytes (build X.XXs)\n"
          "--unprojected FILE: the input records that no output record came from -- no transcript accepted them, or their matches died\n"
          "at pairing -- written to FILE on the way: a BAM (whatever -O says) under the input's header, the records byte for byte as\n"
          "they came in, in input order.  They are picked out and kept on one GPU while the bundles are projected.  Unmapped input\n"
          "records are not among them.  --unprojected-scope record (the default): every such record; name: only the records of read\n"
          "names of which no record was projected (the mate of a half-projected pair stays out).  One more line in front of the final\n"
          "report: [bramble] unprojected: R of N records written (W read names without a projected record, P partly projected; scope record|name)\n"
          "--quant-bam FILE (it needs --quant): a second BAM, under the header the output has without --sort, with the posterior of\n"
          "--quant's EM on the projected records, weighed and rewritten on one GPU.  --quant-bam-mode tag (the default): every\n"
          "projected record in the order of the unsorted output, with ZW:f:<w> appended (RSEM's tag): w is the posterior of (read name,\n"
          "transcript), split evenly among the read's records on that transcript, a pair's two terms added.  sample: one placement per\n"
          "read name, drawn with probability w (Philox4x32-10 under --quant-seed S: the same seed gives the same file), rewritten to\n"
          "NH:i:1, HI:i:1, primary, the MAPQ of a unique record, with ZW:f:<w>.  BAM whatever -O says; --host-deflate applies.  One more\n"
          "line in front of the final report: [bramble] posterior BAM: R of N records written for M read names (mode tag|sample; add X.XXs, weigh Y.YYs)\n"
          "--dedup unique|directional: UMI-aware duplicate removal on one GPU, by READ NAME: two read names are copies of one molecule\n"
          "when they carry the same UMI and were projected to the same set of placements (transcript, unclipped 5' end, strand and mate\n"
          "bits of every record); directional (umi_tools' default) also joins a UMI to a more abundant one a single mismatch away.  Whole\n"
          "read names are kept or dropped, so a multi-mapper's records stay together.  The UMI is what follows the last --dedup-umi-sep\n"
          "character (default _) of the read name (--dedup-umi name, the default: umi_tools extract's convention) or the value of the\n"
          "--dedup-umi-tag tag (default RX; --dedup-umi tag), at most 32 bytes; a read without one is never a duplicate.  With --quant\n"
          "the duplicate names are not counted: quant.tsv holds molecules.  The main output, --coverage (unit, nh) and --unprojected\n"
          "still see every record.  Not with --quant-bam or --coverage-weight em.  --dedup-stats FILE: size<TAB>molecules, a line per\n"
          "molecule size that occurs.  --dedup-bam FILE: the projected records under the header the output has without --sort, without\n"
          "the duplicate names' (--dedup-bam-mode remove, the default) or all of them, the duplicates' with flag 0x400 (mark).  One more\n"
          "line in front of the final report: [bramble] dedup: M molecules of N read names (D duplicates, U without UMI; G position groups; method unique|directional; add X.XXs, finish Y.YYs)\n"
          "--cells PREFIX: a single-cell count matrix on one GPU, beside --quant: the cell barcode of a read name is what lies between\n"
          "the last two --dedup-umi-sep characters (default _) of the read name (--cells-barcode name, the default: umi_tools extract's\n"
          "READ_CB_UMI) or the value of the --cells-barcode-tag tag (default CB; --cells-barcode tag), at most 32 bytes; a read name\n"
          "without one is in no cell.  The features are genes (--cells-features gene, the default: the gene_id of the annotation or\n"
          "--quant-gene-map, as for --quant-genes) or transcripts.  A read name whose transcripts span several features counts for none\n"
          "(--cells-multi unique, the default: integer counts), for each an equal share (uniform) or the shares of an EM run per cell on\n"
          "the GPU (em: STARsolo's and alevin's estimator).  PREFIXmatrix.mtx (Matrix Market, features x cells, the 10x layout),\n"
          "PREFIXbarcodes.tsv, PREFIXfeatures.tsv and PREFIXcells.tsv (Barcode Names Unique Multi Features Iterations); the directory of\n"
          "PREFIX must exist.  The matrix is the raw one unless --cells-whitelist is given; --cells-filter calls the cells.  With --dedup the\n"
          "duplicates are found per cell (umi_tools' --per-cell) and the matrix counts molecules; quant.tsv then reflects the per-cell\n"
          "molecules as well.  One more line in front of the final report: [bramble] cells: C cells, M of N read names counted (B\n"
          "without barcode; Z matrix entries; features gene|transcript; multi unique|uniform|em; add X.XXs, finish Y.YYs)\n"
          "--cells-whitelist FILE: the allowed cell barcodes, plain text, one a line (the first whitespace-delimited field, 32 bytes at\n"
          "most; empty lines and lines starting with # are skipped; not compressed).  Every observed barcode is mapped onto the list on\n"
          "the GPU before the cells and, with --dedup, the per-cell duplicate groups are made.  --cells-correct exact: only barcodes\n"
          "on the list; 1mm (the default, STARsolo's 1MM): a barcode not on the list becomes the one entry that differs from it in one\n"
          "base, and is dropped when there are several or none; 1mm-multi (1MM_multi): among several the one most read names carry\n"
          "exactly, dropped on a tie.  A read name whose barcode is dropped is in no cell.  The barcodes printed are entries of the\n"
          "list; PREFIXcells.tsv gains a last column Corrected.  One more line: [bramble] whitelist: W barcodes; B read names with a\n"
          "barcode: X exact, C corrected, R without match, A ambiguous (D distinct observed; correct exact|1mm|1mm-multi; build\n"
          "X.XXs, resolve Y.YYs)\n"
          "--cells-filter METHOD: the cells are called on the GPU, on their unique counts whatever --cells-multi is, by definitions\n"
          "modelled on STARsolo's --soloCellFilter (not compared with its or CellRanger's output).  topcells: the --cells-expected N\n"
          "(3000) barcodes with the most counts, ties included.  cr2.2: every barcode with at least 1 / --cells-filter-ratio (10) of\n"
          "the count at rank N * (1 - --cells-filter-percentile (0.99)).  emptydrops: those, and of the --cells-ed-candidates (20000)\n"
          "next barcodes with --cells-ed-umi-min (500) counts and --cells-ed-umi-frac (0.01) of the median cell's or more the ones\n"
          "whose counts the ambient profile -- the barcodes at ranks --cells-ed-window LO,HI (45000,90000), Good-Turing smoothed --\n"
          "does not explain: --cells-ed-sims (10000) multinomial simulations under --quant-seed, Benjamini-Hochberg at --cells-ed-fdr\n"
          "(0.01).  PREFIXfiltered_matrix.mtx and PREFIXfiltered_barcodes.tsv (the called cells; features.tsv serves both) and\n"
          "PREFIXcalls.tsv (Barcode Total Rank Status LogLik Lower PValue PAdj; status 1: by count, 2: by emptydrops; a dot where a\n"
          "barcode was no candidate).  One more line: [bramble] cell calling: C of K cells called (...)\n");
}
// a whole number in [lo, hi] / a real in [lo, hi]; false: said
bool parse_count(const char *opt, const char *s, long long lo, long long hi, long long &v) {
  char *e; errno = 0; const long long x = strtoll(s, &e, 10);
  if (e == s || *e || errno || x < lo || x > hi) { fprintf(stderr, "%s: %s is not a whole number in %lld .. %lld\n", opt, s, lo, hi); return false; }
  v = x; return true;
}
bool parse_real(const char *opt, const char *s, double lo, double hi, double &v) {
  char *e; const double x = strtod(s, &e);
  if (e == s || *e || !(x >= lo && x <= hi)) { fprintf(stderr, "%s: %s is not a number in %g .. %g\n", opt, s, lo, hi); return false; }
  v = x; return true;
}
bool parse_u32(const char *s, uint32_t &v) { char *e; unsigned long x = strtoul(s, &e, 10); if (e == s || *e) return false; v = (uint32_t)x; return true; }

// returns 0 to continue, 1 to exit(0), <0 on error
int parse_args(int argc, char **argv, Options &o) {
  memset(&o.cfg, 0, sizeof(o.cfg));
  o.cfg.junc_miss_discount = 1.0;
  bool codec = false, host_codec = false;   // a BGZF codec option was given; one that asks for the host codec
  bool coverage_bigwig_switch_given = false;
  bool coverage_weight_given = false, unprojected_scope_given = false, quant_bam_mode_given = false, dedup_switch_given = false, dedup_bam_mode_given = false, cells_switch_given = false, cells_correct_given = false, cells_filter_switch_given = false;
  auto need = [&](int &i) -> const char * { if (i + 1 >= argc) { fprintf(stderr, "%s: missing value\n", argv[i]); return nullptr; } return argv[++i]; };
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    std::string val; bool has_eq = false;
    if (a.rfind("--", 0) == 0) { size_t eq = a.find('='); if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_eq = true; } }
    auto value = [&]() -> const char * { if (has_eq) return val.c_str(); return need(i); };
    if (a == "--help" || a == "-h") { usage(stdout); return 1; }
    else if (a == "--version" || a == "-V") { printf("version: %s (bramble_amd %s)\n", BRAMBLE_REF_VERSION, br_version()); return 1; }
    else if (a == "--quiet" || a == "-q") o.quiet = true;          // -q: bramble-cli/src/cli.rs:60
    else if (a == "--fr") o.cfg.fr = 1;
    else if (a == "--rf") o.cfg.rf = 1;
    else if (a == "--lr") o.cfg.lr = 1;
    else if (a == "--lr-hq" || a == "--lr:hq") o.cfg.lr_hq = 1;    // Rust spelling: bramble-cli/src/cli.rs:32
    else if (a == "--unordered") {}                                // bramble-cli/src/cli.rs:64: the order here is always the input order
    else if (a == "--unordered-flush-records") { if (!value()) return -1; }
    else if (a == "--strict") o.cfg.strict = 1;
    else if (a == "--max-soft-clip") { const char *v = value(); if (!v || !parse_u32(v, o.cfg.max_clip)) return -1; o.cfg.has_max_clip = 1; }
    else if (a == "--max-junction-insertion") { const char *v = value(); if (!v || !parse_u32(v, o.cfg.max_junc_ins)) return -1; o.cfg.has_max_junc_ins = 1; }
    else if (a == "--max-junction-deletion") { const char *v = value(); if (!v || !parse_u32(v, o.cfg.max_junc_gap)) return -1; o.cfg.has_max_junc_gap = 1; }
    else if (a == "--max-error-exon") { const char *v = value(); if (!v || !parse_u32(v, o.cfg.max_error_exon)) return -1; o.cfg.has_max_error_exon = 1; }
    else if (a == "--similarity-threshold") { const char *v = value(); if (!v) return -1; o.cfg.sim_thr = strtof(v, nullptr); o.cfg.has_sim_thr = 1; }
    else if (a == "-G" || a == "--guide") { const char *v = value(); if (!v) return -1; o.gff = v; }
    else if (a == "-S" || a == "--genome") { const char *v = value(); if (!v) return -1; o.fasta = v; }
    else if (a == "-o" || a == "--out") { const char *v = value(); if (!v) return -1; o.out_bam = v; }
    else if (a == "-p" || a == "--threads") { const char *v = value(); if (!v) return -1; o.threads = atoi(v); if (o.threads < 1) o.threads = 1; }
    else if (a == "--compression-level") { const char *v = value(); if (!v) return -1; o.level = atoi(v); if (o.level < 0 || o.level > 9) return -1; o.device_deflate = false; codec = host_codec = true; }
    else if (a == "--host-deflate") { o.device_deflate = false; codec = host_codec = true; }
    else if (a == "-O" || a == "--output-fmt") {
      const char *v = value(); if (!v) return -1;
      std::string f = v;
      for (auto &ch : f) ch = (char)tolower((unsigned char)ch);
      if (f == "sam") o.sam_out = true;
      else if (f == "bam") o.sam_out = false;
      else { fprintf(stderr, "--output-fmt: unknown format %s (bam or sam)\n", v); return -1; }
    }
    else if (a == "--bundle-size") { const char *v = value(); if (!v) return -1; o.bundle_records = atoll(v); if (o.bundle_records < 1) return -1; }
    else if (a == "--device-deflate") { o.device_deflate = true; codec = true; }
    else if (a == "--device-reader") o.device_reader = 1;
    else if (a == "--host-reader") o.device_reader = 0;
    else if (a == "--collate") o.collate = true;
    else if (a == "--sort") o.sort = true;
    else if (a == "--write-index") o.write_index = true;
    else if (a == "--quant") { const char *v = value(); if (!v) return -1; o.quant = v; }
    else if (a == "--quant-classes") { const char *v = value(); if (!v) return -1; o.quant_classes = v; }
    else if (a == "--quant-length-norm") o.quant_length_norm = 1;
    else if (a == "--quant-no-length-norm") o.quant_length_norm = 0;
    else if (a == "--quant-eff-length") o.quant_eff_length = true;
    else if (a == "--quant-fld") { const char *v = value(); if (!v) return -1; o.quant_fld = v; }
    else if (a == "--quant-bootstraps") {
      const char *v = value(); if (!v) return -1;
      char *e; const long long b = strtoll(v, &e, 10);
      if (e == v || *e || b < 1 || b > 10000) { fprintf(stderr, "--quant-bootstraps: %s is not a number of replicates from 1 to 10000\n", v); return -1; }
      o.quant_bootstraps = (int)b;
    }
    else if (a == "--quant-seed") {
      const char *v = value(); if (!v) return -1;
      char *e; errno = 0; const long long x = strtoll(v, &e, 10);
      if (e == v || *e || errno) { fprintf(stderr, "--quant-seed: %s is not a 64-bit integer\n", v); return -1; }
      o.quant_seed = x; o.quant_seed_given = true;
    }
    else if (a == "--quant-vb") o.quant_vb = true;
    else if (a == "--quant-vb-per-nucleotide") o.quant_vb_per_nt = true;
    else if (a == "--quant-vb-prior") {
      const char *v = value(); if (!v) return -1;
      char *e = nullptr; const double x = strtod(v, &e);
      if (e == v || *e || !(x >= 0.0) || !isfinite(x)) { fprintf(stderr, "--quant-vb-prior: %s is not a finite number >= 0\n", v); return -1; }
      o.quant_vb_prior = x; o.quant_vb_prior_given = true;
    }
    else if (a == "--quant-boot-out") { const char *v = value(); if (!v) return -1; o.quant_boot_out = v; }
    else if (a == "--quant-genes") { const char *v = value(); if (!v) return -1; o.quant_genes = v; }
    else if (a == "--quant-gene-classes") { const char *v = value(); if (!v) return -1; o.quant_gene_classes = v; }
    else if (a == "--quant-gene-map") { const char *v = value(); if (!v) return -1; o.quant_gene_map = v; }
    else if (a == "--coverage") { const char *v = value(); if (!v) return -1; o.coverage = v; }
    else if (a == "--coverage-summary") { const char *v = value(); if (!v) return -1; o.coverage_summary = v; }
    else if (a == "--coverage-primary") o.coverage_primary = true;
    else if (a == "--coverage-bigwig") { const char *v = value(); if (!v) return -1; o.coverage_bigwig = v; }
    else if (a == "--coverage-bigwig-zooms") {
      const char *v = value(); long long z = 0;
      if (!v || !parse_count("--coverage-bigwig-zooms", v, 0, 10, z)) return -1;
      o.coverage_bigwig_zooms = (int)z; coverage_bigwig_switch_given = true;
    }
    else if (a == "--coverage-bigwig-uncompressed") { o.coverage_bigwig_uncompressed = true; coverage_bigwig_switch_given = true; }
    else if (a == "--coverage-weight") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "unit") o.coverage_weight = 0; else if (w == "nh") o.coverage_weight = 1; else if (w == "em") o.coverage_weight = 2;
      else { fprintf(stderr, "--coverage-weight: unknown weight %s (unit, nh or em)\n", v); return -1; }
      coverage_weight_given = true;
    }
    else if (a == "--unprojected") { const char *v = value(); if (!v) return -1; o.unprojected = v; }
    else if (a == "--unprojected-scope") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "record") o.unprojected_scope = 1; else if (w == "name") o.unprojected_scope = 2;
      else { fprintf(stderr, "--unprojected-scope: unknown scope %s (record or name)\n", v); return -1; }
      unprojected_scope_given = true;
    }
    else if (a == "--quant-bam") { const char *v = value(); if (!v) return -1; o.quant_bam = v; }
    else if (a == "--quant-bam-mode") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "tag") o.quant_bam_mode = 0; else if (w == "sample") o.quant_bam_mode = 1;
      else { fprintf(stderr, "--quant-bam-mode: unknown mode %s (tag or sample)\n", v); return -1; }
      quant_bam_mode_given = true;
    }
    else if (a == "--dedup") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "unique") o.dedup = 0; else if (w == "directional") o.dedup = 1;
      else { fprintf(stderr, "--dedup: unknown method %s (unique or directional)\n", v); return -1; }
    }
    else if (a == "--dedup-umi") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "name") o.dedup_umi = 0; else if (w == "tag") o.dedup_umi = 1;
      else { fprintf(stderr, "--dedup-umi: unknown source %s (name or tag)\n", v); return -1; }
      dedup_switch_given = true;
    }
    else if (a == "--dedup-umi-sep") {
      const char *v = value(); if (!v) return -1;
      if (strlen(v) != 1) { fprintf(stderr, "--dedup-umi-sep: %s is not one character\n", v); return -1; }
      o.dedup_umi_sep = (unsigned char)v[0]; dedup_switch_given = true;
    }
    else if (a == "--dedup-umi-tag") {
      const char *v = value(); if (!v) return -1;
      if (strlen(v) != 2) { fprintf(stderr, "--dedup-umi-tag: %s is not a two-character tag\n", v); return -1; }
      o.dedup_umi_tag = (unsigned char)v[0] | (unsigned char)v[1] << 8; dedup_switch_given = true;
    }
    else if (a == "--cells") { const char *v = value(); if (!v) return -1; o.cells = v; }
    else if (a == "--cells-barcode") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "name") o.cells_barcode = 0; else if (w == "tag") o.cells_barcode = 1;
      else { fprintf(stderr, "--cells-barcode: unknown source %s (name or tag)\n", v); return -1; }
      cells_switch_given = true;
    }
    else if (a == "--cells-barcode-tag") {
      const char *v = value(); if (!v) return -1;
      if (strlen(v) != 2) { fprintf(stderr, "--cells-barcode-tag: %s is not a two-character tag\n", v); return -1; }
      o.cells_barcode_tag = (unsigned char)v[0] | (unsigned char)v[1] << 8; cells_switch_given = true;
    }
    else if (a == "--cells-features") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "gene") o.cells_features = 0; else if (w == "transcript") o.cells_features = 1;
      else { fprintf(stderr, "--cells-features: unknown features %s (gene or transcript)\n", v); return -1; }
      cells_switch_given = true;
    }
    else if (a == "--cells-whitelist") { const char *v = value(); if (!v) return -1; o.cells_whitelist = v; }
    else if (a == "--cells-correct") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "exact") o.cells_correct = 0; else if (w == "1mm") o.cells_correct = 1; else if (w == "1mm-multi") o.cells_correct = 2;
      else { fprintf(stderr, "--cells-correct: unknown mode %s (exact, 1mm or 1mm-multi)\n", v); return -1; }
      cells_correct_given = true;
    }
    else if (a == "--cells-multi") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "unique") o.cells_multi = 0; else if (w == "uniform") o.cells_multi = 1; else if (w == "em") o.cells_multi = 2;
      else { fprintf(stderr, "--cells-multi: unknown mode %s (unique, uniform or em)\n", v); return -1; }
      cells_switch_given = true;
    }
    else if (a == "--cells-filter") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "topcells") o.cells_filter = 0; else if (w == "cr2.2") o.cells_filter = 1; else if (w == "emptydrops") o.cells_filter = 2;
      else { fprintf(stderr, "--cells-filter: unknown method %s (topcells, cr2.2 or emptydrops)\n", v); return -1; }
    }
    else if (a == "--cells-expected") { const char *v = value(); if (!v || !parse_count("--cells-expected", v, 1, 0x7fffffffll, o.cells_expected)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-filter-percentile") { const char *v = value(); if (!v || !parse_real("--cells-filter-percentile", v, 0.0, 1.0, o.cells_percentile)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-filter-ratio") { const char *v = value(); if (!v || !parse_real("--cells-filter-ratio", v, 1.0, 1e9, o.cells_ratio)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-ed-window") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      const size_t comma = w.find(',');
      if (comma == std::string::npos || !parse_count("--cells-ed-window", w.substr(0, comma).c_str(), 0, 0x7fffffffll, o.cells_ed_lo) ||
          !parse_count("--cells-ed-window", w.substr(comma + 1).c_str(), 0, 0x7fffffffll, o.cells_ed_hi) || o.cells_ed_lo >= o.cells_ed_hi) {
        fprintf(stderr, "--cells-ed-window: %s is not LO,HI with LO < HI\n", v); return -1;
      }
      cells_filter_switch_given = true;
    }
    else if (a == "--cells-ed-umi-min") { const char *v = value(); if (!v || !parse_count("--cells-ed-umi-min", v, 0, 0xffffffffll, o.cells_ed_umi_min)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-ed-umi-frac") { const char *v = value(); if (!v || !parse_real("--cells-ed-umi-frac", v, 0.0, 1.0, o.cells_ed_umi_frac)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-ed-candidates") { const char *v = value(); if (!v || !parse_count("--cells-ed-candidates", v, 1, 0x7fffffffll, o.cells_ed_candidates)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-ed-fdr") { const char *v = value(); if (!v || !parse_real("--cells-ed-fdr", v, 0.0, 1.0, o.cells_ed_fdr)) return -1; cells_filter_switch_given = true; }
    else if (a == "--cells-ed-sims") { const char *v = value(); if (!v || !parse_count("--cells-ed-sims", v, 1, 0x7fffffffll, o.cells_ed_sims)) return -1; cells_filter_switch_given = true; }
    else if (a == "--dedup-stats") { const char *v = value(); if (!v) return -1; o.dedup_stats = v; dedup_switch_given = true; }
    else if (a == "--dedup-bam") { const char *v = value(); if (!v) return -1; o.dedup_bam = v; dedup_switch_given = true; }
    else if (a == "--dedup-bam-mode") {
      const char *v = value(); if (!v) return -1;
      const std::string w = v;
      if (w == "remove") o.dedup_bam_mode = 0; else if (w == "mark") o.dedup_bam_mode = 1;
      else { fprintf(stderr, "--dedup-bam-mode: unknown mode %s (remove or mark)\n", v); return -1; }
      dedup_switch_given = dedup_bam_mode_given = true;
    }
    else if (a == "--device") { const char *v = value(); if (!v) return -1; o.devices.assign(1, atoi(v)); }
    else if (a == "--devices") {
      const char *v = value(); if (!v) return -1;
      o.devices.clear();
      for (const char *q = v; *q;) { char *e; long d = strtol(q, &e, 10); if (e == q || d < 0) return -1; o.devices.push_back((int)d); q = *e == ',' ? e + 1 : e; if (*e && *e != ',') return -1; }
      if (o.devices.empty() || o.devices.size() > 64) return -1;
    }
    else if (!a.empty() && a[0] == '-' && a != "-") { fprintf(stderr, "unknown option %s\n", a.c_str()); return -1; }
    else if (o.in_bam.empty()) o.in_bam = a;
    else { fprintf(stderr, "unexpected argument %s\n", a.c_str()); return -1; }
  }
  if (o.in_bam.empty()) { fprintf(stderr, "an input (in.bam, in.sam or -) is required\n"); return -1; }
  if (o.out_bam.empty()) { fprintf(stderr, "--out is required\n"); return -1; }
  if (o.gff.empty()) { fprintf(stderr, "--guide is required\n"); return -1; }
  if (!o.fasta.empty()) o.cfg.use_fasta = 1;
  if (o.sam_out && codec) { fprintf(stderr, "--compression-level, --host-deflate and --device-deflate apply to BAM output, not to --output-fmt sam\n"); return -1; }
  if (o.collate && o.devices.size() > 1) { fprintf(stderr, "--collate works on one device: give --device N, not a --devices list\n"); return -1; }
  if (o.sort && o.devices.size() > 1) { fprintf(stderr, "--sort works on one device: give --device N, not a --devices list\n"); return -1; }
  if (!o.cells.empty() && o.devices.size() > 1) { fprintf(stderr, "--cells works on one device: give --device N, not a --devices list\n"); return -1; }
  if (!o.quant.empty() && o.devices.size() > 1) { fprintf(stderr, "--quant works on one device: give --device N, not a --devices list\n"); return -1; }
  if (o.quant.empty() && (!o.quant_classes.empty() || o.quant_length_norm >= 0)) { fprintf(stderr, "--quant-classes, --quant-length-norm and --quant-no-length-norm need --quant\n"); return -1; }
  if (o.quant.empty() && (o.quant_eff_length || !o.quant_fld.empty())) { fprintf(stderr, "--quant-eff-length and --quant-fld need --quant\n"); return -1; }
  if (o.quant.empty() && !o.quant_bam.empty()) { fprintf(stderr, "--quant-bam needs --quant: the weights are the EM's posteriors\n"); return -1; }
  if (quant_bam_mode_given && o.quant_bam.empty()) { fprintf(stderr, "--quant-bam-mode needs --quant-bam\n"); return -1; }
  if (o.quant_bam == "-") { fprintf(stderr, "--quant-bam needs a file, not standard output: that is the main output's\n"); return -1; }
  if (!o.quant_bam.empty() && o.devices.size() > 1) { fprintf(stderr, "--quant-bam works on one device: give --device N, not a --devices list\n"); return -1; }
  if (o.quant.empty() && (o.quant_bootstraps || o.quant_seed_given || !o.quant_boot_out.empty())) { fprintf(stderr, "--quant-bootstraps, --quant-seed and --quant-boot-out need --quant\n"); return -1; }
  if (o.quant.empty() && (o.quant_vb || o.quant_vb_prior_given || o.quant_vb_per_nt)) { fprintf(stderr, "--quant-vb, --quant-vb-prior and --quant-vb-per-nucleotide need --quant\n"); return -1; }
  if (!o.quant_vb && (o.quant_vb_prior_given || o.quant_vb_per_nt)) { fprintf(stderr, "--quant-vb-prior and --quant-vb-per-nucleotide need --quant-vb: without it there is no prior\n"); return -1; }
  if (o.quant_vb_per_nt && (o.quant_length_norm == 0 || ((o.cfg.lr || o.cfg.lr_hq) && o.quant_length_norm != 1))) { fprintf(stderr, "--quant-vb-per-nucleotide needs length normalisation: the prior is scaled by the length the reads are weighted by (not with --quant-no-length-norm; under --lr / --lr-hq only with --quant-length-norm)\n"); return -1; }
  if (o.quant.empty() && !o.quant_genes.empty()) { fprintf(stderr, "--quant-genes needs --quant\n"); return -1; }
  const bool cell_genes = !o.cells.empty() && o.cells_features == 0;   // (--cells takes its genes where --quant-genes does)
  if (o.quant_genes.empty() && (!o.quant_gene_classes.empty() || (!o.quant_gene_map.empty() && !cell_genes))) { fprintf(stderr, "--quant-gene-classes and --quant-gene-map need --quant-genes\n"); return -1; }
  if (cells_switch_given && o.cells.empty()) { fprintf(stderr, "--cells-barcode, --cells-barcode-tag, --cells-features and --cells-multi need --cells\n"); return -1; }
  if (!o.cells_whitelist.empty() && o.cells.empty()) { fprintf(stderr, "--cells-whitelist needs --cells\n"); return -1; }
  if (o.cells_filter >= 0 && o.cells.empty()) { fprintf(stderr, "--cells-filter needs --cells\n"); return -1; }
  if (cells_filter_switch_given && o.cells_filter < 0) { fprintf(stderr, "--cells-expected, --cells-filter-percentile, --cells-filter-ratio and the --cells-ed switches need --cells-filter\n"); return -1; }
  if (cells_correct_given && o.cells_whitelist.empty()) { fprintf(stderr, "--cells-correct needs --cells-whitelist\n"); return -1; }
  if (!o.cells.empty() && o.quant.empty()) { fprintf(stderr, "--cells needs --quant: the matrix is made from the quantifier's classes\n"); return -1; }
  if (!o.quant_boot_out.empty() && !o.quant_bootstraps) { fprintf(stderr, "--quant-boot-out needs --quant-bootstraps: without it there are no replicates\n"); return -1; }
  if (!o.quant_fld.empty() && !o.quant_eff_length) { fprintf(stderr, "--quant-fld needs --quant-eff-length: without it no fragment lengths are counted\n"); return -1; }
  if (o.quant_eff_length && o.quant_length_norm == 0) { fprintf(stderr, "--quant-eff-length is a length normalisation: not with --quant-no-length-norm\n"); return -1; }
  if (o.quant_eff_length && (o.cfg.lr || o.cfg.lr_hq) && o.quant_length_norm != 1) { fprintf(stderr, "--quant-eff-length under --lr / --lr-hq needs --quant-length-norm: long reads are not length-normalised by default\n"); return -1; }
  const bool coverage_wanted = !o.coverage.empty() || !o.coverage_summary.empty() || !o.coverage_bigwig.empty();
  if (o.coverage_primary && !coverage_wanted) { fprintf(stderr, "--coverage-primary needs --coverage, --coverage-summary or --coverage-bigwig\n"); return -1; }
  if (coverage_weight_given && !coverage_wanted) { fprintf(stderr, "--coverage-weight needs --coverage, --coverage-summary or --coverage-bigwig\n"); return -1; }
  if (coverage_bigwig_switch_given && o.coverage_bigwig.empty()) { fprintf(stderr, "--coverage-bigwig-zooms and --coverage-bigwig-uncompressed need --coverage-bigwig\n"); return -1; }
  if (o.coverage_weight == 2 && o.quant.empty()) { fprintf(stderr, "--coverage-weight em needs --quant: the weights are the EM's posteriors\n"); return -1; }
  if (coverage_wanted && o.devices.size() > 1) { fprintf(stderr, "--coverage works on one device: give --device N, not a --devices list\n"); return -1; }
  if (unprojected_scope_given && o.unprojected.empty()) { fprintf(stderr, "--unprojected-scope needs --unprojected\n"); return -1; }
  if (o.unprojected == "-") { fprintf(stderr, "--unprojected needs a file, not standard output: that is the main output's\n"); return -1; }
  if (!o.unprojected.empty() && o.devices.size() > 1) { fprintf(stderr, "--unprojected works on one device: give --device N, not a --devices list\n"); return -1; }
  if (dedup_switch_given && o.dedup < 0) { fprintf(stderr, "--dedup-umi, --dedup-umi-sep, --dedup-umi-tag, --dedup-stats, --dedup-bam and --dedup-bam-mode need --dedup\n"); return -1; }
  if (dedup_bam_mode_given && o.dedup_bam.empty()) { fprintf(stderr, "--dedup-bam-mode needs --dedup-bam\n"); return -1; }
  if (o.dedup_bam == "-") { fprintf(stderr, "--dedup-bam needs a file, not standard output: that is the main output's\n"); return -1; }
  if (o.dedup >= 0 && o.devices.size() > 1) { fprintf(stderr, "--dedup works on one device: give --device N, not a --devices list\n"); return -1; }
  if (o.dedup >= 0 && !o.quant_bam.empty()) { fprintf(stderr, "--dedup not with --quant-bam: the posterior BAM needs a class for every read name with records, and the duplicate names have none\n"); return -1; }
  if (o.dedup >= 0 && o.coverage_weight == 2) { fprintf(stderr, "--dedup not with --coverage-weight em: the weighted coverage needs a class for every read name with records, and the duplicate names have none\n"); return -1; }
  if (o.write_index && !o.sort) { fprintf(stderr, "--write-index needs --sort: a BAI index describes a coordinate-sorted file\n"); return -1; }
  if (o.write_index && o.sam_out) { fprintf(stderr, "--write-index applies to BAM output, not to --output-fmt sam\n"); return -1; }
  if (o.write_index && o.out_bam == "-") { fprintf(stderr, "--write-index needs an output file, not standard output\n"); return -1; }
  if (o.write_index && host_codec) { fprintf(stderr, "--write-index works with the device deflate, not with --host-deflate or --compression-level\n"); return -1; }
  return 0;
}

// ---- FASTA (plain or gzip): name = first word of the '>' line ---------------------------------
struct Fasta { std::vector<std::string> names, seqs; };
bool load_fasta(const char *path, Fasta &fa) {
  gzFile f = gzopen(path, "rb");
  if (!f) return false;
  gzbuffer(f, 1 << 20);
  std::vector<char> buf(1 << 16);
  while (gzgets(f, buf.data(), (int)buf.size())) {
    char *s = buf.data();
    size_t n = strlen(s);
    bool full = n && s[n - 1] == '\n';
    while (n && (s[n - 1] == '\n' || s[n - 1] == '\r')) n--;
    if (s[0] == '>') {
      size_t e = 1; while (e < n && s[e] != ' ' && s[e] != '\t') e++;
      fa.names.emplace_back(s + 1, e - 1); fa.seqs.emplace_back();
      while (!full && gzgets(f, buf.data(), (int)buf.size())) { size_t m = strlen(buf.data()); full = m && buf[m - 1] == '\n'; }
    } else if (!fa.seqs.empty()) fa.seqs.back().append(s, n);
  }
  gzclose(f);
  return true;
}

// ---- output header ------------------------------------------------------------------------------
// src/bramble.cpp:513-623: @HD first, one @SQ per transcript in guide order, then every other input
// line except @SQ / @HD (with the new @PG appended the way sam_hdr_add_pg chains it), then the @CO line.
// --sort: the @HD line with SO:coordinate -- the input's fields in their order, SO replaced (appended when absent), GO and SS
// dropped (they describe another order); "@HD VN:1.6 SO:coordinate" when the input has no such line
std::string sorted_hd_line(const std::string &hd) {
  if (hd.empty()) return "@HD\tVN:1.6\tSO:coordinate";
  std::string out = "@HD";
  bool so = false;
  for (size_t a = hd.find('\t'); a != std::string::npos;) {
    const size_t b = hd.find('\t', a + 1);
    const std::string f = hd.substr(a + 1, b == std::string::npos ? std::string::npos : b - a - 1);
    a = b;
    if (f.compare(0, 3, "GO:") == 0 || f.compare(0, 3, "SS:") == 0 || f.empty()) continue;
    if (f.compare(0, 3, "SO:") == 0) { if (!so) out += "\tSO:coordinate"; so = true; continue; }
    out += '\t'; out += f;
  }
  if (!so) out += "\tSO:coordinate";
  return out;
}

std::string make_header_text(const std::string &in_text, const br_index *ix, const std::string &cl, const std::string &gff, bool sorted) {
  std::vector<std::string> lines;
  for (size_t a = 0; a < in_text.size();) { size_t b = in_text.find('\n', a); if (b == std::string::npos) b = in_text.size(); if (b > a) lines.emplace_back(in_text, a, b - a); a = b + 1; }
  std::string out;
  if (sorted) {
    std::string hd;
    for (auto &l : lines) if (l.compare(0, 3, "@HD") == 0 && hd.empty()) hd = l;
    out += sorted_hd_line(hd); out += '\n';
  } else
    for (auto &l : lines) if (l.compare(0, 3, "@HD") == 0) { out += l; out += '\n'; }
  size_t nt = br_index_num_transcripts(ix);
  for (size_t t = 0; t < nt; t++) {
    int64_t len = br_index_transcript_len(ix, (uint32_t)t);
    if (len > 0) { out += "@SQ\tSN:"; out += br_index_transcript_name(ix, (uint32_t)t); out += "\tLN:"; out += std::to_string(len); out += '\n'; }
  }
  // @PG chain ends: ids no other @PG names as its PP (htslib sam_hdr_add_pg links the new record to each)
  std::vector<std::string> pg_ids, pg_pp;
  auto field = [](const std::string &l, const char *key) -> std::string {
    size_t p = 0;
    while ((p = l.find('\t', p)) != std::string::npos) { p++; if (l.compare(p, 3, key) == 0) { size_t e = l.find('\t', p); return l.substr(p + 3, e == std::string::npos ? std::string::npos : e - p - 3); } }
    return "";
  };
  for (auto &l : lines) if (l.compare(0, 3, "@PG") == 0) { pg_ids.push_back(field(l, "ID:")); pg_pp.push_back(field(l, "PP:")); }
  std::vector<std::string> ends;
  for (auto &id : pg_ids) { bool used = false; for (auto &pp : pg_pp) if (pp == id) used = true; if (!used && !id.empty()) ends.push_back(id); }
  for (auto &l : lines) if (l.compare(0, 3, "@SQ") != 0 && l.compare(0, 3, "@HD") != 0) { out += l; out += '\n'; }
  auto unique_id = [&](int &serial) { for (;;) { std::string id = serial ? "bramble." + std::to_string(serial) : "bramble"; serial++; bool clash = false; for (auto &x : pg_ids) if (x == id) clash = true; if (!clash) { pg_ids.push_back(id); return id; } } };
  int serial = 0;
  auto pg_line = [&](const std::string &pp) {
    std::string l = "@PG\tID:" + unique_id(serial) + "\tPN:bramble";
    if (!pp.empty()) l += "\tPP:" + pp;
    l += "\tVN:" BRAMBLE_REF_VERSION "+amd." + std::string(br_version()) + "\tCL:" + cl + "\n";
    return l;
  };
  if (ends.empty()) out += pg_line("");
  else for (auto &e : ends) out += pg_line(e);
  out += "@CO\tGenerated from GTF: " + gff + "\n";
  return out;
}

std::vector<uint8_t> make_bam_header(const std::string &text, const br_index *ix) {
  std::vector<uint8_t> o;
  auto p32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(v >> (8 * k))); };
  o.insert(o.end(), {'B', 'A', 'M', 1});
  p32((uint32_t)text.size()); o.insert(o.end(), text.begin(), text.end());
  size_t nt = br_index_num_transcripts(ix);
  uint32_t n_sq = 0;
  for (size_t t = 0; t < nt; t++) if (br_index_transcript_len(ix, (uint32_t)t) > 0) n_sq++;
  p32(n_sq);
  for (size_t t = 0; t < nt; t++) {
    int64_t len = br_index_transcript_len(ix, (uint32_t)t);
    if (len <= 0) continue;
    const char *nm = br_index_transcript_name(ix, (uint32_t)t);
    uint32_t l = (uint32_t)strlen(nm) + 1;
    p32(l); o.insert(o.end(), nm, nm + l); p32((uint32_t)len);
  }
  return o;
}

// One worker per listed device: its own index replica and context (the reference's workers share one read-only tree,
// src/threads.cpp:114-162; here every GPU holds a copy), an uploader thread (host bundles only) and a projecting thread.
// Workers take bundles from the input's queue as they become free -- no exchange between them; the writer restores bundle
// order (bramble-cli/src/pipeline.rs:226-240 keeps a BTreeMap for the same purpose).
struct Staged { std::unique_ptr<Bundle> b; int slot; int rc; };
struct Worker {
  int id = 0, device = 0;
  br_index *ix = nullptr; br_ctx *ctx = nullptr;
  int build_rc = 0;
  Slot<Staged> to_main{2};
  std::mutex permit_m; std::condition_variable permit_cv; int permits = 3;   // three device staging slots
  std::mutex done_m; std::condition_variable done_cv; uint64_t produced = 0, written = 0;  // chunks handed to / finished by the writer
  std::thread uploader, runner;
  uint64_t total_complete = 0, total_unique = 0, dropped = 0, n_bundles = 0;
  double gpu_seconds = 0, t_upload = 0, t_wait_in = 0;
};

// the output goes to a temporary name next to the target and is renamed on success: a failed run leaves no file that
// looks complete (a truncated stream with a valid EOF block)
struct OutFile {
  explicit OutFile(const std::string &p) : path(p), tmp(p == "-" ? p : p + ".tmp-bramble"), to_stdout(p == "-") {}
  const std::string path, tmp;
  const bool to_stdout;
  BgzfWriter wr;
  void discard() { wr.abandon(); if (!to_stdout) remove(tmp.c_str()); }   // no EOF block: the stream must not look complete
  bool finish(bool ok) {   // false: the run failed, or closing or renaming the file did (said here)
    if (!ok) { discard(); return false; }
    if (!wr.close()) { fprintf(stderr, "error: %s: %s\n", path.c_str(), wr.error().c_str()); if (!to_stdout) remove(tmp.c_str()); return false; }
    if (!to_stdout && rename(tmp.c_str(), path.c_str()) != 0) { fprintf(stderr, "error: could not rename %s to %s\n", tmp.c_str(), path.c_str()); return false; }
    return true;
  }
};

// the workers and the ordered writer of one run
struct Run {
  const Options &o; Input &in; Outbox &out; BgzfWriter &wr;
  const std::vector<int32_t> &ref_map; std::vector<std::unique_ptr<Worker>> &workers;
  std::vector<std::unique_ptr<Consumer>> &consumers;
  std::vector<Consumer *> order;  // the consumers as add and finish reach them: one that keeps the records comes last
  bool keep = false;              // one of them keeps the records: nothing of a bundle goes to the writer
  bool track_blocks = false;      // --write-index: the writer notes where every BGZF block of the record section starts
  std::vector<br_bgzf_span> spans;
  uint64_t stream_pos = 0;        // uncompressed record bytes written so far
  uint64_t drained_chunks = 0;    // chunks drain() handed to the writer
  std::atomic<int> fail{0};
  std::string writer_err;
  double t_deflate = 0;
  static constexpr uint64_t SORT_PIECE = 128ull << 20;   // record bytes per sorted piece (one deflate / format call and one download)
  void go() {
    for (auto &c : consumers) order.push_back(c.get());
    std::stable_partition(order.begin(), order.end(), [](Consumer *c) { return !c->keeps_records(); });
    keep = !order.empty() && order.back()->keeps_records();
    std::thread writer([this] { write(); });
    for (auto &wp : workers) {
      Worker *w = wp.get();
      if (Slot<Bundle> *q = in.host_queue()) {
        w->uploader = std::thread([this, w, q] { upload(w, *q); });
        w->runner = std::thread([this, w] { run_staged(w); });
      } else w->runner = std::thread([this, w] { run_resident(w, *in.dev_queue((size_t)w->id)); });   // (the bundles are in its HBM already)
    }
    for (auto &w : workers) { if (w->uploader.joinable()) w->uploader.join(); if (w->runner.joinable()) w->runner.join(); }
    for (Consumer *c : order) {   // the device work after the last bundle counts as worker 0's
      if (fail) break;
      Worker *w = workers[0].get();
      if (c->keeps_records()) in.join();   // (the source's last sequence number is final after join)
      auto t0 = now();
      int rc = c->finish();
      if (!rc && c->keeps_records()) rc = drain(w, c);
      w->gpu_seconds += secs(t0, now());
      if (rc) { fprintf(stderr, "error: %s failed on device %d: %s\n", c->failure, w->device, br_strerror(rc)); raise_fail(); }
    }
    out.finish();
    in.join(); writer.join();
  }
  // One failure anywhere stops every runner.  The flag flips under each worker's done_m before its condition variable is
  // notified: a runner that has just evaluated the wait predicate as false holds that mutex until it blocks, so the
  // notification cannot fall between its check and its wait (a lost wakeup would leave it -- and the join -- hanging).
  void raise_fail() {
    for (auto &x : workers) { std::lock_guard<std::mutex> l(x->done_m); fail = 1; }
    in.cancel = true;   // the input stops making bundles nobody will project (the runners keep draining what is queued)
    for (auto &x : workers) x->done_cv.notify_all();
  }
  // ordered writer: chunks arrive tagged with their bundle's sequence number
  void write() {
    OutChunk c;
    while (out.take(c)) {
      auto td0 = now();
      if (c.n) {   // the chunk's bytes may still be on their way from the device
        br_host_bam hb; memset(&hb, 0, sizeof(hb)); hb.data = c.data; hb.n_bytes = c.n;
        int wrc = br_host_bam_wait(workers[(size_t)c.worker]->ctx, &hb);
        if (wrc && writer_err.empty()) { writer_err = std::string("download failed: ") + br_strerror(wrc); raise_fail(); }
      }
      if (writer_err.empty() && c.n && track_blocks && !note_blocks(c)) { writer_err = wr.error().empty() ? "malformed BGZF block from the device" : wr.error(); raise_fail(); }
      if (writer_err.empty() && c.n && !(o.device_deflate || o.sam_out ? wr.write_raw(c.data, (size_t)c.n) : wr.write(c.data, (size_t)c.n))) {
        writer_err = wr.error();
        raise_fail();                      // nothing projected from here on could be written: the runners drain
      }
      t_deflate += secs(td0, now());
      if (c.worker < 0) continue;   // (a piece without records: nothing was produced for it)
      Worker *w = workers[(size_t)c.worker].get();
      { std::lock_guard<std::mutex> l(w->done_m); w->written++; }
      w->done_cv.notify_all();
    }
  }
  // the blocks of a device-deflated chunk: file offset (the header's partial block is closed first) and stream offset of each
  bool note_blocks(const OutChunk &c) {
    if (!wr.flush()) return false;
    const uint64_t at = wr.bytes_out();
    for (uint64_t p = 0; p < c.n;) {
      if (p + 26 > c.n) return false;
      const uint64_t bsize = (uint64_t)(c.data[p + 16] | c.data[p + 17] << 8) + 1;
      if (bsize < 26 || p + bsize > c.n) return false;
      uint32_t isize; memcpy(&isize, c.data + p + bsize - 4, 4);
      spans.push_back(br_bgzf_span{at + p, stream_pos});
      stream_pos += isize; p += bsize;
    }
    return true;
  }
  // the kept records, after the last bundle: piece by piece next_piece -> deflate or format + download (nowait) -> the writer
  int drain(Worker *w, Consumer *c) {
    int rc = 0;
    uint64_t seq = in.next_seq;
    while (!fail) {
      br_device_bam piece;
      rc = c->next_piece(SORT_PIECE, &piece);
      if (rc || piece.n_rows == 0) break;
      { std::unique_lock<std::mutex> l(w->done_m); w->done_cv.wait(l, [&] { return w->written + 2 > w->produced || fail; }); }
      if (fail) break;
      br_host_bam hb;
      rc = br_device_bam_download(w->ctx, &piece, final_mode(), 1, &hb);
      if (rc) break;
      { std::lock_guard<std::mutex> l(w->done_m); w->produced++; }
      out.put(seq++, OutChunk{hb.data, hb.n_bytes, w->id});
      drained_chunks++;
    }
    return rc;
  }
  br_bam_bundle args(Bundle &b) const {
    return br_bam_bundle{b.blob.data(), b.blob.size(), b.off.data(), b.len.data(), (int64_t)b.off.size(), ref_map.data(), (int32_t)ref_map.size(), out_mode()};
  }
  int final_mode() const { return o.sam_out ? BR_OUT_SAM_TEXT : o.device_deflate ? 1 : 0; }   // what the writer gets
  int out_mode() const { return keep ? BR_OUT_RESIDENT : final_mode(); }                       // what a projection call leaves
  // one projection call (none after a failure), once chunk j - 2 of this worker is on disk: the context's two pinned
  // result buffers alternate
  template <typename F>
  void project(Worker *w, br_host_bam &hb, F call) {
    memset(&hb, 0, sizeof(hb));
    if (fail) return;
    { std::unique_lock<std::mutex> l(w->done_m); w->done_cv.wait(l, [&] { return w->written + 2 > w->produced || fail; }); }
    auto t0 = now();
    int prc = fail ? 0 : call(&hb);
    w->gpu_seconds += secs(t0, now());
    if (prc) { fprintf(stderr, "error: projection failed on device %d: %s\n", w->device, br_strerror(prc)); raise_fail(); }
  }
  // the result goes to the writer (after a failure the runners only drain)
  void deliver(Worker *w, uint64_t seq, const br_host_bam &hb) {
    if (fail) return;
    w->total_complete += hb.total_complete; w->total_unique += hb.total_unique; w->dropped += hb.dropped_reads; w->n_bundles++;
    for (Consumer *c : order)
      if (const int rc = c->add(w->ctx)) { fprintf(stderr, "error: the %s could not take a bundle on device %d: %s\n", c->name, w->device, br_strerror(rc)); raise_fail(); return; }
    if (keep) { out.put(seq, OutChunk{nullptr, 0, -1}); return; }   // (the runner sees the bundles in order; nothing for the writer yet)
    { std::lock_guard<std::mutex> l(w->done_m); w->produced++; }
    out.put(seq, OutChunk{hb.data, hb.n_bytes, w->id});
  }
  // uploader: stages bundle k of this worker into device slot k % 3 on the context's copy stream while the runner
  // projects an earlier one; three permits = three slots, a permit returns when a slot's projection is done
  void upload(Worker *w, Slot<Bundle> &q) {
    int64_t k = 0;
    for (;;) {
      auto b = q.take();
      if (!b) break;
      { std::unique_lock<std::mutex> l(w->permit_m); w->permit_cv.wait(l, [&] { return w->permits > 0; }); w->permits--; }
      auto st = std::make_unique<Staged>();
      st->slot = (int)(k++ % 3);
      br_bam_bundle bb = args(*b);
      auto t0 = now();
      st->rc = fail ? 0 : br_bam_bundle_stage(w->ctx, &bb, st->slot);
      w->t_upload += secs(t0, now());
      st->b = std::move(b);
      w->to_main.put(std::move(st));
    }
    w->to_main.finish();
  }
  void run_staged(Worker *w) {
    for (;;) {
      auto tw0 = now();
      auto st = w->to_main.take();
      w->t_wait_in += secs(tw0, now());
      if (!st) break;
      Bundle &b = *st->b;
      if (!fail && st->rc) { fprintf(stderr, "error: upload failed on device %d: %s\n", w->device, br_strerror(st->rc)); raise_fail(); }
      br_bam_bundle bb = args(b);
      br_host_bam hb;
      project(w, hb, [&](br_host_bam *h) { return br_project_bam_staged_nowait(w->ctx, &o.cfg, &bb, st->slot, h); });   // the writer waits for the bytes
      in.recycle(b);
      { std::lock_guard<std::mutex> l(w->permit_m); w->permits++; }
      w->permit_cv.notify_all();
      deliver(w, b.seq, hb);
    }
  }
  void run_resident(Worker *w, Slot<DevBundle> &q) {
    for (;;) {
      auto tw0 = now();
      auto b = q.take();
      w->t_wait_in += secs(tw0, now());
      if (!b) break;
      br_host_bam hb;
      project(w, hb, [&](br_host_bam *h) { return br_project_bam_resident(w->ctx, &o.cfg, &b->recs, ref_map.data(), (int32_t)ref_map.size(), out_mode(), 1, h); });
      b->release();   // (failed or not: the reader may use its chunk again)
      deliver(w, b->seq, hb);
    }
  }
};

}  // namespace

// --quant-gene-map: transcript<TAB>gene lines into `map` (the first line of a transcript counts); every transcript of the guides
// must be there.  false: `err` says what is wrong
static bool load_gene_map(const std::string &path, const br_annotation *ann, std::unordered_map<std::string, std::string> &map, std::string &err) {
  FILE *f = fopen(path.c_str(), "r");
  if (!f) { err = "cannot open the file"; return false; }
  std::string line;
  char buf[65536];
  auto take = [&]() {
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    if (line.empty() || line[0] == '#') return;
    const size_t a = line.find('\t');
    if (a == std::string::npos) return;
    const size_t b = line.find('\t', a + 1);
    std::string gene = line.substr(a + 1, b == std::string::npos ? std::string::npos : b - a - 1);
    if (!gene.empty()) map.emplace(line.substr(0, a), std::move(gene));
  };
  while (fgets(buf, sizeof buf, f)) {
    line += buf;
    if (line.back() != '\n') continue;   // (a line longer than the buffer: read on)
    take();
    line.clear();
  }
  take();
  fclose(f);
  const br_transcript *tx = br_annotation_transcripts(ann);
  for (size_t t = 0, n = br_annotation_num_transcripts(ann); t < n; t++)
    if (!map.count(tx[t].id)) { err = std::string("transcript ") + tx[t].id + " has no gene in it"; return false; }
  return true;
}

static std::atomic<int> g_exit_at_end{0};
extern "C" void br_cli_exit_at_end(int on) { g_exit_at_end.store(on ? 1 : 0); }

extern "C" int br_cli_main(int argc, char **argv) {
  Options o;
  int prc = parse_args(argc, argv, o);
  if (prc > 0) return 0;
  if (prc < 0) { usage(stderr); return 2; }
  std::string cl;
  for (int i = 0; i < argc; i++) { if (i) cl += ' '; cl += argv[i]; }
  auto t_start = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
  if (o.out_bam == "-") o.quiet = true;   // the BAM (or SAM) stream owns standard output
  if (!o.quiet) { printf("\n[bramble] starting version: %s (bramble_amd %s)\n", BRAMBLE_REF_VERSION, br_version()); printf("[bramble] loading reference annotation...\n"); }

  // the guide loader starts first, on a thread of its own: opening the input, reading its header and starting the reader
  // (below) happen beside it instead of in front of it
  br_annotation *ann = nullptr;
  std::future<int> ann_job = std::async(std::launch::async, [&]() { return br_annotation_load_mt(o.gff.c_str(), std::max(1, std::min(o.threads, 32)), &ann); });   // the lines are taken apart by -p threads
  struct AnnJoin { std::future<int> &f; br_annotation *&a; ~AnnJoin() { if (f.valid()) (void)f.get(); if (a) br_annotation_free(a); a = nullptr; } } ann_join{ann_job, ann};   // (an early return: wait for it, drop its result)
  // the devices' first touch (runtime start-up, contexts) happens beside the guide parsing, not in front of the index build
  std::vector<std::thread> warm;
  for (int d : o.devices) warm.emplace_back([d]() { (void)br_device_warmup(d); });
  struct WarmJoin { std::vector<std::thread> &t; ~WarmJoin() { for (auto &x : t) if (x.joinable()) x.join(); } } warm_join{warm};
  int ann_rc = 0;
  auto ann_wait = [&]() { if (ann_job.valid()) ann_rc = ann_job.get(); return ann_rc; };
  // --quant-gene-map is checked against the guides before the input is opened or anything is written
  std::unordered_map<std::string, std::string> gene_map;
  if (std::string gerr; !o.quant_gene_map.empty() && ann_wait() == 0 && !load_gene_map(o.quant_gene_map, ann, gene_map, gerr)) {
    fprintf(stderr, "error: --quant-gene-map %s: %s\n", o.quant_gene_map.c_str(), gerr.c_str());
    return 2;
  }
  Outbox out;
  std::string err;
  std::unique_ptr<Input> in = open_input(o, err);
  if (in && o.collate) in = open_collate(o, std::move(in));
  if (!in || !in->start(out, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 1; }

  // the input is already being read while the guides are parsed and the indexes are built
  std::vector<std::unique_ptr<Worker>> workers;
  std::vector<std::unique_ptr<Consumer>> consumers;
  auto free_all = [&]() {
    consumers.clear();
    for (auto &w : workers) { if (w->ctx) br_ctx_free(w->ctx); if (w->ix) br_index_free(w->ix); w->ctx = nullptr; w->ix = nullptr; }
    if (ann) br_annotation_free(ann);
    ann = nullptr;
  };
  auto give_up = [&]() { free_all(); in->stop(); return 1; };   // a setup error
  int rc = ann_wait();
  const double t_guides = since();
  if (rc) { fprintf(stderr, "error: could not load reference annotation %s: %s\n", o.gff.c_str(), br_strerror(rc)); return give_up(); }
  size_t n_tx = br_annotation_num_transcripts(ann), n_refs = br_annotation_num_refs(ann);
  const char *const *refnames = br_annotation_refnames(ann);
  Fasta fa;
  std::vector<br_fasta_seq> fseqs;
  if (o.cfg.use_fasta) {
    if (!load_fasta(o.fasta.c_str(), fa)) { fprintf(stderr, "error: could not open genome %s\n", o.fasta.c_str()); return give_up(); }
    for (size_t i = 0; i < fa.names.size(); i++) fseqs.push_back({fa.names[i].c_str(), fa.seqs[i].data(), fa.seqs[i].size()});
  }
  if (!o.quiet) {
    printf("[bramble] reference annotation loaded! %zu unique transcripts were found (%.1fs)\n", n_tx, since());
    if (o.cfg.lr) printf("[bramble] using long-read mode (--lr)\n");
    else if (o.cfg.lr_hq) printf("[bramble] using long-read mode (--lr-hq)\n");
    else printf("[bramble] using short-read mode (have long reads? try running with --lr or --lr-hq)\n");
    printf("[bramble] building g2t index%s\n", o.devices.size() > 1 ? " (one replica per device)" : "");
  }

  const size_t n_workers = o.devices.size();
  for (size_t w = 0; w < n_workers; w++) { workers.emplace_back(new Worker()); workers[w]->id = (int)w; workers[w]->device = o.devices[w]; }
  {
    std::vector<std::thread> builders;
    for (auto &wp : workers) builders.emplace_back([&, w = wp.get()]() {
      w->build_rc = br_index_build(br_annotation_transcripts(ann), n_tx, refnames, n_refs, fseqs.empty() ? nullptr : fseqs.data(), fseqs.size(), w->device, &w->ix);
      if (!w->build_rc) w->build_rc = br_ctx_new(w->ix, &w->ctx);
    });
    for (auto &t : builders) t.join();
  }
  for (auto &w : workers)
    if (w->build_rc) { fprintf(stderr, "error: index build failed on device %d: %s\n", w->device, br_strerror(w->build_rc)); return give_up(); }
  const double t_index = since() - t_guides;
  fa = Fasta();  // the indexes hold the exon sequences now
  const br_index *ix0 = workers[0]->ix;
  // input refID -> annotation reference index; names the annotation lacks get ids past its table
  // (gseqs.addName, src/bramble.cpp:384: a new id with no interval tree behind it)
  const BamHeader &hdr = in->hdr;
  std::unordered_map<std::string, int32_t> ref_of;
  for (size_t r = 0; r < n_refs; r++) ref_of.emplace(refnames[r], (int32_t)r);
  std::vector<int32_t> ref_map(hdr.ref_names.size());
  int32_t extra = (int32_t)n_refs;
  for (size_t r = 0; r < hdr.ref_names.size(); r++) { auto it = ref_of.find(hdr.ref_names[r]); ref_map[r] = it != ref_of.end() ? it->second : extra++; }
  // every transcript's name and length, once: a line of a file, an RNAME, a BAI bin belong to the @SQ list, the transcripts of
  // length > 0 in index order (what make_bam_header writes)
  RunEnv env{o, o.devices[0], {}, hdr};
  for (size_t t = 0, nt = br_index_num_transcripts(ix0); t < nt; t++) {
    env.tx.name.push_back(br_index_transcript_name(ix0, (uint32_t)t));
    env.tx.len.push_back(br_index_transcript_len(ix0, (uint32_t)t));
  }
  number_sq(env.tx);
  if (!o.quant_genes.empty() || (!o.cells.empty() && o.cells_features == 0)) {   // the genes beside the names: the annotation's, or the map's
    const char *const *gene_ids = br_annotation_gene_ids(ann);
    if (env.tx.name.size() != n_tx) { fprintf(stderr, "error: the index does not hold the annotation's transcripts\n"); return give_up(); }
    for (size_t t = 0; t < n_tx; t++) env.tx.gene.push_back(o.quant_gene_map.empty() ? gene_ids[t] : gene_map.find(env.tx.name[t])->second.c_str());
    number_genes(env.tx);
  }
  if (o.sam_out) {   // RNAME / RNEXT
    std::vector<const char *> sq;
    for (size_t t = 0; t < env.tx.len.size(); t++) if (env.tx.len[t] > 0) sq.push_back(env.tx.name[t]);
    for (auto &w : workers) {
      int src = br_ctx_set_sam_refs(w->ctx, sq.data(), (int32_t)sq.size());
      if (src) { fprintf(stderr, "error: reference names on device %d: %s\n", w->device, br_strerror(src)); return give_up(); }
    }
  }
  if (!o.unprojected.empty()) {   // (one device: the records stay in worker 0's context until the consumer draws them)
    const int urc = br_ctx_set_param(workers[0]->ctx, "keep_unprojected", o.unprojected_scope);
    if (urc) { fprintf(stderr, "error: unprojected records on device %d: %s\n", workers[0]->device, br_strerror(urc)); return give_up(); }
  }
  if (!o.quant_bam.empty() || !o.dedup_bam.empty()) env.out_header = make_bam_header(make_header_text(hdr.text, ix0, cl, o.gff, false), ix0);
  if (!open_consumers(env, consumers, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return give_up(); }
  OutFile file(o.out_bam);
  if (!file.wr.open(file.tmp.c_str(), o.threads, o.level, !o.sam_out)) { fprintf(stderr, "error: %s\n", file.wr.error().c_str()); return give_up(); }
  {
    const std::string text = make_header_text(hdr.text, ix0, cl, o.gff, o.sort);
    bool ok;
    if (o.sam_out) ok = file.wr.write_raw((const uint8_t *)text.data(), text.size());   // SAM: the header text as it is
    else { std::vector<uint8_t> h = make_bam_header(text, ix0); ok = file.wr.write(h.data(), h.size()); }
    if (!ok) { fprintf(stderr, "error: %s\n", file.wr.error().c_str()); file.discard(); return give_up(); }
  }
  if (!o.quiet) printf("[bramble] processing alignments :-)\n");
  double t_setup = since();
  Run run{o, *in, out, file.wr, ref_map, workers, consumers};
  run.track_blocks = o.write_index;
  run.go();
  int failed = run.fail.load();
  if (!in->err.empty()) { fprintf(stderr, in->err_at_line ? "error: %s:%s\n" : "error: %s: %s\n", o.in_bam.c_str(), in->err.c_str()); failed = 1; }
  if (!run.writer_err.empty()) { fprintf(stderr, "error: %s: %s\n", o.out_bam.c_str(), run.writer_err.c_str()); failed = 1; }
  if (!failed && out.next != in->next_seq + run.drained_chunks) { fprintf(stderr, "error: %s: output incomplete\n", o.out_bam.c_str()); failed = 1; }
  // the consumers' files take the output's route: temporary names, renamed once everything has succeeded; none is begun after a failure
  for (auto &c : consumers) if (!failed && !c->write_files(file.wr, run.spans)) failed = 1;
  if (!file.finish(!failed)) failed = 1;
  for (auto c = consumers.rbegin(); c != consumers.rend(); ++c) if (!(*c)->settle(failed)) failed = 1;
  if (!o.quiet && !failed) for (auto &c : consumers) c->report();
  double t_done = since();
  uint64_t total_complete = 0, total_unique = 0, dropped = 0, n_bundles = 0;
  double gpu_seconds = 0, t_upload = 0, t_wait_gpu_in = 0;
  for (auto &w : workers) {
    total_complete += w->total_complete; total_unique += w->total_unique; dropped += w->dropped; n_bundles += w->n_bundles;
    gpu_seconds += w->gpu_seconds; t_upload += w->t_upload; t_wait_gpu_in += w->t_wait_in;
  }
  // the command line's process ends here: handing tens of gigabytes of device and pinned memory back piece by piece is
  // 0.12-0.16 s that the process exit does for nothing (bramble-cli keeps its index in a ManuallyDrop for the same reason,
  // bramble-cli/src/main.rs:56-60).  That is the `bramble` binary (br_cli_exit_at_end); a host that calls br_cli_main as a
  // function gets everything released, and so does a run under BRAMBLE_AMD_CLI_CLEANUP=1
  if (!g_exit_at_end.load() || getenv("BRAMBLE_AMD_CLI_CLEANUP")) { free_all(); in->stop(); }
  double t_freed = since();
  if (!o.quiet) {  // src/bramble.cpp:727-736
    printf("\n[bramble] final report:\n");
    printf("# input alignments:   %llu\n", (unsigned long long)in->totals.reads.load());
    printf("# unmapped reads:     %llu\n", (unsigned long long)in->totals.unmapped.load());
    printf("# dropped alignments: %llu\n", (unsigned long long)dropped);
    printf("# total alignments:   %llu\n", (unsigned long long)total_complete);
    printf("# unique alignments:  %llu\n\n", (unsigned long long)total_unique);
    printf("[bramble] %llu bundles on %zu device worker(s), %.2fs on the device path (upload + kernels + download, summed), %.2fs wall (setup %.2fs: guides %.2fs + index %.2fs, codec %s)\n",
           (unsigned long long)n_bundles, n_workers, gpu_seconds, since(), t_setup, t_guides, t_index, brio::codec_name());
    printf("[bramble] release of device / pinned memory: %.2fs\n", t_freed - t_done);
    printf("[bramble] stage busy time: inflate %.2fs, split %.2fs, bundle copy %.2fs, upload %.2fs, device %.2fs (waited for input %.2fs), deflate+write %.2fs\n",
           in->t_inflate, in->t_split, in->t_copy, t_upload, gpu_seconds, t_wait_gpu_in, run.t_deflate);
  }
  if (getenv("BRAMBLE_AMD_TIMING")) {   // where the resident memory is: anonymous (record buffers), file, shared (pinned / device-visible)
    if (FILE *f = fopen("/proc/self/status", "r")) {
      char line[256];
      while (fgets(line, sizeof line, f)) if (!strncmp(line, "VmHWM", 5) || !strncmp(line, "VmRSS", 5) || !strncmp(line, "Rss", 3) || !strncmp(line, "AnonHuge", 8)) fprintf(stderr, "[bramble] %s", line);
      fclose(f);
    }
    in->report_timing();
  }
  // the unwinding below this line (record buffers, worker contexts, reader and writer pools) was 0.5 s of a 1.9 s run
  if (g_exit_at_end.load() && !getenv("BRAMBLE_AMD_CLI_CLEANUP")) {   // (tools that write their results from exit handlers -- a profiler -- ask for the clean return)
    if (getenv("BRAMBLE_AMD_TIMING")) { struct timespec t; clock_gettime(CLOCK_REALTIME, &t); fprintf(stderr, "[bramble] leaving at %.3f\n", (double)t.tv_sec + 1e-9 * (double)t.tv_nsec); }
    fflush(stdout); fflush(stderr); _exit(failed);
  }
  return failed;
}

// ---- BGZF utilities (host only) -------------------------------------------------------------------
extern "C" int br_bgzf_write_file(const char *path, const uint8_t *data, uint64_t n, int threads, int level) {
  if (!path || (!data && n)) return BR_ERR_INVALID_ARG;
  BgzfWriter wr;
  if (!wr.open(path, threads, level)) return BR_ERR_INVALID_ARG;
  if (n && !wr.write(data, (size_t)n)) return BR_ERR_INVALID_ARG;
  return wr.close() ? BR_OK : BR_ERR_INVALID_ARG;
}

extern "C" int br_bgzf_read_file(const char *path, int threads, uint8_t **out, uint64_t *n) {
  if (!path || !out || !n) return BR_ERR_INVALID_ARG;
  *out = nullptr; *n = 0;
  BgzfReader rd;
  if (!rd.open(path, threads)) return BR_ERR_INVALID_ARG;
  brio::ByteBuf buf;
  for (;;) { int64_t got = rd.read(buf, 64u << 20); if (got < 0) return BR_ERR_INVALID_ARG; if (got == 0) break; }
  uint8_t *p = (uint8_t *)malloc(buf.size() ? buf.size() : 1);
  if (!p) return BR_ERR_CAPACITY;
  memcpy(p, buf.data(), buf.size());
  *out = p; *n = buf.size();
  return BR_OK;
}

extern "C" void br_free_buffer(uint8_t *p) { free(p); }
extern "C" const char *br_bgzf_codec(void) { return brio::codec_name(); }
