// br_quant: the read names of a whole run reduced to equivalence classes in one device's HBM, and the EM over them
// (quant_kernels.hip).
//
//   add      per read name (a read-name group of the projected batch) the ascending list of the distinct transcript ids of its rows,
//            written into the label arena at the slot of the name's first row -- the rows' offsets are the placement, a product
//            of the projection's own scan -- with its length and a 64-bit hash of (labels, k)
//   finish   the names with labels, compacted -> stable LSD radix sort of (hash & mask, name index) with the collator's passes ->
//            class heads by comparing the label lists of neighbours; a run of equal hashes that holds different lists is ordered
//            on the device by (k, labels, name index) and the heads are found again, so the result is exact at any hash_bits ->
//            counts from the scanned heads -> a second sort of the classes by their first name index -> label_off (a scan), labels
//            -> radix sort of (transcript, label entry): the transposed table, per transcript its classes in ascending order ->
//            classes of more than 64 labels and transcripts in more than 64 classes listed (a wave each in the EM) -> unique /
//            ambiguous names per transcript
//   lengths  ("eff_len") every add also counts, per read name of one label, the length of its first fragment (a pair's two adjacent
//            rows on one transcript: positions and the reference bases of the two rewritten CIGARs) into the add's own histogram,
//            which joins the run's once the add is known to be good; finish scans the histogram into C and S and writes the
//            effective length and w = 1 / eff per transcript, which the EM then takes from the device
//   em       one EM (quant_em_run) over a chunk of W = 2^k replicates that run together, replicate innermost in theta, theta w, q
//            and the counts, so an index is read once for W replicates and a gather is W * 8 contiguous bytes; a replicate's sums
//            do not know W, so its bits are those of the EM run alone on its counts.  Per iteration a class kernel (q_c = n_c /
//            sum over its labels of theta_t w_t) and a transcript kernel (theta'_t = theta_t w_t * sum of q_c over the
//            transcript's classes, gathered through the transposed table); every 16th iteration and the last the transcript
//            kernel also leaves every replicate's largest relative change in a word of its own.  The host reads the W words and
//            clears the bit of a replicate that stops: its theta is copied through from then on.  The EM ends when all have
//            stopped.  br_quant_em is the chunk of one replicate on the observed counts, with kernel instantiations in which
//            W = 1 is a compile-time fact, in buffers the object keeps
//   vb       ("vb") the class and transcript kernels as they are -- alpha in theta's place; the x they leave is replaced -- then three
//            launches that make x from the new alpha: a partial of alpha + p per 256 transcripts, the partials summed in a fixed
//            order by one block a replicate, which also takes psi(S), and a lane per (transcript, replicate) for
//            exp(psi(alpha + p) - psi(S)) w
//   bootstrap B replicates in chunks of W (16 by default): a chunk's class counts are resampled when it starts (a lane a draw:
//            Philox4x32-10 by (draw, replicate), a binary search in the scanned counts, an integer atomicAdd), the EM runs over
//            the chunk in buffers of the call, and its theta go to the B x T result, which a last kernel reduces to mean and
//            variance per transcript
//   genes    (br_quant_genes, after finish) a lane per label entry makes (class << 32) | gene of the label; the radix driver sorts
//            the L keys, the heads of equal keys are the distinct (class, gene) entries and a scan places them in a gene-label
//            arena, a class's gene list where its labels were; a hash of every list (a lane, or a wave above 64 genes), then
//            the routine that made the transcript classes (quant_classes), and the labels with unique / ambiguous names per
//            gene by integer atomics.  The transcripts by gene come from a counting sort on the host; a lane per gene sums
//            theta / tpm / lengths over them in ascending order, a lane per (replicate, gene) the B x T result into B x G,
//            which the transcripts' summary kernel reduces
//   names    ("keep_names") quant_classes, while its sorted items and scanned heads are still there, also scatters every item's final
//            class index to name_cls: sorted item -> head rank -> rank after the sort by first name -> name_cls[item]; after the
//            EM a lane per class makes the posteriors of its label entries (k_q_post), its sum running over the labels one by one
//   One routine, quant_classes, makes the classes of both levels from items: an item owns a list, has a first name and stands for
//   a number of names (its weight).  For finish an item is a read name with labels -- its first name is itself, its weight 1, and
//   neither table exists; for the genes it is a transcript class with its gene list, the class's first name and the class's count
//   (one more scan, of the sorted items' weights, gives a gene class its count).  From the unsorted (hash, item) pairs on, the
//   sort, the heads with the collision repair, the counts, the sort by first name and label_off are the same code
//
// Device memory (N names, of them M with labels; R rows added; C classes; L labels over all classes; T transcripts):
//   while adding   4 R (the arena: a slot per row) + 20 N (offset, k, hash) + 4 bytes a name of the largest add (the list of its
//                  names of many rows); while the tables grow, the old one beside the new
//   finish         adds 8 N (the compaction's scan, freed before the sort), then 32 M (keys 2 x 8, indices 2 x 4, heads 8; 4 M more
//                  for the run marks when hashes collide) and the radix histograms (2 KiB a tile of 2048), 32 C (class starts 8, the
//                  second sort 2 x 8 + 2 x 4), then -- the arena, the name tables and the sort's buffers freed -- 32 L (class of an
//                  entry 4, (transcript, entry) keys 2 x 8 and indices 2 x 4) beside what stays
//   afterwards     24 C (first name, count, label_off) + 8 L (labels, the transposed table's classes) + 24 T (the table's offsets,
//                  unique, ambiguous) + 4 bytes per listed class / transcript
//   em             adds 40 T (theta and theta w twice, w) + 8 C (q)
//   "keep_names"   holds 4 (N + 1) from finish on (name_cls: per name its class), and 4 (C + 1) more while the classes are made
//                  (the inverse of the second sort)
//   posteriors     (br_quant_posteriors, br_coverage_finish_em) hold 8 (L + 1) from the first call after an EM on; a later EM drops them
//   "eff_len"      adds 16 (fld_max + 1 + 3) from the first add on (the histogram and its three counters, the run's and the add's
//                  own), 8 per row and 4 per pool word of a host add's CIGAR copies while it runs, 16 (fld_max + 1) for the
//                  prefixes during finish, and 8 T for eff from finish on (w, 8 T of the EM's 40, is held from finish on as well)
//   bootstrap      ("bootstraps" = B) holds 8 B T (the result, replicate-major) + 8 C (cum) + 8 T (w, if the EM has not made it);
//                  while it runs, for a chunk of W replicates, 32 W T (theta and theta w twice) + 12 W C (q 8, the resampled
//                  counts 4) + 512 bytes (the relative changes); br_quant_boot_counts 4 C a replicate of up to 16 at a time, the
//                  summary 16 T
//   "vb"           holds 8 T (p per transcript) from the first EM or bootstrap on, 8 bytes per 256 transcripts + 512 for the point EM's
//                  partials of S and psi(S); a chunk of W replicates has W times the partials while it runs
//   genes          (G genes, CG gene classes, LG gene labels, LE distinct (class, gene) entries, LG <= LE <= L) holds 24 CG (first
//                  name, count, label_off) + 4 LG (labels) + 24 G (unique, ambiguous, the offsets of a gene's transcripts) + 4 T
//                  (the transcripts by gene); while it runs 4 T (the map) + 32 L (keys 2 x 8, indices 2 x 4, the scanned heads
//                  8) and the radix histograms, then -- those freed -- 4 LE + 12 C (the arena, a class's offset and length) + 4
//                  bytes per class of more than 64 genes + 40 C (keys 2 x 8, indices 2 x 4, heads 8, the scanned member counts
//                  8; 4 C more for the run marks when hashes collide) + 36 CG (gene class starts 8, the second sort 2 x 8 + 2 x
//                  4, the class whose list it is 4); br_quant_gene_result 8 T (tpm) + 8 T (lengths, if given) + 32 G while it
//                  runs; the gene replicates hold 8 B G from the first br_quant_gene_boot* on, their summary 16 G
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "accum.h"
#include "barcode_sort.h"
#include "collate_kernels.h"
#include "ctx.h"
#include "name_window.h"
#include "quant_kernels.h"
#include "quant_view.h"
#include "scan_kernels.h"

using namespace br;

// The buffers of an EM over W replicates (quant_em_alloc): theta and theta w, each twice, T W doubles; q, C W; "vb": the partials of
// S, W per 256 transcripts, and psi(S)
struct QEmBufs { ColBuf theta[2], x[2], q, vb_part, vb_psi; };

struct br_quant : Accum {
  int64_t n_tx = 0;
  std::vector<int64_t> lens;   // empty: no lengths were given
  int hash_bits = 64, length_norm = 1, eff_len = 0, keep_names = 0;
  int64_t fld_max = 1000;      // (salmon's fragLenDistMax)
  int64_t max_iters = 10000;
  double tolerance = 1e-2;
  int vb = 0, vb_per_nt = 0;   // the variational Bayes EM, and its prior per nucleotide
  double vb_prior = 1e-2;      // (salmon's vbPrior)
  bool finished = false, em_done = false;
  int64_t n = 0;               // names added
  uint64_t rows = 0;           // arena slots in use
  int64_t n_assigned = 0;
  uint32_t n_big_cls = 0, n_big_tx = 0;
  double add_s = 0, finish_s = 0, em_s = 0;
  ColBuf lab, noff, nk, hash, big;                       // add
  // the classes of one level in first-name order (quant_classes): per class its first name, count and label_off; the labels
  struct Classes {
    ColBuf first, cnt, loff, labels;
    int64_t n_cls = 0, n_lab = 0;
    uint64_t collisions = 0;
  } cls;                                                 // the transcript classes, after finish
  ColBuf t_cls, t_off, uniq, ambig, big_cls, big_tx;     // after finish
  ColBuf name_cls;                                       // "keep_names": per name its class, from finish on
  ColBuf post;                                           // the posteriors, per label entry, once they were asked for after the EM
  QEmBufs em;                                            // the point EM's, held: theta[cur] and x[cur] are its result
  ColBuf w, prior;                                       // per transcript; "vb": p, held from the first EM or bootstrap on
  ColBuf fld_stage, fld_total, eff;                      // "eff_len": fld_max + 1 bins + Q_FLD_SIDE counters each (an add's, the run's); per transcript
  size_t fld_words() const { return (size_t)fld_max + 1 + Q_FLD_SIDE; }
  int fld_tables() {                                     // (zeroed once; a commit leaves the add's table zero again)
    if (fld_total.p) return BR_OK;                       // (fld_max is fixed from here on: br_quant_set_param)
    const size_t bytes = fld_words() * 8;
    int rc = alloc(fld_stage, bytes);
    if (!rc) rc = alloc(fld_total, bytes);
    if (!rc && (hipMemsetAsync(fld_stage.p, 0, bytes, st) != hipSuccess || hipMemsetAsync(fld_total.p, 0, bytes, st) != hipSuccess)) rc = BR_ERR_HIP;
    if (rc) { drop(fld_stage); drop(fld_total); }        // both, zeroed, or neither
    return rc;
  }
  int cur = 0;
  ColBuf tmp, small;
  // bootstrap replicates: the parameters, the B x T result (replicate-major) and cum (C + 1), both held from br_quant_bootstrap on
  int64_t bootstraps = 0, boot_chunk = 0;
  uint64_t boot_seed = 0;
  bool boot_done = false;
  uint64_t boot_n = 0;         // cum[C]: the names with labels
  double boot_sample_s = 0, boot_em_s = 0;
  int64_t boot_iters = 0;
  ColBuf boot_res, boot_cum;
  // gene level: the tables br_quant_genes leaves, and the B x G gene replicates once they were asked for
  struct Genes : Classes {                                    // the gene classes, and
    ColBuf uniq, ambig, toff, tx;                             // per gene; the transcripts by gene, ascending inside one
    std::vector<uint32_t> n_tx;                               // transcripts per gene
  } gene;
  bool genes_done = false;
  int64_t n_genes = 0;
  double genes_s = 0;
  ColBuf gene_boot;
};
// words of `small`
enum { QS_BITS = 0, QS_COLL = 2, QS_SPAN = 3, QS_NBIG = 5, QS_MAXTID = 6, QS_BAD = 7, QS_REL = 8, QS_NBIG_CLS = 9, QS_NBIG_TX = 10, QS_WORDS = 16 };

extern "C" void br_quant_free(br_quant *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_quant_new(int device, int64_t n_transcripts, const int64_t *lengths, br_quant **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  if (n_transcripts < 0 || n_transcripts >= (1ll << 32)) return BR_ERR_INVALID_ARG;
  br_quant *c = new br_quant();
  c->n_tx = n_transcripts;
  if (lengths) c->lens.assign(lengths, lengths + n_transcripts);
  const int rc = c->open(device, c->small, QS_WORDS);
  if (rc) { br_quant_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_quant_set_param(br_quant *c, const char *name, int64_t value) {
  if (!c || !name) return BR_ERR_INVALID_ARG;
  // the replicates' parameters: until br_quant_bootstrap has run, after finish as well
  if (!strcmp(name, "bootstraps")) { if (value < 0 || value > 10000 || c->boot_done) return BR_ERR_INVALID_ARG; c->bootstraps = value; return BR_OK; }
  if (!strcmp(name, "boot_seed")) { if (c->boot_done) return BR_ERR_INVALID_ARG; c->boot_seed = (uint64_t)value; return BR_OK; }
  if (!strcmp(name, "boot_chunk")) { if (value < 0 || value > 64 || c->boot_done) return BR_ERR_INVALID_ARG; c->boot_chunk = value; return BR_OK; }
  if (c->finished) return BR_ERR_INVALID_ARG;
  if (!strcmp(name, "hash_bits")) { if (value < 1 || value > 64) return BR_ERR_INVALID_ARG; c->hash_bits = (int)value; return BR_OK; }
  if (!strcmp(name, "length_norm")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->length_norm = (int)value; return BR_OK; }
  // what the adds already counted depends on these two, and the histogram's tables are sized by fld_max when the first add that
  // counts fragments makes them: before the first add only, a refused one included
  const bool fixed = c->n > 0 || c->fld_total.p != nullptr;
  if (!strcmp(name, "eff_len")) { if ((value != 0 && value != 1) || fixed) return BR_ERR_INVALID_ARG; c->eff_len = (int)value; return BR_OK; }
  if (!strcmp(name, "keep_names")) { if ((value != 0 && value != 1) || fixed) return BR_ERR_INVALID_ARG; c->keep_names = (int)value; return BR_OK; }
  if (!strcmp(name, "fld_max")) { if (value < 1 || value > 65535 || fixed) return BR_ERR_INVALID_ARG; c->fld_max = value; return BR_OK; }
  if (!strcmp(name, "max_iters")) { if (value < 1) return BR_ERR_INVALID_ARG; c->max_iters = value; return BR_OK; }
  if (!strcmp(name, "vb")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->vb = (int)value; return BR_OK; }
  if (!strcmp(name, "vb_per_nucleotide")) { if (value != 0 && value != 1) return BR_ERR_INVALID_ARG; c->vb_per_nt = (int)value; return BR_OK; }
  if (!strcmp(name, "tolerance_ppm")) { if (value < 0) return BR_ERR_INVALID_ARG; c->tolerance = (double)value * 1e-6; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}
extern "C" int br_quant_set_tolerance(br_quant *c, double tolerance) {
  if (!c || c->finished || !(tolerance >= 0.0)) return BR_ERR_INVALID_ARG;
  c->tolerance = tolerance;
  return BR_OK;
}

extern "C" int br_quant_set_vb_prior(br_quant *c, double prior) {
  if (!c || c->finished || !(prior >= 0.0) || !(prior <= 1.79769313486231570815e308)) return BR_ERR_INVALID_ARG;
  c->vb_prior = prior;
  return BR_OK;
}

// room for m more names whose rows number `rows`
static int quant_reserve(br_quant *c, int64_t m, uint64_t rows) {
  if ((uint64_t)(c->n + m) >= (1ull << 32)) return BR_ERR_CAPACITY;   // (32-bit radix indices)
  const size_t need = (size_t)(c->rows + rows) + 1;
  if (need * 4 > c->lab.cap) RC(c->alloc(c->lab, std::max(need, (size_t)(c->lab.cap / 4) * 3 / 2) * 4, true));
  const size_t nn = (size_t)(c->n + m) + 1;
  if (nn * 8 > c->noff.cap) {
    const size_t want = std::max(nn, (size_t)(c->noff.cap / 8) * 3 / 2);
    RC(c->alloc(c->noff, want * 8, true)); RC(c->alloc(c->hash, want * 8, true)); RC(c->alloc(c->nk, want * 4, true));
  }
  RC(c->alloc(c->big, (size_t)(m + 1) * 4));   // (the list of the names of many rows: no longer than the names)
  return BR_OK;
}

// the names of one add, their tables on the device (A: a, a_bias and names are set; cigar, pool and n_pool_words as well when the
// fragments are counted)
static int quant_add_names(br_quant *c, QAddArgs A) {
  hipStream_t st = c->st;
  const uint64_t m = A.names.r_last - A.names.r_first;
  RC(quant_reserve(c, A.names.n_groups, m));
  if (A.cigar) RC(c->fld_tables());
  uint64_t *small = c->small.as<uint64_t>();
  HIPCHK(hipMemsetAsync(small + QS_NBIG, 0, 8, st)); HIPCHK(hipMemsetAsync(small + QS_BAD, 0, 8, st));
  A.lab_base = c->rows; A.lab = c->lab.as<uint32_t>();
  A.noff = c->noff.as<uint64_t>() + c->n; A.nk = c->nk.as<uint32_t>() + c->n; A.hash = c->hash.as<uint64_t>() + c->n;
  A.big = c->big.as<uint32_t>(); A.n_big = (uint32_t *)(small + QS_NBIG);
  A.max_tid = (uint32_t *)(small + QS_MAXTID); A.bad = (uint32_t *)(small + QS_BAD);
  launch_q_names(st, A);
  if (A.cigar) {
    A.fld_max = (uint32_t)c->fld_max; A.stage = c->fld_stage.as<unsigned long long>();
    launch_q_frag(st, A);
  }
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, small + QS_BAD, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the caller's rows may be reused now
  if (bad) {   // offsets that descend somewhere, or a CIGAR reference that leaves the pool: nothing was added
    if (A.cigar) HIPCHK(hipMemsetAsync(c->fld_stage.p, 0, c->fld_words() * 8, st));
    return BR_ERR_INVALID_ARG;
  }
  if (A.cigar) launch_q_fld_commit(st, A.stage, c->fld_total.as<unsigned long long>(), (uint32_t)c->fld_words());
  c->rows += m; c->n += A.names.n_groups;
  return BR_OK;
}

// rows: a and row_off; cigar, pool, n_pool_words and n_rows as well when the fragments are counted (cigar != NULL)
static int quant_add(br_quant *c, const br_device_rows &rows, const uint32_t *group_off, int64_t n_groups, int on_device, void *stream) {
  if (n_groups == 0) return BR_OK;
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  uint64_t span[2] = {0, 0};
  const uint64_t n_rows = rows.cigar ? (uint64_t)rows.n_rows : ~0ull;   // without the CIGARs nothing says how many rows there are
  RC(names_span(c, rows.row_off, n_rows, group_off, n_groups, on_device != 0, (hipStream_t)stream, c->small.as<uint64_t>() + QS_SPAN, span));
  RowWindow w;   // host tables: a and, when the fragments are counted, the CIGAR references and the pool
  ColBuf d_ro, d_go;
  DropGuard dropper{c, {&w.a, &w.cigar, &w.pool, &d_ro, &d_go}};
  QAddArgs A{};
  if (on_device) {
    A.a = (const uint4 *)rows.a; A.names = device_names(rows.row_off, group_off, n_groups, span);
    A.cigar = rows.cigar; A.pool = rows.pool; A.n_pool_words = (uint64_t)rows.n_pool_words;
  } else {
    RC(c->upload_rows(rows, span[0], span[1], rows.cigar != nullptr, w));
    RC(upload_names(c, rows.row_off, group_off, n_groups, span, d_ro, d_go, &A.names));
    A.a = w.a.as<uint4>(); A.a_bias = w.bias;
    A.cigar = w.cigar.as<uint64_t>(); A.pool = w.pool.as<uint32_t>(); A.n_pool_words = w.n_pool_words;
  }
  return quant_add_names(c, A);   // (it waits for the stream: the uploads are done when the host arrays go)
}

extern "C" int br_quant_add(br_quant *c, const br_row_a *a, const uint64_t *row_off, const uint32_t *group_off, int64_t n_groups,
                            int on_device, void *stream) {
  if (!c || n_groups < 0 || c->finished || (n_groups && (!row_off || !group_off))) return BR_ERR_INVALID_ARG;
  if (c->eff_len) return BR_ERR_INVALID_ARG;   // the fragments need the CIGARs: br_quant_add_rows
  br_device_rows rows{};
  rows.a = a; rows.row_off = row_off;
  return quant_add(c, rows, group_off, n_groups, on_device, stream);
}

extern "C" int br_quant_add_rows(br_quant *c, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups, int on_device,
                                 void *stream) {
  if (!c || !rows || n_groups < 0 || c->finished || (n_groups && (!rows->row_off || !group_off))) return BR_ERR_INVALID_ARG;
  br_device_rows r{};
  r.a = rows->a; r.row_off = rows->row_off;
  if (c->eff_len) {   // (without it: br_quant_add, and nothing else of the table is looked at)
    if (n_groups && (!rows->cigar || rows->n_rows < 0 || rows->n_pool_words < 0 || (rows->n_pool_words && !rows->pool))) return BR_ERR_INVALID_ARG;
    r.cigar = rows->cigar; r.pool = rows->pool; r.n_rows = rows->n_rows; r.n_pool_words = rows->n_pool_words;
  }
  return quant_add(c, r, group_off, n_groups, on_device, stream);
}

extern "C" int br_quant_add_last(br_quant *c, br_ctx *ctx) {
  if (!c || !ctx || !ctx->ix || ctx->ix->device != c->device) return BR_ERR_INVALID_ARG;
  if (ctx->last_n_groups == 0) return c->finished ? BR_ERR_INVALID_ARG : BR_OK;
  return br_quant_add_rows(c, &ctx->last_rows, ctx->last_group_off, ctx->last_n_groups, 1, ctx->last_stream);
}

// the names with a non-zero flag lose their labels before finish looks at them: to everything finish makes they are names without rows
extern "C" int br_quant_drop_names(br_quant *c, const uint8_t *flags, int64_t n, int on_device, int64_t *n_dropped) {
  if (!c || c->finished || n != c->n || (n && !flags)) return BR_ERR_INVALID_ARG;
  if (n_dropped) *n_dropped = 0;
  if (n == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  uint64_t *small = c->small.as<uint64_t>();
  ColBuf d_flags;
  DropGuard dropper{c, {&d_flags}};
  if (!on_device) {
    RC(c->alloc(d_flags, (size_t)n));
    HIPCHK(hipMemcpyAsync(d_flags.p, flags, (size_t)n, hipMemcpyHostToDevice, st));
    flags = d_flags.as<uint8_t>();
  } else RC(c->after(nullptr));   // after whatever made the flags
  HIPCHK(hipMemsetAsync(small + QS_BAD, 0, 8, st));
  launch_q_drop(st, flags, n, c->nk.as<uint32_t>(), (unsigned long long *)(small + QS_BAD));
  uint64_t dropped = 0;
  HIPCHK(hipMemcpyAsync(&dropped, small + QS_BAD, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_dropped) *n_dropped = (int64_t)dropped;
  return BR_OK;
}

static int quant_tmp(br_quant *c, int64_t n) { return c->alloc(c->tmp, scan_tmp_bytes(n)); }
// the radix sort of (key[0], idx[0]) over the digits in which the keys differ (barcode_sort.h): the sorted pairs are those of [0]
static int quant_sort(br_quant *c, ColBuf key[2], ColBuf idx[2], int64_t n) { return sort_pairs(c, key, idx, n, c->tmp, c->small.as<uint64_t>() + QS_BITS); }

// The classes of n items, for every level of the quantifier.  Item i owns the list lab[off[i] .. off[i] + k[i]); its first name is
// first[i] (NULL: i itself -- the item is a read name) and it stands for weight[i] names (NULL: one).  key[0] / idx[0] hold the n
// unsorted (hash & mask, item) pairs, n > 0.  The sort of (hash, item) is stable, so the items of a class ascend; the heads compare
// the lists of neighbours, and a run of equal hashes that holds different lists is put in order by (k, list, item) and the heads
// found again: exact at any hash_bits.  out gets the classes in first-name order -- first, cnt (the sum of the items' weights),
// loff (scanned, loff[C] = L) -- with n_cls = C, n_lab = L and the collisions; rep != NULL gets per class an item whose list is
// the class's; name_cls != NULL gets, at every item's index, the class the item fell into (the caller has filled it with 0xffffffff:
// what is no item keeps that).  Everything else, key and idx included, is dropped when it returns: the caller makes its label
// tables after that
static int quant_classes(br_quant *c, const uint32_t *lab, const uint64_t *off, const uint32_t *k, const uint64_t *first, const uint64_t *weight,
                         ColBuf key[2], ColBuf idx[2], int64_t n, br_quant::Classes &out, ColBuf *rep, uint32_t *name_cls = nullptr) {
  hipStream_t st = c->st;
  uint64_t *small = c->small.as<uint64_t>();
  ColBuf head, mark, pre, gbeg, key2[2], val2[2], inv;
  DropGuard sort_bufs{c, {&key[0], &key[1], &idx[0], &idx[1], &head, &mark, &pre, &gbeg, &key2[0], &key2[1], &val2[0], &val2[1], &inv}};
  RC(quant_sort(c, key, idx, n));
  // class heads; runs of equal hashes with different lists are put in order and the heads found again
  RC(c->alloc(head, (size_t)(n + 1) * 8));
  auto heads = [&](uint32_t *mk, uint64_t *n_coll) -> int {
    HIPCHK(hipMemsetAsync(small + QS_COLL, 0, 8, st));
    launch_q_heads(st, lab, off, k, key[0].as<uint64_t>(), idx[0].as<uint32_t>(), n, head.as<uint64_t>(), (unsigned long long *)(small + QS_COLL), mk);
    HIPCHK(hipMemcpyAsync(n_coll, small + QS_COLL, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return BR_OK;
  };
  uint64_t n_coll = 0;
  RC(heads(nullptr, &n_coll));
  out.collisions = n_coll;
  if (n_coll) {
    RC(c->alloc(mark, (size_t)n * 4));
    HIPCHK(hipMemsetAsync(mark.p, 0, (size_t)n * 4, st));
    RC(heads(mark.as<uint32_t>(), &n_coll));
    launch_q_resolve(st, lab, off, k, key[0].as<uint64_t>(), idx[0].as<uint32_t>(), n, mark.as<uint32_t>(), key[1].as<uint64_t>(), idx[1].as<uint32_t>());
    std::swap(key[0], key[1]); std::swap(idx[0], idx[1]);
    RC(heads(nullptr, &n_coll));
  }
  RC(quant_tmp(c, n));
  launch_scan(st, head.as<uint64_t>(), n, c->tmp.as<uint64_t>());   // head -> class ids (exclusive), head[n] = C
  uint64_t C = 0;
  HIPCHK(hipMemcpyAsync(&C, head.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (C == 0 || C > (uint64_t)n) return BR_ERR_HIP;
  out.n_cls = (int64_t)C;
  const size_t c1 = (size_t)C + 1;
  RC(c->alloc(gbeg, c1 * 8));
  launch_col_gbeg(st, head.as<uint64_t>(), n, gbeg.as<uint64_t>());
  if (weight) {   // a class's count: the integer sum of its items' weights, from one scan over the items in sorted order
    RC(c->alloc(pre, (size_t)(n + 1) * 8));
    launch_qg_member_cnt(st, idx[0].as<uint32_t>(), weight, n, pre.as<uint64_t>());
    launch_scan(st, pre.as<uint64_t>(), n, c->tmp.as<uint64_t>());
  }
  // the classes by their first name
  RC(c->alloc(key2[0], c1 * 8)); RC(c->alloc(key2[1], c1 * 8)); RC(c->alloc(val2[0], c1 * 4)); RC(c->alloc(val2[1], c1 * 4));
  launch_q_class_key(st, gbeg.as<uint64_t>(), idx[0].as<uint32_t>(), first, (int64_t)C, key2[0].as<uint64_t>(), val2[0].as<uint32_t>());
  RC(quant_sort(c, key2, val2, (int64_t)C));
  RC(c->alloc(out.first, c1 * 8)); RC(c->alloc(out.cnt, c1 * 8)); RC(c->alloc(out.loff, c1 * 8));
  if (rep) RC(c->alloc(*rep, c1 * 4));
  launch_q_class_fill(st, key2[0].as<uint64_t>(), val2[0].as<uint32_t>(), gbeg.as<uint64_t>(), idx[0].as<uint32_t>(), pre.as<uint64_t>(), k, (int64_t)C,
                      out.first.as<uint64_t>(), out.cnt.as<uint64_t>(), out.loff.as<uint64_t>(), rep ? rep->as<uint32_t>() : nullptr);
  if (name_cls) {   // sorted item -> head rank -> rank after the second sort -> name_cls[item], while the sort's tables are still here
    RC(c->alloc(inv, c1 * 4));
    launch_q_name_cls(st, head.as<uint64_t>(), idx[0].as<uint32_t>(), n, val2[0].as<uint32_t>(), (int64_t)C, inv.as<uint32_t>(), name_cls);
  }
  RC(quant_tmp(c, (int64_t)C));
  launch_scan(st, out.loff.as<uint64_t>(), (int64_t)C, c->tmp.as<uint64_t>());
  uint64_t L = 0;
  HIPCHK(hipMemcpyAsync(&L, out.loff.as<uint64_t>() + C, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (L >= (1ull << 32)) return BR_ERR_CAPACITY;   // (32-bit radix indices)
  out.n_lab = (int64_t)L;
  return BR_OK;
}

static int quant_finish(br_quant *c) {
  hipStream_t st = c->st;
  const int64_t N = c->n, T = c->n_tx;
  uint64_t *small = c->small.as<uint64_t>();
  RC(c->alloc(c->t_off, (size_t)(T + 2) * 8)); RC(c->alloc(c->uniq, (size_t)(T + 1) * 8)); RC(c->alloc(c->ambig, (size_t)(T + 1) * 8));
  HIPCHK(hipMemsetAsync(c->t_off.p, 0, (size_t)(T + 2) * 8, st));
  HIPCHK(hipMemsetAsync(c->uniq.p, 0, (size_t)(T + 1) * 8, st)); HIPCHK(hipMemsetAsync(c->ambig.p, 0, (size_t)(T + 1) * 8, st));
  HIPCHK(hipStreamSynchronize(st));
  if (N == 0) return BR_OK;
  if (c->keep_names) {   // every name starts without a class
    RC(c->alloc(c->name_cls, (size_t)(N + 1) * 4));
    HIPCHK(hipMemsetAsync(c->name_cls.p, 0xff, (size_t)(N + 1) * 4, st));
  }
  // the names with labels
  uint64_t M = 0;
  ColBuf key[2], idx[2];
  DropGuard sort_bufs{c, {&key[0], &key[1], &idx[0], &idx[1]}};
  {
    ColBuf pos;
    DropGuard dropper{c, {&pos}};
    RC(c->alloc(pos, (size_t)(N + 1) * 8)); RC(quant_tmp(c, N));
    launch_q_flag(st, c->nk.as<uint32_t>(), N, pos.as<uint64_t>());
    launch_scan(st, pos.as<uint64_t>(), N, c->tmp.as<uint64_t>());
    uint32_t max_tid = 0;
    HIPCHK(hipMemcpyAsync(&M, pos.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&max_tid, small + QS_MAXTID, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->n_assigned = (int64_t)M;
    if (M == 0) return BR_OK;
    if ((int64_t)max_tid >= T) return BR_ERR_INVALID_ARG;   // a transcript id the quantifier has no transcript for
    const size_t m1 = (size_t)M + 1;
    RC(c->alloc(key[0], m1 * 8)); RC(c->alloc(key[1], m1 * 8)); RC(c->alloc(idx[0], m1 * 4)); RC(c->alloc(idx[1], m1 * 4));
    const uint64_t mask = c->hash_bits >= 64 ? ~0ull : (1ull << c->hash_bits) - 1;
    launch_q_compact(st, c->nk.as<uint32_t>(), c->hash.as<uint64_t>(), pos.as<uint64_t>(), N, mask, key[0].as<uint64_t>(), idx[0].as<uint32_t>());
    HIPCHK(hipStreamSynchronize(st));
  }
  // their classes: a name is its own first name and counts once; a class's list is its first name's, so no rep
  const uint32_t *lab = c->lab.as<uint32_t>();
  const uint64_t *noff = c->noff.as<uint64_t>();
  RC(quant_classes(c, lab, noff, c->nk.as<uint32_t>(), nullptr, nullptr, key, idx, (int64_t)M, c->cls, nullptr,
                   c->keep_names ? c->name_cls.as<uint32_t>() : nullptr));
  const int64_t C = c->cls.n_cls, L = c->cls.n_lab;
  // labels and the transposed table
  ColBuf ecls, tkey[2], tidx[2], d_lens;
  DropGuard table_bufs{c, {&ecls, &tkey[0], &tkey[1], &tidx[0], &tidx[1], &d_lens}};
  const size_t l1 = (size_t)L + 1;
  RC(c->alloc(c->cls.labels, l1 * 4)); RC(c->alloc(ecls, l1 * 4)); RC(c->alloc(c->t_cls, l1 * 4));
  RC(c->alloc(tkey[0], l1 * 8)); RC(c->alloc(tkey[1], l1 * 8)); RC(c->alloc(tidx[0], l1 * 4)); RC(c->alloc(tidx[1], l1 * 4));
  const bool check_len = c->length_norm && !c->lens.empty();
  if (c->length_norm && c->lens.empty()) return BR_ERR_INVALID_ARG;   // length normalisation without lengths
  if (check_len) {
    RC(c->alloc(d_lens, (size_t)(T + 1) * 8));
    HIPCHK(hipMemcpyAsync(d_lens.p, c->lens.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemsetAsync(small + QS_BAD, 0, 8, st));
  launch_q_labels(st, c->cls.loff.as<uint64_t>(), c->cls.first.as<uint64_t>(), noff, lab, C, L, check_len ? d_lens.as<int64_t>() : nullptr,
                  c->cls.labels.as<uint32_t>(), ecls.as<uint32_t>(), tkey[0].as<uint64_t>(), tidx[0].as<uint32_t>(), (uint32_t *)(small + QS_BAD));
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, small + QS_BAD, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad) return BR_ERR_INVALID_ARG;   // a transcript of length <= 0 has reads, and lengths normalise
  c->drop(c->lab); c->drop(c->noff); c->drop(c->nk); c->drop(c->hash); c->drop(c->big);   // the names are classes now
  RC(quant_sort(c, tkey, tidx, L));
  launch_q_transpose(st, tkey[0].as<uint64_t>(), tidx[0].as<uint32_t>(), ecls.as<uint32_t>(), L, T, c->t_cls.as<uint32_t>(), c->t_off.as<uint64_t>());
  // the wave-sized items
  const size_t most = (size_t)(L / (Q_WAVE_ITEMS + 1) + 1);
  RC(c->alloc(c->big_cls, most * 4)); RC(c->alloc(c->big_tx, most * 4));
  HIPCHK(hipMemsetAsync(small + QS_NBIG_CLS, 0, 16, st));
  launch_q_bin(st, c->cls.loff.as<uint64_t>(), C, c->big_cls.as<uint32_t>(), (uint32_t *)(small + QS_NBIG_CLS));
  launch_q_bin(st, c->t_off.as<uint64_t>(), T, c->big_tx.as<uint32_t>(), (uint32_t *)(small + QS_NBIG_TX));
  uint64_t nb[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(nb, small + QS_NBIG_CLS, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->n_big_cls = (uint32_t)nb[0]; c->n_big_tx = (uint32_t)nb[1];
  launch_q_counts(st, c->t_cls.as<uint32_t>(), c->t_off.as<uint64_t>(), c->cls.loff.as<uint64_t>(), c->cls.cnt.as<uint64_t>(), T, c->big_tx.as<uint32_t>(),
                  c->n_big_tx, c->uniq.as<uint64_t>(), c->ambig.as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

// "eff_len": the histogram's prefixes, then eff and w per transcript
static int quant_eff(br_quant *c) {
  if (!c->eff_len || c->lens.empty()) return BR_OK;
  hipStream_t st = c->st;
  const int64_t T = c->n_tx;
  const uint32_t n_bins = (uint32_t)c->fld_max + 1;
  ColBuf cs, d_lens;
  DropGuard dropper{c, {&cs, &d_lens}};
  RC(c->fld_tables());
  RC(c->alloc(c->eff, (size_t)(T + 1) * 8)); RC(c->alloc(c->w, (size_t)(T + 1) * 8));
  RC(c->alloc(cs, (size_t)n_bins * 16)); RC(c->alloc(d_lens, (size_t)(T + 1) * 8));
  if (T) HIPCHK(hipMemcpyAsync(d_lens.p, c->lens.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
  launch_q_fld_prefix(st, c->fld_total.as<unsigned long long>(), n_bins, cs.as<uint64_t>());
  launch_q_efflen(st, d_lens.as<int64_t>(), T, cs.as<uint64_t>(), n_bins, c->eff.as<double>(), c->w.as<double>());
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

extern "C" int br_quant_finish(br_quant *c, int64_t *n_names, int64_t *n_classes) {
  if (!c || c->finished) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  RC(quant_finish(c));
  RC(quant_eff(c));
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_names) *n_names = c->n;
  if (n_classes) *n_classes = c->cls.n_cls;
  return BR_OK;
}

// one level's classes to the host
static int quant_copy_classes(br_quant *c, const br_quant::Classes &k, uint64_t *label_off, uint32_t *labels, uint64_t *counts,
                              uint64_t *first_name) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const size_t C = (size_t)k.n_cls, L = (size_t)k.n_lab;
  if (label_off) { if (C) HIPCHK(hipMemcpyAsync(label_off, k.loff.p, (C + 1) * 8, hipMemcpyDeviceToHost, st)); else label_off[0] = 0; }
  if (labels && L) HIPCHK(hipMemcpyAsync(labels, k.labels.p, L * 4, hipMemcpyDeviceToHost, st));
  if (counts && C) HIPCHK(hipMemcpyAsync(counts, k.cnt.p, C * 8, hipMemcpyDeviceToHost, st));
  if (first_name && C) HIPCHK(hipMemcpyAsync(first_name, k.first.p, C * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}
extern "C" int br_quant_classes(br_quant *c, uint64_t *label_off, uint32_t *labels, uint64_t *counts, uint64_t *first_name) {
  return c && c->finished ? quant_copy_classes(c, c->cls, label_off, labels, counts, first_name) : BR_ERR_INVALID_ARG;
}

extern "C" int br_quant_name_classes(br_quant *c, int64_t first, int64_t n, uint32_t *cls) {
  if (!c || !c->finished || !c->keep_names || first < 0 || n < 0 || first > c->n || n > c->n - first) return BR_ERR_INVALID_ARG;
  if (!n || !cls) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(cls, c->name_cls.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_quant_fld(br_quant *c, uint64_t *hist, uint64_t *n_obs, uint64_t *n_no_fragment, uint64_t *n_out_of_range) {
  if (!c) return BR_ERR_INVALID_ARG;
  const size_t n_bins = (size_t)c->fld_max + 1;
  uint64_t side[Q_FLD_SIDE] = {0, 0, 0};
  if (hist) memset(hist, 0, n_bins * 8);
  if (c->fld_total.p) {   // (no table yet: nothing was counted)
    HIPCHK(hipSetDevice(c->device));
    if (hist) HIPCHK(hipMemcpyAsync(hist, c->fld_total.p, n_bins * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(side, c->fld_total.as<uint64_t>() + n_bins, sizeof(side), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  if (n_obs) *n_obs = side[0];
  if (n_no_fragment) *n_no_fragment = side[1];
  if (n_out_of_range) *n_out_of_range = side[2];
  return BR_OK;
}

extern "C" int br_quant_eff_lengths(br_quant *c, double *eff) {
  if (!c || !eff || !c->finished || !c->eff_len || c->lens.empty()) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  if (c->n_tx) HIPCHK(hipMemcpyAsync(eff, c->eff.p, (size_t)c->n_tx * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

// w per transcript on the device: 1 / length where lengths normalise, else 1 (with "eff_len" it is 1 / eff, there since finish: k_q_efflen)
static int quant_put_w(br_quant *c) {
  const size_t T = (size_t)c->n_tx;
  RC(c->alloc(c->w, (T + 1) * 8));
  if (c->eff_len) return BR_OK;
  std::vector<double> w(T, 1.0);
  if (c->length_norm) for (size_t t = 0; t < T; t++) w[t] = c->lens[t] > 0 ? 1.0 / (double)c->lens[t] : 0.0;   // (length <= 0: no reads, finish saw to it)
  if (T) HIPCHK(hipMemcpyAsync(c->w.p, w.data(), T * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));   // (w goes)
  return BR_OK;
}
// "vb": p per transcript on the device -- the prior, or per nucleotide the prior times eff (with "eff_len") or the length, 0 where
// the length is <= 0 (quant_em_ready: with lengths)
static int quant_put_prior(br_quant *c) {
  const size_t T = (size_t)c->n_tx;
  RC(c->alloc(c->prior, (T + 1) * 8));
  std::vector<double> p(T, c->vb_prior);
  if (c->vb_per_nt) {
    std::vector<double> eff;
    if (c->eff_len && T) {
      eff.resize(T);
      HIPCHK(hipMemcpyAsync(eff.data(), c->eff.p, T * 8, hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipStreamSynchronize(c->st));
    }
    for (size_t t = 0; t < T; t++) p[t] = c->lens[t] > 0 ? c->vb_prior * (eff.empty() ? (double)c->lens[t] : eff[t]) : 0.0;
  }
  if (T) HIPCHK(hipMemcpyAsync(c->prior.p, p.data(), T * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));   // (p goes)
  return BR_OK;
}
// theta w of the last EM on the host, what the TPM is made of: the device's x, or after a variational run -- whose x is not
// theta w -- the product made here (one rounding, as the device's)
static int quant_host_x(br_quant *c, std::vector<double> &x) {
  const size_t T = (size_t)c->n_tx;
  x.resize(T);
  if (!T) return BR_OK;
  if (!c->vb) {
    HIPCHK(hipMemcpyAsync(x.data(), c->em.x[c->cur].p, T * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return BR_OK;
  }
  std::vector<double> w(T);
  HIPCHK(hipMemcpyAsync(x.data(), c->em.theta[c->cur].p, T * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(w.data(), c->w.p, T * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (size_t t = 0; t < T; t++) x[t] = x[t] * w[t];   // (built without contraction)
  return BR_OK;
}
// what br_quant_em and br_quant_bootstrap both need: effective lengths are a length normalisation, and "vb"'s prior per nucleotide
// needs lengths
static bool quant_em_ready(const br_quant *c) {
  if (!c || !c->finished) return false;
  return !(c->eff_len && (!c->length_norm || c->lens.empty())) && !(c->vb && c->vb_per_nt && c->lens.empty());
}
// w, "vb"'s p and the buffers of an EM over W replicates
static int quant_em_alloc(br_quant *c, QEmBufs &b, size_t W) {
  const size_t T = (size_t)c->n_tx, C = (size_t)c->cls.n_cls;
  RC(quant_put_w(c));
  for (int k = 0; k < 2; k++) { RC(c->alloc(b.theta[k], (T * W + 1) * 8)); RC(c->alloc(b.x[k], (T * W + 1) * 8)); }
  RC(c->alloc(b.q, (C * W + 1) * 8));
  if (c->vb) { RC(quant_put_prior(c)); RC(c->alloc(b.vb_part, ((T + 255) / 256 * W + 1) * 8)); RC(c->alloc(b.vb_psi, 64 * 8)); }
  return BR_OK;
}
// where an EM ended: the buffer that holds theta and x, and per replicate the iteration it stopped at and the relative change read there
struct QEmEnd { int cur = 0; int32_t iters[64] = {}; double rel[64] = {}; };
// One EM from theta = 1 to its end over b, as a chunk of 1 << lw replicates of which the first n_rep run: on the resampled counts
// boot_cnt, or -- NULL, with lw = 0 and n_rep = 1 -- the point EM on the observed ones.  rel: a word per replicate of the chunk.
// Every 16th iteration and the last are looks: the transcript kernel leaves every replicate's largest relative change, the host
// reads them and a replicate that is below the tolerance, or at the last iteration, stops -- frozen at this iteration's theta
static int quant_em_run(br_quant *c, QEmBufs &b, const uint32_t *boot_cnt, int lw, int n_rep, unsigned long long *rel, QEmEnd *end) {
  hipStream_t st = c->st;
  const int64_t T = c->n_tx;
  const size_t W = (size_t)1 << lw;
  QEmArgs A{};
  A.n_cls = c->cls.n_cls; A.n_tx = T;
  A.label_off = c->cls.loff.as<uint64_t>(); A.labels = c->cls.labels.as<uint32_t>(); A.cnt = c->cls.cnt.as<uint64_t>();
  A.t_off = c->t_off.as<uint64_t>(); A.t_cls = c->t_cls.as<uint32_t>();
  A.big_cls = c->big_cls.as<uint32_t>(); A.n_big_cls = c->n_big_cls; A.big_tx = c->big_tx.as<uint32_t>(); A.n_big_tx = c->n_big_tx;
  A.w = c->w.as<double>(); A.q = b.q.as<double>();
  A.boot_cnt = boot_cnt; A.lw = lw;
  A.active = n_rep >= 64 ? ~0ull : (1ull << n_rep) - 1ull;
  // "vb": x from alpha, after the transcript kernel and for alpha = 1 at the start (three launches more an iteration)
  auto vb_x = [&](int k) {
    if (c->vb) launch_q_vb_x(st, b.theta[k].as<double>(), c->prior.as<double>(), A.w, T, lw, A.active, b.vb_part.as<double>(), b.vb_psi.as<double>(), b.x[k].as<double>());
  };
  launch_q_em_init(st, A.w, T, lw, b.theta[0].as<double>(), b.x[0].as<double>());
  vb_x(0);
  uint64_t bits[64];
  int cur = 0;
  int64_t it = 0;
  while (A.active && it < c->max_iters) {
    it++;
    const bool look = it % 16 == 0 || it == c->max_iters;
    if (look) HIPCHK(hipMemsetAsync(rel, 0, W * 8, st));
    launch_q_em_classes(st, A, b.x[cur].as<double>());
    launch_q_em_tx(st, A, b.theta[cur].as<double>(), b.x[cur].as<double>(), b.theta[cur ^ 1].as<double>(), b.x[cur ^ 1].as<double>(), look ? rel : nullptr);
    cur ^= 1;
    vb_x(cur);
    if (!look) continue;
    HIPCHK(hipMemcpyAsync(bits, rel, W * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int j = 0; j < n_rep; j++) {
      if (!((A.active >> j) & 1ull)) continue;
      double r;
      memcpy(&r, &bits[j], 8);
      if (r < c->tolerance || it == c->max_iters) { A.active &= ~(1ull << j); end->iters[j] = (int32_t)it; end->rel[j] = r; }
    }
  }
  end->cur = cur;
  return BR_OK;
}

extern "C" int br_quant_em(br_quant *c, int32_t *n_iters, double *rel_change) {
  if (!quant_em_ready(c)) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->st));
  c->drop(c->post);   // (the posteriors of an earlier EM)
  RC(quant_em_alloc(c, c->em, 1));
  QEmEnd end;
  RC(quant_em_run(c, c->em, nullptr, 0, 1, (unsigned long long *)(c->small.as<uint64_t>() + QS_REL), &end));
  c->cur = end.cur; c->em_done = true;
  c->em_s = timer.seconds();
  if (n_iters) *n_iters = end.iters[0];
  if (rel_change) *rel_change = end.rel[0];
  return BR_OK;
}

// the posteriors on the device, made once per EM: 8 bytes a label
static int quant_post(br_quant *c) {
  if (c->post.p) return BR_OK;
  RC(c->alloc(c->post, (size_t)(c->cls.n_lab + 1) * 8));
  launch_q_post(c->st, c->cls.loff.as<uint64_t>(), c->cls.labels.as<uint32_t>(), c->cls.n_cls, c->vb ? c->em.x[c->cur].as<double>() : c->em.theta[c->cur].as<double>(),
                c->vb ? nullptr : c->w.as<double>(), c->post.as<double>());   // ("vb": x itself)
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}
extern "C" int br_quant_posteriors(br_quant *c, double *post) {
  if (!c || !c->finished || !c->em_done) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  RC(quant_post(c));
  if (post && c->cls.n_lab) {
    HIPCHK(hipMemcpyAsync(post, c->post.p, (size_t)c->cls.n_lab * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  return BR_OK;
}
// what br_coverage_finish_em reads (quant_view.h); the posteriors are made if they are not there yet
int br::quant_view(br_quant *c, QuantView *v) {
  if (!c || !v || !c->finished || !c->em_done || !c->keep_names) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  RC(quant_post(c));
  v->device = c->device; v->n_names = c->n; v->n_cls = c->cls.n_cls; v->n_lab = c->cls.n_lab;
  v->name_cls = c->name_cls.as<uint32_t>(); v->label_off = c->cls.loff.as<uint64_t>(); v->labels = c->cls.labels.as<uint32_t>();
  v->post = c->post.as<double>();
  return BR_OK;
}

int br::quant_class_view(br_quant *c, QuantClassView *v) {
  if (!c || !v || !c->finished || !c->keep_names) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->st));
  v->device = c->device; v->n_names = c->n; v->n_tx = c->n_tx; v->n_cls = c->cls.n_cls; v->n_lab = c->cls.n_lab;
  v->name_cls = c->name_cls.as<uint32_t>(); v->label_off = c->cls.loff.as<uint64_t>(); v->labels = c->cls.labels.as<uint32_t>();
  return BR_OK;
}

// ---- bootstrap replicates (the definitions: bramble_amd.h, br_quant) ---------------------------------------------------------------
// cum: the exclusive prefix sums of the classes' counts, cum[C] = the names with labels
static int quant_boot_cum(br_quant *c) {
  if (c->boot_cum.p) return BR_OK;
  hipStream_t st = c->st;
  const int64_t C = c->cls.n_cls;
  RC(c->alloc(c->boot_cum, (size_t)(C + 1) * 8));
  c->boot_n = 0;
  if (C == 0) return BR_OK;
  RC(quant_tmp(c, C));
  HIPCHK(hipMemcpyAsync(c->boot_cum.p, c->cls.cnt.p, (size_t)C * 8, hipMemcpyDeviceToDevice, st));
  launch_scan(st, c->boot_cum.as<uint64_t>(), C, c->tmp.as<uint64_t>());
  HIPCHK(hipMemcpyAsync(&c->boot_n, c->boot_cum.as<uint64_t>() + C, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}

extern "C" int br_quant_bootstrap(br_quant *c, int32_t *n_iters) {
  if (!quant_em_ready(c) || c->bootstraps == 0) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const int64_t T = c->n_tx, C = c->cls.n_cls, B = c->bootstraps;
  // replicates a chunk, and the power of two that holds them: the layout's W
  const int per = (int)std::min<int64_t>(c->boot_chunk ? c->boot_chunk : (int64_t)Q_BOOT_CHUNK, B);
  int lw = 0;
  while ((1 << lw) < per) lw++;
  const size_t W = (size_t)1 << lw;
  c->boot_sample_s = c->boot_em_s = 0; c->boot_iters = 0;
  RC(quant_boot_cum(c));
  RC(c->alloc(c->boot_res, ((size_t)B * (size_t)T + 1) * 8));
  QEmBufs b;
  ColBuf cnt, d_rel;
  DropGuard chunk_bufs{c, {&b.theta[0], &b.theta[1], &b.x[0], &b.x[1], &b.q, &b.vb_part, &b.vb_psi, &cnt, &d_rel}};
  RC(quant_em_alloc(c, b, W));
  RC(c->alloc(cnt, ((size_t)C * W + 1) * 4)); RC(c->alloc(d_rel, 64 * 8));
  for (int64_t b0 = 0; b0 < B; b0 += per) {
    const int n_rep = (int)std::min<int64_t>(per, B - b0);
    {
      ScopeTimer timer(&c->boot_sample_s);
      HIPCHK(hipMemsetAsync(cnt.p, 0, ((size_t)C * W + 1) * 4, st));
      launch_q_boot_sample(st, c->boot_cum.as<uint64_t>(), C, c->boot_n, c->boot_seed, (uint32_t)b0, (uint32_t)n_rep, cnt.as<uint32_t>(), (int64_t)W, 1);
      HIPCHK(hipStreamSynchronize(st));
    }
    ScopeTimer timer(&c->boot_em_s);
    QEmEnd end;
    RC(quant_em_run(c, b, cnt.as<uint32_t>(), lw, n_rep, d_rel.as<unsigned long long>(), &end));
    for (int j = 0; j < n_rep; j++) {
      c->boot_iters += end.iters[j];
      if (n_iters) n_iters[b0 + j] = end.iters[j];
    }
    launch_q_boot_store(st, b.theta[end.cur].as<double>(), T, lw, n_rep, c->boot_res.as<double>() + (size_t)b0 * (size_t)T);
    HIPCHK(hipStreamSynchronize(st));
  }
  c->boot_done = true;   // the result is there, and the parameters are fixed from here on
  return BR_OK;
}

extern "C" int br_quant_boot_counts(br_quant *c, int32_t first, int32_t count, uint32_t *counts) {
  if (!c || !c->finished || c->bootstraps == 0 || first < 0 || count < 0 || (int64_t)first + count > c->bootstraps || (count && !counts)) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const int64_t C = c->cls.n_cls;
  RC(quant_boot_cum(c));
  if (C == 0 || count == 0) return BR_OK;
  const int32_t piece = std::min<int32_t>(count, Q_BOOT_CHUNK);
  ColBuf rows;
  DropGuard dropper{c, {&rows}};
  RC(c->alloc(rows, (size_t)piece * (size_t)C * 4));
  for (int32_t k = 0; k < count; k += piece) {
    const int32_t n = std::min<int32_t>(piece, count - k);
    HIPCHK(hipMemsetAsync(rows.p, 0, (size_t)n * (size_t)C * 4, st));
    launch_q_boot_sample(st, c->boot_cum.as<uint64_t>(), C, c->boot_n, c->boot_seed, (uint32_t)(first + k), (uint32_t)n, rows.as<uint32_t>(), 1, C);
    HIPCHK(hipMemcpyAsync(counts + (size_t)k * (size_t)C, rows.p, (size_t)n * (size_t)C * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return BR_OK;
}

extern "C" int br_quant_boot_theta(br_quant *c, int32_t first, int32_t count, double *theta) {
  if (!c || !c->boot_done || !c->boot_res.p || first < 0 || count < 0 || (int64_t)first + count > c->bootstraps || (count && !theta)) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  const size_t T = (size_t)c->n_tx;
  if (T && count) HIPCHK(hipMemcpyAsync(theta, c->boot_res.as<double>() + (size_t)first * T, (size_t)count * T * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

// mean and variance over the replicates of the bootstraps x n result res, per column
static int quant_summary(br_quant *c, const ColBuf &res, size_t n, double *mean, double *var) {
  hipStream_t st = c->st;
  ColBuf mv;   // mean, then var
  DropGuard dropper{c, {&mv}};
  RC(c->alloc(mv, (2 * n + 1) * 8));
  launch_q_boot_summary(st, res.as<double>(), (int64_t)n, (int32_t)c->bootstraps, mv.as<double>(), mv.as<double>() + n);
  if (mean && n) HIPCHK(hipMemcpyAsync(mean, mv.p, n * 8, hipMemcpyDeviceToHost, st));
  if (var && n) HIPCHK(hipMemcpyAsync(var, mv.as<double>() + n, n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BR_OK;
}
extern "C" int br_quant_boot_summary(br_quant *c, double *mean, double *var) {
  if (!c || !c->boot_done || !c->boot_res.p) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  return quant_summary(c, c->boot_res, (size_t)c->n_tx, mean, var);
}

extern "C" int br_quant_boot_stats(const br_quant *c, double *sample_seconds, double *em_seconds, int64_t *iterations_total) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (sample_seconds) *sample_seconds = c->boot_sample_s;
  if (em_seconds) *em_seconds = c->boot_em_s;
  if (iterations_total) *iterations_total = c->boot_iters;
  return BR_OK;
}

// tpm from x = theta w, which the stream has brought to the host: one pass over T numbers, in transcript order
static void quant_tpm(const std::vector<double> &x, double *tpm) {
  const size_t T = x.size();
  double sum = 0.0;
  for (size_t t = 0; t < T; t++) sum += x[t];
  for (size_t t = 0; t < T; t++) tpm[t] = sum > 0.0 ? 1e6 * x[t] / sum : 0.0;
}

extern "C" int br_quant_result(br_quant *c, double *theta, double *tpm, uint64_t *unique, uint64_t *ambig) {
  if (!c || !c->finished || ((theta || tpm) && !c->em_done)) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const size_t T = (size_t)c->n_tx;
  if (!T) return BR_OK;
  std::vector<double> x;
  if (theta) HIPCHK(hipMemcpyAsync(theta, c->em.theta[c->cur].p, T * 8, hipMemcpyDeviceToHost, st));
  if (tpm) RC(quant_host_x(c, x));
  if (unique) HIPCHK(hipMemcpyAsync(unique, c->uniq.p, T * 8, hipMemcpyDeviceToHost, st));
  if (ambig) HIPCHK(hipMemcpyAsync(ambig, c->ambig.p, T * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (tpm) quant_tpm(x, tpm);
  return BR_OK;
}

// ---- gene level (the definitions: bramble_amd.h, br_quant) ---------------------------------------------------------------------------
// The map is checked by the caller.  Everything is built in tables of the call's own, which become the object's at the end: a
// call that fails leaves the object as it was.
static int quant_genes(br_quant *c, const uint32_t *tx_gene, int64_t G) {
  hipStream_t st = c->st;
  const int64_t T = c->n_tx, C = c->cls.n_cls, L = c->cls.n_lab;
  uint64_t *small = c->small.as<uint64_t>();
  br_quant::Genes g;
  DropGuard held{c, {&g.first, &g.cnt, &g.loff, &g.labels, &g.uniq, &g.ambig, &g.toff, &g.tx}};
  // per gene its transcripts in ascending order: a counting sort of T numbers on the host
  std::vector<uint64_t> toff((size_t)G + 1, 0);
  std::vector<uint32_t> order((size_t)T);
  g.n_tx.assign((size_t)G, 0);
  for (int64_t t = 0; t < T; t++) g.n_tx[tx_gene[t]]++;
  for (int64_t k = 0; k < G; k++) toff[(size_t)k + 1] = toff[(size_t)k] + g.n_tx[(size_t)k];
  {
    std::vector<uint64_t> at(toff.begin(), toff.end() - 1);
    for (int64_t t = 0; t < T; t++) order[(size_t)at[tx_gene[t]]++] = (uint32_t)t;
  }
  const size_t g1 = (size_t)G + 1;
  RC(c->alloc(g.toff, g1 * 8)); RC(c->alloc(g.tx, ((size_t)T + 1) * 4)); RC(c->alloc(g.uniq, g1 * 8)); RC(c->alloc(g.ambig, g1 * 8));
  HIPCHK(hipMemcpyAsync(g.toff.p, toff.data(), g1 * 8, hipMemcpyHostToDevice, st));
  if (T) HIPCHK(hipMemcpyAsync(g.tx.p, order.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(g.uniq.p, 0, g1 * 8, st)); HIPCHK(hipMemsetAsync(g.ambig.p, 0, g1 * 8, st));
  HIPCHK(hipStreamSynchronize(st));
  if (C > 0) {
    ColBuf d_txg, key[2], idx[2], pos, glab, goff, gk, big, rep;
    DropGuard tables{c, {&d_txg, &key[0], &key[1], &idx[0], &idx[1], &pos, &glab, &goff, &gk, &big, &rep}};
    // the distinct (class, gene) entries, a class's genes ascending: the gene-label arena
    const size_t l1 = (size_t)L + 1, c1 = (size_t)C + 1;
    RC(c->alloc(d_txg, ((size_t)T + 1) * 4));
    HIPCHK(hipMemcpyAsync(d_txg.p, tx_gene, (size_t)T * 4, hipMemcpyHostToDevice, st));
    RC(c->alloc(key[0], l1 * 8)); RC(c->alloc(key[1], l1 * 8)); RC(c->alloc(idx[0], l1 * 4)); RC(c->alloc(idx[1], l1 * 4));
    launch_qg_key(st, c->cls.loff.as<uint64_t>(), c->cls.labels.as<uint32_t>(), d_txg.as<uint32_t>(), C, L, key[0].as<uint64_t>(), idx[0].as<uint32_t>());
    RC(quant_sort(c, key, idx, L));
    RC(c->alloc(pos, l1 * 8)); RC(quant_tmp(c, L));
    launch_qg_flag(st, key[0].as<uint64_t>(), L, pos.as<uint64_t>());
    launch_scan(st, pos.as<uint64_t>(), L, c->tmp.as<uint64_t>());
    uint64_t LE = 0;
    HIPCHK(hipMemcpyAsync(&LE, pos.as<uint64_t>() + L, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (LE == 0 || LE > (uint64_t)L) return BR_ERR_HIP;
    RC(c->alloc(glab, ((size_t)LE + 1) * 4)); RC(c->alloc(goff, c1 * 8)); RC(c->alloc(gk, c1 * 4));
    launch_qg_arena(st, key[0].as<uint64_t>(), pos.as<uint64_t>(), c->cls.loff.as<uint64_t>(), L, C, glab.as<uint32_t>(), goff.as<uint64_t>(), gk.as<uint32_t>());
    HIPCHK(hipStreamSynchronize(st));
    c->drop(d_txg); c->drop(pos);
    for (int k = 0; k < 2; k++) { c->drop(key[k]); c->drop(idx[k]); }
    // the hash of every gene list
    const size_t most = (size_t)(LE / (Q_WAVE_ITEMS + 1) + 1);
    RC(c->alloc(big, most * 4));
    HIPCHK(hipMemsetAsync(small + QS_NBIG, 0, 8, st));
    launch_q_bin(st, goff.as<uint64_t>(), C, big.as<uint32_t>(), (uint32_t *)(small + QS_NBIG));
    uint32_t n_big = 0;
    HIPCHK(hipMemcpyAsync(&n_big, small + QS_NBIG, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    RC(c->alloc(key[0], c1 * 8)); RC(c->alloc(key[1], c1 * 8)); RC(c->alloc(idx[0], c1 * 4)); RC(c->alloc(idx[1], c1 * 4));
    const uint64_t mask = c->hash_bits >= 64 ? ~0ull : (1ull << c->hash_bits) - 1;
    launch_qg_hash(st, glab.as<uint32_t>(), goff.as<uint64_t>(), C, big.as<uint32_t>(), n_big, mask, key[0].as<uint64_t>(), idx[0].as<uint32_t>());
    // their classes: a transcript class's first name and count are the item's, and rep names the class whose gene list it is
    RC(quant_classes(c, glab.as<uint32_t>(), goff.as<uint64_t>(), gk.as<uint32_t>(), c->cls.first.as<uint64_t>(), c->cls.cnt.as<uint64_t>(), key, idx, C, g, &rep));
    if (g.n_lab == 0 || (uint64_t)g.n_lab > LE) return BR_ERR_HIP;
    RC(c->alloc(g.labels, ((size_t)g.n_lab + 1) * 4));
    launch_qg_labels(st, g.loff.as<uint64_t>(), rep.as<uint32_t>(), goff.as<uint64_t>(), glab.as<uint32_t>(), g.cnt.as<uint64_t>(), g.n_cls, g.n_lab,
                     g.labels.as<uint32_t>(), g.uniq.as<uint64_t>(), g.ambig.as<uint64_t>());
    HIPCHK(hipStreamSynchronize(st));
  }
  c->gene = std::move(g);   // (a swap: the guard drops the empty tables the object had)
  return BR_OK;
}

extern "C" int br_quant_genes(br_quant *c, const uint32_t *tx_gene, int64_t n_genes, int64_t *n_gene_classes) {
  if (!c || !c->finished || c->genes_done || n_genes < 0 || n_genes >= (1ll << 32) || (c->n_tx && !tx_gene)) return BR_ERR_INVALID_ARG;
  for (int64_t t = 0; t < c->n_tx; t++) if ((int64_t)tx_gene[t] >= n_genes) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  RC(quant_genes(c, tx_gene, n_genes));
  c->n_genes = n_genes; c->genes_done = true;
  c->genes_s = timer.seconds();
  if (n_gene_classes) *n_gene_classes = c->gene.n_cls;
  return BR_OK;
}

extern "C" int br_quant_gene_classes(br_quant *c, uint64_t *label_off, uint32_t *labels, uint64_t *counts, uint64_t *first_name) {
  return c && c->genes_done ? quant_copy_classes(c, c->gene, label_off, labels, counts, first_name) : BR_ERR_INVALID_ARG;
}

extern "C" int br_quant_gene_result(br_quant *c, double *num_reads, double *tpm, double *length, double *eff_length, uint64_t *unique,
                                    uint64_t *ambig, uint32_t *n_transcripts) {
  if (!c || !c->genes_done) return BR_ERR_INVALID_ARG;
  const bool sums = num_reads || tpm || length || eff_length;
  if (sums && !c->em_done) return BR_ERR_INVALID_ARG;
  if (eff_length && (!c->eff_len || !c->eff.p)) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  const size_t T = (size_t)c->n_tx, G = (size_t)c->n_genes;
  if (!G) return BR_OK;
  ColBuf d_tpm, d_lens, out;   // out: num_reads, tpm, length, eff_length
  DropGuard dropper{c, {&d_tpm, &d_lens, &out}};
  std::vector<double> x(T), tpm_t(T);
  if (sums) {
    const bool has_lens = !c->lens.empty();
    RC(c->alloc(d_tpm, (T + 1) * 8)); RC(c->alloc(out, (4 * G + 1) * 8));
    if (has_lens) RC(c->alloc(d_lens, (T + 1) * 8));
    RC(quant_host_x(c, x));
    quant_tpm(x, tpm_t.data());   // the values br_quant_result returns
    if (T) HIPCHK(hipMemcpyAsync(d_tpm.p, tpm_t.data(), T * 8, hipMemcpyHostToDevice, st));
    if (T && has_lens) HIPCHK(hipMemcpyAsync(d_lens.p, c->lens.data(), T * 8, hipMemcpyHostToDevice, st));
    double *o = out.as<double>();
    launch_qg_sums(st, c->gene.toff.as<uint64_t>(), c->gene.tx.as<uint32_t>(), (int64_t)G, c->em.theta[c->cur].as<double>(), d_tpm.as<double>(),
                   has_lens ? d_lens.as<int64_t>() : nullptr, eff_length ? c->eff.as<double>() : nullptr, o, o + G, o + 2 * G, eff_length ? o + 3 * G : nullptr);
    if (num_reads) HIPCHK(hipMemcpyAsync(num_reads, o, G * 8, hipMemcpyDeviceToHost, st));
    if (tpm) HIPCHK(hipMemcpyAsync(tpm, o + G, G * 8, hipMemcpyDeviceToHost, st));
    if (length) HIPCHK(hipMemcpyAsync(length, o + 2 * G, G * 8, hipMemcpyDeviceToHost, st));
    if (eff_length) HIPCHK(hipMemcpyAsync(eff_length, o + 3 * G, G * 8, hipMemcpyDeviceToHost, st));
  }
  if (unique) HIPCHK(hipMemcpyAsync(unique, c->gene.uniq.p, G * 8, hipMemcpyDeviceToHost, st));
  if (ambig) HIPCHK(hipMemcpyAsync(ambig, c->gene.ambig.p, G * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_transcripts) memcpy(n_transcripts, c->gene.n_tx.data(), G * 4);
  return BR_OK;
}

// the B x G gene replicates, made from the B x T result when they are first asked for (br_quant_genes and br_quant_bootstrap come
// in either order) and held from then on
static int quant_gene_boot(br_quant *c) {
  if (c->gene_boot.p) return BR_OK;
  const size_t B = (size_t)c->bootstraps, G = (size_t)c->n_genes;
  ColBuf t;
  DropGuard dropper{c, {&t}};
  RC(c->alloc(t, (B * G + 1) * 8));
  launch_qg_boot(c->st, c->boot_res.as<double>(), c->n_tx, (int64_t)B, c->gene.toff.as<uint64_t>(), c->gene.tx.as<uint32_t>(), (int64_t)G, t.as<double>());
  HIPCHK(hipStreamSynchronize(c->st));
  c->gene_boot = std::move(t);
  return BR_OK;
}

extern "C" int br_quant_gene_boot(br_quant *c, int32_t first, int32_t count, double *num_reads) {
  if (!c || !c->genes_done || !c->boot_done || !c->boot_res.p || first < 0 || count < 0 || (int64_t)first + count > c->bootstraps) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  RC(quant_gene_boot(c));
  const size_t G = (size_t)c->n_genes;
  if (num_reads && G && count) HIPCHK(hipMemcpyAsync(num_reads, c->gene_boot.as<double>() + (size_t)first * G, (size_t)count * G * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_quant_gene_boot_summary(br_quant *c, double *mean, double *var) {
  if (!c || !c->genes_done || !c->boot_done || !c->boot_res.p) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  RC(quant_gene_boot(c));
  return quant_summary(c, c->gene_boot, (size_t)c->n_genes, mean, var);
}

extern "C" int br_quant_gene_stats(const br_quant *c, double *seconds, int64_t *n_gene_labels, uint64_t *collisions) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (seconds) *seconds = c->genes_s;
  if (n_gene_labels) *n_gene_labels = c->gene.n_lab;
  if (collisions) *collisions = c->gene.collisions;
  return BR_OK;
}

extern "C" int br_quant_stats(const br_quant *c, uint64_t *held_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds,
                              double *em_seconds, uint64_t *collisions, int64_t *n_unassigned, int64_t *n_labels) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (held_bytes) *held_bytes = c->live;
  if (peak_bytes) *peak_bytes = c->peak;
  if (add_seconds) *add_seconds = c->add_s;
  if (finish_seconds) *finish_seconds = c->finish_s;
  if (em_seconds) *em_seconds = c->em_s;
  if (collisions) *collisions = c->cls.collisions;
  if (n_unassigned) *n_unassigned = c->finished ? c->n - c->n_assigned : 0;
  if (n_labels) *n_labels = c->cls.n_lab;
  return BR_OK;
}

// test hook: the device's psi over n numbers in host memory
extern "C" int br_quant_digamma(int device, const double *a, int64_t n, double *out) {
  if (n < 0 || (n && (!a || !out))) return BR_ERR_INVALID_ARG;
  Accum acc;
  RC(acc.open(device));
  ColBuf in, res;
  int rc = BR_OK;
  {
    DropGuard dropper{&acc, {&in, &res}};
    auto run = [&]() -> int {
      if (!n) return BR_OK;
      RC(acc.alloc(in, (size_t)n * 8)); RC(acc.alloc(res, (size_t)n * 8));
      HIPCHK(hipMemcpyAsync(in.p, a, (size_t)n * 8, hipMemcpyHostToDevice, acc.st));
      launch_q_digamma(acc.st, in.as<double>(), n, res.as<double>());
      HIPCHK(hipMemcpyAsync(out, res.p, (size_t)n * 8, hipMemcpyDeviceToHost, acc.st));
      HIPCHK(hipStreamSynchronize(acc.st));
      return BR_OK;
    };
    rc = run();
  }
  acc.close();
  return rc;
}
