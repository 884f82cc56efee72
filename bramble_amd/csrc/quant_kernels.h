// Transcript quantification on the device: read names -> transcript sets -> equivalence classes -> EM (quant_kernels.hip; host
// side: quant.cpp, which holds the pipeline's description).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "names.h"

namespace br {

constexpr int Q_SMALL_ROWS = 16;   // a read name of up to this many rows is one lane's work in k_q_names, a larger one a wave's
constexpr int Q_WAVE_ITEMS = 64;   // a class of more labels / a transcript in more classes than this is a wave's work in the EM
constexpr unsigned Q_BIG_GRID = 1024;   // blocks (of 4 waves) that walk a list whose length only the device knows

// One add.  The rows may be a slice of the caller's table (a host add uploads only what it needs): row r is at a[r - a_bias];
// the names as names.h holds them.
struct QAddArgs {
  const uint4 *a; int64_t a_bias;              // br_row_a
  NameWindow names;
  uint64_t lab_base;          // arena slot of row r_first
  uint32_t *lab;              // label arena: a name's list sits at the slot of its first row (as many slots as it has rows)
  uint64_t *noff; uint32_t *nk; uint64_t *hash;   // per name, at the add's first name: arena offset, labels, hash of (k, labels)
  uint32_t *big; uint32_t *n_big;   // names of more than Q_SMALL_ROWS rows: k_q_names lists them, k_q_names_big takes them
  uint32_t *max_tid;          // the largest transcript id met so far (atomicMax)
  uint32_t *bad;              // a name whose rows leave [r_first, r_last): nothing is written for it
  // the fragment pass (launch_q_frag; "eff_len"): the rows' CIGAR references, at the bias of a, and the pool they point into
  const uint64_t *cigar; const uint32_t *pool; uint64_t n_pool_words;
  uint32_t fld_max;
  unsigned long long *stage;  // the add's own histogram, fld_max + 1 bins, then observations / unique names without a fragment /
                              // lengths out of range (Q_FLD_SIDE words); *bad |= 1 for a pooled CIGAR that leaves the pool
};
constexpr int Q_FLD_SIDE = 3;             // words behind a histogram: n_obs, n_no_fragment, n_out_of_range
constexpr uint32_t Q_FLD_LDS_BINS = 8192; // up to this many bins a block counts in LDS (32 KiB of counters); above, in the table itself
constexpr uint32_t Q_EFF_LDS_BINS = 2048; // up to this many bins k_q_efflen keeps C and S in LDS (32 KiB); above, it loads them from HBM
// span[0] = row_off[group_off[0]], span[1] = row_off[group_off[n_groups]] of device tables
void launch_q_span(hipStream_t st, const uint64_t *row_off, const uint32_t *group_off, int64_t n_groups, uint64_t *span);
void launch_q_names(hipStream_t st, const QAddArgs &A);
// after launch_q_names of the same add (nk and the list of big names are its): per read name of one label its first fragment's
// length into A.stage (definitions: bramble_amd.h, br_quant)
void launch_q_frag(hipStream_t st, const QAddArgs &A);
// total[i] += stage[i]; stage[i] = 0, over fld_max + 1 + Q_FLD_SIDE words
void launch_q_fld_commit(hipStream_t st, unsigned long long *stage, unsigned long long *total, uint32_t n_words);
// cs[f] = C(f), cs[n_bins + f] = S(f): the inclusive prefix sums of hist[f] and f * hist[f]
void launch_q_fld_prefix(hipStream_t st, const unsigned long long *hist, uint32_t n_bins, uint64_t *cs);
// eff[t] and w[t] = 1 / eff[t] (0 where eff is 0) from the lengths and the prefix sums
void launch_q_efflen(hipStream_t st, const int64_t *lens, int64_t n_tx, const uint64_t *cs, uint32_t n_bins, double *eff, double *w);

// br_quant_drop_names: nk[i] = 0 where flags[i] != 0 (k_q_flag then sees a name without labels); *n_dropped += those names
void launch_q_drop(hipStream_t st, const uint8_t *flags, int64_t n, uint32_t *nk, unsigned long long *n_dropped);

// finish: the assigned names (k > 0) in add order -> (hash & mask, name index)
void launch_q_flag(hipStream_t st, const uint32_t *nk, int64_t n, uint64_t *flag);
void launch_q_compact(hipStream_t st, const uint32_t *nk, const uint64_t *hash, const uint64_t *pos, int64_t n, uint64_t mask,
                      uint64_t *key, uint32_t *idx);
// bits[0] = OR, bits[1] = AND over key[0, n) (part: 2 words per block of 256)
void launch_q_bits(hipStream_t st, const uint64_t *key, int64_t n, uint64_t *part, uint64_t *bits);
// head[j] = sorted item j starts a class (its label list differs from item j - 1's); *n_coll = adjacent pairs with equal keys and
// different lists.  mark != NULL: mark[first item of the key's run] = 1 for those pairs
void launch_q_heads(hipStream_t st, const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, const uint64_t *key,
                    const uint32_t *idx, int64_t n, uint64_t *head, unsigned long long *n_coll, uint32_t *mark);
// the marked runs ordered by (k, labels, name index), every other item where it was
void launch_q_resolve(hipStream_t st, const uint32_t *lab, const uint64_t *noff, const uint32_t *nk, const uint64_t *key,
                      const uint32_t *idx, int64_t n, const uint32_t *mark, uint64_t *key_out, uint32_t *idx_out);
// classes in hash order (gbeg: their starts among the sorted items idx) -> (first name, class in hash order), to be sorted.  An
// item's first name is item_first[i]; NULL: i itself (a read name)
void launch_q_class_key(hipStream_t st, const uint64_t *gbeg, const uint32_t *idx, const uint64_t *item_first, int64_t n_cls, uint64_t *key,
                        uint32_t *val);
// classes in their final order: first name, count, number of labels (to be scanned into label_off) and, rep != NULL, an item
// whose list is the class's.  The count is the sum of the items' weights, from pre, the scanned weights of the sorted items; NULL:
// every item weighs 1
void launch_q_class_fill(hipStream_t st, const uint64_t *key, const uint32_t *val, const uint64_t *gbeg, const uint32_t *idx, const uint64_t *pre,
                         const uint32_t *nk, int64_t n_cls, uint64_t *first, uint64_t *cnt, uint64_t *label_off, uint32_t *rep);
// "keep_names": name_cls[idx[j]] = the final index of sorted item j's class.  head: the scanned heads (n + 1 entries), val: the
// classes' hash-order indices in their final order (the second sort's result), inv: n_cls words of scratch
void launch_q_name_cls(hipStream_t st, const uint64_t *head, const uint32_t *idx, int64_t n, const uint32_t *val, int64_t n_cls, uint32_t *inv,
                       uint32_t *name_cls);
// post[e] = theta_t w_t / d_c for label entry e of class c with transcript t, d_c the sum over the class's labels in ascending
// order, one after the other (0 where d_c == 0).  w = NULL: theta is x itself (a variational run's), post[e] = x_t / d_c
void launch_q_post(hipStream_t st, const uint64_t *label_off, const uint32_t *labels, int64_t n_cls, const double *theta, const double *w,
                   double *post);
// one thread per label entry e: labels[e], its class, (transcript, e) for the transposed table; *bad |= 1 for a transcript
// whose length is <= 0 (lens != NULL)
void launch_q_labels(hipStream_t st, const uint64_t *label_off, const uint64_t *first, const uint64_t *noff, const uint32_t *lab,
                     int64_t n_cls, int64_t n_lab, const int64_t *lens, uint32_t *labels, uint32_t *ecls, uint64_t *tkey,
                     uint32_t *tidx, uint32_t *bad);
// the transposed table: t_cls[p] = class of the p-th (transcript, entry) pair; t_off[t] = the first pair of transcript t
void launch_q_transpose(hipStream_t st, const uint64_t *tkey, const uint32_t *tidx, const uint32_t *ecls, int64_t n_lab,
                        int64_t n_tx, uint32_t *t_cls, uint64_t *t_off);
// the items of more than Q_WAVE_ITEMS entries (off: n + 1 offsets), in any order
void launch_q_bin(hipStream_t st, const uint64_t *off, int64_t n, uint32_t *list, uint32_t *n_list);
void launch_q_counts(hipStream_t st, const uint32_t *t_cls, const uint64_t *t_off, const uint64_t *label_off, const uint64_t *cnt,
                     int64_t n_tx, const uint32_t *big, uint32_t n_big, uint64_t *uniq, uint64_t *ambig);

// EM.  x = theta * w.  It runs over a chunk of W = 1 << lw replicates (W <= 64): theta, x (n_tx * W), q and the resampled counts
// (n_cls * W) hold replicate j of item i at [i * W + j].  The point EM is the chunk of one replicate (lw = 0, active = 1) on the
// observed counts, and has instantiations of its own in which those are compile-time facts.  One iteration, per replicate in
// `active`: launch_q_em_classes (q[c] = n_c / sum of x over the class, 0 when that is 0), then launch_q_em_tx (theta'[t] = x[t] *
// sum of q over the classes of t in ascending class order; x'[t] = theta'[t] * w[t]); a frozen replicate's theta and x are copied
// through.  rel != NULL: W words, rel[j] takes the atomicMax of the bits of |theta' - theta| / theta' over theta' > 1e-8 of replicate
// j (non-negative doubles order like their bits)
constexpr int Q_BOOT_CHUNK = 16;   // the bootstrap's default W: a gather of 16 doubles is one 128-byte line
struct QEmArgs {
  int64_t n_cls, n_tx;
  const uint64_t *label_off; const uint32_t *labels;
  const uint64_t *cnt;        // the observed counts, n_cls: the point EM's (a chunk does not read them)
  const uint64_t *t_off; const uint32_t *t_cls;
  const uint32_t *big_cls; uint32_t n_big_cls; const uint32_t *big_tx; uint32_t n_big_tx;
  const double *w;
  double *q;                  // n_cls * W
  // a chunk's; the point instantiations ignore the three
  const uint32_t *boot_cnt;   // the resampled counts, n_cls * W
  int lw;
  uint64_t active;            // bit j: replicate j of the chunk still runs
};
// theta = 1, x = w for every replicate of the chunk
void launch_q_em_init(hipStream_t st, const double *w, int64_t n_tx, int lw, double *theta, double *x);
// boot_cnt == NULL: the point EM
void launch_q_em_classes(hipStream_t st, const QEmArgs &E, const double *x);
void launch_q_em_tx(hipStream_t st, const QEmArgs &E, const double *theta, const double *x, double *theta_out, double *x_out,
                    unsigned long long *rel);

// Bootstrap replicates (definitions: bramble_amd.h, br_quant).
// the resampled counts of replicates b_first .. b_first + n_rep - 1: one lane a draw (Philox4x32-10 under `seed`, counter (draw,
// replicate), rank = high half of u * n, class by binary search in cum, the exclusive prefix sums of the counts with cum[n_cls] = n),
// one integer atomicAdd each into out[c * stride_c + (b - b_first) * stride_b], which the caller has zeroed
void launch_q_boot_sample(hipStream_t st, const uint64_t *cum, int64_t n_cls, uint64_t n, uint64_t seed, uint32_t b_first, uint32_t n_rep,
                          uint32_t *out, int64_t stride_c, int64_t stride_b);
// out[j * n_tx + t] = theta[t * W + j] for j < n_rep
void launch_q_boot_store(hipStream_t st, const double *theta, int64_t n_tx, int lw, int n_rep, double *out);
// mean and variance (over n_boot - 1; 0 for n_boot = 1) per transcript of the n_boot x n_tx result, summed in replicate order
void launch_q_boot_summary(hipStream_t st, const double *res, int64_t n_tx, int32_t n_boot, double *mean, double *var);

// Variational Bayes (definitions: bramble_amd.h, br_quant, `variational`), for the point EM (lw = 0, active = 1) and a chunk alike.
// After launch_q_em_tx has written theta (alpha'): x[t * W + j] = exp(psi(theta + prior[t]) - psi(S_j)) * w[t]
// for every replicate j in `active`, S_j the sum of theta + prior over the transcripts -- per block of 256 transcripts a partial
// (part: ceil(n_tx / 256) * W doubles), the partials in a fixed order (psi_s: W doubles), no atomics.  Three launches
void launch_q_vb_x(hipStream_t st, const double *theta, const double *prior, const double *w, int64_t n_tx, int lw, uint64_t active, double *part,
                   double *psi_s, double *x_out);
// out[i] = the device's psi(a[i]) (NaN where a[i] is not a positive finite number)
void launch_q_digamma(hipStream_t st, const double *a, int64_t n, double *out);

// Gene level (definitions: bramble_amd.h, br_quant).
// key[e] =(class of label entry e << 32) | tx_gene[labels[e]], idx[e] = e: to be sorted
void launch_qg_key(hipStream_t st, const uint64_t *label_off, const uint32_t *labels, const uint32_t *tx_gene, int64_t n_cls, int64_t n_lab,
                   uint64_t *key, uint32_t *idx);
// flag[e] = sorted key e differs from key e - 1: a distinct (class, gene) entry (to be scanned)
void launch_qg_flag(hipStream_t st, const uint64_t *key, int64_t n, uint64_t *flag);
// the gene-label arena from the sorted keys and the scanned flags: glab, and per class its offset (n_cls + 1) and length
void launch_qg_arena(hipStream_t st, const uint64_t *key, const uint64_t *pos, const uint64_t *label_off, int64_t n_lab, int64_t n_cls,
                     uint32_t *glab, uint64_t *goff, uint32_t *gk);
// key[c] = the names' hash of class c's gene list under mask, idx[c] = c; big: the classes of more than Q_WAVE_ITEMS genes (launch_q_bin)
void launch_qg_hash(hipStream_t st, const uint32_t *glab, const uint64_t *goff, int64_t n_cls, const uint32_t *big, uint32_t n_big, uint64_t mask,
                    uint64_t *key, uint32_t *idx);
// w[j] = cnt[idx[j]]: the sorted items' weights (to be scanned into launch_q_class_fill's pre)
void launch_qg_member_cnt(hipStream_t st, const uint32_t *idx, const uint64_t *cnt, int64_t n, uint64_t *w);
// labels[e] from the list of rep[class of e], and cnt of e's class added to uniq / ambig of its gene (zeroed by the caller)
void launch_qg_labels(hipStream_t st, const uint64_t *label_off, const uint32_t *rep, const uint64_t *goff, const uint32_t *glab, const uint64_t *cnt,
                      int64_t n_cls, int64_t n_lab, uint32_t *labels, uint64_t *uniq, uint64_t *ambig);
// per gene the sums over its transcripts g_tx[g_toff[g] .. g_toff[g + 1]) in that order; lens / eff / eff_length may be NULL
void launch_qg_sums(hipStream_t st, const uint64_t *g_toff, const uint32_t *g_tx, int64_t n_genes, const double *theta, const double *tpm_t,
                    const int64_t *lens, const double *eff, double *num_reads, double *tpm, double *length, double *eff_length);
// out[b * n_genes + g] = the sum of res[b * n_tx + t] over the gene's transcripts in that order
void launch_qg_boot(hipStream_t st, const double *res, int64_t n_tx, int64_t n_boot, const uint64_t *g_toff, const uint32_t *g_tx, int64_t n_genes,
                    double *out);

}  // namespace br
