/* bramble_amd -- MI355X-native genome -> transcriptome projection engine.
 *
 * C ABI of libbramble_amd.so: the drop-in boundary for bramble's projection hot
 * path.  Every entry point names the reference interface it replaces
 * (paths relative to the bramble tree).  No torch / HIP types appear here:
 * plain pointers, sizes and opaque handles only.  Device pointers are passed as
 * `void *` / typed pointers that the caller obtained from its own allocator
 * (hipMalloc, a torch tensor's data_ptr, ...).
 *
 * Conventions (same as the reference):
 *   - exon intervals are 1-based half-open [start, end) (GTF end + 1;
 *     src/bramble.cpp:164-165, bramble-rs/src/annotation.rs:52-64);
 *   - ref_start / mate_start are 1-based SAM POS; projected `pos` is the 0-based
 *     BAM core.pos the reference writes (src/core.cpp:153-158);
 *   - CIGAR words are BAM-packed (len << 4 | op), ops 0..9 as in the SAM spec;
 *   - input batches are name-collated: all alignments of one query name are
 *     contiguous (README.md:39-52).
 *
 * All functions return BR_OK (0) or a negative BR_ERR_* code; none aborts.
 * The library never falls back to a CPU path: without a usable HIP device the
 * device entry points return BR_ERR_NO_DEVICE.
 */
#ifndef BRAMBLE_AMD_H
#define BRAMBLE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BR_OK 0
#define BR_ERR_INVALID_ARG (-1)
#define BR_ERR_NO_DEVICE (-2)
#define BR_ERR_HIP (-3)
#define BR_ERR_ANNOTATION (-4) /* unknown seqname, overlapping exons inside a transcript, ... */
#define BR_ERR_CAPACITY (-5)   /* batch exceeds 32-bit device offsets; split it */
#define BR_ERR_UNSUPPORTED (-6)

/* ---- annotation ------------------------------------------------------------ */

/* bramble-rs/src/annotation.rs:13-17 (Exon) */
typedef struct br_exon { uint32_t start, end; } br_exon;

/* bramble-rs/src/annotation.rs:19-25 (Transcript); strand '+' or '-' */
typedef struct br_transcript {
  const char *id;
  const char *seqname;
  char strand;
  const br_exon *exons;
  uint32_t n_exons;
} br_transcript;

/* bramble-rs/src/fasta.rs:21-108 (FastaDb::from_seqs): one named sequence */
typedef struct br_fasta_seq { const char *name; const char *seq; uint64_t len; } br_fasta_seq;

typedef struct br_index br_index; /* immutable after build; shareable across threads (g2tTree) */
typedef struct br_ctx br_ctx;     /* per host thread / per stream scratch (ProjectionContext) */

/* Replaces build_g2t_tree (src/bramble.cpp:132-211) / build_g2t_from_refnames
 * (bramble-rs/src/g2t.rs:515-532).  tid = position in `transcripts`.  `device`
 * is the HIP device ordinal the flattened exon tables are uploaded to; pass -1
 * for a host-only index (accessors work, projection does not).  `fasta` may be
 * NULL (no -S). */
int br_index_build(const br_transcript *transcripts, size_t n_transcripts, const char *const *refnames,
                   size_t n_refnames, const br_fasta_seq *fasta, size_t n_fasta, int device,
                   br_index **out);
/* Same index from flat arrays (the form a GTF loader or a generator holds):
 * transcript t lies on reference tx_ref_id[t] (0-based, < n_refs) with strand
 * tx_strand[t] and exons [tx_exon_off[t], tx_exon_off[t+1]) of (ex_start, ex_end).
 * tx_names may be NULL ("tx<t>"); fasta_by_ref is NULL or n_refs entries
 * (seq == NULL: no sequence for that reference). */
int br_index_build_flat(size_t n_tx, const int32_t *tx_ref_id, const int8_t *tx_strand,
                        const uint64_t *tx_exon_off, const uint32_t *ex_start, const uint32_t *ex_end,
                        const char *const *tx_names, size_t n_refs, const br_fasta_seq *fasta_by_ref,
                        int device, br_index **out);
void br_index_free(br_index *);
/* bramble-rs/src/g2t.rs:320-342 accessors */
size_t br_index_num_transcripts(const br_index *);
const char *br_index_transcript_name(const br_index *, uint32_t tid); /* NULL if out of range */
int64_t br_index_transcript_len(const br_index *, uint32_t tid);      /* -1 if out of range */
size_t br_index_num_refs(const br_index *);
size_t br_index_num_intervals(const br_index *);                      /* transcript-exon rows */
size_t br_index_device_bytes(const br_index *);

/* ---- configuration --------------------------------------------------------- */

/* ProjectionConfig (bramble-rs/src/api.rs:184-206) widened with the C++ CLI
 * switches that select the evaluator presets (src/bramble.cpp:457-485,
 * src/evaluate.cpp:1136-1221).  has_* = the matching --max-... / --similarity-
 * threshold override was given. */
typedef struct br_config {
  int32_t lr, lr_hq, strict; /* --lr, --lr-hq, --strict */
  int32_t use_fasta;         /* -S given (index must have been built with sequences) */
  int32_t fr, rf;            /* --fr, --rf */
  int32_t has_max_clip, has_max_junc_ins, has_max_junc_gap, has_sim_thr, has_max_error_exon;
  uint32_t max_clip, max_junc_ins, max_junc_gap, max_error_exon;
  float sim_thr;
  double junc_miss_discount; /* Rust-only knob (api.rs:197-205); must be 1.0 (C++ has none) */
} br_config;

void br_config_short_read(br_config *); /* ProjectionConfig::short_read, api.rs:210-216 */
void br_config_long_read(br_config *);  /* ProjectionConfig::long_read (= --lr), api.rs:219-225 */

/* Resolved evaluator thresholds (ReadEvaluationConfig, include/evaluate.h:275-285) */
typedef struct br_thresholds {
  uint32_t max_clip, max_junc_ins, max_junc_gap, max_error_exon;
  int32_t ignore_small_exons, filter_by_similarity;
  float similarity_threshold;
} br_thresholds;
int br_config_resolve(const br_config *, br_thresholds *out);

/* ---- struct-of-arrays batches (host memory) --------------------------------- */

/* Flat form of GenomicAlignment[] (bramble-rs/src/api.rs:73-126). */
typedef struct br_batch {
  int64_t n_aln;
  const int32_t *ref_id;     /* 0-based; < 0: alignment skipped (api.rs:316-318) */
  const int32_t *ref_start;  /* 1-based */
  const uint16_t *flags;     /* SAM flag bits: 0x1 paired, 0x10 reverse, 0x40 read1, 0x80 read2 */
  const int8_t *xs;          /* first char of XS tag or 0 */
  const int8_t *ts;          /* first char of ts tag or 0 */
  const uint64_t *cigar_off; /* n_aln + 1 */
  const uint32_t *cigar;
  const int32_t *mate_ref_id; /* -1 if none */
  const int32_t *mate_start;  /* 1-based, 0 if none */
  const uint64_t *name_off;   /* n_aln + 1 */
  const char *names;
  const uint64_t *seq_off;    /* n_aln + 1 or NULL */
  const char *seqs;           /* ASCII bases */
  const int32_t *l_qseq;
} br_batch;

/* Input contract of convert_reads computed on the host: read-name groups
 * (src/core.cpp:347-380) and the mate index of process_pairs
 * (src/bramble.cpp:272-311; at most one mate per alignment).  group_off must
 * hold n_aln + 1 entries; *n_groups receives the group count. */
int br_batch_prepare(const br_batch *, int32_t *mate_idx, uint32_t *group_off, int64_t *n_groups);

/* With -S the clip rescue uses ONE sequence per read-name group: the first
 * record of the group that has one (src/core.cpp:353-378).  seq_src[i] = index of
 * that record for alignment i, or -1. */
int br_batch_seq_source(const br_batch *, const uint32_t *group_off, int64_t n_groups, int32_t *seq_src);

/* One emitted BAM record (ProjectedAlignment, bramble-rs/src/api.rs:135-176, plus
 * the fields the C++ writer sets: rewritten CIGAR, MAPQ, mate fields;
 * src/core.cpp:96-212, src/bam.cpp:531-588).  Struct-of-arrays; arrays are owned
 * by the context and stay valid until the next projection call on it. */
typedef struct br_rows {
  int64_t n_rows;
  const int32_t *input_index;
  const uint32_t *transcript_id;
  const uint32_t *pos;            /* 0-based transcript position (fwpos / rcpos by strand) */
  const int8_t *strand;           /* transcript strand '+' / '-' */
  const uint64_t *cigar_off;      /* n_rows + 1, into cigar */
  const uint32_t *cigar;          /* rewritten CIGAR (update_cigar, src/bam.cpp:502-528) */
  const double *similarity_score;
  const int32_t *clip_score;
  const int32_t *junc_hits;
  const int32_t *aligned_len;     /* ref_consumed: transcript bases spanned */
  const uint32_t *nh, *hi, *mapq;
  const uint8_t *is_primary;      /* best similarity score per read name, libstdc++-exact tie-break (src/core.cpp:243-307) */
  const uint8_t *is_paired;       /* emitted together with its mate */
  const uint8_t *same_transcript_as_mate;
  const uint8_t *is_first;        /* read1 side of the emitted pair */
  const int32_t *mate_transcript_id, *mate_pos, *insert_size;
  const uint32_t *group;          /* read-name group index */
  /* counters of src/bramble.cpp:729-736 */
  uint64_t total_complete, total_unique, dropped_reads, total_processed;
} br_rows;

/* ---- contexts and projection ------------------------------------------------ */

int br_ctx_new(const br_index *, br_ctx **out);
void br_ctx_free(br_ctx *);

/* Replaces convert_reads minus BAM writing (include/evaluate.h:377-381; sole
 * caller process_bundle, src/threads.cpp:100-104): host batch in, rows out.
 * Uploads, runs the HIP pipeline on the context's stream, downloads, and
 * finalises primary flags on the host. */
int br_project_batch(br_ctx *, const br_config *, const br_batch *, br_rows *out);

/* Device-resident form: every pointer is a device pointer on the index's
 * device; offsets are 32-bit.  mate_idx / group_off come from
 * br_batch_prepare.  `stream` is a hipStream_t (NULL = default stream). */
typedef struct br_device_batch {
  int64_t n_aln, n_groups;
  const int32_t *ref_id;
  const int32_t *ref_start;
  const uint16_t *flags;
  const int8_t *xs, *ts;
  const uint32_t *cigar_off; /* n_aln + 1 */
  const uint32_t *cigar;
  const int32_t *mate_idx;   /* n_aln */
  const uint32_t *group_off; /* n_groups + 1 */
  const int32_t *l_qseq;
  const uint32_t *seq_off;   /* n_aln + 1 or NULL */
  const uint8_t *seqs;
  int64_t n_cigar_words;     /* total words in cigar */
  int32_t max_n_cigar;       /* longest single CIGAR in the batch */
  /* -S clip rescue only (use_fasta with --lr / --lr-hq): */
  const int32_t *seq_src;    /* n_aln, from br_batch_seq_source; NULL without sequences */
  int32_t max_soft_clip;     /* longest leading / trailing S op in the batch */
  /* optional read names (primary / secondary choice needs them; NULL: is_primary stays 0) */
  const uint32_t *name_off;  /* n_aln + 1 */
  const uint8_t *names;
} br_device_batch;

/* ABI version 2: the rows of the device-resident entry points are PACKED (24 bytes + 16 bytes of detail per emitted
 * record instead of 22 separate arrays): the row stage of the pipeline is bound by the bytes it writes, and a host
 * that downloads rows pays for them a second time over PCIe.  The wide one-array-per-field view (ABI version 1's
 * br_device_rows, now br_device_wide_rows) is derived from the packed table on request.
 * ABI version 3: the projection writes the 24 bytes only; the 16 bytes of detail (br_row_x) are derived on request as
 * well (br_device_rows.x is NULL: br_device_rows_detail(); host rows carry it with "host_detail" = 1 as before). */
#define BR_ABI_VERSION 3

/* One emitted BAM record (ProjectedAlignment, bramble-rs/src/api.rs:135-176; the fields write_to_bam sets,
 * src/core.cpp:96-212).  Rows of one read name are contiguous and a pair's two records are adjacent (the leader's own
 * record first), so
 *   HI   = 1-based rank of the row among its read name's rows (also stored in br_row_x),
 *   MAPQ = br_row_mapq(nh, long_reads)                                    (get_mapq, src/core.cpp:46-58),
 *   mate transcript / position = the adjacent row's, insert size from the two positions and the read length
 *                                                                         (set_mate_info, src/bam.cpp:531-588). */
typedef struct br_row_a {
  uint32_t transcript_id;
  uint32_t pos;   /* 0-based transcript position (fwpos / rcpos by strand) */
  uint32_t meta;  /* BR_ROW_* bits */
  uint32_t nh;    /* records emitted for the read name (NH tag) */
} br_row_a;
#define BR_ROW_NCIGAR(meta) ((meta) & 0xffffffu) /* ops of the rewritten CIGAR */
#define BR_ROW_MINUS (1u << 24)                  /* transcript strand '-' */
#define BR_ROW_PAIRED (1u << 25)                 /* emitted together with its mate (the adjacent row) */
#define BR_ROW_SAME_TX (1u << 26)                /* ... on the same transcript */
#define BR_ROW_FIRST (1u << 27)                  /* the leading record of the pair / an unpaired record; its input
                                                  * alignment is the leader of row_off[], the other row's is the mate */
#define BR_ROW_PRIMARY (1u << 28)                /* primary record of the read name (src/core.cpp:243-307) */
typedef struct br_row_x {
  uint32_t input_index; /* alignment of the batch this record rewrites */
  uint32_t junc_hits;
  uint32_t aligned_len; /* ref_consumed: transcript bases spanned */
  uint32_t hi;          /* HI tag */
} br_row_x;
uint32_t br_row_mapq(uint32_t nh, int long_reads); /* get_mapq, src/core.cpp:46-58 */

/* Packed rows as device pointers; valid until the next projection call on the context.
 * cigar[r]: the rewritten CIGAR (update_cigar, src/bam.cpp:502-528) itself when it has <= 2 ops (op 0 in the low
 * word, op 1 in the high word), else the offset of its ops in pool[] (on the device: the sparse CIGAR arena the emit
 * pass wrote; the host entry points compact it).  row_off[i] .. row_off[i + 1] are the rows
 * emitted by alignment i as the leader (for itself and, alternating, its mate). */
typedef struct br_device_rows {
  int64_t n_rows, n_matches, n_pool_words;
  const br_row_a *a;
  const uint64_t *cigar;
  const br_row_x *x;              /* NULL: the detail column is derived on request, br_device_rows_detail() */
  const double *similarity_score; /* NULL unless the preset filters by similarity (then every score is 0.0) */
  const int32_t *clip_score;      /* NULL likewise (0) */
  const uint32_t *pool;
  const uint64_t *row_off;        /* n_aln + 1 */
  uint64_t total_complete, total_unique, dropped_reads, total_processed;
} br_device_rows;

/* br_row_x of the rows of the context's last projection call (a device array of n_rows entries, valid until the next
 * projection call): derived on the first request from what the call left in HBM -- the projection itself writes 24 bytes
 * per record (br_row_a + the CIGAR reference). */
int br_device_rows_detail(br_ctx *, void *stream, const br_row_x **x);

/* The wide view: same field meaning as br_rows; is_primary is filled when the batch carries read names. */
typedef struct br_device_wide_rows {
  int64_t n_rows, n_cigar_words;
  const int32_t *input_index;
  const uint32_t *transcript_id, *pos;
  const int8_t *strand;
  const uint64_t *cigar_off;
  const uint32_t *cigar;
  const double *similarity_score;
  const int32_t *clip_score, *junc_hits, *aligned_len;
  const uint32_t *nh, *hi, *mapq;
  const uint8_t *is_paired, *same_transcript_as_mate, *is_first;
  const int32_t *mate_transcript_id, *mate_pos, *insert_size;
  const uint32_t *group;
  const uint8_t *is_primary;
} br_device_wide_rows;

int br_project_batch_device(br_ctx *, const br_config *, const br_device_batch *, void *stream,
                            br_device_rows *out);
/* Derives the wide view of the LAST projection call's rows on the device (arrays owned by the context, valid until
 * the next projection call). */
int br_device_rows_expand(br_ctx *, void *stream, br_device_wide_rows *out);

/* ---- flat batches over PCIe: packed rows home, uploads / downloads overlapped with the projection ------------- */

/* Packed rows in pinned host memory owned by the context (one set per staging slot).  The per-record fields are
 * those of br_device_rows; x (detail) is NULL unless br_ctx_set_param("host_detail", 1).  mate_idx is the mate index
 * the device computed for the batch (process_pairs, src/bramble.cpp:272-311): the input alignment of a row of leader
 * i is i when BR_ROW_FIRST is set, else mate_idx[i]. */
typedef struct br_host_rows {
  int64_t n_rows, n_aln, n_groups, n_pool_words;
  const br_row_a *a;
  const uint64_t *cigar;
  const uint32_t *pool;
  const uint64_t *row_off;  /* n_aln + 1 */
  const int32_t *mate_idx;  /* n_aln */
  const br_row_x *x;
  const double *similarity_score;
  const int32_t *clip_score;
  uint64_t total_complete, total_unique, dropped_reads, total_processed;
} br_host_rows;

/* convert_reads minus BAM writing for a flat host batch in three steps, so that batch k + 1 uploads and batch
 * k - 1 downloads while batch k is projected (one host thread suffices):
 *   br_batch_stage(ctx, batch, slot)      queues the uploads of `batch` on the context's copy stream (slot 0 / 1);
 *                                         the arrays must stay valid, and should be pinned (br_pin_host), until
 *                                         br_project_staged(slot) has returned;
 *   br_project_staged(ctx, cfg, slot, out) computes the input contract on the device (read-name groups, mate index,
 *                                         the group's shared sequence: what br_batch_prepare / br_batch_seq_source
 *                                         do on the host), projects, and queues the download of the packed rows;
 *   br_host_rows_wait(ctx, slot)          returns when that slot's rows are in host memory; they stay valid until
 *                                         the slot's next br_project_staged.
 * br_project_batch_packed = the three in sequence on slot 0. */
int br_batch_stage(br_ctx *, const br_batch *, int slot);
int br_project_staged(br_ctx *, const br_config *, int slot, br_host_rows *out);
int br_host_rows_wait(br_ctx *, int slot);
int br_project_batch_packed(br_ctx *, const br_config *, const br_batch *, br_host_rows *out);
/* Page-locks caller memory for asynchronous transfers (hipHostRegister / hipHostUnregister behind plain C). */
int br_pin_host(void *p, size_t bytes);
int br_unpin_host(void *p);

/* AoS convenience mirroring project_group_with (bramble-rs/src/api.rs:285-464):
 * all alignments of ONE query name in, one br_projected per emitted record out
 * (array owned by the context; alignments with ref_id < 0 are skipped, api.rs:316-318).
 * The shape is the Rust library's, the values are the C++ path's.
 * NOTE FOR CALLERS COMING FROM bramble-rs -- PAIRING DIFFERS: mates pair up by the C++ rule
 * (process_pairs, src/bramble.cpp:272-311: the LEFT mate, mate_start > start, is entered
 * under name + position and only a later RIGHT mate looks it up), not by the order-independent
 * mutual match of find_mate_pairs (groups.rs:125-193).  A group that lists the right-hand mate
 * BEFORE the left-hand one is a pair in bramble-rs and two unpaired alignments here (and in the
 * C++ binary: groups.rs:131-140 describes exactly this).  There is no switch: the C++ path is
 * the results authority of this library.  hit_index is carried for layout parity only (neither
 * rule reads it).  br_project_groups takes any number of name-collated groups in one call
 * (the Rust CLI hands over 64 at a time, bramble-cli/src/pipeline.rs:29): one trip through
 * the device pipeline instead of one per group. */
typedef struct br_alignment { /* GenomicAlignment, api.rs:73-126 */
  const char *query_name;
  int32_t ref_id;
  int64_t ref_start;
  uint8_t is_reverse, is_paired, is_first_in_pair, mate_is_unmapped;
  char xs_strand, ts_strand; /* 0 = absent */
  int32_t hit_index;
  int32_t mate_ref_id;       /* -1 = none */
  int64_t mate_ref_start;    /* 0 = none */
  const uint32_t *cigar;     /* BAM-packed */
  uint32_t n_cigar;
  const char *sequence;      /* ASCII or NULL */
  uint32_t sequence_len;
  uint32_t read_len;
} br_alignment;

typedef struct br_projected { /* ProjectedAlignment, api.rs:135-176 */
  uint32_t transcript_id;
  uint32_t transcript_start; /* align_pos (groups.rs:362-368): fwpos / rcpos, 0-BASED like the Rust code and the BAM
                              * POS field (the doc comment at api.rs:141-142 says 1-based; the code does not add 1) */
  uint32_t transcript_end;   /* transcript_start + aligned_len - 1, saturating */
  uint32_t aligned_len, query_aligned_len;
  uint8_t is_reverse;        /* api.rs:453 <- evaluate.rs:1062: transcript strand != the read's inferred strand
                              * (infer_strand, api.rs:470-489: XS, else ts flipped on a reverse read, else '.': then 1) */
  char transcript_strand;    /* '+' / '-': AlignInfo::strand of the C++ path (what src/bam.cpp:549-553 acts on) */
  double similarity_score;
  uint32_t nh, hi;
  uint8_t is_primary, same_transcript_as_mate, is_paired_out;
  int32_t insert_size;
  uint64_t input_index;
  uint32_t mapq;
  const uint32_t *cigar;     /* rewritten CIGAR, owned by the context */
  uint32_t n_cigar;
} br_projected;

int br_project_group(br_ctx *, const br_config *, const br_alignment *alns, size_t n,
                     const br_projected **out, size_t *n_out);
int br_project_groups(br_ctx *, const br_config *, const br_alignment *alns, size_t n,
                      const br_projected **out, size_t *n_out);

/* ---- BAM record re-encoding (next row of the scope table: the data format after the path) -- */

/* The batch's original alignment records in HBM: BAM file layout starting at refID
 * (without the 4-byte block_size), record i = blob[rec_off[i] .. rec_off[i+1]). */
typedef struct br_device_records {
  const uint8_t *blob;
  const uint64_t *rec_off; /* n_aln + 1 (n_aln suffices when rec_len is given) */
  int64_t n_aln;
  const uint32_t *rec_len; /* n_aln record lengths (the BAM block_size), or NULL: rec_off[i+1]-rec_off[i] */
} br_device_records;

typedef struct br_device_bam {
  const uint8_t *data;     /* [block_size][record] per emitted row, concatenated (uncompressed BAM stream) */
  uint64_t n_bytes;
  const uint64_t *row_off; /* n_rows + 1 */
  int64_t n_rows;
} br_device_bam;

/* Replaces the per-record byte work of write_to_bam (src/core.cpp:96-212: update_cigar,
 * NH/HI/AS tags, XS/ts deletion, reverse_complement_bam, set_mate_info; src/bam.cpp:474-702)
 * for every row of the LAST br_project_batch_device call on this context.  The rows must have
 * been produced with read names (is_primary decides the secondary flag).  A rewritten CIGAR of more
 * than 65535 ops is written the way htslib's bam_write1 writes it: <l_seq>S<ref_len>N in the CIGAR
 * field, the ops in a CG:B,I tag behind the other tags (SAM spec 4.2.2); an input record in that form
 * is read from its tag and loses it, as after bam_read1 (the reference sees records only through
 * htslib, include/bramble.h:29-85).  BR_ERR_UNSUPPORTED only when such a CIGAR spans 2^28 reference
 * bases or more (bam_write1 fails there too). */
int br_bam_encode_device(br_ctx *, const br_config *, const br_device_records *, void *stream,
                         br_device_bam *out);

/* ---- BAM bundle entry: raw alignment records in, raw projected records out ---------------- */

/* Replaces the reader side of process_reads / process_read_in (src/bramble.cpp:313-441: start,
 * refid, XS/ts strand inputs via GSamRecord::tag_char1, gclib/GSam.cpp:310-318; process_pairs,
 * src/bramble.cpp:272-311; the name group's shared sequence, src/core.cpp:353-378), then
 * convert_reads and write_to_bam, for one bundle of raw BAM records that is resident in HBM:
 * every field is extracted from the records on the device.  Records must be mapped
 * (process_reads skips unmapped ones, bramble.cpp:376-379), name-collated, and the bundle must
 * end at a read-name boundary.  ref_map (HOST memory) maps the input header's refID to the
 * annotation's reference index (position in br_index_build's `refnames`), -1 or any id >= br_index_num_refs for names
 * the annotation lacks.  rows_out may be NULL. */
int br_project_bam_device(br_ctx *, const br_config *, const br_device_records *, const int32_t *ref_map,
                          int32_t n_ref_map, void *stream, br_device_rows *rows_out, br_device_bam *out);

/* Host-memory form of the same call (uploads the records, downloads the stream). */
typedef struct br_bam_bundle {
  const uint8_t *blob;      /* uncompressed BAM alignment section */
  uint64_t n_bytes;
  const uint64_t *rec_off;  /* n_records: offset of each record's refID word (just after its block_size) */
  const uint32_t *rec_len;  /* n_records: its block_size */
  int64_t n_records;
  const int32_t *ref_map;
  int32_t n_ref_map;
  int32_t bgzf_on_device;   /* 1: deflate the projected stream on the device; br_host_bam.data then holds complete
                             * BGZF blocks (append them to the output file as they are).  BR_OUT_SAM_TEXT: format it as
                             * SAM text on the device (br_sam_format_device); br_host_bam.data then holds the lines */
} br_bam_bundle;
#define BR_OUT_SAM_TEXT 2

typedef struct br_host_bam {
  const uint8_t *data;      /* [block_size][record]... ready for BGZF framing; owned by the context, valid until
                             * the SECOND next br_project_bam_bundle call (two pinned buffers alternate, so a
                             * writer thread can compress bundle k while bundle k+1 is projected) */
  uint64_t n_bytes;
  int64_t n_rows;
  uint64_t total_complete, total_unique, dropped_reads, total_processed;
} br_host_bam;

int br_project_bam_bundle(br_ctx *, const br_config *, const br_bam_bundle *, br_host_bam *out);

/* The same call in two steps, so that the upload of the next bundles (own copy stream; may be issued from another
 * host thread) overlaps the projection of the current one: stage bundle k into slot k % 3, later project it from that
 * slot.  A slot may be staged again once its br_project_bam_staged call has returned; the bundle's host memory must
 * stay valid until then. */
int br_bam_bundle_stage(br_ctx *, const br_bam_bundle *, int slot /* 0..2 */);
int br_project_bam_staged(br_ctx *, const br_config *, const br_bam_bundle *, int slot, br_host_bam *out);
/* br_project_bam_staged that does not wait for its result to arrive: with bgzf_on_device the counters, n_bytes and the
 * address in out->data are final when the call returns, the bytes behind it may still be crossing PCIe (on a stream of
 * their own, beside the next bundle's kernels).  br_host_bam_wait(ctx, out) -- from any one thread -- returns when they are
 * there; the buffer rule of the br_host_bam structure -- valid until the second next call -- is unchanged.  Without bgzf_on_device the call
 * is br_project_bam_staged. */
int br_project_bam_staged_nowait(br_ctx *, const br_config *, const br_bam_bundle *, int slot, br_host_bam *out);
int br_host_bam_wait(br_ctx *, const br_host_bam *);

/* br_bam_split on the device: `data` is an inflated BAM alignment section in HBM that starts at a record (n_bytes of it);
 * n_ref = the header's reference count (the boundary search tests reference ids against it).  recs->blob = data, rec_off /
 * rec_len = device arrays of the MAPPED records in stream order (owned by the context, valid until its next call),
 * *n_unmapped the records skipped, *consumed the first byte that belongs to no complete record.  Segments of the stream
 * guess their first record and a verification pass against the real chain makes the result exact (split_kernels.hip).
 * BR_ERR_INVALID_ARG on a record whose fixed fields overrun its block_size. */
int br_bam_split_device(br_ctx *, const uint8_t *data, uint64_t n_bytes, int32_t n_ref, void *stream, br_device_records *recs,
                        int64_t *n_unmapped, uint64_t *consumed);

/* A BAM reader on the device: BGZF bytes of the file in (host memory, e.g. the mapped file), bundles of device-resident records
 * of whole read-name groups out -- inflate, record split and the cut at a read-name change (src/bramble.cpp:313-441 reads
 * record by record through htslib and flushes a bundle at a name change) without the host touching an inflated byte.  Needs
 * no index: it can run beside the guide loading.
 *   br_bam_reader_new      header_bytes = inflated size of the BAM header (magic, text, references): the first record follows it
 *   br_bam_reader_next     takes the complete BGZF blocks at the front of data[0 .. n_bytes) (at most ~200 MB inflated per call;
 *                          *consumed says how far it got -- call again from there; `last` != 0: data ends with the file) and
 *                          returns the records of every read-name group that is complete: bundle->blob / rec_off / rec_len in
 *                          HBM (mapped records only, like br_bam_split; *n_unmapped = the ones skipped), valid until
 *                          br_bam_reader_release(id).  The last, possibly unfinished group stays behind for the next call;
 *                          the call that ends the file returns everything.  A bundle may be empty.
 * BR_ERR_INVALID_ARG for malformed BGZF / BAM, a block whose CRC32 is wrong, a file that ends inside a block or a record; a
 * reader that has returned an error is to be freed.  br_bam_reader_next is called from one thread; br_bam_reader_release may
 * come from another (the thread that projects the bundles). */
typedef struct br_bam_reader br_bam_reader;
int br_bam_reader_new(int device, int32_t n_ref, uint64_t header_bytes, br_bam_reader **out);
int br_bam_reader_next(br_bam_reader *, const uint8_t *data, uint64_t n_bytes, int last, uint64_t *consumed,
                       br_device_records *bundle, int64_t *id, int64_t *n_unmapped);
int br_bam_reader_set_piece_blocks(br_bam_reader *, int64_t blocks);   /* BGZF blocks per br_bam_reader_next call (default 3072) */
int br_bam_reader_release(br_bam_reader *, int64_t id);
/* Piece-wise form (round 4: several readers on several devices, uploads beside the inflating of the piece before).  The caller
 * holds the whole file's block table (br_bgzf_scan over the mapping) and hands out pieces [b0, b1) of it, to one reader in
 * order or to several readers: a piece needs nothing from its neighbours.  A piece owns the records between two cuts that
 * are defined the same way at either end (the read-name group that straddles a piece boundary goes to the piece in front,
 * which inflates blocks up to b1x > b1 to find its end); a piece that does not know where a record starts in its first
 * block (start_rel = -1) guesses, and reports where it started: when that differs from the end_rel its neighbour in front
 * reports, the caller processes the piece again with start_rel = that end_rel (the result never depends on a guess).
 *   br_bam_piece_upload    compressed bytes of blocks [b0, b1x) into upload slot 0 / 1 (its own stream; may be called from a
 *                          second thread, one piece ahead of br_bam_piece_process)
 *   br_bam_piece_process   inflate + record split + cuts of the slot's piece [b0, b1) -> bundle (valid until
 *                          br_bam_reader_release(id)) and info.  start_rel >= 0: inflated bytes from the start of block b0 to
 *                          the piece's first record (the BAM header's size for the first piece).  Returns 1 (BR_PIECE_MORE)
 *                          when the end cut lies beyond block b1x: upload up to a larger b1x and call again. */
#define BR_PIECE_MORE 1
/* one BGZF block: its deflate payload in the file, where its bytes go in the inflated stream (br_bgzf_scan) */
typedef struct br_bgzf_block { uint64_t src_off, dst_off; uint32_t clen, ulen, crc, pad; } br_bgzf_block;
typedef struct br_piece_info {
  uint64_t start_rel;   /* where the bundle starts: inflated bytes behind the start of block b0 */
  uint64_t end_rel;     /* where it ends: inflated bytes behind the start of block b1 (= the next piece's start_rel) */
  int64_t n_unmapped;   /* unmapped records between the two (not in the bundle) */
  int32_t guessed, at_end;
} br_piece_info;
int br_bam_piece_upload(br_bam_reader *, int slot, const uint8_t *file, uint64_t file_bytes, const br_bgzf_block *blocks,
                        int64_t n_blocks, int64_t b0, int64_t b1x);
int br_bam_piece_process(br_bam_reader *, int slot, const br_bgzf_block *blocks, int64_t n_blocks, int64_t b1, int64_t start_rel,
                         br_device_records *bundle, int64_t *id, br_piece_info *info);
double br_bam_reader_seconds(const br_bam_reader *);   /* time spent inside br_bam_piece_process so far */
double br_bam_reader_upload_seconds(const br_bam_reader *);   /* ... inside br_bam_piece_upload (host copies into pinned buffers + queueing) */
void br_bam_reader_free(br_bam_reader *);

/* ---- SAM text input (sam_reader.cpp, sam_kernels.hip) ------------------------------------------------------------------
 * The reference reads SAM like BAM, through htslib (GSamReader -> hts_open, gclib/GSam.h:371): every line becomes the bam1_t
 * sam_parse1 builds.  A SAM reader turns SAM record lines into BAM records on the device, laid out as br_bam_split_device lays
 * them out, so its bundles feed br_project_bam_resident unchanged and the records are byte for byte what `samtools view -b`
 * writes for the same lines (bam_write1: no extra NULs after the read name, the CG:B,I form for more than 65535 CIGAR ops).
 *   br_sam_header_scan   host only: the length of the leading '@' lines of data[0, n) (the last one may lack its '\n')
 *   br_sam_reader_new    header_text = the '@' lines; the references are its @SQ lines' SN: names, in order.  The names go to
 *                        a device hash table, built once per reader
 *   br_sam_reader_next   text = SAM record lines in HOST memory (copied to the device through two pinned slots on the reader's
 *                        own stream).  *consumed = up to the start of the last read-name group's first mapped line
 *                        (everything when last != 0, where a final line without '\n' is accepted); 0 when the text holds no
 *                        complete group -- call again with more bytes.  bundle as br_bam_reader_next (mapped records in HBM,
 *                        valid until br_sam_reader_release(id)); *n_unmapped = the lines in front of the cut that are unmapped
 *                        (flag 0x4, an RNAME without an @SQ line, no query-consuming CIGAR op).  BR_ERR_INVALID_ARG for a
 *                        malformed line: *bad_line = its 1-based number counted from the reader's first line,
 *                        br_sam_reader_error says what is wrong with it.  At most 1 GiB of text is taken per call.
 * br_sam_reader_next is called from one thread; br_sam_reader_release may come from another. */
typedef struct br_sam_reader br_sam_reader;
int br_sam_header_scan(const uint8_t *data, uint64_t n, uint64_t *header_bytes);
int br_sam_reader_new(int device, const char *header_text, uint64_t header_len, br_sam_reader **out);
int br_sam_reader_next(br_sam_reader *, const uint8_t *text, uint64_t n_bytes, int last, uint64_t *consumed,
                       br_device_records *bundle, int64_t *id, int64_t *n_unmapped, int64_t *bad_line);
/* The same call in two steps, so that the upload of chunk k+1 overlaps the parse of chunk k (two device text slots; the upload
 * runs on a copy stream of its own and may be called from another thread, one chunk ahead): br_sam_reader_upload puts text
 * into slot 0 / 1 and returns when it is on the device; br_sam_reader_next_staged parses the slot (text must be the same host
 * bytes: the float fallback reads them).  A slot may be uploaded again once its br_sam_reader_next_staged call has returned.
 * br_sam_reader_next is upload + next_staged on slot 0. */
int br_sam_reader_upload(br_sam_reader *, int slot, const uint8_t *text, uint64_t n_bytes);
int br_sam_reader_next_staged(br_sam_reader *, int slot, const uint8_t *text, uint64_t n_bytes, int last, uint64_t *consumed,
                              br_device_records *bundle, int64_t *id, int64_t *n_unmapped, int64_t *bad_line);
int br_sam_reader_release(br_sam_reader *, int64_t id);
void br_sam_reader_free(br_sam_reader *);
const char *br_sam_reader_error(const br_sam_reader *);   /* the reason of the last BR_ERR_INVALID_ARG ("" otherwise) */
/* so far: device time of the text uploads and of the parse (line index through emit), calls, text bytes and lines consumed
 * (any pointer may be NULL) */
int br_sam_reader_stats(const br_sam_reader *, double *upload_seconds, double *parse_seconds, int64_t *chunks, uint64_t *bytes,
                        int64_t *lines);

/* A collator: the mapped records of a whole input, in any order, in one device's HBM; bundles of whole read-name groups out,
 * for br_project_bam_resident.  Its output is C(input): groups in the order of their first record, records in input order
 * inside a group (a stable grouping: an input that is collated already comes out unchanged).  A name is l_read_name and the
 * read_name bytes, compared byte for byte.
 *   br_collator_new        BR_ERR_NO_DEVICE without the device
 *   br_collator_add        copies the records (device memory with on_device != 0, after the work queued on `stream`, which may
 *                          be NULL for the null stream; host memory with on_device = 0) into the collator's arena, [block_size][record] each (the 4
 *                          bytes in front of rec_off[i] are the block_size); returns when the copy is done, so the caller may
 *                          reuse the records.  BR_ERR_CAPACITY when the arena would exceed "max_bytes" or the device's memory
 *                          (the collator may still be freed), BR_ERR_INVALID_ARG after finish
 *   br_collator_finish     key, radix sort, collisions, placement (collate_kernels.hip); the counts of records and groups
 *   br_collator_next       the next bundle: whole groups, max_records or more up to the first group start at or behind that
 *                          (a group larger than max_records alone); n_aln = 0 at the end.  blob is the arena and rec_off / rec_len
 *                          point into it (the offsets are not monotone); valid until br_collator_free
 *   br_collator_order      host: the input index (position among the added records) of every output record
 *   br_collator_set_param  before the first add: "max_bytes" (arena cap, 0 = none), "hash_bits" (test hook: 0..64 bits of the
 *                          name hash are kept, so that different names collide; the result does not change)
 *   br_collator_stats      arena bytes, the most device memory the collator has held, seconds in add and in finish
 * The arena grows by allocating a larger buffer and copying.  Per record the collator holds the arena's 4 + block_size bytes
 * and 12 bytes of tables while adding, 64 bytes during finish, 24 afterwards (collate.cpp). */
typedef struct br_collator br_collator;
int br_collator_new(int device, br_collator **out);
int br_collator_add(br_collator *, const br_device_records *recs, int on_device, void *stream);
int br_collator_finish(br_collator *, int64_t *n_records, int64_t *n_groups);
int br_collator_next(br_collator *, int64_t max_records, br_device_records *bundle);
int br_collator_order(const br_collator *, int64_t *order);
int br_collator_set_param(br_collator *, const char *name, int64_t value);
int br_collator_stats(const br_collator *, uint64_t *arena_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds);
void br_collator_free(br_collator *);

/* A sorter: the projected records of a whole run in one device's HBM, handed out in coordinate order, and the BAI index of that
 * order (sort.cpp, sort_kernels.hip).  The order is defined here, modelled on `samtools sort` (equality with it is not tested:
 * the test machines have no samtools): records are ordered by the 64-bit key
 *     (uint32)refID << 32 | (uint32)(pos + 1) << 1 | ((flag >> 4) & 1)
 * so a refID of -1 sorts last and, at one position, the forward strand comes before the reverse one; equal keys keep the order
 * in which they were added (a stable sort: an input that is sorted already comes out unchanged).
 *   br_sorter_new        BR_ERR_NO_DEVICE without the device
 *   br_sorter_add        copies the rows of `recs` ([block_size][record] each, row i = data[row_off[i] .. row_off[i + 1]), the rows
 *                        contiguous) into the sorter's arena: device memory with on_device != 0, after the work queued on
 *                        `stream` (NULL: the null stream), host memory (data and row_off) with on_device = 0.  Returns when the
 *                        copy is done.  BR_ERR_CAPACITY when the arena would exceed "max_bytes" or the device's memory (the
 *                        sorter may still be freed) or the records would number more than 2^32 - 1 (32-bit radix indices),
 *                        BR_ERR_INVALID_ARG after finish, or for a device row_off that descends somewhere (nothing is added;
 *                        a host row_off is checked the same way)
 *   br_sorter_finish     keys and the radix sort; the number of records.  BR_ERR_INVALID_ARG when a record's pos is below -1 or
 *                        2^31 - 1 (no BAM position: pos + 1 has to fit the key's 31 bits); the sorter is then to be freed
 *   br_sorter_next       the next run of whole records in sorted order, gathered into one contiguous buffer with its row_off:
 *                        at most max_bytes, or one record when that record alone is larger; n_rows = 0 at the end.  The buffer
 *                        is valid until the SECOND next call (two alternate, as the deflate's do)
 *   br_sorter_order      host: the add-order index of every output record
 *   br_sorter_set_param  before the first add: "max_bytes" (arena cap, 0 = none)
 *   br_sorter_stats      arena bytes, the most device memory the sorter has held, seconds in add, finish and next
 * Per record the sorter holds the arena's 4 + block_size bytes and 8 bytes of tables while adding, 44 bytes during finish, 32
 * afterwards (sort.cpp).
 *
 * br_sorter_index builds the BAI file (SAM specification 5.2) of the sorted records on the device, after finish.  `blocks` lists
 * the BGZF blocks that hold the sorted record stream, in file order: coffset = where the block starts in the file, uoffset =
 * which byte of the sorted, uncompressed record stream is its first (blocks[0].uoffset = 0); eof_coffset = where the EOF block
 * starts.  *bai is a host buffer for br_free_buffer.  The content:
 *   virtual offsets  begin of record r = coffset(block holding the first byte of its block_size) << 16 | offset inside that
 *                    block; its end = the begin of record r + 1, eof_coffset << 16 for the last record
 *   bins             reg2bin(pos, end), end = pos + the reference length of the CIGAR field (M D N = X; the spilled
 *                    <l_seq>S<ref_len>N form needs no special case), pos + 1 when that is 0.  A record with refID < 0 or pos < 0 is
 *                    in no bin and counts in n_no_coor; one with end > 2^29 fails the call with BR_ERR_UNSUPPORTED
 *   per reference    its bins in ascending bin number; inside a bin, consecutive records of the file that share the bin are one
 *                    chunk (begin of the first, end of the last) and nothing else is merged (small bins are not folded into their
 *                    parents, as samtools index does: the file is valid for every BAI reader, not byte-identical to samtools');
 *                    pseudo-bin 37450 last, with (begin of the reference's first record, end of its last) and (n_mapped,
 *                    n_unmapped by flag 0x4); a reference without records has n_bin = 0 and n_intv = 0
 *   linear index     n_intv = 1 + max (end - 1) >> 14; ioffset[w] = the smallest begin among the records that overlap window w,
 *                    an empty window takes the value of the next one (filled from the right)
 *   tail             n_no_coor, always
 * BR_ERR_INVALID_ARG for a refID >= n_ref or a block table that does not cover the stream in blocks of less than 64 KiB. */
typedef struct br_sorter br_sorter;
typedef struct br_bgzf_span { uint64_t coffset, uoffset; } br_bgzf_span;
int br_sorter_new(int device, br_sorter **out);
int br_sorter_set_param(br_sorter *, const char *name, int64_t value);
int br_sorter_add(br_sorter *, const br_device_bam *recs, int on_device, void *stream);
int br_sorter_finish(br_sorter *, int64_t *n_records);
int br_sorter_next(br_sorter *, uint64_t max_bytes, br_device_bam *piece);
int br_sorter_order(const br_sorter *, int64_t *order);
int br_sorter_stats(const br_sorter *, uint64_t *arena_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds,
                    double *next_seconds);
int br_sorter_index(br_sorter *, int32_t n_ref, const br_bgzf_span *blocks, int64_t n_blocks, uint64_t eof_coffset, uint8_t **bai,
                    uint64_t *n_bytes);
void br_sorter_free(br_sorter *);

/* A quantifier: the read names of a whole run reduced to equivalence classes in one device's HBM, and per-transcript abundances
 * estimated from them by EM (quant.cpp, quant_kernels.hip).  The definitions:
 *   read name      a read-name group of a projected batch.  Its rows are row_off[group_off[g]] .. row_off[group_off[g + 1]]; its
 *                  transcript set is the ascending list of the distinct transcript_id of those rows.  Both mates count: a pair
 *                  emitted on two different transcripts (mate_case 2 of process_mate_pair) contributes both.  A name without rows
 *                  makes no class and counts in n_unassigned
 *   class          a distinct transcript set; its count is the number of read names that have that set.  Classes are ordered by
 *                  the add-order index of their first read name, the labels ascend inside a class.  How the adds were cut into
 *                  calls does not change the result
 *   per transcript unique[t] = names whose class is {t}; ambig[t] = names whose class holds t and has two labels or more
 *   EM             w[t] = 1 / len[t] with length normalisation, else 1; theta = 1 for every transcript at the start.  One
 *                  iteration: d_c = sum over t in c of theta_t w_t, then theta'_t = theta_t w_t * sum over the classes c that hold
 *                  t of n_c / d_c (a class with d_c == 0 contributes nothing).  After every iteration whose number is a multiple
 *                  of 16, and after the last one, the relative change is the maximum over t with theta'_t > 1e-8 of
 *                  |theta'_t - theta_t| / theta'_t; the run stops when that is < tolerance, or at max_iters (tolerance = 0 runs
 *                  exactly max_iters iterations).  Defaults: max_iters 10000, tolerance 1e-2 (salmon's minAlpha /
 *                  relDiffTolerance convention).  TPM_t = 1e6 theta_t w_t / sum of theta w.  Not modelled: sequence or position
 *                  bias
 *   bootstrap      ("bootstraps" = B > 0.)  C classes with counts n_c in class order, N = sum of n_c (the names with labels; N <
 *                  2^32), cum = the exclusive prefix sums of n_c.  Random numbers: Philox4x32-10 (multipliers 0xD2511F53 /
 *                  0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds) under the key ("boot_seed" low 32 bits, high 32
 *                  bits); the counter of draw i of replicate b is (i & 0xffffffff, i >> 32, b, 0), its output words w0 .. w3, and u =
 *                  w0 | w1 << 32.  Replicate b makes N draws, i = 0 .. N - 1; draw i picks the name rank r = floor(u N / 2^64) (the
 *                  high half of the 64 x 64 product), which lands in the class c with cum[c] <= r < cum[c + 1]; n_c^(b) (uint32) is
 *                  the number of draws that land in c.  N = 0: all counts and all results are 0
 *   replicate EM   the EM above with n_c^(b) in place of n_c: the same w (eff's with "eff_len"), the same start, the same sums in
 *                  the same order, and the same stopping rule for every replicate by its own relative change.  A replicate that has
 *                  stopped keeps the theta of its stopping iteration whatever the replicates that run beside it go on to do, so
 *                  replicate b's theta has the bits a point EM on n_c^(b) would have, however the replicates are cut into chunks
 *   summary        per transcript, float64, no fused multiply-add: mean_t = (theta_t^(0) + ... + theta_t^(B-1)) / B and var_t = (sum
 *                  over b of (theta_t^(b) - mean_t)^2) / (B - 1), both sums in replicate order, one division each; var = 0 for B = 1
 *   gene map       (br_quant_genes.)  tx_gene[t] < n_genes for every transcript, 0 <= n_genes < 2^32.  A gene that owns no
 *                  transcript is allowed: all its results are 0 and n_transcripts[g] = 0
 *   gene class     the gene set of a class is the ascending list of the distinct tx_gene[label] of its labels; the gene classes
 *                  are the distinct gene sets.  A gene class's count is the sum of the counts of the classes that have that set,
 *                  its first_name the smallest of their first_name; gene classes are ordered by first_name, the labels ascend
 *                  inside one.  That is exactly what br_quant_finish would have produced had every row's transcript_id been
 *                  replaced by its gene before the adds
 *   per gene       unique[g] = names whose gene class is {g}; ambig[g] = names whose gene class holds g and has two labels or
 *                  more; n_transcripts[g] = the number of transcripts of g
 *   gene abundance (after br_quant_em.)  float64, no fused multiply-add, no floating-point atomics; every sum runs sequentially
 *                  over the gene's transcripts in ascending transcript order, whatever their number (no wave tree: the bits do not
 *                  depend on a width).  num_reads[g] = sum of theta_t; tpm[g] = sum of tpm_t, the values br_quant_result returns;
 *                  length[g] = (sum of tpm_t * (double)L_t) / tpm[g] when tpm[g] > 0, each product rounded, then added, else (sum
 *                  of (double)L_t) / (double)n_transcripts[g], and 0 for a gene without transcripts or a quantifier without
 *                  lengths; eff_length[g] the same with eff_t in place of L_t ("eff_len" on)
 *   gene bootstrap (after br_quant_bootstrap.)  num_reads^(b)[g] = sum of theta_t^(b) in the same order; mean and var as `summary`
 *                  above defines them, over these gene values
 *   fragment       ("eff_len" = 1; salmon's and kallisto's truncated-mean effective length.)  A row r with BR_ROW_PAIRED |
 *                  BR_ROW_SAME_TX | BR_ROW_FIRST all set, together with row r + 1, which must lie inside the same read name's rows,
 *                  have BR_ROW_PAIRED set and BR_ROW_FIRST clear, and carry the same transcript_id.  A row that fails any of these
 *                  is not a fragment; nothing outside the name's rows is read.  reflen(row) = the sum of the lengths of the row's
 *                  rewritten CIGAR ops that consume the reference (M D N = X: op codes 0, 2, 3, 7, 8), taken from cigar[row] itself
 *                  when BR_ROW_NCIGAR(meta) <= 2, else from pool[cigar[row] ...].  The fragment's length is
 *                  max(pos_r + reflen_r, pos_r+1 + reflen_r+1) - min(pos_r, pos_r+1), in 64-bit arithmetic
 *   observation    only read names whose transcript set has exactly one label contribute, each at most one observation: its
 *                  fragment of lowest row index.  Such a name without a fragment counts in n_no_fragment; a length of 0 or above
 *                  "fld_max" counts in n_out_of_range and not in the histogram.  hist[f], f = 0 .. fld_max, is the number of
 *                  observations of length f (uint64) and n_obs their sum.  How the adds were cut into calls changes nothing
 *   eff. length    C(x) = sum over f <= x of hist[f], S(x) = sum over f <= x of f hist[f], both uint64.  For a transcript of length
 *                  L > 0 and x = min(L, fld_max): eff = (double)L when C(x) == 0 (no pairs at all, long reads, a transcript shorter
 *                  than every observed fragment), else eff = (double)((L + 1) C(x) - S(x)) / (double)C(x), one correctly rounded
 *                  division of two exact integers: L - E[f | f <= L] + 1, always >= 1, the same bits on every machine.  L <= 0
 *                  gives eff = 0.  With "eff_len" on the EM's w[t] = 1 / eff[t], and 0 where eff is 0; everything else is unchanged
 *   numerics       float64 throughout, no floating-point atomics: a class's sum runs over its labels in ascending order, a
 *                  transcript's over its classes in ascending order through a transposed membership table; items of more than 64
 *                  entries are summed by a wave (lane l takes entries l, l + 64, ..., then a fixed tree), so the shape of every sum
 *                  depends on the data alone and two runs on the same input give the same bits
 *   posterior      (br_quant_posteriors, after br_quant_em.)  For label entry e of class c with transcript t: x_t = theta_t * w_t,
 *                  with the theta br_quant_result returns and the w the EM used (1 / eff with "eff_len"); d_c = the sum of x over the
 *                  class's labels in ascending order, one after the other whatever their number (no wave tree); p[e] = x_t / d_c,
 *                  and 0 where d_c == 0.  float64, no fused multiply-add, one rounding per operation: a restatement in the same
 *                  order gives the same bits.  A class of one label has p = 1.0
 *   variational    ("vb" = 1; salmon's default estimator, the variational Bayes EM with a Dirichlet prior.  With "vb" = 0, the
 *                  default, nothing below applies and every result has the bits it had.)  The prior is br_quant_set_vb_prior's,
 *                  finite and >= 0, default 1e-2 (salmon's --vbPrior).  Per transcript p_t = prior; with "vb_per_nucleotide" = 1
 *                  p_t = prior * eff_t when "eff_len" is on, else prior * (double)L_t, and 0 where L_t <= 0.  The state is alpha
 *                  in theta's place: alpha_t = 1 at the start, and the theta br_quant_result returns is the final alpha, without
 *                  the prior (NumReads).  One iteration: A_t = alpha_t + p_t; S = the sum of A_t over all transcripts; e_t =
 *                  exp(psi(A_t) - psi(S)) when A_t > 1e-10 (salmon's digammaMin), else 0; x_t = e_t * w_t with the EM's w; d_c =
 *                  the sum of x_t over the class's labels; alpha'_t = x_t * the sum over the classes that hold t of n_c / d_c (a
 *                  class with d_c == 0 contributes nothing).  Stopping: the EM's rule, unchanged, on alpha.  TPM_t = 1e6 alpha_t
 *                  w_t / sum of alpha w.  The posteriors after a variational run take this x_t, made from the final alpha, in
 *                  place of theta_t w_t; br_coverage_finish_em reads them unchanged.  The replicate EM is this iteration with
 *                  n_c^(b), every replicate with its own S and its own stopping, frozen as `replicate EM` says.  Gene values are
 *                  sums of transcript values as before
 *   psi            (digamma, for a positive argument.)  psi(a) = psi(a + 1) - 1 / a until the argument is 16 or more (the
 *                  threshold is 16; the series then needs no 1 / a^12 term), then ln a - 1/(2a) - 1/(12a^2) + 1/(120a^4) -
 *                  1/(252a^6) + 1/(240a^8) - 1/(132a^10).  Against a float64 library digamma the restatement of this series is
 *                  within 1.4e-15 of max(1, |psi|) over [1e-10, 1e9]
 *   vb numerics    float64, no fused multiply-add, no floating-point atomics.  S is summed in a shape that depends on
 *                  n_transcripts alone: the A_t of transcripts 256 b .. 256 b + 255 make partial b (a xor tree over each 64, the
 *                  four results added in order), thread i of one block adds partials i, i + 256, ... in ascending order and the
 *                  same block sum closes it -- in the point run and, per replicate, in a chunk of any width.  So two runs give
 *                  the same bits and a replicate's bits do not depend on "boot_chunk".  Bit-equality with a CPU restatement
 *                  is not claimed for "vb" = 1: the device's log and exp are not libm's
 *   vb caveat      the iteration sits at an unstable fixed point for transcripts the data cannot tell apart (the same classes
 *                  with the same counts, the same w): rounding decides which of them takes the reads -- two transcripts with
 *                  mirrored classes of 154 / 154 / 2 names end at 1.52 / 1.52 reads under one summation order and at 0 / 3.45
 *                  under another.  The device's result is the same bits in every run, but no more meaningful there than
 *                  salmon's; the plain EM keeps such transcripts equal
 *   name classes   ("keep_names" = 1.)  name_cls[i] = the index, in the classes' order, of the class add-order name i fell into,
 *                  0xffffffff for a name without rows; at any "hash_bits"
 *   br_quant_new        lengths: n_transcripts transcript lengths, or NULL (then "length_norm" must be 0).  BR_ERR_NO_DEVICE
 *                       without the device
 *   br_quant_set_param  before finish: "hash_bits" (test hook: 1..64 bits of the label hash are kept, so that different sets
 *                       collide; the result does not change), "length_norm" 0 / 1 (default 1), "max_iters", "tolerance_ppm"
 *                       (tolerance in millionths; br_quant_set_tolerance takes the double itself); before the first add only, a
 *                       refused one with "eff_len" on included (the histogram is sized by then):
 *                       "eff_len" 0 / 1 (default 0: the fragment-length model above), "fld_max" 1 .. 65535 (default 1000, salmon's
 *                       fragLenDistMax), "keep_names" 0 / 1 (default 0: finish leaves every name's class on the device); before
 *                       finish, as "max_iters": "vb" 0 / 1 (default 0) and "vb_per_nucleotide" 0 / 1 (default 0), see `variational`
 *   br_quant_set_vb_prior  the prior of `variational`, before finish; BR_ERR_INVALID_ARG for a negative or non-finite one
 *   br_quant_add        the read names group_off[0 .. n_groups] of a batch: a / row_off / group_off as br_device_rows and
 *                       br_device_batch hold them (device memory with on_device != 0, read after the work queued on `stream`, NULL
 *                       for the null stream; host memory with on_device = 0).  Returns when the tables have been read.
 *                       BR_ERR_INVALID_ARG after finish, or for offsets that descend (nothing is added); BR_ERR_CAPACITY when the
 *                       device's memory does not take it or the names would number 2^32 or more; BR_ERR_INVALID_ARG with
 *                       "eff_len" on (the fragments need the CIGARs)
 *   br_quant_add_rows   br_quant_add with the whole row table: a, cigar, pool and row_off of `rows` (n_rows and n_pool_words size the
 *                       copies of a host table; on_device = 0 takes the same layout in host memory).  With "eff_len" off it is
 *                       br_quant_add and reads nothing else; with it on the add also counts the fragments.  BR_ERR_INVALID_ARG, and
 *                       nothing added, also for rows past n_rows or a pooled CIGAR reference (of a fragment) that leaves n_pool_words
 *   br_quant_add_last   br_quant_add_rows for the context's last projection call, whichever entry point made it
 *   br_quant_finish     the classes; the numbers of names added and of classes.  BR_ERR_INVALID_ARG for a transcript_id >=
 *                       n_transcripts, or when lengths normalise and a transcript of length <= 0 (or no lengths at all) has a read
 *   br_quant_classes    host copies: label_off (n_classes + 1), labels (label_off[n_classes]), counts, first_name (the add-order
 *                       index of the class's first read name); any pointer may be NULL
 *   br_quant_em         the EM, after finish; the iterations run and the last relative change looked at.  BR_ERR_INVALID_ARG with
 *                       "eff_len" on and "length_norm" off, or without lengths; with "vb" and "vb_per_nucleotide" on and no lengths
 *   br_quant_fld        host copies, any may be NULL: hist ("fld_max" + 1 entries) and the three counters, of the adds so far
 *   br_quant_eff_lengths  eff, n_transcripts doubles; after finish, with "eff_len" on and lengths given
 *   br_quant_result     host copies, n_transcripts each, any may be NULL: theta and tpm (after em), unique and ambig (after finish)
 *   br_quant_stats      device bytes held now, the most held so far, seconds in add / finish / em, label sets met with equal
 *                       hashes and different contents, names without rows, labels over all classes (any pointer may be NULL)
 *   br_quant_set_param  (bootstrap) "bootstraps" 0 .. 10000 (default 0), "boot_seed" (the int64's bits are the seed, default 0),
 *                       "boot_chunk" (test hook: the replicates that run together, 1 .. 64; 0, the default, leaves it to the
 *                       library; the result does not depend on it): accepted, after finish as well, until br_quant_bootstrap has run
 *   br_quant_bootstrap  the B replicates, after finish, before or after br_quant_em, whose result it leaves alone; n_iters (B
 *                       entries, or NULL): the iterations of every replicate.  BR_ERR_INVALID_ARG before finish, with "bootstraps"
 *                       0 or where br_quant_em refuses; BR_ERR_CAPACITY when the B x T result or a chunk does not fit
 *   br_quant_boot_counts  count x n_classes resampled counts, replicate-major, of replicates first .. first + count - 1, generated
 *                       again (the generator is counter-based: nothing of size B x C is kept); after finish with "bootstraps" > 0
 *   br_quant_boot_theta   count x n_transcripts, replicate-major; after br_quant_bootstrap
 *   br_quant_boot_summary mean and var, n_transcripts each, either may be NULL; after br_quant_bootstrap
 *   br_quant_boot_stats   seconds resampling and in the replicates' EM, and the iterations of all replicates together
 *   br_quant_genes      the gene tables from the map (host memory, n_transcripts entries); the number of gene classes.  After finish,
 *                       once, before or after br_quant_em / br_quant_bootstrap, whose results it never changes.
 *                       BR_ERR_INVALID_ARG, and the object as it was, for a second call, a call before finish, a NULL map with
 *                       transcripts, an entry >= n_genes or an n_genes outside 0 .. 2^32 - 1 (the map is checked before anything
 *                       is made).  A run without named reads gives 0 classes and zero tables
 *   br_quant_gene_classes  br_quant_classes of the gene classes; after br_quant_genes; any pointer may be NULL
 *   br_quant_gene_result   host copies, n_genes each, any may be NULL.  BR_ERR_INVALID_ARG for num_reads / tpm / length /
 *                       eff_length before br_quant_em, and for eff_length without "eff_len"
 *   br_quant_gene_boot  count x n_genes, replicate-major, of replicates first .. first + count - 1; after br_quant_genes and
 *                       br_quant_bootstrap, BR_ERR_INVALID_ARG before
 *   br_quant_gene_boot_summary  mean and var, n_genes each, either may be NULL; after both as well
 *   br_quant_gene_stats seconds in br_quant_genes, labels over all gene classes, gene sets met with equal hashes and different
 *                       contents (any pointer may be NULL)
 *   br_quant_name_classes  a host copy of name_cls[first .. first + n); after finish, BR_ERR_INVALID_ARG without "keep_names" or
 *                       outside [0, n_names]
 *   br_quant_posteriors the n_labels posteriors, parallel to the labels of br_quant_classes; after br_quant_em.  post may be NULL: the
 *                       table is then only made and held on the device (br_coverage_finish_em reads it there).  A later br_quant_em
 *                       drops it
 *   br_quant_digamma    test hook: out[i] = the device's psi(a[i]) for n numbers in host memory (NaN where a[i] is not positive
 *                       and finite); BR_ERR_NO_DEVICE without the device
 * Device memory: 4 bytes a row and 20 bytes a read name while adding; finish peaks at 32 more a name with labels, then holds 24
 * bytes a class, 8 a label and 24 a transcript; the EM adds 40 a transcript and 8 a class; "eff_len" adds 16 (fld_max + 4) for the
 * histogram (the run's and an add's own), 16 (fld_max + 1) for the prefixes during finish and 8 a transcript for eff; the bootstrap
 * holds 8 B a transcript (the result) and 8 a class (cum), and while it runs, for a chunk of W replicates (16 by default), 32 W a
 * transcript and 12 W a class, the summary 16 a transcript; br_quant_genes holds 24 bytes a gene class, 4 a gene label, 24 a gene and
 * 4 a transcript, peaks at 32 a label and 4 a transcript beside them, and the gene replicates add 8 B a gene; "keep_names" holds 4
 * bytes a name from finish on (and 4 a class more while the classes are made), the posteriors 8 a label; "vb" holds 8 a transcript more (p) and
 * 8 bytes per 256 transcripts for the partials of S, times W while a chunk runs (quant.cpp). */
typedef struct br_quant br_quant;
int br_quant_new(int device, int64_t n_transcripts, const int64_t *lengths, br_quant **out);
int br_quant_set_param(br_quant *, const char *name, int64_t value);
int br_quant_set_tolerance(br_quant *, double tolerance);
int br_quant_set_vb_prior(br_quant *, double prior);
int br_quant_add(br_quant *, const br_row_a *a, const uint64_t *row_off, const uint32_t *group_off, int64_t n_groups, int on_device,
                 void *stream);
int br_quant_add_rows(br_quant *, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups, int on_device, void *stream);
int br_quant_add_last(br_quant *, br_ctx *);
int br_quant_finish(br_quant *, int64_t *n_names, int64_t *n_classes);
int br_quant_classes(br_quant *, uint64_t *label_off, uint32_t *labels, uint64_t *counts, uint64_t *first_name);
int br_quant_em(br_quant *, int32_t *n_iters, double *rel_change);
int br_quant_result(br_quant *, double *theta, double *tpm, uint64_t *unique, uint64_t *ambig);
int br_quant_fld(br_quant *, uint64_t *hist, uint64_t *n_obs, uint64_t *n_no_fragment, uint64_t *n_out_of_range);
int br_quant_eff_lengths(br_quant *, double *eff);
int br_quant_stats(const br_quant *, uint64_t *held_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds,
                   double *em_seconds, uint64_t *collisions, int64_t *n_unassigned, int64_t *n_labels);
int br_quant_bootstrap(br_quant *, int32_t *n_iters);
int br_quant_boot_counts(br_quant *, int32_t first, int32_t count, uint32_t *counts);
int br_quant_boot_theta(br_quant *, int32_t first, int32_t count, double *theta);
int br_quant_boot_summary(br_quant *, double *mean, double *var);
int br_quant_boot_stats(const br_quant *, double *sample_seconds, double *em_seconds, int64_t *iterations_total);
int br_quant_genes(br_quant *, const uint32_t *tx_gene, int64_t n_genes, int64_t *n_gene_classes);
int br_quant_gene_classes(br_quant *, uint64_t *label_off, uint32_t *labels, uint64_t *counts, uint64_t *first_name);
int br_quant_gene_result(br_quant *, double *num_reads, double *tpm, double *length, double *eff_length, uint64_t *unique,
                         uint64_t *ambig, uint32_t *n_transcripts);
int br_quant_gene_boot(br_quant *, int32_t first, int32_t count, double *num_reads);   /* count x n_genes, replicate-major */
int br_quant_gene_boot_summary(br_quant *, double *mean, double *var);
int br_quant_gene_stats(const br_quant *, double *seconds, int64_t *n_gene_labels, uint64_t *collisions);
int br_quant_name_classes(br_quant *, int64_t first, int64_t n, uint32_t *cls);
int br_quant_posteriors(br_quant *, double *post);
int br_quant_digamma(int device, const double *a, int64_t n, double *out);
void br_quant_free(br_quant *);

/* Coverage: the depth of coverage along every transcript, from the rows of a whole run, in one device's HBM (coverage.cpp,
 * coverage_kernels.hip).  Integers throughout.  The definitions:
 *   transcriptome  n_transcripts lengths L[t]; transcript t owns max(L[t], 0) bases, B is their sum
 *   counted row    every row of every add; with "primary_only" = 1 only the rows with BR_ROW_PRIMARY set, the others count in
 *                  rows_skipped.  Secondary records count by default (for a multi-mapped read the choice of the primary among its
 *                  transcripts is arbitrary, and so would the track be).  Both mates of a pair count, a base they both cover twice
 *                  (samtools depth without -s, bedtools genomecov).  Strand and NH are not looked at
 *   covered bases  the row's rewritten CIGAR is walked from p = pos in 64-bit arithmetic -- taken from cigar[row] itself when
 *                  BR_ROW_NCIGAR(meta) <= 2, else from pool[cigar[row] ...], as br_quant's fragments read it.  M = X (op codes 0, 7,
 *                  8) of length n cover [p, p + n) and advance p; D N (2, 3) advance p and cover nothing (samtools depth without
 *                  -J, genomecov -split); I S H P do nothing.  A covered interval is clamped to [0, L[t]); the bases it loses
 *                  count in clipped_bases (all of them on a transcript with L <= 0)
 *   depth          depth[t][x] = the counted rows that cover base x of t, uint32.  The rows of one object number fewer than 2^32:
 *                  the add that would reach 2^32 returns BR_ERR_CAPACITY and adds nothing, so the depth cannot overflow
 *   per transcript records[t] (uint64) = the counted rows with that transcript_id, however much of them was clipped;
 *                  aligned_bases[t] (uint64) = the sum of the depth; covered_bases[t] (uint64) = the bases of depth > 0;
 *                  max_depth[t] (uint32)
 *   run            a maximal interval [start, end) of one transcript with one depth > 0.  Runs never span two transcripts, whatever
 *                  the depths on both sides of the boundary; they are ordered by (transcript, start)
 *   invariance     how the rows were cut into adds, and their order, changes nothing; two runs give the same bits (integer atomics)
 *   weighted depth ("weight" = 1: nh, 2: em; 0, the default, is everything above and nothing below.)  Fixed point: one unit of depth
 *                  is 2^32 and a depth word is uint64.  A counted row with weight word q leaves + q at the first base of each clamped
 *                  covered interval and - q (mod 2^64) behind its last; the depth is the inclusive scan modulo 2^64.  Rows per
 *                  object stay below 2^32 and q <= 2^32, so no depth overflows.  Which rows count, how intervals are formed,
 *                  merged and clamped, and clipped_bases are exactly as above
 *   weight nh      q = (2^32 + nh / 2) / nh in integer arithmetic, nh the row's br_row_a.nh >= 1.  A row with nh == 0 is skipped and
 *                  counts in rows_skipped; br_coverage_finish then returns BR_ERR_INVALID_ARG
 *   weight em      q = (uint64) rint(p * 4294967296.0), ties to even, p the posterior (br_quant, `posterior`) of (the row's read
 *                  name, the row's transcript): the entry of the row's transcript among the labels of the class the name fell
 *                  into.  A name of a one-label class has q = 2^32 exactly (33 bits: why the depth is 64-bit).  A row with q == 0
 *                  is still a counted record.  NH is not looked at
 *   per transcript (weighted) records[t] = the counted rows (uint64, unweighted); weight_sum[t] = the sum of their q; aligned_hi[t] =
 *                  the sum over the bases of depth >> 32 and aligned_lo[t] = the sum of depth & 0xffffffff (one 64-bit sum of
 *                  fixed-point depths can overflow, these two cannot); covered_bases[t] = the bases of depth > 0; max_depth[t]; all
 *                  uint64
 *   run            (weighted) as above with the fixed-point depth: depths one unit of 2^-32 apart are different runs
 *   br_coverage_new        BR_ERR_INVALID_ARG for a length above 2^32 - 1 (start and end are 32-bit), BR_ERR_NO_DEVICE without the
 *                          device, BR_ERR_CAPACITY when the device's memory does not take 4 (B + 1) bytes
 *   br_coverage_set_param  before the first add: "primary_only" 0 / 1 (default 0); "weight" 0 / 1 / 2 (default 0; diff is made again
 *                          at 8 bytes a base for 1 and 2; BR_ERR_CAPACITY for 2 with 2^40 bases or more)
 *   br_coverage_add_rows   the rows [r0, r1) of a table: a, cigar, pool, n_rows and n_pool_words of `rows` (device memory with
 *                          on_device != 0, read after the work queued on `stream`, NULL for the null stream; host memory in the
 *                          same layout with on_device = 0).  Returns when the tables have been read.  A row whose transcript_id is
 *                          >= n_transcripts is skipped and nothing outside the tables is touched; br_coverage_finish then returns
 *                          BR_ERR_INVALID_ARG.  A row range outside [0, n_rows] or a pooled CIGAR reference that leaves
 *                          n_pool_words makes the add return BR_ERR_INVALID_ARG, and from then on the object answers
 *                          BR_ERR_INVALID_ARG to everything except br_coverage_free: PART OF THAT ADD MAY ALREADY HAVE BEEN COUNTED.
 *                          BR_ERR_INVALID_ARG after finish
 *   br_coverage_add_last   br_coverage_add_rows for all rows of the context's last projection call, whichever entry point made it
 *                          (a call that left no rows: BR_OK)
 *   br_coverage_finish     depth, summary and runs; the number of runs
 *   br_coverage_runs       after finish: runs [first, first + n) as four host arrays (BR_ERR_INVALID_ARG outside [0, n_runs])
 *   br_coverage_depth      after finish: the max(L[tid], 0) depths of one transcript
 *   br_coverage_summary    after finish: n_transcripts entries each
 *   br_coverage_stats      rows counted / skipped and bases clipped by the adds so far, device bytes held now and the most held so
 *                          far, seconds in add / finish
 *   br_coverage_add_names  the rows of the read names group_off[0 .. n_groups] of a batch: the shapes and rules of br_quant_add_rows
 *                          (rows->row_off, n_rows and n_pool_words are read as well).  With "weight" 0 and 1 it is
 *                          br_coverage_add_rows over the names' row range.  With "weight" 2 the add keeps instead of counting: for
 *                          every clamped, non-empty interval of a counted row 16 bytes (the absolute first base, the length, the
 *                          add-order index of the name; a counted row without such an interval leaves one entry of length 0, so
 *                          that its weight reaches weight_sum); records and the counters are updated at the add.  Offsets that
 *                          descend (host tables), or a row that the offsets give to no name (device tables: every row's name
 *                          is checked against the offsets on both sides): BR_ERR_INVALID_ARG and nothing added.
 *                          BR_ERR_CAPACITY at 2^32 names
 *   br_coverage_add_rows   ("weight" 2) BR_ERR_INVALID_ARG: the rows have no names
 *   br_coverage_add_last   ("weight" 2) br_coverage_add_names of the context's last call (a call that left no names: BR_OK)
 *   br_coverage_finish     ("weight" 2) BR_ERR_INVALID_ARG: br_coverage_finish_em
 *   br_coverage_finish_em  "weight" 2 only: the kept entries are applied with the quantifier's posteriors, the arena is freed, then
 *                          depth, summary and runs.  It needs a quantifier on the same device, with "keep_names", after br_quant_em,
 *                          whose names number what this object's add_names were given -- the two were fed the same names in the same
 *                          order; else BR_ERR_INVALID_ARG and the object is as it was.  Every index the apply takes from a table is
 *                          compared with that table's size first: a name past the count, a class past the classes (a name without
 *                          rows among them) or a transcript that is not in the name's class is counted, never looked up, and makes
 *                          the call return BR_ERR_INVALID_ARG (the object answers BR_ERR_INVALID_ARG from then on)
 *   br_coverage_runs64 / _depth64 / _summary64  the getters of the weighted modes (depth words uint64; runs as three uint32 arrays and
 *                          the depth); they answer BR_ERR_INVALID_ARG with "weight" 0, br_coverage_runs / _depth / _summary with
 *                          "weight" 1 and 2.  br_coverage_stats is valid in every mode
 * Any out-pointer may be NULL.  Device memory in a weighted mode: 8 bytes a base and 24 a transcript from "weight" on, 128 bytes of
 * counters; weight em holds 16 bytes a kept entry until finish_em has applied them (room grows by half, the old arena beside the
 * new while copying) and 4 bytes a row of an add while it runs; finish adds 32 a transcript, 24 a run and 8 a tile while it runs
 * (coverage.cpp).  Device memory with "weight" 0: 4 bytes a base (diff, which finish turns into the depth in place) and 16 a transcript
 * from br_coverage_new on; finish adds 20 a transcript, 16 a run and, while it runs, 8 a tile of 4096 bases; a host add holds 24
 * bytes a row and 4 a pool word while it runs (coverage.cpp). */
typedef struct br_coverage br_coverage;
int br_coverage_new(int device, int64_t n_transcripts, const int64_t *lengths, br_coverage **out);
int br_coverage_set_param(br_coverage *, const char *name, int64_t value);
int br_coverage_add_rows(br_coverage *, const br_device_rows *rows, int64_t r0, int64_t r1, int on_device, void *stream);
int br_coverage_add_last(br_coverage *, br_ctx *);
int br_coverage_finish(br_coverage *, int64_t *n_runs);
int br_coverage_runs(br_coverage *, int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth);
int br_coverage_depth(br_coverage *, int64_t tid, uint32_t *depth);
int br_coverage_summary(br_coverage *, uint64_t *records, uint64_t *aligned_bases, uint64_t *covered_bases, uint32_t *max_depth);
int br_coverage_stats(const br_coverage *, uint64_t *rows_counted, uint64_t *rows_skipped, uint64_t *clipped_bases, uint64_t *held_bytes,
                      uint64_t *peak_bytes, double *add_seconds, double *finish_seconds);
/* the weighted modes ("weight" = 1, 2) */
int br_coverage_add_names(br_coverage *, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups, int on_device, void *stream);
int br_coverage_finish_em(br_coverage *, br_quant *, int64_t *n_runs);
int br_coverage_runs64(br_coverage *, int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint64_t *depth);
int br_coverage_depth64(br_coverage *, int64_t tid, uint64_t *depth);
int br_coverage_summary64(br_coverage *, uint64_t *records, uint64_t *weight_sum, uint64_t *aligned_hi, uint64_t *aligned_lo,
                          uint64_t *covered_bases, uint64_t *max_depth);
void br_coverage_free(br_coverage *);

/* The coverage as a bigWig (Kent et al. 2010; UCSC's bbiFile.h layout, version 4), built and compressed in the device's HBM from what
 * br_coverage_finish / _finish_em left there (bigwig.cpp, bigwig_kernels.hip; the host's pieces: host/bigwig_file.cpp).  Little-endian.
 * The file, in order:
 *   header         64 bytes: u32 magic 0x888FFC26, u16 version 4, u16 zoomLevels, u64 chromosomeTreeOffset, fullDataOffset,
 *                  fullIndexOffset, u16 fieldCount 0, definedFieldCount 0, u64 autoSqlOffset 0, totalSummaryOffset, u32 uncompressBufSize,
 *                  u64 extensionOffset 0
 *   zoom headers   24 bytes a level: u32 reductionLevel, u32 0, u64 dataOffset, indexOffset
 *   total summary  40 bytes: u64 validCount, f64 minVal, maxVal, sumData, sumSquares
 *   chromosome tree  32 bytes (u32 magic 0x78CA8C91, blockSize, keySize, valSize 8, u64 itemCount, 0), then nodes: u8 isLeaf, u8 0, u16
 *                  count; leaf items key[keySize] (zero padded), u32 chromId, chromSize; inner items key (the first key below), u64 childOffset
 *   full data      u64 sectionCount, then the sections: before compression 24 bytes (u32 chromId, chromStart, chromEnd, itemStep 0,
 *                  itemSpan 0, u8 type 1 = bedGraph, u8 0, u16 itemCount) and 12 an item (u32 start, end, f32 value)
 *   full index     an R-tree: 48 bytes (u32 magic 0x2468ACE0, blockSize, u64 itemCount, u32 startChromIx, startBase, endChromIx, endBase, u64
 *                  endFileOffset = where the indexed data ends, u32 itemsPerSlot 1, u32 0), then nodes: u8 isLeaf, u8 0, u16 count; leaf
 *                  items 32 bytes (the four u32 bounds, u64 dataOffset, dataSize), inner items 24 (the bounds, u64 childOffset)
 *   per zoom level its data (u32 recordCount, then blocks of 32-byte records: u32 chromId, chromStart, chromEnd, validCount, f32 minVal,
 *                  maxVal, sumData, sumSquares) and its R-tree
 *   u32 magic again
 * Both kinds of tree are written from the root's level down, each level left to right; a level over n items has ceil(n / blockSize)
 * nodes of 4 + blockSize x item bytes, the unused tail zero; a tree of at most blockSize items (or of none) is one leaf; blockSize in a
 * tree's header is min(option, max(itemCount, 1)).  The definitions:
 *   chromosomes    the transcripts with at least one run, no others.  chromId = the rank of the name in bytewise (strcmp) order, which
 *                  is not @SQ order; chromSize = L[t]; keySize = the longest of these names.  Sections, zoom records and tree items are
 *                  ordered by (chromId, start)
 *   value          weight 0: (float) depth; weighted: (float) ((double) depth64 * 2^-32).  One item a run of br_coverage_runs, neighbours
 *                  whose values round to the same float included.  A float holds 24 bits: unit depths above 2^24 lose their low bits
 *   sections       a chromosome's runs in ceil(n / S) sections of S = items_per_slot runs, the last shorter; none spans two
 *                  chromosomes; chromStart / chromEnd: the first start and the last end
 *   zoom level k   R = first_reduction * 4^k.  For every chromosome and every aligned window [w R, min((w + 1) R, L)) with a base of
 *                  depth > 0 one record: validCount = those bases, minVal / maxVal = the values of the least and the greatest depth among
 *                  them, sumData / sumSquares = the sums of the value and of its square over them, summed in double from the depth array
 *                  in a fixed order (the same bits every run) and rounded to float.  Blocks of S consecutive records, across chromosomes
 *   total summary  the same five over all covered bases, in double (from the runs: value x length)
 *   R-tree bounds  a leaf item: (chromId, start) of its first and (chromId, end) of its last item; an inner item: the lexicographic
 *                  minimum and maximum of its children
 *   compression    every section and zoom block is a zlib stream of its own: 0x78 0x9C, one final fixed-Huffman block (RFC 1951 3.2.6)
 *                  from the greedy parse of the BGZF path, Adler-32 big-endian.  Where that block is not smaller than the payload:
 *                  stored (BTYPE 00), payload + 11 bytes (a payload above 65535 bytes -- zoom blocks of more than 2047 records --
 *                  takes a stored block per 65535 bytes, 5 bytes each).  uncompressBufSize = max(24 + 12 S, 32 S); uncompressed: 0.  The
 *                  compressed bytes are no part of the contract, what they decode to is
 *   br_coverage_bigwig        after finish, in every weight mode, any number of times: the image of an earlier call goes when the
 *                  arguments have been accepted.  names: n_transcripts C strings (those of transcripts without runs are not read).  opts
 *                  or NULL; a field that is 0 takes its default.  *n_bytes = the size of the file.  BR_ERR_INVALID_ARG, with nothing made
 *                  and an earlier image kept, before finish, for an option out of range (first_reduction * 4^k must stay below 2^31),
 *                  a NULL or empty name of a transcript with runs, two such transcripts of one name.  BR_ERR_CAPACITY for memory that is
 *                  not there, 2^32 records in a zoom level: no image is left
 *   br_coverage_bigwig_read   a host copy of the image's bytes [off, off + n); outside the image, or without one: BR_ERR_INVALID_ARG
 *   br_coverage_bigwig_stats  of the image: chromosomes, sections, zoom levels, records per level (10 entries), the bytes of all sections
 *                  and zoom blocks before and after compression, the size of the file, the seconds of the build
 *   br_zlib_sections_device   the codec alone: section i is src[off[i] .. off[i + 1]) in host memory, at most 131072 bytes (the public
 *                  file needs 16384 for its sections at the default S); *out (br_free_buffer) holds the streams back to back,
 *                  out_off[0 .. n] their bounds.  mode 0: the fixed code with the stored fallback; 1: stored
 * Device memory: the image, I bytes, is in br_coverage_stats' held bytes from the call's return until the next call or
 * br_coverage_free.  While the call runs every part of the file lies in a buffer of its own, beside them 28 bytes a chromosome, the
 * raw sections (24 a section, 12 a run) with 24 a section of offsets and bounds, compressed also their slots (9/8 of the raw bytes
 * and 32 a section) and 8 a section of sizes; a zoom level holds 40 bytes a window until its records are compacted, then 32 a record
 * and 24 a block; at the end the image beside its parts, so the peak is about 2 I above what finish left (bigwig.cpp). */
typedef struct br_bigwig_opts {   /* 0 in a field: its default */
  uint32_t items_per_slot;   /* S: runs per data section, zoom records per zoom block: default 1024, 1 .. 4096 */
  uint32_t block_size;       /* children per node of both kinds of tree: default 256, 2 .. 4096 */
  int32_t zoom_levels;       /* default 4; -1: none; at most 10 */
  uint32_t first_reduction;  /* bases per window at level 0: default 32 */
  int32_t compress;          /* default 1: zlib sections; -1: uncompressed */
} br_bigwig_opts;
int br_coverage_bigwig(br_coverage *, const char *const *names, const br_bigwig_opts *opts, uint64_t *n_bytes);
int br_coverage_bigwig_read(br_coverage *, uint64_t off, uint64_t n, uint8_t *dst);
int br_coverage_bigwig_stats(const br_coverage *, uint64_t *n_chromosomes, uint64_t *n_sections, int32_t *zoom_levels, uint64_t *zoom_records,
                             uint64_t *raw_bytes, uint64_t *data_bytes, uint64_t *n_bytes, double *seconds);
int br_zlib_sections_device(int device, const uint8_t *src, const uint64_t *off, int64_t n, int mode, uint8_t **out, uint64_t *out_off);

/* br_project_bam_staged / _nowait for records that are in HBM already (a br_bam_reader bundle, or br_bam_split_device's);
 * bgzf_on_device takes the values of br_bam_bundle.bgzf_on_device (0, 1, BR_OUT_SAM_TEXT) */
int br_project_bam_resident(br_ctx *, const br_config *, const br_device_records *recs, const int32_t *ref_map, int32_t n_ref_map,
                            int bgzf_on_device, int nowait, br_host_bam *out);
/* The calls above with bgzf_on_device = BR_OUT_RESIDENT leave the projected records in HBM: no deflate, no SAM text, no
 * download (br_host_bam: the counters and n_rows, n_bytes = 0, data = NULL).  br_ctx_last_device_bam returns them, valid until
 * the context's next call (a br_sorter takes them from there).  In the other output modes the same call returns the records the
 * bundle call encoded before it deflated, formatted or downloaded them, valid as long (br_assign_add_last reads them); a flat
 * batch call leaves none (n_rows = 0).  br_device_bam_download is the other half: a record stream in
 * HBM (a br_sorter_next piece) -> the bytes of out_mode (0 records, 1 BGZF blocks, BR_OUT_SAM_TEXT lines) in the context's
 * pinned buffers, under the buffer rule of br_host_bam; nowait as br_project_bam_staged_nowait (br_host_bam_wait). */
#define BR_OUT_RESIDENT 3
int br_ctx_last_device_bam(const br_ctx *, br_device_bam *out);
int br_device_bam_download(br_ctx *, const br_device_bam *in, int out_mode, int nowait, br_host_bam *out);

/* ---- the records that did not project ------------------------------------------------------ */

/* An input record is unprojected when no output record came from it.  With br_ctx_set_param(ctx, "keep_unprojected", 1)
 * (scope record) or 2 (scope name: only the records of read names of which NO record projected) every bundle call --
 * br_project_bam_device and the entry points above it: br_project_bam_bundle, _staged, _staged_nowait, _resident -- appends the
 * bundle's unprojected records to an arena the context owns: [block_size][record], the input's bytes, in input order.  The
 * work (a flag per input alignment from the emitted rows, a count per read name, two scans, one gather) runs inside the call,
 * beside the record encoder, and is complete when the call returns: the caller may release or overwrite the input records
 * then.  It adds no host wait to the call.  0, the default: nothing is launched and nothing allocated.  Changing the
 * parameter while records are held answers BR_ERR_INVALID_ARG (draw or reset first).
 *
 *   - Flat batches (br_project_batch*, br_project_group*) have no records and add nothing.
 *   - Unmapped input records never reach a bundle (br_bam_split and the readers drop them) and are not in the result.
 *   - Memory: the held bytes plus 8 bytes a record, all in HBM until drawn and reset (while the arena grows, by half, the
 *     old one lies beside the new).  BR_ERR_CAPACITY from the projection call when the device's memory does not take it; the
 *     call's projected records are lost with it, what was held before stays.
 *   - The test hook "unprojected_cap" sets the arena's first capacity in bytes.
 *
 *   br_ctx_unprojected_stats   sums over the calls since the last reset: out[0] records seen, [1] unprojected records,
 *                              [2] their bytes (with the block_size words), [3] read names seen, [4] names with no record
 *                              projected, [5] names partly projected (some records, not all; counted in either scope),
 *                              [6] device bytes of the arena and its offsets now, [7] at most
 *   br_ctx_unprojected_next    the next records in order, up to max_bytes and at least one: a slice of the arena with row_off
 *                              rebased to the piece, valid until the next call on the context; n_rows = 0: that was all.
 *                              br_device_bam_download turns a piece into records, BGZF blocks or SAM lines, as it does a
 *                              sorter's.  Records added after a draw are handed out by the draws that follow
 *   br_ctx_unprojected_reset   forgets what is held, frees the arena and zeroes the counters */
int br_ctx_unprojected_stats(const br_ctx *, uint64_t out[8]);
int br_ctx_unprojected_next(br_ctx *, uint64_t max_bytes, br_device_bam *piece);
int br_ctx_unprojected_reset(br_ctx *);

/* ---- the posterior on the records ----------------------------------------------------------- */

/* br_assign: a run accumulator like br_quant and br_coverage.  It is fed the rows of every projection call by read name, as
 * br_coverage_add_names is, and with them the records the call encoded; after the quantifier's EM it knows the posterior weight of
 * every record and hands the records out again, each with a ZW:f entry (mode tag) or one drawn placement per read name (mode
 * sample).  All arithmetic is float64, no fused multiply-add, one rounding per operation; every sum is sequential in the stated
 * order, whatever its length, so a restatement in the same order gives the same bits.
 *   record r       row r of an add: records and rows of a projection call correspond one to one (br_device_bam row i is
 *                  br_device_rows row i).  The records of all adds are numbered in add order
 *   name(r)        the add-order index of r's read name, from row_off / group_off exactly as br_coverage_add_names takes it
 *   t(r)           a[r].transcript_id
 *   p(r)           the posterior (br_quant_posteriors) of the entry of t(r) among the labels of class name_cls[name(r)].  Every index
 *                  is compared with its table's size before it becomes an address; what fails is counted, never looked up
 *   m(r)           the number of records of name(r) whose transcript is t(r) (at least 1: r itself)
 *   placement      a record with BR_ROW_FIRST set; with BR_ROW_PAIRED set the next record is part of it, which must lie inside the
 *                  same name, have BR_ROW_PAIRED set and BR_ROW_FIRST clear.  A record that belongs to no placement, or a leader
 *                  without such a mate, makes the add BR_ERR_INVALID_ARG.  A name's placements are numbered in record order
 *   w(placement)   p(r0) / (double)m(r0), plus p(r1) / (double)m(r1) for a pair, the leader's term first: a read's (name,
 *                  transcript) posterior is split evenly among its records on that transcript, so the w of a name's placements sum
 *                  to the sum of its posteriors (1 up to rounding); a pair on two transcripts (BR_ROW_SAME_TX clear) is one placement
 *   ZW(r)          (float)w of r's placement, rounded to nearest even; both mates carry the same value
 *   draw           (mode sample) per name with at least one placement: Philox4x32-10 (the bootstrap's generator) under the key
 *                  ("seed" low word, high word) at the counter (name & 0xffffffff, name >> 32, 0, 1) -- word 3 = 1 keeps it apart
 *                  from the bootstrap's counters --; u = w0 | w1 << 32, U = (double)(u >> 11) * 2^-53; W = the sum of w over the
 *                  name's placements in order, target = U * W; the pick is the first placement j with cum_j > target, cum_j =
 *                  cum_(j-1) + w_j from 0; none: the last placement with w > 0; every w 0: placement 0.  A name without rows has no
 *                  pick and no records
 *   rewritten      the input record's bytes with block_size + 7 and the seven bytes 'Z' 'W' 'f' <float32 LE> behind its last byte
 *   record         (behind a CG:B,I spill as well).  In mode sample also: the values of the encoder's NH:i and HI:i entries become 1
 *                  (it writes exactly one of each as 4-byte 'i', AS:i between them for long reads, the CG spill behind them), flag bit
 *                  0x100 is cleared and MAPQ = br_row_mapq(1, "long_reads").  Every other byte is the input's
 *   invariance     how the names were cut into adds, and whether the tables came from host or device memory, changes nothing
 *
 *   br_assign_set_param   before the first add: "mode" 0 tag (default) / 1 sample, "seed" (the int64's bits), "long_reads" 0 / 1,
 *                         "max_bytes" (a cap on the arena's bytes, 0: none)
 *   br_assign_add         the rows of the read names group_off[0 .. n_groups] (shapes and rules of br_coverage_add_names; a is all it
 *                         reads of the rows) and their records: recs->row_off[r] .. [r + 1] of recs->data for row r.  recs is NULL on
 *                         every add or on none (a mix: BR_ERR_INVALID_ARG): without records the object computes w, zw and kept
 *                         only.  recs->n_rows != rows->n_rows, offsets that descend, a row the offsets give to no name, a bad
 *                         placement: BR_ERR_INVALID_ARG and nothing added.  BR_ERR_CAPACITY for memory that is not there, the
 *                         "max_bytes" cap, 2^32 names or records
 *   br_assign_add_last    br_assign_add of the context's last call: its rows, names and records (br_ctx_last_device_bam).  A flat
 *                         batch call has no records: BR_ERR_INVALID_ARG unless the object is without records (an object without
 *                         adds becomes that)
 *   br_assign_finish      needs a quantifier on the same device, with "keep_names", after br_quant_em, whose names number what the
 *                         adds were given; else BR_ERR_INVALID_ARG and the object is as it was.  A name past the count, a class
 *                         past the classes, a transcript that is not in its name's class or a posterior outside [0, 1] is counted,
 *                         never looked up, and makes the call return BR_ERR_INVALID_ARG; from then on every call but
 *                         br_assign_stats and br_assign_free answers that.  The records that will be written and the names with
 *                         records
 *   br_assign_values      after finish: w, zw and kept of the add-order records [first, first + n); any pointer may be NULL
 *   br_assign_next        as br_sorter_next: the next whole kept records, rewritten, up to max_bytes and at least one, with their
 *                         rebased row_off; valid until the second next; n_rows = 0: that was all.  BR_ERR_INVALID_ARG without
 *                         records, and (the object is dead then) for a kept record of mode sample without the NH / HI entries
 *   br_assign_stats       device bytes held now and at most, seconds in add / finish / next, bad[4]: what finish's look-up counted
 *                         (names, classes, transcripts, posteriors); any pointer may be NULL
 * Device memory (n records, K of them kept): the arena's 4 + block_size bytes a record (+ 64; it grows by half, the old one beside
 * the new while copying), 16 bytes a record of notes, 8 of offsets; from finish on 9 a record (w, kept) and 12 a kept record (the
 * list, the rewritten offsets), while it runs 20 a record more (p, m, the ranks); next holds two piece buffers (assign.cpp). */
typedef struct br_assign br_assign;
int br_assign_new(int device, br_assign **out);
int br_assign_set_param(br_assign *, const char *name, int64_t value);
int br_assign_add(br_assign *, const br_device_bam *recs, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups,
                  int on_device, void *stream);
int br_assign_add_last(br_assign *, br_ctx *);
int br_assign_finish(br_assign *, br_quant *, int64_t *n_records_out, int64_t *n_names_with_records);
int br_assign_values(br_assign *, int64_t first, int64_t n, double *w, float *zw, uint8_t *kept);
int br_assign_next(br_assign *, uint64_t max_bytes, br_device_bam *piece);
int br_assign_stats(const br_assign *, uint64_t *held, uint64_t *peak, double *add_s, double *finish_s, double *next_s, uint64_t *bad);
void br_assign_free(br_assign *);

/* ---- UMI-aware duplicate removal ------------------------------------------------------------ */

/* br_dedup: a run accumulator like br_quant, br_coverage and br_assign.  It is fed the rows of every projection call by read name and
 * the records the call encoded, and decides per READ NAME whether it is a PCR copy of another: two names are copies of one molecule
 * when they carry the same UMI (method directional: UMIs one mismatch apart, the rarer joining the more abundant) and project to
 * the same set of placements.  Whole names are kept or dropped, so a multi-mapper's records stay together.  All of it is integer and
 * byte arithmetic: a restatement gives the same bits.
 *   name i         the add-order index of a read name, from row_off / group_off exactly as br_coverage_add_names / br_assign_add take
 *                  it.  Records and rows correspond one to one (br_device_bam row r is br_device_rows row r)
 *   UMI(i)         from the name's first record, at add time; at most 32 bytes, compared as bytes: length first, then content, case-
 *                  sensitive.  A record lies in the stream as [block_size][record]; from the block's start l_read_name is at byte 12,
 *                  n_cigar_op at 16, flag at 18, l_seq at 20, read_name at 36, aux at 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2
 *                  + l_seq.  "umi_source" 0 (name, umi_tools extract's convention): the bytes of read_name (without its NUL) behind
 *                  the last byte equal to "umi_sep" (default '_').  "umi_source" 1 (tag): the value, without its NUL, of the first aux
 *                  field whose two tag bytes equal "umi_tag" (b0 | b1 << 8, default RX) and whose type is Z; a field type outside
 *                  AcCsSiIfZHB or a field that runs past the record's end ends the walk: the name has no UMI and counts in n_bad_aux
 *                  (nothing past the record is read; no error).  No separator, no such tag, a length of 0 or above 32: NO UMI; the
 *                  name counts in n_no_umi (as the n_bad_aux ones do), a length above 32 in n_umi_too_long as well.  A name without a
 *                  UMI is its own molecule and never a duplicate.  A name without rows has no record: its UMI reads as length 0 and it
 *                  is counted nowhere
 *   entry(r)       (t, five, f) of a row r: t = a[r].transcript_id; f = the record's own flag word & 0xD1 (paired, reverse, read1,
 *                  read2); five = the unclipped 5' coordinate, int64: the row's rewritten CIGAR is read as br_quant's fragments read
 *                  it (cigar[r] itself when BR_ROW_NCIGAR(meta) <= 2, else pool[cigar[r] ...]), reflen = the sum over the ops M D N =
 *                  X, lead = the length of an S op that is the first op or follows only H ops, else 0, trail the same from the end -- of
 *                  the ops in the RECORD's order: a row with BR_ROW_MINUS holds them reversed, as the encoder writes them out;
 *                  five = pos - lead when !(f & 0x10), else pos + reflen + trail.  A pooled CIGAR reference that leaves n_pool_words:
 *                  BR_ERR_INVALID_ARG and nothing added
 *   signature(i)   the name's entries in ascending order of (t unsigned, five signed, f), equal ones repeated: a sorted multiset, so
 *                  the order in which an aligner listed a multi-mapper's alignments does not matter
 *   position group the names with at least one row that have equal signatures.  A name without rows is in no group: rep and
 *                  group_first 0xffffffff, dup 0, counted among neither molecules nor duplicates
 *   unique         ("method" 0) a molecule is the names of one position group with equal UMI
 *   directional    ("method" 1, the default; umi_tools' default) per position group the nodes are its distinct UMIs, c_u the number
 *                  of names carrying u; the nodes are ordered by (c descending, length ascending, bytes ascending); an edge u -> v
 *                  when both have the same length, their Hamming distance over bytes is exactly 1 and c_u >= 2 c_v - 1; root(v) is the
 *                  node of lowest order index among v and every node from which v can be reached along edges (umi_tools' breadth-
 *                  first assignment from the highest counts down: the earliest node that reaches v is reachable from no earlier one);
 *                  it is the fixed point of label[v] = min(label[v], label[u] for u -> v), whatever the schedule.  A molecule is the
 *                  names whose UMI has the same root
 *   rep, dup       unique: the molecule's name of lowest index; directional: the lowest-index name among those carrying the root's
 *                  UMI (umi_tools' choice: a read of the most abundant UMI).  rep[i] is that index, dup[i] = 1 when the name has rows
 *                  and rep[i] != i, else 0.  group_first[i]: the lowest name index of i's position group
 *   histogram      hist[s], s = 1 .. "hist_max" (default 1000): the molecules of s names, larger ones in the last bin; hist[0] = 0
 *   invariance     neither how the names were cut into adds, nor whether the tables lay in host or device memory, nor "hash_bits"
 *                  (the quantifier's test hook: fewer bits make unlike signatures collide; equality is always decided on the
 *                  contents) changes any result, and two runs give the same bits
 *
 *   br_dedup_set_param  before the first add: "method", "umi_source", "umi_sep", "umi_tag", "keep_records" 0 / 1 (default 0), "mark"
 *                       0 / 1 (default 0), "max_bytes" (a cap on the arena's bytes, 0: none), "hist_max" 1 .. 65535, "cell_source" and
 *                       "cell_tag" (per cell: behind this block); before finish: "hash_bits" 1 .. 64
 *   br_dedup_add        shapes and rules of br_assign_add, with the rows' cigar and pool: offsets that descend, recs->n_rows !=
 *                       rows->n_rows, a record of less than 36 bytes, a name of 2^30 rows or more: BR_ERR_INVALID_ARG and nothing
 *                       added.  recs is required.  BR_ERR_CAPACITY for memory that is not there, the cap, 2^32 names or rows.  With
 *                       "keep_records" the records are copied into an arena in HBM, growing by half; without, nothing of a record is
 *                       kept beyond the 33 UMI bytes a name and the flag bits in the entries
 *   br_dedup_add_last   the context's last call: its rows, names and records (br_ctx_last_device_bam); a flat batch call has no
 *                       records: BR_ERR_INVALID_ARG
 *   br_dedup_finish     the verdicts; names added, molecules, duplicates (names with rows - molecules).  A failure leaves the object
 *                       answering BR_ERR_INVALID_ARG to everything but br_dedup_stats and br_dedup_free.  The label propagation is
 *                       the only iterative part: it stops when a sweep changes nothing and is bounded by (largest group's node count)
 *                       sweeps, beyond which the call returns BR_ERR_HIP
 *   br_dedup_umis       after any add, for the names added so far: n x 32 bytes zero padded, and the lengths; either may be NULL
 *   br_dedup_result / br_dedup_hist   after finish; any pointer may be NULL; a range outside [0, n_names]: BR_ERR_INVALID_ARG
 *   br_dedup_flags      after finish: dup as a device array of n_names bytes owned by the object (br_quant_drop_names takes it)
 *   br_dedup_next       after finish, with "keep_records" (else BR_ERR_INVALID_ARG), as br_sorter_next / br_assign_next: whole records
 *                       in add order, up to max_bytes and at least one, with row_off rebased; valid until the second next; n_rows = 0:
 *                       that was all.  "mark" 0: the records of the names with dup == 0, every byte the input's; "mark" 1: every
 *                       record, those of duplicate names with 0x400 OR-ed into the flag word at byte 18, every other byte the input's
 *   br_dedup_stats      names, names with rows, n_no_umi, n_umi_too_long, n_bad_aux, position groups, nodes, edges, propagation
 *                       sweeps run (the last, which changed nothing, included), the largest group's node count, collisions met, device
 *                       bytes now and at most, microseconds in add and in finish, records br_dedup_next hands out
 * Device memory: 53 bytes a name (UMI 32, length 1, signature offset 8, length 4, hash 8) and 16 a row (the entry) until finish, with
 * "keep_records" the records' bytes (+ 64; the arena grows by half, the old one beside the new while copying) and 8 a row; an add
 * holds 16 bytes a row and 4 a name of its own while it runs.  From finish on 9 a name (rep, group_first, dup), 8 (hist_max + 1) and,
 * with records, 1 a row and 12 a record handed out; while it runs 4 a name, 32 a name with rows, 105 a node (its UMI 32, length 1, count,
 * first name, group and place 4 each, two labels 8, edge offset 8, cursor 4, molecule size 4, begin 8, two sort pairs 24), 24 a group
 * and 4 an edge (dedup.cpp). */
typedef struct br_dedup br_dedup;
int br_dedup_new(int device, br_dedup **out);
int br_dedup_set_param(br_dedup *, const char *name, int64_t value);
int br_dedup_add(br_dedup *, const br_device_bam *recs, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups,
                 int on_device, void *stream);
int br_dedup_add_last(br_dedup *, br_ctx *);
int br_dedup_finish(br_dedup *, int64_t *n_names, int64_t *n_molecules, int64_t *n_duplicates);
int br_dedup_umis(br_dedup *, int64_t first, int64_t n, uint8_t *umi /* n x 32, zero padded */, uint8_t *len);
int br_dedup_result(br_dedup *, int64_t first, int64_t n, uint32_t *rep, uint32_t *group_first, uint8_t *dup);
int br_dedup_hist(br_dedup *, uint64_t *hist /* hist_max + 1 */);
int br_dedup_flags(br_dedup *, const uint8_t **dup_device, int64_t *n);
int br_dedup_next(br_dedup *, uint64_t max_bytes, br_device_bam *piece);
int br_dedup_stats(const br_dedup *, uint64_t out[16]);
void br_dedup_free(br_dedup *);
/* Before br_quant_finish; n must equal the names added, else BR_ERR_INVALID_ARG and nothing changes.  Every name with a non-zero flag
 * (host or device memory) becomes a name without rows for everything finish makes: classes, counts, unique / ambig, name_cls
 * (0xffffffff), n_unassigned and the bootstrap's resampling pool.  The fragment-length histogram of "eff_len" was counted at the adds
 * and stays as it is.  *n_dropped: the names with a non-zero flag. */
int br_quant_drop_names(br_quant *, const uint8_t *flags, int64_t n, int on_device, int64_t *n_dropped);

/* br_dedup per cell.  "cell_source" (before the first add) 0: none, the default, and everything above as it stands; 1: name; 2: tag,
 * "cell_tag" (b0 | b1 << 8, default CB).  The barcode of a name is read as br_cells reads it (below), with "umi_sep" as the separator;
 * a name without one has the empty barcode.  A position group is then the names with at least one row that have equal signatures AND
 * equal barcodes (length first, then bytes): umi_tools' --per-cell.  The signature groups are made as above; inside them the names
 * are sorted by (length, barcode) with stable radix passes and cut where the barcode changes, by comparing the barcodes themselves, so
 * "hash_bits" has no say in it.  Nodes, edges, rep, dup, group_first, the histogram and the invariance clause read as above with that
 * group.  Device memory: 33 bytes a name more (barcode 32, length 1).
 *
 * br_cells: a run accumulator like br_dedup.  It is fed the names of every projection call and the records the call encoded, keeps the
 * cell barcode of every READ NAME, and at finish turns the quantifier's per-name classes into a sparse cell x feature matrix.
 *   name i         as br_dedup's; records and rows correspond one to one
 *   barcode(i)     from the name's first record, at add time; at most 32 bytes, compared as bytes: length first, then content.
 *                  "barcode_source" 0 (name, umi_tools extract's READ_CB_UMI): with p2 the last byte of read_name (without its NUL)
 *                  equal to "barcode_sep" (default '_') and p1 the last such byte before p2, the bytes between p1 and p2; fewer
 *                  than two separators: none.  "barcode_source" 1 (tag): the value of the first aux field whose tag bytes equal
 *                  "barcode_tag" (default CB) and whose type is Z, the aux walk and its bad_aux rule being br_dedup's.  A length
 *                  of 0 or above 32: NO barcode; the name counts in n_no_barcode (as the n_bad_aux ones do), a length above 32 in
 *                  n_barcode_too_long as well.  A name without rows has no record: length 0, counted nowhere
 *   finish         takes a br_quant on the same device on which br_quant_finish has run with "keep_names" (the EM is not needed)
 *                  and whose name count equals the object's, else BR_ERR_INVALID_ARG and nothing changes; tx_feature[t] <
 *                  n_features for each of the quantifier's transcripts, else the same
 *   counted name   a name with a barcode and name_cls != 0xffffffff (so a name br_quant_drop_names dropped does not count: with
 *                  br_dedup in front the unit is the molecule, without it the read name)
 *   cell k         the distinct barcodes of the counted names, numbered in ascending (length, bytes) order
 *   entry e        of cell k: a distinct class of the cell's counted names, in ascending class index; n_e the number of such names,
 *                  F_e the ascending distinct tx_feature[t] over the class's labels, m_e = |F_e|
 *   slot s         of cell k: the ascending distinct features over the cell's entries
 *   "mode" 0       unique: value[k, f] = the sum of n_e over the entries with F_e = {f}, exact integers; the slots that end at 0
 *                  are not part of the matrix.  Per cell, in every mode: names = the sum of n_e, unique = that over m_e == 1,
 *                  multi = that over the others
 *   "mode" 2       em: theta_s = 1; one iteration: d_e = the sum of theta_f over F_e ascending, q_e = n_e / d_e (0 when d_e == 0),
 *                  theta'_s = theta_s * the sum of q_e over the entries containing s in ascending entry order; rel = the maximum of
 *                  |theta' - theta| / theta' over theta' > 1e-8.  Checked after every iteration, per cell: the cell stops at rel <
 *                  tolerance (default 1e-2) or at "max_iters" (default 10000), which bounds the loop whatever the numbers are.
 *                  value = theta, n_iters per cell.  Every slot is part of the matrix
 *   "mode" 1       uniform: exactly one such iteration, value = the sum of n_e / m_e; n_iters = 1
 *   sums           one after the other in the stated order, except a list of more than 64 items: lane l of a wave takes the items
 *                  l, l + 64, ... in ascending order and the 64 partial sums meet in wave_sum's fixed tree.  No floating-point
 *                  atomic.  Two runs with the same parameters give the same bits; neither the cut into adds, nor host or device
 *                  tables, nor "hash_bits" (accepted for symmetry: the barcodes are sorted by their bytes, nothing is hashed), nor
 *                  "lds_bytes" changes any
 *   routes         the whole iteration loop of a cell runs inside one kernel launch for all cells.  A cell of at most 64 slots and
 *                  at most 64 pairs (entry x feature) is one wave's work, four to a block; a larger one gets a block of 256 threads
 *                  with theta, theta' and q in LDS when 8 (2 slots + entries) + 64 <= "lds_bytes" (0 .. 65536, default 65536), else
 *                  the same code on scratch in HBM
 *
 *   br_cells_set_param / br_cells_set_tolerance   before the first add
 *   br_cells_add / br_cells_add_last   shapes and refusal rules of br_dedup_add; rows->a, cigar and pool are not read
 *   br_cells_barcodes        after any add: n x 32 bytes zero padded, and the lengths; either may be NULL
 *   br_cells_finish          *n_cells, *n_entries (the matrix's).  A failure other than BR_ERR_INVALID_ARG leaves the object dead
 *   br_cells_cell_barcodes / br_cells_name_cells (0xffffffff: in no cell) / br_cells_cell_stats   after finish; pointers may be NULL
 *   br_cells_matrix          CSR by cell over the cells [first_cell, first_cell + n): cell_off (n + 1, from 0), features ascending
 *                            (feature and value hold cell_off[n] items; size them by a first call with both NULL)
 *   br_cells_stats           names, counted names, n_no_barcode, n_barcode_too_long, n_bad_aux, cells, entries, pairs, slots, matrix
 *                            entries, cells of the wave / block / HBM route, microseconds in add, in finish and in the value kernel
 * Device memory: 33 bytes a name until finish; finish and what it keeps: cells.cpp. */
typedef struct br_cells br_cells;
int br_cells_new(int device, br_cells **out);
int br_cells_set_param(br_cells *, const char *name, int64_t value);
int br_cells_set_tolerance(br_cells *, double tolerance);
int br_cells_add(br_cells *, const br_device_bam *recs, const br_device_rows *rows, const uint32_t *group_off, int64_t n_groups,
                 int on_device, void *stream);
int br_cells_add_last(br_cells *, br_ctx *);
int br_cells_barcodes(br_cells *, int64_t first, int64_t n, uint8_t *cb /* n x 32, zero padded */, uint8_t *len);
int br_cells_finish(br_cells *, br_quant *, const uint32_t *tx_feature, int64_t n_features, int64_t *n_cells, int64_t *n_entries);
int br_cells_cell_barcodes(br_cells *, int64_t first, int64_t n, uint8_t *cb, uint8_t *len);
int br_cells_name_cells(br_cells *, int64_t first, int64_t n, uint32_t *cell);
int br_cells_matrix(br_cells *, int64_t first_cell, int64_t n, uint64_t *cell_off, uint32_t *feature, double *value);
int br_cells_cell_stats(br_cells *, int64_t first, int64_t n, uint64_t *names, uint64_t *unique, uint64_t *multi, uint32_t *n_features,
                        uint32_t *n_iters);
int br_cells_stats(const br_cells *, uint64_t out[16]);
void br_cells_free(br_cells *);

/* br_whitelist: the allowed cell barcodes of a run in one device's HBM, built once and read-only afterwards, so one object serves any
 * number of br_cells and br_dedup objects on its device.  With one set, br_cells_finish and br_dedup_finish first map every
 * name's observed barcode onto the list, repairing single-byte errors: STARsolo's --soloCBwhitelist / --soloCBmatchWLtype.
 *   whitelist      W barcodes of 1..32 bytes, compared as bytes: length first, then content, as the cells are.  Duplicates collapse;
 *                  entry w is the barcode's rank among the distinct ones in ascending (length, bytes) order
 *   observed       the barcode of a name as br_cells / br_dedup read it at add time, unchanged
 *   count[w]       the number of names added over the whole run (all adds) whose observed barcode equals entry w exactly.  Only names
 *                  with rows have a barcode; the class of a name and its duplicate verdict play no part, so br_dedup and br_cells,
 *                  fed the same names, resolve every name the same way
 *   candidates     of an observed barcode b that is not in the whitelist: the distinct entries of b's length that differ from b in
 *                  exactly one byte.  They are found by replacing one byte of b by one of A C G T other than the byte itself (an N
 *                  has four replacements), so an entry with other bytes can only match exactly
 *   "correct" 0    exact: b resolves to itself if it is in the whitelist, else to nothing
 *   "correct" 1    1mm (STARsolo 1MM): as exact; a b not in the whitelist resolves to its candidate when it has exactly one, is
 *                  ambiguous with two or more, and has no match with none
 *   "correct" 2    1mm-multi (STARsolo 1MM_multi without base qualities): among the candidates with count > 0 the one with the
 *                  largest count; two or more sharing the largest count: ambiguous; no candidate with count > 0: no match
 *                  An exact hit always wins, whatever lies one byte away
 *   status         per name.  0: no observed barcode; 1: exact; 2: corrected; 3: no match; 4: ambiguous
 *   afterwards     a name of status 1 or 2 carries the entry's bytes as its barcode; a name of status 3 or 4 has none (length 0): for
 *                  br_cells it is in no cell, for br_dedup it has the empty barcode, as a name without one has
 *   table          open addressing in HBM: a power of two >= 2 W slots, 64 at least; a slot is one 64-bit word (tag << 32) | (entry +
 *                  1), 0 when empty, claimed with a 64-bit compare-and-swap, linear probing.  The hash is a 64-bit mix (murmur3's
 *                  fmix64) of the four words and the length, masked to "hash_bits" (1..64; 0: the default, 64); home slot and tag
 *                  are both taken from the masked hash, so at 1 bit every entry has one of two home slots and every tag collides.
 *                  Which slot an entry lands in depends on the order of the atomics; no result does.  Insert and probe loops are
 *                  bounded by the slots
 * Everything is integers and bytes: the same bits come out whatever the cut into adds, host or device tables, or "hash_bits".
 *
 *   br_whitelist_new        cb: n x 32 bytes (what lies past a barcode's length is not read), len: n.  n = 0, n >= 2^31, a length of 0
 *                           or above 32, hash_bits outside 0..64: BR_ERR_INVALID_ARG and nothing is made
 *   br_whitelist_barcodes   the distinct entries [first, first + n) in order; either pointer may be NULL
 *   br_whitelist_match      the n barcodes as n names, one barcode each, from host arrays: length 0 means no barcode (above 32:
 *                           BR_ERR_INVALID_ARG); count is taken over these n.  entry: 0xffffffff for none.  Not to be called from
 *                           two threads at once on one object
 *   br_whitelist_stats      given, distinct, slots, the longest probe chain at build (slots one insert looked at), microseconds in
 *                           build, hash_bits, device bytes held, device bytes at most
 *   br_cells_set_whitelist / br_dedup_set_whitelist   before finish, a whitelist on the object's device and "correct" 0..2, else
 *                           BR_ERR_INVALID_ARG and nothing changes; br_dedup needs "cell_source" != 0.  The whitelist must live until
 *                           finish has returned.  finish resolves after its argument checks; after it br_cells_barcodes returns
 *                           the resolved barcodes.  Without a whitelist set nothing new is launched or allocated
 *   br_cells_name_status    after a finish with a whitelist: the status per add-order name
 *   br_cells_whitelist_stats / br_dedup_whitelist_stats   after such a finish: the names of status 0, 1, 2, 3, 4, the distinct
 *                           observed barcodes D, microseconds in the resolve, "correct"
 * Device memory: 33 bytes an entry and 8 a slot; the resolve's tables (whitelist.cpp) are gone before finish goes on. */
typedef struct br_whitelist br_whitelist;
int br_whitelist_new(int device, const uint8_t *cb /* n x 32, zero padded */, const uint8_t *len, int64_t n, int hash_bits, br_whitelist **out);
int br_whitelist_barcodes(br_whitelist *, int64_t first, int64_t n, uint8_t *cb, uint8_t *len);
int br_whitelist_match(br_whitelist *, const uint8_t *cb, const uint8_t *len, int64_t n, int correct, uint32_t *entry, uint8_t *status);
int br_whitelist_stats(const br_whitelist *, uint64_t out[8]);
void br_whitelist_free(br_whitelist *);
int br_cells_set_whitelist(br_cells *, const br_whitelist *, int correct);
int br_dedup_set_whitelist(br_dedup *, const br_whitelist *, int correct);
int br_cells_name_status(br_cells *, int64_t first, int64_t n, uint8_t *status);
int br_cells_whitelist_stats(const br_cells *, uint64_t out[8]);
int br_dedup_whitelist_stats(const br_dedup *, uint64_t out[8]);

/* br_cellcall: which barcodes of a cell x feature count matrix are cells, in one device's HBM.  The three methods are MODELLED ON
 * STARsolo's --soloCellFilter TopCells | CellRanger2.2 | EmptyDrops_CR; the definitions below are this library's own and are not
 * claimed to give STARsolo's or CellRanger's sets (neither program was at hand to compare with).
 *   matrix         K cells x F features as CSR by cell: cell_off (K + 1, cell_off[0] = 0), feature (ascending inside a cell) and
 *                  count (> 0), in host or device memory.  total[c] = the sum of the cell's counts, below 2^32
 *   rank           the cells sorted by the key (0xffffffff - total) << 32 | c: larger totals first, ties by ascending cell index.
 *                  "total at rank r" below is the total of the cell at that place; K = 0 calls nothing
 *   "method" 0     topcells: t = total at rank min("expected", K) - 1; called (status 1): every cell with total >= max(t, 1), ties
 *                  at the threshold included
 *   "method" 1     cr2.2, the `simple` filter, in float64 as written: r = min(K - 1, (int64)((double)expected * (1.0 - percentile))),
 *                  tmax = total at rank r, tmin = max(1, (int64)((double)tmax / ratio + 0.5)); called (status 1): total >= tmin, the
 *                  rank prefix of length n_simple
 *   "method" 2     emptydrops: the simple filter first (status 1), then the steps below; where a step says `falls back` the result is
 *                  the simple one and the stats' fallback word says why (1: empty window, 2: zero ambient sum, 3: no candidate)
 *   ambient        amb[g] = the sum of count over the cells at ranks ["ind_min", min("ind_max", K)); an empty window or N = sum of amb
 *                  = 0 falls back.  A feature is active if some cell of the matrix holds it
 *   p              br_cellcall_sgt: Simple Good-Turing (Gale & Sampson 1995) over the active features, on the host in float64.  n_r =
 *                  the active features with amb = r; r_1 < ... < r_m the values >= 1 that occur, r_0 = 0, r_{m+1} = 2 r_m - r_{m-1};
 *                  Z_j = 2.0 * n_{r_j} / (r_{j+1} - r_{j-1}); x_j = log r_j, y_j = log Z_j; with all sums in ascending j: mx = (sum x) /
 *                  m, my = (sum y) / m, b = (sum (x_j - mx)(y_j - my)) / (sum (x_j - mx)^2); y(r) = r * pow(1.0 + 1.0 / r, b + 1.0).
 *                  Walking j upward, until switched: if r_j + 1 does not occur, switch; else x = (r + 1) * n_{r+1} / n_r, sd =
 *                  sqrt((r + 1)^2 * (n_{r+1} / (n_r * n_r)) * (1.0 + n_{r+1} / n_r)); |x - y(r)| <= 1.96 sd: switch, else r* = x.
 *                  From the switch on r* = y(r).  P0 = n_1 / N when a feature has count 1 and an active one has count 0, else 0; N' =
 *                  sum of n_r r* (ascending j); p = (1 - P0) r* / N' for a count r >= 1 and P0 / n_0 for an active feature with count
 *                  0; an inactive feature has p = 0.  m < 2 or not b < -1: add-one smoothing instead, p = (amb + 1) / (N + active
 *                  features).  info: the route (0 Good-Turing, 1 add-one), the bits of b, the active features, m
 *   tables         lp[g] = log(p[g]) of the active features (0 for the others; -inf where p is 0); ln[k] = log((double)k), k = 1 ..
 *                  n_max + 1 (ln[0] = 0); cum_g = cum_{g-1} + p[g] over all features in index order, T[g] = (uint64)(cum_g / cum_last
 *                  * 4294967296.0), the last active feature's and every later T = 2^32.  A 32-bit draw u picks the first g with u <
 *                  T[g]: never an inactive feature
 *   candidates     med = total at rank n_simple / 2, lo = max("umi_min", (int64)(umi_frac * (double)med + 0.5), 1): the cells at ranks
 *                  >= n_simple with total >= lo, the first "cand_max" of them in rank order (m of them; none falls back).  n_max =
 *                  the largest candidate total; the wanted totals = the distinct candidate totals, in ascending order
 *   O_c            of a candidate: over the sequence that lists its first feature count_1 times, then its second, ...: from 0.0, step
 *                  i (1-based) that lists feature g for the (k + 1)-th time adds ((ln[i] - ln[k + 1]) + lp[g])
 *   L_s            of simulation s < "sims": draw i (0-based) is output word i & 3 of Philox4x32-10 with counter (i >> 2, s, 0, 2)
 *                  under key ("seed" low, high word); it picks a feature by T; L_s is O's recurrence over the draws 0 .. n_max - 1,
 *                  read off after every wanted total of draws
 *   p-value        lower = #{ s : L_s(total_c) < O_c }; pval = (double)(lower + 1) / (double)(sims + 1)
 *   padj           Benjamini-Hochberg over the m candidates sorted by (lower, rank) ascending: at the 1-based place j, q_j = min(1.0,
 *                  pval * (double)m / (double)j); padj_j = the least q at j or behind.  Status 2 where padj <= "fdr"
 * Every floating-point sum is one chain in the order given, without contraction, and no floating-point atomic is used: the same
 * bits come out whatever "sim_bytes" is.
 *
 *   br_cellcall_set_param / _set_real   before run: "method", "expected" (3000), "ind_min" (45000), "ind_max" (90000), "umi_min" (500),
 *                           "cand_max" (20000), "sims" (10000), "seed" (0), "sim_bytes" (2^31: the count tables of one launch; one
 *                           simulation's table at least), "keep_sims" (0); reals "percentile" (0.99), "ratio" (10.0), "umi_frac"
 *                           (0.01), "fdr" (0.01).  An unknown name, a value out of range, a call after run: BR_ERR_INVALID_ARG
 *   br_cellcall_run         once.  on_device: the three tables are device memory, ready on `stream`.  Offsets that descend or do not
 *                           start at 0, a feature >= n_features or not above the one before it, a count of 0, a total of 2^32 or
 *                           more: BR_ERR_INVALID_ARG, and the object is as it was
 *   br_cellcall_calls       cells [first, first + n): status (0, 1, 2), rank, total.  Here and below any pointer may be NULL
 *   br_cellcall_ambient     features [first, first + n): amb, p, lp, T; BR_ERR_INVALID_ARG where the run made none (methods 0 and 1,
 *                           an empty window; after a zero sum only amb)
 *   br_cellcall_logtable    ln[first .. first + n) of its n_max + 2 entries
 *   br_cellcall_candidates  candidates [first, first + n) in rank order: cell, O, lower, pval, padj
 *   br_cellcall_wanted      the wanted totals [first, first + n)
 *   br_cellcall_sims        with "keep_sims" 1: L of the wanted totals [w_first, w_first + n_w) x simulations [s_first, s_first + n_s),
 *                           n_w rows of n_s; without it L is dropped when the p-values are made
 *   br_cellcall_stats       K, cells of status 1, of status 2, the threshold (t or tmin), n_simple, the window's barcodes, N, active
 *                           features, the route of p (2: none), the bits of b, lo, candidates, n_max, wanted totals, simulation
 *                           launches, the fallback word, microseconds of rank, ambient, simulate, p-value, method, sims, device bytes
 *                           held, device bytes at most, matrix entries, F
 *   br_cellcall_sgt         the paragraph `p` alone, on the host: needs no device */
typedef struct br_cellcall br_cellcall;
int br_cellcall_new(int device, br_cellcall **out);
int br_cellcall_set_param(br_cellcall *, const char *name, int64_t value);
int br_cellcall_set_real(br_cellcall *, const char *name, double value);
int br_cellcall_run(br_cellcall *, int64_t n_cells, int64_t n_features, const uint64_t *cell_off, const uint32_t *feature, const uint32_t *count,
                    int on_device, void *stream);
int br_cellcall_calls(br_cellcall *, int64_t first, int64_t n, uint8_t *status, uint32_t *rank, uint64_t *total);
int br_cellcall_ambient(br_cellcall *, int64_t first, int64_t n, uint64_t *amb, double *p, double *lp, uint64_t *T);
int br_cellcall_logtable(br_cellcall *, int64_t first, int64_t n, double *ln);
int br_cellcall_candidates(br_cellcall *, int64_t first, int64_t n, uint32_t *cell, double *O, uint32_t *lower, double *pval, double *padj);
int br_cellcall_wanted(br_cellcall *, int64_t first, int64_t n, uint64_t *total);
int br_cellcall_sims(br_cellcall *, int64_t s_first, int64_t n_s, int64_t w_first, int64_t n_w, double *L);
int br_cellcall_stats(const br_cellcall *, uint64_t out[32]);
int br_cellcall_sgt(const uint64_t *amb, const uint8_t *active, int64_t n, double *p, uint64_t info[4]);
void br_cellcall_free(br_cellcall *);
/* Calling the cells of a br_cells.  With the parameter "call_counts" 1 (set before the first add) br_cells_finish also keeps the counts
 * the cells are called on: the values of mode "unique" without the entries at 0, as 32-bit integers -- whatever "mode" is, as
 * STARsolo ranks by its unique counts (in mode "unique" they are the matrix's own).  Without it finish launches and allocates
 * nothing new.
 *   br_cells_call           after finish, once: runs a br_cellcall of the same device that has its parameters and has not run on
 *                           those device tables (n_features: the finish's), then copies the matrix's rows of the called cells
 *                           (status != 0) on the device: a flag a cell, two scans, one launch, a wave a row.  Without
 *                           "call_counts", before finish, a second time, a br_cellcall that has run: BR_ERR_INVALID_ARG
 *   br_cells_matrix_called  after br_cells_call: the called cells [first, first + n) in cell order as br_cells_matrix returns cells --
 *                           the "mode"'s values -- and `cells`, their indices; cell_off is required, the others may be NULL */
int br_cells_call(br_cells *, br_cellcall *, int64_t n_features);
int br_cells_matrix_called(br_cells *, int64_t first, int64_t n, uint32_t *cells, uint64_t *cell_off, uint32_t *feature, double *value);

/* ---- SAM text out -------------------------------------------------------------------------- */

/* The reference names RNAME and RNEXT print, in refID order (a refID < 0 or >= n prints '*'); uploaded to HBM once, kept by
 * the context until the next call.  Without it every RNAME prints '*'. */
int br_ctx_set_sam_refs(br_ctx *, const char *const *names, int32_t n);
/* An uncompressed record stream in HBM (br_device_bam: data / n_bytes / row_off / n_rows, as br_project_bam_device leaves it)
 * -> SAM text in HBM, one '\n'-terminated line per record, byte for byte what htslib's bam_read1 + sam_format1 print for it
 * (`samtools view`): a record in the spilled CIGAR form (<l_seq>S<ref_len>N plus CG:B,I) prints its real CIGAR and no CG tag,
 * f values print as printf("%g").  *text is a device pointer owned by the context, valid until its next call.
 * BR_ERR_INVALID_ARG, and no text, when a record has a tag type outside AcCsSiIfZHB or data past its end. */
int br_sam_format_device(br_ctx *, const br_device_bam *in, void *stream, const uint8_t **text, uint64_t *n_bytes);

/* BGZF inflate on the device (one wave per block: the reader side of br_bgzf_deflate_device).  br_bgzf_scan (host) walks
 * the block headers of a piece of a BGZF file -- up to `cap` complete blocks; empty ones (the EOF marker) are stepped over --
 * and lists for every block where its DEFLATE payload lies in `data`, where its bytes go in the inflated stream (dst_off: a
 * running sum from 0), and the CRC32 / ISIZE of its trailer; *consumed is where the next call continues.
 * br_bgzf_inflate_device inflates the listed blocks of the same bytes in HBM (`src`, `n_src`); *out is a device pointer to
 * the inflated stream, valid until the next call on the context.  BR_ERR_INVALID_ARG for a malformed header, or for a block
 * that does not inflate to ISIZE bytes with its CRC32 (what htslib's bgzf_read reports as a read error). */
int br_bgzf_scan(const uint8_t *data, uint64_t n_bytes, int64_t cap, br_bgzf_block *blocks, int64_t *n_blocks,
                 uint64_t *consumed, uint64_t *out_bytes);
int br_bgzf_inflate_device(br_ctx *, const uint8_t *src, uint64_t n_src, const br_bgzf_block *blocks, int64_t n_blocks,
                           void *stream, const uint8_t **out, uint64_t *out_bytes);

/* Walks the block_size chain of an uncompressed BAM alignment section (host): fills rec_off /
 * rec_len for up to `cap` MAPPED records (unmapped ones are counted and skipped like
 * bramble.cpp:376-379) and reports how many bytes were consumed (a trailing partial record is
 * left for the next call).  BR_ERR_INVALID_ARG on a record whose fixed fields overrun its
 * block_size. */
int br_bam_split(const uint8_t *data, uint64_t n_bytes, int64_t cap, uint64_t *rec_off, uint32_t *rec_len,
                 int64_t *n_records, int64_t *n_unmapped, uint64_t *consumed);

/* BGZF-compress n bytes that sit in HBM (one wave per 56 KiB block: hash-table LZ77, per-block dynamic Huffman codes --
 * or the fixed code with br_ctx_set_param("deflate_dynamic", 0) -- and CRC32);
 * *out is a device pointer to the concatenated blocks (no EOF marker), valid until the next call on the context. */
int br_bgzf_deflate_device(br_ctx *, const uint8_t *src, uint64_t n, void *stream, const uint8_t **out, uint64_t *out_bytes);

/* ---- annotation loading and the command line (scope table rows f-1 / f-3) ----------------- */

/* GTF / GFF3 (plain or gzip) -> transcripts in the reference's guide order: gclib GffReader with
 * transcripts only, sorted by location, reference names compared lexicographically
 * (src/bramble.cpp:497-512; gfo_cmpByLoc, gclib/gff.cpp:75-90), so that position = the tid the
 * reference assigns through its output header (src/bramble.cpp:559-596).  Exons are 1-based
 * half-open [start, end+1) like src/bramble.cpp:164-165.  The arrays stay owned by the handle and
 * feed br_index_build directly. */
typedef struct br_annotation br_annotation;
int br_annotation_load(const char *path, br_annotation **out);
/* the same with `threads` workers taking the lines apart (br_annotation_load: up to 16); what the lines mean depends on
 * the lines before them and is applied in file order whatever the thread count */
int br_annotation_load_mt(const char *path, int threads, br_annotation **out);
void br_annotation_free(br_annotation *);
size_t br_annotation_num_transcripts(const br_annotation *);
const br_transcript *br_annotation_transcripts(const br_annotation *);
size_t br_annotation_num_refs(const br_annotation *);            /* reference names in order of first appearance */
const char *const *br_annotation_refnames(const br_annotation *);
/* The gene of every transcript: one C string per transcript, in the order of br_annotation_transcripts, owned by the handle.
 *   GTF    the gene_id attribute of the first line applied to the record that has a non-empty one: the `transcript` line or an
 *          exon-like line, whichever came first in file order
 *   GFF3   the record's gene_id= attribute if a transcript or exon-like line of the record has one; otherwise the first entry of
 *          the transcript line's Parent=; otherwise (a record made by exon lines only, or one without a parent) the transcript's
 *          own id
 * A record for which none of this yields a non-empty string gets its own transcript id: no transcript is left without a gene.
 * The gene id is carried along and never compared: the transcripts' order does not depend on it, and it does not depend on the
 * number of loader threads. */
const char *const *br_annotation_gene_ids(const br_annotation *);

/* The reference's command line (src/bramble.cpp:443-485): in.bam -G -o [-S] [-p] [--fr|--rf]
 * [--lr|--lr-hq] [--strict] [--max-*] [--similarity-threshold] [--quiet], plus --device-deflate (default: BGZF blocks made on the
 * GPU) / --host-deflate / --compression-level N (host codec), --device-reader (default for a regular file on one device: the
 * input is inflated and split into records on the GPU, br_bam_reader) / --host-reader, --bundle-size and --device / --devices,
 * --collate, -O bam|sam, --sort [--write-index], --quant FILE [--quant-classes FILE] [--quant-eff-length [--quant-fld FILE]]
 * [--quant-bootstraps B [--quant-seed S] [--quant-boot-out FILE]] [--quant-genes FILE [--quant-gene-classes FILE] [--quant-gene-map FILE]]
 * (br_quant above; the genes are br_annotation_gene_ids', numbered in order of first appearance in @SQ order, or the map file's), --coverage FILE / --coverage-summary FILE [--coverage-primary] [--coverage-weight unit|nh|em] / --coverage-bigwig FILE [--coverage-bigwig-zooms 0-10] [--coverage-bigwig-uncompressed] (br_coverage and br_coverage_bigwig above;the usage text says the
 * rest).
 * Returns the process exit code. */
int br_cli_main(int argc, char **argv);
/* For a process whose only job is that one call (the `bramble` binary): with `on` != 0 br_cli_main does not return after a
 * run that got as far as the final report -- the output file is closed and renamed, the streams are flushed, and the process
 * leaves through _exit(code) without unwinding gigabytes of record buffers, pinned memory and device allocations first
 * (bramble-cli/src/main.rs:56-60 keeps its index in a ManuallyDrop for the same reason).  Off by default: a host that calls
 * br_cli_main as a function gets every device and pinned allocation of the run released before the call returns. */
void br_cli_exit_at_end(int on);
/* First touch of a device (HIP runtime start-up, context creation): callable from a thread of its own so that it overlaps
 * other start-up work.  BR_ERR_NO_DEVICE when the device does not exist. */
int br_device_warmup(int device);

/* BGZF container utilities (host only; what the reference gets from htslib's bgzf layer behind
 * GSamReader / GSamWriter): whole-file inflate / deflate on `threads` host threads.  The reader
 * verifies each block's CRC32; the writer emits 0xff00-byte payload blocks and the EOF marker. */
int br_bgzf_write_file(const char *path, const uint8_t *data, uint64_t n, int threads, int level);
int br_bgzf_read_file(const char *path, int threads, uint8_t **out, uint64_t *n); /* free with br_free_buffer */
void br_free_buffer(uint8_t *);
const char *br_bgzf_codec(void); /* "libdeflate" (bound at run time when present) or "zlib" */

/* ---- measurement hooks ------------------------------------------------------ */

/* Kernel names reported by br_ctx_kernel_ms / rocprof. */
#define BR_K_SEGMENT 0    /* k_segment */
#define BR_K_COUNT 1      /* k_project<G,false> (count pass; on the large short-read paths the main kernel, without the exon walk) */
#define BR_K_EMIT 2       /* k_emit_dense (general class; the whole list for long-read presets) */
#define BR_K_PAIR_COUNT 3 /* k_pair */
#define BR_K_PAIR_EMIT 4  /* k_pair<true> (per-record {match, input, NH, HI | flags}) */
#define BR_K_ROWS 5       /* k_rows (the packed row table) */
#define BR_K_SCAN 6       /* k_scan_* */
#define BR_K_EMIT_AUX 7   /* k_project<64,true> (alignments with > 64 candidate rows) */
#define BR_K_KSW 8        /* k_ksw (-S clip rescue DP) */
#define BR_K_BAM 9        /* k_bam_scan + k_bam_size + k_bam_tasks (or k_bam_encode<G>) */
#define BR_K_PARSE 10     /* k_rec_fields + k_group_off + k_rec_copy + k_mates* + k_seq_* */
#define BR_K_CODEC 11     /* k_deflate_dynamic | k_deflate_fixed, k_bgzf_compact; k_inflate */
#define BR_K_EMIT_SIMPLE 12 /* k_emit_dense, simple class (one read exon from a single M op) */
#define BR_K_PRIMARY 13   /* k_primary (+ the per-read-name counters) */
#define BR_K_CIGAR_POOL 14 /* unused since ABI version 2 */
#define BR_K_COUNT_WALK 15 /* k_project<G,false,false,2>: the deferred alignments of the split count pass, with the exon walk */
#define BR_K_EXPAND 16    /* k_expand (emit work list) */
#define BR_K_GROUP_IDS 17 /* k_group_ids */
#define BR_K_P1 18        /* unused since the single-pass count + emit variant was removed */
#define BR_K_P1_WALK 19   /* unused since the single-pass count + emit variant was removed */
#define BR_K_EMIT_WL 20   /* unused since the single-pass count + emit variant was removed */
#define BR_K_NAME_SEED 21  /* k_name_seed: first mt19937_64 output per read name (direct rows) */
#define BR_K_PAIR_MASK 22  /* k_pair_mask: pairing on the survivor sets, before the emit pass */
#define BR_K_PAIR_BIG 23   /* k_big<0> + k_pair_big: the same for alignments with > 64 candidate rows */
#define BR_K_GROUP_DESC 24 /* k_group_desc: NH / HI / primary per read name (+ the per-read-name counters) */
#define BR_K_EXPAND_ROWS 25 /* k_expand_rows: emit work list + emit descriptors */
#define BR_K_EMIT_ROWS_SIMPLE 26 /* k_emit_rows<1>: packed rows of the simple class */
#define BR_K_EMIT_ROWS 27  /* k_emit_rows<2>: packed rows of the general class */
#define BR_K_BIG_EMIT 28   /* k_big<1>: packed rows of the alignments with > 64 candidate rows */
#define BR_K_SAM_FORMAT 29 /* k_samfmt_measure<16|64> + k_samfmt_emit16 + k_samfmt_emit64 (SAM text out) */
#define BR_K_NUM 30
/* When enabled, every launch is bracketed by hipEvents on the launch stream. */
int br_ctx_set_profiling(br_ctx *, int enabled);
/* Launch tuning: "group_lanes" (8|16|32|64 lanes cooperating on one alignment),
 * "blocks_per_cu" (grid size of the grid-stride projection kernels), "bam_lanes" (0, the default: a wave per 32
 * re-encoded records, their byte regions as 16-byte copy tasks; 4..64: that many lanes per record), "deflate_dynamic" (1: per-block Huffman codes, 0: the fixed code), "deflate_waves" (test hook: a cap on the dynamic coder's persistent waves, rounded up to 4, so that one wave takes many blocks; 0: as many as the chip holds),
 * "pair_bitmask" (1, the default: direct rows intersect two mates' transcript sets as 64-bit masks where their ids span at most 64; 0: as lists always. Same rows.),
 * "emit_rank_tids" (1, the default: that intersection leaves the pair's common transcript ids as a 16-byte word per alignment and the direct-rows emit kernels take a record's rank from it; 0: they gather the kept survivors' ids, no word is stored. Same rows; br_ctx_direct_tidwords.),
 * "emit_general_preset" (1, the default: on the direct-rows route the short-read preset without --max-error-exon emits its general class with the kernel specialised to it, k_emit_rows<2, 1>; 0: with the kernel of every other preset. Read at every launch. Same rows.).
 * Short-read presets run the count pass of large batches as a main kernel without the exon walk plus a second one for the
 * alignments that need it, and launch the emit work list per class; small batches and the similarity-filter presets use
 * one kernel for each. */
int br_ctx_set_param(br_ctx *, const char *key, int64_t value);
/* Device time (ms) of kernel `which` during the last projection call, summed
 * over its launches; *launches receives the launch count. */
int br_ctx_kernel_ms(br_ctx *, int which, double *ms, int32_t *launches);
/* ... summed over every call since br_ctx_set_profiling(ctx, 1) (a timed loop reads it once, behind its last step) */
int br_ctx_kernel_ms_sum(br_ctx *, int which, double *ms, int64_t *launches);
/* Diagnostic pass (never part of a timed region): computes the exact counters below
 * for the device batch the context projected last.  After a direct-rows call it projects the batch once more through
 * the match-table path with that call's configuration: the context's last-call row tables are then that projection's. */
int br_ctx_collect_counters(br_ctx *, const br_device_batch *, void *stream);
/* Exact algorithmic byte counters (SURVEY.md 8d formula), after br_ctx_collect_counters:
 * out[0]=B_in, out[1]=B_idx, out[2]=B_out, out[3]=sum n_cigar, out[4]=read exons,
 * out[5]=overlap hits, out[6]=matches, out[7]=rewritten-CIGAR words over all matches. */
int br_ctx_last_counters(br_ctx *, uint64_t out[8]);
/* Diagnostic of the last call, which must have been a direct-rows call (else BR_ERR_INVALID_ARG), read from what that call
 * left on the device: out[0] = alignments with more than 64 candidate rows (big_list), out[1] = side-arena attempts,
 * out[2] = arena entries the last attempt asked for, out[3] = arena capacity of that attempt (entries), out[4] = windows
 * that k_pair_mask handed to k_pair_mask_wide, out[5] = work-list entries of the light two-exon class (kept matches of
 * "M N M" alignments whose every survivor meets the annotated junction exactly, emitted by the simple-class kernel; those
 * of alignments with more than 64 candidate rows or their mates are not counted), out[6] = PAIR alignments that k_pair_mask / k_pair_mask_wide resolved by their tid lists, not by 64-bit
 * tid masks: the partner lies outside the window of 62 alignments (+ a neighbour on either side), or the two mates' survivor
 * tids span more than 64 (max - min > 63); counted only with "pair_bitmask" 1, out[7] = 0.  pflags (NULL, or n_aln bytes): the pairing flags per
 * alignment (1 paired, 2 a transcript in common with the mate, 4 the mate of a pair led by the other record, 8 more than
 * 64 candidate rows).  The test hook br_ctx_set_param("side_cap", v >= 64) sets the arena's first capacity; a call that
 * outgrows it grows the arena to what it asked for and repeats once. */
int br_ctx_direct_diag(br_ctx *, uint64_t out[8], uint8_t *pflags);
/* Diagnostic of the last call, which must have been a direct-rows call (else BR_ERR_INVALID_ARG), never part of a timed
 * region: the tid word of each of its n_aln alignments.  base[a] != 0xffffffff: k_pair_mask intersected the pair's
 * transcript sets as 64-bit masks and found a common transcript; base[a] is the pair's smallest transcript id, bit b of
 * common[a] says that transcript base[a] + b is kept, and the emit kernels took a record's rank among the alignment's by
 * counting the bits below its own.  base[a] == 0xffffffff: no word (an alignment without a partner, a pair on the list path
 * or without a common transcript, the partner of an alignment with more than 64 candidate rows): ranked by gathering the kept
 * survivors' ids.  Words of alignments that keep nothing, or that have more than 64 candidate rows, mean nothing.  After a call made with
 * br_ctx_set_param("emit_rank_tids", 0) (1, the default; read at every call; same rows) every alignment reads as "no word". */
int br_ctx_direct_tidwords(br_ctx *, uint64_t *common, uint32_t *base);

/* -S runs: out[0] = rescue problems of the last call, out[1] = ksw2 DP cells (sum of qlen x tlen),
 * out[2] = accepted rescues, out[3] = coded sequence bytes. */
int br_ctx_rescue_stats(br_ctx *, uint64_t out[4]);
/* Diagnostic: routing of the last call's rescue DP problems: pieces, problems per register-array shape (64 / 128 / 256 /
 * 384 target columns), problems left to the general kernel before the DP, direction-tape bytes of the largest piece, 0,
 * leftovers of the last piece after the DP, tape rows (array steps) per shape [4], 0 x 4.  Keys of br_ctx_set_param: "ksw_fast" (0 = general kernel only),
 * "ksw_tape_mb" (tape budget; larger batches are processed in pieces), "ksw_tape_pct" (test hook: share of the tape the
 * array kernels may use). */
int br_ctx_ksw_diag(br_ctx *, uint64_t out[16]);

/* Diagnostic: the -S rescue DP alone (k_ksw = ksw_extz2_sse as src/evaluate.cpp:296-313 calls it, on the device).
 * n (target, query) ASCII pairs in; per pair: ok[p] = the rescue would be accepted (max >= 10 and the walk reached the
 * last cell, src/evaluate.cpp:484,643), max[p], and -- when ok -- the traceback CIGAR in forward order (BAM-packed
 * M / I / D) at cigar[p * cigar_cap ...], n_cigar[p] ops.
 * side (may be null: every pair a right-side problem): side[p] = 0 makes pair p a left-side problem, 1 a right-side one.
 * The DP is the same; the side decides how the traceback becomes a clip segment.  For side 0 the caller passes both
 * strings already reversed, as align_reversed does (src/evaluate.cpp:368-395).
 * refc, n_seg, seg (all three or none): the clip segment of every accepted pair (build_left/right_clip_segment,
 * src/evaluate.cpp:397-448,548-598) as the rescue's emit pass reads it: refc[p] = reference bases consumed, n_seg[p]
 * override ops (len << 4 | 10 match, 11 deletion, 12 insertion, 13 clip; a leftover clip included) at seg[p * cigar_cap ...]; 0 for a pair not accepted. */
int br_ctx_ksw_pairs(br_ctx *, int64_t n, const char *const *tseq, const char *const *qseq, int32_t *ok, int32_t *max,
                     uint32_t *n_cigar, uint32_t *cigar, uint32_t cigar_cap, const uint8_t *side, int32_t *refc,
                     uint32_t *n_seg, uint32_t *seg);

/* The reference's primary tie-break (src/core.cpp:214-218,298-299):
 * uniform_int_distribution<uint32_t>(0, n_tied-1)(mt19937_64(std::hash<std::string>(name))),
 * restated bit-exactly for libstdc++ (GCC 11, x86-64). */
uint32_t br_primary_pick(const char *name, size_t len, uint32_t n_tied);

const char *br_version(void);
const char *br_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* BRAMBLE_AMD_H */
