// ============================================================================
// TEST INFRASTRUCTURE ONLY -- CPU oracle for the genome->transcriptome
// projection hot path.
//
// This file is a literal, dependency-free CPU restatement of the reference
// algorithm (zrudnick/bramble, C++ path).  It exists so that tests/, the
// smoke() entry and bench.py's cpu_baseline leg can CHECK the HIP path.  It is
// never linked into, imported by, or called from the product library
// (bramble_amd/): the product fails loudly when its HIP extension is missing.
//
// Parity status:
//   * interval query, tolerance table, exon-chain evaluation, ideal CIGAR,
//     CIGAR merge, mate pairing, NH/HI/MAPQ: pinned by the reference's own
//     known answers (tests/golden/reference_known_answers.json: K1-K11 of
//     SURVEY.md 8c) -- everything those do not exercise is pinned only by
//     hand-derived cases.
//   * ksw2 clip rescue (ksw_extz2 + ksw_backtrack): "parity unpinned".  The DP
//     recurrence follows the in-tree patch file
//     subprojects/packagefiles/ksw2/ksw2_extz2_sse.cpp, but ksw2.h (pinned at
//     lh3/ksw2@289609b in subprojects/ksw2.wrap) is absent from
//     the reference tree; ksw_reset_extz / ksw_apply_zdrop / ksw_backtrack /
//     ksw_push_cigar are restated from the published upstream header.
//   * cgranges IITree (pinned at lh3/cgranges@b3d5e2c in
//     subprojects/cgranges.wrap) is absent too; its published contract
//     (half-open overlap a.st<en && st<a.en, hits in ascending index of the
//     start-sorted array) is restated in IntervalIndex below.
//
// Every function cites the reference file:line it follows (paths relative to
// the reference tree's root).
// ============================================================================
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

namespace orc {

// ---- htslib constants used on this path (SAM spec values) -------------------
enum : uint8_t {
  C_MATCH = 0, C_INS = 1, C_DEL = 2, C_REF_SKIP = 3, C_SOFT_CLIP = 4,
  C_HARD_CLIP = 5, C_PAD = 6, C_EQUAL = 7, C_DIFF = 8, C_BACK = 9,
  // include/evaluate.h:10-13 (private override op codes)
  C_MATCH_OVERRIDE = 10, C_DEL_OVERRIDE = 11, C_INS_OVERRIDE = 12,
  C_CLIP_OVERRIDE = 13
};
static inline uint32_t cig_op(uint32_t c) { return c & 0xf; }
static inline uint32_t cig_len(uint32_t c) { return c >> 4; }
static inline uint32_t cig_gen(uint32_t l, uint32_t o) { return (l << 4) | o; }

enum : uint16_t {
  F_PAIRED = 0x1, F_PROPER_PAIR = 0x2, F_UNMAP = 0x4, F_MUNMAP = 0x8,
  F_REVERSE = 0x10, F_MREVERSE = 0x20, F_READ1 = 0x40, F_READ2 = 0x80,
  F_SECONDARY = 0x100
};

static const int KSW_NEG_INF = -0x40000000;

struct GSeg { uint32_t start = 0, end = 0; };

// include/evaluate.h:21-128 (Cigar::add_operation coalesces equal neighbours,
// keeps zero lengths)
struct Cigar {
  std::vector<uint32_t> ops;
  void add_operation(uint32_t len, uint8_t op) {
    if (ops.empty()) { ops.push_back(cig_gen(len, op)); return; }
    uint32_t &prev = ops.back();
    if (cig_op(prev) == op) prev = cig_gen(cig_len(prev) + len, op);
    else ops.push_back(cig_gen(len, op));
  }
};

// include/evaluate.h:130-150
struct GuideExon {
  uint32_t tid = 0, start = 0, end = 0, pos = 0, pos_start = 0;
  uint8_t exon_id = 0;
  int32_t left_ins = 0, right_ins = 0, left_gap = 0, right_gap = 0;
  bool has_prev = false, has_next = false;
  uint32_t prev_start = 0, prev_end = 0, next_start = 0, next_end = 0;
  uint32_t transcript_len = 0;
  const std::string *seq = nullptr;
};

// include/evaluate.h:152-181
struct AlignInfo {
  uint32_t fwpos = 0, rcpos = 0;
  char strand = 0;
  Cigar cigar;
  bool primary_alignment = false;
  int clip_score = 0;
  double similarity_score = 0;
  int32_t hit_index = 0;
};
struct ExonChainMatch {
  uint32_t tid = 0;
  AlignInfo align;
  double total_coverage = 0, total_operations = 0;
  int32_t ref_consumed = 0, junc_hits = 0, transcript_len = 0;
  uint8_t prev_op = 0;
};

// include/evaluate.h:183-192
enum ExonStatus { FIRST_EXON = 0, MIDDLE_EXON = 1, LAST_EXON = 2, ONLY_EXON = 3,
                  INS_EXON = 4, GAP_EXON = 5, LEFTC_EXON = 6, RIGHTC_EXON = 7 };

// include/evaluate.h:194-219
struct Segment {
  bool has_gexon = false, has_qexon = false;
  GuideExon gexon;
  GSeg qexon;
  ExonStatus status = FIRST_EXON;
  bool is_small_exon = false;
  Cigar cigar;
  int score = 0;
};
struct TidData {
  bool elim = false, has_left_clip = false, has_right_clip = false;
  ExonChainMatch match;
  std::vector<Segment> segments;
};

// include/evaluate.h:275-285
struct EvalConfig {
  uint32_t max_clip = 5, max_junc_ins = 0, max_junc_gap = 0;
  bool ignore_small_exons = false;
  uint32_t max_error_exon = 0;
  float similarity_threshold = 1.0f;
  bool filter_by_similarity = false;
};

// CLI-level switches (src/bramble.cpp:68-83)
struct Flags {
  bool lr = false, lr_hq = false, strict = false, use_fasta = false;
  bool fr = false, rf = false;
  bool has_max_clip = false, has_max_junc_ins = false, has_max_junc_gap = false,
       has_sim_thr = false, has_max_error_exon = false;
  uint32_t max_clip = 0, max_junc_ins = 0, max_junc_gap = 0, max_error_exon = 0;
  float sim_thr = 0;
  bool long_reads() const { return lr || lr_hq; }  // src/bramble.cpp:504
};

// src/evaluate.cpp:1136-1221 (preset + override resolution; LR before LR_HQ
// before STRICT, so --strict never reaches a long-read run)
static inline EvalConfig resolve_config(const Flags &f) {
  EvalConfig c;
  uint32_t mc, mji, mjg, mee; float thr;
  auto pick = [](bool has, uint32_t v, uint32_t d) { return has ? v : d; };
  if (!f.long_reads()) {
    mc = pick(f.has_max_clip, f.max_clip, f.strict ? 0u : 5u);
    mji = pick(f.has_max_junc_ins, f.max_junc_ins, 0);
    mjg = pick(f.has_max_junc_gap, f.max_junc_gap, 0);
    thr = f.has_sim_thr ? f.sim_thr : (float)1.0;
    mee = pick(f.has_max_error_exon, f.max_error_exon, 0);
  } else if (f.lr) {
    mc = pick(f.has_max_clip, f.max_clip, 40);
    mji = pick(f.has_max_junc_ins, f.max_junc_ins, 40);
    mjg = pick(f.has_max_junc_gap, f.max_junc_gap, 40);
    thr = f.has_sim_thr ? f.sim_thr : (float)0.60;
    mee = pick(f.has_max_error_exon, f.max_error_exon, 35);
  } else {  // lr_hq
    mc = pick(f.has_max_clip, f.max_clip, 5);
    mji = pick(f.has_max_junc_ins, f.max_junc_ins, 10);
    mjg = pick(f.has_max_junc_gap, f.max_junc_gap, 10);
    thr = f.has_sim_thr ? f.sim_thr : (float)0.90;
    mee = pick(f.has_max_error_exon, f.max_error_exon, 35);
  }
  c.max_clip = mc; c.max_junc_ins = mji; c.max_junc_gap = mjg;
  c.max_error_exon = mee; c.similarity_threshold = thr;
  c.ignore_small_exons = (mee > 0);
  c.filter_by_similarity = (thr < 1.0);
  return c;
}

// ---- interval index ---------------------------------------------------------
// include/g2t.h:28-43 (IITData) + cgranges IITree<int,IITData> contract.
struct IITData {
  uint32_t tid = 0; uint8_t exon_id = 0; uint32_t pos_start = 0;
  bool has_prev = false, has_next = false;
  uint32_t prev_start = 0, prev_end = 0, next_start = 0, next_end = 0;
  uint32_t transcript_len = 0;
  std::string seq;  // src/g2t.cpp:50-55 (upper-cased exon sequence, -S only)
};
struct Interval { int st, en; IITData d; };

struct IntervalIndex {
  std::vector<Interval> a;
  std::vector<int> maxend;  // running max of en over a[0..i] (search pruning only)
  void add(int st, int en, const IITData &d) { a.push_back({st, en, d}); }
  void index() {  // IITree::index(): sort by start (tie order is unspecified upstream)
    std::stable_sort(a.begin(), a.end(),
                     [](const Interval &x, const Interval &y) { return x.st < y.st; });
    maxend.resize(a.size());
    int m = std::numeric_limits<int>::min();
    for (size_t i = 0; i < a.size(); i++) { m = std::max(m, a[i].en); maxend[i] = m; }
  }
  // IITree::overlap(): indices with a.st < en && st < a.en, ascending.
  void overlap(int st, int en, std::vector<size_t> &out) const {
    out.clear();
    size_t hi = std::lower_bound(a.begin(), a.end(), en,
        [](const Interval &x, int v) { return x.st < v; }) - a.begin();
    size_t lo = std::upper_bound(maxend.begin(), maxend.begin() + hi, st) - maxend.begin();
    for (size_t i = lo; i < hi; i++)
      if (st < a[i].en) out.push_back(i);
  }
};

struct G2T {
  // src/g2t.cpp:271-287: trees[refid] = (forward, reverse)
  std::vector<std::pair<IntervalIndex, IntervalIndex>> trees;
  std::vector<std::string> tid_names;
  std::vector<uint32_t> tid_lengths;

  const IntervalIndex *tree_for(int refid, char strand) const {  // g2t.cpp:278-287
    if (refid < 0 || (size_t)refid >= trees.size()) return nullptr;
    if (strand == '+' || strand == 1) return &trees[refid].first;
    if (strand == '-' || strand == -1) return &trees[refid].second;
    return nullptr;
  }

  // src/bramble.cpp:132-211 (build_g2t_tree) for one transcript; exons are
  // 1-based half-open [start,end) in genomic order (the caller has applied the
  // reference's end+1).  ref_seq: whole reference sequence (1-based coords) or
  // nullptr.
  uint32_t add_transcript(int refid, char strand, const std::string &name,
                          const std::vector<GSeg> &exons, const std::string *ref_seq) {
    uint32_t tid = (uint32_t)tid_names.size();
    tid_names.push_back(name);
    if (refid >= 0 && (size_t)refid >= trees.size()) trees.resize(refid + 1);
    struct IData { uint32_t start, end; uint8_t idx; uint32_t pos_start; };
    std::vector<IData> iv;
    int exon_count = (int)exons.size();
    uint32_t pos_start = 0;
    for (int k = 0; k < exon_count; k++) {
      int idx = (strand == '-') ? (exon_count - k - 1) : k;
      IData d{exons[idx].start, exons[idx].end, (uint8_t)idx, pos_start};
      iv.push_back(d);
      pos_start += d.end - d.start;
    }
    uint32_t transcript_len = pos_start;
    tid_lengths.push_back(transcript_len);
    if (refid < 0 || (strand != '+' && strand != '-')) return tid;
    IntervalIndex &tree = (strand == '+') ? trees[refid].first : trees[refid].second;
    for (int k = 0; k < exon_count; k++) {
      IITData n;
      n.tid = tid; n.exon_id = iv[k].idx; n.pos_start = iv[k].pos_start;
      if (k > 0) { n.prev_start = iv[k-1].start; n.prev_end = iv[k-1].end; n.has_prev = true; }
      if (k < exon_count - 1) { n.next_start = iv[k+1].start; n.next_end = iv[k+1].end; n.has_next = true; }
      n.transcript_len = transcript_len;
      if (ref_seq) {  // src/g2t.cpp:50-55
        uint32_t s = iv[k].start, e = iv[k].end;  // 1-based [s,e)
        for (uint32_t p = s; p < e; p++) {
          char ch = (p >= 1 && p - 1 < ref_seq->size()) ? (*ref_seq)[p - 1] : 'N';
          if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 'a' + 'A');
          n.seq.push_back(ch);
        }
      }
      tree.add((int)iv[k].start, (int)iv[k].end, n);
    }
    return tid;
  }
  void finish() {  // g2tTree::indexTrees, src/g2t.cpp:318-323
    for (auto &p : trees) { p.first.index(); p.second.index(); }
  }

  static void fill(GuideExon &g, const Interval &iv) {
    g.start = iv.st; g.end = iv.en; g.transcript_len = iv.d.transcript_len;
    g.pos_start = iv.d.pos_start; g.exon_id = iv.d.exon_id;
    g.has_prev = iv.d.has_prev; g.has_next = iv.d.has_next;
    g.prev_start = iv.d.prev_start; g.prev_end = iv.d.prev_end;
    g.next_start = iv.d.next_start; g.next_end = iv.d.next_end;
    g.seq = &iv.d.seq;
  }

  // src/g2t.cpp:70-101 (findOverlappingForTid) via :325-331.  NB the reference
  // leaves pos/left_*/right_* of `gexon` untouched (uninitialised there); the
  // oracle leaves them at their zero default -- no emitted value depends on
  // them (see evaluate: a GAP segment's pos is always overwritten).
  bool guide_exon_for_tid(int refid, char strand, uint32_t tid, uint32_t qstart,
                          uint32_t qend, GuideExon &gexon) const {
    const IntervalIndex *t = tree_for(refid, strand);
    if (!t) return false;
    if (qstart == 0 && qend == 0) return false;
    std::vector<size_t> hits;
    t->overlap((int)qstart, (int)qend, hits);
    for (size_t idx : hits) {
      if (t->a[idx].d.tid == tid) { fill(gexon, t->a[idx]); return true; }
    }
    return false;
  }

  // src/g2t.cpp:103-257 (findOverlapping) via :334-344 (getGuideExons)
  bool guide_exons(int refid, char strand, GSeg q, const EvalConfig &config,
                   ExonStatus status, std::vector<GuideExon> &gexons) const {
    const IntervalIndex *t = tree_for(refid, strand);
    if (!t) return false;
    uint32_t qstart = q.start, qend = q.end;
    std::vector<size_t> hits;
    t->overlap((int)qstart, (int)qend, hits);
    if (hits.empty()) return false;
    for (size_t idx : hits) {
      uint32_t s = (uint32_t)t->a[idx].st, e = (uint32_t)t->a[idx].en;
      uint32_t pos = 0, left_gap = 0, left_ins = 0, right_gap = 0, right_ins = 0;
      const IITData &data = t->a[idx].d;
      if (strand == '+') {
        if (s <= qstart) {
          pos = (qstart - s) + data.pos_start;
          left_gap = qstart - s;
          if (status == MIDDLE_EXON || status == LAST_EXON)
            if (left_gap > config.max_junc_gap) continue;
        } else {
          pos = data.pos_start;
          left_ins = s - qstart;
          if (status == MIDDLE_EXON || status == LAST_EXON) {
            if (left_ins > config.max_junc_ins) continue;
          } else {
            if (left_ins > config.max_clip) continue;
          }
        }
        if (e < qend) {
          right_ins = qend - e;
          if (status == FIRST_EXON || status == MIDDLE_EXON) {
            if (right_ins > config.max_junc_ins) continue;
          } else {
            if (right_ins > config.max_clip) continue;
          }
        } else if (qend < e) {
          right_gap = e - qend;
          if (status == FIRST_EXON || status == MIDDLE_EXON)
            if (right_gap > config.max_junc_gap) continue;
        }
      } else {
        if (qend <= e) {
          pos = (e - qend) + data.pos_start;
          right_gap = e - qend;
          if (status == FIRST_EXON || status == MIDDLE_EXON)
            if (right_gap > config.max_junc_gap) continue;
        } else {
          pos = data.pos_start;
          right_ins = qend - e;
          // src/g2t.cpp:204: `status == FIRST_EXON || MIDDLE_EXON` is always
          // true (MIDDLE_EXON == 1), so max_clip is never consulted here.
          if (right_ins > config.max_junc_ins) continue;
        }
        if (qstart < s) {
          left_ins = s - qstart;
          if (status == MIDDLE_EXON || status == LAST_EXON) {
            if (left_ins > config.max_junc_ins) continue;
          } else {
            if (left_ins > config.max_clip) continue;
          }
        } else if (s < qstart) {
          left_gap = qstart - s;
          if (status == MIDDLE_EXON || status == LAST_EXON)
            if (left_gap > config.max_junc_gap) continue;
        }
      }
      GuideExon ex;
      fill(ex, t->a[idx]);
      ex.tid = data.tid; ex.pos = pos;
      ex.left_gap = (int32_t)left_gap; ex.left_ins = (int32_t)left_ins;
      ex.right_gap = (int32_t)right_gap; ex.right_ins = (int32_t)right_ins;
      gexons.push_back(ex);
    }
    return !gexons.empty();
  }
};

// ---- read model -------------------------------------------------------------
struct Read {
  // src/bramble.cpp:313-327 (process_read_in) + include/bramble.h:130-150
  char strand = '.';
  int refid = -1;
  uint32_t start = 0;             // 1-based
  std::vector<GSeg> segs;         // half-open after end++
  std::vector<uint32_t> cigar;    // BAM-packed real CIGAR
  uint16_t flags = 0;
  int mate_idx = -1;              // pair_idx (at most one entry by construction)
  int l_qseq = 0;
};

// gclib/GSam.cpp:197-291 (setupCoordinates) + src/bramble.cpp:246-255 (end++).
// pos0 is the 0-based BAM core.pos.  Returns false where the reference aborts
// (GError "invalid CIGAR record", GSam.cpp:290).
static inline bool segments_from_cigar(int32_t pos0, const uint32_t *cigar, uint32_t n_cigar,
                                       std::vector<GSeg> &out) {
  out.clear();
  int l = 0;
  int exstart = pos0;
  GSeg exon;
  bool exonStarted = false, intron = false, ins = false;
  for (uint32_t i = 0; i < n_cigar; ++i) {
    uint32_t op = cig_op(cigar[i]);
    switch (op) {
      case C_EQUAL: case C_DIFF: case C_MATCH:
        exonStarted = true; l += (int)cig_len(cigar[i]); intron = false; ins = false; break;
      case C_DEL:
        l += (int)cig_len(cigar[i]); ins = false; break;
      case C_INS:
        ins = true; break;
      case C_REF_SKIP:
        if (!exonStarted) break;
        if (!ins || !intron) {
          exon.end = (uint32_t)(pos0 + l);
          exon.start = (uint32_t)(exstart + 1);
          out.push_back(exon);
        }
        l += (int)cig_len(cigar[i]);
        exstart = pos0 + l;
        intron = true;
        break;
      case C_SOFT_CLIP: ins = false; break;
      case C_HARD_CLIP: ins = false; break;
      case C_PAD: break;
      default: break;  // "Unhandled CIGAR operation" is only a stderr message upstream
    }
  }
  if (!intron) {
    exon.start = (uint32_t)(exstart + 1);
    exon.end = (uint32_t)(pos0 + l);
    out.push_back(exon);
  }
  uint32_t end = 0;
  if (exon.end) end = exon.end;
  if (end == 0) { out.clear(); return false; }
  for (auto &e : out) e.end++;  // src/bramble.cpp:252
  return true;
}

// src/bramble.cpp:213-244 (get_strand) + gclib/GSam.cpp:338-349 (spliceStrand).
// xs / ts: first char of the XS / ts tag or 0 when absent.
static inline char read_strand(const Flags &f, uint16_t flags, char xs, char ts) {
  if (f.long_reads()) return '.';  // src/bramble.cpp:382
  char c = xs;
  if (c == 0) {
    char m = ts;
    if (m == '+' || m == '-') {
      if (flags & F_REVERSE) c = (m == '+') ? '-' : '+';
      else c = m;
    }
  }
  char strand = (c == '+' || c == '-') ? c : '.';
  if (strand == '.' && (f.fr || f.rf)) {
    bool is_paired = flags & F_PAIRED, is_rev = flags & F_REVERSE;
    bool cond = (f.rf && is_rev) || (f.fr && !is_rev);
    if (is_paired) {
      int pair_order = (flags & F_READ1) ? 1 : ((flags & F_READ2) ? 2 : 0);
      if (pair_order == 1) strand = cond ? '-' : '+';
      else strand = cond ? '+' : '-';
    } else {
      strand = cond ? '-' : '+';
    }
  }
  return strand;
}

}  // namespace orc
