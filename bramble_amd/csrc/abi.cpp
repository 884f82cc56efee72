// C ABI of libbramble_amd.so (include/bramble_amd.h): index build, configuration, the batch contract and contexts.  Host
// side of the drop-in boundary; the reference counterparts are cited per function in the header.  The rest of the ABI:
// pipeline.cpp (the projection), bam_path.cpp (BAM records in and out), reader.cpp (the device BAM reader), host_rows.cpp
// (host batches) and sam_reader.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "ctx.h"
#include "primary_pick.h"

int check_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0 || device >= n) return BR_ERR_NO_DEVICE;
  return BR_OK;
}

template <typename T>
static int upload(void **dst, const std::vector<T> &src, size_t &acc) {
  size_t bytes = std::max<size_t>(src.size() * sizeof(T), 16);
  HIPCHK(hipMalloc(dst, bytes));
  if (!src.empty()) HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  acc += bytes;
  return BR_OK;
}

// Common builder over flat arrays: transcript t has reference tx_ref[t], strand
// tx_strand[t] and exons [tx_exon_off[t], tx_exon_off[t+1]) in (ex_start, ex_end).
static int build_index_flat(size_t n_tx, const int32_t *tx_ref, const int8_t *tx_strand, const uint64_t *tx_exon_off,
                            const uint32_t *ex_start, const uint32_t *ex_end, std::vector<std::string> &&names,
                            size_t n_refs, const std::vector<const br_fasta_seq *> &fasta_by_ref, bool has_seq,
                            int device, br_index **out) {
  if (n_tx >= 0xffffffffull) return BR_ERR_CAPACITY;
  br_index *ix = new br_index();
  ix->n_refs = (uint32_t)n_refs;
  ix->has_seq = has_seq;
  ix->names = std::move(names);
  struct Row { uint32_t start, end, tid, gidx, pos_start; };
  std::vector<std::vector<Row>> slabs(2 * n_refs);
  ix->tx_first.reserve(n_tx + 1);
  std::vector<br_exon> ex;
  std::vector<uint32_t> pos_start;
  for (size_t t = 0; t < n_tx; t++) {
    int32_t refid = tx_ref[t];
    if (refid < 0 || (size_t)refid >= n_refs) { delete ix; return BR_ERR_ANNOTATION; }
    ex.clear();
    for (uint64_t k = tx_exon_off[t]; k < tx_exon_off[t + 1]; k++) ex.push_back({ex_start[k], ex_end[k]});
    std::stable_sort(ex.begin(), ex.end(), [](const br_exon &a, const br_exon &b) { return a.start < b.start; });
    for (size_t i = 0; i < ex.size(); i++) {
      if (ex[i].end < ex[i].start || (i + 1 < ex.size() && ex[i].end > ex[i + 1].start)) {
        fprintf(stderr, "[bramble_amd] transcript '%s': exons overlap or are inverted\n", ix->names[t].c_str());
        delete ix; return BR_ERR_ANNOTATION;
      }
    }
    uint32_t tlen = 0;
    for (auto &e : ex) tlen += e.end - e.start;
    if (tlen == 0) {
      // the reference writes no @SQ line for a transcript of length 0 (src/bramble.cpp:588-596) while tids keep counting
      // every guide: its header and its records would disagree.  GTF coordinates are inclusive, so a loader never makes
      // one; refuse it here instead of numbering around it.
      fprintf(stderr, "[bramble_amd] transcript '%s' has no exonic bases\n", ix->names[t].c_str());
      delete ix; return BR_ERR_ANNOTATION;
    }
    ix->lengths.push_back(tlen);
    ix->tx_first.push_back((uint32_t)ix->tx_ex.size());
    char strand = (char)tx_strand[t];
    bool minus = strand == '-';
    bool stranded = strand == '+' || strand == '-';
    const br_fasta_seq *fa = has_seq ? fasta_by_ref[(size_t)refid] : nullptr;
    // pos_start: cumulative spliced offset in TRANSCRIPT order (src/bramble.cpp:161-175)
    uint32_t acc = 0;
    pos_start.assign(ex.size(), 0);
    if (!minus) { for (size_t i = 0; i < ex.size(); i++) { pos_start[i] = acc; acc += ex[i].end - ex[i].start; } }
    else { for (size_t i = ex.size(); i-- > 0;) { pos_start[i] = acc; acc += ex[i].end - ex[i].start; } }
    for (size_t i = 0; i < ex.size(); i++) {
      uint32_t seq_off = 0;
      if (has_seq) {  // src/g2t.cpp:50-55: upper-cased exon sequence
        seq_off = (uint32_t)ix->seq_pool.size();
        for (uint32_t p = ex[i].start; p < ex[i].end; p++) {
          char ch = (fa && p >= 1 && (uint64_t)(p - 1) < fa->len) ? fa->seq[p - 1] : 'N';
          if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 'a' + 'A');
          ix->seq_pool.push_back((uint8_t)ch);
        }
      }
      ix->tx_ex.push_back(make_uint4(ex[i].start, ex[i].end, pos_start[i], seq_off));
      if (stranded) slabs[2 * (size_t)refid + (minus ? 1 : 0)].push_back({ex[i].start, ex[i].end, (uint32_t)t, (uint32_t)i, pos_start[i]});
    }
    ix->tx_ex.push_back(make_uint4(0xffffffffu, 0xffffffffu, 0, 0));  // sentinel
    if (ix->tx_ex.size() >= 0xfffffff0ull || ix->seq_pool.size() >= 0xfffffff0ull) { delete ix; return BR_ERR_CAPACITY; }
  }
  ix->tx_first.push_back((uint32_t)ix->tx_ex.size());
  for (int pad = 0; pad < 4; pad++) ix->tx_ex.push_back(make_uint4(0xffffffffu, 0xffffffffu, 0, 0));  // prefetch slack
  // The slabs (one per reference and strand) and the bucket tables (one per reference) are independent of each other: their
  // places in the flat arrays are fixed first, then a few host threads sort and fill them side by side (the command line
  // waits for this between the guide loader and the first bundle).
  auto for_each_par = [](size_t n, const std::function<void(size_t)> &fn) {
    unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::min<size_t>(n, std::max(1u, std::min(hw ? hw : 1u, 16u)));
    if (nt <= 1) { for (size_t i = 0; i < n; i++) fn(i); return; }
    std::atomic<size_t> next{0};
    auto body = [&]() { for (;;) { const size_t i = next.fetch_add(1); if (i >= n) break; fn(i); } };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back(body);
    body();
    for (auto &x : th) x.join();
  };
  ix->slab_off.assign(slabs.size() + 1, 0);
  {
    uint64_t tot = 0;
    for (size_t k = 0; k < slabs.size(); k++) { tot += slabs[k].size(); if (tot >= 0xfffffff0ull) { delete ix; return BR_ERR_CAPACITY; } ix->slab_off[k + 1] = (uint32_t)tot; }
    ix->s_start.resize((size_t)tot); ix->s_pmax.resize((size_t)tot); ix->s_tid.resize((size_t)tot); ix->s_row.resize((size_t)tot * 2);
  }
  for_each_par(slabs.size(), [&](size_t k) {
    auto &rows = slabs[k];
    std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.start < b.start; });
    uint32_t m = 0;
    size_t at = ix->slab_off[k];
    for (auto &r : rows) {
      m = std::max(m, r.end);
      ix->s_start[at] = r.start; ix->s_pmax[at] = m;
      // one 32-byte row = everything a candidate lane needs, in one 64-byte sector
      ix->s_row[2 * at] = make_uint4(r.start, r.end, ix->tx_ex[ix->tx_first[r.tid] + r.gidx + 1].x /* sentinel start = ~0u */, r.pos_start);
      const uint32_t n_ex = ix->tx_first[r.tid + 1] - ix->tx_first[r.tid] - 1;  // rows of the transcript minus its sentinel
      ix->s_row[2 * at + 1] = make_uint4(r.tid, r.gidx | (n_ex > 256u ? 0x80000000u : 0u), ix->tx_first[r.tid], ix->tx_ex[ix->tx_first[r.tid] + r.gidx + 1].y /* next exon's end */);
      ix->s_tid[at] = r.tid;
      at++;
    }
  });
  // bucket tables (replace the per-read binary search of the slab).  512-base bins: the count pass's candidate rows are a
  // superset bounded by the bins around a read, and narrower bins test fewer rows (bench step: 1 kb -> 512 b bins took the
  // main count kernel from 1.74 to 1.60 ms, 2 kb bins cost 0.18 ms more); the table is 16 bytes per bin and reference
  // (about 100 MB on a human-sized genome), which still leaves the index resident in the Infinity Cache
  const uint32_t SHIFT = 9;
  std::vector<uint64_t> n_bins(ix->n_refs, 2);
  ix->bin_off.assign((size_t)ix->n_refs + 1, 0);
  {
    uint64_t tot = 0;
    for (uint32_t r = 0; r < ix->n_refs; r++) {
      uint64_t nb = 2;
      for (int sd = 0; sd < 2; sd++) {
        uint32_t sb = ix->slab_off[2 * r + sd], se = ix->slab_off[2 * r + sd + 1];
        if (se > sb) nb = std::max<uint64_t>(nb, ((uint64_t)std::max(ix->s_start[se - 1], ix->s_pmax[se - 1]) >> SHIFT) + 2);
      }
      n_bins[r] = nb;
      tot += nb + 1;
      if (tot >= 0xfffffff0ull) { delete ix; return BR_ERR_CAPACITY; }
      ix->bin_off[r + 1] = (uint32_t)tot;
    }
    ix->t_bin.resize((size_t)tot);
  }
  for_each_par(ix->n_refs, [&](size_t r) {
    const uint64_t nb = n_bins[r];
    const size_t first = ix->bin_off[r];
    for (int sd = 0; sd < 2; sd++) {
      uint32_t sb = ix->slab_off[2 * r + sd], se = ix->slab_off[2 * r + sd + 1];
      uint32_t rh = sb, rl = sb;
      for (uint64_t bk = 0; bk <= nb; bk++) {
        if (bk < nb) {
          uint64_t edge = bk << SHIFT;
          while (rh < se && (uint64_t)ix->s_start[rh] < edge) rh++;
          while (rl < se && (uint64_t)ix->s_pmax[rl] <= edge) rl++;
        } else rh = rl = se;
        uint4 &e = ix->t_bin[first + bk];
        if (sd == 0) { e.x = rl; e.y = rh; } else { e.z = rl; e.w = rh; }
      }
    }
  });
  ix->device = device;
  if (device >= 0) {
    int rc = check_device(device);
    if (rc != BR_OK) { delete ix; return rc; }
    HIPCHK(hipSetDevice(device));
    size_t acc = 0;
    if ((rc = upload(&ix->d_slab_off, ix->slab_off, acc)) || (rc = upload(&ix->d_s_start, ix->s_start, acc)) ||
        (rc = upload(&ix->d_s_pmax, ix->s_pmax, acc)) || (rc = upload(&ix->d_bin_off, ix->bin_off, acc)) ||
        (rc = upload(&ix->d_t_bin, ix->t_bin, acc)) ||
        (rc = upload(&ix->d_s_tid, ix->s_tid, acc)) ||
        (rc = upload(&ix->d_s_row, ix->s_row, acc)) || (rc = upload(&ix->d_tx_ex, ix->tx_ex, acc)) ||
        (rc = upload(&ix->d_tx_first, ix->tx_first, acc)) || (rc = upload(&ix->d_seq_pool, ix->seq_pool, acc))) {
      br_index_free(ix); return rc;
    }
    ix->device_bytes = acc;
    DevIndex &d = ix->dev;
    d.n_refs = ix->n_refs; d.n_tx = (uint32_t)n_tx; d.n_rows = (uint32_t)ix->s_start.size();
    d.slab_off = (const uint32_t *)ix->d_slab_off; d.s_start = (const uint32_t *)ix->d_s_start;
    d.s_pmax = (const uint32_t *)ix->d_s_pmax;
    d.bin_shift = SHIFT; d.bin_off = (const uint32_t *)ix->d_bin_off;
    d.t_bin = (const uint4 *)ix->d_t_bin;
    d.s_tid = (const uint32_t *)ix->d_s_tid;
    d.s_row = (const uint4 *)ix->d_s_row; d.tx_ex = (const uint4 *)ix->d_tx_ex;
    d.tx_first = (const uint32_t *)ix->d_tx_first; d.seq_pool = (const uint8_t *)ix->d_seq_pool;
  }
  *out = ix;
  return BR_OK;
}

extern "C" int br_index_build(const br_transcript *transcripts, size_t n_transcripts,
                              const char *const *refnames, size_t n_refnames, const br_fasta_seq *fasta,
                              size_t n_fasta, int device, br_index **out) {
  if (!out || (!transcripts && n_transcripts) || (!refnames && n_refnames)) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  std::unordered_map<std::string, uint32_t> ref_of;
  for (size_t i = 0; i < n_refnames; i++) ref_of.emplace(refnames[i], (uint32_t)i);
  std::vector<const br_fasta_seq *> fa_by_ref(n_refnames, nullptr);
  for (size_t i = 0; i < n_fasta; i++) { auto it = ref_of.find(fasta[i].name ? fasta[i].name : ""); if (it != ref_of.end()) fa_by_ref[it->second] = &fasta[i]; }
  std::vector<int32_t> tx_ref(n_transcripts); std::vector<int8_t> tx_strand(n_transcripts);
  std::vector<uint64_t> off(n_transcripts + 1, 0); std::vector<uint32_t> es, ee; std::vector<std::string> names;
  for (size_t t = 0; t < n_transcripts; t++) {
    const br_transcript &tx = transcripts[t];
    names.emplace_back(tx.id ? tx.id : "");
    auto it = ref_of.find(tx.seqname ? tx.seqname : "");
    if (it == ref_of.end()) {  // bramble-rs/src/g2t.rs:442-444
      fprintf(stderr, "[bramble_amd] reference '%s' of transcript '%s' not in refnames\n",
              tx.seqname ? tx.seqname : "", tx.id ? tx.id : "");
      return BR_ERR_ANNOTATION;
    }
    tx_ref[t] = (int32_t)it->second; tx_strand[t] = (int8_t)tx.strand;
    for (uint32_t k = 0; k < tx.n_exons; k++) { es.push_back(tx.exons[k].start); ee.push_back(tx.exons[k].end); }
    off[t + 1] = es.size();
  }
  return build_index_flat(n_transcripts, tx_ref.data(), tx_strand.data(), off.data(), es.data(), ee.data(),
                          std::move(names), n_refnames, fa_by_ref, n_fasta > 0, device, out);
}

extern "C" int br_index_build_flat(size_t n_tx, const int32_t *tx_ref_id, const int8_t *tx_strand,
                                   const uint64_t *tx_exon_off, const uint32_t *ex_start, const uint32_t *ex_end,
                                   const char *const *tx_names, size_t n_refs, const br_fasta_seq *fasta_by_ref,
                                   int device, br_index **out) {
  if (!out || (n_tx && (!tx_ref_id || !tx_strand || !tx_exon_off))) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  std::vector<std::string> names(n_tx);
  for (size_t t = 0; t < n_tx; t++) names[t] = tx_names ? tx_names[t] : ("tx" + std::to_string(t));
  std::vector<const br_fasta_seq *> fa(n_refs, nullptr);
  if (fasta_by_ref) for (size_t r = 0; r < n_refs; r++) fa[r] = fasta_by_ref[r].seq ? &fasta_by_ref[r] : nullptr;
  return build_index_flat(n_tx, tx_ref_id, tx_strand, tx_exon_off, ex_start, ex_end, std::move(names), n_refs, fa,
                          fasta_by_ref != nullptr, device, out);
}

extern "C" void br_index_free(br_index *ix) {
  if (!ix) return;
  if (ix->device >= 0) {
    (void)hipSetDevice(ix->device);
    void *ptrs[] = {ix->d_slab_off, ix->d_s_start, ix->d_s_pmax, ix->d_bin_off, ix->d_t_bin, ix->d_s_tid, ix->d_s_row, ix->d_tx_ex,
                    ix->d_tx_first, ix->d_seq_pool};
    for (void *p : ptrs) if (p) (void)hipFree(p);
  }
  delete ix;
}
extern "C" size_t br_index_num_transcripts(const br_index *ix) { return ix ? ix->names.size() : 0; }
extern "C" const char *br_index_transcript_name(const br_index *ix, uint32_t tid) {
  return (ix && tid < ix->names.size()) ? ix->names[tid].c_str() : nullptr;
}
extern "C" int64_t br_index_transcript_len(const br_index *ix, uint32_t tid) {
  return (ix && tid < ix->lengths.size()) ? (int64_t)ix->lengths[tid] : -1;
}
extern "C" size_t br_index_num_refs(const br_index *ix) { return ix ? ix->n_refs : 0; }
extern "C" size_t br_index_num_intervals(const br_index *ix) { return ix ? ix->s_start.size() : 0; }
extern "C" size_t br_index_device_bytes(const br_index *ix) { return ix ? ix->device_bytes : 0; }

// ---------------------------------------------------------------------------
// configuration
// ---------------------------------------------------------------------------
extern "C" void br_config_short_read(br_config *c) { memset(c, 0, sizeof(*c)); c->junc_miss_discount = 1.0; }
extern "C" void br_config_long_read(br_config *c) { memset(c, 0, sizeof(*c)); c->lr = 1; c->junc_miss_discount = 1.0; }

// src/evaluate.cpp:1136-1221: presets (+ overrides).  The LR branch comes before
// LR_HQ, and --strict only reaches short-read runs.
extern "C" int br_config_resolve(const br_config *c, br_thresholds *t) {
  if (!c || !t) return BR_ERR_INVALID_ARG;
  if (c->junc_miss_discount != 1.0 && c->junc_miss_discount != 0.0) return BR_ERR_UNSUPPORTED;
  bool longr = c->lr || c->lr_hq;
  uint32_t mc, mji, mjg, mee; float thr;
  if (!longr) { mc = c->strict ? 0 : 5; mji = 0; mjg = 0; thr = 1.0f; mee = 0; }
  else if (c->lr) { mc = 40; mji = 40; mjg = 40; thr = (float)0.60; mee = 35; }
  else { mc = 5; mji = 10; mjg = 10; thr = (float)0.90; mee = 35; }
  if (c->has_max_clip) mc = c->max_clip;
  if (c->has_max_junc_ins) mji = c->max_junc_ins;
  if (c->has_max_junc_gap) mjg = c->max_junc_gap;
  if (c->has_sim_thr) thr = c->sim_thr;
  if (c->has_max_error_exon) mee = c->max_error_exon;
  t->max_clip = mc; t->max_junc_ins = mji; t->max_junc_gap = mjg; t->max_error_exon = mee;
  t->ignore_small_exons = mee > 0; t->similarity_threshold = thr;
  t->filter_by_similarity = thr < 1.0;
  return BR_OK;
}

int make_devcfg(const br_config *c, DevCfg &d) {
  br_thresholds t;
  int rc = br_config_resolve(c, &t);
  if (rc) return rc;
  d.max_clip = t.max_clip; d.max_junc_ins = t.max_junc_ins; d.max_junc_gap = t.max_junc_gap;
  d.max_error_exon = t.max_error_exon; d.ignore_small_exons = t.ignore_small_exons;
  d.filter_by_similarity = t.filter_by_similarity; d.long_reads = (c->lr || c->lr_hq) ? 1 : 0;
  d.use_fasta = c->use_fasta ? 1 : 0; d.fr = c->fr ? 1 : 0; d.rf = c->rf ? 1 : 0;
  d.thr = (double)t.similarity_threshold;  // float widened to double (include/evaluate.h:281)
  return BR_OK;
}

// ---------------------------------------------------------------------------
// host-side input contract: name groups + mate index
// ---------------------------------------------------------------------------
extern "C" int br_batch_prepare(const br_batch *b, int32_t *mate_idx, uint32_t *group_off, int64_t *n_groups) {
  if (!b || !mate_idx || !group_off || !n_groups) return BR_ERR_INVALID_ARG;
  int64_t n = b->n_aln;
  if (n >= 0x7fffffffll) return BR_ERR_CAPACITY;
  int64_t ng = 0;
  for (int64_t i = 0; i < n; i++) mate_idx[i] = -1;
  std::vector<std::pair<int32_t, int32_t>> open_small;  // (ref_start, index) of still-unpaired records
  std::unordered_map<int32_t, int32_t> open_big;
  int64_t i = 0;
  while (i < n) {
    int64_t j = i + 1;
    uint64_t len = b->name_off[i + 1] - b->name_off[i];
    const char *nm = b->names + b->name_off[i];
    while (j < n && b->name_off[j + 1] - b->name_off[j] == len && memcmp(b->names + b->name_off[j], nm, len) == 0) j++;
    group_off[ng++] = (uint32_t)i;
    // src/bramble.cpp:272-311 (process_pairs): key = name + '-' + start; within a
    // name group the name part is constant, so the key is the start.
    bool big = (j - i) > 32;
    open_small.clear();
    if (big) open_big.clear();
    for (int64_t k = i; k < j; k++) {
      if (!(b->flags[k] & 0x1)) continue;
      if (b->ref_id[k] != b->mate_ref_id[k]) continue;
      int32_t ms = b->mate_start[k], rs = b->ref_start[k];
      int32_t found = -1;
      if (big) {
        auto it = open_big.find(ms);
        if (it != open_big.end()) { found = it->second; open_big.erase(it); }
      } else {
        for (size_t q = 0; q < open_small.size(); q++)
          if (open_small[q].first == ms) { found = open_small[q].second; open_small.erase(open_small.begin() + q); break; }
      }
      if (found >= 0) {
        mate_idx[k] = found; mate_idx[found] = (int32_t)k;
      } else if (big) {
        open_big[rs] = (int32_t)k;
      } else {
        bool repl = false;
        for (auto &p : open_small) if (p.first == rs) { p.second = (int32_t)k; repl = true; break; }
        if (!repl) open_small.emplace_back(rs, (int32_t)k);
      }
    }
    i = j;
  }
  group_off[ng] = (uint32_t)n;
  *n_groups = ng;
  return BR_OK;
}

extern "C" int br_batch_seq_source(const br_batch *b, const uint32_t *group_off, int64_t n_groups, int32_t *seq_src) {
  if (!b || !group_off || !seq_src) return BR_ERR_INVALID_ARG;
  for (int64_t g = 0; g < n_groups; g++) {
    int32_t src = -1;
    if (b->seq_off)
      for (uint32_t i = group_off[g]; i < group_off[g + 1]; i++)
        if (b->seq_off[i + 1] > b->seq_off[i]) { src = (int32_t)i; break; }
    for (uint32_t i = group_off[g]; i < group_off[g + 1]; i++) seq_src[i] = src;
  }
  return BR_OK;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" int br_ctx_new(const br_index *ix, br_ctx **out) {
  if (!ix || !out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  if (ix->device < 0) return BR_ERR_NO_DEVICE;
  int rc = check_device(ix->device);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ix->device));
  br_ctx *c = new br_ctx();
  c->ix = ix;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, ix->device));
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIPCHK(hipHostMalloc((void **)&c->rb, sizeof(ReadBack), hipHostMallocDefault));
  memset(c->rb, 0, sizeof(ReadBack));
  const char *bl = getenv("BRAMBLE_AMD_BAM_LANES");
  if (bl) { int v = atoi(bl); if (v == 0 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) c->bam_lanes = v; }
  const char *spec = getenv("BRAMBLE_AMD_SPECULATE");      // A/B: 0 = large batches always through the ordinary pipeline (three host round trips)
  if (spec) c->speculate = atoi(spec) != 0;
  const char *dr = getenv("BRAMBLE_AMD_DIRECT_ROWS");   // A/B: 0 = the match-table path
  if (dr) c->direct_rows = atoi(dr) != 0;
  const char *g = getenv("BRAMBLE_AMD_GROUP_LANES");
  if (g) { int v = atoi(g); if (v == 8 || v == 16 || v == 32 || v == 64) c->group_lanes = v; }
  *out = c;
  return BR_OK;
}

extern "C" void br_ctx_free(br_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->ix->device);   // (the buffers are freed on this device when the context goes)
  for (auto &e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  if (c->rb) (void)hipHostFree(c->rb);
  for (auto &S : c->stage) if (S.ready) (void)hipEventDestroy(S.ready);
  for (auto &S : c->in_slot) {
    if (S.ready) (void)hipEventDestroy(S.ready);
    if (S.rows_home) (void)hipEventDestroy(S.rows_home);
  }
  if (c->rows_busy) (void)hipEventDestroy(c->rows_busy);
  if (c->alt.busy) (void)hipEventDestroy(c->alt.busy);
  if (c->side2_stream) (void)hipStreamDestroy(c->side2_stream);
  if (c->side_stream) { (void)hipStreamDestroy(c->side_stream); for (auto &p : c->side_ev) for (auto &e : p) if (e) (void)hipEventDestroy(e); }
  if (c->run_stream) (void)hipStreamDestroy(c->run_stream);
  if (c->d2h_stream) (void)hipStreamDestroy(c->d2h_stream);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
  for (int k = 0; k < 2; k++) if (c->ev_home[k]) (void)hipEventDestroy(c->ev_home[k]);
  delete c;
}

extern "C" int br_ctx_set_profiling(br_ctx *c, int enabled) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (enabled && !c->profiling) for (int k = 0; k < BR_K_NUM; k++) { c->k_ms_sum[k] = 0; c->k_launches_sum[k] = 0; }
  c->profiling = enabled != 0;
  return BR_OK;
}
extern "C" int br_ctx_kernel_ms_sum(br_ctx *c, int which, double *ms, int64_t *launches) {
  if (!c || which < 0 || which >= BR_K_NUM) return BR_ERR_INVALID_ARG;
  if (ms) *ms = c->k_ms_sum[which];
  if (launches) *launches = c->k_launches_sum[which];
  return BR_OK;
}
extern "C" int br_ctx_set_param(br_ctx *c, const char *key, int64_t v) {
  if (!c || !key) return BR_ERR_INVALID_ARG;
  if (!strcmp(key, "group_lanes")) { if (v != 8 && v != 16 && v != 32 && v != 64) return BR_ERR_INVALID_ARG; c->group_lanes = (int)v; return BR_OK; }
  if (!strcmp(key, "direct_rows")) { c->direct_rows = v != 0; return BR_OK; }
  if (!strcmp(key, "pair_bitmask")) { if (v != 0 && v != 1) return BR_ERR_INVALID_ARG; c->pair_bitmask = v != 0; return BR_OK; }
  if (!strcmp(key, "emit_rank_tids")) { if (v != 0 && v != 1) return BR_ERR_INVALID_ARG; c->emit_rank_tids = v != 0; return BR_OK; }
  if (!strcmp(key, "emit_general_preset")) { if (v != 0 && v != 1) return BR_ERR_INVALID_ARG; c->emit_general_preset = v != 0; return BR_OK; }
  if (!strcmp(key, "small_batch")) { c->small_batch = v != 0; return BR_OK; }
  if (!strcmp(key, "speculate")) { c->speculate = v != 0; return BR_OK; }
  if (!strcmp(key, "speculate_n")) { if (v < 0) return BR_ERR_INVALID_ARG; c->speculate_n = v; return BR_OK; }
  if (!strcmp(key, "small_n")) { if (v < 0) return BR_ERR_INVALID_ARG; c->small_n = v; return BR_OK; }
  if (!strcmp(key, "deflate_dynamic")) { c->deflate_dynamic = v != 0; return BR_OK; }
  if (!strcmp(key, "deflate_waves")) { if (v < 0 || v > (1 << 20)) return BR_ERR_INVALID_ARG; c->deflate_waves = (int)v; return BR_OK; }   // test hook, see deflate_device_impl
  if (!strcmp(key, "bam_lanes")) { if (v != 0 && v != 4 && v != 8 && v != 16 && v != 32 && v != 64) return BR_ERR_INVALID_ARG; c->bam_lanes = (int)v; return BR_OK; }
  if (!strcmp(key, "ksw_fast")) { c->ksw_fast = v != 0; return BR_OK; }
  if (!strcmp(key, "ksw_tape_pct")) { if (v < 0 || v > 100) return BR_ERR_INVALID_ARG; c->ksw_tape_pct = (int)v; return BR_OK; }
  if (!strcmp(key, "ksw_tape_mb")) { if (v < 1) return BR_ERR_INVALID_ARG; c->ksw_tape_mb = v; return BR_OK; }
  if (!strcmp(key, "host_detail")) { c->host_detail = v != 0; return BR_OK; }
  if (!strcmp(key, "split_spoil")) { if (v < 0 || v > 1000000) return BR_ERR_INVALID_ARG; c->split_spoil = (int)v; return BR_OK; }   // test hook, see split_impl
  if (!strcmp(key, "side_cap")) { if (v < 64) return BR_ERR_INVALID_ARG; c->d_side_cap = (uint64_t)v; return BR_OK; }   // test hook: the side arena's first capacity (entries), see run_device_direct
  // the records without an output record are kept (br_ctx_unprojected_*): 1 per record, 2 per read name; not while some are held
  if (!strcmp(key, "keep_unprojected")) { if (v < 0 || v > 2 || (c->un.n && v != c->un.keep)) return BR_ERR_INVALID_ARG; c->un.keep = (int)v; return BR_OK; }
  if (!strcmp(key, "unprojected_cap")) { if (v < 0) return BR_ERR_INVALID_ARG; c->un.first_cap = (uint64_t)v; return BR_OK; }   // test hook: their arena's first capacity (bytes)
  if (!strcmp(key, "blocks_per_cu")) { if (v < 1 || v > 64) return BR_ERR_INVALID_ARG; c->blocks_per_cu = (int)v; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}
extern "C" int br_ctx_kernel_ms(br_ctx *c, int which, double *ms, int32_t *launches) {
  if (!c || which < 0 || which >= BR_K_NUM) return BR_ERR_INVALID_ARG;
  if (ms) *ms = c->k_ms[which];
  if (launches) *launches = c->k_launches[which];
  return BR_OK;
}
// Diagnostic: how the last -S call's DP problems were routed (pieces, problems per array shape, leftovers handed to the
// general kernel before the DP, tape bytes of the largest piece, leftovers of the last piece after the DP).
extern "C" int br_ctx_ksw_diag(br_ctx *c, uint64_t out[16]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  memcpy(out, c->ksw_diag, sizeof(c->ksw_diag));
  out[7] = (uint32_t)c->rb->ksw_left_after;
  return BR_OK;
}

extern "C" int br_ctx_rescue_stats(br_ctx *c, uint64_t out[4]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  memcpy(out, c->rescue_stats, sizeof(c->rescue_stats));
  return BR_OK;
}
extern "C" int br_ctx_last_counters(br_ctx *c, uint64_t out[8]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  memcpy(out, c->counters, sizeof(c->counters));
  return BR_OK;
}

extern "C" int br_pin_host(void *p, size_t bytes) {
  if (!p || !bytes) return BR_ERR_INVALID_ARG;
  HIPCHK(hipHostRegister(p, bytes, hipHostRegisterDefault));
  return BR_OK;
}
extern "C" int br_unpin_host(void *p) {
  if (!p) return BR_ERR_INVALID_ARG;
  HIPCHK(hipHostUnregister(p));
  return BR_OK;
}

extern "C" uint32_t br_primary_pick(const char *name, size_t len, uint32_t n_tied) {
  return n_tied ? br::primary_pick((const uint8_t *)name, len, n_tied) : 0;
}

extern "C" uint32_t br_row_mapq(uint32_t nh, int long_reads) {  // src/core.cpp:46-58
  if (!long_reads) return nh == 1 ? 255u : nh == 2 ? 3u : (nh == 3 || nh == 4) ? 1u : 0u;
  return nh > 1 ? 0u : 3u;
}

// First touch of a device (runtime start-up, context creation: a few tenths of a second) -- something a caller can do on a
// thread of its own while it is busy elsewhere (the command line does, while the guides are parsed).
extern "C" int br_device_warmup(int device) {
  int rc = check_device(device);
  if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipFree(nullptr));
  return BR_OK;
}

extern "C" const char *br_version(void) { return "bramble_amd 0.3.0 (gfx950, ABI 3)"; }
extern "C" const char *br_strerror(int code) {
  switch (code) {
    case BR_OK: return "ok";
    case BR_ERR_INVALID_ARG: return "invalid argument";
    case BR_ERR_NO_DEVICE: return "no usable HIP device (the projection path has no CPU fallback)";
    case BR_ERR_HIP: return "HIP runtime error";
    case BR_ERR_ANNOTATION: return "invalid annotation";
    case BR_ERR_CAPACITY: return "batch exceeds 32-bit device offsets; split it";
    case BR_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return "unknown error";
  }
}
