// The inputs of the command line (cli.cpp): where bundles come from.  One source per format -- the host BAM reader, the device
// BAM readers (cli_input_bam.cpp), the SAM readers (cli_input_sam.cpp) -- behind one interface; the workers, the ordered writer
// and the report see the source's queues, its totals and its first error, never which kind it is.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/bramble_amd.h"
#include "bgzf.h"

namespace brcli {

struct Options {
  std::string in_bam, out_bam, gff, fasta;
  br_config cfg;
  int threads = 1, level = 6;
  std::vector<int> devices{0};  // --device N / --devices a,b,...: one worker (index replica + context + host threads) per entry
  int64_t bundle_records = 1000000;   // (1 M: 1.20 s inside the program for 20.9 M alignments, 2 M: 1.38 s, 0.5 M: 1.47 s; the pinned result buffers scale with it)
  bool quiet = false;
  bool device_deflate = true;   // BGZF blocks made on the GPU unless a host level is asked for
  bool sam_out = false;         // -O sam: SAM text formatted on the GPU (BR_OUT_SAM_TEXT) instead of BAM
  bool collate = false;          // --collate: the whole input is read into one device's memory and regrouped by read name first
  bool sort = false;             // --sort: the projected records stay in one device's memory and are written in coordinate order
  bool write_index = false;      // --write-index: <out>.bai beside the sorted BAM, built on the GPU
  std::string quant, quant_classes;   // --quant FILE / --quant-classes FILE: per-transcript abundances and the equivalence classes (br_quant)
  int quant_length_norm = -1;    // -1: on for the short-read preset, off under --lr / --lr-hq; --quant-length-norm / --quant-no-length-norm
  bool quant_eff_length = false; // --quant-eff-length: the fragment-length model (br_quant "eff_len"): reads weighted by 1 / effective length
  std::string quant_fld;         // --quant-fld FILE: the observed fragment-length histogram
  int quant_bootstraps = 0;      // --quant-bootstraps B: bootstrap replicates (br_quant "bootstraps"), 0: none
  long long quant_seed = 0;      // --quant-seed S: their seed (br_quant "boot_seed")
  bool quant_seed_given = false;
  std::string quant_boot_out;    // --quant-boot-out FILE: every replicate's NumReads per transcript
  bool quant_vb = false;         // --quant-vb: the variational Bayes EM (br_quant "vb")
  double quant_vb_prior = 1e-2;  // --quant-vb-prior P: its prior (br_quant_set_vb_prior; salmon's --vbPrior default)
  bool quant_vb_prior_given = false;
  bool quant_vb_per_nt = false;  // --quant-vb-per-nucleotide: the prior per nucleotide ("vb_per_nucleotide")
  std::string quant_genes, quant_gene_classes;   // --quant-genes FILE / --quant-gene-classes FILE: the gene-level table and the gene classes (br_quant_genes)
  std::string quant_gene_map;    // --quant-gene-map FILE: transcript<TAB>gene lines that replace the annotation's gene ids
  std::string coverage, coverage_summary;   // --coverage FILE / --coverage-summary FILE: the bedGraph of the depth along every transcript and the per-transcript table (br_coverage)
  bool coverage_primary = false; // --coverage-primary: only primary records count ("primary_only")
  std::string coverage_bigwig;   // --coverage-bigwig FILE: the depth as a bigWig track, built on the device (br_coverage_bigwig)
  int coverage_bigwig_zooms = 4; // --coverage-bigwig-zooms N: zoom levels, 0 .. 10
  bool coverage_bigwig_uncompressed = false;   // --coverage-bigwig-uncompressed: plain sections
  int coverage_weight = 0;       // --coverage-weight unit|nh|em: br_coverage's "weight" (0, 1, 2); em reads the --quant consumer's posteriors
  std::string unprojected;       // --unprojected FILE: the input records without an output record, as a BAM under the input's header
  int unprojected_scope = 1;     // --unprojected-scope record|name: the context's "keep_unprojected" (1, 2)
  std::string quant_bam;         // --quant-bam FILE: the projected records with the EM's posterior (ZW:f), as a BAM under the unsorted output's header
  int quant_bam_mode = 0;        // --quant-bam-mode tag|sample: br_assign's "mode" (0, 1)
  int dedup = -1;                // --dedup unique|directional: br_dedup's "method" (0, 1); -1: no duplicate removal
  int dedup_umi = 0;             // --dedup-umi name|tag: "umi_source" (0, 1)
  int dedup_umi_sep = '_';       // --dedup-umi-sep C: "umi_sep"
  int dedup_umi_tag = 'R' | 'X' << 8;   // --dedup-umi-tag XY: "umi_tag"
  std::string dedup_stats;       // --dedup-stats FILE: size<TAB>molecules, a line per non-empty bin of the histogram
  std::string dedup_bam;         // --dedup-bam FILE: the projected records without the duplicate names' (or with 0x400 on them), under the unsorted output's header
  int dedup_bam_mode = 0;        // --dedup-bam-mode remove|mark: br_dedup's "mark" (0, 1)
  std::string cells;             // --cells PREFIX: the cell x feature matrix of the run (br_cells): PREFIXmatrix.mtx, barcodes.tsv, features.tsv, cells.tsv
  int cells_barcode = 0;         // --cells-barcode name|tag: br_cells' "barcode_source" (0, 1); with --dedup its "cell_source" (1, 2)
  int cells_barcode_tag = 'C' | 'B' << 8;   // --cells-barcode-tag XY: "barcode_tag" / "cell_tag"
  int cells_features = 0;        // --cells-features gene|transcript (0, 1)
  int cells_multi = 0;           // --cells-multi unique|uniform|em: br_cells' "mode" (0, 1, 2)
  std::string cells_whitelist;   // --cells-whitelist FILE: the allowed cell barcodes (br_whitelist), one a line
  int cells_correct = 1;         // --cells-correct exact|1mm|1mm-multi: "correct" (0, 1, 2)
  int cells_filter = -1;         // --cells-filter topcells|cr2.2|emptydrops: br_cellcall's "method" (0, 1, 2); -1: the cells are not called
  long long cells_expected = 3000, cells_ed_lo = 45000, cells_ed_hi = 90000, cells_ed_umi_min = 500, cells_ed_candidates = 20000,
            cells_ed_sims = 10000;   // --cells-expected, --cells-ed-window LO,HI, --cells-ed-umi-min, --cells-ed-candidates, --cells-ed-sims
  double cells_percentile = 0.99, cells_ratio = 10.0, cells_ed_umi_frac = 0.01, cells_ed_fdr = 0.01;   // --cells-filter-percentile, -ratio, --cells-ed-umi-frac, -fdr
  int device_reader = -1;       // inflate + record split on the GPU (br_bam_reader): -1 = when the input is a regular file and one device is used
};
inline std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
inline double secs(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
template <typename T>
struct Slot {  // bounded FIFO between two pipeline stages
  explicit Slot(size_t depth = 1) : depth_(depth) {}
  std::mutex m; std::condition_variable cv; std::deque<std::unique_ptr<T>> q; bool done = false; size_t depth_;
  void put(std::unique_ptr<T> v) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return q.size() < depth_; }); q.push_back(std::move(v)); cv.notify_all(); }
  void finish() { std::unique_lock<std::mutex> l(m); done = true; cv.notify_all(); }
  std::unique_ptr<T> take() {
    std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !q.empty() || done; });
    if (q.empty()) return nullptr;
    auto v = std::move(q.front()); q.pop_front(); cv.notify_all(); return v;
  }
};
struct BamHeader { std::string text; std::vector<std::string> ref_names; std::vector<uint32_t> ref_lens; };
// records in host memory (the host reader's): the workers stage them to their devices
struct Bundle { brio::ByteBuf blob; std::vector<uint64_t> off; std::vector<uint32_t> len; uint64_t seq = 0; };
// records a device's reader made in that device's HBM.  The bundle owns the reader's chunk behind `id` and hands it back
// exactly once: at release(), or when it is dropped (an error path, a drain) -- its reader must outlive it
class DevBundle {
 public:
  explicit DevBundle(std::function<void(int64_t)> rel) : rel_(std::move(rel)) {}
  DevBundle(DevBundle &&x) noexcept : recs(x.recs), id(x.id), seq(x.seq), rel_(std::move(x.rel_)) { x.id = -1; }
  ~DevBundle() { release(); }
  void release() { if (id >= 0) rel_(id); id = -1; }
  br_device_records recs{}; int64_t id = -1; uint64_t seq = 0;
 private:
  std::function<void(int64_t)> rel_;
};

struct OutChunk { const uint8_t *data; uint64_t n; int worker; };   // worker -1: a chunk without records, nothing to write
// the ordered writer's inbox: results arrive tagged with their bundle's sequence number and leave in that order
struct Outbox {
  std::mutex m; std::condition_variable cv; std::map<uint64_t, OutChunk> map; uint64_t next = 0; bool done = false;
  void put(uint64_t seq, const OutChunk &c) { { std::lock_guard<std::mutex> l(m); map[seq] = c; } cv.notify_all(); }
  void finish() { { std::lock_guard<std::mutex> l(m); done = true; } cv.notify_all(); }
  bool take(OutChunk &c) {   // false: finished, and the next chunk never came (a worker failed)
    std::unique_lock<std::mutex> l(m);
    cv.wait(l, [&] { return map.count(next) || done; });
    auto it = map.find(next);
    if (it == map.end()) return false;
    c = it->second; map.erase(it); next++;
    return true;
  }
};
struct ReadTotals {
  std::atomic<uint64_t> reads{0}, unmapped{0};
  void add(int64_t n_aln, int64_t n_unmapped) { reads += (uint64_t)(n_aln + n_unmapped); unmapped += (uint64_t)n_unmapped; }
};

// A source of bundles.  start() runs its threads (false: none was started, `err` says why).  The workers take bundles from
// host_queue() (host records, one queue for every worker) or from dev_queue(d) (device d's own); the writer learns from
// next_seq, once join() has returned, how many chunks there were.  stop() cancels, drains the queues, joins and frees the
// readers; it may come again, or after join().
class Input {
 public:
  explicit Input(const Options &o) : o(o) {}
  virtual ~Input() {}
  virtual bool start(Outbox &out, std::string &err) = 0;
  virtual Slot<Bundle> *host_queue() { return nullptr; }
  virtual Slot<DevBundle> *dev_queue(size_t) { return nullptr; }
  virtual void recycle(Bundle &) {}   // a projected bundle's buffer, back to the reader that made it
  virtual void report_timing() const = 0;   // its BRAMBLE_AMD_TIMING line
  void join() { if (reader.joinable()) reader.join(); for (auto &t : threads) if (t.joinable()) t.join(); }
  // (only a started source drains: a queue whose producer never ran is never finished, and taking from it waits for ever)
  void stop() { cancel = true; wake(); if (reader.joinable()) drain(); join(); free_readers(); }
  BamHeader hdr;
  std::atomic<bool> cancel{false};   // a failing worker sets it too: the source stops making bundles nobody will project
  ReadTotals totals;
  uint64_t next_seq = 0;
  std::string err; bool err_at_line = false;   // the first error; at_line: it is "<line>: <reason>" (a malformed SAM line)
  double t_inflate = 0, t_split = 0, t_copy = 0;   // the host reader's stages, for the report
 protected:
  // the first error wins; it cancels the run and wakes the source's waiting threads
  void set_err(const std::string &m, bool at_line = false) {
    { std::lock_guard<std::mutex> l(err_m); if (err.empty()) { err = m; err_at_line = at_line; } cancel = true; }
    wake();
  }
  virtual void wake() {}
  virtual void drain() = 0;
  virtual void free_readers() {}
  const Options &o;
  std::mutex err_m;
  std::thread reader;                 // the reader (host BAM), the feeder (SAM), the wait for the block table (device BAM)
  std::vector<std::thread> threads;   // the per-device threads
};

// the sources that make their bundles on the devices: one queue per device, for that device's runner
class DevInput : public Input {
 public:
  explicit DevInput(const Options &o) : Input(o) { for (size_t d = 0; d < o.devices.size(); d++) to_dev.emplace_back(new Slot<DevBundle>(64)); }
  Slot<DevBundle> *dev_queue(size_t d) override { return to_dev[d].get(); }
 protected:
  void drain() override { for (auto &q : to_dev) while (q->take()) {} }
  // a processed chunk: its reads count; one without alignments goes to the writer as nothing to write, the rest to device d's runner
  void hand_over(size_t d, std::unique_ptr<DevBundle> b, int64_t n_unmapped) {
    totals.add(b->recs.n_aln, n_unmapped);
    if (b->recs.n_aln == 0) { b->release(); out->put(b->seq, OutChunk{nullptr, 0, -1}); return; }
    to_dev[d]->put(std::move(b));
  }
  void processor_done(size_t d, std::chrono::steady_clock::time_point t0) {
    to_dev[d]->finish();
    const double t = secs(t0, now());
    std::lock_guard<std::mutex> l(err_m); t_dev_reader = std::max(t_dev_reader, t);
  }
  std::vector<std::unique_ptr<Slot<DevBundle>>> to_dev;
  Outbox *out = nullptr;
  double t_dev_reader = 0;   // the longest processing thread
};

// BAM or SAM, decided by the bytes, not the name (htslib's hts_open does the same for the reference); nullptr: `err` says why
std::unique_ptr<Input> open_input(const Options &o, std::string &err);
// stream_fd >= 0: a stream open_input has begun to read (peek = its first bytes); else the regular file at o.in_bam
std::unique_ptr<Input> open_sam(const Options &o, int stream_fd, const std::string &peek, std::string &err);
// --collate: `inner` (what open_input opened) read whole into a br_collator on o.devices[0], its read-name groups dealt from there
std::unique_ptr<Input> open_collate(const Options &o, std::unique_ptr<Input> inner);

}  // namespace brcli
