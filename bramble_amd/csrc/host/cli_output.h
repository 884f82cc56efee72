// What consumes a run of the command line (cli.cpp) beside the main output: --sort (cli_output_sort.cpp), --dedup
// (cli_output_dedup.cpp), --quant (cli_output_quant.cpp), --cells (cli_output_cells.cpp), --coverage (cli_output_coverage.cpp), --unprojected (cli_output_unprojected.cpp), --quant-bam (cli_output_assign.cpp), behind one interface.  A consumer takes something from every
// projected bundle on device o.devices[0], does its device work once the input is through, writes its files (cli_output_files.h)
// and prints one report line; the runners, the writer and br_cli_main loop over the consumers and never learn which kind one is.
#pragma once
#include "cli_input.h"
#include "cli_output_files.h"

namespace brcli {

// what every consumer is made from, built once: tid = the index's transcript, its line in a file = the @SQ list's; hdr: the
// input's header (--unprojected writes its file under it)
// out_header: the main output's BAM header as it is without --sort (--quant-bam and --dedup-bam write their files under it; empty
// unless asked for)
struct RunEnv { const Options &o; int device; TxTable tx; const BamHeader &hdr; std::vector<uint8_t> out_header; };

class Consumer {
 public:
  // name: "error: <name> on device ..." (set-up), "the <name> could not take a bundle"; failure: "<failure> failed on device ..."
  Consumer(const RunEnv &env, const char *name, const char *failure) : name(name), failure(failure), env(env) {}
  virtual ~Consumer() {}   // frees the library's object
  // The runner, right after a projection call: the bundle is still where the projection left it (the context's next call comes
  // after this one).  The br_ error code, like finish()
  virtual int add(br_ctx *ctx) = 0;
  virtual int finish() = 0;   // after the last bundle: the device work, and the results come home
  // Into temporary files; false: failed, and said so.  The writer's state is for the index of what it wrote: its stream (flushed
  // by whoever needs the offset of its end) and the blocks of the record section
  virtual bool write_files(brio::BgzfWriter &wr, const std::vector<br_bgzf_span> &spans) = 0;
  virtual bool settle(bool failed) = 0;   // the run is over: SideFile::settle of every file; false: a rename failed
  virtual void report() const = 0;        // its line(s) in front of the final report
  // --sort only.  The records stay with the consumer: a projection call leaves them in HBM (BR_OUT_RESIDENT) and nothing of a
  // bundle goes to the writer; after finish() the writer draws them from next_piece (no rows: that was all)
  virtual bool keeps_records() const { return false; }
  virtual int next_piece(uint64_t, br_device_bam *piece) { memset(piece, 0, sizeof(*piece)); return BR_OK; }
  // --quant only: its quantifier, for a consumer that reads it after the quantifier's finish() (the EM has run by then)
  virtual br_quant *quantifier() { return nullptr; }
  // --dedup only: one byte per read name of the run in HBM, non-zero for a duplicate (br_dedup_flags: BR_ERR_INVALID_ARG before its
  // finish()); the --quant consumer drops those names in front of its own finish().  Every other consumer: BR_ERR_UNSUPPORTED
  virtual int duplicate_flags(const uint8_t **, int64_t *) { return BR_ERR_UNSUPPORTED; }
  // --cells with --cells-whitelist only: its whitelist and "correct", which the --dedup consumer sets on its br_dedup too
  virtual const br_whitelist *whitelist(int *) { return nullptr; }
  // once every consumer is open: one that needs another finds it among them; false: it is not there
  virtual bool meet(const std::vector<std::unique_ptr<Consumer>> &) { return true; }
  const char *const name, *const failure;
 protected:
  const RunEnv &env;
};

// nullptr: `err` is the error line
std::unique_ptr<Consumer> open_sort(const RunEnv &env, std::string &err);
std::unique_ptr<Consumer> open_quant(const RunEnv &env, std::string &err);
std::unique_ptr<Consumer> open_coverage(const RunEnv &env, std::string &err);
std::unique_ptr<Consumer> open_unprojected(const RunEnv &env, std::string &err);   // (begins its file: err is the writer's)
std::unique_ptr<Consumer> open_assign(const RunEnv &env, std::string &err);        // (likewise)
std::unique_ptr<Consumer> open_dedup(const RunEnv &env, std::string &err);         // (likewise, with --dedup-bam)
std::unique_ptr<Consumer> open_cells(const RunEnv &env, std::string &err);         // (it tries PREFIX: err may be the file's)
// (for the three above) T::open() makes the library's object and sets its parameters
template <typename T>
std::unique_ptr<Consumer> open_as(const RunEnv &env, std::string &err) {
  auto c = std::make_unique<T>(env);
  if (const int rc = c->open()) { err = std::string(c->name) + " on device " + std::to_string(env.device) + ": " + br_strerror(rc); return nullptr; }
  return c;
}

// the consumers the options ask for, in the order sort, dedup, quant, cells, coverage, unprojected, quant-bam -- the order of their finish() as well: quant
// drops the names dedup's finish() has found to be duplicates (Consumer::duplicate_flags), coverage under --coverage-weight em and
// --quant-bam read the quantifier (Consumer::quantifier) whose EM quant's finish() has run, cells its classes; false: `err` says which could not be made
inline bool open_consumers(const RunEnv &env, std::vector<std::unique_ptr<Consumer>> &out, std::string &err) {
  const Options &o = env.o;
  const std::pair<bool, decltype(&open_sort)> wanted[] = {{o.sort, open_sort}, {o.dedup >= 0, open_dedup}, {!o.quant.empty(), open_quant}, {!o.cells.empty(), open_cells}, {!o.coverage.empty() || !o.coverage_summary.empty() || !o.coverage_bigwig.empty(), open_coverage}, {!o.unprojected.empty(), open_unprojected}, {!o.quant_bam.empty(), open_assign}};
  for (auto &[want, open] : wanted) {
    if (!want) continue;
    out.push_back(open(env, err));
    if (!out.back()) return false;
  }
  for (auto &c : out) if (!c->meet(out)) { err = std::string(c->name) + ": a consumer it reads is missing"; return false; }
  return true;
}

}  // namespace brcli
