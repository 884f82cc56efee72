// --collate: the input in any order.  CollateInput wraps the source open_input picked (host BAM, device BAM, SAM): its thread
// runs that source with a private Outbox (the source's markers for chunks without records stay there), copies every bundle
// into one br_collator on the single device, and once the input has ended deals the collator's bundles of whole read-name
// groups to the device's runner in output order.  The collated records stay in the collator's arena until the run is over,
// so the bundles' release is a no-op.
#include "cli_input.h"

namespace brcli {
namespace {

class CollateInput : public DevInput {
 public:
  CollateInput(const Options &o, std::unique_ptr<Input> inner) : DevInput(o), inner(std::move(inner)) { hdr = this->inner->hdr; }
  ~CollateInput() override { if (col) br_collator_free(col); }
  bool start(Outbox &out_, std::string &err) override {
    out = &out_;
    if (!inner->start(inner_out, err)) return false;
    reader = std::thread([this] { run(); });
    return true;
  }
  void report_timing() const override {
    inner->report_timing();
    uint64_t arena = 0, peak = 0; double add_s = 0, fin_s = 0;
    if (col) (void)br_collator_stats(col, &arena, &peak, &add_s, &fin_s);
    fprintf(stderr, "[bramble] collate: %lld records in %lld read-name groups; add %.2fs (input read %.2fs), finish %.2fs; arena %.3f GB, "
            "collator peak %.3f GB of device memory\n", (long long)n_rec, (long long)n_grp, add_s, t_input, fin_s, 1e-9 * (double)arena,
            1e-9 * (double)peak);
  }
 private:
  void wake() override { inner->cancel = true; }
  // (the inner source is stopped here: the collator's bundles are done with once the runners have been joined)
  void free_readers() override { inner->stop(); if (col) br_collator_free(col); col = nullptr; }
  void run() {
    auto t0 = now();
    int rc = br_collator_new(o.devices[0], &col);
    if (rc) { set_err(std::string("--collate: ") + br_strerror(rc)); inner->cancel = true; }
    auto fail = [&](int r) {
      if (r == BR_ERR_CAPACITY) set_err("--collate: the input's mapped records do not fit in the memory of device " + std::to_string(o.devices[0]) + " (BR_ERR_CAPACITY)");
      else set_err(std::string("--collate: ") + br_strerror(r));
      inner->cancel = true;   // (the source's queue is still drained below: its threads finish)
    };
    // the whole input into the collator (after an error: only drained)
    if (Slot<Bundle> *q = inner->host_queue()) {
      while (auto b = q->take()) {
        if (cancel) inner->cancel = true;   // (a failing runner sets only this source's flag)
        else {
          br_device_records r{b->blob.data(), b->off.data(), (int64_t)b->off.size(), b->len.data()};
          rc = br_collator_add(col, &r, 0, nullptr);
          if (rc) fail(rc);
        }
        inner->recycle(*b);
      }
    } else {
      Slot<DevBundle> *dq = inner->dev_queue(0);
      while (auto b = dq->take()) {
        if (cancel) inner->cancel = true;
        else { rc = br_collator_add(col, &b->recs, 1, nullptr); if (rc) fail(rc); }
        b->release();   // (the copy is done: the reader takes its chunk back)
      }
    }
    inner->join();
    totals.reads = inner->totals.reads.load(); totals.unmapped = inner->totals.unmapped.load();
    t_inflate = inner->t_inflate; t_split = inner->t_split; t_copy = inner->t_copy;
    if (!inner->err.empty()) set_err(inner->err, inner->err_at_line);
    t_input = secs(t0, now());
    // collate, then the bundles in output order
    uint64_t k = 0;
    if (!cancel) {
      rc = br_collator_finish(col, &n_rec, &n_grp);
      if (rc) fail(rc);
      else if (!o.quiet) printf("[bramble] collated %lld records into %lld read-name groups (%.2fs)\n", (long long)n_rec, (long long)n_grp, secs(t0, now()));
    }
    while (!cancel) {
      auto b = std::make_unique<DevBundle>([](int64_t) {});
      rc = br_collator_next(col, o.bundle_records, &b->recs);
      if (rc) { fail(rc); break; }
      if (b->recs.n_aln == 0) break;
      b->seq = k++;
      to_dev[0]->put(std::move(b));
    }
    next_seq = k;
    processor_done(0, t0);
  }

  std::unique_ptr<Input> inner;
  Outbox inner_out;
  br_collator *col = nullptr;
  int64_t n_rec = 0, n_grp = 0;
  double t_input = 0;
};

}  // namespace

std::unique_ptr<Input> open_collate(const Options &o, std::unique_ptr<Input> inner) { return std::unique_ptr<Input>(new CollateInput(o, std::move(inner))); }

}  // namespace brcli
