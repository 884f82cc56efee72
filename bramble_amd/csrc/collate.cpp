// br_collator: the mapped records of a whole input in one device's HBM, regrouped by read name (collate_kernels.hip).
//
//   add      records of a bundle (device: a reader's chunk; host: a split BAM section) are appended, compacted, to one
//            arena as [block_size][record]; the input-order tables off_in / len_in grow with it.  A device bundle is
//            copied on the collator's stream and the call returns once the copy is done: the caller may release it.
//   finish   key (64-bit name hash, masked to hash_bits) -> stable LSD radix sort of (key, input index), the digits that
//            are constant over all keys skipped -> group starts; equal keys with different names (collisions) are sorted by
//            name on the host, only those runs -> each group placed at the scanned size of the groups whose first record
//            comes earlier -> the permuted offset table (out_off / out_len / out_idx) and the group starts in output order
//   next     bundles of whole groups: [cur, first group start >= cur + max_records), one read-back each
//
// Device memory (n records, R arena bytes = sum of 4 + block_size): add holds R + 12 n (and, while the arena grows, the old
// arena beside the new one); finish adds keys 2 x 8 n, indices 2 x 4 n, head counts 8 n, the permuted tables 12 n, marks
// 8 n and the radix histograms (2 KiB a tile of 2048), so its peak is R + 64 n; afterwards R + 24 n stay until free.  The
// tables of one call are under a guard (accum.h): a finish that fails drops them as well, and the count is what is held.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bramble_amd.h"
#include "accum.h"
#include "collate_kernels.h"
#include "scan_kernels.h"

using namespace br;

struct br_collator : Accum {
  int hash_bits = 64;
  uint64_t max_bytes = 0;     // 0: no cap but the device's memory
  bool finished = false;
  int64_t n = 0, groups = 0, cur = 0;
  uint64_t used = 0;          // arena bytes in use
  double add_s = 0, finish_s = 0;
  ColBuf arena, off_in, len_in;         // input order
  ColBuf out_off, out_len, out_idx, starts;   // output order; starts: G + 1 group starts
  ColBuf tmp, small;
};

extern "C" void br_collator_free(br_collator *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_collator_new(int device, br_collator **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  br_collator *c = new br_collator();
  int rc = c->open(device);
  if (!rc) rc = c->alloc(c->small, 64);
  if (rc) { br_collator_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_collator_set_param(br_collator *c, const char *name, int64_t value) {
  if (!c || !name || c->n || c->finished) return BR_ERR_INVALID_ARG;
  if (!strcmp(name, "hash_bits")) { if (value < 0 || value > 64) return BR_ERR_INVALID_ARG; c->hash_bits = (int)value; return BR_OK; }
  if (!strcmp(name, "max_bytes")) { if (value < 0) return BR_ERR_INVALID_ARG; c->max_bytes = (uint64_t)value; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

// room for m more records of `bytes` arena bytes
static int col_reserve(br_collator *c, int64_t m, uint64_t bytes) {
  if ((uint64_t)(c->n + m) >= (1ull << 32)) return BR_ERR_CAPACITY;   // (32-bit input indices)
  const uint64_t need = c->used + bytes;
  if (c->max_bytes && need > c->max_bytes) return BR_ERR_CAPACITY;
  if (need + 64 > c->arena.cap) {
    uint64_t want = std::max<uint64_t>(need + 64, c->arena.cap + c->arena.cap / 2);
    if (c->max_bytes) want = std::min<uint64_t>(want, c->max_bytes + 64);
    RC(c->alloc(c->arena, (size_t)want, true));
  }
  const size_t rn = (size_t)(c->n + m);
  if (rn * 8 > c->off_in.cap) {
    const size_t want = std::max(rn, (size_t)(c->off_in.cap / 8) * 3 / 2);
    RC(c->alloc(c->off_in, want * 8, true)); RC(c->alloc(c->len_in, want * 4, true));
  }
  return BR_OK;
}

static int col_add_device(br_collator *c, const br_device_records *r, hipStream_t caller) {
  const int64_t m = r->n_aln;
  hipStream_t st = c->st;
  RC(c->after(caller));   // after whatever made the records
  RC(c->alloc(c->tmp, (size_t)(m + 1) * 8 + scan_scratch_bytes(m)));
  uint64_t *bytes = c->tmp.as<uint64_t>(), *scan_tmp = bytes + m + 1;
  launch_col_lens(st, r->rec_off, r->rec_len, m, bytes);
  launch_scan(st, bytes, m, scan_tmp);
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, bytes + m, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  RC(col_reserve(c, m, total));
  launch_col_copy(st, r->blob, r->rec_off, r->rec_len, m, bytes, c->used, c->arena.as<uint8_t>(), c->off_in.as<uint64_t>() + c->n,
                  c->len_in.as<uint32_t>() + c->n);
  HIPCHK(hipStreamSynchronize(st));   // the caller's chunk may go back to its reader now
  c->used += total; c->n += m;
  return BR_OK;
}

static int col_add_host(br_collator *c, const br_device_records *r) {
  const int64_t m = r->n_aln;
  std::vector<uint64_t> off((size_t)m);
  std::vector<uint32_t> len((size_t)m);
  uint64_t total = 0;
  for (int64_t i = 0; i < m; i++) {
    const uint32_t l = r->rec_len ? r->rec_len[i] : (uint32_t)(r->rec_off[i + 1] - r->rec_off[i]);
    if (r->rec_off[i] < 4) return BR_ERR_INVALID_ARG;
    len[(size_t)i] = l; off[(size_t)i] = c->used + total + 4;
    total += 4 + (uint64_t)l;
  }
  RC(col_reserve(c, m, total));
  std::vector<uint8_t> img((size_t)total);
  uint64_t p = 0;
  for (int64_t i = 0; i < m; i++) { memcpy(img.data() + p, r->blob + r->rec_off[i] - 4, 4 + (size_t)len[(size_t)i]); p += 4 + len[(size_t)i]; }
  hipStream_t st = c->st;
  if (total) HIPCHK(hipMemcpyAsync(c->arena.as<uint8_t>() + c->used, img.data(), (size_t)total, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->off_in.as<uint64_t>() + c->n, off.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->len_in.as<uint32_t>() + c->n, len.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  c->used += total; c->n += m;
  return BR_OK;
}

extern "C" int br_collator_add(br_collator *c, const br_device_records *recs, int on_device, void *stream) {
  if (!c || !recs || recs->n_aln < 0 || (recs->n_aln && (!recs->blob || !recs->rec_off)) || c->finished) return BR_ERR_INVALID_ARG;
  if (recs->n_aln == 0) return BR_OK;
  ScopeTimer timer(&c->add_s);
  HIPCHK(hipSetDevice(c->device));
  return on_device ? col_add_device(c, recs, (hipStream_t)stream) : col_add_host(c, recs);
}

// collisions: the runs of equal keys whose names differ are sorted by name on the host (stable: input order inside a name)
static int col_resolve(br_collator *c, uint32_t *idx, std::vector<uint64_t> runs) {
  std::vector<std::pair<uint64_t, uint64_t>> rs;
  for (size_t k = 0; k + 1 < runs.size(); k += 2) rs.emplace_back(runs[k], runs[k + 1]);
  std::sort(rs.begin(), rs.end());
  rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
  size_t m = 0;
  for (auto &r : rs) m += (size_t)(r.second - r.first);
  std::vector<uint32_t> members(m);
  size_t p = 0;
  for (auto &r : rs) {
    HIPCHK(hipMemcpyAsync(members.data() + p, idx + r.first, (size_t)(r.second - r.first) * 4, hipMemcpyDeviceToHost, c->st));
    p += (size_t)(r.second - r.first);
  }
  ColBuf list, slots;
  DropGuard dropper{c, {&list, &slots}};
  RC(c->alloc(list, m * 4)); RC(c->alloc(slots, m * 256));
  HIPCHK(hipMemcpyAsync(list.p, members.data(), m * 4, hipMemcpyHostToDevice, c->st));
  launch_col_names(c->st, c->arena.as<uint8_t>(), c->off_in.as<uint64_t>(), list.as<uint32_t>(), (int64_t)m, slots.as<uint8_t>());
  std::vector<uint8_t> names(m * 256);
  HIPCHK(hipMemcpyAsync(names.data(), slots.p, m * 256, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->drop(list); c->drop(slots);   // (before the host's sort, not after it)
  p = 0;
  std::vector<size_t> ord;
  std::vector<uint32_t> sorted(m);
  for (auto &r : rs) {
    const size_t len = (size_t)(r.second - r.first);
    ord.resize(len);
    for (size_t k = 0; k < len; k++) ord[k] = p + k;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
      const uint8_t *x = names.data() + a * 256, *y = names.data() + b * 256;
      if (x[0] != y[0]) return x[0] < y[0];
      return memcmp(x + 1, y + 1, x[0]) < 0;
    });
    for (size_t k = 0; k < len; k++) sorted[p + k] = members[ord[k]];
    HIPCHK(hipMemcpyAsync(idx + r.first, sorted.data() + p, len * 4, hipMemcpyHostToDevice, c->st));
    p += len;
  }
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

static int col_finish(br_collator *c) {
  hipStream_t st = c->st;
  const int64_t n = c->n;
  const size_t n1 = (size_t)n + 1;
  ColBuf key[2], idx[2], hc, mark, runs;
  DropGuard dropper{c, {&key[0], &key[1], &idx[0], &idx[1], &hc, &mark, &runs}};   // (what finish keeps is swapped out of them)
  RC(c->alloc(key[0], n1 * 8)); RC(c->alloc(key[1], n1 * 8)); RC(c->alloc(idx[0], n1 * 4)); RC(c->alloc(idx[1], n1 * 4));
  RC(c->alloc(c->tmp, scan_tmp_bytes(n)));
  uint64_t *small = c->small.as<uint64_t>();
  const uint64_t mask = c->hash_bits >= 64 ? ~0ull : (1ull << c->hash_bits) - 1;
  launch_col_key(st, c->arena.as<uint8_t>(), c->off_in.as<uint64_t>(), n, mask, key[0].as<uint64_t>(), idx[0].as<uint32_t>(),
                 c->tmp.as<uint64_t>(), small);
  uint64_t bits[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(bits, small, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int cur = 0;
  RC(c->radix_sort(key, idx, n, bits, c->tmp, &cur));
  const uint64_t *K = key[cur].as<uint64_t>();
  uint32_t *I = idx[cur].as<uint32_t>();
  uint64_t *head = key[cur ^ 1].as<uint64_t>();
  // group starts; runs with collisions are sorted by name and the starts found again
  uint64_t run_cap = 4096;
  for (bool resolved = false;;) {
    RC(c->alloc(runs, (size_t)run_cap * 16));
    HIPCHK(hipMemsetAsync(small + 2, 0, 16, st));
    launch_col_heads(st, c->arena.as<uint8_t>(), c->off_in.as<uint64_t>(), K, I, n, head, (unsigned long long *)(small + 2),
                     (unsigned long long *)(small + 3), runs.as<uint64_t>(), run_cap);
    uint64_t cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, small + 2, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cnt[0] == 0 || resolved) break;   // (after the resolution the pairs it counts are the name changes inside a run)
    if (cnt[1] > run_cap) { run_cap = cnt[1]; continue; }   // the list was short: once more with room for every entry
    std::vector<uint64_t> h((size_t)cnt[1] * 2);
    HIPCHK(hipMemcpyAsync(h.data(), runs.p, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    RC(col_resolve(c, I, std::move(h)));
    resolved = true;
  }
  c->drop(runs);
  // place
  launch_scan(st, head, n, c->tmp.as<uint64_t>());   // head -> group ids (exclusive), head[n] = G
  uint64_t G = 0;
  HIPCHK(hipMemcpyAsync(&G, head + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t *gbeg = key[cur].as<uint64_t>();   // (the sorted keys are done with)
  launch_col_gbeg(st, head, n, gbeg);
  RC(c->alloc(hc, n1 * 8));
  HIPCHK(hipMemsetAsync(hc.p, 0, n1 * 8, st));
  launch_col_head_count(st, gbeg, I, (int64_t)G, hc.as<uint64_t>());
  launch_scan(st, hc.as<uint64_t>(), n, c->tmp.as<uint64_t>());
  RC(c->alloc(c->out_off, n1 * 8)); RC(c->alloc(c->out_len, n1 * 4)); RC(c->alloc(mark, n1 * 8));
  uint32_t *out_idx = idx[cur ^ 1].as<uint32_t>();
  launch_col_place(st, head, gbeg, hc.as<uint64_t>(), I, c->off_in.as<uint64_t>(), c->len_in.as<uint32_t>(), n, c->out_off.as<uint64_t>(),
                   c->out_len.as<uint32_t>(), out_idx, mark.as<uint64_t>());
  launch_scan(st, mark.as<uint64_t>(), n, c->tmp.as<uint64_t>());
  launch_col_starts(st, mark.as<uint64_t>(), n, hc.as<uint64_t>());
  HIPCHK(hipStreamSynchronize(st));
  std::swap(c->starts, hc);
  std::swap(c->out_idx, idx[cur ^ 1]);
  for (auto *b : {&c->off_in, &c->len_in, &c->tmp}) c->drop(*b);
  c->groups = (int64_t)G;
  return BR_OK;
}

extern "C" int br_collator_finish(br_collator *c, int64_t *n_records, int64_t *n_groups) {
  if (!c || c->finished) return BR_ERR_INVALID_ARG;
  const ScopeTimer timer;
  HIPCHK(hipSetDevice(c->device));
  if (c->n) RC(col_finish(c));
  c->finished = true;
  c->finish_s = timer.seconds();
  if (n_records) *n_records = c->n;
  if (n_groups) *n_groups = c->groups;
  return BR_OK;
}

extern "C" int br_collator_next(br_collator *c, int64_t max_records, br_device_records *bundle) {
  if (!c || !bundle || max_records < 1 || !c->finished) return BR_ERR_INVALID_ARG;
  memset(bundle, 0, sizeof(*bundle));
  if (c->cur >= c->n) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  uint64_t end = (uint64_t)c->n;
  if ((uint64_t)c->cur + (uint64_t)max_records < (uint64_t)c->n) {
    uint64_t *res = c->small.as<uint64_t>() + 4;
    launch_col_cut(c->st, c->starts.as<uint64_t>(), c->groups, (uint64_t)c->cur + (uint64_t)max_records, res);
    HIPCHK(hipMemcpyAsync(&end, res, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  bundle->blob = c->arena.as<uint8_t>();
  bundle->rec_off = c->out_off.as<uint64_t>() + c->cur;
  bundle->rec_len = c->out_len.as<uint32_t>() + c->cur;
  bundle->n_aln = (int64_t)end - c->cur;
  c->cur = (int64_t)end;
  return BR_OK;
}

extern "C" int br_collator_order(const br_collator *c, int64_t *order) {
  if (!c || !c->finished || (!order && c->n)) return BR_ERR_INVALID_ARG;
  if (!c->n) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint32_t> o((size_t)c->n);
  HIPCHK(hipMemcpyAsync(o.data(), c->out_idx.p, o.size() * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (size_t i = 0; i < o.size(); i++) order[i] = o[i];
  return BR_OK;
}

extern "C" int br_collator_stats(const br_collator *c, uint64_t *arena_bytes, uint64_t *peak_bytes, double *add_seconds, double *finish_seconds) {
  if (!c) return BR_ERR_INVALID_ARG;
  if (arena_bytes) *arena_bytes = c->used;
  if (peak_bytes) *peak_bytes = c->peak;
  if (add_seconds) *add_seconds = c->add_s;
  if (finish_seconds) *finish_seconds = c->finish_s;
  return BR_OK;
}
