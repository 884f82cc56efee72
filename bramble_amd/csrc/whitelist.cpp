// br_whitelist: the allowed cell barcodes in one device's HBM, and the resolution of observed barcodes against them
// (whitelist_kernels.hip; the definitions are in bramble_amd.h).
//
//   new       the barcodes as words in comparison order, uploaded; sorted by (length, bytes) with the field sort's five stable radix
//             passes (barcode_sort.h), cut into the distinct entries by its head flags and a scan; the entries inserted into an
//             open-addressing table of 64-bit slots (a power of two >= 2 W, 64 at least).  Read-only from then on: one object serves
//             any number of accumulators on its device
//   resolve   (wl_resolve: br_cells_finish, br_dedup_finish and br_whitelist_match call it on their own tables, on their own stream)
//             the names with a barcode compacted, sorted and cut the same way into D distinct observed barcodes; one probe each
//             (k_wl_exact), which also leaves count[entry]; with "correct" 1 or 2 the ones that missed listed by a scan and a wave
//             each over their one-byte variants (k_wl_near); a lane per name writes its status and its barcode (k_wl_apply)
//
// Device memory (W barcodes given, E distinct, S slots; N names, n of them with a barcode, D distinct observed, m of them missed): the
// object keeps 33 E + 8 S and 128 bytes of counters; while it is built 33 W more and the sort's 24 W + 8 W of flags.  A resolve holds
// 8 N of flags, then 24 n (two key / index pairs) + 8 n (heads), 8 D + 4 D + 8 D (begins, entries, the missed flags) + 4 m and 8 E
// for count, plus the scans' scratch and 128 bytes of counters.  All of it is dropped before the caller goes on.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "accum.h"
#include "barcode_sort.h"
#include "collate_kernels.h"
#include "scan_kernels.h"
#include "whitelist.h"
#include "whitelist_kernels.h"

using namespace br;

struct br_whitelist : Accum {
  int hash_bits = 64;
  uint64_t n_given = 0, n_entries = 0, n_slots = 0, chain = 0;
  double build_s = 0;
  ColBuf small, cb, len, slots;
  WlTable table() const {
    WlTable T{};
    T.slots = slots.as<uint64_t>(); T.n_slots = n_slots; T.mask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1;
    T.cb = cb.as<uint64_t>(); T.len = len.as<uint8_t>(); T.n_entries = (int64_t)n_entries;
    return T;
  }
};

int br::wl_device(const br_whitelist *wl) { return wl->device; }

// n x 32 bytes -> the words that hold them in comparison order (the bytes past a barcode's length are taken as 0)
static void words_of(const uint8_t *cb, const uint8_t *len, int64_t n, std::vector<uint64_t> &words) {
  words.assign((size_t)n * 4, 0);
  for (int64_t i = 0; i < n; i++)
    for (uint32_t b = 0; b < len[i]; b++) words[(size_t)i * 4 + (b >> 3)] |= (uint64_t)cb[(size_t)i * 32 + b] << (56 - 8 * (b & 7));
}

static int wl_build(br_whitelist *c, const uint8_t *cb, const uint8_t *len, int64_t n) {
  hipStream_t st = c->st;
  uint64_t *small = c->small.as<uint64_t>();
  std::vector<uint64_t> words;
  words_of(cb, len, n, words);
  ColBuf raw, rawlen, head, tmp;
  SortBufs s;
  DropGuard bufs{c, {&raw, &rawlen, &head, &tmp, &s.key[0], &s.key[1], &s.idx[0], &s.idx[1]}};
  const size_t n1 = (size_t)n + 1;
  RC(c->alloc(raw, n1 * 32)); RC(c->alloc(rawlen, n1)); RC(s.make(c, (size_t)n)); RC(c->alloc(head, n1 * 8));
  HIPCHK(hipMemcpyAsync(raw.p, words.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(rawlen.p, len, (size_t)n, hipMemcpyHostToDevice, st));
  // every barcode is an item: flags of 1, scanned, give the identity index
  HIPCHK(hipMemsetAsync(head.p, 0, n1 * 8, st));
  launch_wl_flag(st, rawlen.as<uint8_t>(), n, head.as<uint64_t>(), nullptr);
  uint64_t all = 0;
  RC(c->scan_total(head, n, tmp, &all));
  if (all != (uint64_t)n) return BR_ERR_HIP;
  launch_bc_compact(st, head.as<uint64_t>(), n, s.idx[0].as<uint32_t>());
  RC(sort_by_barcode(c, s, raw.as<uint64_t>(), rawlen.as<uint8_t>(), nullptr, n, tmp, small + WL_BITS));
  launch_bc_heads(st, s.idx[0].as<uint32_t>(), raw.as<uint64_t>(), rawlen.as<uint8_t>(), nullptr, 0, n, head.as<uint64_t>());
  uint64_t E = 0;
  RC(c->scan_total(head, n, tmp, &E));
  if (E == 0 || E > (uint64_t)n) return BR_ERR_HIP;
  RC(c->alloc(c->cb, ((size_t)E + 1) * 32)); RC(c->alloc(c->len, (size_t)E + 1));
  launch_wl_gather(st, head.as<uint64_t>(), s.idx[0].as<uint32_t>(), n, raw.as<uint64_t>(), rawlen.as<uint8_t>(), c->cb.as<uint64_t>(), c->len.as<uint8_t>());
  uint64_t S = (uint64_t)WL_MIN_SLOTS;
  while (S < 2 * (uint64_t)n) S <<= 1;
  RC(c->alloc(c->slots, (size_t)S * 8));
  HIPCHK(hipMemsetAsync(c->slots.p, 0, (size_t)S * 8, st));
  HIPCHK(hipMemsetAsync(small + WL_FULL, 0, 2 * 8, st));   // WL_FULL, WL_CHAIN
  c->n_entries = E; c->n_slots = S;
  launch_wl_insert(st, c->table(), c->slots.as<uint64_t>(), c->small.as<unsigned long long>());
  uint64_t got[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(got, small + WL_FULL, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (got[0]) return BR_ERR_HIP;   // (an entry found no slot)
  c->chain = got[1];
  return BR_OK;
}

extern "C" void br_whitelist_free(br_whitelist *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_whitelist_new(int device, const uint8_t *cb, const uint8_t *len, int64_t n, int hash_bits, br_whitelist **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  if (!cb || !len || n <= 0 || n >= (1ll << 31) || hash_bits < 0 || hash_bits > 64) return BR_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; i++) if (len[i] == 0 || len[i] > 32) return BR_ERR_INVALID_ARG;
  br_whitelist *c = new br_whitelist();
  const ScopeTimer timer;
  int rc = c->open(device, c->small, WL_WORDS);
  c->hash_bits = hash_bits ? hash_bits : 64;
  c->n_given = (uint64_t)n;
  if (!rc) rc = wl_build(c, cb, len, n);
  if (rc) { br_whitelist_free(c); return rc; }
  c->build_s = timer.seconds();
  *out = c;
  return BR_OK;
}

extern "C" int br_whitelist_barcodes(br_whitelist *c, int64_t first, int64_t n, uint8_t *cb, uint8_t *len) {
  if (!c || !in_range(c->n_entries, first, n)) return BR_ERR_INVALID_ARG;
  return c->fetch_fields(c->cb, c->len, first, n, cb, len);
}

extern "C" int br_whitelist_stats(const br_whitelist *c, uint64_t out[8]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  const uint64_t v[8] = {c->n_given, c->n_entries, c->n_slots, c->chain, (uint64_t)(c->build_s * 1e6), (uint64_t)c->hash_bits, c->live, c->peak};
  memcpy(out, v, sizeof(v));
  return BR_OK;
}

int br::wl_stats(const WlResolved &r, int correct, uint64_t out[8]) {
  if (!out) return BR_ERR_INVALID_ARG;
  const uint64_t v[8] = {r.status[0], r.status[1], r.status[2], r.status[3], r.status[4], r.distinct, (uint64_t)(r.seconds * 1e6), (uint64_t)correct};
  memcpy(out, v, sizeof(v));
  return BR_OK;
}

int br::wl_resolve(Accum *c, const br_whitelist *wl, int correct, uint64_t *cb, uint8_t *cblen, int64_t N, uint8_t *status, uint32_t *entry, WlResolved *out) {
  const ScopeTimer timer;
  hipStream_t st = c->st;
  *out = WlResolved{};
  if (N <= 0) return BR_OK;
  const WlTable T = wl->table();
  ColBuf small, flag, tmp, head, obeg, obs_entry, miss, list, count;
  SortBufs s;
  DropGuard bufs{c, {&small, &flag, &tmp, &head, &obeg, &obs_entry, &miss, &list, &count, &s.key[0], &s.key[1], &s.idx[0], &s.idx[1]}};
  RC(c->alloc(small, WL_WORDS * 8));
  HIPCHK(hipMemsetAsync(small.p, 0, WL_WORDS * 8, st));
  HIPCHK(hipMemsetAsync(status, 0, (size_t)N, st));
  // the names with a barcode
  uint64_t M = 0;
  RC(c->alloc(flag, ((size_t)N + 1) * 8));
  launch_wl_flag(st, cblen, N, flag.as<uint64_t>(), entry);
  RC(c->scan_total(flag, N, tmp, &M));
  if (M > (uint64_t)N) return BR_ERR_HIP;
  out->status[0] = (uint64_t)N - M;
  if (M == 0) { out->seconds = timer.seconds(); return BR_OK; }
  const int64_t n = (int64_t)M;
  RC(s.make(c, (size_t)M));
  launch_bc_compact(st, flag.as<uint64_t>(), N, s.idx[0].as<uint32_t>());
  HIPCHK(hipStreamSynchronize(st));
  c->drop(flag);
  // the distinct observed barcodes
  RC(sort_by_barcode(c, s, cb, cblen, nullptr, n, tmp, small.as<uint64_t>() + WL_BITS));
  uint64_t D = 0;
  RC(c->alloc(head, ((size_t)M + 1) * 8));
  launch_bc_heads(st, s.idx[0].as<uint32_t>(), cb, cblen, nullptr, 0, n, head.as<uint64_t>());
  RC(c->scan_total(head, n, tmp, &D));
  if (D == 0 || D > M) return BR_ERR_HIP;
  out->distinct = D;
  for (int k = 0; k < 2; k++) c->drop(s.key[k]);
  c->drop(s.idx[1]);
  const size_t d1 = (size_t)D + 1;
  RC(c->alloc(obeg, d1 * 8)); RC(c->alloc(obs_entry, d1 * 4)); RC(c->alloc(miss, d1 * 8)); RC(c->alloc(count, ((size_t)T.n_entries + 1) * 8));
  launch_col_gbeg(st, head.as<uint64_t>(), n, obeg.as<uint64_t>());
  HIPCHK(hipMemsetAsync(count.p, 0, ((size_t)T.n_entries + 1) * 8, st));
  launch_wl_exact(st, T, s.idx[0].as<uint32_t>(), obeg.as<uint64_t>(), (int64_t)D, cb, cblen, obs_entry.as<uint32_t>(), count.as<uint64_t>(), miss.as<uint64_t>());
  if (correct) {
    uint64_t m = 0;
    RC(c->scan_total(miss, (int64_t)D, tmp, &m));
    if (m > D) return BR_ERR_HIP;
    if (m) {
      RC(c->alloc(list, ((size_t)m + 1) * 4));
      launch_bc_compact(st, miss.as<uint64_t>(), (int64_t)D, list.as<uint32_t>());
      launch_wl_near(st, T, list.as<uint32_t>(), (int64_t)m, s.idx[0].as<uint32_t>(), obeg.as<uint64_t>(), cb, cblen, count.as<uint64_t>(), correct,
                     obs_entry.as<uint32_t>());
    }
  }
  launch_wl_apply(st, T, head.as<uint64_t>(), s.idx[0].as<uint32_t>(), n, obs_entry.as<uint32_t>(), cb, cblen, status, entry, small.as<unsigned long long>());
  uint64_t got[5] = {0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(got, small.as<uint64_t>() + WL_STATUS, sizeof(got), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (got[1] + got[2] + got[3] + got[4] != M) return BR_ERR_HIP;
  for (int k = 1; k <= 4; k++) out->status[k] = got[k];
  out->seconds = timer.seconds();
  return BR_OK;
}

extern "C" int br_whitelist_match(br_whitelist *c, const uint8_t *cb, const uint8_t *len, int64_t n, int correct, uint32_t *entry, uint8_t *status) {
  if (!c || n < 0 || correct < 0 || correct > 2 || n >= (1ll << 32) || (n && (!cb || !len))) return BR_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; i++) if (len[i] > 32) return BR_ERR_INVALID_ARG;
  if (n == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint64_t> words;
  words_of(cb, len, n, words);
  ColBuf d_cb, d_len, d_status, d_entry;
  DropGuard bufs{c, {&d_cb, &d_len, &d_status, &d_entry}};
  const size_t n1 = (size_t)n + 1;
  RC(c->alloc(d_cb, n1 * 32)); RC(c->alloc(d_len, n1)); RC(c->alloc(d_status, n1)); RC(c->alloc(d_entry, n1 * 4));
  HIPCHK(hipMemcpyAsync(d_cb.p, words.data(), (size_t)n * 32, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(d_len.p, len, (size_t)n, hipMemcpyHostToDevice, c->st));
  WlResolved r;
  RC(wl_resolve(c, c, correct, d_cb.as<uint64_t>(), d_len.as<uint8_t>(), n, d_status.as<uint8_t>(), d_entry.as<uint32_t>(), &r));
  if (entry) HIPCHK(hipMemcpyAsync(entry, d_entry.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
  if (status) HIPCHK(hipMemcpyAsync(status, d_status.p, (size_t)n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}
