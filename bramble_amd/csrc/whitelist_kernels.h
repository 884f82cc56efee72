// The cell barcode whitelist on the device (whitelist_kernels.hip; host side: whitelist.cpp, which holds the pipeline's description;
// the definitions -- entry, count, candidates, the three "correct" values, the statuses -- are in bramble_amd.h, br_whitelist).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

constexpr uint32_t WL_NONE = 0xffffffffu;    // obs_entry / a name's entry: no whitelist entry
constexpr uint32_t WL_AMBIG = 0xfffffffeu;   // obs_entry: two or more candidates (entries are < 2^31 - 1)
constexpr int64_t WL_MIN_SLOTS = 64;
// words of a resolve's (and the build's) counters
enum { WL_BITS = 0,       // OR and AND of the sort keys (two words)
       WL_FULL = 2,       // build: entries that found no slot
       WL_CHAIN = 3,      // build: the longest probe chain (slots looked at by one insert)
       WL_STATUS = 4,     // apply: names of the statuses 0 .. 4 (five words)
       WL_WORDS = 16 };

// What a probe reads: the open-addressing table (n_slots a power of two; a slot is tag << 32 | entry + 1, 0 when empty) over the
// distinct entries' words (four each, bytes in comparison order) and lengths.  mask: the hash's "hash_bits"
struct WlTable {
  const uint64_t *slots; uint64_t n_slots, mask;
  const uint64_t *cb; const uint8_t *len; int64_t n_entries;
};

// build.  The distinct barcodes from the sorted index and its scanned heads (pos: n + 1): entry pos[j + 1] - 1 is item idx[j]'s
void launch_wl_gather(hipStream_t st, const uint64_t *pos, const uint32_t *idx, int64_t n, const uint64_t *cb, const uint8_t *len, uint64_t *out_cb,
                      uint8_t *out_len);
// every entry into the table (slots: writable, zeroed by the caller); counters[WL_FULL], counters[WL_CHAIN]
void launch_wl_insert(hipStream_t st, const WlTable &T, uint64_t *slots, unsigned long long *counters);

// resolve.  The distinct observed barcodes from the sorted names (idx, n) and the scanned heads' begins (obeg: D + 1): observed o is
// the barcode of name idx[obeg[o]], of obeg[o + 1] - obeg[o] names.  obs_entry[o] = its entry or WL_NONE, count[entry] = its names
// (count zeroed by the caller), miss[o] = it is not in the whitelist (to be scanned)
void launch_wl_exact(hipStream_t st, const WlTable &T, const uint32_t *idx, const uint64_t *obeg, int64_t n_obs, const uint64_t *cb, const uint8_t *cblen,
                     uint32_t *obs_entry, uint64_t *count, uint64_t *miss);
// one wave per observed barcode of the list (the ones that missed): obs_entry[o] = the entry it is corrected to, WL_NONE or WL_AMBIG.
// correct 1 or 2
void launch_wl_near(hipStream_t st, const WlTable &T, const uint32_t *list, int64_t n_list, const uint32_t *idx, const uint64_t *obeg, const uint64_t *cb,
                    const uint8_t *cblen, const uint64_t *count, int correct, uint32_t *obs_entry);
// one lane per sorted name j (oid: the scanned heads, n + 1): status[idx[j]], entry[idx[j]] (may be NULL) and the name's barcode
// rewritten in place -- the entry's bytes, or nothing (length 0); counters[WL_STATUS + 1 .. 4].  The names without a barcode are the
// caller's (status 0 everywhere first)
void launch_wl_apply(hipStream_t st, const WlTable &T, const uint64_t *oid, const uint32_t *idx, int64_t n, const uint32_t *obs_entry, uint64_t *cb,
                     uint8_t *cblen, uint8_t *status, uint32_t *entry, unsigned long long *counters);
// flag[i] = name i has a barcode (to be scanned), and entry[i] = WL_NONE where entry is given
void launch_wl_flag(hipStream_t st, const uint8_t *cblen, int64_t n, uint64_t *flag, uint32_t *entry);

}  // namespace br
