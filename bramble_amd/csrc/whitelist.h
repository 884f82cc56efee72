// What the accumulators that resolve their names' barcodes against a br_whitelist (cells.cpp, dedup.cpp) share with whitelist.cpp.
// Host only.
#pragma once
#include "accum.h"

struct br_whitelist;

namespace br {

struct WlResolved {
  uint64_t status[5] = {0, 0, 0, 0, 0};   // names of each status
  uint64_t distinct = 0;                  // D: distinct observed barcodes
  double seconds = 0;
};

int wl_device(const br_whitelist *wl);
// br_*_whitelist_stats of an accumulator that resolved against a whitelist: the five statuses, D, microseconds, "correct"
int wl_stats(const WlResolved &r, int correct, uint64_t out[8]);

// The N names' barcodes cb / cblen (device tables of c, which runs the work on its stream and counts the memory) resolved in place
// under "correct" 0 .. 2: status (N bytes on the device) and, where given, entry (N words).  Every table of the resolve is dropped
// before it returns; the stream is done
int wl_resolve(Accum *c, const br_whitelist *wl, int correct, uint64_t *cb, uint8_t *cblen, int64_t N, uint8_t *status, uint32_t *entry, WlResolved *out);

}  // namespace br
