// What bigwig.cpp reads of a br_coverage (coverage.cpp owns the object): the finished depth, runs and offsets, the base that counts
// its device bytes, and the slot that holds the bigWig image between the calls.  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "accum.h"

struct br_coverage;

namespace br {

struct BigwigState;   // bigwig.cpp: the image and its numbers

struct CoverageView {
  Accum *acc;                          // device, stream and the byte account
  int weight;                          // 0: depth words uint32; 1, 2: uint64 in units of 2^-32
  int64_t n_tx, n_runs;
  const std::vector<uint64_t> *off;    // host: n_tx + 1
  const uint64_t *d_off;               // the same on the device
  const void *depth;
  const uint4 *runs;                   // (transcript, start, end, depth or 0)
  const uint64_t *run_depth;           // weighted modes, else NULL
  BigwigState **state;
};

// BR_ERR_INVALID_ARG before finish and on a broken object
int coverage_view(br_coverage *c, CoverageView *v);
// the image's bytes leave the account and the state goes (br_coverage_free calls it; a NULL state is fine)
void bigwig_state_free(Accum *acc, BigwigState *s);

}  // namespace br
