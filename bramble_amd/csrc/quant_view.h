// What another accumulator on the same device may read of a quantifier whose EM has run with "keep_names" on (quant.cpp makes
// it; br_coverage_finish_em is the reader).  Device tables, the quantifier's own: valid until it is freed or its EM runs again.
#pragma once
#include <stdint.h>

#include "../../include/bramble_amd.h"

namespace br {

struct QuantView {
  int device;
  int64_t n_names, n_cls, n_lab;
  const uint32_t *name_cls;     // n_names: the class of add-order name i, 0xffffffff for a name without rows
  const uint64_t *label_off;    // n_cls + 1
  const uint32_t *labels;       // n_lab, ascending inside a class
  const double *post;           // n_lab: the posterior of every label entry
};
// BR_ERR_INVALID_ARG before br_quant_em or without "keep_names"; it waits for the quantifier's stream
int quant_view(br_quant *, QuantView *);

// The classes alone, which br_quant_finish with "keep_names" has made: no EM is asked for (br_cells_finish is the reader).  Valid
// until the quantifier is freed.  BR_ERR_INVALID_ARG before br_quant_finish or without "keep_names"; it waits for the stream
struct QuantClassView {
  int device;
  int64_t n_names, n_tx, n_cls, n_lab;
  const uint32_t *name_cls;     // as above
  const uint64_t *label_off;
  const uint32_t *labels;
};
int quant_class_view(br_quant *, QuantClassView *);

}  // namespace br
