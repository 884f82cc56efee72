// What an accumulator that holds a count matrix in HBM shares with cellcall.cpp.  Host only.
#pragma once
#include <stdint.h>

struct br_cellcall;

namespace br {

// br_cellcall_run behind its argument checks: the matrix's tables on c's device, ready on c's stream; nnz = cell_off[n_cells]
int cc_run(br_cellcall *c, int64_t n_cells, int64_t n_features, const uint64_t *cell_off, const uint32_t *feature, const uint32_t *count, uint64_t nnz);

// c has not run and is on `device`
bool cc_fresh(const br_cellcall *c, int device);
// after a run: the cells' status on the device (n_cells bytes) and how many are called
const uint8_t *cc_status(const br_cellcall *c, int64_t *n_cells, uint64_t *n_called);

}  // namespace br
