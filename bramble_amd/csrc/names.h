// What an add of read names hands its kernels, whichever accumulator takes it (quant, coverage, assign, dedup, cells): the names'
// window of the caller's offset tables and, for the record consumers, the window of the record stream.  Host and device.
#pragma once
#include <stdint.h>

namespace br {

constexpr uint32_t MIN_RECORD = 36;    // [block_size] and the fixed fields of a record
constexpr uint64_t ARENA_SLACK = 64;   // bytes a record arena (br_assign, br_dedup) keeps behind its end: its readers take whole aligned words

// The names [0, n_groups) of one add: name g has the alignments [group_off[g], group_off[g + 1]), alignment a the rows
// [row_off[a - ro_bias], row_off[a + 1 - ro_bias]) -- row_off may be a slice of the caller's table (a host add uploads only what it
// needs) -- and all of them lie in [r_first, r_last) = row_off[group_off[0]], row_off[group_off[n_groups]]
struct NameWindow {
  const uint64_t *row_off; int64_t ro_bias; const uint32_t *group_off; int64_t n_groups;
  uint64_t r_first, r_last;
};

// The records of those rows: row r's record, [block_size][record], is data[rec_off[r - rec_bias] - data_bias ...) up to the next
// row's offset.  rec_off and data may be slices likewise
struct RecordWindow {
  const uint64_t *rec_off; int64_t rec_bias;
  const uint8_t *data; uint64_t data_bias;
};

}  // namespace br
