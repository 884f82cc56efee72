// The add kernels' view of names.h's windows (device code only; include after hip_runtime.h).
#pragma once
#include "names.h"

namespace br {

// the rows of name g: false where its offsets descend or leave the add's rows
__device__ __forceinline__ bool name_rows(const NameWindow &N, int64_t g, uint64_t &r0, uint64_t &r1) {
  r0 = N.row_off[(int64_t)N.group_off[g] - N.ro_bias];
  r1 = N.row_off[(int64_t)N.group_off[g + 1] - N.ro_bias];
  return r0 >= N.r_first && r1 <= N.r_last && r0 <= r1;
}

// row r's record: false where its offsets descend, leave the add's bytes or are too close for the fixed fields
__device__ __forceinline__ bool record_of(const NameWindow &N, const RecordWindow &R, uint64_t r, const uint8_t *&rec, uint64_t &len) {
  const uint64_t *ro = R.rec_off - R.rec_bias;
  const uint64_t first = ro[N.r_first], last = ro[N.r_last], at = ro[r], next = ro[r + 1];
  if (at < first || next < at || next > last || next - at < (uint64_t)MIN_RECORD) return false;
  rec = R.data + (at - R.data_bias); len = next - at;
  return true;
}

}  // namespace br
