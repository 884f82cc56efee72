// BAM records -> SAM text on the device (sam_format_kernels.hip; host side: sam_writer.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

struct SamFmtArgs {
  const uint8_t *data;            // [block_size][record]...
  uint64_t n_bytes;
  const uint64_t *row_off;        // n: offset of each record's block_size word
  int64_t n;
  const uint64_t *name_off;       // n_names + 1
  const uint8_t *names;           // the reference names, concatenated
  int32_t n_names;
  uint64_t *len;                  // n + 1: line lengths, then their exclusive scan (line offsets, [n] = the total)
  uint32_t *long_list;            // records of more than SF_LONG_REC bytes: a whole wave each
  uint32_t *n_long;
  unsigned long long *first_bad;  // lowest record that cannot be formatted (unknown tag type, data past its end)
  uint8_t *text;
};

constexpr uint32_t SF_LONG_REC = 2048;   // records of more bytes get a whole wave (the 16-lane kernels list them)

void launch_sam_fmt_measure(hipStream_t st, const SamFmtArgs &A, int n_cu);
void launch_sam_fmt_emit(hipStream_t st, const SamFmtArgs &A, int n_cu);

}  // namespace br
