// SAM text -> BAM records on the device (sam_kernels.hip; host side: sam_reader.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace br {

// the measure pass's result for one line (the emit pass reads the fields from here instead of tokenizing again)
struct SamLine {
  uint32_t f[12];        // field starts relative to the line start: f[k] = field k (0-based, k < 11); f[11] = the first tag
                         // (len + 1 when the line has none); field k ends at f[k + 1] - 1
  uint32_t len;          // line length without '\n' and a trailing '\r'
  int32_t ref, nref, pos, npos, tlen;
  uint32_t bsize;        // BAM block_size
  uint32_t n_cig;        // CIGAR ops of the line (> 65535: the CG form)
  uint32_t rlen;         // reference length of the CIGAR
  uint32_t l_seq;
  uint32_t aux;          // tag bytes, without the CG tag
  uint16_t flag, bin;
  uint8_t mapq, err, mapped, pad;
};

// a float the device could not convert exactly (outside Clinger's fast path): the host puts (float)strtod(text) there
struct SamFix { uint64_t dst; uint64_t text; uint32_t text_len; uint32_t line; };

enum SamErr : uint8_t {
  SAM_OK = 0, SAM_E_EMPTY, SAM_E_FIELDS, SAM_E_QNAME, SAM_E_FLAG, SAM_E_POS, SAM_E_MAPQ, SAM_E_CIGAR, SAM_E_PNEXT, SAM_E_TLEN,
  SAM_E_SEQ_CIGAR, SAM_E_QUAL_SEQ, SAM_E_TAG, SAM_E_TAG_RANGE, SAM_E_TOO_LONG, SAM_E_FLOAT, SAM_E_COUNT
};

struct SamArgs {
  const uint8_t *text;
  uint64_t n_bytes;
  uint64_t *lend;                // end of line i: its '\n' (or n_bytes for a last line without one)
  int64_t n_lines;
  SamLine *line;
  uint64_t *mapped;              // n_lines + 1: 0 / 1, then its exclusive scan (record index)
  uint64_t *bytes;               // n_lines + 1: 4 + block_size of a mapped line, then its exclusive scan (byte offset)
  unsigned long long *first_bad; // min over bad lines of (line << 8 | error)
  // @SQ names: open addressing over FNV-1a hashes
  const int32_t *h_slot;
  uint32_t h_mask;
  const uint64_t *name_off;      // n_ref + 1
  const uint8_t *names;
  int32_t n_ref;
  // emit
  uint8_t *blob;
  uint64_t *rec_off;
  uint32_t *rec_len;
  uint32_t *rec_line;
  SamFix *fix;
  uint32_t fix_cap;
  uint32_t *n_fix;
};

constexpr uint64_t SAM_NL_TILE = 64u << 10;   // bytes per block of the line index

void launch_sam_nl_count(hipStream_t st, const uint8_t *text, uint64_t n, uint64_t *tile_cnt);
void launch_sam_nl_write(hipStream_t st, const uint8_t *text, uint64_t n, const uint64_t *tile_pre, uint64_t *lend);
void launch_sam_measure(hipStream_t st, const SamArgs &A);
void launch_sam_emit(hipStream_t st, const SamArgs &A);

}  // namespace br
