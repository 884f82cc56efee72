// A short field of a BAM record -- a UMI or a cell barcode -- read on the device (device code only; include after hip_runtime.h).
// dedup_kernels.hip reads a name's UMI and, with "cell_source", its barcode with it; cells_kernels.hip the barcode.  The walk rules
// are those of br_dedup in bramble_amd.h: nothing past the record is read, a field type outside AcCsSiIfZHB or a field that runs past
// the record's end ends the aux walk (bad_aux), a field of more than BC_MAX bytes is none (too_long).
#pragma once
#include <stdint.h>

namespace br {

constexpr int BC_MAX = 32;   // bytes of a field; a name's slot holds them zero padded, as four 64-bit words
// where the field is
enum { BC_NAME_LAST = 0,     // read_name behind its last separator byte (umi_tools extract's UMI)
       BC_TAG = 1,           // the value of the first aux field `tag` of type Z
       BC_NAME_PREV = 2 };   // read_name between its last two separator bytes (umi_tools extract's READ_CB_UMI)

__device__ __forceinline__ uint32_t bc_ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t bc_ld32(const uint8_t *p) { return bc_ld16(p) | bc_ld16(p + 2) << 16; }

// the field of a record (rec: [block_size][record], len bytes) into four words, bytes in comparison order, zero padded; its length,
// 0: none.  too_long / bad_aux: why
__device__ __forceinline__ uint32_t record_field(const uint8_t *rec, uint64_t len, int where, uint32_t sep, uint32_t tag, uint64_t w[4],
                                                 bool &too_long, bool &bad_aux) {
  w[0] = w[1] = w[2] = w[3] = 0;
  too_long = bad_aux = false;
  const uint64_t l_name = rec[12];
  const uint8_t *u = nullptr;
  uint64_t ul = 0;
  if (where != BC_TAG) {
    if (l_name < 2 || 36 + l_name > len) return 0;
    const uint64_t nl = l_name - 1;   // (without its NUL)
    int64_t at = -1, before = -1;     // the last separator, the last before it
    for (uint64_t i = 0; i < nl; i++) if (rec[36 + i] == (uint8_t)sep) { before = at; at = (int64_t)i; }
    if (at < 0) return 0;
    if (where == BC_NAME_LAST) { u = rec + 36 + at + 1; ul = nl - (uint64_t)at - 1; }
    else {
      if (before < 0) return 0;
      u = rec + 36 + before + 1; ul = (uint64_t)(at - before - 1);
    }
  } else {
    const uint64_t n_cigar = bc_ld16(rec + 16), l_seq = bc_ld32(rec + 20);
    uint64_t p = 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    if (p > len) { bad_aux = true; return 0; }
    while (p < len) {
      if (p + 3 > len) { bad_aux = true; return 0; }
      const uint32_t t = bc_ld16(rec + p), type = rec[p + 2];
      p += 3;
      uint64_t size = 0;
      if (type == 'A' || type == 'c' || type == 'C') size = 1;
      else if (type == 's' || type == 'S') size = 2;
      else if (type == 'i' || type == 'I' || type == 'f') size = 4;
      else if (type == 'Z' || type == 'H') {
        uint64_t e = p;
        while (e < len && rec[e]) e++;
        if (e >= len) { bad_aux = true; return 0; }   // no NUL inside the record
        if (type == 'Z' && t == tag) { u = rec + p; ul = e - p; break; }
        size = e - p + 1;
      } else if (type == 'B') {
        if (p + 5 > len) { bad_aux = true; return 0; }
        const uint32_t sub = rec[p];
        const uint64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
        if (!es) { bad_aux = true; return 0; }
        size = 5 + es * (uint64_t)bc_ld32(rec + p + 1);
      } else { bad_aux = true; return 0; }
      if (size > len - p) { bad_aux = true; return 0; }
      p += size;
    }
    if (!u) return 0;
  }
  if (ul > (uint64_t)BC_MAX) { too_long = true; return 0; }
  for (uint64_t i = 0; i < ul; i++) w[i >> 3] |= (uint64_t)u[i] << (56 - 8 * (i & 7));
  return (uint32_t)ul;
}

}  // namespace br
