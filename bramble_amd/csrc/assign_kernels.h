// The posterior of every projected record and the rewritten record stream (assign_kernels.hip; host side: assign.cpp, which holds
// the pipeline's description; the definitions are in bramble_amd.h, br_assign).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "names.h"

namespace br {

constexpr uint32_t AS_M_LANE_MAX = 64;   // a name of up to this many records: a lane per record counts m; a longer one: a wave per name
constexpr int AS_WRITE_LANES = 16;       // lanes per record of the write kernel
constexpr uint32_t AS_TAG_BYTES = 7;     // 'Z' 'W' 'f' + float32
// words of the counters
enum { AS_BAD_NAMES = 0,    // add: a row the offsets give to no name
       AS_BAD_PLACE = 1,    // add: a record that belongs to no placement, or a leader whose mate is not the next record of its name
       AS_BAD_NAME = 2, AS_BAD_CLASS = 3, AS_BAD_LABEL = 4, AS_BAD_POST = 5,   // finish: what the look-up met (br_assign_stats' four)
       AS_N_BIG = 6,        // finish: names of more than AS_M_LANE_MAX records
       AS_N_NAMED = 7,      // finish: names with records
       AS_BAD_REC = 8,      // next (mode sample): a kept record without the encoder's NH / HI entries
       AS_BAD_OFF = 9,      // add: record offsets that descend
       AS_CUT = 10,         // next: the piece's last record + 1 and its bytes (two words)
       AS_WORDS = 16 };

// note bits (uint4 note: x = the add-order name, y = the transcript, z = these, w = 0)
constexpr uint32_t AS_FIRST = 1u, AS_PAIRED = 2u;

// One add: the rows [r_first, r_last) of the caller's table become the records [n0, n0 + r_last - r_first) of the object.  a may be
// a slice: row r is at a[r - a_bias].  The names and the records as names.h holds them: name g's add-order index is name_base + g;
// recs.rec_off NULL: values only; recs.data is not read -- the host copies the records' bytes, to arena_base on
struct AsAddArgs {
  const uint4 *a; int64_t a_bias;
  NameWindow names; uint64_t name_base;
  RecordWindow recs; uint64_t arena_base;
  uint4 *note;          // the object's, at [n0 + ...]
  uint64_t *off;        // likewise (r_last - r_first + 1 entries are written)
  uint64_t n0;
  unsigned long long *counters;
};
void launch_as_add(hipStream_t st, const AsAddArgs &A);

struct AsFinishArgs {
  const uint4 *note; uint64_t n;
  const uint32_t *name_cls; uint64_t n_names;
  const uint64_t *label_off; const uint32_t *labels; uint64_t n_cls, n_lab;
  const double *post;
  double *p;            // n: p(r), 0 where the look-up failed (counted)
  uint32_t *m;          // n
  uint32_t *big;        // n / (AS_M_LANE_MAX + 1) + 1: the first records of the long names
  double *w;            // n: w of the record's placement
  uint8_t *kept;        // n
  uint64_t *rank;       // n + 1: kept[r] as a word, to be scanned (the kept records in front of every record)
  int mode; uint32_t k0, k1;
  unsigned long long *counters;
};
// p, m, w, the draw (or kept = 1) and rank's words; everything on the stream, nothing waited for
void launch_as_finish(hipStream_t st, const AsFinishArgs &F);
// rank scanned: sel[k] = the k-th kept record, out_len[k] = the bytes of its rewritten form (to be scanned: out_off)
void launch_as_select(hipStream_t st, const uint8_t *kept, const uint64_t *rank, const uint64_t *off, uint64_t n, uint32_t *sel, uint64_t *out_len);

// res[0] = the largest e in (cur, n_out] with out_off[e] - out_off[cur] <= max_bytes, cur + 1 when the first record alone is
// larger; res[1] = out_off[e] - out_off[cur]
void launch_as_cut(hipStream_t st, const uint64_t *out_off, uint64_t n_out, uint64_t cur, uint64_t max_bytes, uint64_t *res);

// the kept records [cur, e) rewritten into dst, with the piece's row_off (e - cur + 1 entries)
struct AsWriteArgs {
  const uint8_t *arena; const uint64_t *off; const uint32_t *sel; const uint64_t *out_off; const double *w;
  uint64_t cur, e;
  uint8_t *dst; uint64_t *row_off;
  int mode; uint32_t mapq;
  unsigned long long *counters;
};
void launch_as_write(hipStream_t st, const AsWriteArgs &W);

}  // namespace br
