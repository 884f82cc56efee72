// Single-cell count matrices on the device (cells_kernels.hip; host side: cells.cpp, which holds the pipeline's description; the
// definitions -- barcode, cell, entry, slot, the three modes -- are in bramble_amd.h, br_cells).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "names.h"

namespace br {

constexpr uint32_t CL_WAVE_ITEMS = 64;   // a cell of up to this many slots and pairs is one wave's work; a longer list is summed by the wave
constexpr uint32_t CL_LDS_HEAD = 64;     // bytes of a block cell's LDS in front of theta, theta' and q (the block's reduction)
constexpr uint32_t CL_LDS_MAX = 65536;   // the largest "lds_bytes"
// words of the counters
enum { CL_BAD = 0,        // add: offsets that descend, a record shorter than its fixed fields
       CL_NO_BC = 1, CL_TOO_LONG = 2, CL_BAD_AUX = 3,   // add: the names with rows the barcode parse counted
       CL_SPAN = 4,       // add: the rows of the add's names (two words)
       CL_BITS = 6,       // finish: OR and AND of the sort keys (two words)
       CL_NWAVE = 8, CL_NBLK = 9, CL_NHBM = 10,   // finish: the cells of the wave route, of the block and HBM routes together, of the HBM route
       CL_NEED = 11,      // finish: the most LDS bytes a block-route cell asks for
       CL_WORDS = 16 };

// One add: the names of the add and their records, as names.h holds them
struct ClAddArgs {
  NameWindow names; RecordWindow recs;
  int where; uint32_t sep, tag;        // barcode_inl.h
  uint64_t *cb; uint8_t *cblen;        // per name, at the add's first name: four words, the length
  unsigned long long *counters;
};
void launch_cl_add(hipStream_t st, const ClAddArgs &A);

// finish.  flag[i] = name i counts: it has a barcode and a class
void launch_cl_flag(hipStream_t st, const uint8_t *cblen, const uint32_t *name_cls, int64_t n, uint64_t *flag);
// cid: the scanned heads (n + 1).  name_cell[idx[j]] = the cell of item j; the cell's barcode from its first item; key[j] = cell << 32 |
// class of idx[j], to be sorted
void launch_cl_cells(hipStream_t st, const uint64_t *cid, const uint32_t *idx, int64_t n, const uint64_t *cb, const uint8_t *cblen,
                     const uint32_t *name_cls, uint32_t *name_cell, uint64_t *cell_cb, uint8_t *cell_len, uint64_t *key);
// the entries from the sorted (cell, class) keys and their runs' begins (ebeg: n_ent + 1): cell, class, n_e, the pairs of the entry
// (gk of its class; n_ent + 1 words, to be scanned into pair_off) and cell_eoff (n_cells + 1): a cell's first entry
void launch_cl_entries(hipStream_t st, const uint64_t *key, const uint64_t *ebeg, int64_t n_ent, int64_t n_cells, const uint32_t *gk,
                       uint32_t *e_cell, uint32_t *e_cls, uint32_t *e_n, uint64_t *pair_cnt, uint64_t *cell_eoff);
// the pairs of every entry in ascending feature order: key[p] = cell << 32 | feature, idx[p] = p, p_ent[p] = the entry
void launch_cl_pairs(hipStream_t st, int64_t n_ent, const uint32_t *e_cell, const uint32_t *e_cls, const uint64_t *pair_off, const uint32_t *glab,
                     const uint64_t *goff, uint64_t *key, uint32_t *idx, uint32_t *p_ent);
// the sorted pairs (stable: a slot's pairs in ascending entry order) and their scanned flags sid: pslot[idx[q]] = the slot of sorted
// pair q, t_ent[q] = the entry of sorted pair q
void launch_cl_transpose(hipStream_t st, const uint32_t *idx, const uint64_t *sid, int64_t n_pairs, const uint32_t *p_ent, uint32_t *pslot,
                         uint32_t *t_ent);
// the slots from the sorted keys and their runs' begins (sbeg: n_slots + 1): the feature, and cell_soff (n_cells + 1): a cell's first slot
void launch_cl_slots(hipStream_t st, const uint64_t *key, const uint64_t *sbeg, int64_t n_slots, int64_t n_cells, uint32_t *s_feat,
                     uint64_t *cell_soff);

// What the value kernels read: cell k has the entries [cell_eoff[k], cell_eoff[k + 1]), the slots [cell_soff[k], cell_soff[k + 1]) and,
// in entry order and in slot order alike, the pairs [pair_off[first entry], pair_off[last entry + 1])
struct ClTables {
  int64_t n_cells;
  const uint64_t *cell_eoff, *cell_soff, *pair_off, *sbeg;
  const uint32_t *e_n, *pslot, *t_ent;
};
// the routes: wave_list / blk_list (n_cells words each; the block list holds the block and HBM cells) and the counters CL_NWAVE ..
// CL_NEED (zeroed by the caller).  The order inside a list is that of integer atomics; no result depends on it
void launch_cl_route(hipStream_t st, const ClTables &T, uint32_t lds_bytes, uint32_t *wave_list, uint32_t *blk_list, unsigned long long *counters);
// "mode" 1 and 2: theta (n_slots) and n_iters (n_cells) of every cell, the whole iteration loop inside ONE launch: the first n_blk
// blocks take a block-list cell each -- theta, theta' and q in LDS where they fit in lds_bytes, else in scratch (theta' at
// scratch[slot], q at scratch[n_slots + entry]) -- and every wave of the blocks behind them a wave-list cell.  lds: the counters'
// CL_NEED.  No floating-point atomic: a sum is one lane's loop in ascending order, a list of more than CL_WAVE_ITEMS the wave's (lane l
// takes the items l, l + 64, ..., then wave_sum's fixed tree), so a cell's bits do not depend on its route
struct ClEmArgs {
  ClTables T;
  const uint32_t *wave_list, *blk_list; uint32_t n_wave, n_blk;
  uint32_t lds_bytes, lds;
  uint32_t max_iters; double tolerance;
  int64_t n_slots;
  double *theta, *scratch; uint32_t *n_iters;
};
void launch_cl_em(hipStream_t st, const ClEmArgs &E);
// "mode" 0: val[s] = the sum of n_e over the slot's entries of one feature
void launch_cl_unique(hipStream_t st, const ClTables &T, int64_t n_slots, double *val);
// per cell: names, unique (entries of one feature), multi (the others)
void launch_cl_cell_stats(hipStream_t st, const ClTables &T, uint64_t *names, uint64_t *unique, uint64_t *multi);
// flag[s] = the slot is part of the matrix (drop_zero: val[s] != 0; else every slot), to be scanned
void launch_cl_keep(hipStream_t st, const double *val, int64_t n_slots, int drop_zero, uint64_t *flag);
// the matrix from the scanned flags: m_off (n_cells + 1), m_feat, m_val, n_feat per cell
void launch_cl_matrix(hipStream_t st, const ClTables &T, const uint64_t *pos, int64_t n_slots, const uint32_t *s_feat, const double *val,
                      uint64_t *m_off, uint32_t *m_feat, double *m_val, uint32_t *n_feat);

}  // namespace br
