// UMI-aware duplicate removal by read name (dedup_kernels.hip; host side: dedup.cpp, which holds the pipeline's description; the
// definitions -- UMI, entry, signature, position group, molecule, representative -- are in bramble_amd.h, br_dedup).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "names.h"

namespace br {

constexpr int DD_UMI_MAX = 32;           // bytes of a UMI; a name's slot holds them zero padded, as four 64-bit words
constexpr int DD_SMALL_ROWS = 16;        // a read name of up to this many rows is one lane's work in k_dd_sig, a larger one a wave's
constexpr uint32_t DD_WAVE_OPS = 64;     // a pooled CIGAR of more ops than this is summed by the wave
constexpr unsigned DD_BIG_GRID = 1024;   // blocks (of 4 waves) that walk a list whose length only the device knows
constexpr int DD_WRITE_LANES = 16;       // lanes per record of the gather
// words of the counters
enum { DD_BAD = 0,        // add: offsets that descend, a record shorter than its fixed fields, a pooled CIGAR that leaves the pool
       DD_NBIG = 1,       // add: names of more than DD_SMALL_ROWS rows (the list's length)
       DD_NO_UMI = 2, DD_TOO_LONG = 3, DD_BAD_AUX = 4,   // add: the names with rows the UMI parse counted
       DD_COLL = 5,       // finish: neighbours with equal keys and different signatures
       DD_BITS = 6,       // finish: OR and AND of the sort keys (two words)
       DD_MAXM = 8,       // finish: the largest group's node count
       DD_CHANGED = 9,    // finish: a sweep changed a label
       DD_MOLS = 10,      // finish: molecules
       DD_CUT = 11,       // next: the piece's last record + 1 and its bytes (two words)
       DD_SPAN = 13,      // add: the rows of the add's names (two words)
       DD_WORDS = 16 };

// One add: the names [0, n_groups) of the add become the names [name_base, ...) of the object, their rows [r_first, r_last) its rows
// [row_base, ...).  a, cigar may be slices: row r is at [r - a_bias]; the names and the records as names.h holds them.
struct DdAddArgs {
  const uint4 *a; const uint64_t *cigar; int64_t a_bias;
  const uint32_t *pool; uint64_t n_pool_words;
  NameWindow names; RecordWindow recs;
  int umi_source; uint32_t umi_sep, umi_tag;
  int cell_source; uint32_t cell_tag;             // "cell_source" 0: no barcode is read and cb, cblen are not written
  uint4 *raw;            // the add's entries in row order (r_last - r_first), scratch
  uint32_t *ent;         // the object's entry arena, four words an entry: a name's sorted entries sit at its first row's slot
  uint64_t row_base;
  uint64_t *noff; uint32_t *nk; uint64_t *hash;   // per name, at the add's first name: arena offset and length in WORDS, the signature's hash
  uint64_t *umi; uint8_t *ulen;                   // per name likewise: four words, the length
  uint64_t *cb; uint8_t *cblen;                   // with "cell_source": the cell barcode likewise (a name without one: length 0)
  uint32_t *big;         // the names of more than DD_SMALL_ROWS rows
  uint64_t *rec_at;      // NULL, or ("keep_records") the arena offsets of the add's records, r_last - r_first + 1 of them from arena_base
  uint64_t arena_base;
  unsigned long long *counters;
};
void launch_dd_add(hipStream_t st, const DdAddArgs &A);

// finish.  The sorted items are (key, name) pairs; gid: the scanned heads (n + 1 entries)
// group_first[idx[j]] = idx[gbeg[group of j]], name_gid[idx[j]] = the group of j
void launch_dd_groups(hipStream_t st, const uint64_t *gid, const uint64_t *gbeg, const uint32_t *idx, int64_t n, uint32_t *group_first, uint32_t *name_gid);
// the nodes in (group, length, bytes) order: key[q] = group << 32 | ~count, val[q] = q: to be sorted (stable) into the node order
void launch_dd_node_key(hipStream_t st, const uint64_t *nbeg, const uint32_t *idx, const uint32_t *name_gid, int64_t n_nodes, uint64_t *key, uint32_t *val);
struct DdNodes {
  int64_t n_nodes, n_groups;
  uint64_t *umi; uint8_t *len; uint32_t *cnt; uint32_t *first; uint32_t *gid;   // per node in node order
  uint32_t *inv;         // node in (group, length, bytes) order -> its place in node order
  uint64_t *gn0;         // n_groups + 1: a group's first node
  uint64_t *work;        // n_groups + 1: a group's tile pairs (to be scanned)
  uint64_t *indeg;       // n_nodes + 1: edges into a node (to be scanned into eoff)
  uint32_t *cursor;      // n_nodes
  uint32_t *esrc;        // the edges' sources, by target
  uint32_t *label[2];    // n_nodes
  uint32_t *msize;       // n_nodes: names of the molecule rooted here
  unsigned long long *counters;
};
// the node tables from the sorted order val (place p holds node val[p]); the groups' first nodes, their tile pairs (0 for a group
// of one node), counters[DD_MAXM]
void launch_dd_nodes(hipStream_t st, const DdNodes &N, const uint32_t *val, const uint64_t *nbeg, const uint32_t *idx, const uint64_t *umi,
                     const uint8_t *ulen, const uint32_t *name_gid);
// one wave per tile pair (64 targets x 64 sources of one group): fill = false counts the edges into every target (indeg, zeroed),
// fill = true stores their sources behind eoff (cursor zeroed).  n_work: work[n_groups] after the scan
void launch_dd_edges(hipStream_t st, const DdNodes &N, const uint64_t *eoff, uint64_t n_work, bool fill);
// label[p] = p
void launch_dd_label_init(hipStream_t st, uint32_t *label, int64_t n_nodes);
// one sweep: out[p] = min(in[p], in[u] for every edge u -> p); counters[DD_CHANGED] = 1 where that lowered one
void launch_dd_sweep(hipStream_t st, const DdNodes &N, const uint64_t *eoff, const uint32_t *in, uint32_t *out);
// msize, the histogram (hist_max + 1 words, zeroed) and counters[DD_MOLS] from the final labels
void launch_dd_molecules(hipStream_t st, const DdNodes &N, const uint32_t *label, uint64_t *hist, uint32_t hist_max);
// rep and dup of the names of the sorted items (nid: the scanned node heads)
void launch_dd_verdict(hipStream_t st, const DdNodes &N, const uint32_t *label, const uint64_t *nid, const uint32_t *idx, int64_t n, uint32_t *rep,
                       uint8_t *dup);

// records.  rank[r] = record r is handed out (mark: every record; else those whose name is no duplicate), to be scanned
void launch_dd_keep(hipStream_t st, const uint64_t *noff, int64_t n_names, const uint8_t *dup, uint64_t n_rows, int mark, uint64_t *rank, uint8_t *rdup);
// rank scanned: sel[k] = the k-th record handed out, out_len[k] = its bytes (to be scanned: out_off)
void launch_dd_select(hipStream_t st, const uint64_t *rank, const uint64_t *rec_at, uint64_t n_rows, uint32_t *sel, uint64_t *out_len);
// the records sel[cur, e) copied to dst with the piece's row_off; flag 0x400 set on those of rdup
void launch_dd_write(hipStream_t st, const uint8_t *arena, const uint64_t *rec_at, const uint32_t *sel, const uint64_t *out_off, const uint8_t *rdup,
                     uint64_t cur, uint64_t e, uint8_t *dst, uint64_t *row_off);

}  // namespace br
