// The host's parts of a bigWig image (bramble_amd.h, br_coverage_bigwig: the layout and the definitions): the order of the
// chromosome names, the chromosome B+ tree, the arithmetic of a tree's levels and the fixed-size headers.  Plain data in, bytes
// out; no call into the library or the device, so the unit builds and runs alone.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace brbw {

constexpr uint32_t BIGWIG_MAGIC = 0x888FFC26u, CHROM_TREE_MAGIC = 0x78CA8C91u, RTREE_MAGIC = 0x2468ACE0u;
constexpr uint64_t HEADER_BYTES = 64, ZOOM_HEADER_BYTES = 24, SUMMARY_BYTES = 40, CHROM_TREE_HEADER = 32, RTREE_HEADER = 48;

// A tree over n items with up to bs children a node, from the leaves up: items[0] = n, items[l + 1] = the nodes of level l, until a
// level is one node (a tree of at most bs items, or of none, is one leaf)
struct TreeShape {
  uint32_t bs = 1;                  // min(the option, max(n, 1)): what the tree's header says
  std::vector<uint64_t> items;      // per level, leaves first
  uint64_t nodes(size_t level) const { const uint64_t m = (items[level] + bs - 1) / bs; return m ? m : 1; }
  // bytes of the levels above `level` (they come first in the file) and of all levels, for items of leaf_item / inner_item bytes
  uint64_t bytes_above(size_t level, uint64_t leaf_item, uint64_t inner_item) const;
  uint64_t bytes(uint64_t leaf_item, uint64_t inner_item) const { return bytes_above(0, leaf_item, inner_item) + nodes(0) * (4 + bs * leaf_item); }
};
TreeShape tree_shape(uint64_t n, uint32_t block_size);

// order[id] = the index of the name with chromId id: the names in bytewise (strcmp) order.  false, and *err, for a NULL or empty
// name and for two equal names.  *key_size = the longest name's length (0 without names)
bool name_order(const std::vector<const char *> &names, std::vector<uint32_t> *order, uint32_t *key_size, std::string *err);

// the chromosome tree (header and nodes) of the names in chromId order with their sizes; file_off: where the tree begins in the file
std::vector<uint8_t> chrom_tree(const std::vector<const char *> &sorted_names, const std::vector<uint32_t> &sizes, uint32_t key_size,
                                uint32_t block_size, uint64_t file_off);

struct ZoomHeader { uint32_t reduction; uint64_t data_off, index_off; };
struct Summary { uint64_t valid; double min_val, max_val, sum, sum_squares; };
// header, zoom headers and total summary: the first 64 + 24 Z + 40 bytes of the file
std::vector<uint8_t> file_head(const std::vector<ZoomHeader> &zooms, uint64_t chrom_tree_off, uint64_t data_off, uint64_t index_off,
                               uint32_t uncompress_buf, const Summary &total);
// the 48 bytes in front of an R-tree's nodes; lo / hi: the root's bounds (chromId << 32 | base)
std::vector<uint8_t> rtree_header(uint32_t bs, uint64_t n_items, uint64_t lo, uint64_t hi, uint64_t end_file_off);

}  // namespace brbw
