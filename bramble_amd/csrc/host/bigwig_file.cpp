// bigwig_file.h: name order, chromosome tree, tree shapes and the headers of a bigWig image.  Little-endian throughout.
#include "bigwig_file.h"

#include <algorithm>
#include <cstring>

namespace brbw {
namespace {

void put(std::vector<uint8_t> &b, uint64_t v, int bytes) { for (int k = 0; k < bytes; k++) b.push_back((uint8_t)(v >> (8 * k))); }
void put_f64(std::vector<uint8_t> &b, double d) { uint64_t v; memcpy(&v, &d, 8); put(b, v, 8); }

}  // namespace

TreeShape tree_shape(uint64_t n, uint32_t block_size) {
  TreeShape t;
  t.bs = (uint32_t)std::min<uint64_t>(block_size, std::max<uint64_t>(n, 1));
  t.items.push_back(n);
  while (t.nodes(t.items.size() - 1) > 1) t.items.push_back(t.nodes(t.items.size() - 1));
  return t;
}

uint64_t TreeShape::bytes_above(size_t level, uint64_t leaf_item, uint64_t inner_item) const {
  uint64_t b = 0;
  for (size_t l = level + 1; l < items.size(); l++) b += nodes(l) * (4 + bs * (l ? inner_item : leaf_item));
  return b;
}

bool name_order(const std::vector<const char *> &names, std::vector<uint32_t> *order, uint32_t *key_size, std::string *err) {
  order->resize(names.size());
  *key_size = 0;
  for (size_t i = 0; i < names.size(); i++) {
    if (!names[i] || !names[i][0]) { if (err) *err = "a transcript with coverage has no name"; return false; }
    (*order)[i] = (uint32_t)i;
    *key_size = std::max<uint32_t>(*key_size, (uint32_t)strlen(names[i]));
  }
  std::sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) { return strcmp(names[a], names[b]) < 0; });
  for (size_t i = 1; i < names.size(); i++)
    if (!strcmp(names[(*order)[i - 1]], names[(*order)[i]])) { if (err) *err = std::string("two transcripts with coverage are named ") + names[(*order)[i]]; return false; }
  return true;
}

std::vector<uint8_t> chrom_tree(const std::vector<const char *> &sorted_names, const std::vector<uint32_t> &sizes, uint32_t key_size,
                                uint32_t block_size, uint64_t file_off) {
  const uint64_t n = sorted_names.size(), item = (uint64_t)key_size + 8;
  const TreeShape t = tree_shape(n, block_size);
  std::vector<uint8_t> b;
  put(b, CHROM_TREE_MAGIC, 4); put(b, t.bs, 4); put(b, key_size, 4); put(b, 8, 4); put(b, n, 8); put(b, 0, 8);
  const uint64_t node_bytes = 4 + t.bs * item;
  auto key = [&](uint64_t i) { const size_t len = strlen(sorted_names[i]); b.insert(b.end(), sorted_names[i], sorted_names[i] + len); b.insert(b.end(), key_size - len, 0); };
  for (size_t l = t.items.size(); l-- > 0;) {   // the root's level first, each level left to right
    const uint64_t m = t.items[l];
    // one item of level l stands for bs^l names; the level below begins behind this one
    uint64_t span = 1;
    for (size_t k = 0; k < l; k++) span *= t.bs;
    const uint64_t below = file_off + CHROM_TREE_HEADER + t.bytes_above(l, item, item) + t.nodes(l) * node_bytes;
    for (uint64_t node = 0; node < t.nodes(l); node++) {
      const uint64_t first = node * t.bs, count = std::min<uint64_t>(t.bs, m > first ? m - first : 0);
      put(b, l == 0 ? 1 : 0, 1); put(b, 0, 1); put(b, count, 2);
      for (uint64_t k = 0; k < count; k++) {
        const uint64_t i = first + k;
        key(i * span);
        if (l == 0) { put(b, i, 4); put(b, sizes[i], 4); } else put(b, below + i * node_bytes, 8);
      }
      b.insert(b.end(), (size_t)((t.bs - count) * item), 0);
    }
  }
  return b;
}

std::vector<uint8_t> file_head(const std::vector<ZoomHeader> &zooms, uint64_t chrom_tree_off, uint64_t data_off, uint64_t index_off,
                               uint32_t uncompress_buf, const Summary &total) {
  std::vector<uint8_t> b;
  put(b, BIGWIG_MAGIC, 4); put(b, 4, 2); put(b, zooms.size(), 2); put(b, chrom_tree_off, 8); put(b, data_off, 8); put(b, index_off, 8);
  put(b, 0, 2); put(b, 0, 2); put(b, 0, 8); put(b, HEADER_BYTES + ZOOM_HEADER_BYTES * zooms.size(), 8); put(b, uncompress_buf, 4); put(b, 0, 8);
  for (const ZoomHeader &z : zooms) { put(b, z.reduction, 4); put(b, 0, 4); put(b, z.data_off, 8); put(b, z.index_off, 8); }
  put(b, total.valid, 8); put_f64(b, total.min_val); put_f64(b, total.max_val); put_f64(b, total.sum); put_f64(b, total.sum_squares);
  return b;
}

std::vector<uint8_t> rtree_header(uint32_t bs, uint64_t n_items, uint64_t lo, uint64_t hi, uint64_t end_file_off) {
  std::vector<uint8_t> b;
  put(b, RTREE_MAGIC, 4); put(b, bs, 4); put(b, n_items, 8); put(b, lo >> 32, 4); put(b, lo & 0xffffffffu, 4); put(b, hi >> 32, 4);
  put(b, hi & 0xffffffffu, 4); put(b, end_file_off, 8); put(b, 1, 4); put(b, 0, 4);
  return b;
}

}  // namespace brbw
