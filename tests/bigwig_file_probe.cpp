// Test probe of bramble_amd/csrc/host/bigwig_file.cpp (tests/test_bigwig_cpu.py builds the two under the address and
// undefined-behaviour sanitizers and runs the result as a child process).
//   probe tree BS N OFF   the chromosome tree of the N names "c000000", "c000001", ... with sizes 100 + i, at file offset OFF: hex
//   probe order NAME...   the chromIds' names in order, one a line, or "refused: REASON" ("-" stands for an empty name, "!" for NULL)
//   probe shape BS N      blockSize, then the items of every level from the leaves up
//   probe head            file_head and rtree_header of fixed numbers: hex, a line each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bramble_amd/csrc/host/bigwig_file.h"

static void hex(const std::vector<uint8_t> &b) {
  for (uint8_t x : b) printf("%02x", x);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string what = argv[1];
  if (what == "tree" && argc == 5) {
    const uint32_t bs = (uint32_t)atoi(argv[2]);
    const int n = atoi(argv[3]);
    std::vector<std::string> names;
    std::vector<const char *> p;
    std::vector<uint32_t> sizes;
    for (int i = 0; i < n; i++) { char b[16]; snprintf(b, sizeof b, "c%06d", i); names.push_back(b); sizes.push_back(100u + (uint32_t)i); }
    for (auto &s : names) p.push_back(s.c_str());
    hex(brbw::chrom_tree(p, sizes, n ? 7 : 0, bs, strtoull(argv[4], nullptr, 10)));
    return 0;
  }
  if (what == "order") {
    std::vector<const char *> p;
    for (int i = 2; i < argc; i++) p.push_back(!strcmp(argv[i], "!") ? nullptr : !strcmp(argv[i], "-") ? "" : argv[i]);
    std::vector<uint32_t> order;
    uint32_t ks = 0;
    std::string err;
    if (!brbw::name_order(p, &order, &ks, &err)) { printf("refused: %s\n", err.c_str()); return 0; }
    printf("%u\n", ks);
    for (uint32_t i : order) printf("%s\n", p[i]);
    return 0;
  }
  if (what == "shape" && argc == 4) {
    const brbw::TreeShape t = brbw::tree_shape(strtoull(argv[3], nullptr, 10), (uint32_t)atoi(argv[2]));
    printf("%u", t.bs);
    for (uint64_t m : t.items) printf(" %llu", (unsigned long long)m);
    printf(" %llu\n", (unsigned long long)t.bytes(32, 24));
    return 0;
  }
  if (what == "head") {
    hex(brbw::file_head({{32, 1000, 2000}, {128, 3000, 1ull << 33}}, 152, 300, 900, 32768, {12, 1.0, 3.0, 22.0, 44.0}));
    hex(brbw::rtree_header(4, 9, (2ull << 32) | 7, (5ull << 32) | 11, 1ull << 32));
    return 0;
  }
  return 2;
}
