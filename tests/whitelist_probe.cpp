// Stand-alone probe of the command line's whitelist reader (bramble_amd/csrc/host/whitelist_file.cpp), built by
// tests/test_whitelist_cpu.py under the address and undefined-behaviour sanitizers and run as a child process.
//   whitelist_probe FILE   ->  "ok <n>" and a line "<len> <barcode>" per barcode (the 32 - len bytes behind it must be 0), exit 0;
//                              or "error <message>", exit 1
#include <cstdio>

#include "../bramble_amd/csrc/host/whitelist_file.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::vector<uint8_t> cb, len;
  std::string err;
  if (!brcli::read_whitelist_file(argv[1], cb, len, err)) {
    printf("error %s\n", err.c_str());
    return cb.empty() && len.empty() ? 1 : 3;   // (a refusal leaves nothing behind)
  }
  if (cb.size() != 32 * len.size()) return 4;
  printf("ok %zu\n", len.size());
  for (size_t i = 0; i < len.size(); i++) {
    for (size_t b = len[i]; b < 32; b++) if (cb[32 * i + b]) return 5;
    printf("%u ", (unsigned)len[i]);
    fwrite(cb.data() + 32 * i, 1, len[i], stdout);
    fputc('\n', stdout);
  }
  return 0;
}
