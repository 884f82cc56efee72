// The references of a SAM header: its @SQ lines' SN: / LN: fields, in order (what a BAM made from the header lists).  One
// definition for the device reader (sam_reader.cpp) and the command line (host/cli.cpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace br {

// false: an @SQ line without SN:
inline bool sam_header_refs(const char *text, size_t n, std::vector<std::string> &names, std::vector<uint32_t> &lens) {
  for (size_t a = 0; a < n;) {
    const char *nl = (const char *)memchr(text + a, '\n', n - a);
    const size_t e = nl ? (size_t)(nl - text) : n;
    size_t le = e;
    if (le > a && text[le - 1] == '\r') le--;
    const std::string l(text + a, le - a);
    a = e + 1;
    if (l.compare(0, 4, "@SQ\t") != 0) continue;
    std::string sn;
    uint32_t ln = 0;
    bool has_sn = false;
    for (size_t p = 4; p <= l.size();) {
      size_t q = l.find('\t', p);
      if (q == std::string::npos) q = l.size();
      if (l.compare(p, 3, "SN:") == 0) { sn = l.substr(p + 3, q - p - 3); has_sn = true; }
      else if (l.compare(p, 3, "LN:") == 0) ln = (uint32_t)strtoul(l.c_str() + p + 3, nullptr, 10);
      p = q + 1;
    }
    if (!has_sn) return false;
    names.push_back(sn);
    lens.push_back(ln);
  }
  return true;
}

}  // namespace br
