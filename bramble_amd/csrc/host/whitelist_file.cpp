// --cells-whitelist FILE (whitelist_file.h)
#include "whitelist_file.h"

#include <cerrno>
#include <cstdio>
#include <cstring>

namespace brcli {

bool read_whitelist_file(const std::string &path, std::vector<uint8_t> &cb, std::vector<uint8_t> &len, std::string &err) {
  cb.clear(); len.clear();
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { err = "--cells-whitelist: could not read " + path + ": " + strerror(errno); return false; }
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) { err = "--cells-whitelist: could not read " + path; return false; }
  auto blank = [](char ch) { return ch == ' ' || ch == '\t' || ch == '\v' || ch == '\f' || ch == '\r'; };
  size_t line = 0;
  for (size_t at = 0; at < text.size();) {
    size_t end = text.find('\n', at);
    if (end == std::string::npos) end = text.size();
    size_t a = at, b = end;
    at = end + 1; line++;
    if (b > a && text[b - 1] == '\r') b--;
    if (a < b && text[a] == '#') continue;
    while (a < b && blank(text[a])) a++;
    size_t e = a;
    while (e < b && !blank(text[e])) e++;
    if (e == a) continue;
    if (e - a > 32) {
      err = "--cells-whitelist: " + path + " line " + std::to_string(line) + ": a barcode of " + std::to_string(e - a) + " bytes (32 at most)";
      cb.clear(); len.clear();
      return false;
    }
    cb.resize(cb.size() + 32, 0);
    memcpy(cb.data() + cb.size() - 32, text.data() + a, e - a);
    len.push_back((uint8_t)(e - a));
  }
  if (len.empty()) { err = "--cells-whitelist: " + path + " holds no barcode"; return false; }
  return true;
}

}  // namespace brcli
