// --cells-whitelist FILE: the reader of a barcode list (whitelist_file.cpp).  Plain data in and out, no call into the library, so a
// stand-alone probe can test it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace brcli {

// One barcode per line: the first whitespace-delimited field.  A trailing '\r' is dropped; empty lines (and lines of white space)
// and lines starting with '#' are skipped; the last line needs no newline.  -> cb (n x 32 bytes, zero padded) and len (n, 1..32).
// false: `err` names the file and what is wrong -- it cannot be read, a field is longer than 32 bytes (with its line), no barcode
bool read_whitelist_file(const std::string &path, std::vector<uint8_t> &cb, std::vector<uint8_t> &len, std::string &err);

}  // namespace brcli
