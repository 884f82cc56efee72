// Stand-alone probe of bramble_amd/csrc/host/cli_output_files.cpp (test_cli_output_cpu.py builds and runs it; nothing of the library
// is linked).  The inputs below are restated in the test, which builds the expected bytes from them.
//   probe formats DIR              every formatter's file into DIR; one line "fetch <file> <first> <n>" per page a bedGraph asked for
//   probe sidefile PATH MODE FAIL  a SideFile at PATH (MODE text|binary): open, write, close, settle(FAIL, or a failed close); what each returned
#include <string.h>
#include <unistd.h>

#include "../bramble_amd/csrc/host/cli_output_files.h"

using namespace brcli;

static const uint64_t BIG = (1ull << 32) + 5;

static int formats(const std::string &dir) {
  TxTable tx;
  tx.name = {"tA", "tZero", "tB", "tC"};
  tx.len = {1500, 0, (1ll << 32) + 7, 30};
  number_sq(tx);
  const std::vector<double> theta = {5e-7, 123.0, 0.9999995, 1e9 + 0.5}, tpm = {999999.9999995, 7.0, 0.0, 4.4999995e-6}, eff = {1234.5678, 9.0, 0.0005, 29.9995};
  const std::vector<uint64_t> unique = {0, 9, BIG, 3}, ambig = {1ull << 40, 9, 2, BIG};
  auto to = [&](const char *name) { return fopen((dir + "/" + name).c_str(), "w"); };
  FILE *f = to("quant.tsv"); write_quant_table(f, tx, nullptr, theta, tpm, unique, ambig); fclose(f);
  f = to("quant_eff.tsv"); write_quant_table(f, tx, &eff, theta, tpm, unique, ambig); fclose(f);
  // a class on both sides of the transcript without length, one of a single transcript, one of all three
  f = to("classes.txt"); write_quant_classes(f, tx, 3, {0, 2, 3, 6}, {0, 2, 3, 0, 2, 3}, {BIG, 1, 1ull << 40}); fclose(f);
  f = to("classes0.txt"); write_quant_classes(f, tx, 0, {0}, {}, {}); fclose(f);
  std::vector<uint64_t> hist(1001);
  for (size_t k = 0; k < hist.size(); k++) hist[k] = k * k + (k == 1000 ? 1ull << 33 : 0);
  f = to("fld.tsv"); write_fragment_lengths(f, hist); fclose(f);
  // run k: transcripts 0, 2, 3 in turn, [10 k, 10 k + 5), depth k + 1 -- but 2^32 - 1 for run 5
  for (int64_t n_runs : {0, 6, 7, 8}) {
    const std::string name = n_runs == 8 ? "bed_fail" : "bed" + std::to_string(n_runs);
    f = to(name.c_str());
    const int rc = write_bedgraph(f, tx, n_runs, 3, [&](int64_t first, int64_t n, uint32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
      printf("fetch %s %lld %lld\n", name.c_str(), (long long)first, (long long)n);
      if (n_runs == 8 && first == 3) return -3;   // the second page fails: the file ends behind the first
      for (int64_t k = first; k < first + n; k++) {
        const size_t i = (size_t)(k - first);
        tid[i] = (uint32_t)(k % 3 ? k % 3 + 1 : 0); start[i] = (uint32_t)(10 * k); end[i] = (uint32_t)(10 * k + 5); depth[i] = k == 5 ? 0xffffffffu : (uint32_t)(k + 1);
      }
      return 0;
    });
    fclose(f);
    printf("rc %s %d\n", name.c_str(), rc);
  }
  f = to("cov.tsv"); write_coverage_summary(f, tx, {BIG, 1, 0, 7}, {1ull << 40, 1, 1, 10}, {1499, 1, BIG, 20}, {0xffffffffu, 1, 0, 3}); fclose(f);
  return 0;
}

static int sidefile(const char *path, bool binary, bool fail) {
  static const char text[] = "line one\nline two\n", bytes[] = {'a', 0, '\n', '\r', '\r', '\n', 0, 'b'};
  SideFile s(path);
  FILE *f = s.open(binary);
  printf("open %d\n", f != nullptr);
  const size_t n = binary ? sizeof(bytes) : sizeof(text) - 1;
  if (f && (fwrite(binary ? bytes : text, 1, n, f) != n || fflush(f) != 0)) return 1;
  printf("tmp %d\n", access(s.tmp.c_str(), F_OK) == 0);
  const bool closed = s.close();
  printf("close %d\n", (int)closed);
  printf("settle %d\n", (int)s.settle(fail || !closed));   // (as the command line does: a file that failed fails the run)
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "formats")) return formats(argv[2]);
  if (argc == 5 && !strcmp(argv[1], "sidefile")) return sidefile(argv[2], !strcmp(argv[3], "binary"), !strcmp(argv[4], "1"));
  return 2;
}
