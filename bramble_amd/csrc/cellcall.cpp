// br_cellcall: which barcodes of a cell x feature count matrix are cells, in one device's HBM (cellcall_kernels.hip; the definitions
// are in bramble_amd.h).
//
//   run      the matrix (CSR by cell, in host or device memory) checked and summed per cell in one launch -- a matrix that is refused
//            has changed nothing; (0xffffffff - total) << 32 | cell sorted by the accumulators' radix driver (barcode_sort.h): the
//            rank order.  The sorted keys come to the host once (8 K bytes): every threshold of the three methods is a total at a
//            rank or the end of a rank prefix, found there by binary search
//   ed       ("method" 2) the ambient counts of the window's cells by integer atomics and the features' flags; both to the host,
//            where br_cellcall_sgt makes the probabilities and the tables (log p, log k, the 2^32-scaled thresholds); the candidates
//            are a rank range, their log-likelihoods one lane each; the simulations in launches of as many as "sim_bytes" of count
//            table holds, a wave each; a block per candidate counts the simulations below it; Benjamini-Hochberg over the
//            candidates on the host (at most "cand_max" of them), and the called ones marked
//
// Device memory (K cells, Z matrix entries, F features, A of them active, m candidates, W distinct candidate totals, n_max the largest,
// S simulations, C of them a launch; every table has one entry more than its items): the object keeps 17 K (status 1, rank 4, order 4,
// total 8) and, after an "ed" run, 32 F (ambient, p, log p, T) + 8 n_max (log k) + 28 m (cell 4, O 8, lower 4, the total's index 4,
// p-value 8 on the host only) and with "keep_sims" 8 W S.  While it runs: a host matrix's copy 8 K + 8 Z; 24 K (two key / index pairs)
// and the sort's histograms; F flags; 16 A (thresholds and log p of the active features), 4 n_max (the totals' indices), 8 W S (L) and
// the count tables 4 A C <= "sim_bytes" (one simulation's table where that is more).  128 bytes of counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "accum.h"
#include "barcode_sort.h"
#include "cellcall.h"
#include "cellcall_kernels.h"
#include "scan_kernels.h"

using namespace br;

struct br_cellcall : Accum {
  // the parameters
  int method = 2;
  int64_t expected = 3000, ind_min = 45000, ind_max = 90000, umi_min = 500, cand_max = 20000, sims = 10000, sim_bytes = 1ll << 31;
  uint64_t seed = 0;
  int keep_sims = 0;
  double percentile = 0.99, ratio = 10.0, umi_frac = 0.01, fdr = 0.01;
  bool ran = false;
  // the run
  int64_t K = 0, F = 0;
  uint64_t nnz = 0, n_called = 0, n_simple = 0, n_ed = 0, thr = 0, window = 0, amb_n = 0, n_active = 0, lo = 0, m = 0, n_max = 0, n_want = 0, chunks = 0;
  uint64_t fallback = 0, sgt[4] = {2, 0, 0, 0};
  double sort_s = 0, amb_s = 0, sim_s = 0, pv_s = 0;
  bool ed = false;   // the ambient tables are there
  std::vector<uint64_t> want_total;
  std::vector<double> pval, padj;
  ColBuf small, status, rank, order, total;
  ColBuf amb, p, lp, T, ln, cand_cell, cand_O, cand_lower, cand_widx, L;
};

extern "C" void br_cellcall_free(br_cellcall *c) {
  if (!c) return;
  c->close();
  delete c;
}

extern "C" int br_cellcall_new(int device, br_cellcall **out) {
  if (!out) return BR_ERR_INVALID_ARG;
  *out = nullptr;
  br_cellcall *c = new br_cellcall();
  int rc = c->open(device);
  if (!rc) rc = c->alloc(c->small, CC_WORDS * 8);
  if (!rc && (hipMemsetAsync(c->small.p, 0, CC_WORDS * 8, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess)) rc = BR_ERR_HIP;
  if (rc) { br_cellcall_free(c); return rc; }
  *out = c;
  return BR_OK;
}

extern "C" int br_cellcall_set_param(br_cellcall *c, const char *name, int64_t v) {
  if (!c || !name || c->ran) return BR_ERR_INVALID_ARG;
  const int64_t i31 = 0x7fffffffll;
  if (!strcmp(name, "method")) { if (v < 0 || v > 2) return BR_ERR_INVALID_ARG; c->method = (int)v; return BR_OK; }
  if (!strcmp(name, "expected")) { if (v < 1 || v > i31) return BR_ERR_INVALID_ARG; c->expected = v; return BR_OK; }
  if (!strcmp(name, "ind_min")) { if (v < 0 || v > i31) return BR_ERR_INVALID_ARG; c->ind_min = v; return BR_OK; }
  if (!strcmp(name, "ind_max")) { if (v < 0 || v > i31) return BR_ERR_INVALID_ARG; c->ind_max = v; return BR_OK; }
  if (!strcmp(name, "umi_min")) { if (v < 0 || v > 0xffffffffll) return BR_ERR_INVALID_ARG; c->umi_min = v; return BR_OK; }
  if (!strcmp(name, "cand_max")) { if (v < 1 || v > i31) return BR_ERR_INVALID_ARG; c->cand_max = v; return BR_OK; }
  if (!strcmp(name, "sims")) { if (v < 1 || v > i31) return BR_ERR_INVALID_ARG; c->sims = v; return BR_OK; }
  if (!strcmp(name, "seed")) { c->seed = (uint64_t)v; return BR_OK; }
  if (!strcmp(name, "sim_bytes")) { if (v < 0) return BR_ERR_INVALID_ARG; c->sim_bytes = v; return BR_OK; }
  if (!strcmp(name, "keep_sims")) { if (v < 0 || v > 1) return BR_ERR_INVALID_ARG; c->keep_sims = (int)v; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

extern "C" int br_cellcall_set_real(br_cellcall *c, const char *name, double v) {
  if (!c || !name || c->ran) return BR_ERR_INVALID_ARG;
  if (!strcmp(name, "percentile")) { if (!(v >= 0.0 && v <= 1.0)) return BR_ERR_INVALID_ARG; c->percentile = v; return BR_OK; }
  if (!strcmp(name, "ratio")) { if (!(v >= 1.0 && v <= 1e9)) return BR_ERR_INVALID_ARG; c->ratio = v; return BR_OK; }
  if (!strcmp(name, "umi_frac")) { if (!(v >= 0.0 && v <= 1.0)) return BR_ERR_INVALID_ARG; c->umi_frac = v; return BR_OK; }
  if (!strcmp(name, "fdr")) { if (!(v >= 0.0 && v <= 1.0)) return BR_ERR_INVALID_ARG; c->fdr = v; return BR_OK; }
  return BR_ERR_INVALID_ARG;
}

// ---- the ambient probabilities (host only; the definition: bramble_amd.h, br_cellcall, paragraph `ambient`) --------------------------
extern "C" int br_cellcall_sgt(const uint64_t *amb, const uint8_t *active, int64_t n, double *p, uint64_t info[4]) {
  if (n < 0 || (n && (!amb || !active || !p))) return BR_ERR_INVALID_ARG;
  std::vector<uint64_t> r;   // the counts of the active features, sorted
  uint64_t N = 0;
  for (int64_t g = 0; g < n; g++) {
    p[g] = 0.0;
    if (active[g]) { r.push_back(amb[g]); N += amb[g]; }
    else if (amb[g]) return BR_ERR_INVALID_ARG;
  }
  const uint64_t n_active = r.size();
  std::sort(r.begin(), r.end());
  std::vector<uint64_t> rv, nr;   // r_1 < ... < r_m and their n_r
  uint64_t n0 = 0;
  for (uint64_t x : r) {
    if (x == 0) n0++;
    else if (!rv.empty() && rv.back() == x) nr.back()++;
    else { rv.push_back(x); nr.push_back(1); }
  }
  const size_t m = rv.size();
  double b = 0.0;
  bool use = m >= 2;
  std::vector<double> rstar(m, 0.0);
  if (use) {
    std::vector<double> lx(m), ly(m);
    double sx = 0.0, sy = 0.0;
    for (size_t j = 0; j < m; j++) {
      const uint64_t prev = j ? rv[j - 1] : 0, next = j + 1 < m ? rv[j + 1] : 2 * rv[j] - rv[j - 1];
      const double Z = 2.0 * (double)nr[j] / (double)(next - prev);
      lx[j] = log((double)rv[j]); ly[j] = log(Z);
      sx = sx + lx[j]; sy = sy + ly[j];
    }
    const double mx = sx / (double)m, my = sy / (double)m;
    double sxy = 0.0, sxx = 0.0;
    for (size_t j = 0; j < m; j++) {
      const double dx = lx[j] - mx;
      sxy = sxy + dx * (ly[j] - my); sxx = sxx + dx * dx;
    }
    b = sxy / sxx;
    use = b < -1.0;
  }
  if (info) { info[0] = use ? 0 : 1; memcpy(&info[1], &b, 8); info[2] = n_active; info[3] = (uint64_t)m; }
  if (!use) {   // add-one smoothing over the active features
    const double den = (double)(N + n_active);
    for (int64_t g = 0; g < n; g++) if (active[g]) p[g] = (double)(amb[g] + 1) / den;
    return BR_OK;
  }
  bool switched = false;
  double Np = 0.0;
  for (size_t j = 0; j < m; j++) {
    const double rr = (double)rv[j], y = rr * pow(1.0 + 1.0 / rr, b + 1.0);
    if (!switched) {
      if (j + 1 >= m || rv[j + 1] != rv[j] + 1) switched = true;
      else {
        const double rp1 = (double)(rv[j] + 1), n1 = (double)nr[j + 1], n0r = (double)nr[j];
        const double x = rp1 * n1 / n0r, sd = sqrt(rp1 * rp1 * (n1 / (n0r * n0r)) * (1.0 + n1 / n0r));
        if (fabs(x - y) <= 1.96 * sd) switched = true;
        else rstar[j] = x;
      }
    }
    if (switched) rstar[j] = y;
    Np = Np + (double)nr[j] * rstar[j];
  }
  const double P0 = (rv[0] == 1 && n0 > 0) ? (double)nr[0] / (double)N : 0.0;
  for (int64_t g = 0; g < n; g++) {
    if (!active[g]) continue;
    if (amb[g] == 0) p[g] = n0 ? P0 / (double)n0 : 0.0;
    else {
      const size_t j = (size_t)(std::lower_bound(rv.begin(), rv.end(), amb[g]) - rv.begin());
      p[g] = (1.0 - P0) * rstar[j] / Np;
    }
  }
  return BR_OK;
}

bool br::cc_fresh(const br_cellcall *c, int device) { return c && !c->ran && c->device == device; }
const uint8_t *br::cc_status(const br_cellcall *c, int64_t *n_cells, uint64_t *n_called) {
  *n_cells = c->K; *n_called = c->n_simple + c->n_ed;
  return c->ran ? c->status.as<uint8_t>() : nullptr;
}

// ---- run ---------------------------------------------------------------------------------------------------------------------------
namespace {
struct Csr { const uint64_t *off; const uint32_t *feat, *cnt; };

inline uint64_t key_total(uint64_t key) { return 0xffffffffull - (key >> 32); }
// the ranks with a total of t or more: a prefix of the (descending) rank order
int64_t count_ge(const std::vector<uint64_t> &key, uint64_t t) {
  int64_t lo = 0, hi = (int64_t)key.size();
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key_total(key[mid]) >= t) lo = mid + 1; else hi = mid; }
  return lo;
}
double stage_seconds(br_cellcall *c, const ScopeTimer &t) { (void)hipStreamSynchronize(c->st); return t.seconds(); }
}  // namespace

// method 2 behind the simple filter: BR_OK with c->fallback set where the ambient profile or a candidate cannot be had
static int cc_emptydrops(br_cellcall *c, const Csr &M, const std::vector<uint64_t> &key) {
  hipStream_t st = c->st;
  const int64_t K = c->K, F = c->F;
  const size_t f1 = (size_t)F + 1;
  // the ambient counts and the features' flags
  const int64_t w0 = c->ind_min, w1 = std::min<int64_t>(c->ind_max, K);
  if (w0 >= w1) { c->fallback = 1; return BR_OK; }
  c->window = (uint64_t)(w1 - w0);
  std::vector<uint64_t> amb((size_t)F);
  std::vector<uint8_t> active((size_t)F);
  {
    const ScopeTimer timer;
    ColBuf flags;
    DropGuard bufs{c, {&flags}};
    RC(c->alloc(c->amb, f1 * 8)); RC(c->alloc(flags, f1));
    HIPCHK(hipMemsetAsync(c->amb.p, 0, f1 * 8, st));
    HIPCHK(hipMemsetAsync(flags.p, 0, f1, st));
    launch_cc_ambient(st, c->order.as<uint32_t>(), w0, w1, M.off, M.feat, M.cnt, c->amb.as<unsigned long long>());
    launch_cc_active(st, M.feat, c->nnz, flags.as<uint8_t>());
    if (F) {
      HIPCHK(hipMemcpyAsync(amb.data(), c->amb.p, (size_t)F * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(active.data(), flags.p, (size_t)F, hipMemcpyDeviceToHost, st));
    }
    c->amb_s = stage_seconds(c, timer);
  }
  c->ed = true;
  for (uint64_t a : amb) c->amb_n += a;
  for (uint8_t a : active) c->n_active += a;
  if (c->amb_n == 0) { c->fallback = 2; return BR_OK; }
  // the candidates: a rank range
  const uint64_t med = key_total(key[(size_t)(c->n_simple / 2)]);
  c->lo = std::max<uint64_t>((uint64_t)std::max<int64_t>(c->umi_min, (int64_t)(c->umi_frac * (double)med + 0.5)), 1);
  const int64_t r0 = (int64_t)c->n_simple, r1 = std::min<int64_t>(count_ge(key, c->lo), r0 + c->cand_max);
  // the probabilities and the tables
  std::vector<double> p((size_t)F), lp((size_t)F, 0.0);
  std::vector<uint64_t> T((size_t)F, 0);
  RC(br_cellcall_sgt(amb.data(), active.data(), F, p.data(), c->sgt));
  std::vector<uint64_t> Td;
  std::vector<double> lpd;
  {
    double cum = 0.0;
    std::vector<double> cums((size_t)F);
    int64_t last = -1;
    for (int64_t g = 0; g < F; g++) { cum = cum + p[g]; cums[g] = cum; if (active[g]) { lp[g] = log(p[g]); last = g; } }
    for (int64_t g = 0; g < F; g++) T[g] = g >= last ? 1ull << 32 : (uint64_t)(cums[g] / cum * 4294967296.0);
    for (int64_t g = 0; g < F; g++) if (active[g]) { Td.push_back(T[g]); lpd.push_back(lp[g]); }
  }
  RC(c->alloc(c->p, f1 * 8)); RC(c->alloc(c->lp, f1 * 8)); RC(c->alloc(c->T, f1 * 8));
  HIPCHK(hipMemcpyAsync(c->p.p, p.data(), (size_t)F * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->lp.p, lp.data(), (size_t)F * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->T.p, T.data(), (size_t)F * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  if (r1 <= r0) { c->fallback = 3; return BR_OK; }
  const int64_t m = r1 - r0;
  c->m = (uint64_t)m;
  c->n_max = key_total(key[(size_t)r0]);
  if (c->n_max >= (1ull << 28)) return BR_ERR_CAPACITY;
  const uint32_t n_max = (uint32_t)c->n_max, sims = (uint32_t)c->sims;
  // the wanted totals, ascending, and where each candidate's is
  std::vector<uint32_t> want((size_t)n_max + 1, CC_NONE), widx((size_t)m);
  for (int64_t j = m - 1; j >= 0; j--) {
    const uint64_t t = key_total(key[(size_t)(r0 + j)]);
    if (c->want_total.empty() || c->want_total.back() != t) { want[(size_t)t] = (uint32_t)c->want_total.size(); c->want_total.push_back(t); }
    widx[(size_t)j] = want[(size_t)t];
  }
  c->n_want = c->want_total.size();
  std::vector<double> ln((size_t)n_max + 2, 0.0);
  for (uint32_t k = 1; k <= n_max + 1; k++) ln[k] = log((double)k);
  // the observed log-likelihoods
  ColBuf d_T, d_lp, d_want, table;
  DropGuard bufs{c, {&d_T, &d_lp, &d_want, &table}};
  const size_t A = Td.size();
  RC(c->alloc(c->ln, ln.size() * 8)); RC(c->alloc(d_want, want.size() * 4)); RC(c->alloc(d_T, (A + 1) * 8)); RC(c->alloc(d_lp, (A + 1) * 8));
  RC(c->alloc(c->cand_cell, ((size_t)m + 1) * 4)); RC(c->alloc(c->cand_O, ((size_t)m + 1) * 8)); RC(c->alloc(c->cand_lower, ((size_t)m + 1) * 4));
  RC(c->alloc(c->cand_widx, ((size_t)m + 1) * 4));
  HIPCHK(hipMemcpyAsync(c->ln.p, ln.data(), ln.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_want.p, want.data(), want.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_T.p, Td.data(), A * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_lp.p, lpd.data(), A * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->cand_widx.p, widx.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
  launch_cc_observed(st, c->order.as<uint32_t>(), r0, m, M.off, M.feat, M.cnt, c->ln.as<double>(), c->lp.as<double>(), c->cand_cell.as<uint32_t>(),
                     c->cand_O.as<double>());
  HIPCHK(hipStreamSynchronize(st));   // (the host tables are read until here)
  // the simulations
  {
    const ScopeTimer timer;
    RC(c->alloc(c->L, ((size_t)c->n_want * sims + 1) * 8));
    const uint64_t per = (uint64_t)A * 4;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(sims, std::max<uint64_t>(1, (uint64_t)c->sim_bytes / per));
    RC(c->alloc(table, (size_t)chunk * per));
    CcSimArgs S{};
    S.T = d_T.as<uint64_t>(); S.lp = d_lp.as<double>(); S.n_active = (uint32_t)A;
    while (S.bits < 32 && (A - 1) >> S.bits) S.bits++;
    S.ln = c->ln.as<double>(); S.want = d_want.as<uint32_t>(); S.n_max = n_max;
    S.sims = sims; S.k0 = (uint32_t)c->seed; S.k1 = (uint32_t)(c->seed >> 32);
    S.table = table.as<uint32_t>(); S.L = c->L.as<double>();
    for (uint32_t s = 0; s < sims; s += chunk) {
      S.s_first = s; S.n_sims = std::min(chunk, sims - s);
      HIPCHK(hipMemsetAsync(table.p, 0, (size_t)S.n_sims * per, st));
      launch_cc_simulate(st, S);
      c->chunks++;
    }
    HIPCHK(hipGetLastError());
    c->sim_s = stage_seconds(c, timer);
  }
  // the p-values and Benjamini-Hochberg
  const ScopeTimer timer;
  std::vector<uint32_t> lower((size_t)m), cell((size_t)m);
  launch_cc_lower(st, c->L.as<double>(), sims, c->cand_widx.as<uint32_t>(), c->cand_O.as<double>(), m, c->cand_lower.as<uint32_t>());
  HIPCHK(hipMemcpyAsync(lower.data(), c->cand_lower.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int64_t> by((size_t)m);
  std::iota(by.begin(), by.end(), 0);
  std::stable_sort(by.begin(), by.end(), [&](int64_t a, int64_t b) { return lower[(size_t)a] < lower[(size_t)b]; });
  c->pval.resize((size_t)m); c->padj.resize((size_t)m);
  for (int64_t j = 0; j < m; j++) c->pval[(size_t)j] = (double)(lower[(size_t)j] + 1) / (double)(sims + 1);
  std::vector<uint8_t> called((size_t)m, 0);
  double run = 1.0;
  for (int64_t pos = m; pos >= 1; pos--) {
    const size_t j = (size_t)by[(size_t)(pos - 1)];
    const double q = std::min(1.0, c->pval[j] * (double)m / (double)pos);
    run = std::min(run, q);
    c->padj[j] = run;
    if (run <= c->fdr) { called[j] = 1; c->n_ed++; }
  }
  ColBuf d_called;
  DropGuard bufs2{c, {&d_called}};
  RC(c->alloc(d_called, (size_t)m + 1));
  HIPCHK(hipMemcpyAsync(d_called.p, called.data(), (size_t)m, hipMemcpyHostToDevice, st));
  launch_cc_mark(st, c->cand_cell.as<uint32_t>(), d_called.as<uint8_t>(), m, c->status.as<uint8_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  if (!c->keep_sims) c->drop(c->L);
  c->pv_s = timer.seconds();
  return BR_OK;
}

int br::cc_run(br_cellcall *c, int64_t n_cells, int64_t n_features, const uint64_t *d_off, const uint32_t *d_feat, const uint32_t *d_cnt, uint64_t nnz) {
  hipStream_t st = c->st;
  const Csr M{d_off, d_feat, d_cnt};
  const size_t k1 = (size_t)n_cells + 1;
  uint64_t *small = c->small.as<uint64_t>();
  std::vector<uint64_t> key((size_t)n_cells);
  {
    const ScopeTimer timer;
    ColBuf total, tmp;
    SortBufs s;
    DropGuard bufs{c, {&total, &tmp, &s.key[0], &s.key[1], &s.idx[0], &s.idx[1]}};
    RC(c->alloc(total, k1 * 8)); RC(s.make(c, (size_t)n_cells));
    HIPCHK(hipMemsetAsync(small, 0, CC_WORDS * 8, st));
    launch_cc_totals(st, n_cells, n_features, nnz, M.off, M.feat, M.cnt, total.as<uint64_t>(), s.key[0].as<uint64_t>(), s.idx[0].as<uint32_t>(),
                     c->small.as<unsigned long long>());
    uint64_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, small + CC_BAD, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return BR_ERR_INVALID_ARG;   // (nothing of the object has changed)
    RC(sort_pairs(c, s, n_cells, tmp, small + CC_BITS));
    if (n_cells) HIPCHK(hipMemcpyAsync(key.data(), s.key[0].p, (size_t)n_cells * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::swap(c->total, total); std::swap(c->order, s.idx[0]);
    c->sort_s = timer.seconds();
  }
  c->ran = true; c->K = n_cells; c->F = n_features; c->nnz = nnz;
  RC(c->alloc(c->status, k1)); RC(c->alloc(c->rank, k1 * 4));
  const int64_t K = n_cells;
  if (K) {
    if (c->method == 0) c->thr = std::max<uint64_t>(key_total(key[(size_t)(std::min<int64_t>(c->expected, K) - 1)]), 1);
    else {
      const int64_t r = std::min<int64_t>(K - 1, (int64_t)((double)c->expected * (1.0 - c->percentile)));
      const uint64_t tmax = key_total(key[(size_t)r]);
      c->thr = (uint64_t)std::max<int64_t>(1, (int64_t)((double)tmax / c->ratio + 0.5));
    }
    c->n_simple = (uint64_t)count_ge(key, c->thr);
  }
  launch_cc_rank(st, c->order.as<uint32_t>(), K, (int64_t)c->n_simple, c->rank.as<uint32_t>(), c->status.as<uint8_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  if (c->method == 2 && K) RC(cc_emptydrops(c, M, key));
  return BR_OK;
}

extern "C" int br_cellcall_run(br_cellcall *c, int64_t n_cells, int64_t n_features, const uint64_t *cell_off, const uint32_t *feature,
                               const uint32_t *count, int on_device, void *stream) {
  if (!c || c->ran || n_cells < 0 || n_cells >= (1ll << 31) || n_features < 0 || n_features >= (1ll << 31) || !cell_off) return BR_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->st;
  uint64_t ends[2] = {0, 0};
  if (on_device) {
    RC(c->after((hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(&ends[0], cell_off, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&ends[1], cell_off + n_cells, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  } else { ends[0] = cell_off[0]; ends[1] = cell_off[n_cells]; }
  const uint64_t nnz = ends[1];
  if (ends[0] != 0 || nnz >= (1ull << 40) || (nnz && (!feature || !count))) return BR_ERR_INVALID_ARG;
  if (on_device) return cc_run(c, n_cells, n_features, cell_off, feature, count, nnz);
  for (int64_t i = 0; i < n_cells; i++) if (cell_off[i] > cell_off[i + 1]) return BR_ERR_INVALID_ARG;   // (what bounds the copies below)
  ColBuf off, feat, cnt;
  DropGuard bufs{c, {&off, &feat, &cnt}};
  RC(c->alloc(off, ((size_t)n_cells + 1) * 8)); RC(c->alloc(feat, ((size_t)nnz + 1) * 4)); RC(c->alloc(cnt, ((size_t)nnz + 1) * 4));
  HIPCHK(hipMemcpyAsync(off.p, cell_off, ((size_t)n_cells + 1) * 8, hipMemcpyHostToDevice, st));
  if (nnz) {
    HIPCHK(hipMemcpyAsync(feat.p, feature, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cnt.p, count, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  return cc_run(c, n_cells, n_features, off.as<uint64_t>(), feat.as<uint32_t>(), cnt.as<uint32_t>(), nnz);
}

// ---- reading out ---------------------------------------------------------------------------------------------------------------------
namespace {
struct Piece { void *to; const ColBuf *from; size_t width; };
bool slice_ok(int64_t first, int64_t n, uint64_t have) { return first >= 0 && n >= 0 && (uint64_t)first <= have && (uint64_t)n <= have - (uint64_t)first; }
int read_out(br_cellcall *c, int64_t first, int64_t n, std::initializer_list<Piece> pieces) {
  if (n == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  for (const Piece &x : pieces)
    if (x.to) HIPCHK(hipMemcpyAsync(x.to, (const uint8_t *)x.from->p + (size_t)first * x.width, (size_t)n * x.width, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}
}  // namespace

extern "C" int br_cellcall_calls(br_cellcall *c, int64_t first, int64_t n, uint8_t *status, uint32_t *rank, uint64_t *total) {
  if (!c || !c->ran || !slice_ok(first, n, (uint64_t)c->K)) return BR_ERR_INVALID_ARG;
  return read_out(c, first, n, {{status, &c->status, 1}, {rank, &c->rank, 4}, {total, &c->total, 8}});
}

extern "C" int br_cellcall_ambient(br_cellcall *c, int64_t first, int64_t n, uint64_t *amb, double *p, double *lp, uint64_t *T) {
  if (!c || !c->ran || !c->ed || !slice_ok(first, n, (uint64_t)c->F)) return BR_ERR_INVALID_ARG;
  if (!c->p.p && (p || lp || T)) return BR_ERR_INVALID_ARG;   // (a zero ambient sum: there are only the counts)
  return read_out(c, first, n, {{amb, &c->amb, 8}, {p, &c->p, 8}, {lp, &c->lp, 8}, {T, &c->T, 8}});
}

extern "C" int br_cellcall_logtable(br_cellcall *c, int64_t first, int64_t n, double *ln) {
  if (!c || !c->ran || !slice_ok(first, n, c->m ? c->n_max + 2 : 0)) return BR_ERR_INVALID_ARG;
  return read_out(c, first, n, {{ln, &c->ln, 8}});
}

extern "C" int br_cellcall_candidates(br_cellcall *c, int64_t first, int64_t n, uint32_t *cell, double *O, uint32_t *lower, double *pval, double *padj) {
  if (!c || !c->ran || !slice_ok(first, n, c->m)) return BR_ERR_INVALID_ARG;
  if (pval && n) memcpy(pval, c->pval.data() + first, (size_t)n * 8);
  if (padj && n) memcpy(padj, c->padj.data() + first, (size_t)n * 8);
  return read_out(c, first, n, {{cell, &c->cand_cell, 4}, {O, &c->cand_O, 8}, {lower, &c->cand_lower, 4}});
}

extern "C" int br_cellcall_wanted(br_cellcall *c, int64_t first, int64_t n, uint64_t *total) {
  if (!c || !c->ran || !slice_ok(first, n, c->n_want)) return BR_ERR_INVALID_ARG;
  if (total && n) memcpy(total, c->want_total.data() + first, (size_t)n * 8);
  return BR_OK;
}

extern "C" int br_cellcall_sims(br_cellcall *c, int64_t s_first, int64_t n_s, int64_t w_first, int64_t n_w, double *L) {
  if (!c || !c->ran || !c->L.p || !slice_ok(s_first, n_s, (uint64_t)c->sims) || !slice_ok(w_first, n_w, c->n_want)) return BR_ERR_INVALID_ARG;
  if (!L || n_s == 0 || n_w == 0) return BR_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy2DAsync(L, (size_t)n_s * 8, c->L.as<double>() + (size_t)w_first * (size_t)c->sims + (size_t)s_first, (size_t)c->sims * 8, (size_t)n_s * 8,
                          (size_t)n_w, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return BR_OK;
}

extern "C" int br_cellcall_stats(const br_cellcall *c, uint64_t out[32]) {
  if (!c || !out) return BR_ERR_INVALID_ARG;
  const uint64_t v[32] = {(uint64_t)c->K, c->n_simple, c->n_ed, c->thr, c->n_simple, c->window, c->amb_n, c->n_active, c->sgt[0], c->sgt[1], c->lo, c->m,
                          c->n_max, c->n_want, c->chunks, c->fallback, (uint64_t)(c->sort_s * 1e6), (uint64_t)(c->amb_s * 1e6),
                          (uint64_t)(c->sim_s * 1e6), (uint64_t)(c->pv_s * 1e6), (uint64_t)c->method, (uint64_t)c->sims, c->live, c->peak, c->nnz,
                          (uint64_t)c->F, 0, 0, 0, 0, 0, 0};
  memcpy(out, v, sizeof(v));
  return BR_OK;
}
