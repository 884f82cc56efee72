// SAM text -> BAM records on the device: the front end of br_sam_reader (sam_reader.cpp).  Its output is laid out the way
// br_bam_split_device lays out an inflated BAM stream ([block_size][record]..., rec_off = each record's refID word), so
// everything from the record split on (br_project_bam_resident) runs unchanged.  The reference never parses text itself:
// htslib's sam_parse1 turns each line into a bam1_t (gclib/GSam.h over hts_open), and bam_write1 is what a BAM file made
// from the same text holds.  The rules below restate what those two produce; each is repeated at the code that applies it.
//
//   k_sam_nl_count / k_sam_nl_write   line index: 64 KiB per block, 16-byte loads, '\n' counted with wave ballots
//   (launch_scan, scan_kernels.h)     exclusive scans
//   k_sam_measure                     one wave per line: fields, tags, CIGAR -> block_size, mapped / unmapped, error code
//   k_sam_emit                        one wave per mapped line: the BAM record, every write inside the measured size
//
// Malformed text never faults: every read is checked against the end of its line, every write against the record's
// measured size, and a bad line only sets an error code (the lowest bad line wins: first_bad).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sam_kernels.h"
#include "wave_inl.h"

namespace br {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4u __attribute__((aligned(1)));

// ---- line index -----------------------------------------------------------------------------------
// 16 bytes of text at a (a multiple of 16 from the buffer's start); bytes at or past n read as 0 (nothing past n is touched)
__device__ __forceinline__ void load16(const uint8_t *t, uint64_t a, uint64_t n, uint8_t b[16]) {
  if (a + 16 <= n) {
    const uint4 v = *(const uint4 *)(t + a);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  } else {
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = a + j < n ? t[a + j] : 0;
  }
}

__global__ void __launch_bounds__(256) k_sam_nl_count(const uint8_t *t, uint64_t n, uint64_t *tile_cnt) {
  __shared__ uint32_t sh[4];
  const uint64_t base = (uint64_t)blockIdx.x * SAM_NL_TILE;
  uint32_t cnt = 0;   // wave-uniform
  for (int it = 0; it < (int)(SAM_NL_TILE / 4096); it++) {
    const uint64_t a = base + (uint64_t)it * 4096 + threadIdx.x * 16;
    uint8_t b[16];
    load16(t, a, n, b);
#pragma unroll
    for (int j = 0; j < 16; j++) cnt += (uint32_t)__popcll(__ballot(b[j] == '\n'));
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint64_t)sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void __launch_bounds__(256) k_sam_nl_write(const uint8_t *t, uint64_t n, const uint64_t *tile_pre, uint64_t *lend) {
  __shared__ uint64_t sh[4];
  const uint64_t base = (uint64_t)blockIdx.x * SAM_NL_TILE;
  uint64_t out = tile_pre[blockIdx.x];
  for (int it = 0; it < (int)(SAM_NL_TILE / 4096); it++) {
    const uint64_t a = base + (uint64_t)it * 4096 + threadIdx.x * 16;
    uint8_t b[16];
    load16(t, a, n, b);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) m |= (uint32_t)(b[j] == '\n') << j;
    uint64_t tot;
    uint64_t k = out + block_excl_scan_256((uint64_t)__popc(m), sh, tot);
    while (m) { const int j = __ffs(m) - 1; m &= m - 1; lend[k++] = a + (uint64_t)j; }
    out += tot;
  }
}

// ---- one wave per line ----------------------------------------------------------------------------
__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// The bytes of [lo, hi) in the window of 1024 bytes at wb (16-aligned) that match KIND (0: '\t', 1: not a digit) ->
// pos[0 .. return value), ascending, relative to the line start ls.  Wave-uniform result; one block = one wave.
template <int KIND>
__device__ uint32_t wfind(const uint8_t *t, uint64_t wb, uint64_t lo, uint64_t hi, uint64_t ls, uint32_t *pos) {
  const int lane = threadIdx.x;
  const uint64_t a = wb + (uint64_t)lane * 16;
  uint8_t b[16];
  if (a >= lo && a + 16 <= hi) load16(t, a, hi, b);
  else {
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = (a + j >= lo && a + j < hi) ? t[a + j] : 0;
  }
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const bool in = a + j >= lo && a + j < hi;
    const bool hit = KIND == 0 ? b[j] == '\t' : !is_digit(b[j]);
    m |= (uint32_t)(in && hit) << j;
  }
  const uint32_t c = (uint32_t)__popc(m);
  const uint32_t incl = wave_scan(c);
  const uint32_t total = __shfl(incl, 63);
  __syncthreads();   // (the caller is done with the previous window's positions)
  uint32_t k = incl - c;
  while (m) { const int j = __ffs(m) - 1; m &= m - 1; pos[k++] = (uint32_t)(a + (uint64_t)j - ls); }
  __syncthreads();
  return total;
}

// decimal [s, s + n) -> v in [lo, hi]; an optional sign when lo < 0.  False for anything else.
__device__ bool parse_int(const uint8_t *s, uint32_t n, int64_t lo, int64_t hi, int64_t &v) {
  uint32_t i = 0;
  bool neg = false;
  if (n && lo < 0 && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
  if (i == n) return false;
  while (i + 1 < n && s[i] == '0') i++;
  if (n - i > 18) return false;
  int64_t x = 0;
  for (; i < n; i++) { if (!is_digit(s[i])) return false; x = x * 10 + (s[i] - '0'); }
  v = neg ? -x : x;
  return v >= lo && v <= hi;
}

__constant__ double c_p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// 'f' values are (float)strtod(text): two roundings, first to double, then to float.  The device takes Clinger's exact case:
// [+-]digits[.digits][(e|E)[+-]digits] with a decimal mantissa <= 2^53 (at most 19 significant digits) and a power of ten
// within 10^+-22 -- the mantissa and the power are exact doubles, so one IEEE multiply or divide is the correctly rounded
// double strtod returns; the cast to float is the second rounding.  Anything else (long mantissas, subnormals, huge
// exponents, inf / nan / hex) goes to the host, which calls strtod itself (SamFix).
__device__ bool fast_float(const uint8_t *s, uint32_t n, float &out) {
  uint32_t i = 0;
  bool neg = false, any = false;
  if (i < n && (s[i] == '-' || s[i] == '+')) { neg = s[i] == '-'; i++; }
  uint64_t m = 0;
  int nd = 0, e10 = 0;
  for (; i < n && is_digit(s[i]); i++) {
    any = true;
    if (m == 0 && s[i] == '0') continue;
    if (nd >= 19) return false;
    m = m * 10 + (s[i] - '0'); nd++;
  }
  if (i < n && s[i] == '.') {
    for (i++; i < n && is_digit(s[i]); i++) {
      any = true;
      if (m == 0 && s[i] == '0') { e10--; continue; }
      if (nd >= 19) return false;
      m = m * 10 + (s[i] - '0'); nd++; e10--;
    }
  }
  if (!any) return false;
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    i++;
    bool eneg = false;
    if (i < n && (s[i] == '-' || s[i] == '+')) { eneg = s[i] == '-'; i++; }
    if (i == n) return false;
    int ex = 0;
    for (; i < n && is_digit(s[i]); i++) { if (ex < 100000) ex = ex * 10 + (s[i] - '0'); }
    e10 += eneg ? -ex : ex;
  }
  if (i != n) return false;
  if (m == 0) { out = neg ? -0.0f : 0.0f; return true; }
  if (m > (1ull << 53) || e10 < -22 || e10 > 22) return false;
  double d = (double)m;
  d = e10 >= 0 ? d * c_p10[e10] : d / c_p10[-e10];
  out = (float)(neg ? -d : d);
  return true;
}

// The text strtod takes whole (the measure pass checks every float here, so a malformed one is an error of its own line whether
// the line is mapped or not): leading white space, a sign, then digits with an optional fraction and decimal exponent, a hex
// mantissa ("0x") with an optional binary exponent, "inf" / "infinity", or "nan" with an optional "(chars)".  An exponent
// marker without digits is not taken by strtod, so it is malformed here.
__device__ bool float_syntax(const uint8_t *s, uint32_t n) {
  uint32_t i = 0;
  auto lower = [](uint8_t c) { return (uint8_t)(c >= 'A' && c <= 'Z' ? c + 32 : c); };
  auto word = [&](const char *w) { uint32_t k = 0; while (w[k] && i + k < n && lower(s[i + k]) == (uint8_t)w[k]) k++; if (w[k]) return false; i += k; return true; };
  auto is_hex = [&](uint8_t c) { c = lower(c); return is_digit(c) || (c >= 'a' && c <= 'f'); };
  while (i < n && (s[i] == ' ' || s[i] == '\v' || s[i] == '\f' || s[i] == '\r')) i++;
  if (i < n && (s[i] == '-' || s[i] == '+')) i++;
  if (word("infinity") || word("inf")) return i == n;
  if (word("nan")) {
    if (i < n && s[i] == '(') {
      uint32_t j = i + 1;
      while (j < n && (is_digit(s[j]) || (lower(s[j]) >= 'a' && lower(s[j]) <= 'z') || s[j] == '_')) j++;
      if (j < n && s[j] == ')') i = j + 1;
    }
    return i == n;
  }
  const bool hex = i + 1 < n && s[i] == '0' && lower(s[i + 1]) == 'x';
  uint32_t j = hex ? i + 2 : i, nd = 0;
  for (; j < n && (hex ? is_hex(s[j]) : is_digit(s[j])); j++) nd++;
  if (j < n && s[j] == '.') for (j++; j < n && (hex ? is_hex(s[j]) : is_digit(s[j])); j++) nd++;
  if (nd == 0) return false;
  if (j < n && (hex ? lower(s[j]) == 'p' : lower(s[j]) == 'e')) {
    j++;
    if (j < n && (s[j] == '-' || s[j] == '+')) j++;
    uint32_t ne = 0;
    for (; j < n && is_digit(s[j]); j++) ne++;
    if (ne == 0) return false;
  }
  return j == n;
}

__device__ __forceinline__ void put16(uint8_t *d, uint32_t v) { d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void put32(uint8_t *d, uint32_t v) { d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24); }

// B-array subtype -> element size (0: not a subtype)
__device__ __forceinline__ uint32_t b_size(uint8_t c) {
  return c == 'c' || c == 'C' ? 1u : c == 's' || c == 'S' ? 2u : c == 'i' || c == 'I' || c == 'f' ? 4u : 0u;
}
// one B-array element [s, s + n) of subtype sub at d (d == null: check only).  False: does not parse or overflows.
__device__ bool b_elem(const SamArgs &A, const uint8_t *s, uint32_t n, uint8_t sub, uint8_t *d, uint32_t line) {
  if (sub == 'f') {
    if (n == 0 || (!d && !float_syntax(s, n))) return false;
    float f;
    if (fast_float(s, n, f)) { if (d) put32(d, __float_as_uint(f)); return true; }
    if (d) {
      const uint32_t k = atomicAdd(A.n_fix, 1u);
      if (k < A.fix_cap) A.fix[k] = SamFix{(uint64_t)(d - A.blob), (uint64_t)(s - A.text), n, line};
    }
    return true;
  }
  int64_t lo = 0, hi = 0;
  switch (sub) {
    case 'c': lo = -128; hi = 127; break;
    case 'C': lo = 0; hi = 255; break;
    case 's': lo = -32768; hi = 32767; break;
    case 'S': lo = 0; hi = 65535; break;
    case 'i': lo = -2147483648ll; hi = 2147483647ll; break;
    default: lo = 0; hi = 4294967295ll; break;
  }
  int64_t v;
  if (!parse_int(s, n, lo, hi, v)) return false;
  if (d) { const uint32_t es = b_size(sub); for (uint32_t k = 0; k < es; k++) d[k] = (uint8_t)((uint64_t)v >> (8 * k)); }
  return true;
}

// One tag "XX:T:value" = text[s, e) -> its BAM bytes at d (d == null: size only).  Returns the size; *err on a bad tag.
//   A      one byte
//   i      the smallest type that holds the value: < 0: >= -128 c, >= -32768 s, else i; >= 0: <= 255 C, <= 65535 S, else I;
//          outside [-2^31, 2^32 - 1] an error
//   f      (float)strtod(text) (fast_float, or the host)
//   Z, H   the text and a NUL
//   B      subtype (cCsSiIf), a 32-bit count, the values in that subtype
// zmax: Z / H values longer than this are left to the caller (header and NUL written, the body not): the emit pass copies them
// with the whole wave (minimap2's MM:Z on ultra-long reads is tens of kB)
constexpr uint32_t SAM_ZMAX = 128;
__device__ uint32_t tag_bytes(const SamArgs &A, uint64_t s, uint64_t e, uint8_t *d, uint32_t line, uint32_t &err,
                              uint32_t zmax = 0xffffffffu) {
  const uint8_t *t = A.text;
  auto bad = [&](uint32_t code) { if (!err) err = code; return 0u; };
  if (e < s + 5 || t[s + 2] != ':' || t[s + 4] != ':') return bad(SAM_E_TAG);
  const uint8_t c0 = t[s], c1 = t[s + 1];
  const bool a0 = (c0 >= 'A' && c0 <= 'Z') || (c0 >= 'a' && c0 <= 'z');
  const bool a1 = a0 && ((c1 >= 'A' && c1 <= 'Z') || (c1 >= 'a' && c1 <= 'z') || is_digit(c1));
  if (!a1) return bad(SAM_E_TAG);
  const uint8_t ty = t[s + 3];
  const uint64_t v = s + 5;
  const uint32_t n = (uint32_t)(e - v);
  if (d) { d[0] = c0; d[1] = c1; }
  switch (ty) {
    case 'A':
      if (n != 1) return bad(SAM_E_TAG);
      if (d) { d[2] = 'A'; d[3] = t[v]; }
      return 4;
    case 'i': {
      int64_t x;
      if (!parse_int(t + v, n, -2147483648ll, 4294967295ll, x)) {
        int64_t y;   // a number outside the range, or no number at all
        return bad(parse_int(t + v, n, -999999999999999999ll, 999999999999999999ll, y) || n > 18 ? SAM_E_TAG_RANGE : SAM_E_TAG);
      }
      uint8_t ct; uint32_t w;
      if (x < 0) { if (x >= -128) { ct = 'c'; w = 1; } else if (x >= -32768) { ct = 's'; w = 2; } else { ct = 'i'; w = 4; } }
      else { if (x <= 255) { ct = 'C'; w = 1; } else if (x <= 65535) { ct = 'S'; w = 2; } else { ct = 'I'; w = 4; } }
      if (d) { d[2] = ct; for (uint32_t k = 0; k < w; k++) d[3 + k] = (uint8_t)((uint64_t)x >> (8 * k)); }
      return 3 + w;
    }
    case 'f': {
      if (n == 0) return bad(SAM_E_FLOAT);   // an empty value is a malformed float, as an empty B:f element is
      if (!d && !float_syntax(t + v, n)) return bad(SAM_E_FLOAT);
      if (d) { d[2] = 'f'; if (!b_elem(A, t + v, n, 'f', d + 3, line)) return bad(SAM_E_TAG); }
      return 7;
    }
    case 'Z':
    case 'H':
      if (d) { d[2] = ty; if (n <= zmax) for (uint32_t k = 0; k < n; k++) d[3 + k] = t[v + k]; d[3 + n] = 0; }
      return 4 + n;
    case 'B': {
      if (n < 1) return bad(SAM_E_TAG);
      const uint8_t sub = t[v];
      const uint32_t es = b_size(sub);
      if (!es) return bad(SAM_E_TAG);
      uint32_t cnt = 0;
      if (n > 1) {
        if (t[v + 1] != ',') return bad(SAM_E_TAG);
        uint64_t p = v + 2;
        for (;;) {
          uint64_t q = p;
          while (q < e && t[q] != ',') q++;
          if (!b_elem(A, t + p, (uint32_t)(q - p), sub, d ? d + 8 + (uint64_t)es * cnt : nullptr, line))
            return bad(sub == 'f' ? SAM_E_FLOAT : q > p ? SAM_E_TAG_RANGE : SAM_E_TAG);
          cnt++;
          if (q >= e) break;
          p = q + 1;
        }
      }
      if (d) { d[2] = 'B'; d[3] = sub; put32(d + 4, cnt); }
      return 8 + es * cnt;
    }
    default:
      return bad(SAM_E_TAG);
  }
}

// ref name [s, s + n) -> @SQ index, -1 when the header has no such name
__device__ int32_t ref_lookup(const SamArgs &A, const uint8_t *s, uint32_t n) {
  if (A.n_ref <= 0) return -1;
  uint64_t h = 1469598103934665603ull;
  for (uint32_t k = 0; k < n; k++) { h ^= s[k]; h *= 1099511628211ull; }
  for (uint32_t k = (uint32_t)h & A.h_mask;; k = (k + 1) & A.h_mask) {
    const int32_t r = A.h_slot[k];
    if (r < 0) return -1;
    const uint64_t o = A.name_off[r], l = A.name_off[r + 1] - o;
    if (l != n) continue;
    bool eq = true;
    for (uint32_t j = 0; j < n && eq; j++) eq = A.names[o + j] == s[j];
    if (eq) return r;
  }
}

// CIGAR op letter -> BAM op code (MIDNSHP=X), -1 for anything else
__device__ __forceinline__ int cig_op(uint8_t c) {
  switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1;
  }
}

// The CIGAR field [cs, ce) of the line at ls (relative offsets): every op is 1-9 digits (< 2^28) and one of MIDNSHP=X.
// Counts ops, query length (M I S = X) and reference length (M D N = X); writes the op words at ops when not null.
// Wave-cooperative: the op letters of a 1024-byte window are found with ballots, one lane per op.
__device__ void cigar_walk(const SamArgs &A, uint64_t ls, uint32_t cs, uint32_t ce, uint32_t *pos, uint8_t *ops,
                           uint32_t &n_ops, uint64_t &qlen, uint64_t &rlen, uint32_t &err) {
  const int lane = threadIdx.x;
  const uint8_t *t = A.text;
  uint32_t prev = cs - 1, n = 0, lerr = 0;
  uint64_t q = 0, r = 0;
  for (uint64_t wb = (ls + cs) & ~15ull; wb < ls + ce; wb += 1024) {
    const uint32_t T = wfind<1>(t, wb, ls + cs, ls + ce, ls, pos);
    for (uint32_t k = lane; k < T; k += 64) {
      const uint32_t p = pos[k], pp = k ? pos[k - 1] : prev;
      const uint32_t nd = p - pp - 1;
      const int op = cig_op(t[ls + p]);
      if (nd == 0 || nd > 9 || op < 0) { lerr = SAM_E_CIGAR; continue; }
      uint32_t len = 0;
      for (uint32_t j = pp + 1; j < p; j++) len = len * 10 + (t[ls + j] - '0');
      if (len >= (1u << 28)) { lerr = SAM_E_CIGAR; continue; }
      if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) q += len;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) r += len;
      if (ops) put32(ops + 4ull * (n + k), len << 4 | (uint32_t)op);
    }
    if (T) prev = pos[T - 1];
    n += T;
  }
  if (prev != ce - 1) lerr = SAM_E_CIGAR;   // digits after the last op (or no op at all)
  q = wave_sum(q); r = wave_sum(r); lerr = wave_max(lerr);
  n_ops = n; qlen = q; rlen = r;
  if (lerr && !err) err = lerr;
}

// UCSC binning scheme (SAM spec 5.3, hts_reg2bin(beg, end, 14, 5))
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

__device__ __forceinline__ void line_span(const SamArgs &A, int64_t i, uint64_t &ls, uint64_t &le) {
  ls = i ? A.lend[i - 1] + 1 : 0;
  le = A.lend[i];
  if (le > ls && A.text[le - 1] == '\r') le--;   // CRLF: the '\r' is not part of the last field
}

__global__ void __launch_bounds__(64) k_sam_measure(SamArgs A) {
  __shared__ uint32_t pos[1024];
  __shared__ uint32_t fs[12];
  const int lane = threadIdx.x;
  const uint8_t *t = A.text;
  for (int64_t i = blockIdx.x; i < A.n_lines; i += gridDim.x) {
    uint64_t ls, le;
    line_span(A, i, ls, le);
    const uint32_t len = (uint32_t)(le - ls);
    uint32_t err = len == 0 ? (uint32_t)SAM_E_EMPTY : 0u;   // an empty line among the records is an error
    // every tab of the line: the first 11 fields, then one tag between two tabs (a lane per tag)
    uint32_t nt = 0, last = 0, lerr = 0;
    uint64_t aux = 0;
    if (lane == 0) fs[0] = 0;
    for (uint64_t wb = ls & ~15ull; wb < le; wb += 1024) {
      const uint32_t T = wfind<0>(t, wb, ls, le, ls, pos);
      for (uint32_t k = lane; k < T; k += 64) {
        const uint32_t g = nt + k, p = pos[k];
        if (g < 11) fs[g + 1] = p + 1;
        else aux += tag_bytes(A, ls + (k ? pos[k - 1] : last) + 1, ls + p, nullptr, (uint32_t)i, lerr);
      }
      if (T) last = pos[T - 1];
      nt += T;
    }
    if (nt >= 11 && lane == 0) aux += tag_bytes(A, ls + last + 1, le, nullptr, (uint32_t)i, lerr);   // the last tag ends the line
    if (nt == 10 && lane == 0) fs[11] = len + 1;
    aux = wave_sum(aux); lerr = wave_max(lerr);
    __syncthreads();
    if (!err && nt < 10) err = SAM_E_FIELDS;   // fewer than 11 fields
    if (!err && lerr) err = lerr;
    uint32_t f[12];
    for (int k = 0; k < 12; k++) f[k] = fs[k];
    auto flen = [&](int k) { return f[k + 1] - 1 - f[k]; };
    auto star = [&](int k) { return flen(k) == 1 && t[ls + f[k]] == '*'; };
    // CIGAR: '*' = no ops
    uint32_t n_cig = 0; uint64_t qlen = 0, rlen = 0;
    if (!err && !star(5)) {
      if (flen(5) == 0) err = SAM_E_CIGAR;
      else cigar_walk(A, ls, f[5], f[5] + flen(5), pos, nullptr, n_cig, qlen, rlen, err);
    }
    if (lane == 0 && err) {   // (the field offsets of a line with fewer than 11 fields are not to be read)
      SamLine L{};
      L.err = (uint8_t)err;
      A.line[i] = L; A.mapped[i] = 0; A.bytes[i] = 0;
      atomicMin(A.first_bad, (unsigned long long)i << 8 | err);
    } else if (lane == 0) {
      SamLine L{};
      for (int k = 0; k < 12; k++) L.f[k] = f[k];
      L.len = len;
      int64_t flag = 0, pos1 = 0, mapq = 0, pnext = 0, tlen = 0;
      // l_read_name = strlen(QNAME) + 1, at most 255 (no extra NULs: bam_write1 drops htslib's l_extranul)
      if (!err && (flen(0) < 1 || flen(0) > 254)) err = SAM_E_QNAME;
      // FLAG, MAPQ, POS, PNEXT, TLEN are decimal; the record stores POS - 1 and PNEXT - 1
      if (!err && !parse_int(t + ls + f[1], flen(1), 0, 65535, flag)) err = SAM_E_FLAG;
      if (!err && !parse_int(t + ls + f[3], flen(3), 0, 2147483647ll, pos1)) err = SAM_E_POS;
      if (!err && !parse_int(t + ls + f[4], flen(4), 0, 255, mapq)) err = SAM_E_MAPQ;
      if (!err && !parse_int(t + ls + f[7], flen(7), 0, 2147483647ll, pnext)) err = SAM_E_PNEXT;
      if (!err && !parse_int(t + ls + f[8], flen(8), -2147483647ll - 1, 2147483647ll, tlen)) err = SAM_E_TLEN;
      // RNAME: '*' -> -1; a name without an @SQ line -> -1 (htslib: "unrecognized reference name; treated as unmapped")
      // RNEXT: '=' -> the record's refID, '*' -> -1, an unknown name -> -1
      int32_t ref = -1, nref = -1;
      if (!err) {
        if (!star(2)) ref = ref_lookup(A, t + ls + f[2], flen(2));
        if (flen(6) == 1 && t[ls + f[6]] == '=') nref = ref;
        else if (!star(6)) nref = ref_lookup(A, t + ls + f[6], flen(6));
      }
      // SEQ '*' -> l_seq 0; QUAL '*' -> 0xFF x l_seq.  SEQ must match the CIGAR's query length, QUAL the SEQ's length.
      const uint32_t l_seq = star(9) ? 0u : flen(9);
      if (!err && n_cig && !star(9) && qlen != l_seq) err = SAM_E_SEQ_CIGAR;
      if (!err && !star(10) && flen(10) != l_seq) err = SAM_E_QUAL_SEQ;
      // refID -1 sets flag 0x4 (htslib: BAM_FUNMAP when tid < 0), and so does a mapped record without a query-consuming op
      // (CIGAR '*' included); such records are unmapped: skipped and counted, like br_bam_split
      if (ref < 0 || qlen == 0) flag |= 4;
      L.ref = ref; L.nref = nref; L.pos = (int32_t)(pos1 - 1); L.npos = (int32_t)(pnext - 1); L.tlen = (int32_t)tlen;
      L.flag = (uint16_t)flag; L.mapq = (uint8_t)mapq; L.n_cig = n_cig; L.rlen = (uint32_t)min<uint64_t>(rlen, 0xffffffffu);
      L.l_seq = l_seq; L.aux = (uint32_t)min<uint64_t>(aux, 0xffffffffu);
      // more than 65535 ops: bam_write1's on-disk form -- <l_seq>S<rlen>N in the CIGAR field, the real ops in a CG:B,I tag
      // behind the other tags
      const uint64_t ncf = n_cig > 65535 ? 2 : n_cig, cg = n_cig > 65535 ? 8ull + 4ull * n_cig : 0;
      const uint64_t bs = 32ull + (flen(0) + 1) + 4 * ncf + (l_seq + 1ull) / 2 + l_seq + aux + cg;
      if (!err && (bs > (1ull << 30) || rlen >= (1ull << 31))) err = SAM_E_TOO_LONG;
      // bin = reg2bin(pos, pos + rlen), rlen 0 -> 1 (the output keeps the input's bin)
      L.bin = (uint16_t)reg2bin(pos1 - 1, pos1 - 1 + (int64_t)(rlen ? rlen : 1));
      L.bsize = (uint32_t)bs;
      L.err = (uint8_t)err;
      L.mapped = !err && !(flag & 4);
      A.line[i] = L;
      A.mapped[i] = L.mapped;
      A.bytes[i] = L.mapped ? 4ull + bs : 0ull;
      if (err) atomicMin(A.first_bad, (unsigned long long)i << 8 | err);
    }
  }
}

// seq_nt16_table (htslib): '=' 0, A 1, C 2, M 3, G 4, R 5, S 6, V 7, T 8, W 9, Y 10, H 11, K 12, D 13, B 14, N 15 in either case;
// htslib's table also maps U to 8 and the digits 0-3 to 1, 2, 4, 8; every other byte -> 15
__constant__ uint8_t c_nt16[128] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 1,  2,  4,  8,  15, 15, 15, 15, 15, 15, 15, 15, 15, 0,  15, 15,
    15, 1,  14, 2,  13, 15, 15, 4,  11, 15, 15, 12, 15, 3,  15, 15, 15, 15, 5,  6,  8,  8,  7,  9,  15, 10, 15, 15, 15, 15, 15, 15,
    15, 1,  14, 2,  13, 15, 15, 4,  11, 15, 15, 12, 15, 3,  15, 15, 15, 15, 5,  6,  8,  8,  7,  9,  15, 10, 15, 15, 15, 15, 15, 15};

__global__ void __launch_bounds__(64) k_sam_emit(SamArgs A) {
  __shared__ uint32_t pos[1024];
  __shared__ uint8_t nt16[256];
  const int lane = threadIdx.x;
  for (int k = lane; k < 256; k += 64) nt16[k] = k < 128 ? c_nt16[k] : 15;
  __syncthreads();
  const uint8_t *t = A.text;
  for (int64_t i = blockIdx.x; i < A.n_lines; i += gridDim.x) {
    const SamLine L = A.line[i];
    if (!L.mapped) continue;
    const uint64_t ls = i ? A.lend[i - 1] + 1 : 0;
    const uint64_t off = A.bytes[i], idx = A.mapped[i];
    uint8_t *o = A.blob + off;
    const uint32_t lqn = L.f[1] - L.f[0], ncf = L.n_cig > 65535 ? 2u : L.n_cig;
    const uint32_t l_seq = L.l_seq;
    uint8_t *cig = o + 36 + lqn, *seq = cig + 4ull * ncf, *qual = seq + (l_seq + 1ull) / 2, *aux = qual + l_seq, *cg = aux + L.aux;
    if (lane == 0) {
      put32(o, L.bsize); put32(o + 4, (uint32_t)L.ref); put32(o + 8, (uint32_t)L.pos);
      o[12] = (uint8_t)lqn; o[13] = L.mapq; put16(o + 14, L.bin); put16(o + 16, ncf); put16(o + 18, L.flag);
      put32(o + 20, l_seq); put32(o + 24, (uint32_t)L.nref); put32(o + 28, (uint32_t)L.npos); put32(o + 32, (uint32_t)L.tlen);
      A.rec_off[idx] = off + 4; A.rec_len[idx] = L.bsize; A.rec_line[idx] = (uint32_t)i;
      o[36 + lqn - 1] = 0;
      if (L.n_cig > 65535) {
        put32(cig, l_seq << 4 | 4u); put32(cig + 4, L.rlen << 4 | 3u);
        cg[0] = 'C'; cg[1] = 'G'; cg[2] = 'B'; cg[3] = 'I'; put32(cg + 4, L.n_cig);
      }
    }
    for (uint32_t k = lane; k + 1 < lqn; k += 64) o[36 + k] = t[ls + k];
    if (L.n_cig) {
      uint32_t n_ops, cerr = 0; uint64_t q, r;
      cigar_walk(A, ls, L.f[5], L.f[6] - 1, pos, L.n_cig > 65535 ? cg + 8 : cig, n_ops, q, r, cerr);
    }
    // SEQ: two bases a byte (high nibble first), 32 bases -> 16 bytes a lane with vector loads and stores
    const bool seq_star = L.f[10] - 1 - L.f[9] == 1 && t[ls + L.f[9]] == '*';
    if (l_seq && !seq_star) {
      const uint8_t *s = t + ls + L.f[9];
      const uint32_t nb = (l_seq + 1) / 2;
      for (uint32_t b0 = (uint32_t)lane * 16; b0 < nb; b0 += 1024) {
        if (b0 + 16 <= nb && 2 * b0 + 32 <= l_seq) {
          const u32x4 x0 = *(const u32x4u *)(s + 2 * b0), x1 = *(const u32x4u *)(s + 2 * b0 + 16);
          const uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
          u32x4 y;
          uint32_t yw[4];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int h = 0; h < 4; h++) {
              const uint32_t src = w[(q * 8 + 2 * h) >> 2];
              const uint32_t sh = 8 * ((2 * h) & 3);
              const uint8_t a = (uint8_t)(src >> sh), b = (uint8_t)(src >> (sh + 8));
              v |= (uint32_t)(nt16[a] << 4 | nt16[b]) << (8 * h);
            }
            yw[q] = v;
          }
          y.x = yw[0]; y.y = yw[1]; y.z = yw[2]; y.w = yw[3];
          *(u32x4u *)(seq + b0) = y;
        } else {
          for (uint32_t k = b0; k < b0 + 16 && k < nb; k++) {
            const uint8_t hi = nt16[s[2 * k]], lo = 2 * k + 1 < l_seq ? nt16[s[2 * k + 1]] : 0;
            seq[k] = (uint8_t)(hi << 4 | lo);
          }
        }
      }
    }
    // QUAL: each character - 33; '*' -> 0xFF for every base
    const bool qual_star = L.f[11] - 1 - L.f[10] == 1 && t[ls + L.f[10]] == '*';
    if (l_seq) {
      const uint8_t *s = t + ls + L.f[10];
      for (uint32_t b0 = (uint32_t)lane * 16; b0 < l_seq; b0 += 1024) {
        if (b0 + 16 <= l_seq) {
          u32x4 y;
          if (qual_star) y = u32x4{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
          else {
            const u32x4 x = *(const u32x4u *)(s + b0);
            // bytewise - 33 without borrows between the bytes
            y.x = ((x.x | 0x80808080u) - 0x21212121u) ^ ((x.x ^ 0x80808080u) & 0x80808080u);
            y.y = ((x.y | 0x80808080u) - 0x21212121u) ^ ((x.y ^ 0x80808080u) & 0x80808080u);
            y.z = ((x.z | 0x80808080u) - 0x21212121u) ^ ((x.z ^ 0x80808080u) & 0x80808080u);
            y.w = ((x.w | 0x80808080u) - 0x21212121u) ^ ((x.w ^ 0x80808080u) & 0x80808080u);
          }
          *(u32x4u *)(qual + b0) = y;
        } else {
          for (uint32_t k = b0; k < l_seq; k++) qual[k] = qual_star ? (uint8_t)0xff : (uint8_t)(s[k] - 33);
        }
      }
    }
    // tags, in line order: a lane per tag, placed by a scan of their sizes; long Z / H values copied by the wave
    auto wave_copy = [&](bool mine, uint64_t src, uint8_t *dst, uint32_t n) {
      uint64_t m = __ballot(mine);
      while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const uint64_t sj = __shfl(src, j);
        uint8_t *dj = (uint8_t *)__shfl((uint64_t)dst, j);
        const uint32_t nj = __shfl(n, j);
        for (uint32_t q = lane; q < nj; q += 64) dj[q] = t[sj + q];
      }
    };
    if (L.f[11] <= L.len) {
      uint32_t last = L.f[11] - 1, terr = 0;
      uint64_t ao = 0;
      const uint64_t le = ls + L.len;
      for (uint64_t wb = (ls + L.f[11]) & ~15ull; wb < le; wb += 1024) {
        const uint32_t T = wfind<0>(t, wb, ls + L.f[11], le, ls, pos);
        for (uint32_t k0 = 0; k0 < T; k0 += 64) {
          const uint32_t k = k0 + lane;
          uint64_t s = 0, e = 0, sz = 0;
          if (k < T) { s = ls + (k ? pos[k - 1] : last) + 1; e = ls + pos[k]; sz = tag_bytes(A, s, e, nullptr, (uint32_t)i, terr); }
          const uint64_t incl = wave_scan(sz);
          if (k < T) (void)tag_bytes(A, s, e, aux + ao + incl - sz, (uint32_t)i, terr, SAM_ZMAX);
          const bool zl = k < T && (t[s + 3] == 'Z' || t[s + 3] == 'H') && e - s - 5 > SAM_ZMAX;
          wave_copy(zl, s + 5, aux + ao + incl - sz + 3, (uint32_t)(e - s - 5));
          ao += __shfl(incl, 63);
        }
        if (T) last = pos[T - 1];
      }
      const uint64_t s = ls + last + 1;
      if (lane == 0) (void)tag_bytes(A, s, le, aux + ao, (uint32_t)i, terr, SAM_ZMAX);
      wave_copy(lane == 0 && (t[s + 3] == 'Z' || t[s + 3] == 'H') && le - s - 5 > SAM_ZMAX, s + 5, aux + ao + 3, (uint32_t)(le - s - 5));
    }
  }
}

void launch_sam_nl_count(hipStream_t st, const uint8_t *text, uint64_t n, uint64_t *tile_cnt) {
  const uint64_t tiles = (n + SAM_NL_TILE - 1) / SAM_NL_TILE;
  if (tiles) hipLaunchKernelGGL(k_sam_nl_count, dim3((unsigned)tiles), dim3(256), 0, st, text, n, tile_cnt);
}
void launch_sam_nl_write(hipStream_t st, const uint8_t *text, uint64_t n, const uint64_t *tile_pre, uint64_t *lend) {
  const uint64_t tiles = (n + SAM_NL_TILE - 1) / SAM_NL_TILE;
  if (tiles) hipLaunchKernelGGL(k_sam_nl_write, dim3((unsigned)tiles), dim3(256), 0, st, text, n, tile_pre, lend);
}
static unsigned line_grid(int64_t n) { return (unsigned)(n < (1 << 20) ? (n > 0 ? n : 1) : (1 << 20)); }
void launch_sam_measure(hipStream_t st, const SamArgs &A) {
  if (A.n_lines) hipLaunchKernelGGL(k_sam_measure, dim3(line_grid(A.n_lines)), dim3(64), 0, st, A);
}
void launch_sam_emit(hipStream_t st, const SamArgs &A) {
  if (A.n_lines) hipLaunchKernelGGL(k_sam_emit, dim3(line_grid(A.n_lines)), dim3(64), 0, st, A);
}

}  // namespace br
