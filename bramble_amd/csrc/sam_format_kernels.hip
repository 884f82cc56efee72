// BAM records -> SAM text on the device: the writer-side counterpart of sam_kernels.hip.  Each record becomes the line
// htslib's bam_read1 + sam_format1 print for it (`samtools view`); the rules are repeated at the code that applies them.
//
//   k_samfmt_measure<16>  16 lanes per record of at most SF_LONG_REC bytes: the exact line length (longer records are listed)
//   k_samfmt_measure<64>  a whole wave per listed record
//   (launch_scan)         line lengths -> line offsets
//   k_samfmt_emit16       16 lanes per short record: the line is composed in LDS at the alignment of its destination and
//                         leaves with 16-byte streaming stores (a line longer than the slot is written in place)
//   k_samfmt_emit64       a whole wave per listed record, written in place
//
// Both passes run the same walk (sam_line<G, W>): the measure pass with W = false counts what the emit pass writes.  Every
// read is checked against the record's end; a record that cannot be formatted (a tag type outside AcCsSiIfZHB, a value or
// an array past the record's end, fixed fields past it) only sets first_bad, and the host stops before the emit pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_cg.h"
#include "sam_format.h"
#include "wave_inl.h"

namespace br {

constexpr int SF_SLOT = 1024;   // LDS bytes per 16-lane group of k_samfmt_emit16
typedef uint32_t sfw4 __attribute__((ext_vector_type(4)));

// ---- numbers ------------------------------------------------------------------------------------------
__device__ __forceinline__ int ndig(uint32_t v) {
  return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
         (v >= 100000000u) + (v >= 1000000000u);
}
// the decimal digits of v, n of them, at o
__device__ __forceinline__ void put_digits(uint8_t *o, uint32_t v, int n) {
  for (int k = n - 1; k >= 0; k--) { o[k] = (uint8_t)('0' + v % 10u); v /= 10u; }
}
// a signed number: its length, and its text at o when o is set
__device__ __forceinline__ int put_int(uint8_t *o, int64_t x) {
  const bool neg = x < 0;
  const uint32_t mag = (uint32_t)(neg ? -x : x);   // (every value here is within 32 bits of magnitude)
  const int n = ndig(mag);
  if (o) { if (neg) o[0] = '-'; put_digits(o + neg, mag, n); }
  return n + neg;
}

// ---- printf("%g", (double)f), exactly ---------------------------------------------------------------
// A finite float is m * 2^e (m < 2^24).  Its six significant digits D (10^5 <= D < 10^6) and decimal exponent X come from double
// arithmetic first; integer comparisons of 2 * m * 2^e against K * 10^(X - 5) then settle the floor and the rounding (ties to
// even, as glibc rounds).  Both sides fit 192 bits for every float (|X - 5| <= 51).
struct U3 { uint64_t a, b, c; };   // a: the low word
__device__ __forceinline__ void u3_mul(U3 &x, uint64_t s) {   // s < 2^32
  const uint64_t la = x.a * s, ha = __umul64hi(x.a, s);
  const uint64_t lb = x.b * s, hb = __umul64hi(x.b, s);
  const uint64_t lc = x.c * s;
  x.a = la;
  x.b = lb + ha; const uint64_t cb = x.b < lb;
  x.c = lc + hb + cb;
}
__device__ __forceinline__ void u3_shl(U3 &x, int s) {   // 0 <= s < 192
  if (s >= 128) { x.c = x.a; x.b = 0; x.a = 0; s -= 128; }
  else if (s >= 64) { x.c = x.b; x.b = x.a; x.a = 0; s -= 64; }
  if (s) { x.c = (x.c << s) | (x.b >> (64 - s)); x.b = (x.b << s) | (x.a >> (64 - s)); x.a <<= s; }
}
__device__ __forceinline__ void u3_pow5(U3 &x, int k) {
  for (; k >= 13; k -= 13) u3_mul(x, 1220703125ull);   // 5^13
  uint64_t p = 1;
  for (; k > 0; k--) p *= 5;
  u3_mul(x, p);
}
// sign of 2 * m * 2^e - K * 10^q
__device__ int cmp_dec(uint32_t m, int e, uint32_t K, int q) {
  U3 L{m, 0, 0}, R{K, 0, 0};
  if (q < 0) u3_pow5(L, -q); else u3_pow5(R, q);
  const int le = e + 1 - (q < 0 ? q : 0), re = q > 0 ? q : 0, s = le < re ? le : re;
  u3_shl(L, le - s); u3_shl(R, re - s);
  if (L.c != R.c) return L.c < R.c ? -1 : 1;
  if (L.b != R.b) return L.b < R.b ? -1 : 1;
  if (L.a != R.a) return L.a < R.a ? -1 : 1;
  return 0;
}

struct GNum {
  uint32_t d;      // the digits to print (trailing zeros gone, except those of the integer part of the fixed form)
  int nd;          // their count
  int x;           // decimal exponent
  uint8_t kind;    // 0: finite non-zero, 1: zero, 2: inf, 3: nan
  bool neg;
};
__device__ GNum g_decompose(uint32_t u) {
  GNum g{0, 1, 0, 0, (u >> 31) != 0};
  const uint32_t E = (u >> 23) & 0xffu, M = u & 0x7fffffu;
  if (E == 0xffu) { g.kind = M ? 3 : 2; return g; }
  if (E == 0 && M == 0) { g.kind = 1; return g; }
  const uint32_t m = E ? (M | 0x800000u) : M;
  const int e = E ? (int)E - 150 : -149;
  const double v = ldexp((double)m, e);
  int X = (int)floor(log10(v));
  uint32_t D = 0;
  for (int it = 0; it < 4; it++) {
    const int q = X - 5;
    double t = v / exp10((double)q);
    t = t < 99999.0 ? 99999.0 : t > 1000000.0 ? 1000000.0 : t;
    D = (uint32_t)t;
    for (int k = 0; k < 3 && D > 0 && cmp_dec(m, e, 2 * D, q) < 0; k++) D--;        // D * 10^q <= v ...
    for (int k = 0; k < 3 && cmp_dec(m, e, 2 * D + 2, q) >= 0; k++) D++;           // ... < (D + 1) * 10^q
    if (D < 100000u) { X--; continue; }
    if (D >= 1000000u) { X++; continue; }
    break;
  }
  const int c = cmp_dec(m, e, 2 * D + 1, X - 5);   // against the midpoint: up, or a tie to even
  if (c > 0 || (c == 0 && (D & 1u))) D++;
  if (D == 1000000u) { D = 100000u; X++; }
  // %g: the exponent form below 1e-4 and from 1e6 on; trailing zeros go (not those in front of the point)
  int nd = 6;
  while (nd > 1 && D % 10u == 0) { D /= 10u; nd--; }
  if (X >= 0 && X <= 5 && nd < X + 1) { for (int k = nd; k < X + 1; k++) D *= 10u; nd = X + 1; }
  g.d = D; g.nd = nd; g.x = X;
  return g;
}
// its text at o when o is set; the length
__device__ int g_put(const GNum &g, uint8_t *o) {
  int p = 0;
  if (g.neg) { if (o) o[0] = '-'; p = 1; }
  if (g.kind == 1) { if (o) o[p] = '0'; return p + 1; }
  if (g.kind >= 2) { if (o) { const char *s = g.kind == 2 ? "inf" : "nan"; o[p] = s[0]; o[p + 1] = s[1]; o[p + 2] = s[2]; } return p + 3; }
  const int X = g.x, nd = g.nd;
  if (X < -4 || X >= 6) {   // d[.ddddd]e+XX
    const int mant = nd > 1 ? nd + 1 : 1;
    const uint32_t ax = (uint32_t)(X < 0 ? -X : X);
    const int ne = ax >= 100 ? 3 : 2;
    if (o) {
      uint32_t v = g.d;
      for (int i = nd - 1; i >= 0; i--) { o[p + (i ? i + 1 : 0)] = (uint8_t)('0' + v % 10u); v /= 10u; }
      if (nd > 1) o[p + 1] = '.';
      o[p + mant] = 'e'; o[p + mant + 1] = X < 0 ? '-' : '+';
      put_digits(o + p + mant + 2, ax, ne);
    }
    return p + mant + 2 + ne;
  }
  if (X >= 0) {   // ddd[.ddd]
    const int frac = nd - (X + 1);
    if (o) {
      uint32_t v = g.d;
      for (int i = nd - 1; i >= 0; i--) { o[p + (i <= X ? i : i + 1)] = (uint8_t)('0' + v % 10u); v /= 10u; }
      if (frac > 0) o[p + X + 1] = '.';
    }
    return p + X + 1 + (frac > 0 ? frac + 1 : 0);
  }
  const int z = -X - 1;   // 0.000ddd
  if (o) {
    o[p] = '0'; o[p + 1] = '.';
    for (int k = 0; k < z; k++) o[p + 2 + k] = '0';
    put_digits(o + p + 2 + z, g.d, nd);
  }
  return p + 2 + z + nd;
}

// ---- lanes of a group ---------------------------------------------------------------------------------

// the first NUL in [p, e), as an offset from p, or -1: G lanes test 4 bytes each per step
template <int G>
__device__ int64_t find_nul(const uint8_t *p, const uint8_t *e, int lane) {
  for (const uint8_t *b = p; b < e; b += 4 * G) {
    const uint8_t *c = b + 4 * lane;
    uint32_t hit = 0xffffffffu;
    if (e - c >= 4) {
      const uint32_t w = ld_u32(c), z = (w - 0x01010101u) & ~w & 0x80808080u;
      if (z) hit = 4u * lane + (__builtin_ctz(z) >> 3);
    } else {
      for (int k = 0; c + k < e; k++) if (c[k] == 0) { hit = 4u * lane + k; break; }
    }
    hit = wave_min<uint32_t, G>(hit);
    if (hit != 0xffffffffu) return (b - p) + hit;
  }
  return -1;
}

__device__ __forceinline__ uint8_t nt16(uint32_t k) {   // "=ACMGRSVTWYHKDBN"[k]
  const uint64_t lo = 0x565352474d43413dull /* =ACMGRSV */, hi = 0x4e42444b48595754ull /* TWYHKDBN */;
  return (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xffu);
}
__device__ __forceinline__ uint8_t cigar_chr(uint32_t op) {   // "MIDNSHP=XB"[min(op, 9)]
  return op < 8 ? (uint8_t)((0x3d5048534e44494dull /* MIDNSHP= */ >> (8 * op)) & 0xffu) : op == 8 ? 'X' : 'B';
}
__device__ __forceinline__ int isize(uint8_t t) {
  return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I') ? 4 : 0;
}
__device__ __forceinline__ int64_t ival(uint8_t t, const uint8_t *v) {
  switch (t) {
    case 'c': return (int8_t)v[0];
    case 'C': return v[0];
    case 's': return (int16_t)ld_u16(v);
    case 'S': return ld_u16(v);
    case 'i': return (int32_t)ld_u32(v);
    default: return ld_u32(v);
  }
}

// One record -> its line (with the '\n'); the length, or -1 when it cannot be formatted.  Every lane of the group runs it with
// the same record and gets the same result; with W the lanes write the line at o.
template <int G, bool W>
__device__ int64_t sam_line(const SamFmtArgs &A, const uint8_t *r, uint32_t rlen, uint8_t *o, int lane) {
  if (rlen < 32) return -1;
  const int32_t rid = (int32_t)ld_u32(r), pos = (int32_t)ld_u32(r + 4), l_seq = (int32_t)ld_u32(r + 16);
  const int32_t nrid = (int32_t)ld_u32(r + 20), npos = (int32_t)ld_u32(r + 24), tlen = (int32_t)ld_u32(r + 28);
  const uint32_t lqn = r[8], mapq = r[9], ncig = ld_u16(r + 12), flag = ld_u16(r + 14);
  if (lqn == 0 || l_seq < 0) return -1;   // (bam_read1 refuses both)
  const uint64_t ls = (uint64_t)l_seq, aux0 = 32ull + lqn + 4ull * ncig + (ls + 1) / 2 + ls;
  if (aux0 > rlen) return -1;
  // the CIGAR: the field's ops, or those of the CG tag of a record in the spilled form (bam_tag2cigar), whose tag then goes
  const uint8_t *cig = r + 32 + lqn;
  uint32_t nops = ncig, cg_at = 0xffffffffu, cg_len = 0;
  CgTag cg;
  if (cg_find(r, rlen, lqn, ncig, l_seq, cg)) { cig = r + cg.tag_at + 8; nops = cg.n; cg_at = cg.tag_at; cg_len = cg.tag_len; }
  const bool w0 = W && lane == 0;
  uint8_t *o0 = w0 ? o : nullptr;   // what lane 0 alone writes
  auto at = [&](int64_t p) { return o0 ? o0 + p : nullptr; };
  auto name = [&](int64_t p, int32_t id) -> int64_t {   // RNAME / RNEXT: the name, '*' past the list
    if (id < 0 || id >= A.n_names) { if (w0) o[p] = '*'; return 1; }
    const uint64_t a = A.name_off[id], n = A.name_off[id + 1] - a;
    if (W) for (uint64_t k = lane; k < n; k += G) o[p + k] = A.names[a + k];
    return (int64_t)n;
  };
  auto tab = [&](int64_t p) { if (w0) o[p] = '\t'; return (int64_t)1; };
  int64_t p = 0;
  // QNAME FLAG RNAME POS MAPQ
  const uint32_t lq = lqn - 1;
  if (W) for (uint32_t k = lane; k < lq; k += G) o[k] = r[32 + k];
  p = lq;
  p += tab(p); p += put_int(at(p), flag);
  p += tab(p); p += name(p, rid);
  p += tab(p); p += put_int(at(p), (int64_t)pos + 1);
  p += tab(p); p += put_int(at(p), mapq);
  p += tab(p);
  // CIGAR: one lane per op, placed by a prefix sum of the op lengths
  if (nops == 0) { if (w0) o[p] = '*'; p += 1; }
  for (uint32_t b = 0; b < nops; b += G) {
    const uint32_t k = b + lane;
    uint32_t w = 0, len = 0;
    if (k < nops) { w = ld_u32(cig + 4ull * k); len = (uint32_t)ndig(w >> 4) + 1; }
    const uint32_t inc = wave_scan<uint32_t, G>(len);
    if (W && k < nops) {
      const int64_t q = p + inc - len;
      put_digits(o + q, w >> 4, (int)len - 1);
      o[q + len - 1] = cigar_chr(w & 15u);
    }
    p += __shfl(inc, G - 1, G);
  }
  // RNEXT PNEXT TLEN
  p += tab(p);
  if (nrid < 0 || nrid == rid) { if (w0) o[p] = nrid < 0 ? '*' : '='; p += 1; }
  else p += name(p, nrid);
  p += tab(p); p += put_int(at(p), (int64_t)npos + 1);
  p += tab(p); p += put_int(at(p), tlen);
  p += tab(p);
  // SEQ: one lane per byte pair
  const uint8_t *s = r + 32 + lqn + 4ull * ncig;
  if (ls == 0) { if (w0) o[p] = '*'; p += 1; }
  else {
    if (W)
      for (uint64_t k = lane; k < (ls + 1) / 2; k += G) {
        const uint32_t v = s[k];
        o[p + 2 * k] = nt16(v >> 4);
        if (2 * k + 1 < ls) o[p + 2 * k + 1] = nt16(v & 15u);
      }
    p += (int64_t)ls;
  }
  p += tab(p);
  // QUAL: four bytes per lane, + 33 in the register ('*' without a sequence, or when the first byte is 0xff)
  const uint8_t *qs = s + (ls + 1) / 2;
  if (ls == 0 || qs[0] == 0xff) { if (w0) o[p] = '*'; p += 1; }
  else {
    if (W)
      for (uint64_t k = 4ull * lane; k < ls; k += 4ull * G) {
        if (k + 4 <= ls) {
          const uint32_t v = ld_u32(qs + k), x = ((v & 0x7f7f7f7fu) + 0x21212121u) ^ (v & 0x80808080u);
          o[p + k] = (uint8_t)x; o[p + k + 1] = (uint8_t)(x >> 8); o[p + k + 2] = (uint8_t)(x >> 16); o[p + k + 3] = (uint8_t)(x >> 24);
        } else {
          for (uint64_t j = k; j < ls; j++) o[p + j] = (uint8_t)(qs[j] + 33);
        }
      }
    p += (int64_t)ls;
  }
  // tags, in their order: \tXY:T:value
  const uint8_t *q = r + aux0, *e = r + rlen;
  while (q < e) {
    if (e - q < 3) return -1;
    if ((uint32_t)(q - r) == cg_at) { q += cg_len; continue; }
    const uint8_t t = q[2];
    const int sz = isize(t);
    const uint8_t *v = q + 3;
    if (w0) { o[p] = '\t'; o[p + 1] = q[0]; o[p + 2] = q[1]; o[p + 3] = ':'; o[p + 4] = sz ? 'i' : t; o[p + 5] = ':'; }
    p += 6;
    if (t == 'A') {
      if (e - v < 1) return -1;
      if (w0) o[p] = v[0];
      p += 1; q = v + 1;
    } else if (sz) {   // c C s S i I all print as :i:
      if (e - v < sz) return -1;
      p += put_int(at(p), ival(t, v));
      q = v + sz;
    } else if (t == 'f') {
      if (e - v < 4) return -1;
      int len = 0;
      if (lane == 0) { const GNum g = g_decompose(ld_u32(v)); len = g_put(g, W ? o + p : nullptr); }
      p += __shfl(len, 0, G);
      q = v + 4;
    } else if (t == 'Z' || t == 'H') {
      const int64_t n = find_nul<G>(v, e, lane);
      if (n < 0) return -1;
      if (W) for (int64_t k = lane; k < n; k += G) o[p + k] = v[k];
      p += n; q = v + n + 1;
    } else if (t == 'B') {
      if (e - v < 5) return -1;
      const uint8_t sub = v[0];
      const uint32_t cnt = ld_u32(v + 1);
      const int esz = sub == 'f' ? 4 : isize(sub);
      if (!esz || (uint64_t)(e - v - 5) < (uint64_t)cnt * (uint64_t)esz) return -1;
      if (w0) o[p] = sub;
      p += 1;
      const uint8_t *a = v + 5;
      for (uint32_t b = 0; b < cnt; b += G) {   // one lane per element, placed by a prefix sum: ,value
        const uint32_t k = b + lane;
        uint32_t len = 0;
        GNum g{};
        int64_t x = 0;
        if (k < cnt) {
          if (sub == 'f') { g = g_decompose(ld_u32(a + 4ull * k)); len = 1 + (uint32_t)g_put(g, nullptr); }
          else { x = ival(sub, a + (uint64_t)esz * k); len = 1 + (uint32_t)put_int(nullptr, x); }
        }
        const uint32_t inc = wave_scan<uint32_t, G>(len);
        if (W && k < cnt) {
          uint8_t *d = o + p + inc - len;
          d[0] = ',';
          if (sub == 'f') (void)g_put(g, d + 1); else (void)put_int(d + 1, x);
        }
        p += __shfl(inc, G - 1, G);
      }
      q = a + (uint64_t)cnt * esz;
    } else {
      return -1;
    }
  }
  if (w0) o[p] = '\n';
  return p + 1;
}

// the record of row i: its bytes from refID on and its block_size, or false when they overrun the stream
__device__ __forceinline__ bool row_rec(const SamFmtArgs &A, int64_t i, const uint8_t *&r, uint32_t &rlen) {
  const uint64_t off = A.row_off[i];
  if (off > A.n_bytes || A.n_bytes - off < 4) return false;
  rlen = ld_u32(A.data + off);
  if (A.n_bytes - off - 4 < rlen) return false;
  r = A.data + off + 4;
  return true;
}

template <int G>
__device__ __forceinline__ void measure_one(const SamFmtArgs &A, int64_t i, const uint8_t *r, uint32_t rlen, bool ok, int lane) {
  const int64_t L = ok ? sam_line<G, false>(A, r, rlen, nullptr, lane) : -1;
  if (lane == 0) {
    A.len[i] = L < 0 ? 0 : (uint64_t)L;
    if (L < 0) atomicMin(A.first_bad, (unsigned long long)i);
  }
}

template <int G>
__global__ void __launch_bounds__(256) k_samfmt_measure(SamFmtArgs A) {
  const int lane = threadIdx.x % G;
  const int64_t per = 256 / G, g0 = (int64_t)blockIdx.x * per + threadIdx.x / G, stride = (int64_t)gridDim.x * per;
  if (G == 64) {
    const int64_t n = *A.n_long;
    for (int64_t j = g0; j < n; j += stride) {
      const int64_t i = A.long_list[j];
      const uint8_t *r = nullptr; uint32_t rlen = 0;
      const bool ok = row_rec(A, i, r, rlen);
      measure_one<G>(A, i, r, rlen, ok, lane);
    }
    return;
  }
  for (int64_t i = g0; i < A.n; i += stride) {
    const uint8_t *r = nullptr; uint32_t rlen = 0;
    const bool ok = row_rec(A, i, r, rlen);
    if (ok && rlen > SF_LONG_REC) { if (lane == 0) A.long_list[atomicAdd(A.n_long, 1u)] = (uint32_t)i; continue; }
    measure_one<G>(A, i, r, rlen, ok, lane);
  }
}

// 16 lanes per record: the line is composed in the group's LDS slot at the offset its destination has in a 16-byte word, then
// the whole words leave with 16-byte streaming stores and the two partial ones byte by byte (the neighbouring lines own the
// rest of them).  A line that does not fit the slot is written in place.
__global__ void __launch_bounds__(256) k_samfmt_emit16(SamFmtArgs A) {
  __shared__ __attribute__((aligned(16))) uint8_t slot[16][SF_SLOT];
  const int lane = threadIdx.x & 15, g = threadIdx.x >> 4;
  for (int64_t base = (int64_t)blockIdx.x * 16; base < A.n; base += (int64_t)gridDim.x * 16) {   // (the same trip count in every wave)
    const int64_t i = base + g;
    bool staged = false;
    uint64_t d = 0, L = 0;
    if (i < A.n) {
      const uint8_t *r = nullptr; uint32_t rlen = 0;
      if (row_rec(A, i, r, rlen) && rlen <= SF_LONG_REC) {
        d = A.len[i]; L = A.len[i + 1] - d;
        staged = (d & 15u) + L <= SF_SLOT;
        (void)sam_line<16, true>(A, r, rlen, staged ? slot[g] + (d & 15u) : A.text + d, lane);
      }
    }
    __syncthreads();
    if (staged) {
      const uint64_t w0 = d >> 4, w1 = (d + L + 15) >> 4;
      for (uint64_t w = w0 + lane; w < w1; w += 16) {
        const uint64_t lo = w * 16 > d ? w * 16 : d, hi = w * 16 + 16 < d + L ? w * 16 + 16 : d + L;
        const uint8_t *src = slot[g] + (w - w0) * 16;
        if (lo == w * 16 && hi == w * 16 + 16) __builtin_nontemporal_store(*(const sfw4 *)src, (sfw4 *)(A.text + w * 16));
        else for (uint64_t b = lo; b < hi; b++) A.text[b] = src[b - w * 16];
      }
    }
    __syncthreads();
  }
}

// a whole wave per record of the long list, written in place
__global__ void __launch_bounds__(256) k_samfmt_emit64(SamFmtArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t n = *A.n_long;
  for (int64_t j = (int64_t)blockIdx.x * 4 + threadIdx.x / 64; j < n; j += (int64_t)gridDim.x * 4) {
    const int64_t i = A.long_list[j];
    const uint8_t *r = nullptr; uint32_t rlen = 0;
    if (!row_rec(A, i, r, rlen)) continue;
    (void)sam_line<64, true>(A, r, rlen, A.text + A.len[i], lane);
  }
}

static unsigned grid_for(int64_t n, int per_block) {
  const int64_t b = (n + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b > (1 << 20) ? (1 << 20) : b);
}
void launch_sam_fmt_measure(hipStream_t st, const SamFmtArgs &A, int n_cu) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_samfmt_measure<16>, dim3(grid_for(A.n, 16)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_samfmt_measure<64>, dim3((unsigned)(n_cu > 0 ? n_cu : 256)), dim3(256), 0, st, A);
}
void launch_sam_fmt_emit(hipStream_t st, const SamFmtArgs &A, int n_cu) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_samfmt_emit16, dim3(grid_for(A.n, 16)), dim3(256), 0, st, A);
  hipLaunchKernelGGL(k_samfmt_emit64, dim3((unsigned)(n_cu > 0 ? n_cu : 256)), dim3(256), 0, st, A);
}

}  // namespace br
