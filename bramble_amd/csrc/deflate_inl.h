// What the DEFLATE encoders share (device code only; include after hip_runtime.h and wave_inl.h): the fixed code's bit patterns, the
// LSB-first bit writer and the greedy LZ77 parse.  codec_kernels.hip (BGZF blocks of the record stream) and bigwig_kernels.hip (the
// zlib streams of a bigWig's sections) are built on it; the parse sees at most 65 535 bytes at a time (a table entry is 16 bits).
#pragma once
#include <stdint.h>

namespace br {

typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint64_t u64u __attribute__((aligned(1)));
typedef uint16_t u16u __attribute__((aligned(1)));

#ifndef HASH_BITS
#define HASH_BITS 11   // 4 KiB of LDS per wave: occupancy (7 workgroups per CU) matters more than the last 0.3 % of ratio
#endif
#define HASH_SIZE (1 << HASH_BITS)
#define EMPTY16 0xffffu
#define OBUF_WORDS 132  // one round emits <= 31 carried bits + 64 * (31 + 31) bits

__device__ __forceinline__ uint32_t bitrev(uint32_t v, int nbits) { return __builtin_bitreverse32(v) >> (32 - nbits); }

// length 3..258 -> fixed-Huffman bits (code reversed, then the extra bits): returns bit count, value in v
__device__ __forceinline__ int len_bits(uint32_t len, uint32_t &v) {
  uint32_t sym, eb = 0, ev = 0;
  uint32_t m = len - 3u;
  if (len == 258u) sym = 285u;
  else if (m < 8u) sym = 257u + m;
  else { eb = (31u - (uint32_t)__builtin_clz(m)) - 2u; sym = 261u + 4u * eb + ((m >> eb) - 4u); ev = m & ((1u << eb) - 1u); }
  int nb;
  uint32_t code;
  if (sym < 280u) { code = bitrev(sym - 256u, 7); nb = 7; } else { code = bitrev(0xC0u + (sym - 280u), 8); nb = 8; }
  v = code | (ev << nb);
  return nb + (int)eb;
}
// distance 1..32768 -> 5-bit code (reversed) + extra bits
__device__ __forceinline__ int dist_bits(uint32_t dist, uint32_t &v) {
  uint32_t m = dist - 1u, dc, eb = 0, ev = 0;
  if (m < 4u) dc = m;
  else { eb = (31u - (uint32_t)__builtin_clz(m)) - 1u; dc = 2u * (eb + 1u) + ((m >> eb) & 1u); ev = m & ((1u << eb) - 1u); }
  v = bitrev(dc, 5) | (ev << 5);
  return 5 + (int)eb;
}

// ---- shared pieces ----------------------------------------------------------------------------------
// LSB-first bit stream of one BGZF payload, assembled 64 tokens at a time in an LDS buffer with atomic ORs
struct BitWriter {
  uint32_t *obuf;   // LDS, all zero between rounds
  uint8_t *pay;     // payload start in the slot
  uint32_t carry, cbits, wbase;

  // every lane contributes up to two pieces (<= 31 bits each), A before B, lane order
  __device__ __forceinline__ void round(int lane, uint32_t va, uint32_t na, uint32_t vb, uint32_t nb) {
    const uint32_t nbits = na + nb, inc = wave_scan(nbits);
    uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63) + cbits;
    uint32_t pos = cbits + inc - nbits;
    if (lane == 0) obuf[0] = carry;
    __builtin_amdgcn_wave_barrier();
    if (na) {
      uint64_t lo = (uint64_t)va << (pos & 31u);
      atomicOr(&obuf[pos >> 5], (uint32_t)lo);
      if ((uint32_t)(lo >> 32)) atomicOr(&obuf[(pos >> 5) + 1], (uint32_t)(lo >> 32));
    }
    if (nb) {
      uint32_t p2 = pos + na;
      uint64_t lo = (uint64_t)vb << (p2 & 31u);
      atomicOr(&obuf[p2 >> 5], (uint32_t)lo);
      if ((uint32_t)(lo >> 32)) atomicOr(&obuf[(p2 >> 5) + 1], (uint32_t)(lo >> 32));
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t full = total >> 5;                       // <= (31 + 64 * 62) / 32 = 124
    for (uint32_t i = lane; i < full; i += 64) *(u32u *)(pay + 4u * (wbase + i)) = obuf[i];
    uint32_t nxt = obuf[full];
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i <= full + 1u && i < OBUF_WORDS; i += 64) obuf[i] = 0;
    __builtin_amdgcn_wave_barrier();
    cbits = total & 31u;
    carry = cbits ? (nxt & ((1u << cbits) - 1u)) : 0u;
    wbase += full;
  }
  // flush the remaining bits (plus `extra_zero_bits` zero bits) and return the payload byte count
  __device__ __forceinline__ uint32_t finish(int lane) {
    uint32_t nbytes = 4u * wbase + (cbits + 7u) / 8u;
    if (lane < 4) { if (4u * wbase + (uint32_t)lane < nbytes) pay[4u * wbase + lane] = (uint8_t)(carry >> (8 * lane)); }
    return nbytes;
  }
};

// Greedy parse, 128 positions per step (two half-rounds of 64, one position per lane each).  The table look-ups and the
// four-byte candidate checks of both halves are issued together -- the step is bound by dependent memory latency, and
// this halves the number of latency chains per byte.  The second half does not see the first half's table entries
// (distances below 128 are rare in a record stream and cost little).  Token kinds: 0 none, 1 literal, 2 match.
struct Token { uint32_t kind, byte, len, dist; };

// the greedy walk over one half-round: which of the 64 positions start a token, given each lane's checked candidate
__device__ __forceinline__ Token parse_half(const uint8_t *in, uint32_t n, uint32_t p, int lane, uint32_t w, uint32_t cand,
                                            uint32_t dist, bool v4, uint32_t &skip_until) {
  Token tk{0, 0, 0, 0};
  const uint32_t q = p + lane;
  const bool act = q < n;
  const bool can = q + 4u <= n;
  if (p + 64u <= skip_until) return tk;              // the whole half lies inside a match
  const uint64_t active = __ballot(act);
  const uint64_t covered = __ballot(act && q < skip_until);
  const uint64_t hasm = __ballot(v4 && q >= skip_until);
  // only the matches that are TAKEN get their length computed, by the whole wave: lane L compares bytes
  // [4 + 4L, 8 + 4L), one step covers all 258
  uint32_t mlen = 0;
  uint64_t lit = 0, mat = 0, undec = active & ~covered;
  while (undec) {
    uint64_t mm = hasm & undec;
    if (!mm) { lit |= undec; break; }
    int f = __builtin_ctzll(mm);
    uint64_t below = (1ull << f) - 1ull;
    lit |= undec & below;
    mat |= 1ull << f;
    const uint32_t qf = p + (uint32_t)f;
    const uint32_t cf = (uint32_t)__builtin_amdgcn_readlane((int)cand, f);
    uint32_t lim = n - qf; if (lim > 258u) lim = 258u;
    const uint32_t off = 4u + 4u * (uint32_t)lane;
    uint32_t x = 0;
    if (off < lim) {
      if (qf + off + 4u <= n) {
        x = *(const u32u *)(in + cf + off) ^ *(const u32u *)(in + qf + off);
        if (off + 4u > lim) x &= (1u << (8u * (lim - off))) - 1u;
      } else {
        for (uint32_t b2 = 0; b2 < 4u && off + b2 < lim; b2++) x |= (uint32_t)(in[cf + off + b2] ^ in[qf + off + b2]) << (8u * b2);
      }
    }
    uint64_t mis = __ballot(x != 0);
    uint32_t L = lim;
    if (mis) {
      int fl = __builtin_ctzll(mis);
      uint32_t xf = (uint32_t)__builtin_amdgcn_readlane((int)x, fl);
      L = 4u + 4u * (uint32_t)fl + ((uint32_t)__builtin_ctz(xf) >> 3);
    }
    if (lane == f) mlen = L;
    uint32_t end = (uint32_t)f + L;
    uint64_t cov = end >= 64u ? (~0ull << f) : (((1ull << end) - 1ull) & ~below);
    undec &= ~(below | cov);
    if (p + end > skip_until) skip_until = p + end;
  }
  if ((lit >> lane) & 1ull) { tk.kind = 1; tk.byte = can ? (w & 0xffu) : (uint32_t)in[q]; }
  else if ((mat >> lane) & 1ull) { tk.kind = 2; tk.len = mlen; tk.dist = dist; }
  return tk;
}

__device__ __forceinline__ void parse_step(const uint8_t *in, uint32_t n, uint32_t p, int lane, uint16_t *tab, uint32_t w0, uint32_t w1,
                                           uint32_t &skip_until, Token &ta, Token &tb) {
  const uint32_t q0 = p + lane, q1 = p + 64u + lane;
  const bool can0 = q0 + 4u <= n, can1 = q1 + 4u <= n;
  const uint32_t h0 = (w0 * 2654435761u) >> (32 - HASH_BITS), h1 = (w1 * 2654435761u) >> (32 - HASH_BITS);
  ta = Token{0, 0, 0, 0}; tb = Token{0, 0, 0, 0};
  if (p + 128u <= skip_until) {                      // everything lies inside a match: only feed the table
    if (can0) tab[h0] = (uint16_t)q0;
    __builtin_amdgcn_wave_barrier();
    if (can1) tab[h1] = (uint16_t)q1;
    return;
  }
  uint32_t c0 = can0 ? tab[h0] : EMPTY16, c1 = can1 ? tab[h1] : EMPTY16;
  __builtin_amdgcn_wave_barrier();
  if (can0) tab[h0] = (uint16_t)q0;                  // any writer of a clashing slot is fine: all are < the next step's p
  __builtin_amdgcn_wave_barrier();
  if (can1) tab[h1] = (uint16_t)q1;                  // the later half wins a clash within the lane
  uint32_t d0 = q0 - c0, d1 = q1 - c1;
  bool try0 = can0 && q0 >= skip_until && c0 != EMPTY16 && d0 <= 32768u;
  bool try1 = can1 && q1 >= skip_until && c1 != EMPTY16 && d1 <= 32768u;
  uint32_t f0 = try0 ? *(const u32u *)(in + c0) : 0u, f1 = try1 ? *(const u32u *)(in + c1) : 0u;   // both in flight together
  bool v0 = try0 && f0 == w0, v1 = try1 && f1 == w1;
  ta = parse_half(in, n, p, lane, w0, c0, d0, v0, skip_until);
  if (p + 64u < n) tb = parse_half(in, n, p + 64u, lane, w1, c1, d1, v1, skip_until);
}

}  // namespace br
