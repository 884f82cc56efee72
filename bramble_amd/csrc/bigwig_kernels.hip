// The bigWig of a finished br_coverage on the device (bigwig_kernels.h; host side and the pipeline's description: bigwig.cpp).
//
//   k_bw_run_first     a lane per transcript: its first run, by bisection of the runs' transcript ids
//   k_bw_sections      a lane per section of the full data: its 24-byte header, where it begins, its bounds for the R-tree
//   k_bw_pack          a lane per run in (chromId, start) order: start, end, (float) value behind its section's header
//   k_bw_total         the total summary's partial sums over the runs, a fixed grid and a fixed order
//   k_bw_zoom_windows  G lanes per window of a zoom level: covered bases, least and greatest depth, the sums of the value and of its
//                      square in double from the depth array, each lane its bases G apart in order, then the xor butterfly: no
//                      floating-point atomics, the same bits every run
//   k_bw_zoom_compact  the records of the windows with a covered base, in order (after a scan of their flags)
//   k_bw_zoom_blocks   where the blocks of S zoom records begin, and their bounds
//   k_bw_zlib          one wave per payload: Adler-32 by 64 lane-chunks, then one final fixed-Huffman block from the greedy parse of
//                      the BGZF path (deflate_inl.h), or stored blocks where that is not smaller than the payload
//   k_bw_gather        slots -> one dense byte stream (after a scan of the stream sizes)
//   k_bw_tree_reduce / k_bw_tree_nodes   the bounds and the nodes of one R-tree level
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigwig_kernels.h"
#include "wave_inl.h"
#include "deflate_inl.h"

namespace br {

// the largest c in [0, n) with tab[c] <= v (tab ascends, tab[0] <= v)
__device__ __forceinline__ uint64_t last_at_most(const uint64_t *tab, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (tab[mid] <= v) lo = mid; else hi = mid; }
  return lo;
}

__device__ __forceinline__ double value_of(uint64_t d, bool wide) { return wide ? (double)d * (1.0 / 4294967296.0) : (double)d; }

__global__ void __launch_bounds__(256) k_bw_run_first(const uint4 *runs, uint64_t n_runs, int64_t n_tx, uint64_t *first) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t > n_tx) return;
  uint64_t lo = 0, hi = n_runs;   // the first run with transcript >= t
  while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if ((int64_t)runs[mid].x < t) lo = mid + 1; else hi = mid; }
  first[t] = lo;
}

__global__ void __launch_bounds__(256) k_bw_sections(BwPackArgs A) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sec) return;
  const uint64_t c = last_at_most(A.sec0, A.n_chrom, s);
  const uint64_t k0 = (s - A.sec0[c]) * A.S, nc = A.cum[c + 1] - A.cum[c];   // the section's first run among the chromosome's
  const uint64_t cnt = nc - k0 < A.S ? nc - k0 : A.S;
  const uint64_t r0 = A.run0[c] + k0;
  const uint32_t start = A.runs[r0].y, end = A.runs[r0 + cnt - 1].z;
  const uint64_t at = 24 * s + 12 * (A.cum[c] + k0);
  A.raw_off[s] = at;
  if (s + 1 == A.n_sec) A.raw_off[A.n_sec] = 24 * A.n_sec + 12 * A.n_runs;
  uint32_t *h = (uint32_t *)(A.raw + at);
  h[0] = (uint32_t)c; h[1] = start; h[2] = end; h[3] = 0; h[4] = 0; h[5] = 1u | ((uint32_t)cnt << 16);   // type 1: bedGraph
  A.lo[s] = (c << 32) | start; A.hi[s] = (c << 32) | end;
}

__global__ void __launch_bounds__(256) k_bw_pack(BwPackArgs A) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n_runs) return;
  const uint64_t c = last_at_most(A.cum, A.n_chrom, j);
  const uint64_t k = j - A.cum[c], r = A.run0[c] + k, sec = A.sec0[c] + k / A.S;
  const uint4 run = A.runs[r];
  const float v = A.run_depth ? (float)value_of(A.run_depth[r], true) : (float)run.w;
  uint32_t *item = (uint32_t *)(A.raw + 24 * (sec + 1) + 12 * j);
  item[0] = run.y; item[1] = run.z; item[2] = __float_as_uint(v);
}

__global__ void __launch_bounds__(256) k_bw_total(const uint4 *runs, const uint64_t *run_depth, uint64_t n_runs, uint64_t *partial) {
  __shared__ uint64_t sh_n[4], sh_mn[4], sh_mx[4];
  __shared__ double sh_s[4], sh_q[4];
  uint64_t n = 0, mn = ~0ull, mx = 0;
  double sum = 0, sq = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * 256) {
    const uint4 run = runs[r];
    const uint64_t d = run_depth ? run_depth[r] : (uint64_t)run.w;
    const double len = (double)(run.z - run.y), v = value_of(d, run_depth != nullptr);
    n += run.z - run.y; mn = d < mn ? d : mn; mx = d > mx ? d : mx;
    sum += v * len; sq += v * v * len;
  }
  n = wave_sum(n); mn = wave_min(mn); mx = wave_max(mx); sum = wave_sum(sum); sq = wave_sum(sq);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh_n[w] = n; sh_mn[w] = mn; sh_mx[w] = mx; sh_s[w] = sum; sh_q[w] = sq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; i++) { n += sh_n[i]; mn = sh_mn[i] < mn ? sh_mn[i] : mn; mx = sh_mx[i] > mx ? sh_mx[i] : mx; sum += sh_s[i]; sq += sh_q[i]; }
    uint64_t *p = partial + 5 * (uint64_t)blockIdx.x;
    p[0] = n; p[1] = mn; p[2] = mx; p[3] = (uint64_t)__double_as_longlong(sum); p[4] = (uint64_t)__double_as_longlong(sq);
  }
}

template <typename W>
__global__ void __launch_bounds__(256) k_bw_zoom_windows(BwZoomArgs A) {
  constexpr bool wide = sizeof(W) == 8;
  const int G = A.G, g = (int)(threadIdx.x & (unsigned)(G - 1));
  const uint64_t w = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / (unsigned)G;
  const bool on = w < A.n_win;
  uint64_t c = 0, start = 0, len = 0;
  const W *d = nullptr;
  if (on) {
    c = last_at_most(A.win0, A.n_chrom, w);
    const uint32_t t = A.tid[c];
    const uint64_t b = A.off[t], L = A.off[t + 1] - b;
    start = (w - A.win0[c]) * A.R;           // below L: the chromosome has ceil(L / R) windows
    len = L - start < A.R ? L - start : A.R;
    d = (const W *)A.depth + b + start;
  }
  uint64_t cnt = 0, mn = ~0ull, mx = 0;
  double sum = 0, sq = 0;
  for (uint64_t x = (uint64_t)g; x < len; x += (unsigned)G) {
    const uint64_t v = (uint64_t)d[x];
    if (v) {
      const double f = value_of(v, wide);
      cnt++; mn = v < mn ? v : mn; mx = v > mx ? v : mx; sum += f; sq += f * f;
    }
  }
  for (int m = G >> 1; m >= 1; m >>= 1) {    // (the whole wave: lanes of other windows stay among themselves)
    cnt += __shfl_xor(cnt, m); sum += __shfl_xor(sum, m); sq += __shfl_xor(sq, m);
    const uint64_t a = __shfl_xor(mn, m), b = __shfl_xor(mx, m);
    mn = a < mn ? a : mn; mx = b > mx ? b : mx;
  }
  if (!on || g) return;
  uint4 head, tail;
  head.x = (uint32_t)c; head.y = (uint32_t)start; head.z = (uint32_t)(start + len); head.w = (uint32_t)cnt;
  tail.x = cnt ? __float_as_uint((float)value_of(mn, wide)) : 0u; tail.y = __float_as_uint((float)value_of(mx, wide));
  tail.z = __float_as_uint((float)sum); tail.w = __float_as_uint((float)sq);
  A.rec[2 * w] = head; A.rec[2 * w + 1] = tail;
  A.flag[w] = cnt ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_bw_zoom_compact(const uint4 *rec, const uint64_t *pos, uint64_t n_win, uint4 *out) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_win || pos[w + 1] == pos[w]) return;
  out[2 * pos[w]] = rec[2 * w]; out[2 * pos[w] + 1] = rec[2 * w + 1];
}

__global__ void __launch_bounds__(256) k_bw_zoom_blocks(const uint4 *rec, uint64_t n_rec, uint32_t S, uint64_t n_blocks, uint64_t *off, uint64_t *lo,
                                                        uint64_t *hi) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b > n_blocks) return;
  const uint64_t first = b * S < n_rec ? b * S : n_rec;
  off[b] = 32 * first;
  if (b == n_blocks) return;
  const uint64_t last = (b + 1) * S < n_rec ? (b + 1) * S - 1 : n_rec - 1;
  const uint4 f = rec[2 * first], l = rec[2 * last];
  lo[b] = ((uint64_t)f.x << 32) | f.y; hi[b] = ((uint64_t)l.x << 32) | l.z;
}

// ---- zlib sections ---------------------------------------------------------------------------------------------------------------
// Adler-32 (RFC 1950) of in[0, n): lane l takes the bytes [l chunk, (l + 1) chunk) and leaves a_l = their sum and b_l = the sum of the
// running a over them (a <= 255 x 2048 and b <= 2048 a: both below 2^32, no reduction inside).  With t_l bytes behind the chunk,
// a = 1 + sum a_l and b = n + sum (b_l + a_l t_l), modulo 65521: the products in 64 bits, reduced per lane before the wave's sum
__device__ __forceinline__ uint32_t adler32_wave(const uint8_t *in, uint32_t n, int lane) {
  const uint32_t chunk = n <= 64u * BW_ADLER_CHUNK ? BW_ADLER_CHUNK : (((n + 63u) / 64u) + 3u) & ~3u;
  const uint32_t s = (uint32_t)lane * chunk;
  uint32_t a = 0, b = 0, e = s;
  if (s < n) {
    e = s + chunk < n ? s + chunk : n;
    uint32_t j = s;
    for (; j + 4u <= e; j += 4u) {
      const uint32_t d = *(const u32u *)(in + j);
      a += d & 0xffu; b += a; a += (d >> 8) & 0xffu; b += a; a += (d >> 16) & 0xffu; b += a; a += d >> 24; b += a;
    }
    for (; j < e; j++) { a += in[j]; b += a; }
  }
  const uint32_t part = s < n ? (uint32_t)(((uint64_t)a * (n - e) + b) % 65521u) : 0u;
  const uint32_t A = (1u + wave_sum(a)) % 65521u, B = (n % 65521u + wave_sum(part)) % 65521u;
  return (B << 16) | A;
}

__global__ void __launch_bounds__(256) k_bw_zlib(const uint8_t *src, const uint64_t *off, uint64_t n_streams, int mode, uint8_t *slots, uint64_t *sizes) {
  __shared__ uint16_t sh_tab[4][HASH_SIZE];
  __shared__ uint32_t sh_obuf[4][OBUF_WORDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t i = (uint64_t)blockIdx.x * 4 + wave;
  if (i >= n_streams) return;                        // wave-uniform; no block barrier below
  const uint64_t o = off[i];
  const uint8_t *in = src + o;
  const uint32_t n = (uint32_t)(off[i + 1] - o);     // at most BW_MAX_PAYLOAD: the host has seen to it
  uint8_t *out = slots + bw_slot_off(o, i);
  const uint32_t adler = adler32_wave(in, n, lane);
  bool stored = mode == 1;
  uint32_t total = 0;
  if (!stored) {
    uint16_t *tab = sh_tab[wave];
    for (int k = lane; k < OBUF_WORDS; k += 64) sh_obuf[wave][k] = 0;
    BitWriter bw{sh_obuf[wave], out + 2, 3u, 3u, 0u};   // BFINAL = 1, BTYPE = 01 (fixed Huffman)
    for (uint32_t s0 = 0; s0 < n; s0 += BW_SEGMENT) {   // matches stay inside a segment; the tokens of all are one block
      const uint8_t *sin = in + s0;
      const uint32_t sn = n - s0 < BW_SEGMENT ? n - s0 : BW_SEGMENT;
      for (int k = lane; k < HASH_SIZE; k += 64) tab[k] = EMPTY16;
      __builtin_amdgcn_wave_barrier();
      uint32_t skip_until = 0;
      uint32_t wn0 = (lane + 4u <= sn) ? *(const u32u *)(sin + lane) : 0u, wn1 = (lane + 68u <= sn) ? *(const u32u *)(sin + lane + 64u) : 0u;
      for (uint32_t p = 0; p < sn; p += 128) {
        const uint32_t w0 = wn0, w1 = wn1;
        if (p + lane + 128u + 4u <= sn) wn0 = *(const u32u *)(sin + p + lane + 128u);
        if (p + lane + 192u + 4u <= sn) wn1 = *(const u32u *)(sin + p + lane + 192u);
        Token tk[2];
        parse_step(sin, sn, p, lane, tab, w0, w1, skip_until, tk[0], tk[1]);
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
          if (!__ballot(tk[hh].kind != 0)) continue;
          uint32_t va = 0, na = 0;
          if (tk[hh].kind == 1) {
            if (tk[hh].byte < 144u) { va = bitrev(0x30u + tk[hh].byte, 8); na = 8; } else { va = bitrev(0x190u + (tk[hh].byte - 144u), 9); na = 9; }
          } else if (tk[hh].kind == 2) {
            uint32_t lv, dv;
            int ln = len_bits(tk[hh].len, lv), dn = dist_bits(tk[hh].dist, dv);
            va = lv | (dv << ln); na = (uint32_t)(ln + dn);
          }
          bw.round(lane, va, na, 0, 0);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    bw.round(lane, 0, lane == 0 ? 7u : 0u, 0, 0);    // end-of-block symbol 256: seven zero bits
    const uint32_t nbytes = bw.finish(lane);
    total = 2u + nbytes + 4u;
    if (nbytes >= n) { stored = true; __threadfence(); }   // not smaller than the payload: the slot is written again
  }
  if (stored) {   // BTYPE 00 blocks of up to 65535 bytes: one for every payload the public entry point takes
    const uint32_t nblk = n ? (n + 65534u) / 65535u : 1u;
    for (uint32_t j = lane; j < n; j += 64) out[2u + 5u * (j / 65535u + 1u) + j] = in[j];
    if ((uint32_t)lane < nblk) {
      const uint32_t first = (uint32_t)lane * 65535u, len = n - first < 65535u ? n - first : 65535u;
      uint8_t *h = out + 2u + 5u * (uint32_t)lane + first;
      h[0] = (uint32_t)lane + 1u == nblk ? 1 : 0;
      h[1] = (uint8_t)len; h[2] = (uint8_t)(len >> 8); h[3] = (uint8_t)~len; h[4] = (uint8_t)(~len >> 8);
    }
    total = 2u + 5u * nblk + n + 4u;
  }
  if (lane == 0) {
    out[0] = 0x78; out[1] = 0x9c;
    uint8_t *t = out + total - 4u;
    t[0] = (uint8_t)(adler >> 24); t[1] = (uint8_t)(adler >> 16); t[2] = (uint8_t)(adler >> 8); t[3] = (uint8_t)adler;
    sizes[i] = total;
  }
}

__global__ void __launch_bounds__(256) k_bw_gather(const uint8_t *slots, const uint64_t *off, const uint64_t *pos, uint64_t n, uint8_t *dst) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t i = (uint64_t)blockIdx.x * 4 + wave;
  if (i >= n) return;
  const uint8_t *s = slots + bw_slot_off(off[i], i);
  uint8_t *d = dst + pos[i];
  const uint32_t len = (uint32_t)(pos[i + 1] - pos[i]), n16 = len & ~15u;
  struct __attribute__((packed, aligned(1))) W4 { uint32_t a, b, c, d; };
  for (uint32_t k = 16u * lane; k < n16; k += 16u * 64u) *(W4 *)(d + k) = *(const W4 *)(s + k);
  for (uint32_t k = n16 + lane; k < len; k += 64) d[k] = s[k];
}

// ---- R-tree levels -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bw_tree_reduce(const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t bs, uint64_t *lo_out, uint64_t *hi_out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j * bs >= n) return;
  const uint64_t e = (j + 1) * bs < n ? (j + 1) * bs : n;
  uint64_t a = lo[j * bs], b = hi[j * bs];
  for (uint64_t i = j * bs + 1; i < e; i++) { a = lo[i] < a ? lo[i] : a; b = hi[i] > b ? hi[i] : b; }
  lo_out[j] = a; hi_out[j] = b;
}

// a lane per item slot of the level: node = slot / bs.  The words of a node begin 4 bytes into it, so 64-bit fields go as two words
__global__ void __launch_bounds__(256) k_bw_tree_nodes(BwNodeArgs A) {
  const uint64_t slot = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= A.n_nodes * A.bs) return;
  const uint64_t node = slot / A.bs, k = slot - node * A.bs, i = slot;
  const uint32_t words = A.leaf ? 8u : 6u;
  uint32_t *base = (uint32_t *)(A.out + node * (4 + (uint64_t)A.bs * 4 * words));
  if (k == 0) {
    const uint64_t left = A.n > node * A.bs ? A.n - node * A.bs : 0;
    base[0] = (A.leaf ? 1u : 0u) | ((uint32_t)(left < A.bs ? left : A.bs) << 16);
  }
  uint32_t *item = base + 1 + k * words;
  if (i >= A.n) { for (uint32_t q = 0; q < words; q++) item[q] = 0; return; }
  const uint64_t a = A.lo[i], b = A.hi[i];
  item[0] = (uint32_t)(a >> 32); item[1] = (uint32_t)a; item[2] = (uint32_t)(b >> 32); item[3] = (uint32_t)b;
  if (A.leaf) {
    const uint64_t at = A.data_base + A.pos[i], len = A.pos[i + 1] - A.pos[i];
    item[4] = (uint32_t)at; item[5] = (uint32_t)(at >> 32); item[6] = (uint32_t)len; item[7] = (uint32_t)(len >> 32);
  } else {
    const uint64_t at = A.child_off + i * A.child_size;
    item[4] = (uint32_t)at; item[5] = (uint32_t)(at >> 32);
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
static inline unsigned blocks_of(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

void launch_bw_run_first(hipStream_t st, const uint4 *runs, uint64_t n_runs, int64_t n_tx, uint64_t *first) {
  hipLaunchKernelGGL(k_bw_run_first, dim3(blocks_of((uint64_t)n_tx + 1)), dim3(256), 0, st, runs, n_runs, n_tx, first);
}
void launch_bw_sections(hipStream_t st, const BwPackArgs &A) {
  if (A.n_sec) hipLaunchKernelGGL(k_bw_sections, dim3(blocks_of(A.n_sec)), dim3(256), 0, st, A);
}
void launch_bw_pack(hipStream_t st, const BwPackArgs &A) {
  if (A.n_runs) hipLaunchKernelGGL(k_bw_pack, dim3(blocks_of(A.n_runs)), dim3(256), 0, st, A);
}
void launch_bw_total(hipStream_t st, const uint4 *runs, const uint64_t *run_depth, uint64_t n_runs, uint64_t *partial) {
  hipLaunchKernelGGL(k_bw_total, dim3(BW_TOTAL_BLOCKS), dim3(256), 0, st, runs, run_depth, n_runs, partial);
}
void launch_bw_zoom_windows(hipStream_t st, const BwZoomArgs &A) {
  if (!A.n_win) return;
  const dim3 grid(blocks_of(A.n_win * (uint64_t)A.G));
  if (A.wide) hipLaunchKernelGGL(k_bw_zoom_windows<uint64_t>, grid, dim3(256), 0, st, A);
  else hipLaunchKernelGGL(k_bw_zoom_windows<uint32_t>, grid, dim3(256), 0, st, A);
}
void launch_bw_zoom_compact(hipStream_t st, const uint4 *rec, const uint64_t *pos, uint64_t n_win, uint4 *out) {
  if (n_win) hipLaunchKernelGGL(k_bw_zoom_compact, dim3(blocks_of(n_win)), dim3(256), 0, st, rec, pos, n_win, out);
}
void launch_bw_zoom_blocks(hipStream_t st, const uint4 *rec, uint64_t n_rec, uint32_t S, uint64_t n_blocks, uint64_t *off, uint64_t *lo, uint64_t *hi) {
  hipLaunchKernelGGL(k_bw_zoom_blocks, dim3(blocks_of(n_blocks + 1)), dim3(256), 0, st, rec, n_rec, S, n_blocks, off, lo, hi);
}
void launch_bw_zlib(hipStream_t st, const uint8_t *src, const uint64_t *off, uint64_t n, int mode, uint8_t *slots, uint64_t *sizes) {
  if (n) hipLaunchKernelGGL(k_bw_zlib, dim3(blocks_of(n, 4)), dim3(256), 0, st, src, off, n, mode, slots, sizes);
}
void launch_bw_gather(hipStream_t st, const uint8_t *slots, const uint64_t *off, const uint64_t *pos, uint64_t n, uint8_t *dst) {
  if (n) hipLaunchKernelGGL(k_bw_gather, dim3(blocks_of(n, 4)), dim3(256), 0, st, slots, off, pos, n, dst);
}
void launch_bw_tree_reduce(hipStream_t st, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t bs, uint64_t *lo_out, uint64_t *hi_out) {
  if (n) hipLaunchKernelGGL(k_bw_tree_reduce, dim3(blocks_of((n + bs - 1) / bs)), dim3(256), 0, st, lo, hi, n, bs, lo_out, hi_out);
}
void launch_bw_tree_nodes(hipStream_t st, const BwNodeArgs &A) {
  hipLaunchKernelGGL(k_bw_tree_nodes, dim3(blocks_of(A.n_nodes * A.bs)), dim3(256), 0, st, A);
}

}  // namespace br
