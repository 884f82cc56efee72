// Coordinate sort and BAI index on the device (host side: sort.cpp, which holds the pipeline's description).
//
//   add      k_sort_offs: the offset table of the appended rows (the bytes themselves are one device copy)
//   key      k_sort_key: refID, pos, strand -> key; the CIGAR walk leaves each record's end for the index
//   sort     launch_col_radix_pass (collate_kernels.hip) per 8-bit digit that is not constant
//   next     k_sort_lens + scan: offsets in the sorted stream; k_sort_cut; k_sort_gather: SORT_GATHER_LANES lanes per record (64: a wave)
//   index    k_bai_rec (virtual offset, bin, largest end per reference) -> radix sort of (refID, bin) -> k_bai_heads + scans ->
//            k_bai_binc0 -> k_bai_refs + scans (sizes) -> k_bai_lin (atomicMin per window) -> k_bai_write_refs / _items
#include <hip/hip_runtime.h>

#include "collate_kernels.h"
#include "sort_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }
// (the image's fields sit at multiples of 4)
__device__ __forceinline__ void st32(uint8_t *out, uint64_t at, uint32_t v) { *(uint32_t *)(out + at) = v; }
__device__ __forceinline__ void st64(uint8_t *out, uint64_t at, uint64_t v) { st32(out, at, (uint32_t)v); st32(out, at + 4, (uint32_t)(v >> 32)); }
// SAM specification 5.3: the smallest bin that holds [beg, end)
__device__ __forceinline__ uint32_t reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
  return 0;
}
// the first k in [0, n) with a[k] >= v (n when none)
__device__ __forceinline__ int64_t lower_bound(const uint64_t *a, int64_t n, uint64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ int32_t key_ref(uint64_t k) { return (int32_t)(uint32_t)(k >> 32); }
__device__ __forceinline__ int32_t key_pos(uint64_t k) { return (int32_t)((uint32_t)k >> 1) - 1; }
}  // namespace

// (*bad is set when the table descends somewhere: the rows would have negative sizes)
__global__ void __launch_bounds__(256) k_sort_offs(const uint64_t *row_off, int64_t m, uint64_t base, uint64_t *off, uint32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  off[i] = base + (row_off[i] - row_off[0]);
  if (i < m && row_off[i + 1] < row_off[i]) *bad = 1;
}

__global__ void __launch_bounds__(256) k_sort_key(const uint8_t *arena, const uint64_t *off, int64_t n, uint64_t *key, uint32_t *idx,
                                                  uint32_t *ends, uint64_t *part, uint32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t o = 0, a = ~0ull;
  if (i < n) {
    const uint64_t at = off[i], bytes = off[i + 1] - at;
    uint64_t k = ~0ull;      // (a row too short for the fixed fields: last, in no bin)
    uint32_t e = 0;
    if (bytes >= 36) {
      const uint8_t *r = arena + at + 4;
      const int32_t ref = (int32_t)ld32(r), pos = (int32_t)ld32(r + 4);
      const uint32_t l_name = r[8], flag = ld16(r + 14);
      uint32_t n_cig = ld16(r + 12);
      const uint64_t room = bytes - 36 >= l_name ? (bytes - 36 - l_name) / 4 : 0;   // CIGAR words the row has room for
      if (n_cig > room) n_cig = (uint32_t)room;
      const uint8_t *c = r + 32 + l_name;
      uint64_t rl = 0;
      for (uint32_t q = 0; q < n_cig; q++) {
        const uint32_t w = ld32(c + 4 * q), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += w >> 4;   // M D N = X
      }
      if (pos < -1 || pos == 0x7fffffff) *bad = 1;   // (no BAM position: pos + 1 would not fit the key's 31 bits)
      k = (uint64_t)(uint32_t)ref << 32 | (uint64_t)(uint32_t)(pos + 1) << 1 | ((flag >> 4) & 1u);
      const int64_t end = (int64_t)pos + (int64_t)(rl ? rl : 1);
      e = (uint32_t)(end < 0 ? 0 : end > (int64_t)SORT_END_MAX ? (int64_t)SORT_END_MAX : end) | ((flag >> 2) & 1u) << 31;
    }
    key[i] = k; idx[i] = (uint32_t)i; ends[i] = e;
    o = k; a = k;
  }
  block_bits(o, a, part + 2 * blockIdx.x);
}

__global__ void __launch_bounds__(256) k_sort_lens(const uint64_t *off, const uint32_t *idx, int64_t n, uint64_t *len) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) { const uint32_t i = idx[j]; len[j] = off[i + 1] - off[i]; }
}

__global__ void k_sort_cut(const uint64_t *s_off, int64_t n, int64_t cur, uint64_t max_bytes, uint64_t *res) {
  const uint64_t base = s_off[cur];
  int64_t lo = cur + 1, hi = n;   // the largest e with s_off[e] - base <= max_bytes
  while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (s_off[mid] - base <= max_bytes) lo = mid; else hi = mid - 1; }
  res[0] = (uint64_t)lo; res[1] = s_off[lo] - base;
}

// SORT_GATHER_LANES lanes per record (a record of the projected stream is some 220 bytes: 28 words), grid-stride.  Source and
// destination have any alignment: the destination's 8-byte words are built from two aligned, non-temporal source words (the
// arena is read once), the ends go byte by byte.
__global__ void __launch_bounds__(256) k_sort_gather(const uint8_t *arena, const uint64_t *off, const uint32_t *idx, const uint64_t *s_off,
                                                     int64_t cur, int64_t e, uint8_t *dst, uint64_t *row_off) {
  constexpr uint32_t G = SORT_GATHER_LANES;
  const uint32_t lane = threadIdx.x & (G - 1);
  const int64_t groups = (int64_t)gridDim.x * (256 / G);
  const uint64_t base = s_off[cur];
  for (int64_t j = cur + (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; j < e; j += groups) {
    const uint32_t i = idx[j];
    const uint64_t d = s_off[j] - base, len = s_off[j + 1] - s_off[j];
    const uint8_t *s = arena + off[i];
    uint8_t *t = dst + d;
    uint64_t head = (8 - ((uintptr_t)t & 7)) & 7;
    if (head > len) head = len;
    if (lane < head) t[lane] = s[lane];
    const uint64_t words = (len - head) >> 3;
    const uint8_t *sb = s + head;
    const uint32_t sh = (uint32_t)((uintptr_t)sb & 7) * 8;
    const uint64_t *sa = (const uint64_t *)((uintptr_t)sb & ~(uintptr_t)7);
    uint64_t *ta = (uint64_t *)(t + head);
    for (uint64_t w = lane; w < words; w += G) {
      uint64_t v = __builtin_nontemporal_load(sa + w);
      if (sh) v = v >> sh | __builtin_nontemporal_load(sa + w + 1) << (64 - sh);
      ta[w] = v;
    }
    const uint64_t done = head + (words << 3);
    if (done + lane < len) t[done + lane] = s[done + lane];
    if (lane == 0) { row_off[j - cur] = d; if (j == e - 1) row_off[e - cur] = d + len; }
  }
}

// ---- the index -----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_bai_rec(BaiArgs A) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t o = 0, a = ~0ull;
  bool no_coor = false;
  uint32_t err = 0;
  if (j < A.n) {
    const uint64_t u = A.s_off[j];
    int64_t lo = 0, hi = A.n_blk;   // the last block that starts at or before u
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (A.blk[2 * mid + 1] <= u) lo = mid + 1; else hi = mid; }
    uint64_t v = 0;
    if (lo == 0 || u - A.blk[2 * (lo - 1) + 1] >= 65536) err |= BAI_ERR_BLOCKS;
    else v = A.blk[2 * (lo - 1)] << 16 | (u - A.blk[2 * (lo - 1) + 1]);
    A.vo[j] = v;
    if (j == 0) A.vo[A.n] = A.eof_coffset << 16;
    const uint64_t k = A.key[j];
    const int32_t ref = key_ref(k), pos = key_pos(k);
    const uint32_t e = A.ends[A.idx[j]], end = e & SORT_END_MAX;
    A.um[j] = e >> 31;
    uint64_t k2 = SORT_NO_BIN;
    if (ref >= A.n_ref) err |= BAI_ERR_REF;
    else if (ref < 0 || pos < 0) no_coor = true;
    else if (end > BAI_MAX_END) err |= BAI_ERR_RANGE;
    else {
      k2 = (uint64_t)(uint32_t)ref << 32 | reg2bin((uint32_t)pos, end);
      // the reference's largest end: a record whose successor on the same reference ends no earlier leaves it to that one,
      // so a pile of reads on one transcript is a few atomics on its counter, not one per read
      bool mine = true;
      if (j + 1 < A.n) {
        const uint64_t kn = A.key[j + 1];
        if (key_ref(kn) == ref && key_pos(kn) >= 0 && (A.ends[A.idx[j + 1]] & SORT_END_MAX) >= end) mine = false;
      }
      if (mine) atomicMax(&A.refmax[ref], end);
    }
    A.key2[0][j] = k2; A.idx2[0][j] = (uint32_t)j;
    o = k2; a = k2;
  }
  // the records without coordinate are one run at the end of the file: a count per block through LDS, one atomic a block
  __shared__ uint32_t s_nc, s_err;
  if (threadIdx.x == 0) { s_nc = 0; s_err = 0; }
  __syncthreads();
  const uint64_t bal = __ballot(no_coor);
  uint32_t werr = 0;
  for (uint32_t b = 1; b <= BAI_ERR_REF; b <<= 1) if (__ballot(err & b)) werr |= b;
  if ((threadIdx.x & 63) == 0) { if (bal) atomicAdd(&s_nc, (uint32_t)__popcll(bal)); if (werr) atomicOr(&s_err, werr); }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_nc) atomicAdd((unsigned long long *)(A.small + 2), (unsigned long long)s_nc);
    if (s_err) atomicOr((unsigned long long *)(A.small + 3), (unsigned long long)s_err);
  }
  block_bits(o, a, A.part + 2 * blockIdx.x);
}

// in (refID, bin) order: a bin starts at a new key, a chunk at a new bin or where the record is not the file successor of the one
// in front (the sort is stable: inside a bin the records are in file order)
__global__ void __launch_bounds__(256) k_bai_heads(BaiArgs A) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= A.n) return;
  const uint64_t *K = A.key2[A.cur];
  const uint32_t *I = A.idx2[A.cur];
  const uint64_t me = K[k];
  const bool valid = me != SORT_NO_BIN;
  const bool bh = valid && (k == 0 || K[k - 1] != me);
  const bool ch = valid && (bh || I[k] != I[k - 1] + 1);
  A.bh[k] = bh; A.ch[k] = ch;
}

// binc0[b] = the first chunk of bin b; binc0[n_bins] = the number of chunks
__global__ void __launch_bounds__(256) k_bai_binc0(BaiArgs A) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < A.n && A.bh[k + 1] != A.bh[k]) A.binc0[A.bh[k]] = A.ch[k];
  if (k == A.n) A.binc0[A.bh[A.n]] = A.ch[A.n];
}

__global__ void __launch_bounds__(256) k_bai_refs(BaiArgs A) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= A.n_ref) return;
  const uint64_t *K = A.key2[A.cur];
  BaiRef R;
  R.jb = (uint64_t)lower_bound(A.key, A.n, (uint64_t)r << 32 | 2u);   // (pos >= 0: the key's low word is 2 or more)
  R.je = (uint64_t)lower_bound(A.key, A.n, (uint64_t)(r + 1) << 32);
  const int64_t k0 = lower_bound(K, A.n, (uint64_t)r << 32), k1 = lower_bound(K, A.n, (uint64_t)(r + 1) << 32);
  R.bin0 = A.bh[k0]; R.n_bin = A.bh[k1] - R.bin0;
  R.chunk0 = A.ch[k0]; R.n_chunk = A.ch[k1] - R.chunk0;
  R.n_intv = R.je > R.jb ? 1u + ((A.refmax[r] - 1u) >> 14) : 0;
  A.ref[r] = R;
  A.lin_off[r] = R.n_intv;
  A.ref_pos[r] = 4 + 8 * R.n_bin + 16 * R.n_chunk + (R.je > R.jb ? 40 : 0) + 4 + 8 * R.n_intv;
}

// ioffset: the smallest virtual offset among the records that overlap a window.  A window that the record in front (same
// reference, an earlier offset) overlaps too is left to that record.
__global__ void __launch_bounds__(256) k_bai_lin(BaiArgs A) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n) return;
  const uint64_t k = A.key[j];
  const int32_t ref = key_ref(k), pos = key_pos(k);
  if (ref < 0 || pos < 0) return;
  const uint32_t end = A.ends[A.idx[j]] & SORT_END_MAX;
  uint32_t w = (uint32_t)pos >> 14;
  const uint32_t we = (end - 1) >> 14;
  if (j > 0) {
    const uint64_t kp = A.key[j - 1];
    if (key_ref(kp) == ref && key_pos(kp) >= 0) {
      const uint32_t pe = ((A.ends[A.idx[j - 1]] & SORT_END_MAX) - 1) >> 14;
      if (pe + 1 > w) w = pe + 1;
    }
  }
  unsigned long long *lin = (unsigned long long *)(A.lin + A.lin_off[ref]);
  const unsigned long long v = A.vo[j];
  for (; w <= we; w++) atomicMin(lin + w, v);
}

// per reference: n_bin, the pseudo-bin, n_intv and the windows (an empty one takes the next one's value, from the right);
// the thread behind the last reference writes the magic, n_ref and the trailing n_no_coor
__global__ void __launch_bounds__(256) k_bai_write_refs(BaiArgs A) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > A.n_ref) return;
  if (r == A.n_ref) {
    st32(A.out, 0, 0x01494142u);   // "BAI\1"
    st32(A.out, 4, (uint32_t)A.n_ref);
    st64(A.out, 8 + A.ref_pos[A.n_ref], A.small[2]);
    return;
  }
  const BaiRef R = A.ref[r];
  const bool any = R.je > R.jb;
  uint64_t p = 8 + A.ref_pos[r];
  st32(A.out, p, (uint32_t)R.n_bin + (any ? 1u : 0u));
  p += 4 + 8 * R.n_bin + 16 * R.n_chunk;
  if (any) {
    const uint64_t n_un = A.um[R.je] - A.um[R.jb];
    st32(A.out, p, 37450u); st32(A.out, p + 4, 2u);
    st64(A.out, p + 8, A.vo[R.jb]); st64(A.out, p + 16, A.vo[R.je]);
    st64(A.out, p + 24, R.je - R.jb - n_un); st64(A.out, p + 32, n_un);
    p += 40;
  }
  st32(A.out, p, (uint32_t)R.n_intv);
  p += 4;
  const uint64_t *lin = A.lin + A.lin_off[r];
  uint64_t last = ~0ull;
  for (int64_t w = (int64_t)R.n_intv - 1; w >= 0; w--) {
    uint64_t v = lin[w];
    if (v == ~0ull) v = last; else last = v;
    st64(A.out, p + 8 * (uint64_t)w, v);
  }
}

// per record in (refID, bin) order: a bin head writes the bin's number and chunk count, a chunk head the chunk's begin, a
// chunk's last record its end (the begin of the file's next record)
__global__ void __launch_bounds__(256) k_bai_write_items(BaiArgs A) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= A.n) return;
  const uint64_t *K = A.key2[A.cur];
  const uint32_t *I = A.idx2[A.cur];
  const uint64_t me = K[k];
  if (me == SORT_NO_BIN) return;
  const BaiRef R = A.ref[me >> 32];
  const uint64_t b = A.bh[k + 1] - 1, c = A.ch[k + 1] - 1, c0 = A.binc0[b];
  const uint64_t binpos = 8 + A.ref_pos[me >> 32] + 4 + 8 * (b - R.bin0) + 16 * (c0 - R.chunk0);
  if (A.bh[k + 1] != A.bh[k]) { st32(A.out, binpos, (uint32_t)me); st32(A.out, binpos + 4, (uint32_t)(A.binc0[b + 1] - c0)); }
  const uint64_t cp = binpos + 8 + 16 * (c - c0);
  if (A.ch[k + 1] != A.ch[k]) st64(A.out, cp, A.vo[I[k]]);
  if (k + 1 >= A.n || K[k + 1] == SORT_NO_BIN || A.ch[k + 2] != A.ch[k + 1]) st64(A.out, cp + 8, A.vo[I[k] + 1]);
}

static unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

void launch_sort_offs(hipStream_t st, const uint64_t *row_off, int64_t m, uint64_t base, uint64_t *off, uint32_t *bad) {
  hipLaunchKernelGGL(k_sort_offs, dim3(blocks256(m + 1)), dim3(256), 0, st, row_off, m, base, off, bad);
}
void launch_sort_key(hipStream_t st, const uint8_t *arena, const uint64_t *off, int64_t n, uint64_t *key, uint32_t *idx, uint32_t *ends,
                     uint64_t *part, uint64_t *bits, uint32_t *bad) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sort_key, dim3(blocks256(n)), dim3(256), 0, st, arena, off, n, key, idx, ends, part, bad);
  launch_col_bits(st, part, (int64_t)blocks256(n), bits);
}
void launch_sort_lens(hipStream_t st, const uint64_t *off, const uint32_t *idx, int64_t n, uint64_t *len) {
  if (n > 0) hipLaunchKernelGGL(k_sort_lens, dim3(blocks256(n)), dim3(256), 0, st, off, idx, n, len);
}
void launch_sort_cut(hipStream_t st, const uint64_t *s_off, int64_t n, int64_t cur, uint64_t max_bytes, uint64_t *res) {
  hipLaunchKernelGGL(k_sort_cut, dim3(1), dim3(1), 0, st, s_off, n, cur, max_bytes, res);
}
void launch_sort_gather(hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint32_t *idx, const uint64_t *s_off, int64_t cur,
                        int64_t e, uint8_t *dst, uint64_t *row_off) {
  if (e <= cur) return;
  const int64_t per = 256 / SORT_GATHER_LANES, g = (e - cur + per - 1) / per;
  hipLaunchKernelGGL(k_sort_gather, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(256), 0, st, arena, off, idx, s_off, cur, e, dst, row_off);
}
void launch_bai_rec(hipStream_t st, const BaiArgs &A) {
  if (A.n <= 0) return;
  hipLaunchKernelGGL(k_bai_rec, dim3(blocks256(A.n)), dim3(256), 0, st, A);
  launch_col_bits(st, A.part, (int64_t)blocks256(A.n), A.small);
}
void launch_bai_heads(hipStream_t st, const BaiArgs &A) {
  if (A.n > 0) hipLaunchKernelGGL(k_bai_heads, dim3(blocks256(A.n)), dim3(256), 0, st, A);
}
void launch_bai_binc0(hipStream_t st, const BaiArgs &A) { hipLaunchKernelGGL(k_bai_binc0, dim3(blocks256(A.n + 1)), dim3(256), 0, st, A); }
void launch_bai_refs(hipStream_t st, const BaiArgs &A) {
  if (A.n_ref > 0) hipLaunchKernelGGL(k_bai_refs, dim3(blocks256(A.n_ref)), dim3(256), 0, st, A);
}
void launch_bai_lin(hipStream_t st, const BaiArgs &A) {
  if (A.n > 0) hipLaunchKernelGGL(k_bai_lin, dim3(blocks256(A.n)), dim3(256), 0, st, A);
}
void launch_bai_write(hipStream_t st, const BaiArgs &A) {
  hipLaunchKernelGGL(k_bai_write_refs, dim3(blocks256((int64_t)A.n_ref + 1)), dim3(256), 0, st, A);
  if (A.n > 0) hipLaunchKernelGGL(k_bai_write_items, dim3(blocks256(A.n)), dim3(256), 0, st, A);
}

}  // namespace br
