// The unprojected records of a bundle: the complement of the emitted rows' input alignments (host side: unprojected.cpp).
//
//   mark     k_unproj_mark: one thread per emitted row stores 1 at its input alignment (plain stores into a zeroed array)
//   names    k_unproj_names: per read-name group the number of flagged alignments -> the two name counters; scope name: the
//            groups with a flag are flagged whole.  A lane per group up to 64 alignments, the wave per group above
//   sizes    k_unproj_size: 4 + block_size and 1 for every unflagged record, else 0 (scanned by launch_scan)
//   gather   k_unproj_gather<G>: G lanes per unprojected record, grid-stride: [block_size][record] into the arena, its offset
//            into the offset table
#include <hip/hip_runtime.h>

#include "unprojected_kernels.h"
#include "wave_inl.h"

namespace br {

namespace {
__device__ __forceinline__ uint32_t rec_bytes(const UnprojArgs &A, int64_t i) {
  return A.rec_len ? A.rec_len[i] : (uint32_t)(A.rec_off[i + 1] - A.rec_off[i]);
}
}  // namespace

__global__ void __launch_bounds__(256) k_unproj_mark(UnprojArgs A) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= A.n_rows) return;
  const uint32_t i = ((const uint32_t *)(A.r_rec + r))[A.rec_x ? 0 : 1];
  if ((int64_t)i < A.n_aln) A.flag[i] = 1;
}

// a wave takes 64 consecutive groups: every lane counts its own group when that has at most 64 alignments, then the wave
// goes through the larger ones together (the dense locus, multimappers)
__global__ void __launch_bounds__(256) k_unproj_names(UnprojArgs A) {
  const uint32_t lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t a = 0, e = 0;
  if (g < A.n_groups) { a = A.group_off[g]; e = A.group_off[g + 1]; }
  const bool big = e - a > 64;
  uint32_t cnt = 0;
  if (!big) {
    for (uint32_t i = a; i < e; i++) cnt += A.flag[i];
    if (A.scope == 2 && cnt && cnt < e - a) for (uint32_t i = a; i < e; i++) A.flag[i] = 1;
  }
  wave_turns(big, [&](int src) {
    const uint32_t ba = (uint32_t)__shfl((int)a, src), be = (uint32_t)__shfl((int)e, src);
    uint32_t c = 0;
    for (uint32_t i = ba + lane; i < be; i += 64) c += A.flag[i];
    c = wave_sum(c);
    if (A.scope == 2 && c && c < be - ba) for (uint32_t i = ba + lane; i < be; i += 64) A.flag[i] = 1;
    if ((int)lane == src) cnt = c;
  });
  const bool none = g < A.n_groups && e > a && cnt == 0, part = g < A.n_groups && cnt && cnt < e - a;
  const uint64_t b_none = __ballot(none), b_part = __ballot(part);
  if (lane == 0) {
    if (b_none) atomicAdd((unsigned long long *)(A.small + UNPROJ_NAMES_NONE), (unsigned long long)__popcll(b_none));
    if (b_part) atomicAdd((unsigned long long *)(A.small + UNPROJ_NAMES_PART), (unsigned long long)__popcll(b_part));
  }
}

__global__ void __launch_bounds__(256) k_unproj_size(UnprojArgs A) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_aln) return;
  const bool un = A.flag[i] == 0;
  A.len[i] = un ? 4u + rec_bytes(A, i) : 0u;
  A.one[i] = un ? 1u : 0u;
}

// Source and destination have any alignment: the block_size word and the bytes up to the destination's first 8-byte boundary
// go byte by byte, the destination's 8-byte words are built from two aligned, non-temporal source words (the input is read
// once; an aligned word that holds a byte of the record lies inside the record's allocation granule, so nothing is read that
// the record does not reach into), the rest goes byte by byte.
template <uint32_t G>
__global__ void __launch_bounds__(256) k_unproj_gather(UnprojArgs A) {
  const uint32_t lane = threadIdx.x & (G - 1);
  const int64_t groups = (int64_t)gridDim.x * (256 / G);
  for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < A.n_aln; i += groups) {
    const uint64_t d = A.out_off[i], bytes = A.out_off[i + 1] - d;
    if (bytes == 0) continue;   // projected
    const uint64_t len = bytes - 4;
    const uint8_t *s = A.blob + A.rec_off[i];
    uint8_t *t = A.arena + A.arena_base + d;
    if (lane < 4) t[lane] = (uint8_t)(len >> (8 * lane));
    t += 4;
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
    const uint64_t done = head + (words << 3);   // (fewer than 8 bytes are left)
    if (done + lane < len) t[done + lane] = s[done + lane];
    if (lane == 0) {
      const uint64_t k = A.rank[i];
      A.off[k] = A.arena_base + d;
      if (k + 1 == A.n_new) A.off[A.n_new] = A.arena_base + A.new_bytes;
    }
  }
}

static unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

void launch_unproj_mark(hipStream_t st, const UnprojArgs &A) {
  if (A.n_rows > 0) hipLaunchKernelGGL(k_unproj_mark, dim3(blocks256(A.n_rows)), dim3(256), 0, st, A);
}
void launch_unproj_names(hipStream_t st, const UnprojArgs &A) {
  if (A.n_groups > 0) hipLaunchKernelGGL(k_unproj_names, dim3(blocks256(A.n_groups)), dim3(256), 0, st, A);
}
void launch_unproj_size(hipStream_t st, const UnprojArgs &A) {
  if (A.n_aln > 0) hipLaunchKernelGGL(k_unproj_size, dim3(blocks256(A.n_aln)), dim3(256), 0, st, A);
}
void launch_unproj_gather(hipStream_t st, const UnprojArgs &A, int lanes, int n_cu) {
  if (A.n_aln <= 0 || A.n_new == 0) return;
  const int64_t per = 256 / lanes, want = (A.n_aln + per - 1) / per, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 8;
  const dim3 grid((unsigned)(want < cap ? want : cap));
  if (lanes == 64) hipLaunchKernelGGL(k_unproj_gather<64>, grid, dim3(256), 0, st, A);
  else if (lanes == 32) hipLaunchKernelGGL(k_unproj_gather<32>, grid, dim3(256), 0, st, A);
  else hipLaunchKernelGGL(k_unproj_gather<16>, grid, dim3(256), 0, st, A);
}

}  // namespace br
