// The field sort on the device (host side: barcode_sort.h, which holds the passes): the items that take part, the key of one pass
// and the heads of the sorted items' runs.  Integers only, a lane per item, no atomics.
#include <hip/hip_runtime.h>

#include "barcode_kernels.h"

namespace br {

namespace {
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

__global__ void __launch_bounds__(256) k_bc_compact(const uint64_t *pos, int64_t n, uint32_t *idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && pos[i + 1] != pos[i]) idx[pos[i]] = (uint32_t)i;
}
void launch_bc_compact(hipStream_t st, const uint64_t *pos, int64_t n, uint32_t *idx) {
  if (n > 0) hipLaunchKernelGGL(k_bc_compact, dim3(blocks256(n)), dim3(256), 0, st, pos, n, idx);
}

__global__ void __launch_bounds__(256) k_bc_key(const uint32_t *idx, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int64_t n, int w,
                                                uint64_t *key) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = idx[j];
  key[j] = w < 4 ? words[4 * (uint64_t)i + w] : ((gid ? (uint64_t)gid[i] << 8 : 0ull) | (uint64_t)len[i]);
}
void launch_bc_key(hipStream_t st, const uint32_t *idx, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int64_t n, int w, uint64_t *key) {
  if (n > 0) hipLaunchKernelGGL(k_bc_key, dim3(blocks256(n)), dim3(256), 0, st, idx, words, len, gid, n, w, key);
}

__global__ void __launch_bounds__(256) k_bc_heads(const uint32_t *idx, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int empty_is_head,
                                                  int64_t n, uint64_t *head) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  uint64_t h = 1;
  if (j > 0) {
    const uint64_t a = idx[j], b = idx[j - 1];
    h = ((empty_is_head && len[a] == 0) || len[a] != len[b] || (gid && gid[a] != gid[b]) || words[4 * a] != words[4 * b] ||
         words[4 * a + 1] != words[4 * b + 1] || words[4 * a + 2] != words[4 * b + 2] || words[4 * a + 3] != words[4 * b + 3]) ? 1 : 0;
  }
  head[j] = h;
}
void launch_bc_heads(hipStream_t st, const uint32_t *idx, const uint64_t *words, const uint8_t *len, const uint32_t *gid, int empty_is_head, int64_t n,
                     uint64_t *head) {
  if (n > 0) hipLaunchKernelGGL(k_bc_heads, dim3(blocks256(n)), dim3(256), 0, st, idx, words, len, gid, empty_is_head, n, head);
}

}  // namespace br
