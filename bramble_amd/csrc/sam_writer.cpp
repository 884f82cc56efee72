// SAM text out: br_ctx_set_sam_refs, br_sam_format_device, and the formatting step the bundle entry points take instead of the
// deflate (project_bam_tail, bam_path.cpp).  The reference writes only BAM; the text is what `samtools view` prints for the
// records of the same run (sam_format_kernels.hip).
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "sam_format.h"
#include "scan_kernels.h"

extern "C" int br_ctx_set_sam_refs(br_ctx *c, const char *const *names, int32_t n) {
  if (!c || n < 0 || (n && !names)) return BR_ERR_INVALID_ARG;
  std::vector<uint64_t> off((size_t)n + 1, 0);
  std::string blob;
  for (int32_t i = 0; i < n; i++) {
    if (!names[i]) return BR_ERR_INVALID_ARG;
    off[(size_t)i] = blob.size();
    blob += names[i];
  }
  off[(size_t)n] = blob.size();
  HIPCHK(hipSetDevice(c->ix->device));
  RC(c->sf_name_off.ensure(off.size() * 8)); RC(c->sf_names.ensure(blob.size() + 1));
  HIPCHK(hipMemcpy(c->sf_name_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  if (!blob.empty()) HIPCHK(hipMemcpy(c->sf_names.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
  c->sf_n_names = n;
  return BR_OK;
}

// measure -> scan -> (the total on the host: the text's size) -> emit; the text is complete when the call returns
int sam_format_impl(br_ctx *c, const br_device_bam *in, hipStream_t st, const uint8_t **text, uint64_t *n_bytes) {
  *text = nullptr; *n_bytes = 0;
  Prof pf{c, st};
  c->events_used = 0;
  const int64_t n = in->n_rows;
  if (n == 0) return pf.collect();
  if (n >= 0xffffffffll) return BR_ERR_CAPACITY;   // (the long list holds 32-bit row numbers)
  RC(c->sf_len.ensure(((size_t)n + 1) * 8)); RC(c->sf_long.ensure((size_t)n * 4)); RC(c->sf_small.ensure(16));
  RC(c->sf_tmp.ensure(scan_scratch_bytes(n)));
  if (!c->sf_name_off.p) {   // no names set: every RNAME / RNEXT prints '*'
    RC(c->sf_name_off.ensure(8)); RC(c->sf_names.ensure(8));
    HIPCHK(hipMemsetAsync(c->sf_name_off.p, 0, 8, st));
  }
  unsigned long long *first_bad = c->sf_small.as<unsigned long long>();
  uint32_t *n_long = (uint32_t *)(c->sf_small.as<uint8_t>() + 8);
  HIPCHK(hipMemsetAsync(first_bad, 0xff, 8, st));
  HIPCHK(hipMemsetAsync(n_long, 0, 4, st));
  SamFmtArgs A{};
  A.data = in->data; A.n_bytes = in->n_bytes; A.row_off = in->row_off; A.n = n;
  A.name_off = c->sf_name_off.as<uint64_t>(); A.names = c->sf_names.as<uint8_t>(); A.n_names = c->sf_n_names;
  A.len = c->sf_len.as<uint64_t>(); A.long_list = c->sf_long.as<uint32_t>(); A.n_long = n_long; A.first_bad = first_bad;
  RC(pf.begin(BR_K_SAM_FORMAT));
  launch_sam_fmt_measure(st, A, c->n_cu);
  RC(pf.end());
  RC(pf.begin(BR_K_SCAN));
  launch_scan(st, A.len, n, c->sf_tmp.as<uint64_t>());
  RC(pf.end());
  HIPCHK(hipMemcpyAsync(&c->rb->sam_bad, first_bad, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&c->rb->sam_bytes, A.len + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->rb->sam_bad != ~0ull) { pf.collect(); return BR_ERR_INVALID_ARG; }   // a record the text cannot say: no line of it
  const uint64_t total = c->rb->sam_bytes;
  DevBuf &tb = c->sf_text[c->sf_which];
  RC(tb.ensure((size_t)total + 16));
  A.text = tb.as<uint8_t>();
  RC(pf.begin(BR_K_SAM_FORMAT));
  launch_sam_fmt_emit(st, A, c->n_cu);
  RC(pf.end());
  HIPCHK(hipStreamSynchronize(st));
  RC(pf.collect());
  *text = A.text; *n_bytes = total;
  return BR_OK;
}

extern "C" int br_sam_format_device(br_ctx *c, const br_device_bam *in, void *stream, const uint8_t **text, uint64_t *n_bytes) {
  if (!c || !in || !text || !n_bytes || in->n_rows < 0 || (in->n_rows && (!in->data || !in->row_off))) return BR_ERR_INVALID_ARG;
  *text = nullptr; *n_bytes = 0;
  HIPCHK(hipSetDevice(c->ix->device));
  return sam_format_impl(c, in, (hipStream_t)stream, text, n_bytes);
}
