// The front end of an add of read names, shared by the accumulators that take one (quant.cpp, coverage.cpp, assign.cpp, dedup.cpp,
// cells.cpp): the rows the names span, the names' window of host tables uploaded, the record window of the rows, and the record
// stream the context's last call left.  What an accumulator does differently stands at its call.  Host only.
#pragma once
#include "accum.h"
#include "ctx.h"
#include "quant_kernels.h"

namespace br {

// span = the rows of the names [0, ng), ng > 0: row_off[group_off[0]], row_off[group_off[ng]].  Host tables: refused where group_off
// or the names' part of row_off descends.  Device tables: read after whatever `caller` holds, through d_span, two words of the
// caller's on the device (the add kernels check every name's offsets).  Refused as well where the span descends or leaves n_rows
inline int names_span(Accum *c, const uint64_t *row_off, uint64_t n_rows, const uint32_t *group_off, int64_t ng, bool on_device, hipStream_t caller,
                      uint64_t *d_span, uint64_t span[2]) {
  if (on_device) {
    RC(c->after(caller));
    launch_q_span(c->st, row_off, group_off, ng, d_span);
    HIPCHK(hipMemcpyAsync(span, d_span, 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  } else {
    for (int64_t g = 0; g < ng; g++) if (group_off[g + 1] < group_off[g]) return BR_ERR_INVALID_ARG;
    for (uint32_t i = group_off[0]; i < group_off[ng]; i++) if (row_off[i + 1] < row_off[i]) return BR_ERR_INVALID_ARG;
    span[0] = row_off[group_off[0]]; span[1] = row_off[group_off[ng]];
  }
  return span[1] < span[0] || span[1] > n_rows ? BR_ERR_INVALID_ARG : BR_OK;
}

// the names of device tables, as they are
inline NameWindow device_names(const uint64_t *row_off, const uint32_t *group_off, int64_t ng, const uint64_t span[2]) {
  return NameWindow{row_off, 0, group_off, ng, span[0], span[1]};
}

// the names of host tables: their part of row_off and group_off into d_ro / d_go, which the caller holds under a DropGuard; the
// copies are on the stream, not waited for
inline int upload_names(Accum *c, const uint64_t *row_off, const uint32_t *group_off, int64_t ng, const uint64_t span[2], ColBuf &d_ro, ColBuf &d_go,
                        NameWindow *out) {
  const uint32_t a0 = group_off[0], a1 = group_off[ng];
  RC(c->alloc(d_ro, (size_t)(a1 - a0 + 1) * 8)); RC(c->alloc(d_go, (size_t)(ng + 1) * 4));
  HIPCHK(hipMemcpyAsync(d_ro.p, row_off + a0, (size_t)(a1 - a0 + 1) * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(d_go.p, group_off, (size_t)(ng + 1) * 4, hipMemcpyHostToDevice, c->st));
  *out = NameWindow{d_ro.as<uint64_t>(), (int64_t)a0, d_go.as<uint32_t>(), ng, span[0], span[1]};
  return BR_OK;
}

// The records of the rows [r0, r1): *src (host or device memory, as the stream is) holds their *bytes bytes, the first row's record
// first; w: their offsets and w->data_bias, the first record's offset -- w->data is the caller's to set.  Refused where the ends
// descend or leave n_bytes and, for a host stream, where an offset descends; a host stream's offsets [r0, r1] are uploaded into
// d_rec (the caller's, under a DropGuard; not waited for).  Names without rows: no record is looked at
inline int record_window(Accum *c, const br_device_bam &recs, uint64_t r0, uint64_t r1, bool on_device, ColBuf &d_rec, RecordWindow *w,
                         const uint8_t **src, uint64_t *bytes) {
  uint64_t ends[2] = {0, 0};
  if (r1 > r0 && on_device) {
    HIPCHK(hipMemcpyAsync(&ends[0], recs.row_off + r0, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(&ends[1], recs.row_off + r1, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  } else if (r1 > r0) {
    for (uint64_t r = r0; r < r1; r++) if (recs.row_off[r + 1] < recs.row_off[r]) return BR_ERR_INVALID_ARG;
    ends[0] = recs.row_off[r0]; ends[1] = recs.row_off[r1];
  }
  if (ends[1] < ends[0] || ends[1] > recs.n_bytes) return BR_ERR_INVALID_ARG;
  *w = RecordWindow{recs.row_off, 0, nullptr, ends[0]};
  if (!on_device) {
    RC(c->alloc(d_rec, (size_t)(r1 - r0 + 1) * 8));
    if (r1 > r0) HIPCHK(hipMemcpyAsync(d_rec.p, recs.row_off + r0, (size_t)(r1 - r0 + 1) * 8, hipMemcpyHostToDevice, c->st));
    w->rec_off = d_rec.as<uint64_t>(); w->rec_bias = (int64_t)r0;
  }
  *src = r1 > r0 ? recs.data + ends[0] : nullptr; *bytes = ends[1] - ends[0];
  return BR_OK;
}

// what the context's last call left a record consumer: *flat: rows and no records (a flat batch call); *recs: its record stream,
// empty where it had names without rows -- no record stream was made then
inline void last_call_records(const br_ctx *ctx, br_device_bam *recs, bool *flat) {
  *flat = ctx->last_rows.n_rows && ctx->last_bam.n_rows != ctx->last_rows.n_rows;
  *recs = ctx->last_rows.n_rows ? ctx->last_bam : br_device_bam{};
}

}  // namespace br
