// Constant-time sums and scalar arithmetic over device rows (bpp_rows_msm_enqueue, bpp_rows_scalar_enqueue; include/bpp.h): the
// engine's side of rows_msm.h.  The refusals -- the arguments' own (rows_msm_refusal, rows_scalar_refusal) and the pointer kinds --
// come before anything is counted or launched; then the launches go onto the context's stream: the record's init, per slab of
// BPP_ROWS_SLAB rows the points' decoding and k_rows_msm (shared bases: k_rows_bases once, in front), the record's finish.  Nothing
// is allocated but the context's ticket events and its point buffers (by the first call of a size), nothing is copied, nothing is
// waited for, and no copy of the scalars is made: the kernel reads them where they lie.
#pragma once

namespace {

int rows_pointer_kinds(bpp_ctx *ctx, const std::vector<std::pair<std::string, const void *>> &arrays) {
  for (const auto &a : arrays) {
    if (!a.second) continue;
    const int kind = device_pointer_kind(ctx->device, a.second);
    if (kind != BPP_PTR_THIS_DEVICE)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, a.first + " is not device memory of this context's device (" + upload_pointer_kinds[kind] + ")");
  }
  return BPP_OK;
}

template <bool SHARED>
void rows_msm_launch(uint32_t kp, uint32_t rows, hipStream_t s, const RowsMsm &a) {
  const dim3 grid(cdiv(rows, BPP_CT_QUADS / kp)), block(64);
  switch (kp) {  // (K is public)
    case 1: hipLaunchKernelGGL((k_rows_msm<1, SHARED>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_rows_msm<2, SHARED>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_rows_msm<4, SHARED>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((k_rows_msm<8, SHARED>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_rows_msm<16, SHARED>), grid, block, 0, s, a); break;
  }
}

}  // namespace

extern "C" int bpp_rows_msm_enqueue(bpp_ctx *ctx, const bpp_rows_msm *in, uint8_t *out_dev, size_t out_stride, const uint8_t *live_dev,
                                    uint8_t *done_mask_dev, bpp_device_rows_record *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  try {
    const std::string why = rows_msm_refusal(in, out_dev, out_stride, live_dev, done_mask_dev, record_dev);
    if (!why.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, why);
    if (const int rc = rows_pointer_kinds(ctx, {{"scalars_dev", in->scalars_dev}, {"points_dev", in->points_dev}, {"out_dev", out_dev},
                                                {"live_dev", live_dev}, {"done_mask_dev", done_mask_dev}, {"record_dev", record_dev}}))
      return rc;
    RowsMsm a;
    rows_msm_args(a, *in, out_dev, out_stride, live_dev, done_mask_dev, record_dev);
    bpp_ctx::RowsWork &w = ctx->rows;
    hipStream_t s = ctx->stream;
    const bool shared = in->point_stride == 0;
    const uint32_t K = in->K, kp = rows_kp(K);
    const size_t slab = std::min<size_t>(in->n, BPP_ROWS_SLAB);
    // (a buffer that grows is freed first: hipFree waits for the device, so what an earlier call enqueued has finished with it)
    bool first = enqueue_events_ensure(ctx);
    auto grow = [&](auto &buf, size_t count) {
      const void *before = buf.p;
      buf.alloc(count);
      first |= buf.p != before;
    };
    if (shared) {
      grow(w.base_tab, (size_t)BPP_ROWS_K_MAX * BPP_CTS_ENTRIES * 40);
      grow(w.bad, std::max<size_t>(BPP_ROWS_K_MAX, w.bad.n));
    } else {
      grow(w.pts, slab * K);
      grow(w.bad, std::max<size_t>(slab * K, BPP_ROWS_K_MAX));
    }
    a.pts = w.pts.p, a.bad = w.bad.p, a.base_tab = w.base_tab.p;
    w.stats.calls++;
    if (first) w.stats.first_calls++;
    if (record_dev) hipLaunchKernelGGL(k_rows_record_init, dim3(1), dim3(64), 0, s, record_dev);
    if (shared) hipLaunchKernelGGL(k_rows_bases, dim3(1), dim3(64), 0, s, a);
    for (size_t row0 = 0; row0 < in->n; row0 += slab) {
      a.row0 = (uint32_t)row0;
      a.rows = (uint32_t)std::min<size_t>(slab, in->n - row0);
      if (shared) {
        rows_msm_launch<true>(kp, a.rows, s, a);
      } else {
        hipLaunchKernelGGL(k_rows_decode, dim3((uint32_t)(((uint64_t)a.rows * K + 63) / 64)), dim3(64), 0, s, a);
        rows_msm_launch<false>(kp, a.rows, s, a);
      }
    }
    if (record_dev) hipLaunchKernelGGL(k_rows_record_finish, dim3(1), dim3(64), 0, s, record_dev);
    HIP_CHECK(hipGetLastError());
    const uint64_t t = enqueue_ticket_issue(ctx, s);
    if (ticket) *ticket = t;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

extern "C" int bpp_rows_scalar_enqueue(bpp_ctx *ctx, size_t n, const bpp_scalar_rows *a, const bpp_scalar_rows *b, const bpp_scalar_rows *c,
                                       uint8_t *out_dev, size_t out_stride, const uint8_t *live_dev, uint8_t *done_mask_dev,
                                       bpp_device_rows_record *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  try {
    const std::string why = rows_scalar_refusal(n, a, b, c, out_dev, out_stride, live_dev, done_mask_dev, record_dev);
    if (!why.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, why);
    if (const int rc = rows_pointer_kinds(ctx, {{"a.dev", a->dev}, {"b.dev", b->dev}, {"c.dev", c ? c->dev : nullptr}, {"out_dev", out_dev},
                                                {"live_dev", live_dev}, {"done_mask_dev", done_mask_dev}, {"record_dev", record_dev}}))
      return rc;
    RowsScalar r;
    rows_scalar_args(r, n, a, b, c, out_dev, out_stride, live_dev, done_mask_dev, record_dev);
    hipStream_t s = ctx->stream;
    const bool first = enqueue_events_ensure(ctx);
    ctx->rows.stats.calls++;
    if (first) ctx->rows.stats.first_calls++;
    if (record_dev) hipLaunchKernelGGL(k_rows_record_init, dim3(1), dim3(64), 0, s, record_dev);
    hipLaunchKernelGGL(k_rows_scalar, dim3(cdiv((uint32_t)n, 64)), dim3(64), 0, s, r);
    if (record_dev) hipLaunchKernelGGL(k_rows_record_finish, dim3(1), dim3(64), 0, s, record_dev);
    HIP_CHECK(hipGetLastError());
    const uint64_t t = enqueue_ticket_issue(ctx, s);
    if (ticket) *ticket = t;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

extern "C" int bpp_rows_stats(bpp_ctx *ctx, struct bpp_rows_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->rows.stats;
  return BPP_OK;
}
