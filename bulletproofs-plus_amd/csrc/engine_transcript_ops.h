// Merlin on the stream (bpp_transcripts_enqueue, include/bpp.h): the engine's side of transcript_ops.h.  The refusals -- the
// arguments' own (transcript_ops_refusal) and the pointer kinds -- come before anything is counted or launched; then the launch
// arguments are made on the host (the labels copied, NEW's state computed once) and at most three launches go onto the context's
// stream: the record's init, k_transcript_ops (or k_transcript_ops_rng, where the program holds a transcript-protocol or transcript-RNG
// kind) over n blocks of one wavefront, the record's finish.  Nothing is allocated but the
// context's ticket events (once, where no enqueue made them), nothing is copied, nothing is waited for.
#pragma once

extern "C" int bpp_transcripts_enqueue(bpp_ctx *ctx, uint8_t *states203_dev, size_t n, const bpp_transcript_op *ops, size_t n_ops,
                                       const uint8_t *live_dev, uint8_t *done_mask_dev, bpp_device_transcripts_record *record_dev,
                                       uint64_t *ticket) {
  BPP_ENTRY(ctx);
  try {
    const std::string why = transcript_ops_refusal(states203_dev, n, ops, n_ops, live_dev, done_mask_dev, record_dev);
    if (!why.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, why);
    {
      std::vector<std::pair<std::string, const void *>> arrays = {
          {"states203_dev", states203_dev}, {"live_dev", live_dev}, {"done_mask_dev", done_mask_dev}, {"record_dev", record_dev}};
      for (size_t j = 0; j < n_ops; j++) {
        arrays.push_back({"ops[" + std::to_string(j) + "].data_dev", ops[j].data_dev});
        arrays.push_back({"ops[" + std::to_string(j) + "].lens_dev", ops[j].lens_dev});
      }
      for (const auto &a : arrays) {
        if (!a.second) continue;
        const int kind = device_pointer_kind(ctx->device, a.second);
        if (kind != BPP_PTR_THIS_DEVICE)
          return fail(ctx, BPP_ERR_INVALID_ARGUMENT, a.first + " is not device memory of this context's device (" + upload_pointer_kinds[kind] + ")");
      }
    }
    TranscriptOps a;
    transcript_ops_args(a, states203_dev, n, ops, n_ops, live_dev, done_mask_dev, record_dev);
    struct bpp_transcripts_stats &ts = ctx->tops_stats;
    hipStream_t s = ctx->stream;
    (void)enqueue_events_ensure(ctx);
    ts.calls++;
    if (ts.calls == 1) ts.first_calls++;
    if (record_dev) hipLaunchKernelGGL(k_transcript_record_init, dim3(1), dim3(64), 0, s, record_dev);
    // (the program's kinds are public: one that holds none of the transcript-protocol / RNG kinds runs the kernel without them)
    const bool extended = transcript_ops_extended(a);
    if (extended) hipLaunchKernelGGL(k_transcript_ops_rng, dim3((uint32_t)n), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_transcript_ops, dim3((uint32_t)n), dim3(64), 0, s, a);
    if (record_dev && extended) hipLaunchKernelGGL(k_transcript_record_finish_or, dim3(1), dim3(64), 0, s, record_dev);
    else if (record_dev) hipLaunchKernelGGL(k_transcript_record_finish, dim3(1), dim3(64), 0, s, record_dev);
    HIP_CHECK(hipGetLastError());
    const uint64_t t = enqueue_ticket_issue(ctx, s);
    if (ticket) *ticket = t;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

extern "C" int bpp_transcripts_stats(bpp_ctx *ctx, struct bpp_transcripts_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->tops_stats;
  return BPP_OK;
}
