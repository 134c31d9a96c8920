// Stream-ordered proving from device arrays on a RESIDENT PLAN (bpp_prove_plan_create / bpp_prove_enqueue, include/bpp.h).
// bpp_prove_openings_device(_transcripts) does per call what depends on nothing but m[], the strides and which arrays are given: the
// per-item host checks, the sort, the layout, the arena, the staging of the public tables -- and then waits for the device three
// times over.  A plan does all of that ONCE and keeps it: the blocking call's whole-call refusals (prove_device_refusals,
// engine_prove.h) and its shape step (prove_device_shape, prove_ingest.h: the result stays in ProveDeviceIO::shape), then a ProveCall
// (engine_prove.h) that lives as long as the plan, over an arena and a page-locked staging of the plan's own.  An enqueue runs the
// SAME stages -- enqueue_init / enqueue_step / enqueue_finish, launch for launch what the blocking call enqueues -- between a fork
// from the context's stream and a join back into it, and returns.
//
// What differs from the blocking call, all of it in ProveCall behind `resident`:
//   - the tables (descriptors, rows, states) are copied from the plan's page-locked memory per enqueue: the arena range they land in
//     was zeroed by the previous enqueue's wipe on the same stream, and the copy also puts back bit 0 of ProveDesc::flags, which
//     k_prove_ingest sets.  The host never rewrites that memory.
//   - the outcome records go to a table in call order (outcome_item) outside the arena, for k_prove_summary behind the join; nothing
//     is copied to the host.
//   - the arena always has a state row per slot: whether an enqueue asks for the advanced transcripts is the enqueue's choice.
// The streams and events are the context's (a blocking prove call on the same context is ordered against the plan's work by them);
// the join events are the plan's.
//
// Hazards across enqueues of one plan, none of which needs the host: sub-batch q's arena range is written and wiped on lane stream q
// alone (its side and MSM streams are joined into the lane stream in front of kp_finish, as in every prove call), so enqueue k + 1's
// first write of the range is behind enqueue k's wipe in stream order.  outcome_item is written on the lane streams and read by
// k_prove_summary on the context's stream behind the join; enqueue k + 1's lane streams start behind its fork, which is behind that
// kernel.  The refused items' launch runs on the context's stream in front of the fork.
#pragma once

namespace {

struct ProvePlan : bpp_ctx::ProvePlanBase {
  std::shared_ptr<Params> P;
  uint64_t params = 0;
  uint32_t flags = 0;
  size_t commit_stride = 0, proof_stride = 0;
  // the shape: the caller's struct with m and the transcript pointing at the plan's copies; the device fields say "given" (non-null)
  // between enqueues and hold the caller's addresses during one
  bpp_prove_arrays arrays{};
  std::vector<uint32_t> m;
  std::vector<uint8_t> transcript;  // the 203-byte state or the label
  DevBuf<uint8_t> refused;          // io.shape.refused on the device
  DevBuf<bpp_device_prove_status> outcome_item;
  PinnedBuf<uint8_t> pin;
  ProveDeviceIO io{};               // (io.shape: the plan's proof lengths, host findings and tables, made once)
  ProveRequest req{};
  std::unique_ptr<ProveCall> call;  // null: the host refused every item
  std::vector<hipEvent_t> join;
  bool enqueued = false;

  ~ProvePlan() override {
    for (auto &e : join) (void)hipEventDestroy(e);
  }
};

ProvePlan *prove_plan_find(bpp_ctx *ctx, uint64_t handle) {
  auto it = ctx->prove_plans.find(handle);
  return it == ctx->prove_plans.end() ? nullptr : static_cast<ProvePlan *>(it->second.get());
}

// the optional arrays of a bpp_prove_arrays, by name: what a plan remembers as given or absent
struct ProveOptionalField {
  const char *name;
  const void *p;
};
std::array<ProveOptionalField, 5> prove_optional_fields(const bpp_prove_arrays &a) {
  return {{{"commitments32", a.commitments32},
           {"min_values", a.min_values},
           {"min_present", a.min_present},
           {"seed_nonces32", a.seed_nonces32},
           {"seed_present", a.seed_present}}};
}

// every stream the plan's call enqueued on, joined into the context's stream behind what is on it now
void prove_plan_join(bpp_ctx *ctx, ProvePlan &pl) {
  ProveCall &c = *pl.call;
  std::vector<hipStream_t> streams;
  for (uint32_t q = 0; q < c.n_sub; q++) {
    streams.push_back(c.lane_stream(q));
    if (c.prio) streams.push_back(ctx->prove_streams[q]);
    streams.push_back(ctx->prove_aux_streams[q]);
  }
  if (c.fifo) streams.push_back(ctx->prove_msm_stream);
  for (size_t k = 0; k < streams.size(); k++) {  // (pl.join holds one event per stream: made with the plan)
    HIP_CHECK(hipEventRecord(pl.join[k], streams[k]));
    HIP_CHECK(hipStreamWaitEvent(ctx->stream, pl.join[k], 0));
  }
}

}  // namespace

extern "C" int bpp_prove_plan_create(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *shape, size_t commit_stride, size_t proof_stride,
                                     uint32_t flags, uint64_t *plan, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  try {
    if (!shape || !plan) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    if (flags & ~BPP_PROVE_PLAN_ITEM_STATES) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "unknown flag", errbuf, errbuf_len);
    const bool per_item = (flags & BPP_PROVE_PLAN_ITEM_STATES) != 0;
    if (!shape->m || shape->n_items == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    // (the blocking call's refusals, its text for prove_check included)
    std::shared_ptr<Params> Pp;
    if (const int rc = prove_device_refusals(ctx, params, *shape, per_item, nullptr, nullptr, Pp, errbuf, errbuf_len)) return rc;
    const size_t n_items = shape->n_items;

    auto owned = std::make_unique<ProvePlan>();
    ProvePlan &pl = *owned;
    pl.P = Pp;
    pl.params = params;
    pl.flags = flags;
    pl.commit_stride = commit_stride;
    pl.proof_stride = proof_stride;
    pl.m.assign(shape->m, shape->m + n_items);
    pl.arrays = *shape;
    pl.arrays.m = pl.m.data();
    if (shape->transcript_state) {
      pl.transcript.assign(shape->transcript_state, shape->transcript_state + 203);
      pl.arrays.transcript_state = pl.transcript.data();
      pl.arrays.transcript_label = nullptr;
      pl.arrays.label_len = 0;
    } else if (shape->transcript_label) {
      pl.transcript.assign(shape->transcript_label, shape->transcript_label + shape->label_len);
      pl.transcript.push_back(0);  // (never empty: a zero-length label keeps a pointer that is not null)
      pl.arrays.transcript_label = pl.transcript.data();
    }

    // the host's part of the checks and the two tables: the shape step (prove_ingest.h), once for the plan's life
    const bool fields_ok = shape->values && shape->blindings32 && shape->rng_bytes && (shape->min_values || !shape->min_present);
    if (!prove_device_shape(ParamShape{Pp->n_bits, Pp->m_max, Pp->t}, pl.m.data(), n_items, shape->m_stride, shape->rng_stride, proof_stride,
                            commit_stride, fields_ok, pl.io.shape))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m_stride is below an aggregation factor", errbuf, errbuf_len);
    const std::vector<ProveDevRow> &refused = pl.io.shape.refused;
    hipStream_t s = ctx->stream;
    pl.outcome_item.alloc(n_items);
    HIP_CHECK(hipMemsetAsync(pl.outcome_item.p, 0, n_items * sizeof(bpp_device_prove_status), s));
    if (!refused.empty()) {
      pl.refused.alloc(refused.size() * sizeof(ProveDevRow));
      HIP_CHECK(hipMemcpyAsync(pl.refused.p, refused.data(), refused.size() * sizeof(ProveDevRow), hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));  // (the table is pageable memory of this frame; the one wait of a plan's life besides its arena's)

    pl.io.in = &pl.arrays;
    pl.io.commit_stride = commit_stride;
    pl.io.proof_stride = proof_stride;
    pl.io.per_item = per_item;
    pl.io.outcome_item = pl.outcome_item.p;
    if (!pl.io.shape.rows.empty()) {
      pl.req = ProveRequest{params, nullptr, pl.io.shape.rows.size(), nullptr, 0, nullptr};
      pl.req.mixed = true;
      pl.req.dev = &pl.io;
      pl.call.reset(new ProveCall(ctx, *pl.P, pl.req));
      ProveCall &c = *pl.call;
      c.resident = true;
      c.arena = &pl.arena;
      c.pin_in = &pl.pin;
      c.staging_clean = true;  // (no witness byte ever reaches the host or the staging)
      c.pack();
      c.plan();
      c.carve();
      c.ensure_fb_table();
      c.ensure_streams();
      c.stage_in();
      pl.join.resize((size_t)c.n_sub * 3 + 1);
      for (auto &e : pl.join) e = nullptr;
      for (auto &e : pl.join) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      if (!ctx->prove_dev_event) HIP_CHECK(hipEventCreateWithFlags(&ctx->prove_dev_event, hipEventDisableTiming));
    }
    const uint64_t h = ctx->prove_plan_next++;
    ctx->prove_plans[h] = std::move(owned);
    *plan = h;
    set_err(errbuf, errbuf_len, "");
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

extern "C" int bpp_prove_plan_shape(bpp_ctx *ctx, uint64_t plan, size_t *proof_lens, int *host_status) {
  BPP_ENTRY(ctx);
  ProvePlan *pl = prove_plan_find(ctx, plan);
  if (!pl) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown prove plan");
  if (!proof_lens) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  for (size_t i = 0; i < pl->m.size(); i++) {
    proof_lens[i] = pl->io.shape.proof_lens[i];
    if (host_status) host_status[i] = prove_msg_code(pl->io.shape.msg[i]);
  }
  return BPP_OK;
}

extern "C" int bpp_prove_plan_destroy(bpp_ctx *ctx, uint64_t plan) {
  BPP_ENTRY(ctx);
  if (!prove_plan_find(ctx, plan)) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown prove plan");
  (void)hipStreamSynchronize(ctx->stream);  // (every stream of the plan's enqueues is joined into it, behind the arena wipes)
  ctx->prove_plans.erase(plan);
  return BPP_OK;
}

extern "C" int bpp_prove_enqueue(bpp_ctx *ctx, uint64_t plan, const bpp_prove_arrays *in_dev, const uint8_t *item_states_dev,
                                 const uint8_t *live_dev, uint8_t *commitments_out_dev, uint8_t *proofs_out_dev, uint8_t *states_out_dev,
                                 bpp_device_prove_status *status_dev, uint8_t *ok_mask_dev, bpp_device_prove_summary *summary_dev,
                                 uint64_t *ticket) {
  BPP_ENTRY(ctx);
  try {
    ProvePlan *plp = prove_plan_find(ctx, plan);
    if (!plp) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown prove plan");
    ProvePlan &pl = *plp;
    if (!in_dev) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    // ---- the refusals: nothing is launched, nothing counted, no array dereferenced on the host
    if (!commitments_out_dev) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "commitments_out_dev is null");
    if (!proofs_out_dev) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "proofs_out_dev is null");
    const std::string why = prove_arrays_refusal(ctx, *in_dev, commitments_out_dev, proofs_out_dev, status_dev, item_states_dev, states_out_dev,
                                                 live_dev, ok_mask_dev, summary_dev);
    if (!why.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, why);
    const bool per_item = (pl.flags & BPP_PROVE_PLAN_ITEM_STATES) != 0;
    if (item_states_dev && !per_item)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "item_states_dev is given, but the plan was made without BPP_PROVE_PLAN_ITEM_STATES");
    if (!item_states_dev && per_item)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "item_states_dev is null, but the plan was made with BPP_PROVE_PLAN_ITEM_STATES");
    if (per_item && (in_dev->transcript_state || in_dev->transcript_label))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "transcript_state / transcript_label must be null: item i continues row i of item_states_dev");
    {
      const auto given = prove_optional_fields(*in_dev), planned = prove_optional_fields(pl.arrays);
      for (size_t k = 0; k < given.size(); k++)
        if ((given[k].p != nullptr) != (planned[k].p != nullptr))
          return fail(ctx, BPP_ERR_INVALID_ARGUMENT,
                      std::string(given[k].name) + (given[k].p ? " is given, but the plan was made without it" : " is null, but the plan was made with it"));
      const struct {
        const char *name;
        bool given, planned;
      } required[] = {{"values", in_dev->values != nullptr, pl.arrays.values != nullptr},
                      {"blindings32", in_dev->blindings32 != nullptr, pl.arrays.blindings32 != nullptr},
                      {"rng_bytes", in_dev->rng_bytes != nullptr, pl.arrays.rng_bytes != nullptr}};
      for (const auto &f : required)
        if (f.given != f.planned)
          return fail(ctx, BPP_ERR_INVALID_ARGUMENT,
                      std::string(f.name) + (f.given ? " is given, but the plan was made without it" : " is null, but the plan was made with it"));
    }
    if (in_dev->n_items != pl.arrays.n_items)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "n_items differs from the plan's (" + std::to_string(in_dev->n_items) + " != " + std::to_string(pl.arrays.n_items) + ")");
    if (in_dev->m_stride != pl.arrays.m_stride)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m_stride differs from the plan's (" + std::to_string(in_dev->m_stride) + " != " + std::to_string(pl.arrays.m_stride) + ")");
    if (in_dev->rng_stride != pl.arrays.rng_stride)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "rng_stride differs from the plan's (" + std::to_string(in_dev->rng_stride) + " != " + std::to_string(pl.arrays.rng_stride) + ")");
    if (in_dev->m) {
      if (device_pointer_kind(ctx->device, in_dev->m) != BPP_PTR_HOST_OR_UNKNOWN)
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m must be host memory (or null: the plan's own)");
      for (size_t i = 0; i < pl.m.size(); i++)
        if (in_dev->m[i] != pl.m[i])
          return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m[" + std::to_string(i) + "] differs from the plan's (" + std::to_string(in_dev->m[i]) + " != " + std::to_string(pl.m[i]) + ")");
    }
    if (prove_states_overlap(item_states_dev, states_out_dev, pl.m.size()))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "item_states_dev and states_out_dev overlap");

    // ---- the enqueue
    struct bpp_prove_enqueue_stats &es = ctx->prove_enq_stats;
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)pl.m.size();
    if (enqueue_events_ensure(ctx)) es.allocations++;  // (the context's first ticket)
    es.calls++;
    if (!pl.enqueued) es.first_calls++;
    pl.enqueued = true;
    // the caller's addresses for this enqueue; m and the transcript stay the plan's
    bpp_prove_arrays &A = pl.arrays;
    A.values = in_dev->values, A.blindings32 = in_dev->blindings32, A.commitments32 = in_dev->commitments32;
    A.min_values = in_dev->min_values, A.min_present = in_dev->min_present;
    A.seed_nonces32 = in_dev->seed_nonces32, A.seed_present = in_dev->seed_present, A.rng_bytes = in_dev->rng_bytes;
    pl.io.commitments_out = commitments_out_dev;
    pl.io.proofs_out = proofs_out_dev;
    pl.io.status_dev = status_dev;
    pl.io.item_states = item_states_dev;
    pl.io.states_out = states_out_dev;
    pl.io.live = live_dev;
    pl.io.ok_mask = ok_mask_dev;
    // the refused items' records and zeroed slots, as in front of the blocking call; the table is the plan's and stays resident
    if (const size_t n_refused = pl.io.shape.refused.size()) launch_prove_refused(s, (const ProveDevRow *)pl.refused.p, (uint32_t)n_refused, pl.io);
    if (pl.call) {
      ProveCall &c = *pl.call;
      c.ev_used = 0;
      c.arena_clean = false;
      try {
        c.fork_from_ctx();
        for (uint32_t q = 0; q < c.n_sub; q++) c.enqueue_init(q);
        for (uint32_t j = 0; j <= c.rounds; j++)
          for (uint32_t q = 0; q < c.n_sub; q++) c.enqueue_step(j, q);
        for (uint32_t q = 0; q < c.n_sub; q++) c.enqueue_finish(q);
        HIP_CHECK(hipGetLastError());
        prove_plan_join(ctx, pl);
      } catch (...) {  // a HIP error: whatever reached the arena is wiped before the call returns -- the one path that waits
        es.host_waits++;
        c.wipe_secrets();
        c.arena_clean = true;
        throw;
      }
      c.arena_clean = true;  // (zeroed on the streams, which the context's stream now waits for)
    }
    if (summary_dev) {
      hipLaunchKernelGGL(k_prove_summary, dim3(1), dim3(BPP_PROVE_SUMMARY_BLOCK), 0, s, (const bpp_device_prove_status *)pl.outcome_item.p, n,
                         summary_dev);
      HIP_CHECK(hipGetLastError());
    }
    const uint64_t t = enqueue_ticket_issue(ctx, s);
    if (ticket) *ticket = t;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

extern "C" int bpp_prove_summary_result(const bpp_device_prove_summary *host_copy, bpp_shard_result *out) {
  if (!host_copy || !out || !(host_copy->flags & BPP_PROVE_SUMMARY_WRITTEN) || host_copy->msg > BPP_PROVE_MSG_ENGINE) return BPP_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  shard_result_set(*out, host_copy->code, host_copy->msg ? BPP_TIER_CONSTRUCTION : BPP_TIER_NONE, -1, host_copy->index, prove_msg_text(host_copy->msg));
  return BPP_OK;
}

extern "C" int bpp_prove_enqueue_stats(bpp_ctx *ctx, struct bpp_prove_enqueue_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->prove_enq_stats;
  return BPP_OK;
}
