// Stream-ordered proving from device arrays on a RESIDENT PLAN (bpp_prove_plan_create / bpp_prove_enqueue, include/bpp.h).
// bpp_prove_openings_device(_transcripts) does per call what depends on nothing but m[], the strides and which arrays are given: the
// per-item host checks, the sort, the layout, the arena, the staging of the public tables -- and then waits for the device three
// times over.  A plan does all of that ONCE and keeps it: a ProveCall (engine_prove.h) that lives as long as the plan, over an arena
// and a page-locked staging of the plan's own.  An enqueue runs the SAME stages -- enqueue_init / enqueue_step / enqueue_finish, launch
// for launch what the blocking call enqueues -- between a fork from the context's stream and a join back into it, and returns.
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
  std::vector<size_t> proof_lens;
  std::vector<uint32_t> msg;        // per item: the host's finding, 0 for an item that has a slot
  uint32_t n_refused = 0;
  DevBuf<uint8_t> refused;          // ProveDevRow x n_refused
  DevBuf<bpp_device_prove_status> outcome_item;
  PinnedBuf<uint8_t> pin;
  ProveDeviceIO io{};
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
    if (device_pointer_kind(ctx->device, shape->m) != BPP_PTR_HOST_OR_UNKNOWN)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m must be host memory: it sizes the call's layout", errbuf, errbuf_len);
    if (shape->m_stride == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m_stride is 0", errbuf, errbuf_len);
    if (ctx->opt.prove_check > 0)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT,
                  "prove_check = 1 is not supported by bpp_prove_openings_device: the self-check remakes from host items; verify the outputs "
                  "with bpp_verify_batch_mixed_device",
                  errbuf, errbuf_len);
    if (per_item && (shape->transcript_state || shape->transcript_label))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "transcript_state / transcript_label must be null: item i continues row i of item_states_dev",
                  errbuf, errbuf_len);
    if (shape->transcript_state && shape->transcript_state[200] >= BPP_STROBE_R)
      return fail(ctx, prove_err(BPP_PROVE_MSG_TRANSCRIPT_STATE).code, prove_msg_text(BPP_PROVE_MSG_TRANSCRIPT_STATE), errbuf, errbuf_len);
    std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    const size_t n_items = shape->n_items;
    if (n_items > (1u << 24)) return fail(ctx, BPP_ERR_SIZE_OVERFLOW, "batch too large", errbuf, errbuf_len);
    const ParamShape ps{Pp->n_bits, Pp->m_max, Pp->t};

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

    // the host's part of the checks, per item, as prove_openings_device runs it per call
    const bool fields_ok = shape->values && shape->blindings32 && shape->rng_bytes && (shape->min_values || !shape->min_present);
    pl.proof_lens.assign(n_items, 0);
    pl.msg.assign(n_items, BPP_PROVE_MSG_OK);
    std::map<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> classes;
    std::vector<ProveDevRow> refused;
    for (size_t i = 0; i < n_items; i++) {
      const uint32_t mi = pl.m[i];
      pl.proof_lens[i] = prove_item_len_host(ps, mi);
      pl.msg[i] = prove_item_layout_finding(ps, mi, proof_stride, true, commit_stride, fields_ok);
      if (!pl.msg[i] && mi > shape->m_stride)
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m_stride is below an aggregation factor", errbuf, errbuf_len);
      if (!pl.msg[i]) pl.msg[i] = prove_item_rng_finding(ps, mi, shape->rng_stride);
      if (!pl.msg[i]) {
        classes[mi].push_back((uint32_t)i);
        continue;
      }
      uint32_t zero = 0;
      if (pl.proof_lens[i] && proof_stride >= pl.proof_lens[i]) zero |= BPP_PROVE_ROW_ZERO_PROOF;
      if (pl.proof_lens[i] && commit_stride >= (size_t)32 * mi) zero |= BPP_PROVE_ROW_ZERO_COMMIT;
      refused.push_back(ProveDevRow{(uint32_t)i, mi, (uint32_t)pl.proof_lens[i], pl.msg[i], zero});
    }
    hipStream_t s = ctx->stream;
    pl.n_refused = (uint32_t)refused.size();
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
    for (auto &kv : classes)
      for (uint32_t i : kv.second) {
        pl.io.m_sorted.push_back(kv.first);
        pl.io.rows.push_back(
            ProveDevRow{i, kv.first, (uint32_t)pl.proof_lens[i], BPP_PROVE_MSG_OK, BPP_PROVE_ROW_ZERO_PROOF | BPP_PROVE_ROW_ZERO_COMMIT});
      }
    if (!pl.io.rows.empty()) {
      pl.req = ProveRequest{params, nullptr, pl.io.rows.size(), nullptr, 0, nullptr};
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
    proof_lens[i] = pl->proof_lens[i];
    if (host_status) host_status[i] = prove_msg_code(pl->msg[i]);
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
    static const char *const kinds[] = {"", "memory of another device", "host memory or memory the runtime does not know", "managed memory"};
    const struct {
      const char *name;
      const void *p;
    } arrays[] = {{"values", in_dev->values},
                  {"blindings32", in_dev->blindings32},
                  {"commitments32", in_dev->commitments32},
                  {"min_values", in_dev->min_values},
                  {"min_present", in_dev->min_present},
                  {"seed_nonces32", in_dev->seed_nonces32},
                  {"seed_present", in_dev->seed_present},
                  {"rng_bytes", in_dev->rng_bytes},
                  {"commitments_out_dev", commitments_out_dev},
                  {"proofs_out_dev", proofs_out_dev},
                  {"status_dev", status_dev},
                  {"item_states_dev", item_states_dev},
                  {"states_out_dev", states_out_dev},
                  {"live_dev", live_dev},
                  {"ok_mask_dev", ok_mask_dev},
                  {"summary_dev", summary_dev}};
    for (const auto &a : arrays) {
      if (!a.p) continue;
      const int kind = device_pointer_kind(ctx->device, a.p);
      if (kind != BPP_PTR_THIS_DEVICE)
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, std::string(a.name) + " is not device memory of this context's device (" + kinds[kind] + ")");
    }
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
    if (item_states_dev && states_out_dev) {
      const uintptr_t a = (uintptr_t)item_states_dev, b = (uintptr_t)states_out_dev;
      const uintptr_t len = (uintptr_t)pl.m.size() * BPP_ITEM_STATE_BYTES;
      if (a < b + len && b < a + len) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "item_states_dev and states_out_dev overlap");
    }

    // ---- the enqueue
    struct bpp_prove_enqueue_stats &es = ctx->prove_enq_stats;
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)pl.m.size();
    if (ctx->enq_events.empty()) {  // (the context's first ticket)
      ctx->enq_events.resize(64);
      for (auto &e : ctx->enq_events) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      es.allocations++;
    }
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
    if (pl.n_refused) {  // the refused items' records and zeroed slots, as in front of the blocking call
      ProveEmit e;
      memset(&e, 0, sizeof(e));
      e.rows = (const ProveDevRow *)pl.refused.p;
      e.n = pl.n_refused;
      e.proofs_out = proofs_out_dev;
      e.proof_stride = pl.proof_stride;
      e.commitments_out = commitments_out_dev;
      e.commit_stride = pl.commit_stride;
      e.status_dev = status_dev;
      e.states_out = states_out_dev;
      e.ok_mask = ok_mask_dev;
      e.outcome_item = pl.outcome_item.p;
      hipLaunchKernelGGL(k_prove_emit, dim3(cdiv(e.n, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, e);
      HIP_CHECK(hipGetLastError());
    }
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
    const uint64_t t = ctx->enq_next++;
    HIP_CHECK(hipEventRecord(ctx->enq_events[t % ctx->enq_events.size()], s));
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
