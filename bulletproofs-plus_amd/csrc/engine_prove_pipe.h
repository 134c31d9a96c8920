// bpp_prove_submit / bpp_prove_collect: prove calls in flight from ONE thread and ONE context, the prover's form of
// bpp_verify_submit_packed / bpp_verify_collect (engine.hip), over the same tickets-and-lanes protocol (lanes::TicketLanes).
//
// One context, `depth` lanes.  A lane is a private child context (the prover's streams, arena and page-locked staging of its own)
// plus a worker thread.  submit checks every item ON THE CALLING THREAD (prove_item_check, as prove_mixed does), takes a copy of
// the ones that pass -- everything they point to, ProveJobCopy in prove_job_host.h -- and hands the job to the lane whose turn it
// is; the caller's buffers are free when submit returns.  The lane's worker runs prove_mixed over the copy on the lane's context,
// merges the device's outcomes with those of the check into the caller's order, and wipes the copy.  collect hands out exactly
// what bpp_prove_batch_mixed / bpp_prove_openings over the same items return: bytes, lengths, statuses, zeroed slots, code, message.
// No kernel of its own: the device work is prove_uniform's, launched as a blocking call launches it.
// Part of engine.hip's translation unit.
#pragma once

struct ProveJob {
  uint64_t ticket = 0;
  uint64_t params = 0;
  std::shared_ptr<Params> Pp;
  bool openings = false;
  size_t n_items = 0, proof_stride = 0, commit_stride = 0;
  ProveJobCopy copy;  // the items that passed the check, and every item's outcome so far
  // results, in the caller's order, in rows of the job's own (the parameters' longest proof, 32 * m_max commitment bytes): the
  // caller's strides are applied when they are collected
  size_t row = 0, crow = 0;
  std::vector<uint8_t> proofs, commits;
  int call_rc = BPP_OK;  // a finding of the whole call (an exception of the lane's prove_mixed): collect returns it and writes nothing
  std::string call_msg;
  std::vector<std::array<uint8_t, 32>> note;  // what the lane's call left for bpp_prove_item_message (check_recovery_failed)
  bool done = false;
};

// (tickets in a number space of its own: bpp_verify_collect counts from 1 and never gets here, and a verify ticket is none of these)
static const uint64_t PROVE_FIRST_TICKET = (1ull << 48) + 1;

namespace {

// the lane's call over the job's copy: what bpp_prove_batch_mixed / bpp_prove_openings do between BPP_ENTRY and the return
void prove_pipe_run(bpp_ctx *&c, ProveJob &job) {
  ScopeExit wipe_copy{[&] { job.copy.wipe(); }};  // on every way out: the witness bytes are not needed once the call has returned
  const size_t n = job.copy.items.size();
  if (n == 0) return;  // (nothing passed the check: the blocking call returns before any device work as well)
  std::vector<uint8_t> proofs(n * job.row, 0), commits(job.openings ? n * job.crow : 0, 0);
  std::vector<size_t> lens(n, 0);
  std::vector<uint8_t *> slots(job.openings ? n : 0);
  for (size_t k = 0; k < slots.size(); k++) slots[k] = commits.data() + k * job.crow;
  const std::vector<size_t> caps(slots.size(), job.crow);
  MixedOutcome out;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    try {
      if (hipSetDevice(c->device) != hipSuccess) throw EngineError{BPP_ERR_NO_DEVICE, "hipSetDevice failed"};
      prove_mixed(c, job.params, job.copy.items.data(), n, proofs.data(), job.row, lens.data(), out, job.openings ? &slots : nullptr,
                  job.openings ? &caps : nullptr);
    } catch (const EngineError &e) {
      job.call_rc = fail(c, e.code, e.msg);
      job.call_msg = e.msg;
    } catch (const ProofErr &e) {
      job.call_rc = fail(c, e.code, e.msg);
      job.call_msg = e.msg;
    } catch (const std::exception &e) {
      job.call_rc = fail(c, BPP_ERR_ENGINE, e.what());
      job.call_msg = e.what();
    }
    std::lock_guard<std::mutex> nk(c->check_note_mu);
    job.note = c->check_recovery_failed;
  }
  if (job.call_rc != BPP_OK) return;
  for (size_t k = 0; k < n; k++) {  // into the caller's order, beside what the check found at submit
    const size_t i = job.copy.index[k];
    job.copy.code[i] = out.code[k];
    job.copy.msg[i] = out.msg[k];
    if (out.code[k] != BPP_OK) continue;
    memcpy(&job.proofs[i * job.row], &proofs[k * job.row], lens[k]);
    if (job.openings) memcpy(&job.commits[i * job.crow], &commits[k * job.crow], (size_t)32 * job.copy.m[i]);
  }
}

void prove_pipe_threw(ProveJob &job, const char *what) {  // (an allocation of the merge itself: nothing escapes a worker)
  job.call_rc = BPP_ERR_ENGINE;
  job.call_msg = std::string("prove pipeline: ") + (what ? what : "unexpected failure");
}

std::shared_ptr<ProvePipeline> prove_pipeline_get(bpp_ctx *ctx) {
  return pipeline_get(ctx, ctx->prove_pipe_init_mu, ctx->prove_pipe, ctx->prove_pipe_depth, "prove pipeline lane: context creation failed",
                      [](std::vector<bpp_ctx *> children) {
                        return std::make_shared<ProvePipeline>(std::move(children), PROVE_FIRST_TICKET, prove_pipe_run, prove_pipe_threw);
                      });
}

std::shared_ptr<ProvePipeline> prove_pipeline_peek(bpp_ctx *ctx) { return pipeline_peek(ctx->prove_pipe_init_mu, ctx->prove_pipe); }

// the sum over the lanes of what `one(lane's context)` answers; the first code that is not BPP_OK ends it
template <class F>
int prove_pipeline_sum(bpp_ctx *ctx, F one) {
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  int rc = BPP_OK;
  if (pp)
    pp->for_each_lane([&](bpp_ctx *c) {
      if (rc == BPP_OK) rc = one(c);
    });
  return rc;
}

}  // namespace

void prove_pipeline_shutdown(bpp_ctx *ctx) {
  // (every posted job has run, and its worker has wiped its copy; results never collected are public, a copy still held is not)
  pipeline_end(ctx->prove_pipe_init_mu, ctx->prove_pipe, [](ProveJob &job) { job.copy.wipe(); });
}

int prove_pipeline_check_stats(bpp_ctx *ctx, struct bpp_prove_check_stats *sum) {
  return prove_pipeline_sum(ctx, [&](bpp_ctx *c) { return add_check_stats(c, *sum); });
}

int prove_pipeline_recovery_stats(bpp_ctx *ctx, uint64_t *replayed, uint64_t *mismatched) {
  return prove_pipeline_sum(ctx, [&](bpp_ctx *c) { return add_recovery_stats(c, *replayed, *mismatched); });
}

int prove_pipeline_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero) {
  // (waits for a lane's running call: its staging is looked at between calls)
  const int rc = prove_pipeline_sum(ctx, [&](bpp_ctx *c) {
    uint64_t seen = 0, cnt = 0;
    const int one = bpp_prove_secret_bytes(c, &seen, &cnt);
    if (one == BPP_OK) {
      *examined += seen;
      *nonzero += cnt;
    }
    return one;
  });
  if (rc == BPP_OK) (void)hipSetDevice(ctx->device);
  return rc;
}

extern "C" {

int bpp_prove_pipeline_depth(bpp_ctx *ctx, uint32_t depth) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  std::lock_guard<std::mutex> lk(ctx->prove_pipe_init_mu);
  if (ctx->prove_pipe) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "the prove pipeline is already running");
  if (depth < 1 || depth > 8) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "prove pipeline depth must be 1..8");
  ctx->prove_pipe_depth = depth;
  return BPP_OK;
}

int bpp_prove_submit(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, size_t proof_stride, int openings,
                     size_t commit_stride, uint64_t *ticket, char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  if (hipSetDevice(ctx->device) != hipSuccess) return BPP_ERR_NO_DEVICE;
  try {
    // (the findings of the whole call that need no look at an item, in prove_mixed's order and words)
    const std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    if (!items || n_items == 0 || !ticket) return fail(nullptr, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    auto job = std::make_shared<ProveJob>();
    job->params = params;
    job->Pp = Pp;
    job->openings = openings != 0;
    job->n_items = n_items;
    job->proof_stride = proof_stride;
    job->commit_stride = job->openings ? commit_stride : 0;
    const ParamShape shape{Pp->n_bits, Pp->m_max, Pp->t};
    job->copy.take(shape, items, n_items, proof_stride, job->openings, job->commit_stride);  // nothing of the caller's is read after this
    job->row = prove_item_len(*Pp, Pp->m_max);
    job->crow = (size_t)32 * Pp->m_max;
    job->proofs.assign(n_items * job->row, 0);
    if (job->openings) job->commits.assign(n_items * job->crow, 0);
    const std::shared_ptr<ProvePipeline> pp = prove_pipeline_get(ctx);
    ProvePipeline::Claim lane = pp->claim();  // its previous job is done (collected or not): arena and staging are free
    // the lane keeps the parameters alive for as long as it lives, whatever the caller does with its own reference
    int held = BPP_OK;
    if (!lane.lane()->held_params.count(params)) held = bpp_params_retain(lane.lane(), params);
    (void)hipSetDevice(ctx->device);
    if (held != BPP_OK) return fail(nullptr, held, "unknown params handle", errbuf, errbuf_len);  // (the claim gives the lane back)
    *ticket = pp->post(lane, job);
    set_err(errbuf, errbuf_len, "");
    return BPP_OK;
  }
  BPP_CATCH(nullptr, errbuf, errbuf_len)
}

int bpp_prove_ticket_done(bpp_ctx *ctx, uint64_t ticket, int *done) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  if (!done) return BPP_ERR_INVALID_ARGUMENT;
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  if (!pp) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket");
  const lanes::TicketState st = pp->done(ticket);
  if (st == lanes::TicketState::unknown) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket");
  *done = st == lanes::TicketState::done ? 1 : 0;
  return BPP_OK;
}

int bpp_prove_collect(bpp_ctx *ctx, uint64_t ticket, uint8_t *commitments_out, uint8_t *proofs_out, size_t *proof_lens, int *item_status,
                      char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  if (!pp) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);
  std::shared_ptr<ProveJob> job = pp->peek(ticket);
  if (!job) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);
  // (the blocking calls' "null argument": the ticket stays collectable)
  if (!proofs_out || !proof_lens || (job->openings && !commitments_out))
    return fail(nullptr, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  job = pp->take(ticket);
  if (!job) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);  // (another thread was first)
  {  // asking this context about an item right after the collect answers for this ticket (bpp_prove_item_message)
    std::lock_guard<std::mutex> lk(ctx->check_note_mu);
    ctx->check_recovery_failed = job->note;
  }
  if (job->call_rc != BPP_OK) return fail(nullptr, job->call_rc, job->call_msg, errbuf, errbuf_len);
  const ProveJobCopy &c = job->copy;
  for (size_t i = 0; i < job->n_items; i++) {
    proof_lens[i] = c.len[i];
    uint8_t *slot = proofs_out + i * job->proof_stride;
    uint8_t *cslot = job->openings ? commitments_out + i * job->commit_stride : nullptr;
    const size_t cbytes = (size_t)32 * c.m[i];
    if (c.code[i] == BPP_OK) {
      memcpy(slot, &job->proofs[i * job->row], c.len[i]);
      if (cslot) memcpy(cslot, &job->commits[i * job->crow], cbytes);
    } else if (c.len[i]) {  // a failed item's slots are zeroed where they can hold it (prove_mixed's last two loops)
      if (job->proof_stride >= c.len[i]) memset(slot, 0, c.len[i]);
      if (cslot && job->commit_stride >= cbytes) memset(cslot, 0, cbytes);
    }
  }
  if (item_status) memcpy(item_status, c.code.data(), job->n_items * sizeof(int));
  for (size_t i = 0; i < job->n_items; i++)
    if (c.code[i] != BPP_OK) return fail(nullptr, c.code[i], c.msg[i], errbuf, errbuf_len);
  set_err(errbuf, errbuf_len, "");
  return BPP_OK;
}

}  // extern "C"
