// bpp_prove_submit / bpp_prove_collect: prove calls in flight from ONE thread and ONE context, the prover's form of
// bpp_verify_submit_packed / bpp_verify_collect (Pipeline / PipeLane / pipe_worker in engine.hip).
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
  bool done = false, collected = false;
};

struct ProveLane {
  bpp_ctx *child = nullptr;
  std::thread th;
  std::shared_ptr<ProveJob> job;  // posted by submit, taken by the worker
  bool busy = false;              // from the moment submit claims the lane until its job is done (not: collected)
};

struct ProvePipeline {
  std::mutex mu;  // lanes' state, tickets
  std::condition_variable cv;
  std::mutex submit_mu;  // one submit at a time: lanes are claimed in ticket order
  std::vector<std::unique_ptr<ProveLane>> lanes;
  std::map<uint64_t, std::shared_ptr<ProveJob>> tickets;
  // a number space of its own: bpp_verify_collect counts from 1 and never gets here, and a verify ticket is none of these
  uint64_t next_ticket = (1ull << 48) + 1;
  uint32_t next_lane = 0;
  bool quit = false;
};

namespace {

// the lane's call over the job's copy: what bpp_prove_batch_mixed / bpp_prove_openings do between BPP_ENTRY and the return
void prove_pipe_run(ProveLane *lane, ProveJob &job) {
  ScopeExit wipe_copy{[&] { job.copy.wipe(); }};  // on every way out: the witness bytes are not needed once the call has returned
  const size_t n = job.copy.items.size();
  if (n == 0) return;  // (nothing passed the check: the blocking call returns before any device work as well)
  bpp_ctx *c = lane->child;
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

void prove_pipe_worker(bpp_ctx *owner, ProvePipeline *pp, ProveLane *lane) {
  (void)hipSetDevice(owner->device);
  for (;;) {
    std::shared_ptr<ProveJob> job;
    {
      std::unique_lock<std::mutex> lk(pp->mu);
      pp->cv.wait(lk, [&] { return pp->quit || lane->job; });
      if (!lane->job) return;  // quit with nothing posted
      job = std::move(lane->job);
      lane->job.reset();
    }
    try {
      prove_pipe_run(lane, *job);
    } catch (const std::exception &e) {  // (an allocation of the merge itself: nothing may escape a worker)
      job->call_rc = BPP_ERR_ENGINE;
      job->call_msg = std::string("prove pipeline: ") + e.what();
    }
    {
      std::lock_guard<std::mutex> lk(pp->mu);
      job->done = true;
      lane->busy = false;  // the lane is free now: the results wait in the job
    }
    pp->cv.notify_all();
  }
}

ProvePipeline *prove_pipeline_get(bpp_ctx *ctx) {
  {
    std::lock_guard<std::mutex> lk(ctx->prove_pipe_init_mu);
    if (ctx->prove_pipe) return ctx->prove_pipe.get();
  }
  // the knobs of the caller's context as they are now hold on every lane (the self-check's tamper knobs stay behind).  Read
  // BEFORE the pipeline's own lock is taken: nothing takes the context's lock while it holds the pipeline's
  bpp_ctx::Options opt;
  {
    std::lock_guard<std::mutex> ck(ctx->mu);
    opt = ctx->opt;
  }
  std::lock_guard<std::mutex> lk(ctx->prove_pipe_init_mu);
  if (ctx->prove_pipe) return ctx->prove_pipe.get();  // (another thread's first submit was quicker)
  auto pp = std::make_shared<ProvePipeline>();
  for (uint32_t i = 0; i < ctx->prove_pipe_depth; i++) {
    auto lane = std::make_unique<ProveLane>();
    if (bpp_ctx_create(&lane->child, ctx->device) != BPP_OK) {
      for (auto &l : pp->lanes) bpp_ctx_destroy(l->child);
      throw EngineError{BPP_ERR_ENGINE, "prove pipeline lane: context creation failed"};
    }
    lane->child->opt = opt;
    pp->lanes.push_back(std::move(lane));
  }
  for (auto &lane : pp->lanes) lane->th = std::thread(prove_pipe_worker, ctx, pp.get(), lane.get());
  ctx->prove_pipe = std::move(pp);
  return ctx->prove_pipe.get();
}

std::shared_ptr<ProvePipeline> prove_pipeline_peek(bpp_ctx *ctx) {
  std::lock_guard<std::mutex> lk(ctx->prove_pipe_init_mu);
  return ctx->prove_pipe;
}

}  // namespace

void prove_pipeline_shutdown(bpp_ctx *ctx) {
  std::shared_ptr<ProvePipeline> pp;
  {
    std::lock_guard<std::mutex> lk(ctx->prove_pipe_init_mu);
    pp = std::move(ctx->prove_pipe);
    ctx->prove_pipe.reset();
  }
  if (!pp) return;
  {
    std::unique_lock<std::mutex> lk(pp->mu);
    pp->cv.wait(lk, [&] {  // jobs in flight finish first (every posted job runs, and its worker wipes its copy)
      for (auto &l : pp->lanes)
        if (l->busy) return false;
      return true;
    });
    pp->quit = true;
  }
  pp->cv.notify_all();
  for (auto &l : pp->lanes) {
    if (l->th.joinable()) l->th.join();
    bpp_ctx_destroy(l->child);
  }
  for (auto &kv : pp->tickets) kv.second->copy.wipe();  // results never collected are public; a copy still held is not
  pp->tickets.clear();
}

int prove_pipeline_check_stats(bpp_ctx *ctx, struct bpp_prove_check_stats *sum) {
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  if (!pp) return BPP_OK;
  for (auto &l : pp->lanes) {  // (the lanes are fixed once the pipeline exists)
    struct bpp_prove_check_stats s;
    const int rc = bpp_prove_check_stats(l->child, &s);
    if (rc != BPP_OK) return rc;
    sum->calls += s.calls;
    sum->proofs += s.proofs;
    sum->batch_failures += s.batch_failures;
    sum->remade += s.remade;
    sum->failed += s.failed;
  }
  return BPP_OK;
}

int prove_pipeline_recovery_stats(bpp_ctx *ctx, uint64_t *replayed, uint64_t *mismatched) {
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  if (!pp) return BPP_OK;
  for (auto &l : pp->lanes) {
    uint64_t r = 0, m = 0;
    const int rc = bpp_prove_check_recovery_stats(l->child, &r, &m);
    if (rc != BPP_OK) return rc;
    *replayed += r;
    *mismatched += m;
  }
  return BPP_OK;
}

int prove_pipeline_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero) {
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  if (!pp) return BPP_OK;
  for (auto &l : pp->lanes) {  // (waits for a lane's running call: its staging is looked at between calls)
    uint64_t seen = 0, cnt = 0;
    const int rc = bpp_prove_secret_bytes(l->child, &seen, &cnt);
    if (rc != BPP_OK) return rc;
    *examined += seen;
    *nonzero += cnt;
  }
  (void)hipSetDevice(ctx->device);
  return BPP_OK;
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
    ProvePipeline *pp = prove_pipeline_get(ctx);
    std::lock_guard<std::mutex> submit_lock(pp->submit_mu);
    ProveLane *lane;
    {
      std::unique_lock<std::mutex> lk(pp->mu);
      lane = pp->lanes[pp->next_lane].get();
      pp->cv.wait(lk, [&] { return !lane->busy; });  // its previous job is done (collected or not): arena and staging are free
      lane->busy = true;
      pp->next_lane = (pp->next_lane + 1) % (uint32_t)pp->lanes.size();
    }
    // the lane keeps the parameters alive for as long as it lives, whatever the caller does with its own reference
    int held = BPP_OK;
    if (!lane->child->held_params.count(params)) held = bpp_params_retain(lane->child, params);
    (void)hipSetDevice(ctx->device);
    if (held != BPP_OK) {
      {
        std::lock_guard<std::mutex> lk(pp->mu);
        lane->busy = false;
      }
      pp->cv.notify_all();
      return fail(nullptr, held, "unknown params handle", errbuf, errbuf_len);
    }
    {
      std::lock_guard<std::mutex> lk(pp->mu);
      job->ticket = pp->next_ticket++;
      pp->tickets[job->ticket] = job;
      lane->job = job;
      *ticket = job->ticket;
    }
    pp->cv.notify_all();
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
  std::lock_guard<std::mutex> lk(pp->mu);
  auto it = pp->tickets.find(ticket);
  if (it == pp->tickets.end()) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket");
  *done = it->second->done ? 1 : 0;
  return BPP_OK;
}

int bpp_prove_collect(bpp_ctx *ctx, uint64_t ticket, uint8_t *commitments_out, uint8_t *proofs_out, size_t *proof_lens, int *item_status,
                      char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  const std::shared_ptr<ProvePipeline> pp = prove_pipeline_peek(ctx);
  if (!pp) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);
  std::shared_ptr<ProveJob> job;
  {
    std::unique_lock<std::mutex> lk(pp->mu);
    auto it = pp->tickets.find(ticket);
    if (it == pp->tickets.end()) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);
    job = it->second;
    // (the blocking calls' "null argument": the ticket stays collectable)
    if (!proofs_out || !proof_lens || (job->openings && !commitments_out))
      return fail(nullptr, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    pp->cv.wait(lk, [&] { return job->done; });
    if (job->collected) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);  // (another thread was first)
    job->collected = true;
    pp->tickets.erase(ticket);
  }
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
