// bpp_prove_pool: pools the small prove calls of many host threads (a wallet service or an exchange making outputs) into
// mixed-aggregation engine calls.
//
// Why: a call of one proof is a chain of latency-bound launches (kp_init, kp_A, a round kernel and a fixed-base MSM per round,
// the final step) that the chip runs in about the time a call of a few hundred proofs takes.  The pool gives separate callers
// the second form, the way bpp_batcher does for verify_batch: every caller hands over its items (any aggregation factors;
// bpp_prove_pool_prove blocks until its proofs are there); whichever caller finds a lane free leads the next pooled call, takes
// what queued up while the previous pooled calls ran (plus what arrives within max_wait_us), proves everybody's items as ONE
// bpp_prove_batch_mixed on the lane's context and hands every caller its own proofs and outcome.  No thread of its own.
// Each caller gets exactly what bpp_prove_batch_mixed(ctx, params, its items, ...) would have returned: a proof depends on its
// own item alone and every item carries its own outcome, so nobody else's items change a caller's bytes, status or message.
// The lanes keep copies of the callers' item DESCRIPTORS only (pointers into the callers' buffers); the witness bytes, nonces
// and the page-locked staging that held them are wiped by the prover itself before the engine call returns.
// Part of engine.hip's translation unit.
#pragma once

struct bpp_prove_pool {
  struct Req : lanes::PoolReq {
    const bpp_prove_item *items = nullptr;
    size_t n_items = 0;
    uint8_t *proofs_out = nullptr;
    size_t proof_stride = 0;
    size_t *proof_lens = nullptr;
    // bpp_prove_pool_openings: the request's items may come without commitments, and every successful item's go to
    // commitments_out + i * commit_stride (bpp_prove_openings).  Requests of both kinds share pooled calls.
    bool openings = false;
    uint8_t *commitments_out = nullptr;
    size_t commit_stride = 0;
    int code = BPP_OK;
    std::string msg;
  };
  struct Lane {
    bpp_ctx *ctx = nullptr;  // a context of its own (streams, arena, staging)
    bool own = false;
    std::vector<bpp_prove_item> items;
    std::vector<uint8_t> proofs;
    std::vector<size_t> lens;
    std::vector<uint8_t *> commit_slots;  // per item of the pooled call: into its caller's commitments_out, or null (prove_mixed)
    std::vector<size_t> commit_caps;
  };
  uint64_t params = 0;
  std::shared_ptr<Params> P;
  size_t plen_max = 0;  // the longest proof these parameters can make (m = m_max): the lanes' output stride
  lanes::LeaderPool<Lane, Req> pool;  // the leader protocol (lanes_host.h); a request's weight is its number of proofs
  std::atomic<uint64_t> openings_calls{0}, both_kinds_calls{0};  // requests of bpp_prove_pool_openings; pooled engine calls that held both kinds
  bpp_prove_pool(std::vector<Lane> lanes, uint32_t max_wait_us, uint32_t max_calls) : pool(std::move(lanes), max_wait_us, max_calls, 4096) {}
};

namespace {

// A call of more than max_proofs items is a large call by itself, and one whose stride is too short for one of its proofs, or
// whose arguments are missing, gets its answer from a call of its own: all go through bpp_prove_batch_mixed (bpp_prove_openings
// for a request of that kind) directly.
bool prove_pool_poolable(const bpp_prove_pool *p, uint32_t max_proofs, const bpp_prove_pool::Req *r) {
  if (r->openings && !r->commitments_out) return false;
  if (!r->items || r->n_items == 0 || !r->proofs_out || !r->proof_lens || r->n_items > max_proofs) return false;
  for (size_t i = 0; i < r->n_items; i++)
    if (r->proof_stride < prove_item_len(*p->P, r->items[i].m)) return false;
  return true;
}

void prove_pool_solo(bpp_prove_pool *p, bpp_prove_pool::Lane &L, bpp_prove_pool::Req *r) {
  char err[256];
  err[0] = 0;
  if (r->openings)
    r->code = bpp_prove_openings(L.ctx, p->params, r->items, r->n_items, r->commitments_out, r->commit_stride, r->proofs_out,
                                 r->proof_stride, r->proof_lens, nullptr, err, sizeof(err));
  else
    r->code = bpp_prove_batch_mixed(L.ctx, p->params, r->items, r->n_items, r->proofs_out, r->proof_stride, r->proof_lens, nullptr, err,
                                    sizeof(err));
  r->msg = err;
}

// one pooled engine call on `lane` over `reqs`; fills every request's code / msg (nothing may escape: callers are waiting)
void prove_pool_run(bpp_prove_pool *p, bpp_prove_pool::Lane &L, const std::vector<bpp_prove_pool::Req *> &reqs) {
  ScopeExit clear_lane{[&] { L.items.clear(); }};
  if (reqs.size() == 1) {
    prove_pool_solo(p, L, reqs[0]);
    return;
  }
  try {
    size_t n = 0;
    for (auto *r : reqs) n += r->n_items;
    L.items.resize(n);
    L.lens.assign(n, 0);
    L.proofs.resize(n * p->plen_max);
    L.commit_slots.assign(n, nullptr);
    L.commit_caps.assign(n, 0);
    size_t at = 0;
    bool any_openings = false, any_without = false;
    for (auto *r : reqs) {
      any_without = any_without || !r->openings;
      std::copy(r->items, r->items + r->n_items, L.items.begin() + (ptrdiff_t)at);
      for (size_t i = 0; r->openings && i < r->n_items; i++) {
        L.commit_slots[at + i] = r->commitments_out + i * r->commit_stride;
        L.commit_caps[at + i] = r->commit_stride;
        any_openings = true;
      }
      at += r->n_items;
    }
    if (any_openings && any_without) p->both_kinds_calls++;
    MixedOutcome out;
    {
      std::lock_guard<std::mutex> lk(L.ctx->mu);
      if (hipSetDevice(L.ctx->device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
      prove_mixed(L.ctx, p->params, L.items.data(), n, L.proofs.data(), p->plen_max, L.lens.data(), out,
                  any_openings ? &L.commit_slots : nullptr, any_openings ? &L.commit_caps : nullptr);
    }
    // fan out: a caller's outcome is its first failing item's (bpp_prove_batch_mixed's return value and message).  An engine fault
    // (a negative code: an allocation the pooled call needed, a HIP error) is nobody's input: the callers it hit get a call of their own.
    // BPP_ERR_SELF_CHECK is an item's own outcome, after its one remake: it is handed on like a finding.
    at = 0;
    for (auto *r : reqs) {
      bool fault = false;
      for (size_t i = 0; i < r->n_items; i++) fault = fault || (out.code[at + i] < 0 && out.code[at + i] != BPP_ERR_SELF_CHECK);
      if (fault) {
        prove_pool_solo(p, L, r);
        at += r->n_items;
        continue;
      }
      r->code = BPP_OK;
      r->msg.clear();
      for (size_t i = 0; i < r->n_items; i++) {
        const size_t g = at + i, len = L.lens[g];
        r->proof_lens[i] = len;
        if (len) memcpy(r->proofs_out + i * r->proof_stride, &L.proofs[g * p->plen_max], len);
        if (out.code[g] != BPP_OK && r->code == BPP_OK) {
          r->code = out.code[g];
          r->msg = out.msg[g];
        }
      }
      at += r->n_items;
    }
  } catch (const EngineError &e) {  // an engine fault should not be pinned on all of them: everybody gets a call of their own
    for (auto *r : reqs) prove_pool_solo(p, L, r);
  } catch (const ProofErr &e) {
    for (auto *r : reqs) prove_pool_solo(p, L, r);
  } catch (const std::exception &e) {
    fail_requests(reqs, std::string("prove pool: ") + e.what());
  } catch (...) {
    fail_requests(reqs, "prove pool: unexpected failure");
  }
}

}  // namespace

extern "C" {

int bpp_prove_pool_create(bpp_ctx *ctx, uint64_t params, uint32_t lanes, uint32_t max_wait_us, uint32_t max_calls, bpp_prove_pool **out) {
  if (!ctx || !out) return BPP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const std::shared_ptr<Params> Pp = params_registry().get(params);
  if (!Pp || Pp->device != ctx->device) return BPP_ERR_BAD_HANDLE;
  if (lanes == 0) lanes = 2;
  if (lanes > 8) lanes = 8;
  std::vector<bpp_prove_pool::Lane> made;
  // the knobs of the caller's context, as they are when the pool is made, hold on every lane
  const int rc = make_pool_lanes(ctx, params, lanes, [](bpp_ctx *c, const bpp_ctx::Options &opt) { c->opt = opt; }, made);
  if (rc != BPP_OK) return rc;
  auto p = std::make_unique<bpp_prove_pool>(std::move(made), max_wait_us, max_calls ? max_calls : 64);
  p->params = params;
  p->P = Pp;
  p->plen_max = prove_item_len(*Pp, Pp->m_max);
  *out = p.release();
  return BPP_OK;
}

int bpp_prove_pool_set_limits(bpp_prove_pool *p, uint32_t max_calls, uint32_t max_proofs) {
  if (!p) return BPP_ERR_BAD_HANDLE;
  p->pool.set_limits(max_calls, max_proofs);
  return BPP_OK;
}

int bpp_prove_pool_stats(bpp_prove_pool *p, uint64_t *pooled_calls, uint64_t *engine_calls, uint64_t *solo_calls, uint32_t *largest_calls,
                         uint32_t *largest_proofs) {
  if (!p) return BPP_ERR_BAD_HANDLE;
  const lanes::PoolStats s = p->pool.stats();
  if (pooled_calls) *pooled_calls = s.pooled_calls;
  if (engine_calls) *engine_calls = s.engine_calls;
  if (solo_calls) *solo_calls = s.solo_calls;
  if (largest_calls) *largest_calls = s.largest_pool_calls;
  if (largest_proofs) *largest_proofs = s.largest_pool_weight;
  return BPP_OK;
}

int bpp_prove_pool_check_stats(bpp_prove_pool *p, struct bpp_prove_check_stats *out) {
  if (!p || !out) return BPP_ERR_BAD_HANDLE;
  memset(out, 0, sizeof(*out));
  int rc = BPP_OK;
  p->pool.for_each_lane([&](bpp_prove_pool::Lane &L) { rc = rc == BPP_OK ? add_check_stats(L.ctx, *out) : rc; });
  return rc;
}

int bpp_prove_pool_check_recovery_stats(bpp_prove_pool *p, uint64_t *replayed, uint64_t *mismatched) {
  if (!p) return BPP_ERR_BAD_HANDLE;
  uint64_t r = 0, m = 0;
  int rc = BPP_OK;
  p->pool.for_each_lane([&](bpp_prove_pool::Lane &L) { rc = rc == BPP_OK ? add_recovery_stats(L.ctx, r, m) : rc; });
  if (rc != BPP_OK) return rc;
  if (replayed) *replayed = r;
  if (mismatched) *mismatched = m;
  return BPP_OK;
}

void bpp_prove_pool_destroy(bpp_prove_pool *p) {
  if (!p) return;
  p->pool.drain();
  p->pool.for_each_lane([](bpp_prove_pool::Lane &L) {
    if (L.own) bpp_ctx_destroy(L.ctx);
  });
  delete p;
}

}  // extern "C"

namespace {
// one request through the pool: blocks until its outcome is there.  `openings`: the request's items may come without commitments
int prove_pool_submit(bpp_prove_pool *p, bool openings, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out, size_t commit_stride,
                      uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, char *errbuf, size_t errbuf_len) {
  if (!p) return BPP_ERR_BAD_HANDLE;
  bpp_prove_pool::Req me;
  me.items = items;
  me.n_items = n_items;
  me.proofs_out = proofs_out;
  me.proof_stride = proof_stride;
  me.proof_lens = proof_lens;
  me.openings = openings;
  me.commitments_out = commitments_out;
  me.commit_stride = commit_stride;
  if (openings) p->openings_calls++;
  p->pool.serve(
      me, [&](uint32_t max_proofs) { return prove_pool_poolable(p, max_proofs, &me); }, [](const bpp_prove_pool::Req &r) { return r.n_items; },
      [](const bpp_prove_pool::Req &, const bpp_prove_pool::Req &) { return true; },
      [&](bpp_prove_pool::Lane &L, const std::vector<bpp_prove_pool::Req *> &reqs) { prove_pool_run(p, L, reqs); });
  set_err(errbuf, errbuf_len, me.msg);
  return me.code;
}
}  // namespace

extern "C" {

int bpp_prove_pool_prove(bpp_prove_pool *p, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out, size_t proof_stride,
                         size_t *proof_lens, char *errbuf, size_t errbuf_len) {
  return prove_pool_submit(p, false, items, n_items, nullptr, 0, proofs_out, proof_stride, proof_lens, errbuf, errbuf_len);
}

int bpp_prove_pool_openings(bpp_prove_pool *p, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out, size_t commit_stride,
                            uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, char *errbuf, size_t errbuf_len) {
  return prove_pool_submit(p, true, items, n_items, commitments_out, commit_stride, proofs_out, proof_stride, proof_lens, errbuf, errbuf_len);
}

int bpp_prove_pool_openings_stats(bpp_prove_pool *p, uint64_t *openings_calls, uint64_t *both_kinds_calls) {
  if (!p) return BPP_ERR_BAD_HANDLE;
  if (openings_calls) *openings_calls = p->openings_calls.load();
  if (both_kinds_calls) *both_kinds_calls = p->both_kinds_calls.load();
  return BPP_OK;
}

}  // extern "C"
