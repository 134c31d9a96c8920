// Host side of the mixed form of ingest.h (bpp_batch_upload_mixed_device): the prelude in front of the run, which makes the table of
// IngestMixedRow the kernel packs by, and the plan behind it.  Pure host C++ over upload_host.h.  Shared by the engine's driver
// (engine.hip: upload_device_form) and by the sanitizer harness (hosttest_ingest_mixed.cpp), which holds prelude + ingest_run_host<true> + plan to
// upload_pass_a + upload_pass_b over item views of the same rows.
//
// Split of the checks (lowest-index construction finding wins, as in upload_run_parts):
//   host, no proof byte needed: the geometry (upload_mixed_geometry), pass A's size limits on the running sums, and per item what
//     upload_check_item raises before it reads a byte (upload_check_statement_shape).  h = the lowest index with such a finding.
//   device, items [0, h) only (ingest.h).  A device finding (always below h) wins; otherwise item h's is the call's.
//   host, behind the run: rounds, dyn_off, rounds_bad and the degree finding per item from t0 (ingest_mixed_finish_plan).
#pragma once
#include "ingest.h"

namespace bpp {

// what the prelude works out from proof_lens[] and m[]
struct IngestMixedPrelude {
  std::vector<IngestMixedRow> rows;
  uint64_t proof_bytes = 0, sum_m = 0;
  size_t h = 0;     // lowest index with a finding the host can tell without a proof byte; n_items: none
  ProofErr h_err{BPP_OK, ""};
};

// What needs no proof byte, in front of the run: the geometry refusals, pass A's limits on the running sums (they come before every
// per-item check of pass B; the slot limit 2^31 cannot be reached once these hold -- a round takes 64 proof bytes and an item at
// most 64 rounds, so the slots stay below 2^28 + 3 * 2^24 + 2^27), the table, and h.  false: no proofs array -- every item's
// finding then depends on its nonce alone; the engine stages the other arrays and takes the host form.
inline bool ingest_mixed_host_prelude(const bpp_mixed_batch &mx, const ParamShape &P, IngestMixedPrelude &pre) {
  upload_mixed_geometry(mx);
  const size_t n = mx.n_items;
  uint64_t proof_bytes = 0, sum_m = 0;
  pre.rows.assign(n, IngestMixedRow{});
  for (size_t i = 0; i < n; i++) {
    pre.rows[i] = IngestMixedRow{(uint32_t)mx.proof_lens[i], (uint32_t)proof_bytes, (uint32_t)sum_m, mx.m[i]};
    proof_bytes += mx.proofs ? mx.proof_lens[i] : 0;
    sum_m += mx.m[i];
    if (proof_bytes + sum_m * 32 >= (1ull << 32) || sum_m >= (1ull << 28))
      throw ProofErr{BPP_ERR_SIZE_OVERFLOW, "batch too large for one call (4 GB of proof bytes)"};
  }
  pre.proof_bytes = proof_bytes;
  pre.sum_m = sum_m;
  if (!mx.proofs) return false;
  pre.h = n;
  for (size_t i = 0; i < n; i++) {
    try {
      upload_check_statement_shape(mx.m[i], mx.commitments32 != nullptr, mx.min_values != nullptr, mx.min_present != nullptr, P);
    } catch (const ProofErr &e) {
      pre.h = i;
      pre.h_err = e;
      pre.h_err.index = (uint32_t)i;
      break;
    }
  }
  return true;
}

inline Ingest ingest_mixed_args(const bpp_mixed_batch &mx, const ParamShape &P, const IngestMixedPrelude &pre, const IngestMixedRow *rows,
                                uint8_t *bytes, uint64_t *minvals, uint8_t *seeds, uint8_t *info, uint32_t *result) {
  Ingest a;
  memset(&a, 0, sizeof(a));
  a.proofs = mx.proofs;
  a.proof_stride = mx.proof_stride;
  a.commitments32 = mx.commitments32;
  a.min_values = mx.min_values;
  a.min_present = mx.min_present;
  a.seed_nonces32 = mx.seed_nonces32;
  a.seed_present = mx.seed_present;
  a.rows = rows;
  a.n_run = (uint32_t)pre.h;
  a.m_stride = mx.m_stride;
  a.n_bits = P.n_bits;
  a.tr_bad = (mx.transcript_state && mx.transcript_state[200] >= BPP_STROBE_R) ? 1u : 0u;
  a.proof_bytes = pre.proof_bytes;
  a.bytes_total = pre.proof_bytes + pre.sum_m * 32;
  a.bytes = bytes;
  a.minvals = minvals;
  a.seeds = mx.seed_nonces32 ? seeds : nullptr;
  a.info = info;
  a.result = result;
  return a;
}

// The call's construction finding, if it has one: the device's (an index below h) before the host's at h.  `res`: the result words
// of the run over [0, h), or null when h is 0 and nothing ran.
inline void ingest_mixed_throw_finding(const IngestMixedPrelude &pre, size_t n_items, const uint32_t *res) {
  if (res) ingest_throw_finding(res);
  if (pre.h < n_items) throw pre.h_err;
}

// Behind the run (first bytes all equal, h == n_items): the plan upload_pass_a + upload_pass_b make of the equivalent items, per
// item from t0, proof_lens[i] and m[i]; throws the lowest-index construction finding.  `info`: the per-item bytes, or null when
// ingest_needs_info said no.  The plan's promise and nonce arrays stay empty: they are on the device.
inline void ingest_mixed_finish_plan(const bpp_mixed_batch &mx, const ParamShape &P, const IngestMixedPrelude &pre, const uint32_t *res,
                                     const uint8_t *info, UploadPlan &pl) {
  const size_t n = mx.n_items;
  ingest_mixed_throw_finding(pre, n, res);
  const size_t t0 = res[BPP_ING_RES_T0] & 255u;
  pl.n_items = n;
  pl.desc.assign(n, ProofDesc{});  // state_idx 0 everywhere: one transcript
  pl.rounds_bad.assign(n, 0);
  pl.defer.assign(n, 0);
  pl.seeds.clear();
  pl.minvals.clear();
  pl.pre.clear();
  pl.states.assign(203, 0);
  pl.tr_err_index = n;
  if (mx.transcript_state) {
    memcpy(pl.states.data(), mx.transcript_state, 203);
    if (pl.states[200] >= BPP_STROBE_R) pl.tr_err_index = 0;
  } else {
    Strobe st;
    merlin_new(st, mx.transcript_label, (uint32_t)(mx.transcript_label ? mx.label_len : 0));
    strobe_to_bytes(pl.states.data(), st);
  }
  pl.proof_bytes = (size_t)pre.proof_bytes;
  pl.sum_m = (size_t)pre.sum_m;
  pl.bytes_total = (size_t)(pre.proof_bytes + pre.sum_m * 32);
  const uint8_t degree = t0 != P.t ? BPP_DEFER_DEGREE : 0;
  const bool promises = res[BPP_ING_RES_ANY_PROMISE] != 0 && info;
  uint64_t dyn64 = 0;
  uint32_t rounds0 = 0;
  pl.any_rounds_bad = false;
  pl.uniform_rounds = true;
  pl.rmax = pl.max_mn = 0;
  for (size_t i = 0; i < n; i++) {
    const IngestMixedRow &r = pre.rows[i];
    const size_t nchunks = ((size_t)r.proof_len - 1) / 32;  // (proof_len >= 1: an empty proof is a finding)
    uint32_t rounds = 0;
    if (nchunks > t0 + 5) rounds = (uint32_t)std::min<size_t>((nchunks - (t0 + 5)) / 2, BPP_MAX_WIRE_ROUNDS);
    if (i == 0) rounds0 = rounds;
    const uint64_t mn = (uint64_t)r.m * P.n_bits;
    ProofDesc &d = pl.desc[i];
    d.proof_off = r.proof_off;
    d.rounds = rounds;
    d.m = r.m;
    d.commit_off = (uint32_t)(pl.proof_bytes + 32 * (size_t)r.minval_idx);
    d.minval_idx = r.minval_idx;
    d.dyn_off = (uint32_t)dyn64;
    d.flags = !mx.seed_nonces32 ? 0u : (!mx.seed_present ? 1u : (info ? (uint32_t)(info[i] & BPP_ING_INFO_SEED) : 0u));
    pl.rounds_bad[i] = rounds >= 32 ? BPP_ERR_SIZE_OVERFLOW : ((1ull << rounds) != mn ? BPP_ERR_INVALID_LENGTH : 0);
    pl.defer[i] = (uint8_t)(degree | (promises ? (info[i] & BPP_ING_INFO_PROMISE) : 0));
    if (pl.rounds_bad[i]) pl.any_rounds_bad = true;
    if (rounds != rounds0) pl.uniform_rounds = false;
    pl.rmax = std::max(pl.rmax, rounds);
    pl.max_mn = std::max(pl.max_mn, (uint32_t)mn);
    dyn64 += (uint64_t)r.m + 3 + 2 * (uint64_t)rounds;
  }
  if (dyn64 >= (1ull << 31)) throw ProofErr{BPP_ERR_SIZE_OVERFLOW, "batch too large for one call (4 GB of proof bytes)"};
  pl.total_dyn = (uint32_t)dyn64;
  pl.any_seed = res[BPP_ING_RES_ANY_SEED] != 0;
  pl.any_defer = degree != 0 || res[BPP_ING_RES_ANY_PROMISE] != 0;
}

}  // namespace bpp
