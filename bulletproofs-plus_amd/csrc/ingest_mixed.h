// Device side of bpp_batch_upload_mixed_device: a batch of MIXED aggregation factors (bpp_mixed_batch: rows of proof_stride bytes
// and of m_stride entries, the used part of every row in the two host arrays proof_lens[] and m[]) is checked and packed where it
// lies.  The counterpart of ingest.h's packed routines; the per-proof walk (ingest_check_item), the copy (ingest_copy) and the result
// words (BPP_ING_RES_*) are those of ingest.h.  The destination layout is the item form's (upload_pass_a): proofs back to back in item
// order, then the commitments, then BPP_BYTES_SLACK zero bytes; promises at the prefix sum of m.  All of it follows from the two
// host arrays, so the host computes it and hands the kernel one IngestMixedRow per item.  Shared by the kernel (k_ingest_mixed),
// by the engine's driver (engine.hip: upload_mixed_device_impl) and by the sanitizer harness (hosttest_ingest_mixed.cpp), which runs
// them on the host against upload_pass_a + upload_pass_b over item views of the same rows.
//
// Split of the checks (lowest-index construction finding wins, as in upload_run_parts):
//   host, no proof byte needed: the geometry (upload_mixed_geometry), pass A's size limits on the running sums, and per item what
//     upload_check_item raises before it reads a byte (upload_check_statement_shape).  h = the lowest index with such a finding.
//   device, items [0, h) only: a seed nonce with m[i] > 1; the walk of parse_proof; at item 0 the unusable transcript state; the
//     promises.  A device finding (always below h) wins; otherwise item h's is the call's.
//   host, behind the run: rounds, dyn_off, rounds_bad and the degree finding per item from t0 (ingest_mixed_finish_plan).
//
// ROW SLACK is never checked and never copied: every loop below is bounded by the item's own proof_len and m.  ingest_copy's word
// path reads the two aligned source words a destination word straddles; sw[w + 1] is read only for a word whose four source bytes
// all lie inside the n bytes asked for (words = (n - head) / 4: the tail goes byte-wise), and it holds the last of those four, so
// it is the aligned word of a byte of the row itself -- never a word that starts behind the row.  That holds for the last row of
// the array as for any other: the at most three bytes of that word beyond the row are shifted out, and an aligned word that holds
// a byte of an allocation lies inside the allocation's page.
#pragma once
#include "ingest.h"

namespace bpp {

// where item i comes from (its used lengths) and where it goes: all the kernel needs besides the row strides
struct IngestMixedRow {
  uint32_t proof_len;   // < 2^32: the size limits
  uint32_t proof_off;   // prefix sum of proof_len = ProofDesc::proof_off
  uint32_t minval_idx;  // prefix sum of m = ProofDesc::minval_idx; the commitments go to proof_bytes + 32 * minval_idx
  uint32_t m;
};

struct IngestMixed {
  const uint8_t *proofs;
  uint64_t proof_stride;
  const uint8_t *commitments32;
  const uint64_t *min_values;
  const uint8_t *min_present, *seed_nonces32, *seed_present;
  const IngestMixedRow *rows;  // n_items of the batch; the run looks at the first n_run
  uint32_t n_run;              // items [0, n_run) are checked and moved (n_run = h, the first item the host has a finding for)
  uint32_t m_stride, n_bits;
  uint32_t tr_bad;             // as in IngestPacked
  uint64_t proof_bytes, bytes_total;  // of the WHOLE batch: where the commitments start, where the slack starts
  uint8_t *bytes;              // proof_bytes, then sum(m) * 32 commitment bytes, then BPP_BYTES_SLACK zero bytes
  uint64_t *minvals;           // sum(m)
  uint8_t *seeds;              // n_items * 32, or null when seed_nonces32 is
  uint8_t *info;               // n_items: BPP_ING_INFO_*
  uint32_t *result;            // BPP_ING_RES_WORDS words, zero before the run
};

BPP_HD bool ingest_seed_present(const IngestMixed &a, size_t i) {
  return a.seed_nonces32 && (!a.seed_present || a.seed_present[i]);
}

// the first byte the batch's proofs are compared with: proof 0's, or 0 (no proof has it) when proof 0 is empty
BPP_HD uint32_t ingest_mixed_t0(const IngestMixed &a) { return a.rows[0].proof_len ? (uint32_t)a.proofs[0] : 0u; }

// What `lane` of the `lanes` lanes that share item i moves; ingest_item_arrays with the item's own lengths and offsets.
BPP_HD uint32_t ingest_item_arrays(const IngestMixed &a, size_t i, uint32_t lane, uint32_t lanes) {
  const IngestMixedRow r = a.rows[i];
  const size_t row = i * (size_t)a.m_stride;
  ingest_copy(a.bytes + r.proof_off, a.proofs + i * (size_t)a.proof_stride, (size_t)r.proof_len, lane, lanes);
  ingest_copy(a.bytes + (size_t)a.proof_bytes + 32 * (size_t)r.minval_idx, a.commitments32 + 32 * row, 32 * (size_t)r.m, lane, lanes);
  if (i == 0) ingest_zero(a.bytes + (size_t)a.bytes_total, BPP_BYTES_SLACK, lane, lanes);
  uint32_t bits = 0;
  for (uint32_t j = lane; j < r.m; j += lanes) {
    const bool present = a.min_present ? a.min_present[row + j] != 0 : false;
    const uint64_t v = (present && a.min_values) ? a.min_values[row + j] : 0;
    if (present && a.n_bits < 64 && (v >> a.n_bits) > 0) bits |= BPP_ING_INFO_PROMISE;
    a.minvals[(size_t)r.minval_idx + j] = v;
  }
  if (a.seeds) {
    if (ingest_seed_present(a, i)) {
      ingest_copy(a.seeds + 32 * i, a.seed_nonces32 + 32 * i, 32, lane, lanes);
      bits |= BPP_ING_INFO_SEED;
    } else {
      ingest_zero(a.seeds + 32 * i, 32, lane, lanes);
    }
  }
  return bits;
}

// the check of item i and what it adds to the result words, by the item's first lane.  An empty proof has no first byte to
// compare (ingest_check_item reports it without reading one).
BPP_HD uint32_t ingest_item_check(const IngestMixed &a, size_t i, uint32_t *key_out) {
  const IngestMixedRow r = a.rows[i];
  const uint8_t *p = a.proofs + i * (size_t)a.proof_stride;
  const IngestFinding f = ingest_check_item(p, (size_t)r.proof_len, r.m, ingest_seed_present(a, i), a.tr_bad && i == 0);
  *key_out = f.msg ? ingest_key((uint32_t)i, f.msg) : 0u;
  return r.proof_len ? ((uint32_t)p[0] ^ ingest_mixed_t0(a)) : 0u;
}

#if defined(__HIPCC__)
// The geometry of k_ingest_packed: BPP_INGEST_LANES lanes per item, 256-lane blocks, so four items share a wavefront -- here four
// items of different lengths and aggregation factors.  Every loop bound is the item's own, the lanes of a short item fall through
// their loops early, and NO lane returns: all 64 reach the width-16 shuffles and the ballots (a lane past n_run with zeros).
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_ingest_mixed(IngestMixed a) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t i = gid / BPP_INGEST_LANES;
  const uint32_t lane = (uint32_t)(gid % BPP_INGEST_LANES);
  const bool live = i < a.n_run;
  uint32_t bits = 0, differs = 0;
  if (live) {
    if (lane == 0) {
      uint32_t key;
      differs = ingest_item_check(a, i, &key);
      if (key) atomicMax(&a.result[BPP_ING_RES_FINDING], key);
      if (i == 0) a.result[BPP_ING_RES_T0] = ingest_mixed_t0(a);
    }
    bits = ingest_item_arrays(a, i, lane, BPP_INGEST_LANES);
  }
  for (uint32_t o = BPP_INGEST_LANES / 2; o; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, (int)o, (int)BPP_INGEST_LANES);
  if (live && lane == 0) a.info[i] = (uint8_t)bits;
  const bool d = __ballot(differs != 0) != 0, s = __ballot((bits & BPP_ING_INFO_SEED) != 0) != 0,
             pr = __ballot((bits & BPP_ING_INFO_PROMISE) != 0) != 0;
  if ((threadIdx.x & 63u) == 0) {
    if (d) atomicOr(&a.result[BPP_ING_RES_DIFFERS], 1u);
    if (s) atomicOr(&a.result[BPP_ING_RES_ANY_SEED], 1u);
    if (pr) atomicOr(&a.result[BPP_ING_RES_ANY_PROMISE], 1u);
  }
}
#endif

// ---- host side: the prelude in front of the run, the plan behind it.  Pure host C++ over upload_host.h.

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

inline IngestMixed ingest_mixed_args(const bpp_mixed_batch &mx, const ParamShape &P, const IngestMixedPrelude &pre, const IngestMixedRow *rows,
                                     uint8_t *bytes, uint64_t *minvals, uint8_t *seeds, uint8_t *info, uint32_t *result) {
  IngestMixed a;
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

inline bool ingest_mixed_needs_info(const bpp_mixed_batch &mx, const uint32_t *res) {
  return res[BPP_ING_RES_ANY_PROMISE] != 0 || (res[BPP_ING_RES_ANY_SEED] != 0 && mx.seed_present != nullptr);
}

// The call's construction finding, if it has one: the device's (an index below h) before the host's at h.  `res`: the result words
// of the run over [0, h), or null when h is 0 and nothing ran.
inline void ingest_mixed_throw_finding(const IngestMixedPrelude &pre, size_t n_items, const uint32_t *res) {
  if (res && res[BPP_ING_RES_FINDING]) {
    const uint32_t key = 0xffffffffu - res[BPP_ING_RES_FINDING];
    ProofErr e{ingest_finding(key & 255u).code, ingest_message(key & 255u)};
    e.index = key >> 8;
    throw e;
  }
  if (pre.h < n_items) throw pre.h_err;
}

// Behind the run (first bytes all equal, h == n_items): the plan upload_pass_a + upload_pass_b make of the equivalent items, per
// item from t0, proof_lens[i] and m[i]; throws the lowest-index construction finding.  `info`: the per-item bytes, or null when
// ingest_mixed_needs_info said no.  The plan's promise and nonce arrays stay empty: they are on the device.
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

// the run itself on the host, one lane per item, reduced as the kernel reduces: the model hosttest_ingest_mixed.cpp holds to the
// item form
inline void ingest_mixed_run_host(const IngestMixed &a) {
  for (int w = 0; w < BPP_ING_RES_WORDS; w++) a.result[w] = 0;
  for (size_t i = 0; i < a.n_run; i++) {
    uint32_t key;
    const uint32_t differs = ingest_item_check(a, i, &key);
    if (key > a.result[BPP_ING_RES_FINDING]) a.result[BPP_ING_RES_FINDING] = key;
    if (i == 0) a.result[BPP_ING_RES_T0] = ingest_mixed_t0(a);
    const uint32_t bits = ingest_item_arrays(a, i, 0, 1);
    a.info[i] = (uint8_t)bits;
    if (differs) a.result[BPP_ING_RES_DIFFERS] |= 1u;
    if (bits & BPP_ING_INFO_SEED) a.result[BPP_ING_RES_ANY_SEED] |= 1u;
    if (bits & BPP_ING_INFO_PROMISE) a.result[BPP_ING_RES_ANY_PROMISE] |= 1u;
  }
}

}  // namespace bpp
