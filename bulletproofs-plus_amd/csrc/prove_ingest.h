// Device side of bpp_prove_openings_device: the openings of a prove call (bpp_prove_arrays: rows of m_stride entries per item, the
// used part of every row in the host array m[]) are checked and packed where they lie in device memory, and the proofs, commitments
// and per-item outcomes are scattered into the caller's rows in device memory.  The prover's counterpart of ingest_mixed.h: the copy
// (ingest_copy / ingest_zero) and the launch geometry are those of ingest.h.  Shared by the kernels (k_prove_ingest, k_prove_emit), by
// the engine's driver (engine_prove.h) and by the sanitizer harness (hosttest_prove_ingest.cpp), which runs the routines on the host,
// lane by lane, against ProvePack::pack and prove_item_check_host on the sorted equivalent items.
//
// Split of the checks (prove_job_host.h states them and their order):
//   host, no witness byte needed: prove_item_layout_finding + prove_item_rng_finding per item from m[], the strides and which arrays
//     are given.  An item they fail never reaches the device (as in prove_mixed).
//   device (prove_ingest_check): a nonce on an item with m > 1; per opening j in order "Value exceeds bit vector capacity!" then
//     "Minimum value is larger than value"; per blinding factor in order "blinding factor is not canonical"; "seed nonce is not
//     canonical".  The precedence inside an item is prove_item_check_host's.
//   ONE precedence difference: the host routine raises "Mask recovery is not supported..." BEFORE the rng-length check, but the host
//     cannot see seed_present; an item with both a nonce at m > 1 and an rng_stride too short for its m reports the rng-length
//     finding here.  Reachable only with an rng_stride below what the call's largest m needs.
//
// The host's part lives HERE as well, once: prove_device_shape (the host section below) runs those two findings per item, refuses a
// call whose m_stride is below an aggregation factor, sorts the items that pass largest m first and makes the ProveDevRow tables of
// the slots and of the refused items.  The blocking calls, bpp_prove_plan_create and the three prover harnesses all call it.
//
// The layout is the host's (prove_plan_device: ProveDesc rows, roff, mslot, offsets and transcript states from m[] alone, sorted
// largest m first as prove_mixed sorts); the kernel writes the bytes ProvePack::pack would have written for the sorted items, so that
// the prover's kernels read nothing new.  A FAILING item is never copied: its slot receives a fixed, public, valid substitute
// witness (value 0, first blinding factor 1 and the others 0, no promises, no nonce; its commitment is the first blinding base, not
// the identity), costs what a live slot costs and has its result discarded -- the launch geometry depends on nothing the host does
// not know.
//
// ROW SLACK is never read and never written: every loop is bounded by the item's own m, rng length and proof length.
//
// PER-ITEM TRANSCRIPTS (bpp_prove_openings_device_transcripts): row i of the caller's item_states (n x 203 bytes of device memory, at
// any byte address) is the STROBE state item i's proof continues, prove_with_rng(&mut Transcript, ...) per proof.  The finding
// "transcript state has pos >= rate" then belongs to the item and is prove_ingest_check's last stage, as it is
// prove_item_check_host's last throw: one load of byte 200 of the row.  The call-wide head of RangeProofTranscript::new, which the
// host applies once per distinct transcript (ProvePack::advance_states), runs on the device here, once per slot: k_prove_item_states
// behind k_prove_ingest and in front of kp_init writes row k of the sub-batch's state table, and the plan gives slot k state_idx = k.
// A slot with ANY finding continues a fixed public state (203 zero bytes: a sponge at position 0) and nothing of its row but byte
// 200 is ever read.  On the way out k_prove_emit turns the row kp_finish<true> left in the arena into the caller's 203 bytes for a
// slot whose outcome is OK, and writes 203 zero bytes for every other one, refused items included (k_states_out's rule).
//
// THE LIVE MASK, THE OK MASK AND THE SUMMARY (bpp_prove_enqueue, engine_prove_plan.h): byte i of ProveIngest::live equal to zero makes
// item i dead -- prove_ingest_check returns a key that carries BPP_PROVE_MSG_EMPTY before it touches any row of the item, so the slot
// takes the failed slot's path (substitute witness, fixed public state, zeroed output ranges) with a code of 0.  k_prove_emit also
// writes one byte per item, 1 where the outcome is OK (the live mask of the verifier's refill), and the outcome records in call
// order; k_prove_summary reduces those to the record the blocking call's return code and message come from.  All null in the
// blocking calls, which run as before.
#pragma once
#include "item_states.h"
#include "prove_pack_host.h"

namespace bpp {

// sorted slot k of a sub-batch (or a row of the refused items' table): the caller's item it reads and writes
struct ProveDevRow {
  uint32_t item;       // src[k]: the row of the caller's arrays
  uint32_t m;
  uint32_t proof_len;  // prove_item_len_host(m): 0 for an m no statement can have
  uint32_t msg;        // a finding the host already has (a refused item: it has no slot), else 0
  uint32_t zero;       // a failed item: bit 0 the proof slot, bit 1 the commitment slot may be zeroed (the strides hold them)
};
#define BPP_PROVE_ROW_ZERO_PROOF 1u
#define BPP_PROVE_ROW_ZERO_COMMIT 2u

// the caller's arrays as the ingest kernel sees them, and where a sub-batch's pieces go
struct ProveIngest {
  const uint8_t *values;  // (bytes: the array may lie at any byte address)
  const uint8_t *blindings32, *commitments32;
  const uint8_t *min_values;
  const uint8_t *min_present, *seed_nonces32, *seed_present, *rng_bytes;
  uint64_t rng_stride;
  uint32_t m_stride, n_bits, t, nb;
  const uint8_t *g0_32;  // the compressed first blinding base: what a substitute slot brings where the call brings commitments
  const ProveDevRow *rows;
  ProveDesc *desc;       // nb rows as the host planned them; bit 0 of flags is the kernel's
  uint8_t *bytes;
  uint64_t *minvals;
  uint8_t *minpres;
  uint32_t *finding;     // nb words: 0, or prove_ingest_key of the item's first finding
  const uint8_t *item_states;  // the caller's n x 203 bytes, row i = item i's transcript; null: one transcript for the call
  const uint8_t *live;         // (bpp_prove_enqueue) n bytes by item, 0 = the item is dead: nothing of its rows is read; null: every item
};

// the live mask: a dead item's slot reads one byte of the mask and nothing else of the caller's
BPP_HD bool prove_slot_dead(const ProveIngest &a, uint32_t k) { return a.live && a.live[a.rows[k].item] == 0; }

BPP_HD bool prove_seed_present(const ProveIngest &a, size_t i) { return a.seed_nonces32 && (!a.seed_present || a.seed_present[i]); }

BPP_HD uint64_t prove_load_le64(const uint8_t *p) {
  uint64_t v = 0;
  for (int k = 0; k < 8; k++) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

// A finding's key: the larger key is the EARLIER finding in prove_item_check_host's order -- stage (nonce on an aggregated item,
// openings, blinding factors, nonce, transcript state), then the index inside the stage -- so that a maximum over the item's lanes is
// its first one.
#define BPP_PROVE_STAGE_SEED_AGGREGATED 0u
#define BPP_PROVE_STAGE_OPENINGS 1u  // index 2 j: the value, 2 j + 1: its promise
#define BPP_PROVE_STAGE_BLINDINGS 2u
#define BPP_PROVE_STAGE_SEED_NONCE 3u
#define BPP_PROVE_STAGE_TRANSCRIPT 4u  // (per-item transcripts only) byte 200 of the item's row
#define BPP_PROVE_STAGE_LIVE_MASK 0u   // (a live mask only) the item is dead: in front of everything, and nothing else is looked at
BPP_HD uint32_t prove_ingest_key(uint32_t stage, uint32_t index, uint32_t msg) { return 0xffffffffu - ((stage << 28) | (index << 8) | msg); }
BPP_HD uint32_t prove_ingest_key_msg(uint32_t key) { return key ? ((0xffffffffu - key) & 255u) : 0u; }
BPP_HD uint32_t prove_key_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// `lane`'s share of the witness checks of sorted slot k: the key of the first finding among what this lane looked at, 0 for none
BPP_HD uint32_t prove_ingest_check(const ProveIngest &a, uint32_t k, uint32_t lane, uint32_t lanes) {
  // a dead slot: its "finding" is BPP_PROVE_MSG_EMPTY -- the slot gets the substitute witness and the fixed public state as a
  // failed one does, and k_prove_emit zeroes its ranges -- and no row of the item is touched, not even byte 200 of its state
  if (prove_slot_dead(a, k)) return lane == 0 ? prove_ingest_key(BPP_PROVE_STAGE_LIVE_MASK, 0, BPP_PROVE_MSG_EMPTY) : 0u;
  const size_t i = a.rows[k].item, row = i * (size_t)a.m_stride;
  const uint32_t m = a.desc[k].m;
  const bool seed = prove_seed_present(a, i);
  uint32_t key = 0;
  if (lane == 0 && seed && m > 1) key = prove_ingest_key(BPP_PROVE_STAGE_SEED_AGGREGATED, 0, BPP_PROVE_MSG_SEED_AGGREGATED);
  for (uint32_t j = lane; j < m; j += lanes) {
    const uint64_t v = prove_load_le64(a.values + 8 * (row + j));
    if (a.n_bits < 64 && (v >> a.n_bits) > 0) key = prove_key_max(key, prove_ingest_key(BPP_PROVE_STAGE_OPENINGS, 2 * j, BPP_PROVE_MSG_VALUE));
    const bool present = a.min_present ? a.min_present[row + j] != 0 : false;
    if (present && v < prove_load_le64(a.min_values + 8 * (row + j)))
      key = prove_key_max(key, prove_ingest_key(BPP_PROVE_STAGE_OPENINGS, 2 * j + 1, BPP_PROVE_MSG_MINIMUM));
  }
  for (uint32_t q = lane; q < m * a.t; q += lanes)
    if (!sc_is_canonical(a.blindings32 + 32 * (row * a.t + q)))
      key = prove_key_max(key, prove_ingest_key(BPP_PROVE_STAGE_BLINDINGS, q, BPP_PROVE_MSG_BLINDING));
  if (lane == 0 && seed && !sc_is_canonical(a.seed_nonces32 + 32 * i))
    key = prove_key_max(key, prove_ingest_key(BPP_PROVE_STAGE_SEED_NONCE, 0, BPP_PROVE_MSG_SEED_NONCE));
  if (lane == 0 && a.item_states && a.item_states[i * (size_t)BPP_ITEM_STATE_BYTES + BPP_ITEM_STATE_POS] >= BPP_STROBE_R)
    key = prove_key_max(key, prove_ingest_key(BPP_PROVE_STAGE_TRANSCRIPT, 0, BPP_PROVE_MSG_TRANSCRIPT_STATE));
  return key;
}

// `lane`'s share of what sorted slot k receives: the item's bytes, or (failed) the substitute's.  Every byte of the slot's ranges is
// written by exactly one lane.
BPP_HD void prove_ingest_move(const ProveIngest &a, uint32_t k, bool failed, uint32_t lane, uint32_t lanes) {
  const ProveDesc d = a.desc[k];
  const size_t i = a.rows[k].item, row = i * (size_t)a.m_stride;
  const uint32_t m = d.m, wsz = 8 + 32 * a.t;
  const size_t rng_len = (size_t)d.seed_off - d.ext_off;  // (rounds + 3) x 32: the plan's
  uint8_t *wit = a.bytes + d.wit_off, *com = a.bytes + d.commit_off;
  if (failed) {
    for (uint32_t q = lane; q < m * wsz; q += lanes) wit[q] = (q % wsz) == 8 ? 1 : 0;  // v = 0, r[0] = 1, r[1..t) = 0
    for (uint32_t q = lane; q < 32 * m; q += lanes) com[q] = a.commitments32 ? a.g0_32[q & 31u] : 0;
    ingest_zero(a.bytes + d.ext_off, rng_len, lane, lanes);
    ingest_zero(a.bytes + d.seed_off, 32, lane, lanes);
    for (uint32_t j = lane; j < m; j += lanes) {
      a.minvals[d.minval_idx + j] = 0;
      a.minpres[d.minval_idx + j] = 0;
    }
    return;
  }
  for (uint32_t j = 0; j < m; j++) {
    for (uint32_t q = lane; q < 8; q += lanes) wit[j * wsz + q] = a.values[8 * (row + j) + q];
    ingest_copy(wit + j * wsz + 8, a.blindings32 + 32 * (row + j) * a.t, 32 * (size_t)a.t, lane, lanes);
  }
  if (a.commitments32) ingest_copy(com, a.commitments32 + 32 * row, 32 * (size_t)m, lane, lanes);
  else ingest_zero(com, 32 * (size_t)m, lane, lanes);  // (to be made: kp_adopt_commitments writes them here)
  ingest_copy(a.bytes + d.ext_off, a.rng_bytes + i * (size_t)a.rng_stride, rng_len, lane, lanes);
  if (prove_seed_present(a, i)) {
    ingest_copy(a.bytes + d.seed_off, a.seed_nonces32 + 32 * i, 32, lane, lanes);
    if (lane == 0) a.desc[k].flags = d.flags | 1u;
  } else {
    ingest_zero(a.bytes + d.seed_off, 32, lane, lanes);
  }
  for (uint32_t j = lane; j < m; j += lanes) {
    const bool present = a.min_present ? a.min_present[row + j] != 0 : false;
    a.minvals[d.minval_idx + j] = present ? prove_load_le64(a.min_values + 8 * (row + j)) : 0;
    a.minpres[d.minval_idx + j] = present ? 1 : 0;
  }
}

// what the emit kernel reads of a sub-batch behind kp_finish (or, slots == 0, of the refused items' table) and where it writes
struct ProveEmit {
  const ProveDevRow *rows;
  uint32_t n;
  uint32_t slots;             // 1: row k is sorted slot k of the sub-batch; 0: the rows carry their finding and have no slot
  const uint32_t *finding;    // the ingest kernel's words
  const uint8_t *status;      // ProveState::status of slot 0 ...
  uint32_t status_stride;     // ... and the bytes from one slot's to the next
  const uint8_t *proofs;      // rows of plen
  uint32_t plen;
  const uint8_t *commit32;    // what the witness check computed, rows of 32 x mslot
  uint32_t mslot;
  uint8_t *proofs_out;
  uint64_t proof_stride;
  uint8_t *commitments_out;
  uint64_t commit_stride;
  bpp_device_prove_status *status_dev;  // by item; may be null
  bpp_device_prove_status *outcome;     // by slot: what travels to the host (null without slots)
  const uint32_t *tstates;              // kp_finish<true>'s rows, by slot (null without slots or without states_out) ...
  uint32_t tstate_words;                // ... of BPP_STATE_ROW_WORDS words, whose first 203 bytes are the ABI's
  uint8_t *states_out;                  // by item: the caller's n x 203 bytes at any byte address; may be null
  // (bpp_prove_enqueue, else null) by item, refused rows included: 1 where the outcome is OK, else 0 -- the live mask of the
  // verifier's refill -- and the outcome records in call order, which k_prove_summary reads behind the join
  uint8_t *ok_mask;
  bpp_device_prove_status *outcome_item;
};

// the outcome of row k: the host's finding, else the ingest finding, else the proof's status bits as prove_mixed maps them
BPP_HD uint32_t prove_emit_msg(const ProveEmit &e, uint32_t k) {
  if (e.rows[k].msg) return e.rows[k].msg;
  if (!e.slots) return BPP_PROVE_MSG_OK;
  if (e.finding[k]) return prove_ingest_key_msg(e.finding[k]);
  const uint8_t *s = e.status + (size_t)k * e.status_stride;
  const uint32_t st = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
  if (st & 2u) return BPP_PROVE_MSG_OPENING;   // PV_STATUS_COMMIT_MISMATCH
  if (st & 1u) return BPP_PROVE_MSG_IDENTITY;  // PV_STATUS_TRANSCRIPT
  return BPP_PROVE_MSG_OK;
}

BPP_HD void prove_emit_row(const ProveEmit &e, uint32_t k, uint32_t lane, uint32_t lanes) {
  const ProveDevRow r = e.rows[k];
  const uint32_t msg = prove_emit_msg(e, k);
  uint8_t *po = e.proofs_out + (size_t)r.item * e.proof_stride, *co = e.commitments_out + (size_t)r.item * e.commit_stride;
  if (msg == BPP_PROVE_MSG_OK) {
    ingest_copy(po, e.proofs + (size_t)k * e.plen, r.proof_len, lane, lanes);
    ingest_copy(co, e.commit32 + (size_t)k * 32 * e.mslot, 32 * (size_t)r.m, lane, lanes);
  } else {
    if (r.zero & BPP_PROVE_ROW_ZERO_PROOF) ingest_zero(po, r.proof_len, lane, lanes);
    if (r.zero & BPP_PROVE_ROW_ZERO_COMMIT) ingest_zero(co, 32 * (size_t)r.m, lane, lanes);
  }
  if (e.states_out) {  // (dense rows: every item has one, whatever its strides hold)
    const bool give = msg == BPP_PROVE_MSG_OK && e.slots;
    states_out_row(e.states_out, give ? e.tstates + (size_t)k * e.tstate_words : nullptr, r.item, give, lane, lanes);
  }
  if (lane == 0) {
    const bpp_device_prove_status rec{prove_msg_code(msg), msg};
    if (e.status_dev) e.status_dev[r.item] = rec;
    if (e.outcome) e.outcome[k] = rec;
    if (e.outcome_item) e.outcome_item[r.item] = rec;
    if (e.ok_mask) e.ok_mask[r.item] = msg == BPP_PROVE_MSG_OK ? 1 : 0;
  }
}

// ---- the call's summary (bpp_prove_enqueue): a reduction over the outcome records in call order.  A finding is a record whose msg is
// neither OK nor EMPTY; the summary names the first one -- the item whose code and message the blocking call returns -- and counts.
struct ProveSummaryPart {
  uint32_t first;  // the smallest index with a finding, 0xffffffff for none
  uint32_t n_ok, n_failed, n_empty;
};
BPP_HD ProveSummaryPart prove_summary_none() { return ProveSummaryPart{0xffffffffu, 0u, 0u, 0u}; }
BPP_HD ProveSummaryPart prove_summary_merge(const ProveSummaryPart &a, const ProveSummaryPart &b) {
  return ProveSummaryPart{a.first < b.first ? a.first : b.first, a.n_ok + b.n_ok, a.n_failed + b.n_failed, a.n_empty + b.n_empty};
}
// `lane`'s share of the n records
BPP_HD ProveSummaryPart prove_summary_scan(const bpp_device_prove_status *outcome, uint32_t n, uint32_t lane, uint32_t lanes) {
  ProveSummaryPart p = prove_summary_none();
  for (uint32_t i = lane; i < n; i += lanes) {
    const uint32_t msg = outcome[i].msg;
    if (msg == BPP_PROVE_MSG_OK) p.n_ok++;
    else if (msg == BPP_PROVE_MSG_EMPTY) p.n_empty++;
    else {
      p.n_failed++;
      if (i < p.first) p.first = i;
    }
  }
  return p;
}
BPP_HD void prove_summary_write(bpp_device_prove_summary *out, const bpp_device_prove_status *outcome, const ProveSummaryPart &p) {
  bpp_device_prove_summary s;
  const bool found = p.first != 0xffffffffu;
  s.code = found ? outcome[p.first].code : 0;
  s.msg = found ? outcome[p.first].msg : 0u;
  s.index = found ? p.first : 0u;
  s.flags = BPP_PROVE_SUMMARY_WRITTEN;
  s.n_ok = p.n_ok, s.n_failed = p.n_failed, s.n_empty = p.n_empty, s.reserved = 0;
  *out = s;
}
#define BPP_PROVE_SUMMARY_BLOCK 256

// ---- per-item transcripts: what k_prove_item_states reads and writes for sorted slot k of a sub-batch
struct ProveItemStates {
  const uint8_t *src;       // the caller's rows, n x 203 bytes at any byte address
  const ProveDevRow *rows;  // slot k -> the caller's item
  const ProveDesc *desc;    // its m: the "M" append
  const uint32_t *finding;  // the ingest kernel's words: a slot with a finding reads nothing of its row
  const uint8_t *hg32;      // the parameters' H and G bases, (t + 1) x 32 bytes
  uint32_t n_bits, t, nb;
  uint8_t *states;          // the sub-batch's table, nb x 203: row k is what kp_init continues (ProveDesc::state_idx = k)
};

// byte q (< 203) of the state slot k's transcript starts from: the caller's row, or the fixed public state of a slot with a finding
// (zeros: a sponge at position 0, which no Merlin transcript is).  Byte-wise: never outside the row.
BPP_HD bool prove_item_state_take(const ProveItemStates &a, uint32_t k) { return a.finding[k] == 0; }
BPP_HD uint8_t prove_item_state_byte(const ProveItemStates &a, uint32_t k, bool take, uint32_t q) {
  return take ? a.src[(size_t)a.rows[k].item * BPP_ITEM_STATE_BYTES + q] : (uint8_t)0;
}

#if defined(__HIPCC__)
// The geometry of k_ingest_mixed: BPP_INGEST_LANES lanes per item, 256-lane blocks, four items of different m to a wavefront.  Every
// loop bound is the item's own and NO lane returns: all 64 reach the width-16 shuffles (a lane past nb with a zero key).  The
// item's lanes first agree on its finding, then all of them move the item or all of them write the substitute.
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_prove_ingest(ProveIngest a) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t k = gid / BPP_INGEST_LANES;
  const uint32_t lane = (uint32_t)(gid % BPP_INGEST_LANES);
  const bool live = k < a.nb;
  uint32_t key = live ? prove_ingest_check(a, (uint32_t)k, lane, BPP_INGEST_LANES) : 0u;
  for (uint32_t o = BPP_INGEST_LANES / 2; o; o >>= 1) key = prove_key_max(key, (uint32_t)__shfl_xor((int)key, (int)o, (int)BPP_INGEST_LANES));
  if (live) {
    prove_ingest_move(a, (uint32_t)k, key != 0, lane, BPP_INGEST_LANES);
    if (lane == 0) a.finding[k] = key;
  }
}

// Per-item transcripts, between k_prove_ingest and kp_init on the sub-batch's lane stream: kp_init's geometry (one wavefront per slot,
// its ProveLds) and its cooperative sponge.  The slot's starting state -- the caller's row, or zeros for a slot with a finding: a
// wavefront-uniform choice, and no lane returns on it -- gets the seven appends of ProvePack::advance_states (RangeProofTranscript::new,
// src/transcripts.rs:59-89: domain separator, H, the G bases, N, T, M) and goes to row k of the table kp_init reads.  The states are
// public; the LDS is wiped all the same, as by every prover kernel.
__global__ void __launch_bounds__(64) k_prove_item_states(ProveItemStates a) {
  const uint32_t k = blockIdx.x;
  if (k >= a.nb) return;
  __shared__ ProveLds L;
  const KeccakLanes K = keccak_lanes(L.wk[0]);
  const bool take = prove_item_state_take(a, k);
  for (uint32_t q = threadIdx.x; q < 200; q += 64) ((uint8_t *)L.tr)[q] = prove_item_state_byte(a, k, take, q);
  WStrobe tr;
  tr.st = L.tr;
  tr.pos = prove_item_state_byte(a, k, take, BPP_ITEM_STATE_POS);
  tr.pos_begin = prove_item_state_byte(a, k, take, BPP_ITEM_STATE_POS + 1);
  tr.cur_flags = prove_item_state_byte(a, k, take, BPP_ITEM_STATE_POS + 2);
  __syncthreads();
  wm_append_message(tr, K, "dom-sep", 7, BytesAt{(const uint8_t *)"Bulletproofs+ Range Proof"}, 25);
  wm_append_message(tr, K, "H", 1, BytesAt{a.hg32}, 32);
  for (uint32_t g = 0; g < a.t; g++) wm_append_message(tr, K, "G", 1, BytesAt{a.hg32 + 32 * (size_t)(g + 1)}, 32);
  wm_append_u64(tr, K, "N", 1, a.n_bits);
  wm_append_u64(tr, K, "T", 1, a.t);
  wm_append_u64(tr, K, "M", 1, a.desc[k].m);
  ws_sync();
  uint8_t *row = a.states + (size_t)k * BPP_ITEM_STATE_BYTES;
  for (uint32_t q = threadIdx.x; q < 200; q += 64) row[q] = ((const uint8_t *)L.tr)[q];
  if (threadIdx.x == 0) {
    row[BPP_ITEM_STATE_POS] = (uint8_t)tr.pos;
    row[BPP_ITEM_STATE_POS + 1] = (uint8_t)tr.pos_begin;
    row[BPP_ITEM_STATE_POS + 2] = (uint8_t)tr.cur_flags;
  }
  lds_wipe(L);
}

// Behind kp_finish: the same geometry, BPP_INGEST_LANES lanes per row.
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_prove_emit(ProveEmit e) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t k = gid / BPP_INGEST_LANES;
  if (k < e.n) prove_emit_row(e, (uint32_t)k, (uint32_t)(gid % BPP_INGEST_LANES), BPP_INGEST_LANES);
}

// On the context's stream behind the join of every sub-batch stream: one block over the n outcome records, a tree in LDS, one
// record out.  Public data in, public data out.
__global__ void __launch_bounds__(BPP_PROVE_SUMMARY_BLOCK) k_prove_summary(const bpp_device_prove_status *outcome, uint32_t n,
                                                                          bpp_device_prove_summary *out) {
  __shared__ ProveSummaryPart part[BPP_PROVE_SUMMARY_BLOCK];
  part[threadIdx.x] = prove_summary_scan(outcome, n, threadIdx.x, BPP_PROVE_SUMMARY_BLOCK);
  __syncthreads();
  for (uint32_t o = BPP_PROVE_SUMMARY_BLOCK / 2; o; o >>= 1) {
    if (threadIdx.x < o) part[threadIdx.x] = prove_summary_merge(part[threadIdx.x], part[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) prove_summary_write(out, outcome, part[0]);
}
#endif

// ---- host side: the plan in front of the run.  Pure host C++ over prove_pack_host.h.

// The slots of a sub-batch: the call is cut into "prove_subs" sub-batches (2 unless the option says otherwise, at most 16) of never
// fewer than 64 slots.  ProveCall::plan cuts by it; with per-item transcripts the plan below needs the cut as well.
inline uint32_t prove_sub_size(uint32_t B, int prove_subs) {
  const uint32_t subs = prove_subs > 0 ? (uint32_t)std::min(16, prove_subs) : 2u;
  return std::max<uint32_t>(64, (B + subs - 1) / subs);
}
// the bytes of a sub-batch's state table (ProveCall::carve: d_states): the call's distinct states, or a row per slot
inline size_t prove_states_table_bytes(const ProvePack &pk, uint32_t per_item_sub, uint32_t nb) {
  return per_item_sub ? (size_t)nb * BPP_ITEM_STATE_BYTES : pk.states.size();
}

// THE SHAPE STEP of every device form (bpp_prove_openings_device(_transcripts) per call, bpp_prove_plan_create once per plan, and
// the sanitizer harnesses): what follows from m[], the strides and which arrays are given.  Per item the proof length and the host's
// part of the checks -- the layout finding, then the rng length -- and from those the two tables the emit and ingest kernels read.
struct ProveDeviceShape {
  std::vector<size_t> proof_lens;    // per item: prove_item_len_host
  std::vector<uint32_t> msg;         // per item: the host's finding, 0 for an item that has a slot
  std::vector<ProveDevRow> refused;  // the items with a finding, in item order; zeroed where the strides can hold them, as prove_mixed does
  std::vector<ProveDevRow> rows;     // the slots: largest m first, the caller's order inside a class; msg 0, both zero flags
  std::vector<uint32_t> m_sorted;    // rows[k].m
  size_t m_stride_below = 0;         // (a false return) the item the step stopped at
};
// false: item sh.m_stride_below passes the layout finding, but its m is above m_stride -- an item the layout holds, but not a row of
// the arrays: the geometry is the call's, and the whole call is refused.  proof_lens and msg are then filled up to that item.
inline bool prove_device_shape(const ParamShape &P, const uint32_t *m, size_t n_items, uint32_t m_stride, size_t rng_stride, size_t proof_stride,
                               size_t commit_stride, bool fields_ok, ProveDeviceShape &sh) {
  sh = ProveDeviceShape{};
  sh.proof_lens.assign(n_items, 0);
  sh.msg.assign(n_items, BPP_PROVE_MSG_OK);
  for (size_t i = 0; i < n_items; i++) {
    const uint32_t mi = m[i];
    const size_t len = sh.proof_lens[i] = prove_item_len_host(P, mi);
    uint32_t &msg = sh.msg[i];
    msg = prove_item_layout_finding(P, mi, proof_stride, true, commit_stride, fields_ok);
    if (!msg && mi > m_stride) {
      sh.m_stride_below = i;
      return false;
    }
    if (!msg) msg = prove_item_rng_finding(P, mi, rng_stride);
    if (!msg) {
      sh.rows.push_back(ProveDevRow{(uint32_t)i, mi, (uint32_t)len, BPP_PROVE_MSG_OK, BPP_PROVE_ROW_ZERO_PROOF | BPP_PROVE_ROW_ZERO_COMMIT});
      continue;
    }
    uint32_t zero = 0;
    if (len && proof_stride >= len) zero |= BPP_PROVE_ROW_ZERO_PROOF;
    if (len && commit_stride >= (size_t)32 * mi) zero |= BPP_PROVE_ROW_ZERO_COMMIT;
    sh.refused.push_back(ProveDevRow{(uint32_t)i, mi, (uint32_t)len, msg, zero});
  }
  std::stable_sort(sh.rows.begin(), sh.rows.end(), [](const ProveDevRow &a, const ProveDevRow &b) { return a.m > b.m; });
  for (const ProveDevRow &r : sh.rows) sh.m_sorted.push_back(r.m);
  return true;
}

// What ProvePack::pack makes of the sorted equivalent items, as far as it follows from their aggregation factors alone: the
// descriptors with their offsets, roff, the distinct transcript states with the call-level appends, the call's m, rounds and proof
// length, and bytes_len.  `bytes`, `minvals` and `minpres` stay empty: the ingest kernel writes them on the device.
// m_sorted: the aggregation factors of the items that passed the host's part of the checks, largest first.  brought: the call
// brings a commitments array.  One transcript source for the call: a state for every distinct m, in the order they first appear.
// per_item_sub != 0 (per-item transcripts; the value: the slots of a sub-batch, prove_sub_size): the host sees no state.  Slot i reads
// row i % per_item_sub of its sub-batch's table, which k_prove_item_states writes, and pk.states stays empty.
inline void prove_plan_device(const ParamShape &P, const uint8_t *hg32, const uint32_t *m_sorted, size_t n_items, bool brought,
                              const uint8_t *transcript_state, const uint8_t *transcript_label, size_t label_len, ProvePack &pk,
                              uint32_t per_item_sub = 0) {
  const uint32_t t = P.t, B = (uint32_t)n_items;
  pk.m = m_sorted[0];
  pk.plen = prove_item_len_host(P, pk.m);
  pk.rounds = pk.rounds_min = prove_rounds_host(P, pk.m);
  pk.desc.assign(B, ProveDesc{});
  pk.roff.assign(B, 0);
  std::vector<uint32_t> state_m;
  size_t at = 0;
  for (uint32_t i = 0; i < B; i++) {
    const uint32_t mi = m_sorted[i], rounds_i = prove_rounds_host(P, mi);
    ProveDesc &d = pk.desc[i];
    d.m = mi;
    d.mslot = pk.m;
    d.roff = pk.roff[i] = pk.rounds - rounds_i;
    pk.rounds_min = std::min(pk.rounds_min, rounds_i);
    d.minval_idx = i * pk.m;
    d.wit_off = (uint32_t)at;
    at += (size_t)mi * (8 + 32 * t);
    d.commit_off = (uint32_t)at;
    at += (size_t)mi * 32;
    d.ext_off = (uint32_t)at;
    at += 32 * (size_t)(rounds_i + 3);
    d.seed_off = (uint32_t)at;
    at += 32;
    d.flags = brought ? 0u : PV_FLAG_MAKE_COMMITMENTS;
    if (per_item_sub) {
      d.state_idx = i % per_item_sub;
      continue;
    }
    if (i && m_sorted[i - 1] == mi) {
      d.state_idx = pk.desc[i - 1].state_idx;
      continue;
    }
    d.state_idx = (uint32_t)state_m.size();
    state_m.push_back(mi);
  }
  pk.bytes_len = at;
  pk.states.assign(state_m.size() * 203, 0);
  for (size_t id = 0; id < state_m.size(); id++) {
    if (transcript_state) {
      memcpy(&pk.states[id * 203], transcript_state, 203);
    } else {
      Strobe st;
      merlin_new(st, transcript_label, (uint32_t)(transcript_label ? label_len : 0));
      strobe_to_bytes(&pk.states[id * 203], st);
    }
  }
  pk.advance_states(P, hg32, state_m);
}

// k_prove_item_states on the host: the same starting bytes, the appends on merlin.h's one-lane sponge
inline void prove_item_states_run_host(const ProveItemStates &a) {
  for (uint32_t k = 0; k < a.nb; k++) {
    const bool take = prove_item_state_take(a, k);
    uint8_t b[BPP_ITEM_STATE_BYTES];
    for (uint32_t q = 0; q < BPP_ITEM_STATE_BYTES; q++) b[q] = prove_item_state_byte(a, k, take, q);
    Strobe st;
    strobe_from_bytes(st, b);
    merlin_append_message(st, (const uint8_t *)"dom-sep", 7, (const uint8_t *)"Bulletproofs+ Range Proof", 25);
    merlin_append_message(st, (const uint8_t *)"H", 1, a.hg32, 32);
    for (uint32_t g = 0; g < a.t; g++) merlin_append_message(st, (const uint8_t *)"G", 1, a.hg32 + (size_t)(g + 1) * 32, 32);
    merlin_append_u64(st, (const uint8_t *)"N", 1, a.n_bits);
    merlin_append_u64(st, (const uint8_t *)"T", 1, a.t);
    merlin_append_u64(st, (const uint8_t *)"M", 1, a.desc[k].m);
    strobe_to_bytes(a.states + (size_t)k * BPP_ITEM_STATE_BYTES, st);
  }
}

// the run of one sub-batch on the host, `lanes` lanes per item reduced as the kernel reduces: the model the harness holds to the
// item form
inline void prove_ingest_run_host(const ProveIngest &a, uint32_t lanes) {
  for (uint32_t k = 0; k < a.nb; k++) {
    uint32_t key = 0;
    for (uint32_t lane = 0; lane < lanes; lane++) key = prove_key_max(key, prove_ingest_check(a, k, lane, lanes));
    for (uint32_t lane = 0; lane < lanes; lane++) prove_ingest_move(a, k, key != 0, lane, lanes);
    a.finding[k] = key;
  }
}

// k_prove_summary on the host: the same scan per lane, merged as the tree merges
inline void prove_summary_run_host(const bpp_device_prove_status *outcome, uint32_t n, uint32_t lanes, bpp_device_prove_summary *out) {
  std::vector<ProveSummaryPart> part(lanes);
  for (uint32_t lane = 0; lane < lanes; lane++) part[lane] = prove_summary_scan(outcome, n, lane, lanes);
  for (uint32_t o = lanes / 2; o; o >>= 1)
    for (uint32_t lane = 0; lane < o; lane++) part[lane] = prove_summary_merge(part[lane], part[lane + o]);
  prove_summary_write(out, outcome, part[0]);
}

}  // namespace bpp
