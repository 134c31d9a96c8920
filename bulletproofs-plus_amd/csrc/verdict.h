// Verdict resolution shared by host and device: the reference's error precedence over the proofs of ONE verify() call, restated
// as a minimum over per-proof keys -- no exceptions, no messages -- so that a kernel can resolve it behind the final MSM
// (bpp_verify_enqueue) and the host can hold it to the throwing routines of upload_host.h (hosttest_verdict.cpp).
//
// What it restates: check_deferred + check_chunk_errors (upload_host.h) and the final-check line of verify_flow_once (engine.hip):
//   tier DEGREE over all proofs, then PROMISE, then STATEMENT_POINT, then PASS1, each at its lowest index; then PASS 2 in proof
//   order, and inside one proof decompression before SizeOverflow before InvalidLength; the MSM last, and only for a group that is
//   held to the final check.
//
// Key layout (64 bits, smaller = raised first; all ones = nothing found):
//   bits 34..36  tier (BPP_TIER_DEGREE .. BPP_TIER_PASS2)
//   bits  2..33  index of the proof inside its group
//   bits  0..1   order inside PASS 2 of one proof: 0 decompression, 1 SizeOverflow, 2 InvalidLength (0 in every other tier)
#pragma once
#include <stdint.h>

#include "../../include/bpp.h"
#include "field.h"   // BPP_HD
#include "layout.h"  // BPP_ST_*

namespace bpp {

// (the BPP_DEFER_* bits of upload_host.h, which a kernel cannot include: the host test holds the two to each other)
#define BPP_VERDICT_DEFER_DEGREE 1u
#define BPP_VERDICT_DEFER_PROMISE 2u
#define BPP_VERDICT_KEY_NONE (~0ull)

BPP_HD uint64_t verdict_key_make(uint32_t tier, uint32_t index, uint32_t sub) {
  return ((uint64_t)tier << 34) | ((uint64_t)index << 2) | (uint64_t)sub;
}

// the first finding the reference raises among those of ONE proof (a proof's findings of a lower tier always come before its
// findings of a higher one: the index is the same)
BPP_HD uint64_t verdict_key(uint32_t defer_bits, uint32_t status_bits, uint32_t rounds_bad, uint32_t index_in_group) {
  if (defer_bits & BPP_VERDICT_DEFER_DEGREE) return verdict_key_make(BPP_TIER_DEGREE, index_in_group, 0);
  if (defer_bits & BPP_VERDICT_DEFER_PROMISE) return verdict_key_make(BPP_TIER_PROMISE, index_in_group, 0);
  if (status_bits & BPP_ST_COMMIT_FAIL) return verdict_key_make(BPP_TIER_STATEMENT_POINT, index_in_group, 0);
  if (status_bits & BPP_ST_TRANSCRIPT_FAIL) return verdict_key_make(BPP_TIER_PASS1, index_in_group, 0);
  if (status_bits & BPP_ST_DECOMPRESS_FAIL) return verdict_key_make(BPP_TIER_PASS2, index_in_group, 0);
  if (rounds_bad == (uint32_t)BPP_ERR_SIZE_OVERFLOW) return verdict_key_make(BPP_TIER_PASS2, index_in_group, 1);
  if (rounds_bad == (uint32_t)BPP_ERR_INVALID_LENGTH) return verdict_key_make(BPP_TIER_PASS2, index_in_group, 2);
  return BPP_VERDICT_KEY_NONE;
}

BPP_HD uint64_t verdict_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// the ProofError kind of a key's finding
BPP_HD int32_t verdict_code(uint32_t tier, uint32_t sub) {
  switch (tier) {
    case BPP_TIER_DEGREE: return BPP_ERR_INVALID_ARGUMENT;
    case BPP_TIER_PROMISE: return BPP_ERR_INVALID_LENGTH;
    case BPP_TIER_STATEMENT_POINT: return BPP_ERR_INVALID_ARGUMENT;
    case BPP_TIER_PASS1: return BPP_ERR_VERIFICATION_FAILED;
    case BPP_TIER_PASS2: return sub == 0 ? BPP_ERR_INVALID_ARGUMENT : (sub == 1 ? BPP_ERR_SIZE_OVERFLOW : BPP_ERR_INVALID_LENGTH);
    case BPP_TIER_MSM: return BPP_ERR_VERIFICATION_FAILED;
    default: return BPP_OK;
  }
}

// One group's record from the minimum of its proofs' keys.
//   want_msm      the call ran the weight chains, PASS 2 and the final MSM (verify_flow_once: want_msm)
//   action        the group's VerifyAction; a RecoverOnly group is never held to the final check
//   is_identity   the group's flag of the final MSM (looked at only when the group is held to it)
//   zero_weight   a device weight of the call came out zero: every group that needed weights claims nothing but the redraw
BPP_HD bpp_device_verdict verdict_finish(uint64_t key, bool want_msm, int action, bool is_identity, bool zero_weight) {
  bpp_device_verdict v;
  v.code = BPP_OK;
  v.tier = BPP_TIER_NONE;
  v.index = 0;
  v.flags = BPP_VERDICT_WRITTEN;
  const bool held = want_msm && action != BPP_RECOVER_ONLY;
  if (held && zero_weight) {
    v.flags |= BPP_VERDICT_REDRAW;
    return v;
  }
  if (key != BPP_VERDICT_KEY_NONE) {
    v.tier = (uint32_t)(key >> 34) & 7u;
    v.index = (uint32_t)(key >> 2);
    v.code = verdict_code(v.tier, (uint32_t)key & 3u);
    return v;
  }
  if (held && !is_identity) {
    v.tier = BPP_TIER_MSM;
    v.code = BPP_ERR_VERIFICATION_FAILED;
  }
  return v;
}

// ---- the live count of a batch (bpp_batch_refill_enqueue_count): items at and beyond it are dead slots.  A batch without a count
// word passes BPP_VERDICT_ALL_LIVE and everything below is what it was.
#define BPP_VERDICT_ALL_LIVE 0xffffffffu
// is item i live
BPP_HD bool verdict_item_live(uint32_t i, uint32_t live) { return i < live; }
// group [p0, p1): its live length -- the proofs its verify() call runs over; 0: an empty group
BPP_HD uint32_t verdict_group_live(uint32_t p0, uint32_t p1, uint32_t live) { return p0 >= live ? 0u : (p1 < live ? p1 : live) - p0; }

// ---- liveness per item (bpp_batch_refill_enqueue_live): a batch is in the form of its last refill, and the view names that form
// alone -- `count`, the batch's count word (a prefix is live), or `mask`, the batch's own normalised copy of the refill's mask,
// one byte per slot, 0 or 1 (any set of slots is live).  Both null: every item is live.  A live group's verify() call runs over its
// live slots in slot order; the finding's index stays the slot offset p - p0, which is the slot of the reference's k-th live item.
struct LiveView {
  const uint32_t *count;
  const uint8_t *mask;
};
// is item i live
BPP_HD bool verdict_item_live(const LiveView &v, uint32_t i) {
  return v.mask ? v.mask[i] != 0 : verdict_item_live(i, v.count ? *v.count : BPP_VERDICT_ALL_LIVE);
}
// group [p0, p1): how many live items it holds; 0: an empty group.  (One lane's form: k_verdict_finish and k_weight_chain count a
// masked group with a ballot per 64 slots.)
BPP_HD uint32_t verdict_group_live(const LiveView &v, uint32_t p0, uint32_t p1) {
  if (!v.mask) return verdict_group_live(p0, p1, v.count ? *v.count : BPP_VERDICT_ALL_LIVE);
  uint32_t n = 0;
  for (uint32_t p = p0; p < p1; p++) n += v.mask[p] != 0 ? 1u : 0u;
  return n;
}

// ---- the refill-state word of a batch (refill.h: k_refill_finish writes it, bpp_batch_refill_enqueue owns it).  Zero: the batch's
// last refill took, or it was never refilled.  Otherwise bits 0..7 hold the BPP_REFILL_* flags of the refill record, bits 8..15 the
// message id, bits 16..23 the code as a signed byte, bits 32..63 the index inside the batch.
BPP_HD uint64_t refill_state_make(uint32_t flags, int32_t code, uint32_t msg, uint32_t index) {
  if (!(flags & (BPP_REFILL_FINDING | BPP_REFILL_FALLBACK | BPP_REFILL_COUNT))) return 0;
  return (uint64_t)(flags & 255u) | ((uint64_t)(msg & 255u) << 8) | ((uint64_t)((uint32_t)code & 255u) << 16) | ((uint64_t)index << 32);
}

// verdict_finish with the refill-state word: a refill that did not take answers for every group of every enqueue until the next
// refill -- nothing of the verification is claimed, whatever it found.  A zero word gives verdict_finish as it is.
BPP_HD bpp_device_verdict verdict_finish(uint64_t key, bool want_msm, int action, bool is_identity, bool zero_weight, uint64_t refill_state) {
  if (!(refill_state & (BPP_REFILL_FINDING | BPP_REFILL_FALLBACK | BPP_REFILL_COUNT))) return verdict_finish(key, want_msm, action, is_identity, zero_weight);
  bpp_device_verdict v;
  v.code = BPP_OK;
  v.tier = BPP_TIER_NONE;
  v.index = 0;
  v.flags = BPP_VERDICT_WRITTEN | BPP_VERDICT_REFILL;
  if (!(refill_state & (BPP_REFILL_FALLBACK | BPP_REFILL_COUNT))) {  // (a bad count and the fall-back come first and claim nothing)
    v.code = (int32_t)(int8_t)(uint8_t)(refill_state >> 16);
    v.tier = BPP_TIER_CONSTRUCTION;
    v.index = (uint32_t)(refill_state >> 32);
  }
  return v;
}

// ... and with the group's live length (verdict_group_live): a refill that did not take still answers for every group; otherwise a
// group without a live item claims nothing at all -- not even the redraw, which only a live item's weight can raise
BPP_HD bpp_device_verdict verdict_finish(uint64_t key, bool want_msm, int action, bool is_identity, bool zero_weight, uint64_t refill_state,
                                         uint32_t live_len) {
  if (live_len != 0 || (refill_state & (BPP_REFILL_FINDING | BPP_REFILL_FALLBACK | BPP_REFILL_COUNT)))
    return verdict_finish(key, want_msm, action, is_identity, zero_weight, refill_state);
  bpp_device_verdict v;
  v.code = BPP_OK;
  v.tier = BPP_TIER_NONE;
  v.index = 0;
  v.flags = BPP_VERDICT_WRITTEN | BPP_VERDICT_EMPTY;
  return v;
}

// the text the blocking calls return with a (tier, code) pair ("" for Ok and for pairs no check raises)
inline const char *verdict_message(uint32_t tier, int32_t code) {
  switch (tier) {
    case BPP_TIER_DEGREE: return code == BPP_ERR_INVALID_ARGUMENT ? "Inconsistent extension degree" : "";
    case BPP_TIER_PROMISE: return code == BPP_ERR_INVALID_LENGTH ? "Minimum value promise exceeds bit vector capacity" : "";
    case BPP_TIER_STATEMENT_POINT:
      return code == BPP_ERR_INVALID_ARGUMENT ? "Statement commitment is not the canonical encoding of a point" : "";
    case BPP_TIER_PASS1:
      return code == BPP_ERR_VERIFICATION_FAILED ? "Identity element cannot be added to the transcript / transcript challenge cannot be zero" : "";
    case BPP_TIER_PASS2:
      if (code == BPP_ERR_INVALID_ARGUMENT) return "A proof member was not the canonical encoding of a point";
      if (code == BPP_ERR_SIZE_OVERFLOW) return "Internal size overflow";
      if (code == BPP_ERR_INVALID_LENGTH) return "Vector L/R length not adequate";
      return "";
    case BPP_TIER_MSM: return code == BPP_ERR_VERIFICATION_FAILED ? "Range proof batch not valid" : "";
    default: return "";
  }
}

#if defined(__HIPCC__)

// ---- the two launches behind the final MSM of bpp_verify_enqueue: together they take the place of k_results_out in that path.
//
// k_verdict_scan: workgroups of BPP_VERDICT_BLOCK proofs (= BPP_STATUS_BLOCK).  Every lane reads its proof's status word, its
// rounds_bad byte and its deferred bits (a null array: all clear) and puts status[] back to status0[] -- k_results_out's contract:
// the next verification of the batch starts clean.  A lane with a finding looks its group up in group_first[0 .. G] by binary
// search; the keys are min-reduced per wavefront with cross-lane operations, group by group for the groups the wavefront touches,
// and ONE 64-bit atomicMin per (wavefront, group) goes to the group's key word.  A wavefront without a finding issues no atomic and
// stores nothing but the status reset.
// MASKED (a batch whose last refill took a mask): live.mask is read, one byte per lane, in place of the count word.
#define BPP_VERDICT_BLOCK 256u
template <bool MASKED = false>
__global__ void __launch_bounds__(BPP_VERDICT_BLOCK) k_verdict_scan(uint32_t *__restrict__ status, const uint32_t *__restrict__ status0,
                                                                    const uint8_t *__restrict__ rounds_bad, const uint8_t *__restrict__ defer,
                                                                    uint32_t B, const uint32_t *__restrict__ group_first, uint32_t G,
                                                                    unsigned long long *__restrict__ keys,
                                                                    const LiveView live = LiveView{nullptr, nullptr}) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lv = (!MASKED && live.count) ? *live.count : BPP_VERDICT_ALL_LIVE;
  uint32_t st = 0, rb = 0, df = 0;
  if (i < B) {
    st = status[i];
    status[i] = status0[i];
    if (rounds_bad) rb = rounds_bad[i];
    if (defer) df = defer[i];
    // a dead slot is put back like any other and contributes no key, whatever it holds (its sanitised bytes do raise PASS-1 findings)
    if (MASKED ? live.mask[i] == 0 : !verdict_item_live(i, lv)) st = rb = df = 0;
  }
  uint32_t g = 0;
  uint64_t key = BPP_VERDICT_KEY_NONE;
  if (i < B && (st | rb | df) != 0) {
    // largest g in [0, G) with group_first[g] <= i  (group_first[0] = 0, group_first[G] = B > i)
    uint32_t lo = 0, hi = G;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (group_first[mid] <= i) lo = mid;
      else hi = mid;
    }
    g = lo;
    key = verdict_key(df, st, rb, i - group_first[g]);
  }
  bool pending = key != BPP_VERDICT_KEY_NONE;
  unsigned long long todo = __ballot(pending);
  const uint32_t lane = threadIdx.x & 63u;
  while (todo) {  // (uniform over the wavefront: one turn per group it touches)
    const int lead = __ffsll(todo) - 1;
    const uint32_t g_lead = (uint32_t)__shfl((int)g, lead, 64);
    const bool mine = pending && g == g_lead;
    uint64_t k = mine ? key : BPP_VERDICT_KEY_NONE;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const uint32_t lo32 = (uint32_t)__shfl_xor((int)(uint32_t)k, off, 64);
      const uint32_t hi32 = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off, 64);
      k = verdict_min(k, ((uint64_t)hi32 << 32) | lo32);
    }
    if (lane == (uint32_t)lead) atomicMin(&keys[g_lead], (unsigned long long)k);
    if (mine) pending = false;
    todo = __ballot(pending);
  }
}

// a masked group's live items, counted by one wavefront with a ballot per 64 mask bytes (every lane calls it; also k_weight_chain's)
__device__ __forceinline__ uint32_t verdict_group_live_wave(const uint8_t *__restrict__ mask, uint32_t p0, uint32_t p1, uint32_t lane) {
  uint32_t n = 0;
  for (uint32_t w0 = p0; w0 < p1; w0 += 64) {
    const uint32_t p = w0 + lane;
    n += (uint32_t)__popcll(__ballot(p < p1 && mask[p] != 0));
  }
  return n;
}

// k_verdict_finish: one wavefront per group.  Lane 0 turns the group's key, its identity flag, its action and the call's
// zero-weight word into the 16-byte record and puts the key word back to all ones for the next enqueue; the wavefront then
// hands out the group's mask rows, 16 bytes per lane and turn: the engine's rows for the items that carry a seed nonce when the
// verdict is Ok and the action recovers, zeros otherwise (an Err returns no masks), and mask_present per item.  The zero-weight
// word is cleared once every group has read it: each wavefront counts itself in `groups_done` behind its read, and the one that
// brings the count to G clears both words, so the next enqueue finds them as it expects them.
//   is_identity == nullptr: the call ran no final MSM (want_msm = 0)
//   masks == nullptr: the call recovered no masks (no group asked, or no item carries a seed nonce)
//   refill_state == nullptr, or a zero word: the batch's contents are what its last upload or refill made them; otherwise every
//     group gets the refill's record (verdict_finish above) and no masks
//   live.count == nullptr: every item is live; otherwise a group that starts at or beyond *live.count gets the EMPTY record, and
//     mask rows and mask_present are handed out below it only (zeros beyond).  groups_done still reaches G.
//   MASKED: live.mask in place of the count word.  The wavefront counts the group's live slots with a ballot per 64 mask bytes;
//     a group without one gets the EMPTY record wherever it lies, and rows and mask_present go to live slots only.
template <bool MASKED = false>
__global__ void __launch_bounds__(64) k_verdict_finish(unsigned long long *__restrict__ keys, const uint32_t *__restrict__ is_identity,
                                                       const int *__restrict__ actions, int action_all, uint32_t *__restrict__ zero_word,
                                                       uint32_t *__restrict__ groups_done, const uint32_t *__restrict__ group_first,
                                                       uint32_t G, const ProofDesc *__restrict__ desc, const uint4 *__restrict__ masks,
                                                       uint32_t row_pieces, bpp_device_verdict *__restrict__ verdicts,
                                                       uint4 *__restrict__ masks_out, uint8_t *__restrict__ mask_present,
                                                       const unsigned long long *__restrict__ refill_state = nullptr,
                                                       const LiveView live = LiveView{nullptr, nullptr}) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= G) return;
  const uint32_t lv = (!MASKED && live.count) ? *live.count : BPP_VERDICT_ALL_LIVE;
  const uint32_t p0 = group_first[g], p1 = group_first[g + 1];
  const uint32_t live_len = MASKED ? verdict_group_live_wave(live.mask, p0, p1, lane) : verdict_group_live(p0, p1, lv);
  int give = 0;
  if (lane == 0) {
    const uint64_t key = keys[g];
    keys[g] = BPP_VERDICT_KEY_NONE;
    const int action = actions ? actions[g] : action_all;
    const bool zero = *zero_word != 0;
    const bpp_device_verdict v = verdict_finish(key, is_identity != nullptr, action, is_identity ? is_identity[g] != 0 : true, zero,
                                                refill_state ? (uint64_t)*refill_state : 0ull, live_len);
    *reinterpret_cast<uint4 *>(&verdicts[g]) = make_uint4((uint32_t)v.code, v.tier, v.index, v.flags);
    give = (masks != nullptr && v.tier == BPP_TIER_NONE && !(v.flags & (BPP_VERDICT_REDRAW | BPP_VERDICT_REFILL | BPP_VERDICT_EMPTY)) &&
            action != BPP_VERIFY_ONLY) ? 1 : 0;
    // every group has read the zero-weight word once the count reaches G: the last one clears both
    __threadfence();
    if (atomicAdd(groups_done, 1u) == G - 1) {
      *zero_word = 0;
      *groups_done = 0;
    }
  }
  give = __shfl(give, 0, 64);
  if (mask_present)
    for (uint32_t p = p0 + lane; p < p1; p += 64) mask_present[p] = (give && (MASKED ? live.mask[p] != 0 : verdict_item_live(p, lv)) && (desc[p].flags & 1u)) ? 1 : 0;
  if (masks_out) {
    const size_t q0 = (size_t)p0 * row_pieces, q1 = (size_t)p1 * row_pieces;
    for (size_t q = q0 + lane; q < q1; q += 64) {
      const uint32_t p = (uint32_t)(q / row_pieces);
      masks_out[q] = (give && (MASKED ? live.mask[p] != 0 : verdict_item_live(p, lv)) && (desc[p].flags & 1u)) ? masks[q] : make_uint4(0, 0, 0, 0);
    }
  }
}

#endif  // __HIPCC__

}  // namespace bpp
