// Device side of bpp_batch_refill_enqueue_mixed: a resident batch of MIXED aggregation factors, made by bpp_batch_upload_mixed_device on
// its device path, takes new contents of the SAME shape from rows in device memory, on the stream, with no host involvement.  The
// counterpart of refill.h for ingest_mixed.h: the shape is the VECTOR (proof_len[i], m[i]) per slot -- the batch's own table of
// IngestMixedRow, which the upload left in device memory -- plus the first byte t0 and which optional arrays exist.  The record, the
// reduction words, the state word, k_refill_finish and the two live forms (a count, a mask) are refill.h's and are not restated here.
//
// THE HARD REQUIREMENT of refill.h holds unchanged: an item's first lane decides -- TAKE unless the item is dead, has a construction
// finding or a foreign first byte -- and broadcasts the decision to the item's lanes BEFORE any lane moves a byte.  A slot that is not
// taken is sanitised with the slot's OWN lengths: t0 and proof_len[i] - 1 zeros at proof_off, 32 * m[i] zero bytes at its commitments,
// zero promises at minval_idx, a zero nonce with the nonce flag clear.  The sanitised slot passes ingest_check_item for (proof_len[i],
// m[i]) whatever they are: the walk depends on the first byte and the length alone, and the upload accepted that length under t0.
//
// Findings: what the host can tell from m[] alone was settled at upload and cannot change under a refill, so the run covers all N slots
// (the upload's n_run was h, and a batch exists only where h == N).  What is left is per item and found here: a seed nonce with
// m[i] > 1, the walk of parse_proof, the promises.
//
// ROW SLACK is never read, and neither is anything of a dead row: every loop is bounded by the slot's own proof_len and m, and the
// source address of a row is only FORMED (never dereferenced) unless the decision says TAKE.  ingest_mixed.h's argument about the
// aligned word behind the last byte of a row therefore needs a taken row -- one whose bytes exist -- and says nothing else: the source
// arrays may end behind the last live row.
//
// Shared by the kernel (k_refill_mixed), by the engine's driver (engine.hip: batch_refill_mixed_locked) and by the sanitizer harness
// (hosttest_refill_mixed.cpp), which runs the one-lane model refill_mixed_run_host against ingest_mixed_run_host + ingest_mixed_finish_plan.
#pragma once
#include "ingest_mixed.h"
#include "refill.h"

namespace bpp {

struct RefillMixed {
  IngestMixed in;         // the caller's arrays and strides; rows = the batch's table; the batch's bytes / minvals / seeds (n_run = every
                          // slot; info, result and tr_bad are not used)
  uint32_t n_items;       // slots of the batch
  uint32_t t0;            // the batch's first byte
  uint32_t degree_bit;    // BPP_DEFER_DEGREE when t0 is not the parameters' extension degree: uniform over the batch
  uint8_t *defer;         // n: the deferred bits k_verdict_scan reads
  ProofDesc *desc;        // n: only flags is written (bit 0: seed nonce present)
  uint32_t *status0, *status;  // n each: cleared here, COMMIT_FAIL is written by the decompression that follows
  uint32_t *masks;        // n rows of mask_row_words words: the engine's recovered masks of the old contents, wiped
  uint32_t mask_row_words;
  uint32_t *red;          // BPP_REFILL_RED_WORDS
  const uint32_t *count;  // one word, read when the kernel runs: the live count; null: every item
  const uint8_t *mask;    // n bytes, read when the kernel runs: item i is live when mask[i] != 0; null: no mask
  uint8_t *mask_out;      // n bytes of the batch: the normalised mask, written with a mask only
};

// the forms of k_refill_mixed
#define BPP_REFILL_MIXED_PLAIN 0   // every item, or a live count
#define BPP_REFILL_MIXED_MASKED 1  // a live mask

// under a mask, by the item's first lane: the one load of the item's byte, and the normalised byte to the batch's own mask
BPP_HD bool refill_item_live_mask(const RefillMixed &r, size_t i) {
  const bool lv = r.mask[i] != 0;
  r.mask_out[i] = lv ? 1 : 0;
  return lv;
}

// the decision for the LIVE item i, by its first lane: BPP_REFILL_ITEM_* bits, and the item's key for the reduction (0: no finding)
BPP_HD uint32_t refill_item_check(const RefillMixed &r, size_t i, uint32_t *key_out) {
  const IngestMixed &a = r.in;
  const IngestMixedRow row = a.rows[i];
  const uint8_t *p = a.proofs + i * (size_t)a.proof_stride;
  const IngestFinding f = ingest_check_item(p, (size_t)row.proof_len, row.m, ingest_seed_present(a, i), false);
  *key_out = f.msg ? ingest_key((uint32_t)i, f.msg) : 0u;
  const bool foreign = row.proof_len ? (uint32_t)p[0] != r.t0 : false;  // (an empty slot cannot exist: the upload refuses it)
  return ((f.msg == BPP_ING_OK && !foreign) ? BPP_REFILL_ITEM_TAKE : 0u) | (foreign ? BPP_REFILL_ITEM_FOREIGN : 0u);
}

// the sanitised slot of item i, from the slot's own lengths and offsets: nothing of the source is looked at
BPP_HD void refill_item_sanitise(const RefillMixed &r, size_t i, uint32_t lane, uint32_t lanes) {
  const IngestMixed &a = r.in;
  const IngestMixedRow row = a.rows[i];
  uint8_t *slot = a.bytes + row.proof_off;
  for (size_t k = lane; k < (size_t)row.proof_len; k += lanes) slot[k] = k == 0 ? (uint8_t)r.t0 : (uint8_t)0;
  ingest_zero(a.bytes + (size_t)a.proof_bytes + 32 * (size_t)row.minval_idx, 32 * (size_t)row.m, lane, lanes);
  for (uint32_t j = lane; j < row.m; j += lanes) a.minvals[(size_t)row.minval_idx + j] = 0;
  if (a.seeds) ingest_zero(a.seeds + 32 * i, 32, lane, lanes);
}

// what `lane` of the item's lanes moves, by the broadcast decision; returns this lane's share of the item's info bits
BPP_HD uint32_t refill_item_arrays(const RefillMixed &r, size_t i, uint32_t decision, uint32_t lane, uint32_t lanes) {
  uint32_t bits = 0;
  if (decision & BPP_REFILL_ITEM_TAKE) bits = ingest_item_arrays(r.in, i, lane, lanes);
  else refill_item_sanitise(r, i, lane, lanes);
  // nothing of the old contents outlives the refill: the status words, the engine's masks of this item
  if (lane == 0) r.status0[i] = r.status[i] = 0;
  uint32_t *mrow = r.masks + i * (size_t)r.mask_row_words;
  for (uint32_t k = lane; k < r.mask_row_words; k += lanes) mrow[k] = 0;
  return bits;
}

// the item's folded info bits to where the verification reads them, by the item's first lane (as refill.h's refill_item_finish)
BPP_HD void refill_item_finish(const RefillMixed &r, size_t i, uint32_t bits) {
  r.defer[i] = (uint8_t)(r.degree_bit | (bits & BPP_ING_INFO_PROMISE));
  r.desc[i].flags = bits & BPP_ING_INFO_SEED;
}

#if defined(__HIPCC__)
// k_refill_mixed: the geometry of k_ingest_mixed, BPP_INGEST_LANES lanes per item and BPP_INGEST_BLOCK per workgroup, so four items of
// DIFFERENT lengths and aggregation factors share a wavefront.  The item's first lane decides (liveness, refill_item_check); the
// decision reaches the item's lanes by a shuffle of width BPP_INGEST_LANES BEFORE any lane copies or sanitises.  NO lane returns: all
// 64 reach the shuffles and the ballot in uniform control flow -- every branch above them is closed again before them -- a lane past
// the last slot with a zero decision, and the lanes of a short item fall through their loops early.
// FORM PLAIN: the live count (r.count, null: every item) is one uniform load per lane; slots at and beyond it -- every slot when it
// exceeds the batch -- are dead.  FORM MASKED (r.mask and r.mask_out set): the item's first lane loads the item's byte and stores the
// normalised one; liveness reaches the item's lanes inside the decision, which is zero for a dead item.
template <int FORM>
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_refill_mixed(RefillMixed r) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t i = gid / BPP_INGEST_LANES;
  const uint32_t lane = (uint32_t)(gid % BPP_INGEST_LANES);
  const uint32_t n_items = r.n_items;
  const bool slot = i < n_items;  // a slot of the batch
  uint32_t decision = 0, key = 0;
  if constexpr (FORM == BPP_REFILL_MIXED_MASKED) {
    if (slot && lane == 0 && refill_item_live_mask(r, i)) decision = refill_item_check(r, i, &key);
  } else {
    const uint32_t count = r.count ? *r.count : n_items;
    if (lane == 0 && refill_item_live(i, count, n_items)) decision = refill_item_check(r, i, &key);
  }
  decision = (uint32_t)__shfl((int)decision, 0, (int)BPP_INGEST_LANES);
  uint32_t bits = 0;
  if (slot) bits = refill_item_arrays(r, i, decision, lane, BPP_INGEST_LANES);
  for (uint32_t o = BPP_INGEST_LANES / 2; o; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, (int)o, (int)BPP_INGEST_LANES);
  if (slot && lane == 0) {
    refill_item_finish(r, i, bits);
    if (key) atomicMax(&r.red[BPP_REFILL_RED_FINDING], key);
  }
  const bool d = __ballot((decision & BPP_REFILL_ITEM_FOREIGN) != 0) != 0;
  if ((threadIdx.x & 63u) == 0 && d) atomicOr(&r.red[BPP_REFILL_RED_DIFFERS], 1u);
}
#endif

// ---- host side
// the kernel's arguments from the caller's struct (every array an address in device memory; proof_lens, m and the transcript fields are
// not looked at: the batch keeps its own) and the batch's table and buffers
inline RefillMixed refill_mixed_args(const bpp_mixed_batch &mx, const ParamShape &P, uint8_t t0, const IngestMixedRow *rows, size_t n_items,
                                     uint64_t proof_bytes, uint64_t sum_m, uint8_t *bytes, uint64_t *minvals, uint8_t *seeds, uint8_t *defer,
                                     ProofDesc *desc, uint32_t *status0, uint32_t *status, uint32_t *masks, uint32_t *red,
                                     const uint32_t *count = nullptr, const uint8_t *mask = nullptr, uint8_t *mask_out = nullptr) {
  RefillMixed r;
  memset(&r, 0, sizeof(r));
  r.in.proofs = mx.proofs;
  r.in.proof_stride = mx.proof_stride;
  r.in.commitments32 = mx.commitments32;
  r.in.min_values = mx.min_values;
  r.in.min_present = mx.min_present;
  r.in.seed_nonces32 = mx.seed_nonces32;
  r.in.seed_present = mx.seed_present;
  r.in.rows = rows;
  r.in.n_run = (uint32_t)n_items;
  r.in.m_stride = mx.m_stride;
  r.in.n_bits = P.n_bits;
  r.in.proof_bytes = proof_bytes;
  r.in.bytes_total = proof_bytes + sum_m * 32;
  r.in.bytes = bytes;
  r.in.minvals = minvals;
  r.in.seeds = mx.seed_nonces32 ? seeds : nullptr;
  r.n_items = (uint32_t)n_items;
  r.t0 = t0;
  r.degree_bit = t0 != P.t ? BPP_DEFER_DEGREE : 0u;
  r.defer = defer;
  r.desc = desc;
  r.status0 = status0;
  r.status = status;
  r.masks = masks;
  r.mask_row_words = P.t * 8;
  r.red = red;
  r.count = count;
  r.mask = mask;
  r.mask_out = mask ? mask_out : nullptr;
  return r;
}

// the two kernels on the host, one lane per item, reduced as the kernels reduce: the model hosttest_refill_mixed.cpp holds to
// ingest_mixed_run_host + ingest_mixed_finish_plan.  `red` is expected clear and is left clear.  `live` (may be null) takes the
// clamped count.  With r.mask the items' liveness is the mask's, r.mask_out takes the normalised bytes, and no count is read or written.
inline void refill_mixed_run_host(const RefillMixed &r, uint64_t *state, bpp_device_refill *record, uint32_t *live = nullptr) {
  const uint32_t n_items = r.n_items;
  const uint32_t count = (r.count && !r.mask) ? *r.count : n_items;
  for (size_t i = 0; i < n_items; i++) {
    const bool live_item = r.mask ? refill_item_live_mask(r, i) : refill_item_live(i, count, n_items);
    uint32_t key = 0;
    const uint32_t decision = live_item ? refill_item_check(r, i, &key) : 0u;
    const uint32_t bits = refill_item_arrays(r, i, decision, 0, 1);
    refill_item_finish(r, i, bits);
    if (key > r.red[BPP_REFILL_RED_FINDING]) r.red[BPP_REFILL_RED_FINDING] = key;
    if (decision & BPP_REFILL_ITEM_FOREIGN) r.red[BPP_REFILL_RED_DIFFERS] |= 1u;
  }
  if (live && !r.mask) *live = refill_live(count, n_items);
  const bpp_device_refill rec = refill_record(r.red[BPP_REFILL_RED_FINDING], r.red[BPP_REFILL_RED_DIFFERS], count, n_items);
  r.red[BPP_REFILL_RED_FINDING] = r.red[BPP_REFILL_RED_DIFFERS] = 0;
  *state = refill_state_make(rec.flags, rec.code, rec.msg, rec.index);
  if (record) *record = rec;
}

}  // namespace bpp
