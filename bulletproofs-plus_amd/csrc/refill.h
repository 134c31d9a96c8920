// Device side of bpp_batch_refill_enqueue and its _count, _live and _mixed forms: a resident batch made by a device upload (ingest.h)
// takes new contents of the SAME shape from arrays in device memory, on the stream, with no host involvement.  Everything the host
// decided at upload follows from the shape: layout, slots, rounds_bad, the degree finding, the MSM plan.  The shape is the item count,
// the first byte t0, which optional arrays exist, and per slot (proof_len, m): one pair for a packed batch (ROWS == false: the slot
// is arithmetic and no table is loaded), the batch's own table of IngestMixedRow, left in device memory by the upload, for a mixed one
// (ROWS == true; the strides are the SOURCE's and need only hold the longest row).  What follows from the bytes is found here, per
// item, by the one-item routines of ingest.h over ingest_slot<ROWS>, and STAYS on the device: the construction finding of lowest index
// and "some first byte is not t0" are reduced into two words of the batch, turned into the refill record and the batch's refill-state
// word by k_refill_finish, and reach the verdict records through k_verdict_finish (verdict.h).  What the host can tell from the shape
// alone was settled at upload, so the run covers all N slots.
//
// HARD REQUIREMENT -- no verification kernel sees bytes the blocking upload would have stopped.  The host does not know what a
// refill found, so the verification kernels run on whatever it left.  Several of them assume what the upload's checks established
// (canonical scalars above all: a non-canonical one must never reach the MSM recode).  So an item with a construction finding, or
// with a foreign first byte, is NOT copied: its slot is sanitised with the slot's OWN lengths -- t0 and proof_len - 1 zero bytes at
// proof_off, 32 * m zero bytes at its commitments, zero promises, a zero nonce with the nonce flag clear.  That is a proof which
// passes ingest_check_item for (proof_len, m) whatever they are (the walk depends on the first byte and the length alone, and the
// upload accepted that length under t0; the harnesses hold it to that) and which every kernel already handles as hostile input:
// identity encodings give a PASS-1 finding.  The decision is made by the item's first lane and BROADCAST to the item's lanes before
// any lane moves a byte, so that copying depends on it.
//
// THE LIVE COUNT (bpp_batch_refill_enqueue_count) -- a refill may carry fewer items than the batch holds: one word in device memory,
// read here on the stream, says how many.  Items at and beyond it are DEAD: neither checked (what lies there is neither a finding
// nor a fall-back) nor read; their slots take the same broadcast decision as a refused item's and are sanitised, so the requirement
// above holds for them as well.  k_refill_finish leaves the clamped count in a word of the batch, which is what the weight chains
// (chain_dev.h) and the verdict kernels (verdict.h) read afterwards; every other kernel runs over all slots, and a dead proof
// contributes nothing because its weight is zero.  A count beyond the batch makes nothing live and sets BPP_REFILL_COUNT.
//
// THE LIVE MASK (bpp_batch_refill_enqueue_live) -- liveness per item instead of per prefix: N bytes in device memory, read here on
// the stream, one load per item by the item's first lane; any non-zero byte is live.  A dead item is treated exactly as the count
// form's: not checked, not read, its slot sanitised by the same broadcast decision.  The first lane also writes the normalised byte
// (0 or 1) to the batch's own mask, which is what the chains and the verdict kernels read afterwards (their MASKED forms); the
// caller's array is not looked at again.  A mask refill carries no count: k_refill_finish gets null for both count pointers,
// clamps nothing and leaves the batch's count word alone.
//
// ROW SLACK is never read, and neither is anything of a dead or refused row: every loop is bounded by the slot's own proof_len and m,
// and the source address of a row is only FORMED (ingest_slot), never dereferenced, unless the row is live (its first lane reads it
// for the check) or the decision says TAKE.  ingest_copy's argument about the aligned word behind the last byte of a row therefore
// needs a live row -- one whose bytes exist -- and says nothing else: the source arrays may end behind the last live row.
//
// Shared by the kernels, by the engine's driver (engine.hip: batch_refill_locked) and by the sanitizer harnesses
// (hosttest_refill*.cpp), which run the one-lane model refill_run_host<ROWS> against ingest_run_host<ROWS> + the form's plan.
#pragma once
#include "ingest_mixed.h"
#include "verdict.h"

namespace bpp {

// words the kernel reduces into (device memory of the batch; zero before the run, left zero by k_refill_finish)
#define BPP_REFILL_RED_FINDING 0  // ingest_key of the lowest-index finding under atomicMax; 0 = none
#define BPP_REFILL_RED_DIFFERS 1  // some proof's first byte is not t0
#define BPP_REFILL_RED_WORDS 2

// bits of the per-item decision the first lane broadcasts
#define BPP_REFILL_ITEM_TAKE 1u     // the item is copied; clear: its slot is sanitised
#define BPP_REFILL_ITEM_FOREIGN 2u  // its first byte is not t0

struct Refill {
  Ingest in;              // the caller's arrays and strides, the batch's table (mixed) and its bytes / minvals / seeds (n_run = every slot;
                          // info, result and tr_bad are not used)
  uint32_t n_items;       // slots of the batch
  uint32_t t0;            // the batch's first byte
  uint32_t degree_bit;    // BPP_DEFER_DEGREE when t0 is not the parameters' extension degree: uniform over the batch
  uint8_t *defer;         // n: the deferred bits k_verdict_scan reads
  ProofDesc *desc;        // n: only flags is written (bit 0: seed nonce present)
  uint32_t *status0, *status;  // n each: cleared here, COMMIT_FAIL is written by the decompression that follows
  uint32_t *masks;        // n rows of mask_row_words words: the engine's recovered masks of the old contents, wiped
  uint32_t mask_row_words;
  uint32_t *red;          // BPP_REFILL_RED_WORDS
  const uint32_t *count;  // one word, read when the kernel runs: the live count c; null: every item (bpp_batch_refill_enqueue_count)
  const uint8_t *mask;    // n bytes, read when the kernel runs: item i is live when mask[i] != 0; null: no mask (bpp_batch_refill_enqueue_live)
  uint8_t *mask_out;      // n bytes of the batch: the normalised mask, written with a mask only
};

// the live count as the batch keeps it: c clamped -- a count beyond the batch makes nothing live (BPP_REFILL_COUNT)
BPP_HD uint32_t refill_live(uint32_t count, uint32_t n_items) { return count <= n_items ? count : 0u; }
// is item i of the caller's arrays live: i < min(count, N) and count <= N
BPP_HD bool refill_item_live(size_t i, uint32_t count, uint32_t n_items) { return count <= n_items && i < (size_t)count; }
// ... under a mask, by the item's first lane: the one load of the item's byte, and the normalised byte to the batch's own mask
BPP_HD bool refill_item_live_mask(const Refill &r, size_t i) {
  const bool lv = r.mask[i] != 0;
  r.mask_out[i] = lv ? 1 : 0;
  return lv;
}

// the decision for the LIVE item i, by its first lane: BPP_REFILL_ITEM_* bits, and the item's key for the reduction (0: no finding)
BPP_HD uint32_t refill_item_check(const Refill &r, const IngestSlot &sl, size_t i, uint32_t *key_out) {
  const IngestFinding f = ingest_check_item(sl.proof, sl.proof_len, sl.m, ingest_seed_present(r.in, i), false);
  *key_out = f.msg ? ingest_key((uint32_t)i, f.msg) : 0u;
  const bool foreign = sl.proof_len ? (uint32_t)sl.proof[0] != r.t0 : false;  // (an empty slot cannot exist: the upload refuses it)
  return ((f.msg == BPP_ING_OK && !foreign) ? BPP_REFILL_ITEM_TAKE : 0u) | (foreign ? BPP_REFILL_ITEM_FOREIGN : 0u);
}

// the sanitised slot of item i, from the slot's own lengths and offsets: nothing of the source is looked at
BPP_HD void refill_item_sanitise(const Refill &r, const IngestSlot &sl, size_t i, uint32_t lane, uint32_t lanes) {
  const Ingest &a = r.in;
  uint8_t *slot = a.bytes + sl.proof_off;
  for (size_t k = lane; k < sl.proof_len; k += lanes) slot[k] = k == 0 ? (uint8_t)r.t0 : (uint8_t)0;
  ingest_zero(a.bytes + (size_t)a.proof_bytes + 32 * sl.minval_idx, 32 * (size_t)sl.m, lane, lanes);
  for (uint32_t j = lane; j < sl.m; j += lanes) a.minvals[sl.minval_idx + j] = 0;
  if (a.seeds) ingest_zero(a.seeds + 32 * i, 32, lane, lanes);
}

// what `lane` of the item's lanes moves, by the broadcast decision; returns this lane's share of the item's info bits
BPP_HD uint32_t refill_item_arrays(const Refill &r, const IngestSlot &sl, size_t i, uint32_t decision, uint32_t lane, uint32_t lanes) {
  uint32_t bits = 0;
  if (decision & BPP_REFILL_ITEM_TAKE) bits = ingest_item_arrays(r.in, sl, i, lane, lanes);
  else refill_item_sanitise(r, sl, i, lane, lanes);
  // nothing of the old contents outlives the refill: the status words, the engine's masks of this item
  if (lane == 0) r.status0[i] = r.status[i] = 0;
  uint32_t *row = r.masks + i * (size_t)r.mask_row_words;
  for (uint32_t k = lane; k < r.mask_row_words; k += lanes) row[k] = 0;
  return bits;
}

// the item's folded info bits to where the verification reads them, by the item's first lane
BPP_HD void refill_item_finish(const Refill &r, size_t i, uint32_t bits) {
  r.defer[i] = (uint8_t)(r.degree_bit | (bits & BPP_ING_INFO_PROMISE));
  r.desc[i].flags = bits & BPP_ING_INFO_SEED;
}

// the record of a refill from its two reduction words: the fall-back comes before any finding, as bpp_batch_upload_packed_device
// decides "differs" before ingest_finish_plan throws
// A count beyond the batch (count > n_items) comes before both: no item was looked at.
BPP_HD bpp_device_refill refill_record(uint32_t finding_word, uint32_t differs, uint32_t count = 0, uint32_t n_items = 0) {
  bpp_device_refill rec;
  rec.code = BPP_OK;
  rec.msg = BPP_ING_OK;
  rec.index = 0;
  rec.flags = BPP_REFILL_WRITTEN;
  if (count > n_items) {
    rec.flags |= BPP_REFILL_COUNT;
  } else if (differs) {
    rec.flags |= BPP_REFILL_FALLBACK;
  } else if (finding_word) {
    const uint32_t key = 0xffffffffu - finding_word;
    rec.flags |= BPP_REFILL_FINDING;
    rec.msg = key & 255u;
    rec.index = key >> 8;
    rec.code = ingest_finding(rec.msg).code;
  }
  return rec;
}

#if defined(__HIPCC__)
// The refill kernels: the geometry of the ingest kernels, BPP_INGEST_LANES lanes per item and BPP_INGEST_BLOCK per workgroup, so four
// items -- in the mixed form of DIFFERENT lengths and aggregation factors -- share a wavefront.  The item's first lane decides:
// liveness, then ingest_check_item, then the first byte against t0.  The decision reaches the item's lanes by a shuffle of width
// BPP_INGEST_LANES BEFORE any lane copies or sanitises (the requirement in this file's header).  NO lane returns: all 64 reach the
// shuffles and the ballot in uniform control flow -- every branch above them is closed again before them -- a lane past the last slot
// with a zero decision, and the lanes of a short item fall through their loops early.
// Plain: the live count (r.count, null: every item) is one uniform load per lane; slots at and beyond it -- every slot when it exceeds
// the batch -- are dead: not checked, so they carry the zero decision too, and the broadcast decision sanitises their slots as it
// does a refused item's.  MASKED (r.mask and r.mask_out set, r.count null): the item's first lane loads the item's mask byte, stores
// the normalised one and checks the item only if it is live; liveness reaches the item's lanes inside the decision, which is zero for
// a dead item.
template <bool ROWS, bool MASKED>
__device__ __forceinline__ void refill_kernel_body(const Refill &r) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t i = gid / BPP_INGEST_LANES;
  const uint32_t lane = (uint32_t)(gid % BPP_INGEST_LANES);
  const uint32_t n_items = r.n_items;
  const bool slot = i < n_items;  // a slot of the batch
  IngestSlot sl{};
  if (slot) sl = ingest_slot<ROWS>(r.in, i);
  uint32_t decision = 0, key = 0;
  if constexpr (MASKED) {
    if (slot && lane == 0 && refill_item_live_mask(r, i)) decision = refill_item_check(r, sl, i, &key);
  } else {
    const uint32_t count = r.count ? *r.count : n_items;
    if (lane == 0 && refill_item_live(i, count, n_items)) decision = refill_item_check(r, sl, i, &key);
  }
  decision = (uint32_t)__shfl((int)decision, 0, (int)BPP_INGEST_LANES);
  uint32_t bits = 0;
  if (slot) bits = refill_item_arrays(r, sl, i, decision, lane, BPP_INGEST_LANES);
  for (uint32_t o = BPP_INGEST_LANES / 2; o; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, (int)o, (int)BPP_INGEST_LANES);
  if (slot && lane == 0) {
    refill_item_finish(r, i, bits);
    if (key) atomicMax(&r.red[BPP_REFILL_RED_FINDING], key);
  }
  const bool d = __ballot((decision & BPP_REFILL_ITEM_FOREIGN) != 0) != 0;
  if ((threadIdx.x & 63u) == 0 && d) atomicOr(&r.red[BPP_REFILL_RED_DIFFERS], 1u);
}
template <bool MASKED = false>
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_refill_packed(Refill r) {
  refill_kernel_body<false, MASKED>(r);
}
template <bool MASKED>
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_refill_mixed(Refill r) {
  refill_kernel_body<true, MASKED>(r);
}

// k_refill_finish: one wavefront behind the refill kernel.  Its first lane turns the reduction words into the record at `record`
// (may be null) and into the batch's refill-state word, and leaves the reduction words clear for the next refill, so that no
// memset is ever enqueued between two refills.  count (null: every item) is the caller's word, read here for the last time: the
// clamped value goes to the batch's own word `live` (null: the batch never took a count), which is what later kernels read.
// A refill under a mask passes null for both: nothing is clamped and the batch's count word is left alone.
__global__ void __launch_bounds__(64) k_refill_finish(uint32_t *__restrict__ red, unsigned long long *__restrict__ state,
                                                      bpp_device_refill *__restrict__ record, const uint32_t *__restrict__ count = nullptr,
                                                      uint32_t n_items = 0, uint32_t *__restrict__ live = nullptr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t c = count ? *count : n_items;
  if (live) *live = refill_live(c, n_items);
  const bpp_device_refill rec = refill_record(red[BPP_REFILL_RED_FINDING], red[BPP_REFILL_RED_DIFFERS], c, n_items);
  red[BPP_REFILL_RED_FINDING] = 0;
  red[BPP_REFILL_RED_DIFFERS] = 0;
  *state = refill_state_make(rec.flags, rec.code, rec.msg, rec.index);
  if (record) {
    record->code = rec.code;
    record->msg = rec.msg;
    record->index = rec.index;
    record->flags = rec.flags;
  }
}
#endif

// ---- host side
// what every refill's arguments share, around an `in` made by ingest_args / ingest_mixed_args
inline Refill refill_args_around(const Ingest &in, size_t n_items, const ParamShape &P, uint8_t t0, uint8_t *defer, ProofDesc *desc, uint32_t *status0,
                                 uint32_t *status, uint32_t *masks, uint32_t *red, const uint32_t *count, const uint8_t *mask, uint8_t *mask_out) {
  Refill r;
  memset(&r, 0, sizeof(r));
  r.in = in;
  r.in.n_run = r.n_items = (uint32_t)n_items;
  r.in.tr_bad = 0;  // the batch keeps its transcript
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

// the kernel's arguments from the caller's struct and the batch's buffers (every pointer an address in device memory; the transcript
// fields are not looked at)
inline Refill refill_args(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0, uint8_t *bytes, uint64_t *minvals, uint8_t *seeds,
                          uint8_t *defer, ProofDesc *desc, uint32_t *status0, uint32_t *status, uint32_t *masks, uint32_t *red,
                          const uint32_t *count = nullptr, const uint8_t *mask = nullptr, uint8_t *mask_out = nullptr) {
  bpp_packed_batch in = pk;
  in.transcript_state = nullptr;
  return refill_args_around(ingest_args(in, P, bytes, minvals, seeds, nullptr, nullptr), pk.n_items, P, t0, defer, desc, status0, status, masks,
                            red, count, mask, mask_out);
}

// ... of the mixed form (proof_lens and m are not looked at either: the batch keeps its own table, `rows`)
inline Refill refill_mixed_args(const bpp_mixed_batch &mx, const ParamShape &P, uint8_t t0, const IngestMixedRow *rows, size_t n_items,
                                uint64_t proof_bytes, uint64_t sum_m, uint8_t *bytes, uint64_t *minvals, uint8_t *seeds, uint8_t *defer,
                                ProofDesc *desc, uint32_t *status0, uint32_t *status, uint32_t *masks, uint32_t *red,
                                const uint32_t *count = nullptr, const uint8_t *mask = nullptr, uint8_t *mask_out = nullptr) {
  bpp_mixed_batch in = mx;
  in.transcript_state = nullptr;
  IngestMixedPrelude pre;
  pre.proof_bytes = proof_bytes;
  pre.sum_m = sum_m;
  return refill_args_around(ingest_mixed_args(in, P, pre, rows, bytes, minvals, seeds, nullptr, nullptr), n_items, P, t0, defer, desc, status0,
                            status, masks, red, count, mask, mask_out);
}

// the two kernels on the host, one lane per item, reduced as the kernels reduce: the model the harnesses hold to ingest_run_host<ROWS>
// + the form's plan.  `red` is expected clear and is left clear.  `live` (may be null) takes the clamped count.  With r.mask the
// items' liveness is the mask's, r.mask_out takes the normalised bytes, and no count is read or written.
template <bool ROWS>
inline void refill_run_host(const Refill &r, uint64_t *state, bpp_device_refill *record, uint32_t *live = nullptr) {
  const uint32_t n_items = r.n_items;
  const uint32_t count = (r.count && !r.mask) ? *r.count : n_items;
  for (size_t i = 0; i < n_items; i++) {
    const IngestSlot sl = ingest_slot<ROWS>(r.in, i);
    const bool live_item = r.mask ? refill_item_live_mask(r, i) : refill_item_live(i, count, n_items);
    uint32_t key = 0;
    const uint32_t decision = live_item ? refill_item_check(r, sl, i, &key) : 0u;
    const uint32_t bits = refill_item_arrays(r, sl, i, decision, 0, 1);
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
