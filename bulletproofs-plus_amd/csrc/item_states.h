// Per-item transcripts on the device paths: IN at upload and refill (k_item_states), OUT behind an enqueued call (k_states_out).
//
// IN -- bpp_batch_upload_*_device_transcripts and bpp_batch_refill_enqueue*_transcripts hand the engine one 203-byte STROBE state
// per item (state[200] | pos | pos_begin | cur_flags) in device memory; row i of the batch's table (Batch::states) is the state
// item i is verified under, ProofDesc::state_idx = i.  k_item_states runs on the stream behind k_ingest_* / k_refill_* and in front
// of k_refill_finish.  Per row, by the row's first lane: is the row live (the count word, or the batch's own normalised copy of the
// mask: the caller's array is not read a second time), and if so byte 200 of the source row, its `pos`.  pos >= BPP_STROBE_R is the
// item form's finding "transcript state has pos >= rate" (upload_host.h: tr_err_index): ingest_key(i, BPP_ING_TRANSCRIPT) goes
// into the SAME finding word the ingest / refill kernel reduces into, under atomicMax.  The key orders by index first and message id
// second, and BPP_ING_TRANSCRIPT is the highest id, so the lowest item wins and, at one item, everything its proof's parse raises
// comes first -- the order of upload_check_item.  The decision reaches the row's lanes by a shuffle BEFORE any lane moves a byte: a
// bad row is never copied, its slot and every dead slot get 203 zero bytes (which no Merlin state is), and no load is formed from a
// dead row.
//
// OUT -- bpp_verify_enqueue_states: PASS 1 (k_transcripts<true> / k_transcripts_wave<true>) leaves every proof's advanced
// transcript as a row of BPP_STATE_ROW_WORDS words in device memory of the batch; k_states_out runs behind k_verdict_finish and
// turns them into the ABI's 203 bytes at the caller's address.  Row i is handed out when its group's record is exactly
// {BPP_OK, BPP_TIER_NONE, 0, BPP_VERDICT_WRITTEN} and slot i is live; every other row is 203 zero bytes.
//
// Rows are 203 bytes, so neither end shares an alignment with anything: the copies are ingest_copy's (ingest.h), whole words of the
// destination put together from the two aligned source words they straddle, never reading outside a byte's own aligned word.
//
// The per-row routines are shared by the kernels, the engine's drivers (engine.hip) and the sanitizer harness
// (hosttest_item_states.cpp), which runs the one-lane models against upload_pass_a of the equivalent item array.
#pragma once
#include "refill.h"

namespace bpp {

#define BPP_ITEM_STATE_BYTES 203u
#define BPP_ITEM_STATE_POS 200u  // the byte of a row that holds the sponge's position

struct ItemStates {
  const uint8_t *src;     // the caller's rows, n_items x 203 bytes at any byte address
  uint8_t *table;         // the batch's table, n_items x 203 bytes
  uint32_t n_items;       // slots of the batch
  uint32_t n_run;         // rows [0, n_run) are looked at (the mixed upload stops at the first item the host has a finding for)
  uint32_t *finding;      // the ingest / refill kernel's finding word (ingest_key under atomicMax)
  const uint32_t *count;  // one word, read when the kernel runs: the live count; null: every row
  const uint8_t *mask;    // the BATCH's normalised mask (0 or 1 per slot), written by the refill kernel in front; null: no mask
};

// is row i live: inside the run, and by the count (a count beyond the batch makes nothing live) or the mask
BPP_HD bool item_state_live(const ItemStates &a, size_t i) {
  if (i >= (size_t)a.n_run) return false;
  if (a.mask) return a.mask[i] != 0;
  return refill_item_live(i, a.count ? *a.count : a.n_items, a.n_items);
}

// the decision for a LIVE row, by its first lane: one load of the row's pos.  true: the row is copied; false: its key is the finding
BPP_HD bool item_state_decide(const ItemStates &a, size_t i, uint32_t *key_out) {
  const bool bad = a.src[i * (size_t)BPP_ITEM_STATE_BYTES + BPP_ITEM_STATE_POS] >= BPP_STROBE_R;
  *key_out = bad ? ingest_key((uint32_t)i, BPP_ING_TRANSCRIPT) : 0u;
  return !bad;
}

// 203 zero bytes at dst, shared among `lanes` lanes (>= 3); on the device the middle goes as whole words
BPP_HD void item_state_zero(uint8_t *dst, uint32_t lane, uint32_t lanes) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
  if (lane < head) dst[lane] = 0;
  const uint32_t words = (BPP_ITEM_STATE_BYTES - head) / 4u;
  uint32_t *d = reinterpret_cast<uint32_t *>(dst + head);
  for (uint32_t w = lane; w < words; w += lanes) d[w] = 0u;
  const uint32_t done = head + 4u * words;
  if (lane < BPP_ITEM_STATE_BYTES - done) dst[done + lane] = 0;
#else
  ingest_zero(dst, BPP_ITEM_STATE_BYTES, lane, lanes);
#endif
}

// what `lane` of the row's lanes moves, by the broadcast decision: the copy, or the zero row (nothing of the source is read)
BPP_HD void item_state_move(const ItemStates &a, size_t i, bool take, uint32_t lane, uint32_t lanes) {
  uint8_t *dst = a.table + i * (size_t)BPP_ITEM_STATE_BYTES;
  if (take) ingest_copy(dst, a.src + i * (size_t)BPP_ITEM_STATE_BYTES, BPP_ITEM_STATE_BYTES, lane, lanes);
  else item_state_zero(dst, lane, lanes);
}

// ---- OUT: is row i handed out -- its group's record is Ok and nothing else, and the slot is live
BPP_HD bool states_out_give(const bpp_device_verdict &v, bool slot_live) {
  return slot_live && v.code == BPP_OK && v.tier == BPP_TIER_NONE && v.index == 0 && v.flags == BPP_VERDICT_WRITTEN;
}

// row i of the caller's array from the row PASS 1 wrote (`row`: BPP_STATE_ROW_WORDS words, whose first 203 bytes are the ABI's)
BPP_HD void states_out_row(uint8_t *out, const uint32_t *row, size_t i, bool give, uint32_t lane, uint32_t lanes) {
  uint8_t *dst = out + i * (size_t)BPP_ITEM_STATE_BYTES;
  if (give) ingest_copy(dst, reinterpret_cast<const uint8_t *>(row), BPP_ITEM_STATE_BYTES, lane, lanes);
  else item_state_zero(dst, lane, lanes);
}

// the group of slot i: the largest g in [0, G) with group_first[g] <= i  (group_first[0] = 0, group_first[G] > i)
BPP_HD uint32_t states_out_group(const uint32_t *group_first, uint32_t G, uint32_t i) {
  uint32_t lo = 0, hi = G;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (group_first[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct StatesOut {
  const uint32_t *rows;               // B rows of row_words words, as PASS 1 wrote them
  uint32_t row_words;                 // BPP_STATE_ROW_WORDS
  uint8_t *out;                       // the caller's B x 203 bytes at any byte address
  const bpp_device_verdict *verdicts; // the G records k_verdict_finish wrote in front
  const uint32_t *group_first;        // G + 1
  uint32_t G, B;
  LiveView live;                      // the form of the batch's last refill
};

BPP_HD void states_out_item(const StatesOut &a, uint32_t i, uint32_t lane, uint32_t lanes) {
  const bpp_device_verdict v = a.verdicts[states_out_group(a.group_first, a.G, i)];
  const bool give = states_out_give(v, verdict_item_live(a.live, i));
  states_out_row(a.out, a.rows + (size_t)i * a.row_words, i, give, lane, lanes);
}

#if defined(__HIPCC__)
// k_item_states: the geometry of k_ingest_packed, BPP_INGEST_LANES lanes per row.  The row's first lane decides (liveness, then the
// one byte of a live row); the decision is shuffled to the row's lanes before any lane moves a byte.  No lane leaves before the
// shuffle: lanes beyond the last slot carry a zero decision and move nothing.
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_item_states(ItemStates a) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t i = gid / BPP_INGEST_LANES;
  const uint32_t lane = (uint32_t)(gid % BPP_INGEST_LANES);
  const bool slot = i < (size_t)a.n_items;
  uint32_t take = 0, key = 0;
  if (slot && lane == 0 && item_state_live(a, i)) take = item_state_decide(a, i, &key) ? 1u : 0u;
  take = (uint32_t)__shfl((int)take, 0, (int)BPP_INGEST_LANES);
  if (slot) item_state_move(a, i, take != 0, lane, BPP_INGEST_LANES);
  if (key) atomicMax(a.finding, key);
}

// k_states_out: the same geometry over the batch's slots.  Every lane of a row looks the row's group up and reads its record (the
// same few cached words for all of them), so there is no cross-lane operation and a lane beyond the last slot simply has nothing to do.
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_states_out(StatesOut a) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t i = gid / BPP_INGEST_LANES;
  if (i < (size_t)a.B) states_out_item(a, (uint32_t)i, (uint32_t)(gid % BPP_INGEST_LANES), BPP_INGEST_LANES);
}
#endif

// ---- the kernels on the host, one lane per row, reduced as the kernels reduce (the models of hosttest_item_states.cpp)
inline void item_states_run_host(const ItemStates &a) {
  for (size_t i = 0; i < a.n_items; i++) {
    uint32_t key = 0;
    const bool take = item_state_live(a, i) && item_state_decide(a, i, &key);
    item_state_move(a, i, take, 0, 1);
    if (key > *a.finding) *a.finding = key;
  }
}

inline void states_out_run_host(const StatesOut &a) {
  for (uint32_t i = 0; i < a.B; i++) states_out_item(a, i, 0, 1);
}

}  // namespace bpp
