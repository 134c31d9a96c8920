// Merlin on the stream (bpp_transcripts_enqueue): Transcript::new, append_message and challenge_bytes, row-wise, on n transcript rows
// of 203 bytes in device memory (state[200] | pos | pos_begin | cur_flags, at any byte address), in place.  It makes the rows that the
// *_transcripts / item_states_dev calls take and goes on with the rows that the *_states calls hand back, so that a caller's
// Fiat-Shamir protocol around a range proof stays on the context's stream.
//
// One wavefront per row on the cooperative sponge of wstrobe.h, the geometry of k_prove_item_states: a row's program is a latency
// chain of Keccak-f, and rows are independent.  The program -- at most BPP_TOP_MAX_OPS operations with their labels -- and NEW's
// state (public, the same for every row, computed once on the host by merlin_new) travel in the launch arguments.
//
// PER ROW, by the row's first lane and broadcast before any lane moves a byte (top_row_decide):
//   DEAD  live[i] == 0: one byte of the mask is read and nothing else of the row, of its data rows or of lens[i].  The state row is
//         not written; its CHALLENGE rows are zeroed; done_mask[i] = 0.
//   VOID  a live row that (the program not beginning with NEW) has pos >= 166 or cur_flags == 0, or for which some APPEND has
//         lens[i] > len.  Bytes 200 and 202 of the row and the lens words are all that is read.  The row becomes 203 zero bytes, its
//         CHALLENGE rows zero, done_mask[i] = 0; it counts in n_void and competes for first_void.
//         cur_flags == 0 is stricter than the host helpers (bpp_transcript_append_message looks at pos alone): no Merlin transcript has
//         that byte zero, but the zero rows k_states_out and k_prove_emit write for rejected, failed and dead items do, and they must
//         stay zero here instead of becoming a plausible-looking transcript.
//   GO    the row is advanced: the bytes merlin.h's routines leave on a host copy of the row, in program order.
// ROW SLACK (stride > len) is neither read nor written: every loop is bounded by the row's own length.
//
// Rows lie at any byte address: the 203 bytes go into LDS and come back with ingest_copy (ingest.h), which never reads outside a byte's
// own aligned word and writes whole words only inside the range; a challenge is squeezed into LDS and copied to its row the same way.
//
// The per-row rules are BPP_HD and shared by the kernel, by the engine's refusals (transcript_ops_refusal) and by the host model
// (transcript_ops_run_host: one lane per row on merlin.h's sponge), which hosttest_transcript_ops.cpp holds to merlin.h's routines
// under ASan with every dead row and every void row's data poisoned.
//
// THE TRANSCRIPT PROTOCOL AND THE TRANSCRIPT RNG (BPP_TOP_APPEND_POINT, _CHALLENGE_SCALAR, _RNG_*): a program that holds one of these
// kinds -- public, known on the host -- runs k_transcript_ops_rng, the same walk with a second STROBE state in LDS (the RNG: a clone
// of the transcript, merlin's TranscriptRngBuilder / TranscriptRng on wstrobe.h's wm_rng_*) and the scalar arithmetic of scalar.h.  A
// program of NEW / APPEND / CHALLENGE alone runs k_transcript_ops, which carries neither.  What is new per row:
//   VOID up front also where an RNG_REKEY has lens[i] > len, and where an APPEND_POINT's row is 32 zero bytes (the identity's
//        encoding; the point rows are read only where no other rule voids the row: BPP_TOP_ROW_VOID_POINT, flag BPP_TOPS_IDENTITY).
//   VOID in the middle of the program where a CHALLENGE_SCALAR or an RNG_SCALARS draw reduces to zero (flag BPP_TOPS_ZERO_SCALAR): the
//        flag is made wave-uniform by a ballot before any lane acts on it, the walk stops, and the row ends as every void row ends.
//   Dead and void rows have every OUTPUT row of the program zeroed (top_kind_writes).
// SECRETS: REKEY's and FINALIZE's rows and all that FILL / FILL32 / SCALARS write.  They pass through the RNG's state, the draw buffer
// and the result buffer in LDS and through registers; no branch, address or loop bound is made of them but the zero-scalar void.  The
// reduction (top_scalar_from_wide: sc_mont_from_wide, sc_from_mont -- select-based conditional subtractions, no branch) runs in one lane
// per draw under a mask that is the draw's index.  lds_wipe covers all of it on every path.
#pragma once
#include <stddef.h>
#include <string.h>

#include <string>
#include <vector>

#include "item_states.h"
#include "scalar.h"
#if defined(__HIPCC__)
#include "wstrobe.h"
#endif

namespace bpp {

#define BPP_TOP_LABEL_WORDS (BPP_TOP_LABEL_MAX / 4)
#define BPP_TOP_STATE_WORDS 51u  // 203 bytes, the last word's top byte unused
#define BPP_TOP_CHUNK 256u       // a challenge leaves the sponge through LDS in pieces of this many bytes

// one operation as the kernel sees it: 26 words
struct TopOp {
  uint32_t kind, label_len;
  uint8_t *data;         // row i at data + i * stride
  uint64_t stride;
  const uint32_t *lens;  // APPEND: row i's own length (len is the cap), or null
  uint32_t len, reserved;
  uint32_t label_w[BPP_TOP_LABEL_WORDS];  // the label's bytes
};
#define BPP_TOP_OP_WORDS 26
static_assert(sizeof(TopOp) == 4 * BPP_TOP_OP_WORDS, "TopOp is staged into LDS word by word");

// the launch arguments: everything the kernel needs, by value
struct TranscriptOps {
  uint8_t *states;  // n x 203 at any byte address, in place
  const uint8_t *live;
  uint8_t *done_mask;
  bpp_device_transcripts_record *record;
  uint32_t n, n_ops;
  uint32_t new_w[BPP_TOP_STATE_WORDS + 1];  // NEW's 203 bytes (ops[0].kind == BPP_TOP_NEW), else zeros
  TopOp ops[BPP_TOP_MAX_OPS];
};

#define BPP_TOP_ROW_DEAD 0u
#define BPP_TOP_ROW_VOID 1u
#define BPP_TOP_ROW_GO 2u
#define BPP_TOP_ROW_VOID_POINT 3u  // void by an APPEND_POINT of the identity's encoding
#define BPP_TOP_SCALARS_AT_ONCE (BPP_TOP_CHUNK / 64u)  // wide draws the LDS chunk holds: a lane each reduces them

BPP_HD bool top_kind_known(uint32_t k) {
  return (k >= BPP_TOP_NEW && k <= BPP_TOP_CHALLENGE) || k == BPP_TOP_APPEND_POINT || k == BPP_TOP_CHALLENGE_SCALAR ||
         (k >= BPP_TOP_RNG_BEGIN && k <= BPP_TOP_RNG_SCALARS);
}
// the kinds k_transcript_ops does not know: a program with one of them runs k_transcript_ops_rng
BPP_HD bool top_kind_extended(uint32_t k) { return k > BPP_TOP_CHALLENGE; }
// the kinds whose rows are the call's OUTPUT (every other kind's rows are read)
BPP_HD bool top_kind_writes(uint32_t k) {
  return k == BPP_TOP_CHALLENGE || k == BPP_TOP_CHALLENGE_SCALAR || k == BPP_TOP_RNG_FILL || k == BPP_TOP_RNG_FILL32 || k == BPP_TOP_RNG_SCALARS;
}
BPP_HD bool top_kind_takes_lens(uint32_t k) { return k == BPP_TOP_APPEND || k == BPP_TOP_RNG_REKEY; }

// Scalar::from_bytes_mod_order_wide on 64 little-endian bytes -> the 32 canonical bytes; 1 where the scalar is zero.  The one scalar
// routine of challenge_scalar and Scalar::random: the kernel (a lane per draw), the host model and the host helpers call it.
BPP_HD uint32_t top_scalar_from_wide(uint8_t out32[32], const uint8_t wide[64]) {
  sc m, c;
  sc_mont_from_wide(m, wide);
  sc_from_mont(c, m);
  sc_store_words(out32, c);
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) any |= c.v[k];
  return any == 0 ? 1u : 0u;
}

BPP_HD bool top_row_live(const uint8_t *live, size_t i) { return !live || live[i] != 0; }
BPP_HD uint8_t *top_state_row(uint8_t *states, size_t i) { return states + i * (size_t)BPP_ITEM_STATE_BYTES; }
BPP_HD uint8_t *top_data_row(const TopOp &op, size_t i) { return op.data + i * (size_t)op.stride; }
// the message length of a GO row's APPEND (top_row_decide made sure it is inside the cap)
BPP_HD uint32_t top_append_len(const TopOp &op, size_t i) { return op.lens ? op.lens[i] : op.len; }

// The decision for row i, by its first lane.  What it reads, in this order and stopping at the first answer: live[i]; bytes 200 and
// 202 of the row (a program that does not begin with NEW); lens[i] of every APPEND that has one.
// X: the program may hold the extended kinds (k_transcript_ops_rng and its model): then also lens[i] of every RNG_REKEY that has one
// and, last and only for a row nothing else voids, the 32 bytes of every APPEND_POINT's row up to the first that is all zero.
template <bool X>
BPP_HD uint32_t top_row_decide_t(const uint8_t *states, const uint8_t *live, const TopOp *ops, uint32_t n_ops, size_t i) {
  if (!top_row_live(live, i)) return BPP_TOP_ROW_DEAD;
  if (ops[0].kind != BPP_TOP_NEW) {
    const uint8_t *row = states + i * (size_t)BPP_ITEM_STATE_BYTES;
    if (row[BPP_ITEM_STATE_POS] >= BPP_STROBE_R || row[BPP_ITEM_STATE_POS + 2] == 0) return BPP_TOP_ROW_VOID;
  }
  for (uint32_t j = 0; j < n_ops; j++)
    if ((ops[j].kind == BPP_TOP_APPEND || (X && ops[j].kind == BPP_TOP_RNG_REKEY)) && ops[j].lens && ops[j].lens[i] > ops[j].len)
      return BPP_TOP_ROW_VOID;
  if (X)
    for (uint32_t j = 0; j < n_ops; j++)
      if (ops[j].kind == BPP_TOP_APPEND_POINT) {
        const uint8_t *p = top_data_row(ops[j], i);
        uint32_t any = 0;
        for (uint32_t k = 0; k < 32; k++) any |= p[k];
        if (any == 0) return BPP_TOP_ROW_VOID_POINT;
      }
  return BPP_TOP_ROW_GO;
}
BPP_HD uint32_t top_row_decide(const uint8_t *states, const uint8_t *live, const TopOp *ops, uint32_t n_ops, size_t i) {
  return top_row_decide_t<false>(states, live, ops, n_ops, i);
}

// `lane`'s share of what a row that is not advanced receives: zeros in its state row (void only) and in its CHALLENGE rows -- with
// X, in every output row of the program
template <bool X>
BPP_HD void top_row_refuse_t(uint8_t *states, const TopOp *ops, uint32_t n_ops, size_t i, bool is_void, uint32_t lane, uint32_t lanes) {
  if (is_void) item_state_zero(top_state_row(states, i), lane, lanes);
  for (uint32_t j = 0; j < n_ops; j++)
    if (X ? top_kind_writes(ops[j].kind) : ops[j].kind == BPP_TOP_CHALLENGE) ingest_zero(top_data_row(ops[j], i), ops[j].len, lane, lanes);
}
BPP_HD void top_row_refuse(uint8_t *states, const TopOp *ops, uint32_t n_ops, size_t i, bool is_void, uint32_t lane, uint32_t lanes) {
  top_row_refuse_t<false>(states, ops, n_ops, i, is_void, lane, lanes);
}

#if defined(__HIPCC__)
struct TopLds {
  uint64_t st[25];
  uint32_t trailer;  // pos | pos_begin << 8 | cur_flags << 16: bytes 200..202 of the row, right behind the state -- one copy in, one out
  uint32_t reserved;
  uint32_t wk[WK_LDS_DWORDS_RC];
  TopOp ops[BPP_TOP_MAX_OPS];
  uint8_t out[BPP_TOP_CHUNK];
};
static_assert(offsetof(TopLds, trailer) == 200, "the row's 203 bytes are contiguous in LDS");
// k_transcript_ops_rng's: behind it the transcript RNG's state and the canonical bytes of the scalars reduced at once -- secrets, and
// inside the one object lds_wipe clears
struct TopLdsRng : TopLds {
  uint64_t rst[25];
  uint8_t res[32 * BPP_TOP_SCALARS_AT_ONCE];
};
template <bool X>
struct TopLdsOf {
  typedef TopLds type;
};
template <>
struct TopLdsOf<true> {
  typedef TopLdsRng type;
};

struct TopOpWords {
  uint32_t w[BPP_TOP_OP_WORDS];
};

// a value every lane holds, as a wave-uniform register
__device__ __forceinline__ uint32_t top_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t top_u64(uint64_t v) { return (uint64_t)top_u32((uint32_t)v) | ((uint64_t)top_u32((uint32_t)(v >> 32)) << 32); }
template <class T>
__device__ __forceinline__ T *top_uptr(T *p) {
  return (T *)(uintptr_t)top_u64((uint64_t)(uintptr_t)p);
}

// challenge_bytes (wm_challenge_bytes, the squeeze cut into pieces that fit the LDS buffer): every piece is copied to the row behind
// the squeeze's trailing barrier, and the next squeeze starts with a barrier of its own
__device__ __forceinline__ void top_challenge(WStrobe &tr, const KeccakLanes &K, const char *label, uint32_t llen, uint8_t *row, uint32_t n,
                                              uint8_t *buf) {
  ws_begin_op(tr, K, BPP_FLAG_M | BPP_FLAG_A, false);
  ws_absorb(tr, K, BytesAt{(const uint8_t *)label}, llen);
  ws_absorb(tr, K, WordAt{n}, 4);
  ws_begin_op(tr, K, BPP_FLAG_I | BPP_FLAG_A | BPP_FLAG_C, false);
  uint32_t off = 0;
  do {
    const uint32_t c = n - off < BPP_TOP_CHUNK ? n - off : BPP_TOP_CHUNK;
    ws_squeeze(tr, K, buf, c);
    ingest_copy(row + off, buf, c, ws_lane(), 64);
    off += c;
  } while (off < n);
}

// TranscriptRng::fill_bytes(n) (wm_rng_fill with the squeeze cut into pieces, as top_challenge cuts challenge_bytes)
__device__ __forceinline__ void top_rng_fill(WStrobe &rng, const KeccakLanes &K, uint8_t *row, uint32_t n, uint8_t *buf) {
  ws_begin_op(rng, K, BPP_FLAG_M | BPP_FLAG_A, false);
  ws_absorb(rng, K, WordAt{n}, 4);
  ws_begin_op(rng, K, BPP_FLAG_I | BPP_FLAG_A | BPP_FLAG_C, false);
  uint32_t off = 0;
  do {
    const uint32_t c = n - off < BPP_TOP_CHUNK ? n - off : BPP_TOP_CHUNK;
    ws_squeeze(rng, K, buf, c);
    ingest_copy(row + off, buf, c, ws_lane(), 64);
    off += c;
  } while (off < n);
}
// n / 32 successive fill_bytes(32): as many as the buffer holds are drawn into it, then copied to the row in one piece
__device__ __forceinline__ void top_rng_fill32(WStrobe &rng, const KeccakLanes &K, uint8_t *row, uint32_t n, uint8_t *buf) {
  for (uint32_t off = 0; off < n;) {
    const uint32_t left = (n - off) / 32u, c = left < BPP_TOP_CHUNK / 32u ? left : BPP_TOP_CHUNK / 32u;
    for (uint32_t k = 0; k < c; k++) wm_rng_fill(rng, K, buf + 32u * k, 32);
    ingest_copy(row + off, buf, 32u * c, ws_lane(), 64);
    off += 32u * c;
  }
}
// `count` scalars, each from a 64-byte draw that draw(p) squeezes to p (behind its trailing barrier): BPP_TOP_SCALARS_AT_ONCE draws go
// into the buffer, a lane each reduces them into res, and the canonical bytes are copied to the row in one piece.  The "is zero" flags
// become wave-uniform through a ballot before anything acts on them.  True: a scalar was zero (nothing more is drawn or written).
template <class Draw>
__device__ __forceinline__ bool top_scalars(Draw draw, uint8_t *row, uint32_t count, uint8_t *buf, uint8_t *res) {
  for (uint32_t done = 0; done < count;) {
    const uint32_t left = count - done, c = left < BPP_TOP_SCALARS_AT_ONCE ? left : BPP_TOP_SCALARS_AT_ONCE;
    for (uint32_t k = 0; k < c; k++) draw(buf + 64u * k);
    uint32_t zero = 0;
    if (ws_lane() < c) zero = top_scalar_from_wide(res + 32u * ws_lane(), buf + 64u * ws_lane());
    ws_sync();
    if (__builtin_amdgcn_ballot_w64(zero != 0) != 0) return true;
    ingest_copy(row + 32u * done, res, 32u * c, ws_lane(), 64);
    done += c;
  }
  return false;
}

// one operation of the kinds k_transcript_ops_rng adds to APPEND / APPEND_POINT / CHALLENGE (`kind` and `u` wave-uniform, `u` what the
// refusals let through).  True: a scalar reduced to zero.
__device__ __forceinline__ bool top_extended_op(uint32_t kind, WStrobe &tr, WStrobe &rng, const KeccakLanes &K, const char *label, uint32_t llen,
                                                const TopOp &u, size_t i, uint8_t *drow, TopLdsRng &L) {
  if (kind == BPP_TOP_CHALLENGE_SCALAR)
    return top_scalars([&](uint8_t *p) { wm_challenge_bytes(tr, K, label, llen, p, 64); }, drow, 1, L.out, L.res);
  if (kind == BPP_TOP_RNG_BEGIN) {
    ws_clone(rng, L.rst, tr);
  } else if (kind == BPP_TOP_RNG_REKEY) {
    const uint32_t wlen = top_u32(top_append_len(u, i));
    wm_rng_rekey(rng, K, label, llen, BytesAt{drow}, wlen);
  } else if (kind == BPP_TOP_RNG_FINALIZE) {
    if (u.data) wm_rng_finalize(rng, K, BytesAt{drow});
    else wm_rng_finalize(rng, K, ZeroAt{});
  } else if (kind == BPP_TOP_RNG_FILL) {
    top_rng_fill(rng, K, drow, u.len, L.out);
  } else if (kind == BPP_TOP_RNG_FILL32) {
    top_rng_fill32(rng, K, drow, u.len, L.out);
  } else {  // BPP_TOP_RNG_SCALARS
    return top_scalars([&](uint8_t *p) { wm_rng_fill(rng, K, p, 64); }, drow, u.len / 32u, L.out, L.res);
  }
  return false;
}

// One wavefront per row; the launch geometry is n blocks of 64 lanes whatever the mask and the rows hold.  The program is staged from
// the by-value arguments into LDS with constant indices (no address of an argument is taken: no scratch); the op walk reads it from
// there through wave-uniform registers.  The decision is lane 0's and broadcast; the branch on it is wave-uniform, so all 64 lanes
// reach every wave-level exchange of the sponge.  Public data throughout in k_transcript_ops (X false: the kernel as it always was,
// register for register); the LDS is wiped all the same, as by every prover kernel.  X true is k_transcript_ops_rng: the extended
// kinds, whose secrets the header's opening lists.
template <bool X>
__global__ void __launch_bounds__(64) k_transcript_ops_t(TranscriptOps a) {
  __shared__ typename TopLdsOf<X>::type L;
  const uint32_t lane = threadIdx.x;
  const size_t i = blockIdx.x;
  const KeccakLanes K = keccak_lanes(L.wk);
#pragma unroll
  for (int j = 0; j < BPP_TOP_MAX_OPS; j++) {
    const TopOpWords W = __builtin_bit_cast(TopOpWords, a.ops[j]);
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < BPP_TOP_OP_WORDS; w++) v = lane == (uint32_t)w ? W.w[w] : v;
    if (lane < BPP_TOP_OP_WORDS) ((uint32_t *)&L.ops[j])[lane] = v;
  }
  ws_sync();
  const uint32_t n_ops = a.n_ops;
  uint32_t code = BPP_TOP_ROW_DEAD;
  if (lane == 0) code = top_row_decide_t<X>(a.states, a.live, L.ops, n_ops, i);
  code = top_u32(code);
  if (code != BPP_TOP_ROW_GO) {
    const bool is_void = code != BPP_TOP_ROW_DEAD;
    top_row_refuse_t<X>(a.states, L.ops, n_ops, i, is_void, lane, 64);
    if (lane == 0) {
      if (a.done_mask) a.done_mask[i] = 0;
      if (is_void && a.record) {
        atomicAdd(&a.record->n_void, 1u);
        atomicMin(&a.record->first_void, (uint32_t)i);
        if (X && code == BPP_TOP_ROW_VOID_POINT) atomicOr(&a.record->flags, BPP_TOPS_IDENTITY);
      }
    }
  } else {
    uint8_t *row = top_state_row(a.states, i);
    const bool fresh = top_u32(L.ops[0].kind) == BPP_TOP_NEW;
    if (fresh) {
      uint32_t v = 0;
#pragma unroll
      for (int w = 0; w < (int)BPP_TOP_STATE_WORDS; w++) v = lane == (uint32_t)w ? a.new_w[w] : v;
      if (lane < BPP_TOP_STATE_WORDS) ((uint32_t *)L.st)[lane] = v;
    } else {
      ingest_copy((uint8_t *)L.st, row, BPP_ITEM_STATE_BYTES, lane, 64);
    }
    ws_sync();
    const uint32_t t0 = top_u32(L.trailer);
    WStrobe tr;
    tr.st = L.st;
    tr.pos = t0 & 255u;
    tr.pos_begin = (t0 >> 8) & 255u;
    tr.cur_flags = (t0 >> 16) & 255u;
    WStrobe rng = tr;  // (X: re-made by RNG_BEGIN, which the refusals put in front of every other RNG op)
    bool zero_scalar = false;  // wave-uniform
    for (uint32_t j = fresh ? 1u : 0u; j < n_ops && !zero_scalar; j++) {
      const TopOp &op = L.ops[j];
      const uint32_t kind = top_u32(op.kind), llen = top_u32(op.label_len);
      TopOp u;  // the op's scalars, wave-uniform (the label stays in LDS)
      u.data = top_uptr(op.data);
      u.stride = top_u64(op.stride);
      u.lens = top_uptr(op.lens);
      u.len = top_u32(op.len);
      const char *label = (const char *)op.label_w;
      uint8_t *drow = top_data_row(u, i);
      if (kind == BPP_TOP_APPEND || (X && kind == BPP_TOP_APPEND_POINT)) {
        const uint32_t mlen = top_u32(top_append_len(u, i));
        wm_append_message(tr, K, label, llen, BytesAt{drow}, mlen);
      } else if (!X || kind == BPP_TOP_CHALLENGE) {
        top_challenge(tr, K, label, llen, drow, u.len, L.out);
      } else {
        if constexpr (X) zero_scalar = top_extended_op(kind, tr, rng, K, label, llen, u, i, drow, L);
      }
    }
    if (X && zero_scalar) {
      // void in the middle of the program: what was written is withdrawn behind a fence, and the row ends as a void row ends
      __threadfence();
      top_row_refuse_t<X>(a.states, L.ops, n_ops, i, true, lane, 64);
      if (lane == 0) {
        if (a.done_mask) a.done_mask[i] = 0;
        if (a.record) {
          atomicAdd(&a.record->n_void, 1u);
          atomicMin(&a.record->first_void, (uint32_t)i);
          atomicOr(&a.record->flags, BPP_TOPS_ZERO_SCALAR);
        }
      }
    } else {
      ws_sync();
      if (lane == 0) L.trailer = tr.pos | (tr.pos_begin << 8) | (tr.cur_flags << 16);
      ws_sync();
      ingest_copy(row, (const uint8_t *)L.st, BPP_ITEM_STATE_BYTES, lane, 64);
      if (lane == 0) {
        if (a.done_mask) a.done_mask[i] = 1;
        if (a.record) atomicAdd(&a.record->n_done, 1u);
      }
    }
  }
  lds_wipe(L);
}

// The two instantiations by the names the rest of the project uses.  (The kernel itself is the template, with its LDS object declared
// inside: a body shared through a function that takes the object by reference cost the plain instantiation 31 VGPRs.)
constexpr auto k_transcript_ops = k_transcript_ops_t<false>;
constexpr auto k_transcript_ops_rng = k_transcript_ops_t<true>;

// the record, on the stream: in front of k_transcript_ops (whose rows add to it with vector atomics) and behind it
__global__ void k_transcript_record_init(bpp_device_transcripts_record *rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *rec = bpp_device_transcripts_record{0u, 0u, 0xffffffffu, 0u};
}
__global__ void k_transcript_record_finish(bpp_device_transcripts_record *rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0) rec->flags = BPP_TOPS_WRITTEN;
}
// ... behind k_transcript_ops_rng, whose rows may have set BPP_TOPS_IDENTITY / BPP_TOPS_ZERO_SCALAR: those stay
__global__ void k_transcript_record_finish_or(bpp_device_transcripts_record *rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(&rec->flags, BPP_TOPS_WRITTEN);
}
#endif

// ---- host side: the refusals in front of any launch, the launch arguments, the model.  Pure host C++.

// What bpp_transcripts_enqueue refuses from the arguments alone (no pointer is dereferenced but ops and the labels' addresses are not
// even read here): the field is named.  Empty: nothing to refuse.  The pointer kinds are the engine's to check.
inline std::string transcript_ops_refusal(const uint8_t *states, size_t n, const bpp_transcript_op *ops, size_t n_ops, const uint8_t *live,
                                          const uint8_t *done_mask, const bpp_device_transcripts_record *record) {
  if (n == 0) return "n is 0";
  if (n > 0x7fffffffu) return "n is above 2^31 - 1";
  if (!states) return "states203_dev is null";
  if (n_ops == 0 || n_ops > BPP_TOP_MAX_OPS || !ops) return "n_ops must be 1 .. " + std::to_string(BPP_TOP_MAX_OPS) + " (and ops not null)";
  struct Range {
    std::string name;
    uintptr_t lo, hi;
    bool written;
  };
  std::vector<Range> ranges;
  ranges.push_back(Range{"states203_dev", (uintptr_t)states, (uintptr_t)states + n * (size_t)BPP_ITEM_STATE_BYTES, true});
  int rng = 0;  // the program's transcript RNG at op j: 0 none, 1 a builder (behind RNG_BEGIN), 2 finalised
  for (size_t j = 0; j < n_ops; j++) {
    const bpp_transcript_op &o = ops[j];
    const std::string at = "ops[" + std::to_string(j) + "].";
    if (!top_kind_known(o.kind)) return at + "kind " + std::to_string(o.kind) + " is unknown";
    if (o.kind == BPP_TOP_NEW && j != 0) return at + "kind: NEW must be op 0";
    if (!o.label && o.label_len) return at + "label is null with label_len > 0";
    if (o.kind == BPP_TOP_NEW) {
      if (o.data_dev || o.len || o.lens_dev) return at + "data_dev / len / lens_dev: NEW takes no data";
      continue;
    }
    if (o.kind == BPP_TOP_RNG_BEGIN) {
      if (o.label_len) return at + "label_len: RNG_BEGIN takes no label";
      if (o.data_dev || o.len || o.lens_dev) return at + "data_dev / len / lens_dev: RNG_BEGIN takes no data";
      rng = 1;
      continue;
    }
    const bool fills = o.kind == BPP_TOP_RNG_FILL || o.kind == BPP_TOP_RNG_FILL32 || o.kind == BPP_TOP_RNG_SCALARS;
    if (o.label_len > BPP_TOP_LABEL_MAX) return at + "label_len is above " + std::to_string(BPP_TOP_LABEL_MAX);
    if ((fills || o.kind == BPP_TOP_RNG_FINALIZE) && o.label_len)
      return at + "label_len: RNG_FINALIZE / RNG_FILL / RNG_FILL32 / RNG_SCALARS have no label in merlin";
    if (o.len > BPP_TOP_LEN_MAX) return at + "len is above " + std::to_string(BPP_TOP_LEN_MAX);
    if (o.stride < o.len) return at + "stride is below len";
    if (o.stride > ((size_t)1 << 40)) return at + "stride is above 2^40";
    if (!o.data_dev && o.len) return at + "data_dev is null with len > 0";
    if (o.lens_dev && !top_kind_takes_lens(o.kind)) return at + "lens_dev belongs to an APPEND or an RNG_REKEY only";
    if ((o.kind == BPP_TOP_APPEND_POINT || o.kind == BPP_TOP_CHALLENGE_SCALAR) && o.len != 32)
      return at + "len must be 32 (a point's or a scalar's encoding)";
    if (o.kind == BPP_TOP_RNG_FINALIZE && o.len != (o.data_dev ? 32u : 0u))
      return at + "len must be 32 (the external RNG's one draw), or data_dev null with len 0 (NullRng)";
    if ((o.kind == BPP_TOP_RNG_FILL32 || o.kind == BPP_TOP_RNG_SCALARS) && o.len % 32u) return at + "len must be a multiple of 32";
    if (o.kind == BPP_TOP_RNG_REKEY || o.kind == BPP_TOP_RNG_FINALIZE) {
      if (rng != 1) return at + "kind: RNG_REKEY / RNG_FINALIZE need an RNG_BEGIN in front and no RNG_FINALIZE of that RNG between";
      if (o.kind == BPP_TOP_RNG_FINALIZE) rng = 2;
    }
    if (fills && rng != 2) return at + "kind: RNG_FILL / RNG_FILL32 / RNG_SCALARS need a finalised RNG (RNG_BEGIN .. RNG_FINALIZE in front)";
    if (o.data_dev && o.len)
      ranges.push_back(Range{at + "data_dev", (uintptr_t)o.data_dev, (uintptr_t)o.data_dev + (n - 1) * o.stride + o.len, top_kind_writes(o.kind)});
    if (o.lens_dev) ranges.push_back(Range{at + "lens_dev", (uintptr_t)o.lens_dev, (uintptr_t)o.lens_dev + 4 * n, false});
  }
  if (live) ranges.push_back(Range{"live_dev", (uintptr_t)live, (uintptr_t)live + n, false});
  if (done_mask) ranges.push_back(Range{"done_mask_dev", (uintptr_t)done_mask, (uintptr_t)done_mask + n, true});
  if (record) ranges.push_back(Range{"record_dev", (uintptr_t)record, (uintptr_t)record + sizeof(bpp_device_transcripts_record), true});
  for (size_t x = 0; x < ranges.size(); x++)
    for (size_t y = x + 1; y < ranges.size(); y++)
      if ((ranges[x].written || ranges[y].written) && ranges[x].lo < ranges[y].hi && ranges[y].lo < ranges[x].hi)
        return ranges[x].name + " and " + ranges[y].name + " overlap";
  return std::string();
}

// the launch arguments of a call that passed the refusals: the labels are copied, NEW's state is made here
inline void transcript_ops_args(TranscriptOps &a, uint8_t *states, size_t n, const bpp_transcript_op *ops, size_t n_ops, const uint8_t *live,
                                uint8_t *done_mask, bpp_device_transcripts_record *record) {
  memset(&a, 0, sizeof(a));
  a.states = states, a.live = live, a.done_mask = done_mask, a.record = record;
  a.n = (uint32_t)n, a.n_ops = (uint32_t)n_ops;
  for (size_t j = 0; j < n_ops; j++) {
    const bpp_transcript_op &o = ops[j];
    TopOp &t = a.ops[j];
    t.kind = o.kind;
    if (o.kind == BPP_TOP_NEW) {
      Strobe s;
      merlin_new(s, o.label, o.label_len);
      uint8_t b[4 * (BPP_TOP_STATE_WORDS + 1)] = {0};
      strobe_to_bytes(b, s);
      memcpy(a.new_w, b, sizeof(a.new_w));
      continue;
    }
    t.label_len = o.label_len;
    if (o.label_len) memcpy(t.label_w, o.label, o.label_len);
    t.data = o.data_dev, t.stride = o.stride, t.lens = o.lens_dev, t.len = o.len;
  }
}

// k_transcript_ops and the two record kernels on the host: one lane per row on merlin.h's sponge, the same decision, the same bytes read
// which kernel a program runs: k_transcript_ops_rng where it holds a kind beyond NEW / APPEND / CHALLENGE (the kinds are public)
inline bool transcript_ops_extended(const TranscriptOps &a) {
  for (uint32_t j = 0; j < a.n_ops; j++)
    if (top_kind_extended(a.ops[j].kind)) return true;
  return false;
}

// one operation of the extended kinds on the model's sponges, as top_extended_op; wide_hook (tests only, or null) may replace a 64-byte
// draw before it is reduced -- the only way to a zero scalar.  True: a scalar reduced to zero.
typedef void (*top_wide_hook)(uint8_t wide[64], size_t row, uint32_t op, uint32_t draw);
inline bool top_extended_op_host(const TopOp &op, uint32_t j, Strobe &st, Strobe &rng, size_t i, top_wide_hook hook) {
  const uint8_t *label = (const uint8_t *)op.label_w;
  uint8_t *drow = top_data_row(op, i);
  uint8_t wide[64];
  const uint8_t zeros[32] = {0};
  auto scalars = [&](uint32_t count, bool challenge) {
    for (uint32_t k = 0; k < count; k++) {
      if (challenge) merlin_challenge_bytes(st, label, op.label_len, wide, 64);
      else merlin_rng_fill(rng, wide, 64);
      if (hook) hook(wide, i, j, k);
      uint8_t s32[32];
      const uint32_t zero = top_scalar_from_wide(s32, wide);
      if (zero) return true;
      ingest_copy(drow + 32u * k, s32, 32, 0, 1);
    }
    return false;
  };
  switch (op.kind) {
    case BPP_TOP_CHALLENGE_SCALAR: return scalars(1, true);
    case BPP_TOP_RNG_BEGIN: rng = st; break;
    case BPP_TOP_RNG_REKEY: merlin_rng_rekey(rng, label, op.label_len, drow, top_append_len(op, i)); break;
    case BPP_TOP_RNG_FINALIZE: merlin_rng_finalize(rng, op.data ? drow : zeros); break;
    case BPP_TOP_RNG_FILL: merlin_rng_fill(rng, drow, op.len); break;
    case BPP_TOP_RNG_FILL32:
      for (uint32_t off = 0; off < op.len; off += 32) merlin_rng_fill(rng, drow + off, 32);
      break;
    default: return scalars(op.len / 32u, false);  // BPP_TOP_RNG_SCALARS
  }
  return false;
}

template <bool X>
inline void transcript_ops_run_host_t(const TranscriptOps &a, top_wide_hook hook) {
  bpp_device_transcripts_record rec{0u, 0u, 0xffffffffu, 0u};
  const bool fresh = a.ops[0].kind == BPP_TOP_NEW;
  auto count_void = [&](size_t i) {
    rec.n_void++;
    if ((uint32_t)i < rec.first_void) rec.first_void = (uint32_t)i;
  };
  for (size_t i = 0; i < a.n; i++) {
    const uint32_t code = top_row_decide_t<X>(a.states, a.live, a.ops, a.n_ops, i);
    if (code != BPP_TOP_ROW_GO) {
      const bool is_void = code != BPP_TOP_ROW_DEAD;
      top_row_refuse_t<X>(a.states, a.ops, a.n_ops, i, is_void, 0, 1);
      if (a.done_mask) a.done_mask[i] = 0;
      if (is_void) count_void(i);
      if (code == BPP_TOP_ROW_VOID_POINT) rec.flags |= BPP_TOPS_IDENTITY;
      continue;
    }
    uint8_t *row = top_state_row(a.states, i);
    uint8_t b[BPP_ITEM_STATE_BYTES];
    if (fresh) memcpy(b, a.new_w, BPP_ITEM_STATE_BYTES);
    else ingest_copy(b, row, BPP_ITEM_STATE_BYTES, 0, 1);
    Strobe st, rng;
    strobe_from_bytes(st, b);
    rng = st;
    bool zero_scalar = false;
    for (uint32_t j = fresh ? 1u : 0u; j < a.n_ops && !zero_scalar; j++) {
      const TopOp &op = a.ops[j];
      const uint8_t *label = (const uint8_t *)op.label_w;
      if (op.kind == BPP_TOP_APPEND || (X && op.kind == BPP_TOP_APPEND_POINT))
        merlin_append_message(st, label, op.label_len, top_data_row(op, i), top_append_len(op, i));
      else if (!X || op.kind == BPP_TOP_CHALLENGE) merlin_challenge_bytes(st, label, op.label_len, top_data_row(op, i), op.len);
      else zero_scalar = top_extended_op_host(op, j, st, rng, i, hook);
    }
    if (zero_scalar) {
      top_row_refuse_t<X>(a.states, a.ops, a.n_ops, i, true, 0, 1);
      if (a.done_mask) a.done_mask[i] = 0;
      count_void(i);
      rec.flags |= BPP_TOPS_ZERO_SCALAR;
      continue;
    }
    strobe_to_bytes(b, st);
    ingest_copy(row, b, BPP_ITEM_STATE_BYTES, 0, 1);
    if (a.done_mask) a.done_mask[i] = 1;
    rec.n_done++;
  }
  rec.flags |= BPP_TOPS_WRITTEN;
  if (a.record) *a.record = rec;
}
inline void transcript_ops_run_host(const TranscriptOps &a, top_wide_hook hook = nullptr) {
  if (transcript_ops_extended(a)) transcript_ops_run_host_t<true>(a, hook);
  else transcript_ops_run_host_t<false>(a, nullptr);
}

}  // namespace bpp
