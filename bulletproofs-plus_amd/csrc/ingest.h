// Device side of bpp_batch_upload_packed_device and bpp_batch_upload_mixed_device: a batch whose arrays already lie in device memory
// is checked and packed where it lies.  What depends on the data is, per item, the first byte of the proof, the canonicity of t + 2
// scalars, the minimum-value promises and whether a seed nonce is present.  The one-item routines below restate, in the same order,
// what upload_check_item / parse_proof do for item i; the host form throws, these return {code, message id}.
//
// ONE SLOT GEOMETRY, two forms.  Where item i comes from and where it goes is an IngestSlot, and every routine here works on one:
//   packed (ROWS == false): rows of proof_stride bytes, every item proof_len bytes and m entries, so the slot is arithmetic
//     (upload_host.h: upload_plan_packed) and no table is loaded;
//   mixed (ROWS == true): rows of proof_stride bytes and m_stride entries, the used part of every row in the host arrays proof_lens[]
//     and m[].  The destination is the item form's (upload_pass_a): proofs back to back in item order, then the commitments, then
//     BPP_BYTES_SLACK zero bytes; promises at the prefix sum of m.  The host computes that and hands over one IngestMixedRow per item
//     (ingest_mixed.h: the prelude and the plan of this form).
// Packed is the mixed form whose row is arithmetic.  Shared by the kernels (k_ingest_packed, k_ingest_mixed), by the engine's driver
// (engine.hip: upload_device_form) and by the sanitizer harnesses (hosttest_ingest.cpp, hosttest_ingest_mixed.cpp), which run the routines on the
// host against the host packers of upload_host.h.
//
// Split of the checks (lowest-index construction finding wins, as in upload_run_parts):
//   host, no proof byte needed: m a power of two and <= m_max, null fields, lengths and strides, the 4 GB limits (ingest_host_prelude,
//     ingest_mixed_host_prelude; the mixed form finds h, the lowest index with such a finding, and runs items [0, h) only)
//   per item, device: a seed nonce with m > 1; the walk of parse_proof; at item 0 the unusable transcript state; the promises
//   host, behind the run: rounds, rounds_bad and the degree finding from t0 (ingest_finish_plan, ingest_mixed_finish_plan)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bpp.h"
#include "layout.h"
#include "scalar.h"

namespace bpp {

// message ids of the per-item construction findings (texts: ingest_message)
#define BPP_ING_OK 0u
#define BPP_ING_SEED_AGGREGATED 1u
#define BPP_ING_TOO_SHORT 2u
#define BPP_ING_DEGREE 3u
#define BPP_ING_PARSING 4u
#define BPP_ING_UNUSED_DATA 5u
#define BPP_ING_ROUNDS_OVERFLOW 6u
#define BPP_ING_LAYOUT 7u
#define BPP_ING_TRANSCRIPT 8u

// bits of the per-item info byte the kernel leaves
#define BPP_ING_INFO_SEED 1u     // == ProofDesc::flags bit 0
#define BPP_ING_INFO_PROMISE 2u  // == BPP_DEFER_PROMISE

// words of the small result the kernel reduces into (device memory, fetched by one copy)
#define BPP_ING_RES_FINDING 0  // 0xffffffff - (index << 8 | message id) of the lowest-index finding under atomicMax; 0 = none
#define BPP_ING_RES_T0 1       // first byte of proof 0
#define BPP_ING_RES_DIFFERS 2  // some proof's first byte is not t0
#define BPP_ING_RES_ANY_SEED 3
#define BPP_ING_RES_ANY_PROMISE 4
#define BPP_ING_RES_WORDS 8

struct IngestFinding {
  int code;
  uint32_t msg;
};

BPP_HD IngestFinding ingest_finding(uint32_t msg) {
  int code = BPP_OK;
  switch (msg) {
    case BPP_ING_OK: code = BPP_OK; break;
    case BPP_ING_TOO_SHORT:
    case BPP_ING_UNUSED_DATA: code = BPP_ERR_INVALID_LENGTH; break;
    case BPP_ING_ROUNDS_OVERFLOW: code = BPP_ERR_SIZE_OVERFLOW; break;
    case BPP_ING_LAYOUT: code = BPP_ERR_ENGINE; break;
    default: code = BPP_ERR_INVALID_ARGUMENT; break;
  }
  return IngestFinding{code, msg};
}

BPP_HD uint32_t ingest_key(uint32_t index, uint32_t msg) { return 0xffffffffu - ((index << 8) | msg); }  // index < 2^24

// one row of the mixed form's table: the used lengths of item i and where it goes.  Also the batch's resident table (refill.h)
struct IngestMixedRow {
  uint32_t proof_len;   // < 2^32: the size limits
  uint32_t proof_off;   // prefix sum of proof_len = ProofDesc::proof_off
  uint32_t minval_idx;  // prefix sum of m = ProofDesc::minval_idx; the commitments go to proof_bytes + 32 * minval_idx
  uint32_t m;
};

// the batch as the kernel sees it (every array pointer an address in device memory) and where its pieces go
struct Ingest {
  const uint8_t *proofs;
  uint64_t proof_stride;
  const uint8_t *commitments32;
  const uint64_t *min_values;
  const uint8_t *min_present, *seed_nonces32, *seed_present;
  const IngestMixedRow *rows;  // mixed: one per item of the batch; packed: null, and proof_len / m below say it all
  uint64_t proof_len;          // packed only
  uint32_t m, m_stride;        // packed only; mixed only
  uint32_t n_run;              // items [0, n_run) are checked and moved (packed: every item; mixed: h, the host's first finding)
  uint32_t n_bits;
  uint32_t tr_bad;     // the call's transcript state is unusable (pos >= rate): reported at item 0, after its proof parsed
  uint64_t proof_bytes, bytes_total;  // of the WHOLE batch: where the commitments start, where the slack starts
  uint8_t *bytes;      // proof_bytes, then sum(m) * 32 commitment bytes, then BPP_BYTES_SLACK zero bytes
  uint64_t *minvals;   // sum(m)
  uint8_t *seeds;      // 32 per item, or null when seed_nonces32 is
  uint8_t *info;       // one per item: BPP_ING_INFO_*
  uint32_t *result;    // BPP_ING_RES_WORDS words, zero before the run
};

// where item i comes from and where it goes
struct IngestSlot {
  const uint8_t *proof;  // source: the row's first byte (formed, not dereferenced, here)
  size_t proof_len;      // its used length
  size_t proof_off;      // destination offset in bytes
  size_t entry;          // source index of the item's first entry in commitments32 / min_values / min_present
  uint32_t m;
  size_t minval_idx;     // destination index of its first promise; its commitments go to proof_bytes + 32 * minval_idx
};

template <bool ROWS>
BPP_HD IngestSlot ingest_slot(const Ingest &a, size_t i) {
  const uint8_t *p = a.proofs + i * (size_t)a.proof_stride;
  if constexpr (ROWS) {
    const IngestMixedRow r = a.rows[i];
    return IngestSlot{p, r.proof_len, r.proof_off, i * (size_t)a.m_stride, r.m, r.minval_idx};
  } else {
    return IngestSlot{p, (size_t)a.proof_len, i * (size_t)a.proof_len, i * (size_t)a.m, a.m, i * (size_t)a.m};
  }
}

BPP_HD bool ingest_seed_present(const Ingest &a, size_t i) {
  return a.seed_nonces32 && (!a.seed_present || a.seed_present[i]);
}

// the first byte the batch's proofs are compared with: proof 0's, or 0 (no proof has it) when proof 0 is empty -- which only the
// mixed form can see: the packed prelude declines proof_len < 1
template <bool ROWS>
BPP_HD uint32_t ingest_t0(const Ingest &a) {
  return ingest_slot<ROWS>(a, 0).proof_len ? (uint32_t)a.proofs[0] : 0u;
}

// upload_check_item from its first data-dependent check to its last construction error, for item i of a packed batch (`p`:
// proof_len bytes).  parse_proof's need() failures stay between the canonicity checks: a non-canonical d1[0] beats a body that
// is too short for r1.
BPP_HD IngestFinding ingest_check_item(const uint8_t *p, size_t len, uint32_t m, bool seed, bool tr_bad_here) {
  if (seed && m > 1) return ingest_finding(BPP_ING_SEED_AGGREGATED);
  // RangeProof::from_bytes (parse_proof)
  if (len < 1) return ingest_finding(BPP_ING_TOO_SHORT);
  const uint32_t t = p[0];
  if (t < 1 || t > 6) return ingest_finding(BPP_ING_DEGREE);
  const size_t body = len - 1, nchunks = body / 32, rem = body % 32;
  for (size_t k = 0; k < t; k++) {
    if (k >= nchunks) return ingest_finding(BPP_ING_TOO_SHORT);
    if (!sc_is_canonical(p + 1 + 32 * k)) return ingest_finding(BPP_ING_PARSING);
  }
  if ((size_t)t + 2 >= nchunks) return ingest_finding(BPP_ING_TOO_SHORT);  // need(t), need(t + 1), need(t + 2)
  for (size_t k = (size_t)t + 3; k <= (size_t)t + 4; k++) {
    if (k >= nchunks) return ingest_finding(BPP_ING_TOO_SHORT);
    if (!sc_is_canonical(p + 1 + 32 * k)) return ingest_finding(BPP_ING_PARSING);
  }
  const size_t rest = nchunks - ((size_t)t + 5);
  if (rest / 2 == 0) return ingest_finding(BPP_ING_TOO_SHORT);
  if ((rest % 2) || rem) return ingest_finding(BPP_ING_UNUSED_DATA);
  if (rest / 2 > BPP_MAX_WIRE_ROUNDS) return ingest_finding(BPP_ING_ROUNDS_OVERFLOW);
  // the count the layout was sized with (pass A) against the one the proof parsed to
  const size_t laid_out = (nchunks - ((size_t)t + 5)) / 2 < BPP_MAX_WIRE_ROUNDS ? (nchunks - ((size_t)t + 5)) / 2 : BPP_MAX_WIRE_ROUNDS;
  if (rest / 2 != laid_out) return ingest_finding(BPP_ING_LAYOUT);
  if (tr_bad_here) return ingest_finding(BPP_ING_TRANSCRIPT);
  return ingest_finding(BPP_ING_OK);
}

// n bytes from src to dst, shared among `lanes` lanes; neither end is aligned to anything (proof lengths are odd, the caller's
// base may be at any byte).  On the device the middle goes as whole words of the DESTINATION, each put together from the two
// aligned source words it straddles: those lie in the same aligned word as a byte of the source, so inside its page.
// ROW SLACK is therefore never read: sw[w + 1] is read only for a word whose four source bytes all lie inside the n bytes asked for
// (words = (n - head) / 4: the tail goes byte-wise), and it holds the last of those four, so it is the aligned word of a byte of the
// row itself -- never a word that starts behind the row.  That holds for the last row of the array as for any other: the at most
// three bytes of that word beyond the row are shifted out.
BPP_HD void ingest_copy(uint8_t *dst, const uint8_t *src, size_t n, uint32_t lane, uint32_t lanes) {
#if defined(__HIP_DEVICE_COMPILE__)
  size_t head = (size_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
  if (head > n) head = n;
  if (lane < head) dst[lane] = src[lane];
  const size_t words = (n - head) / 4;
  const uint8_t *s = src + head;
  uint32_t *d = reinterpret_cast<uint32_t *>(dst + head);
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3u) * 8u;
  const uint32_t *sw = reinterpret_cast<const uint32_t *>((uintptr_t)s & ~(uintptr_t)3);
  if (sh == 0) {
    for (size_t w = lane; w < words; w += lanes) d[w] = sw[w];
  } else {
    for (size_t w = lane; w < words; w += lanes) d[w] = (sw[w] >> sh) | (sw[w + 1] << (32u - sh));
  }
  const size_t done = head + 4 * words;
  if (lane < n - done) dst[done + lane] = src[done + lane];
#else
  for (size_t k = lane; k < n; k += lanes) dst[k] = src[k];
#endif
}

BPP_HD void ingest_zero(uint8_t *dst, size_t n, uint32_t lane, uint32_t lanes) {
  for (size_t k = lane; k < n; k += lanes) dst[k] = 0;
}

// What `lane` of the `lanes` lanes that share item i moves: proof and commitment bytes to the slot's offsets, the promises (0 where
// not present), the nonce (zero where absent); item 0's lanes also clear the slack behind the last commitment.  Every loop is
// bounded by the slot's own proof_len and m.  Returns this lane's share of the item's info bits.
BPP_HD uint32_t ingest_item_arrays(const Ingest &a, const IngestSlot &sl, size_t i, uint32_t lane, uint32_t lanes) {
  ingest_copy(a.bytes + sl.proof_off, sl.proof, sl.proof_len, lane, lanes);
  ingest_copy(a.bytes + (size_t)a.proof_bytes + 32 * sl.minval_idx, a.commitments32 + 32 * sl.entry, 32 * (size_t)sl.m, lane, lanes);
  if (i == 0) ingest_zero(a.bytes + (size_t)a.bytes_total, BPP_BYTES_SLACK, lane, lanes);
  uint32_t bits = 0;
  for (uint32_t j = lane; j < sl.m; j += lanes) {
    const bool present = a.min_present ? a.min_present[sl.entry + j] != 0 : false;
    const uint64_t v = (present && a.min_values) ? a.min_values[sl.entry + j] : 0;
    if (present && a.n_bits < 64 && (v >> a.n_bits) > 0) bits |= BPP_ING_INFO_PROMISE;
    a.minvals[sl.minval_idx + j] = v;
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

// the check of item i and what it adds to the result words, by the item's first lane.  An empty proof has no first byte to compare
// (ingest_check_item reports it without reading one).
BPP_HD uint32_t ingest_item_check(const Ingest &a, const IngestSlot &sl, size_t i, uint32_t t0, uint32_t *key_out) {
  const IngestFinding f = ingest_check_item(sl.proof, sl.proof_len, sl.m, ingest_seed_present(a, i), a.tr_bad && i == 0);
  *key_out = f.msg ? ingest_key((uint32_t)i, f.msg) : 0u;
  return sl.proof_len ? ((uint32_t)sl.proof[0] ^ t0) : 0u;
}

#if defined(__HIPCC__)
// BPP_INGEST_LANES lanes per proof (the copies are 700-1100 bytes per item), 256-lane blocks, so four items share a wavefront -- in
// the mixed form four items of different lengths and aggregation factors.  The item's first lane runs the check.  The lanes of a
// short item fall through their loops early, and NO lane returns: all 64 reach the width-16 shuffles that fold the info bits across
// an item's lanes, and the ballots (a lane past n_run with zeros).
#define BPP_INGEST_LANES 16u
#define BPP_INGEST_BLOCK 256u
template <bool ROWS>
__device__ __forceinline__ void ingest_kernel_body(const Ingest &a) {
  const size_t gid = (size_t)blockIdx.x * BPP_INGEST_BLOCK + threadIdx.x;
  const size_t i = gid / BPP_INGEST_LANES;
  const uint32_t lane = (uint32_t)(gid % BPP_INGEST_LANES);
  const bool live = i < a.n_run;
  uint32_t bits = 0, differs = 0;
  if (live) {
    const IngestSlot sl = ingest_slot<ROWS>(a, i);
    if (lane == 0) {
      const uint32_t t0 = ingest_t0<ROWS>(a);
      uint32_t key;
      differs = ingest_item_check(a, sl, i, t0, &key);
      if (key) atomicMax(&a.result[BPP_ING_RES_FINDING], key);
      if (i == 0) a.result[BPP_ING_RES_T0] = t0;
    }
    bits = ingest_item_arrays(a, sl, i, lane, BPP_INGEST_LANES);
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
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_ingest_packed(Ingest a) { ingest_kernel_body<false>(a); }
__global__ void __launch_bounds__(BPP_INGEST_BLOCK) k_ingest_mixed(Ingest a) { ingest_kernel_body<true>(a); }
#endif

}  // namespace bpp

// ---- host side: the uniform checks in front of the run, the plan behind it.  Pure host C++ over upload_host.h.
#include "upload_host.h"

namespace bpp {

inline const char *ingest_message(uint32_t msg) {
  switch (msg) {
    case BPP_ING_SEED_AGGREGATED: return "Mask recovery is not supported with an aggregated statement";
    case BPP_ING_TOO_SHORT: return "Serialized proof is too short";
    case BPP_ING_DEGREE: return "Extension degree not valid";
    case BPP_ING_PARSING: return "Invalid parsing";
    case BPP_ING_UNUSED_DATA: return "Unused data after deserialization";
    case BPP_ING_ROUNDS_OVERFLOW: return "Internal size overflow (more than 64 (L, R) pairs)";
    case BPP_ING_LAYOUT: return "internal: layout and parse disagree on the round count";
    case BPP_ING_TRANSCRIPT: return "transcript state has pos >= rate";
    default: return "";
  }
}

// What needs no proof byte, in front of the run.  false: upload_pass_a_packed would decline this batch (the item form: the
// engine stages it and takes the host path).  Throws what item 0 would be the first to report in either host form; the size
// limits are those of pass A, which come before every per-item check.
inline bool ingest_host_prelude(const bpp_packed_batch &pk, const ParamShape &P) {
  const uint64_t n = pk.n_items, proof_bytes = pk.proofs ? n * (uint64_t)pk.proof_len : 0, sum_m = n * (uint64_t)pk.m;
  if ((pk.proofs && pk.proof_len >= (1ull << 32)) || proof_bytes + sum_m * 32 >= (1ull << 32) || sum_m >= (1ull << 28))
    throw ProofErr{BPP_ERR_SIZE_OVERFLOW, "batch too large for one call (4 GB of proof bytes)"};
  if (!pk.proofs || pk.proof_len < 1 || pk.proof_stride < pk.proof_len) return false;
  if (pk.m == 0 || (pk.m & (pk.m - 1))) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "Number of commitments must be a power of two"};
  if (!pk.commitments32 || (!pk.min_values && pk.min_present))
    throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "Incorrect number of minimum value promises"};
  if (P.m_max < pk.m) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "Not enough generators for this statement"};
  return true;
}

inline Ingest ingest_args(const bpp_packed_batch &pk, const ParamShape &P, uint8_t *bytes, uint64_t *minvals, uint8_t *seeds, uint8_t *info,
                          uint32_t *result) {
  Ingest a;
  memset(&a, 0, sizeof(a));
  a.proofs = pk.proofs;
  a.proof_len = pk.proof_len;
  a.proof_stride = pk.proof_stride;
  a.commitments32 = pk.commitments32;
  a.min_values = pk.min_values;
  a.min_present = pk.min_present;
  a.seed_nonces32 = pk.seed_nonces32;
  a.seed_present = pk.seed_present;
  a.m = pk.m;
  a.n_run = (uint32_t)pk.n_items;
  a.proof_bytes = (uint64_t)pk.n_items * pk.proof_len;
  a.bytes_total = a.proof_bytes + (uint64_t)pk.n_items * pk.m * 32;
  a.n_bits = P.n_bits;
  a.tr_bad = (pk.transcript_state && pk.transcript_state[200] >= BPP_STROBE_R) ? 1u : 0u;
  a.bytes = bytes;
  a.minvals = minvals;
  a.seeds = pk.seed_nonces32 ? seeds : nullptr;
  a.info = info;
  a.result = result;
  return a;
}

// does the per-item info have to come back?  Only for the promise findings and for nonces that only some items have
template <class Batch>  // bpp_packed_batch or bpp_mixed_batch
inline bool ingest_needs_info(const Batch &in, const uint32_t *res) {
  return res[BPP_ING_RES_ANY_PROMISE] != 0 || (res[BPP_ING_RES_ANY_SEED] != 0 && in.seed_present != nullptr);
}

// throws the run's construction finding, the one of lowest index, if its result words hold one
inline void ingest_throw_finding(const uint32_t *res) {
  if (!res[BPP_ING_RES_FINDING]) return;
  const uint32_t key = 0xffffffffu - res[BPP_ING_RES_FINDING];
  ProofErr e{ingest_finding(key & 255u).code, ingest_message(key & 255u)};
  e.index = key >> 8;
  throw e;
}

// Behind the run (first bytes all equal): the plan upload_pass_a_packed + upload_pass_b_packed would have made, built
// arithmetically from t0 and the result words; throws the lowest-index construction finding.  `info`: the per-item bytes, or
// null when ingest_needs_info said no.  The plan's promise and nonce arrays stay empty: they are on the device.
inline void ingest_finish_plan(const bpp_packed_batch &pk, const ParamShape &P, const uint32_t *res, const uint8_t *info, UploadPlan &pl) {
  const uint8_t t0 = (uint8_t)res[BPP_ING_RES_T0];
  upload_plan_packed(pk, t0, pl, false);  // (pass A's limits come before pass B's findings)
  ingest_throw_finding(res);
  const size_t n = pk.n_items;
  const uint32_t rounds = pl.packed_rounds, per_dyn = pk.m + 3 + 2 * rounds;
  const uint64_t mn = (uint64_t)pk.m * P.n_bits;
  const uint8_t rounds_bad = rounds >= 32 ? BPP_ERR_SIZE_OVERFLOW : ((1ull << rounds) != mn ? BPP_ERR_INVALID_LENGTH : 0);
  const uint8_t degree = t0 != P.t ? BPP_DEFER_DEGREE : 0;
  const bool promises = res[BPP_ING_RES_ANY_PROMISE] != 0 && info;
  for (size_t i = 0; i < n; i++) {
    ProofDesc &d = pl.desc[i];
    d.proof_off = (uint32_t)(i * pk.proof_len);
    d.rounds = rounds;
    d.m = pk.m;
    d.commit_off = (uint32_t)(pl.proof_bytes + 32 * i * (size_t)pk.m);
    d.minval_idx = (uint32_t)(i * pk.m);
    d.dyn_off = (uint32_t)(i * per_dyn);
    d.flags = !pk.seed_nonces32 ? 0u : (!pk.seed_present ? 1u : (info ? (uint32_t)(info[i] & BPP_ING_INFO_SEED) : 0u));
    pl.rounds_bad[i] = rounds_bad;
    pl.defer[i] = (uint8_t)(degree | (promises ? (info[i] & BPP_ING_INFO_PROMISE) : 0));
  }
  pl.any_seed = res[BPP_ING_RES_ANY_SEED] != 0;
  pl.any_rounds_bad = rounds_bad != 0;
  pl.any_defer = degree != 0 || res[BPP_ING_RES_ANY_PROMISE] != 0;
  pl.uniform_rounds = true;
  pl.rmax = rounds;
  pl.max_mn = (uint32_t)mn;
}

// the run itself on the host, one lane per item, reduced as the kernel reduces: the model the harnesses hold to the host packers
template <bool ROWS>
inline void ingest_run_host(const Ingest &a) {
  for (int w = 0; w < BPP_ING_RES_WORDS; w++) a.result[w] = 0;
  for (size_t i = 0; i < a.n_run; i++) {
    const IngestSlot sl = ingest_slot<ROWS>(a, i);
    const uint32_t t0 = ingest_t0<ROWS>(a);
    uint32_t key;
    const uint32_t differs = ingest_item_check(a, sl, i, t0, &key);
    if (key > a.result[BPP_ING_RES_FINDING]) a.result[BPP_ING_RES_FINDING] = key;
    if (i == 0) a.result[BPP_ING_RES_T0] = t0;
    const uint32_t bits = ingest_item_arrays(a, sl, i, 0, 1);
    a.info[i] = (uint8_t)bits;
    if (differs) a.result[BPP_ING_RES_DIFFERS] |= 1u;
    if (bits & BPP_ING_INFO_SEED) a.result[BPP_ING_RES_ANY_SEED] |= 1u;
    if (bits & BPP_ING_INFO_PROMISE) a.result[BPP_ING_RES_ANY_PROMISE] |= 1u;
  }
}

}  // namespace bpp
