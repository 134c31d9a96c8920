// Host side of a prove call's items: the per-item check every prove entry point applies, and the job-owned copy that
// bpp_prove_submit takes of the caller's items so that the caller's buffers are free when it returns.
// Pure host C++ (no HIP): engine_prove.h / engine_prove_pipe.h use it inside the engine, hosttest_prove_job.cpp drives it under
// AddressSanitizer / UBSan in the CPU test suite.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "upload_host.h"

namespace bpp {

// the rounds of the inner-product argument for an m that passes RangeStatement::init: log2(m x n_bits), rounded up
inline uint32_t prove_rounds_host(const ParamShape &P, uint32_t m) {
  uint32_t rounds = 0;
  while ((1u << rounds) < m * P.n_bits) rounds++;
  return rounds;
}

// the proof length of an item whose m passes RangeStatement::init, 0 otherwise
inline size_t prove_item_len_host(const ParamShape &P, uint32_t m) {
  if (m == 0 || (m & (m - 1)) || P.m_max < m || m * P.n_bits < 2) return 0;
  return 1 + 32 * (size_t)(P.t + 5 + 2 * prove_rounds_host(P, m));
}

// The per-item findings of a prove call, by id (include/bpp.h: BPP_PROVE_MSG_*): the code and the text each one has in every
// prove entry point.  The device form (prove_ingest.h) carries the id in its finding words and status records.
BPP_HD int prove_msg_code(uint32_t msg) {
  switch (msg) {
    case BPP_PROVE_MSG_OK:
    case BPP_PROVE_MSG_EMPTY: return BPP_OK;  // (a slot the live mask of bpp_prove_enqueue switched off: no finding)
    case BPP_PROVE_MSG_BITS:
    case BPP_PROVE_MSG_PROOF_STRIDE:
    case BPP_PROVE_MSG_COMMIT_STRIDE:
    case BPP_PROVE_MSG_RNG_LEN:
    case BPP_PROVE_MSG_VALUE: return BPP_ERR_INVALID_LENGTH;
    case BPP_PROVE_MSG_IDENTITY: return BPP_ERR_VERIFICATION_FAILED;
    case BPP_PROVE_MSG_ENGINE: return BPP_ERR_ENGINE;
    default: return BPP_ERR_INVALID_ARGUMENT;
  }
}

inline const char *prove_msg_text(uint32_t msg) {
  static const char *const text[] = {"",
                                     "Number of commitments must be a power of two",
                                     "Not enough generators for this statement",
                                     "bit_length * aggregation factor must be at least 2",
                                     "proof_stride too small",
                                     "commit_stride too small",
                                     "null witness / statement field",
                                     "Mask recovery is not supported with an aggregated statement",
                                     "not enough external randomness: need (rounds + 3) * 32 bytes",
                                     "Value exceeds bit vector capacity!",
                                     "Minimum value is larger than value",
                                     "blinding factor is not canonical",
                                     "seed nonce is not canonical",
                                     "transcript state has pos >= rate",
                                     "Witness opening is invalid!",
                                     "Identity element cannot be added to the transcript / zero challenge",
                                     "engine fault: see bpp_ctx_last_error",
                                     ""};
  return msg < sizeof(text) / sizeof(text[0]) ? text[msg] : "unknown finding";
}

inline ProofErr prove_err(uint32_t msg) { return ProofErr{prove_msg_code(msg), prove_msg_text(msg)}; }

// The per-item checks come in two parts, in this order.
// PART ONE needs no witness byte: the aggregation factor, the strides, which fields are given (fields_ok: values, blinding factors,
// rng bytes, commitments unless they are to be made, no min_present without min_values), and the length of the external randomness.
// Returns the first finding's id, 0 for none.  prove_item_check_host runs it on an item; bpp_prove_openings_device runs it per
// item from m[] and the call's strides and array pointers alone, and an item it fails never reaches the device.
inline uint32_t prove_item_layout_finding(const ParamShape &P, uint32_t m, size_t proof_stride, bool openings, size_t commit_stride,
                                          bool fields_ok) {
  if (m == 0 || (m & (m - 1))) return BPP_PROVE_MSG_POWER_OF_TWO;
  if (P.m_max < m) return BPP_PROVE_MSG_GENERATORS;
  if (m * P.n_bits < 2) return BPP_PROVE_MSG_BITS;
  if (proof_stride < prove_item_len_host(P, m)) return BPP_PROVE_MSG_PROOF_STRIDE;
  if (openings && commit_stride < (size_t)32 * m) return BPP_PROVE_MSG_COMMIT_STRIDE;
  if (!fields_ok) return BPP_PROVE_MSG_NULL_FIELD;
  return BPP_PROVE_MSG_OK;
}
inline uint32_t prove_item_rng_finding(const ParamShape &P, uint32_t m, size_t rng_len) {
  return rng_len < 32 * (size_t)(prove_rounds_host(P, m) + 3) ? BPP_PROVE_MSG_RNG_LEN : BPP_PROVE_MSG_OK;
}

// the host-side checks of a one-item bpp_prove_batch on `it`, in the same order and with the same codes and messages.
// openings: an item of bpp_prove_openings / bpp_prove_pool_openings, which may come without commitments and whose commitments go
// to a slot of commit_stride bytes.  Nothing behind a pointer is read before the checks of m and of the pointers have passed.
// PART TWO, what reads witness bytes (a nonce on an aggregated item, the values and promises, the blinding factors, the nonce), is
// restated for arrays in device memory by prove_ingest.h (prove_ingest_check); hosttest_prove_ingest.cpp holds the two to each other.
// There the "Mask recovery is not supported..." finding comes AFTER the rng length: the host cannot see which items carry a nonce.
inline void prove_item_check_host(const ParamShape &P, const bpp_prove_item &it, size_t proof_stride, bool openings, size_t commit_stride) {
  const uint32_t n = P.n_bits, t = P.t, m = it.m;
  const bool fields_ok = it.values && it.blindings32 && (it.commitments32 || openings) && it.rng_bytes && (it.min_values || !it.min_present);
  if (const uint32_t f = prove_item_layout_finding(P, m, proof_stride, openings, commit_stride, fields_ok)) throw prove_err(f);
  if (it.seed_nonce32 && m > 1) throw prove_err(BPP_PROVE_MSG_SEED_AGGREGATED);
  if (const uint32_t f = prove_item_rng_finding(P, m, it.rng_len)) throw prove_err(f);
  for (uint32_t j = 0; j < m; j++) {
    if (n < 64 && (it.values[j] >> n) > 0) throw prove_err(BPP_PROVE_MSG_VALUE);
    const bool present = it.min_present ? it.min_present[j] != 0 : false;
    if (present && it.values[j] < it.min_values[j]) throw prove_err(BPP_PROVE_MSG_MINIMUM);
  }
  for (uint32_t q = 0; q < m * t; q++)
    if (!sc_is_canonical(it.blindings32 + 32 * (size_t)q)) throw prove_err(BPP_PROVE_MSG_BLINDING);
  if (it.seed_nonce32 && !sc_is_canonical(it.seed_nonce32)) throw prove_err(BPP_PROVE_MSG_SEED_NONCE);
  if (it.transcript_state && it.transcript_state[200] >= BPP_STROBE_R) throw prove_err(BPP_PROVE_MSG_TRANSCRIPT_STATE);
}

// What a ticket of the prove pipeline owns of its caller's items.  take() checks every item where the caller keeps it and copies
// the ones that pass -- everything they point to, in ONE buffer -- so that nothing of the caller's is read after it returns; the
// outcome of the ones that fail is recorded and they are never looked at again.  The buffer holds witness bytes (values, blinding
// factors, seed nonces, rng bytes) beside public ones; wipe() zeroes all of it, and so does the destructor.
struct ProveJobCopy {
  size_t n_items = 0;
  std::vector<uint32_t> m;          // per item of the caller: its aggregation factor as given
  std::vector<size_t> len;          // per item of the caller: prove_item_len_host (0 for an m no statement can have)
  std::vector<int> code;            // per item of the caller: BPP_OK, or what the check found
  std::vector<std::string> msg;
  std::vector<bpp_prove_item> items;  // the items that passed, in the caller's order, pointing into `store`
  std::vector<uint32_t> index;        // their places in the caller's array
  std::vector<uint64_t> store;        // (words: the copied values keep their alignment)
  size_t store_bytes = 0;

  ProveJobCopy() = default;
  ProveJobCopy(const ProveJobCopy &) = delete;
  ProveJobCopy &operator=(const ProveJobCopy &) = delete;
  ~ProveJobCopy() { wipe(); }

  uint8_t *bytes() { return reinterpret_cast<uint8_t *>(store.data()); }
  const uint8_t *bytes() const { return reinterpret_cast<const uint8_t *>(store.data()); }

  void wipe() {
    secure_wipe(store.data(), store.size() * sizeof(uint64_t));
    for (bpp_prove_item &it : items) memset(&it, 0, sizeof(it));
  }

  static size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

  // the bytes prove_uniform reads of a passing item's external randomness: (rounds + 3) draws (rng_len may be longer)
  static size_t rng_need(const ParamShape &P, uint32_t m) { return 32 * (size_t)(prove_rounds_host(P, m) + 3); }

  // the same transcript source as the previous item (one label or state buffer for the whole call, the common case): the copy is
  // shared, so that the prover still sees one source
  static bool same_transcript(const bpp_prove_item &a, const bpp_prove_item &b) {
    return a.transcript_state == b.transcript_state && a.transcript_label == b.transcript_label && a.label_len == b.label_len;
  }

  void take(const ParamShape &P, const bpp_prove_item *src, size_t n, size_t proof_stride, bool openings, size_t commit_stride) {
    n_items = n;
    m.assign(n, 0);
    len.assign(n, 0);
    code.assign(n, BPP_OK);
    msg.assign(n, std::string());
    items.clear();
    index.clear();
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
      const bpp_prove_item &it = src[i];
      m[i] = it.m;
      len[i] = prove_item_len_host(P, it.m);
      try {
        prove_item_check_host(P, it, proof_stride, openings, commit_stride);
      } catch (const ProofErr &e) {
        code[i] = e.code;
        msg[i] = e.msg;
        continue;
      }
      const bool shared = !index.empty() && same_transcript(src[index.back()], it);
      index.push_back((uint32_t)i);
      const size_t mi = it.m;
      total += pad8(8 * mi) + pad8(32 * mi * P.t) + pad8(rng_need(P, it.m));
      if (it.commitments32) total += pad8(32 * mi);
      if (it.min_values) total += pad8(8 * mi);
      if (it.min_present) total += pad8(mi);
      if (it.seed_nonce32) total += 32;
      if (!shared) total += it.transcript_state ? pad8(203) : (it.transcript_label ? pad8(it.label_len) : 0);
    }
    store.assign(total / 8 + 1, 0);  // (never empty: a zero-length label still gets a pointer that is not null)
    store_bytes = total;
    items.resize(index.size());
    size_t at = 0;
    auto put = [&](const void *p, size_t bytes_n) -> uint8_t * {
      uint8_t *dst = bytes() + at;
      if (bytes_n) memcpy(dst, p, bytes_n);
      at += pad8(bytes_n);
      return dst;
    };
    for (size_t k = 0; k < index.size(); k++) {
      const bpp_prove_item &it = src[index[k]];
      bpp_prove_item &o = items[k];
      memset(&o, 0, sizeof(o));
      const size_t mi = it.m;
      o.m = it.m;
      o.values = reinterpret_cast<const uint64_t *>(put(it.values, 8 * mi));
      o.blindings32 = put(it.blindings32, 32 * mi * P.t);
      if (it.commitments32) o.commitments32 = put(it.commitments32, 32 * mi);
      if (it.min_values) o.min_values = reinterpret_cast<const uint64_t *>(put(it.min_values, 8 * mi));
      if (it.min_present) o.min_present = put(it.min_present, mi);
      if (it.seed_nonce32) o.seed_nonce32 = put(it.seed_nonce32, 32);
      if (k && same_transcript(src[index[k - 1]], it)) {
        o.transcript_state = items[k - 1].transcript_state;
        o.transcript_label = items[k - 1].transcript_label;
        o.label_len = items[k - 1].label_len;
      } else if (it.transcript_state) {
        o.transcript_state = put(it.transcript_state, 203);
      } else if (it.transcript_label) {
        o.transcript_label = put(it.transcript_label, it.label_len);
        o.label_len = it.label_len;
      }
      o.rng_len = rng_need(P, it.m);
      o.rng_bytes = put(it.rng_bytes, o.rng_len);
    }
  }
};

}  // namespace bpp
