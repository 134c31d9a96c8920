// Host side of a prove call's witness: the packer that turns the caller's items into what the prover's kernels read -- one
// descriptor per proof, one block of witness bytes, the distinct transcript states, the minimum-value rows and the ragged
// schedule's offsets.  It is the one routine of the prover that copies caller-owned SECRET bytes by computed offsets.
// Pure host C++ (no HIP): engine_prove.h packs every call with it, hosttest_prove_job.cpp drives it under AddressSanitizer /
// UBSan and hosttest.cpp exposes it to the CPU test suite, which recomputes offsets, bytes and states on its own.
#pragma once
#include <map>

#include "prove_job_host.h"

namespace bpp {

struct ProvePack {
  std::vector<ProveDesc> desc;    // per proof, call order; offsets into `bytes` as a whole
  std::vector<uint8_t> bytes;     // per proof: (v LE64 || r[0..t)) per opening, m commitments, (rounds + 3) x 32 rng bytes, seed slot
  std::vector<uint8_t> states;    // the distinct transcripts, 203 bytes each, advanced by the call-level appends
  std::vector<uint64_t> minvals;  // rows of `m` per proof
  std::vector<uint8_t> minpres;
  std::vector<uint32_t> roff;     // ProveDesc::roff per proof
  uint32_t m = 0;                 // items[0].m: the call's largest (a uniform call: every item's)
  uint32_t rounds = 0;            // its rounds: the call's global steps
  uint32_t rounds_min = 0;        // the smallest class's rounds: "ct" = 2's ex_back is clamped to it
  size_t plen = 0;                // the longest proof
  size_t bytes_len = 0;           // bytes.size(), or what the ingest kernel writes on the device where `bytes` stays empty (prove_ingest.h)
  bool packed = false;            // `bytes` may hold secrets

  ProvePack() = default;
  ProvePack(const ProvePack &) = delete;
  ProvePack &operator=(const ProvePack &) = delete;
  ~ProvePack() { wipe(); }

  // `bytes` holds values, blinding factors and seed nonces.  (Once per pack: the prover wipes early, behind the events that say
  // the staging has been read, and the destructor does not pay for the same megabytes again on the caller's clock.)
  void wipe() {
    if (packed) secure_wipe(bytes.data(), bytes.size());
    packed = false;
  }

  // RangeStatement::init (src/range_statement.rs:43-62) and RangeWitness construction (src/range_proof.rs:238-311) for every
  // item, in call order: an item is checked (prove_item_check_host: the routine every prove entry point applies) and THEN
  // copied, so nothing behind the pointers of an item that fails is read; the first finding is thrown.  The strides are the
  // caller's business (they say nothing about the witness): the check runs without them.
  // hg32: the parameters' H and G bases, (t + 1) x 32 bytes.  mixed: the items may differ in m, sorted largest first.
  // openings: an item may come without commitments (its slot is zero and flagged PV_FLAG_MAKE_COMMITMENTS).
  void pack(const ParamShape &P, const uint8_t *hg32, const bpp_prove_item *items, size_t n_items, bool mixed, bool openings) {
    const uint32_t t = P.t, B = (uint32_t)n_items;
    packed = true;
    m = items[0].m;
    plen = prove_item_len_host(P, m);  // (0: items[0] fails its check below, before anything is sized by m)
    rounds = rounds_min = plen ? prove_rounds_host(P, m) : 0;
    desc.assign(B, ProveDesc{});
    roff.assign(B, 0);
    std::vector<uint32_t> state_m;  // the aggregation factor each distinct transcript state is for (its "M" append)
    std::map<std::string, uint32_t> state_ids;
    for (uint32_t i = 0; i < B; i++) {
      const bpp_prove_item &it = items[i];
      ProveDesc &d = desc[i];
      if (i && !mixed && it.m != m) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "all items of one prove batch must share the aggregation factor"};
      if (i && mixed && (it.m == 0 || (it.m & (it.m - 1)) || it.m > items[i - 1].m))
        throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "mixed prove batch: items must be sorted by aggregation factor"};
      prove_item_check_host(P, it, SIZE_MAX, openings, SIZE_MAX);
      if (i == 0) {
        minvals.assign((size_t)B * m, 0);
        minpres.assign((size_t)B * m, 0);
        bytes.reserve((size_t)B * (m * (8 + 32 * t) + 32 * m + 32 * (rounds + 3) + 32));
      }
      const uint32_t mi = it.m, rounds_i = prove_rounds_host(P, mi);
      d.m = mi;
      d.mslot = m;
      d.roff = roff[i] = rounds - rounds_i;
      rounds_min = std::min(rounds_min, rounds_i);
      d.minval_idx = i * m;
      for (uint32_t j = 0; j < mi; j++) {
        const bool present = it.min_present ? it.min_present[j] != 0 : false;
        minvals[(size_t)i * m + j] = present ? it.min_values[j] : 0;
        minpres[(size_t)i * m + j] = present ? 1 : 0;
      }
      d.wit_off = (uint32_t)bytes.size();
      for (uint32_t j = 0; j < mi; j++) {
        uint8_t v8[8];
        for (int k = 0; k < 8; k++) v8[k] = (uint8_t)(it.values[j] >> (8 * k));
        bytes.insert(bytes.end(), v8, v8 + 8);
        bytes.insert(bytes.end(), it.blindings32 + (size_t)j * t * 32, it.blindings32 + (size_t)(j + 1) * t * 32);
      }
      d.commit_off = (uint32_t)bytes.size();
      if (it.commitments32) bytes.insert(bytes.end(), it.commitments32, it.commitments32 + (size_t)mi * 32);
      else bytes.insert(bytes.end(), (size_t)mi * 32, 0);  // (to be made: kp_adopt_commitments writes them here)
      d.ext_off = (uint32_t)bytes.size();
      bytes.insert(bytes.end(), it.rng_bytes, it.rng_bytes + 32 * (size_t)(rounds_i + 3));
      d.seed_off = (uint32_t)bytes.size();
      d.flags = (it.seed_nonce32 ? 1u : 0u) | (it.commitments32 ? 0u : PV_FLAG_MAKE_COMMITMENTS);
      if (it.seed_nonce32) bytes.insert(bytes.end(), it.seed_nonce32, it.seed_nonce32 + 32);
      else bytes.insert(bytes.end(), 32, 0);
      // the same transcript source as the previous item (the common case: one label for the whole call): same id, no key, no lookup
      if (i && ProveJobCopy::same_transcript(items[i - 1], it) && items[i - 1].m == it.m) {
        d.state_idx = desc[i - 1].state_idx;
        continue;
      }
      std::string key;
      if (it.transcript_state) {
        key.assign((const char *)it.transcript_state, 203);
        key.push_back('S');
      } else {
        if (it.transcript_label) key.assign((const char *)it.transcript_label, it.label_len);
        key.push_back('L');
      }
      key.append((const char *)&mi, sizeof(mi));  // (the state continues with "M" = this proof's aggregation factor)
      auto sit = state_ids.find(key);
      if (sit == state_ids.end()) {
        const uint32_t id = (uint32_t)(states.size() / 203);
        states.resize(states.size() + 203);
        state_m.push_back(mi);
        if (it.transcript_state) {
          memcpy(&states[(size_t)id * 203], it.transcript_state, 203);
        } else {
          Strobe st;
          merlin_new(st, it.transcript_label, (uint32_t)(it.transcript_label ? it.label_len : 0));
          strobe_to_bytes(&states[(size_t)id * 203], st);
        }
        sit = state_ids.emplace(key, id).first;
      }
      d.state_idx = sit->second;
    }

    bytes_len = bytes.size();
    advance_states(P, hg32, state_m);
  }

  // state_m: the aggregation factor each distinct transcript state is for (its "M" append)
  void advance_states(const ParamShape &P, const uint8_t *hg32, const std::vector<uint32_t> &state_m) {
    const uint32_t t = P.t;
    // RangeProofTranscript::new (src/transcripts.rs:59-89) starts every proof's transcript with the same seven appends -- the
    // domain separator, H, the G bases, N, T, M: parameters of the call, not of the proof.  They are applied HERE, once per distinct
    // caller transcript; kp_init continues with the proof's own commitments and promises (two Keccak-f fewer per proof on the call's
    // first stretch, where no fixed-base MSM runs yet).
    for (size_t id = 0; id < states.size() / 203; id++) {
      Strobe st;
      strobe_from_bytes(st, &states[id * 203]);
      merlin_append_message(st, (const uint8_t *)"dom-sep", 7, (const uint8_t *)"Bulletproofs+ Range Proof", 25);
      merlin_append_message(st, (const uint8_t *)"H", 1, hg32, 32);
      for (uint32_t k = 0; k < t; k++) merlin_append_message(st, (const uint8_t *)"G", 1, hg32 + (size_t)(k + 1) * 32, 32);
      merlin_append_u64(st, (const uint8_t *)"N", 1, P.n_bits);
      merlin_append_u64(st, (const uint8_t *)"T", 1, t);
      merlin_append_u64(st, (const uint8_t *)"M", 1, state_m[id]);
      strobe_to_bytes(&states[id * 203], st);
    }
  }
};

}  // namespace bpp
