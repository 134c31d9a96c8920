// Sanitizer harness (CPU test suite only): the one-item routines of ingest.h -- what k_ingest_packed runs per proof of a packed
// batch that lies in device memory -- run on the host over a corpus and are held to the host packer of upload_host.h: for every
// case {code, message text, index} equal those of upload_pass_a_packed + upload_pass_b_packed (or of the item form where pass A
// declines), and on success the descriptors (flags included), promises, nonces, staged bytes, rounds_bad and defer are equal.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_ingest_host.py runs; every input array is an
// exact-size heap allocation, so a read past the end of untrusted input is an ASan report.  Prints one "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "ingest.h"

using namespace bpp;

namespace {

std::mt19937_64 rng(20261020);

const ParallelFor serial_for = [](uint32_t n, const std::function<void(uint32_t)> &fn) {
  for (uint32_t i = 0; i < n; i++) fn(i);
};

void canonical_scalar(uint8_t *p) {
  for (int i = 0; i < 32; i++) p[i] = (uint8_t)rng();
  p[31] &= 0x0f;  // < 2^252 < l
}

// wire bytes with the structure of a proof: [t] d1[t] A A1 B r1 s1 (L R)*rounds; points are random bytes (not looked at here)
std::vector<uint8_t> make_proof(uint32_t t, uint32_t rounds) {
  std::vector<uint8_t> p(1 + 32 * (size_t)(t + 5 + 2 * (size_t)rounds));
  p[0] = (uint8_t)t;
  for (size_t i = 1; i < p.size(); i++) p[i] = (uint8_t)rng();
  for (uint32_t k = 0; k < t; k++) canonical_scalar(&p[1 + 32 * k]);
  canonical_scalar(&p[1 + 32 * (t + 3)]);
  canonical_scalar(&p[1 + 32 * (t + 4)]);
  return p;
}

// l, l - 1, 2^255, all ones
void edge_scalar(int which, uint8_t out[32]) {
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  memcpy(out, L, 32);
  if (which == 1) out[0] = 0xec;
  if (which == 2) {
    memset(out, 0, 32);
    out[31] = 0x80;
  }
  if (which == 3) memset(out, 0xff, 32);
}

// a packed batch that owns exact-size copies of its arrays
struct Case {
  size_t n = 0, len = 0, stride = 0;
  uint32_t m = 1;
  std::unique_ptr<uint8_t[]> proofs, commits, present, seeds, seed_present;
  std::unique_ptr<uint64_t[]> minv;
  std::vector<uint8_t> state;
  bpp_packed_batch pk;

  Case(const std::vector<std::vector<uint8_t>> &items, uint32_t m_, size_t extra_stride = 0) : n(items.size()), m(m_) {
    len = items.empty() ? 0 : items[0].size();
    stride = len + extra_stride;
    const size_t extent = n ? (n - 1) * stride + len : 0;
    proofs.reset(new uint8_t[extent ? extent : 1]);
    memset(proofs.get(), 0xee, extent);
    for (size_t i = 0; i < n && len; i++) memcpy(proofs.get() + i * stride, items[i].data(), len);
    commits.reset(new uint8_t[32 * n * m + 1]);
    for (size_t i = 0; i < 32 * n * m; i++) commits[i] = (uint8_t)rng();
    memset(&pk, 0, sizeof(pk));
    pk.n_items = n;
    pk.proofs = proofs.get();
    pk.proof_len = len;
    pk.proof_stride = stride;
    pk.commitments32 = commits.get();
    pk.m = m;
    pk.transcript_label = (const uint8_t *)"harness";
    pk.label_len = 7;
  }
  void promises(const std::vector<uint64_t> &v, const std::vector<uint8_t> &p) {
    minv.reset(new uint64_t[n * m]);
    present.reset(new uint8_t[n * m]);
    for (size_t q = 0; q < n * m; q++) {
      minv[q] = v[q % v.size()];
      present[q] = p[q % p.size()];
    }
    pk.min_values = minv.get();
    pk.min_present = present.get();
  }
  void nonces(const std::vector<uint8_t> *which) {  // null: every item has one
    seeds.reset(new uint8_t[32 * n]);
    for (size_t i = 0; i < 32 * n; i++) seeds[i] = (uint8_t)(rng() | 1);
    pk.seed_nonces32 = seeds.get();
    if (which) {
      seed_present.reset(new uint8_t[n]);
      for (size_t i = 0; i < n; i++) seed_present[i] = (*which)[i % which->size()];
      pk.seed_present = seed_present.get();
    }
  }
  void bad_state() {
    state.assign(203, 0x5a);
    state[200] = (uint8_t)BPP_STROBE_R;  // pos >= rate
    pk.transcript_state = state.data();
  }
};

struct Outcome {
  int code = 0;
  std::string msg;
  uint32_t index = 0;
  bool fallback = false;  // (model only) the engine would stage the arrays and take the host path
  UploadPlan pl;
  std::vector<uint8_t> bytes, seeds;
  std::vector<uint64_t> minvals;
};

// the host packer, as upload_host_pack drives it; *declined: pass A sent the batch through the item form
void expected(const bpp_packed_batch &pk, const ParamShape &P, Outcome &o, bool *declined) {
  try {
    std::vector<bpp_verify_item> synth;
    const bool arithmetic = upload_pass_a_packed(pk, o.pl, serial_for);
    *declined = !arithmetic;
    if (!arithmetic) {
      upload_packed_as_items(pk, synth);
      upload_pass_a(synth.data(), synth.size(), o.pl);
    }
    o.bytes.assign(o.pl.bytes_total + BPP_BYTES_SLACK, 0xcd);
    memset(o.bytes.data() + o.pl.bytes_total, 0, BPP_BYTES_SLACK);
    if (arithmetic) upload_pass_b_packed(pk, P, o.pl, o.bytes.data(), serial_for);
    else upload_pass_b(synth.data(), P, o.pl, o.bytes.data(), serial_for);
    o.seeds = o.pl.seeds;
    o.minvals = o.pl.minvals;
  } catch (const ProofErr &e) {
    o.code = e.code;
    o.msg = e.msg;
    o.index = e.index;
  }
}

// the device form with the host standing in for the kernel: prelude, the one-item routines over every item, the plan
void model(const bpp_packed_batch &pk, const ParamShape &P, Outcome &o) {
  try {
    if (!ingest_host_prelude(pk, P)) {
      o.fallback = true;
      return;
    }
    const size_t n = pk.n_items, bytes_total = n * pk.proof_len + n * (size_t)pk.m * 32;
    // exact sizes: a write past the end of what the engine allocates is an ASan report
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[bytes_total + BPP_BYTES_SLACK]), seeds(new uint8_t[pk.seed_nonces32 ? n * 32 : 1]),
        info(new uint8_t[n]);
    std::unique_ptr<uint64_t[]> minvals(new uint64_t[n * pk.m]);
    memset(bytes.get(), 0xcd, bytes_total + BPP_BYTES_SLACK);
    uint32_t res[BPP_ING_RES_WORDS];
    const Ingest a = ingest_args(pk, P, bytes.get(), minvals.get(), seeds.get(), info.get(), res);
    ingest_run_host<false>(a);
    if (res[BPP_ING_RES_DIFFERS]) {
      o.fallback = true;
      return;
    }
    ingest_finish_plan(pk, P, res, ingest_needs_info(pk, res) ? info.get() : nullptr, o.pl);
    o.bytes.assign(bytes.get(), bytes.get() + bytes_total + BPP_BYTES_SLACK);
    o.minvals.assign(minvals.get(), minvals.get() + n * pk.m);
    if (pk.seed_nonces32) o.seeds.assign(seeds.get(), seeds.get() + n * 32);
  } catch (const ProofErr &e) {
    o.code = e.code;
    o.msg = e.msg;
    o.index = e.index;
  }
}

bool same_plan(const Outcome &h, const Outcome &d, size_t n) {
  const UploadPlan &a = h.pl, &b = d.pl;
  return a.desc.size() == n && b.desc.size() == n && memcmp(a.desc.data(), b.desc.data(), n * sizeof(ProofDesc)) == 0 &&
         h.minvals == d.minvals && h.seeds == d.seeds && h.bytes == d.bytes && a.states == b.states && a.defer == b.defer &&
         a.rounds_bad == b.rounds_bad && a.total_dyn == b.total_dyn && a.rmax == b.rmax && a.max_mn == b.max_mn &&
         a.any_seed == b.any_seed && a.any_defer == b.any_defer && a.any_rounds_bad == b.any_rounds_bad &&
         a.uniform_rounds == b.uniform_rounds && a.sum_m == b.sum_m && a.proof_bytes == b.proof_bytes && a.bytes_total == b.bytes_total &&
         a.tr_err_index == b.tr_err_index;
}

// one item of pk as a packed batch of its own (what the one-item routine is held to when the whole batch takes the item form)
bpp_packed_batch single(const bpp_packed_batch &pk, size_t i) {
  bpp_packed_batch s = pk;
  s.n_items = 1;
  s.proofs = pk.proofs + i * pk.proof_stride;
  s.commitments32 = pk.commitments32 ? pk.commitments32 + 32 * i * (size_t)pk.m : nullptr;
  s.min_values = pk.min_values ? pk.min_values + i * (size_t)pk.m : nullptr;
  s.min_present = pk.min_present ? pk.min_present + i * (size_t)pk.m : nullptr;
  s.seed_nonces32 = pk.seed_nonces32 ? pk.seed_nonces32 + 32 * i : nullptr;
  s.seed_present = pk.seed_present ? pk.seed_present + i : nullptr;
  return s;
}

int fails = 0, checked = 0;
const char *why = "";

bool agree(const bpp_packed_batch &pk, const ParamShape &P, int depth = 0) {
  Outcome h, d;
  bool declined = false;
  expected(pk, P, h, &declined);
  model(pk, P, d);
  checked++;
  if (d.fallback) {
    // the engine takes the host path with the staged arrays: nothing of the device form decides the outcome.  It must be a batch
    // pass A declines as well; its items, one at a time, still hold the one-item routine to the item form
    if (!declined) return why = "model falls back where pass A does not decline", false;
    if (depth == 0 && pk.proofs && pk.proof_len >= 1 && pk.proof_stride >= pk.proof_len && pk.n_items > 1)
      for (size_t i = 0; i < pk.n_items; i++)
        if (!agree(single(pk, i), P, 1)) return false;
    return true;
  }
  if (declined) return why = "pass A declines where the model does not", false;
  if (h.code != d.code || h.msg != d.msg || h.index != d.index) {
    printf("   host {%d, \"%s\", %u}  model {%d, \"%s\", %u}\n", h.code, h.msg.c_str(), h.index, d.code, d.msg.c_str(), d.index);
    return why = "findings differ", false;
  }
  if (h.code == 0 && !same_plan(h, d, pk.n_items)) return why = "plans differ", false;
  return true;
}

#define EXPECT(name, cond)                                      \
  do {                                                          \
    if (cond) {                                                 \
      printf("ok %s\n", name);                                  \
    } else {                                                    \
      printf("FAIL %s (line %d): %s\n", name, __LINE__, why);   \
      fails++;                                                  \
    }                                                           \
  } while (0)

// what a case must come to on BOTH sides (so that a corpus that silently stopped failing is noticed)
bool outcome_is(const bpp_packed_batch &pk, const ParamShape &P, int code, const char *msg, uint32_t index) {
  Outcome h;
  bool declined;
  expected(pk, P, h, &declined);
  if (h.code != code || h.index != index || (msg && h.msg != msg)) {
    printf("   host {%d, \"%s\", %u}, wanted {%d, \"%s\", %u}\n", h.code, h.msg.c_str(), h.index, code, msg ? msg : "", index);
    return why = "the host form's outcome is not the one the case is about", false;
  }
  return agree(pk, P);
}

}  // namespace

int main() {
  const ParamShape P64{64, 8, 1}, P64t3{64, 4, 3}, P8{8, 2, 1}, P16t2{16, 4, 2};
  for (uint32_t t : {1u, 3u}) {  // every truncation of a valid proof, alone and behind a sound-length neighbour of the same length
    const ParamShape &P = t == 1 ? P64 : P64t3;
    const std::vector<uint8_t> full = make_proof(t, 6);
    bool all = true;
    for (size_t len = 0; len <= full.size() && all; len++) {
      std::vector<uint8_t> cut(full.begin(), full.begin() + len);
      Case one({cut}, 1), three({cut, cut, cut}, 1, 5);
      all = agree(one.pk, P) && agree(three.pk, P);
      // ... and with a non-canonical d1[0] under the same cut: it beats a body too short for r1
      if (all && len >= 33) {
        std::vector<uint8_t> bad = cut;
        edge_scalar(0, &bad[1]);
        Case two({bad, cut}, 1);
        all = outcome_is(two.pk, P, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 0);
      }
    }
    EXPECT(t == 1 ? "truncations_t1" : "truncations_t3", all);
  }
  {  // first byte 0 and 7: every proof, and one proof of the batch (the mixed case: the item form)
    bool all = true;
    for (uint8_t b : {(uint8_t)0, (uint8_t)7}) {
      std::vector<uint8_t> p = make_proof(1, 6), q = p;
      q[0] = b;
      Case every({q, q, q}, 1), one({q}, 1), mixed({p, q, p}, 1);
      all = all && outcome_is(every.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Extension degree not valid", 0) && agree(one.pk, P64) &&
            outcome_is(mixed.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Extension degree not valid", 1);
    }
    EXPECT("first_byte_0_and_7", all);
  }
  for (uint32_t t : {1u, 3u}) {  // l, l - 1, 2^255, all ones in each of d1[k], r1, s1: alone, in pairs inside one proof, across two proofs
    const ParamShape &P = t == 1 ? P64 : P64t3;
    std::vector<uint32_t> fields;
    for (uint32_t k = 0; k < t; k++) fields.push_back(k);
    fields.push_back(t + 3);
    fields.push_back(t + 4);
    const std::vector<uint8_t> good = make_proof(t, 6);
    bool all = true;
    for (size_t f = 0; f < fields.size(); f++)
      for (int v = 0; v < 4; v++) {
        std::vector<uint8_t> bad = good;
        edge_scalar(v, &bad[1 + 32 * fields[f]]);
        Case c({good, good, bad, good}, 1);
        all = all && (v == 1 ? outcome_is(c.pk, P, 0, nullptr, 0) : outcome_is(c.pk, P, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 2));
        for (size_t g = f + 1; g < fields.size(); g++)
          for (int w = 0; w < 4; w++) {
            std::vector<uint8_t> both = bad, other = good;
            edge_scalar(w, &both[1 + 32 * fields[g]]);
            edge_scalar(w, &other[1 + 32 * fields[g]]);
            Case in_one({good, good, both, good}, 1), in_two({good, other, bad, good}, 1, 7);
            all = all && agree(in_one.pk, P) && agree(in_two.pk, P);
            if (v != 1 && w != 1) all = all && outcome_is(in_two.pk, P, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 1);
          }
      }
    EXPECT(t == 1 ? "edge_scalars_t1" : "edge_scalars_t3", all);
  }
  {  // 64 (L, R) pairs are laid out (and refused at verify time), 65 are refused here
    Case c64({make_proof(1, 6 + 58), make_proof(1, 64)}, 1), c65({make_proof(1, 65), make_proof(1, 65)}, 1);
    EXPECT("wire_rounds_64_and_65", outcome_is(c64.pk, P64, 0, nullptr, 0) &&
                                        outcome_is(c65.pk, P64, BPP_ERR_SIZE_OVERFLOW, "Internal size overflow (more than 64 (L, R) pairs)", 0));
  }
  {  // a seed nonce with m = 2: every item; only item 3, behind a non-canonical s1 in item 2 (index 2 wins); no item after all
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 5; i++) items.push_back(make_proof(1, 7));
    Case every(items, 2);
    every.nonces(nullptr);
    std::vector<uint8_t> only3{0, 0, 0, 1, 0}, none{0};
    edge_scalar(0, &items[2][1 + 32 * 5]);
    Case mixed(items, 2), alone(std::vector<std::vector<uint8_t>>(5, make_proof(1, 7)), 2), nobody(std::vector<std::vector<uint8_t>>(5, make_proof(1, 7)), 2);
    mixed.nonces(&only3);
    alone.nonces(&only3);
    nobody.nonces(&none);
    const char *txt = "Mask recovery is not supported with an aggregated statement";
    EXPECT("seed_with_m2", outcome_is(every.pk, P64, BPP_ERR_INVALID_ARGUMENT, txt, 0) &&
                               outcome_is(mixed.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 2) &&
                               outcome_is(alone.pk, P64, BPP_ERR_INVALID_ARGUMENT, txt, 3) && outcome_is(nobody.pk, P64, 0, nullptr, 0));
  }
  {  // nonces at m = 1: all, every other item (flags bit 0, zeros where absent), none
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 9; i++) items.push_back(make_proof(1, 6));
    Case all_(items, 1), alt(items, 1, 3), none(items, 1);
    std::vector<uint8_t> other{1, 0}, zero{0};
    all_.nonces(nullptr);
    alt.nonces(&other);
    none.nonces(&zero);
    alt.promises({5, 0, 77}, {1, 0, 1});
    EXPECT("nonces_m1", outcome_is(all_.pk, P64, 0, nullptr, 0) && outcome_is(alt.pk, P64, 0, nullptr, 0) && outcome_is(none.pk, P64, 0, nullptr, 0));
  }
  {  // a transcript state with pos >= rate: reported at item 0 once its proof has parsed, behind item 0's own findings
    std::vector<uint8_t> good = make_proof(1, 6), bad = good;
    edge_scalar(0, &bad[1 + 32 * 4]);
    Case a({good, good, bad}, 1), b({bad, good, good}, 1);
    a.bad_state();
    b.bad_state();
    EXPECT("bad_transcript_state", outcome_is(a.pk, P64, BPP_ERR_INVALID_ARGUMENT, "transcript state has pos >= rate", 0) &&
                                       outcome_is(b.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 0));
  }
  {  // promises 2^n - 1 and 2^n at n = 8: the second is a finding of its item, raised at verify time
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 6; i++) items.push_back(make_proof(1, 3));
    Case fits(items, 1), over(items, 1), unset(items, 1);
    fits.promises({255}, {1});
    over.promises({255, 255, 256, 255, 256, 255}, {1});
    unset.promises({256}, {0});
    Outcome d;
    model(over.pk, P8, d);
    const bool found = d.code == 0 && d.pl.any_defer && d.pl.defer == std::vector<uint8_t>({0, 0, BPP_DEFER_PROMISE, 0, BPP_DEFER_PROMISE, 0});
    Outcome f;
    model(fits.pk, P8, f);
    EXPECT("promises_at_the_capacity", outcome_is(fits.pk, P8, 0, nullptr, 0) && outcome_is(over.pk, P8, 0, nullptr, 0) &&
                                           outcome_is(unset.pk, P8, 0, nullptr, 0) && found && f.code == 0 && !f.pl.any_defer);
    // m = 2: the promise of the second commitment of item 1
    std::vector<std::vector<uint8_t>> items2;
    for (int i = 0; i < 3; i++) items2.push_back(make_proof(1, 4));
    Case agg(items2, 2);
    agg.promises({1, 2, 3, 256, 5, 6}, {1});
    Outcome g;
    model(agg.pk, P8, g);
    EXPECT("promise_of_an_aggregated_item", outcome_is(agg.pk, P8, 0, nullptr, 0) && g.pl.defer == std::vector<uint8_t>({0, BPP_DEFER_PROMISE, 0}));
  }
  {  // parameters of t = 2 over t = 1 proofs with an oversized promise in an earlier item: both recorded, the degree on every item
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 5; i++) items.push_back(make_proof(1, 4));
    Case c(items, 1);
    c.promises({0, 1ull << 16, 0, 0, 0}, {1});
    Outcome d;
    model(c.pk, P16t2, d);
    EXPECT("degree_and_promise", outcome_is(c.pk, P16t2, 0, nullptr, 0) &&
                                     d.pl.defer == std::vector<uint8_t>({1, 3, 1, 1, 1}));
  }
  {  // rounds that do not fit the statement (m = 2 proofs under m = 1 statements): recorded, raised at verify time
    Case c({make_proof(1, 7), make_proof(1, 7)}, 1);
    Outcome d;
    model(c.pk, P64, d);
    EXPECT("rounds_bad", outcome_is(c.pk, P64, 0, nullptr, 0) && d.pl.any_rounds_bad && d.pl.rounds_bad[1] == BPP_ERR_INVALID_LENGTH);
  }
  {  // what is uniform over the batch
    std::vector<std::vector<uint8_t>> items(3, make_proof(1, 6));
    Case m3(items, 3), m16(items, 16), nocommit(items, 1), nominv(items, 1), noproofs(items, 1), overlap(items, 1), empty_len(std::vector<std::vector<uint8_t>>(2), 1);
    nocommit.pk.commitments32 = nullptr;
    nominv.promises({1}, {1});
    nominv.pk.min_values = nullptr;
    noproofs.pk.proofs = nullptr;
    overlap.pk.proof_stride = overlap.len - 64;
    EXPECT("uniform_findings", outcome_is(m3.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Number of commitments must be a power of two", 0) &&
                                   outcome_is(m16.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Not enough generators for this statement", 0) &&
                                   outcome_is(nocommit.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Incorrect number of minimum value promises", 0) &&
                                   outcome_is(nominv.pk, P64, BPP_ERR_INVALID_ARGUMENT, "Incorrect number of minimum value promises", 0) &&
                                   outcome_is(noproofs.pk, P64, BPP_ERR_INVALID_LENGTH, "Serialized proof is too short", 0) &&
                                   agree(overlap.pk, P64) && agree(empty_len.pk, P64));
    // the 4 GB limits need no array: sizes only
    bpp_packed_batch big = m3.pk;
    big.m = 1;
    big.n_items = (1u << 24);
    big.proof_len = big.proof_stride = 577;
    Outcome d;
    model(big, P64, d);
    EXPECT("size_limit", d.code == BPP_ERR_SIZE_OVERFLOW && d.msg == "batch too large for one call (4 GB of proof bytes)");
  }
  {  // another extension degree in the same number of bytes in ONE item: pass A declines, every item alone still agrees
    std::vector<std::vector<uint8_t>> items(7, make_proof(1, 6));
    items[4] = make_proof(3, 5);
    Case c(items, 1, 7);
    Outcome d;
    model(c.pk, P64, d);
    EXPECT("mixed_first_bytes_fall_back", d.fallback && agree(c.pk, P64));
  }
  {  // random mutations of length and content, batches of three
    bool all = true;
    for (int iter = 0; iter < 1500 && all; iter++) {
      const uint32_t t = 1 + (uint32_t)(rng() % 3), r = 1 + (uint32_t)(rng() % 8), m = 1u << (rng() % 3);
      size_t len = 1 + 32 * (size_t)(t + 5 + 2 * r);
      if (rng() % 3 == 0) len = 1 + rng() % (len + 70);
      std::vector<std::vector<uint8_t>> items;
      for (int i = 0; i < 3; i++) {
        std::vector<uint8_t> p = make_proof(t, r);
        p.resize(len, (uint8_t)rng());
        for (int k = 0; k < (int)(rng() % 3); k++) p[rng() % len] = (uint8_t)rng();
        items.push_back(p);
      }
      Case c(items, m, rng() % 9);
      c.promises({rng(), rng() & 0xffff, 0}, {(uint8_t)(rng() & 1), 1, 0});
      if (rng() & 1) {
        std::vector<uint8_t> w{(uint8_t)(rng() & 1), (uint8_t)(rng() & 1), 1};
        c.nonces((rng() & 1) ? &w : nullptr);
      }
      all = agree(c.pk, (rng() & 1) ? P64t3 : P16t2);
    }
    EXPECT("mutations", all);
  }
  printf("%d comparisons\n", checked);
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
