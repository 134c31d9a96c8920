// Sanitizer harness (CPU test suite only): the one-item routines of ingest.h in their mixed form -- what k_ingest_mixed runs per proof
// of a batch of mixed aggregation factors that lies in device memory -- the host prelude and the plan (ingest_mixed.h), run on the
// host over a corpus and held
// to upload_pass_a + upload_pass_b on the equivalent item array (upload_mixed_as_items): for every case {code, message text, index}
// are equal, and on success bytes[], minvals, seeds, every ProofDesc field, rounds_bad, defer and the plan's sums and maxima.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_ingest_mixed_host.py runs.
// The struct addresses its rows by a stride, so the rows of an array share one allocation; it ends with the last byte the last row
// uses, and the slack of every other row is poisoned twice: with values that would change the outcome if they were used (0xFF in
// proof and commitment slack, a present promise of 2^63 in promise slack) and with ASAN_POISON_MEMORY_REGION, so that a read of
// slack is an AddressSanitizer report.  Row strides are multiples of eight bytes wherever that poisoning has to be exact (ASan
// poisons in granules of eight).  Prints one "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "ingest_mixed.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)(p), (void)(n))
#define UNPOISON(p, n) ((void)(p), (void)(n))
#endif

using namespace bpp;

namespace {

std::mt19937_64 rng(20261021);

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

void group_order(uint8_t out[32]) {
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  memcpy(out, L, 32);
}

struct Item {
  std::vector<uint8_t> proof;
  uint32_t m = 1;
  bool nonce = false;
  std::vector<uint64_t> minv;     // empty: no promise
  std::vector<uint8_t> present;
};

uint32_t log2u(uint32_t v) {
  uint32_t r = 0;
  while ((1u << r) < v) r++;
  return r;
}
// a sound item of aggregation factor m under parameters of n_bits and t
Item good(uint32_t m, uint32_t n_bits, uint32_t t) {
  Item it;
  it.m = m;
  it.proof = make_proof(t, log2u(m * n_bits));
  return it;
}

enum Nonces { NO_NONCES, NONCE_ARRAY_ONLY, NONCE_FLAGS };  // no array; array without seed_present (every item); array and flags

// a mixed batch that owns its arrays: one allocation per array, exact to the last used byte, slack poisoned
struct Case {
  size_t n = 0, stride = 0;
  uint32_t m_stride = 0;
  std::vector<size_t> lens;
  std::vector<uint32_t> ms;
  uint8_t *proofs = nullptr, *commits = nullptr, *present = nullptr, *seeds = nullptr, *seed_present = nullptr;
  uint64_t *minv = nullptr;
  size_t proofs_n = 0, entries = 0;
  std::vector<uint8_t> state;
  bpp_mixed_batch mx;

  Case(const std::vector<Item> &items, Nonces nonces, bool promises, size_t extra_stride = 8, uint32_t m_stride_ = 8) : n(items.size()), m_stride(m_stride_) {
    size_t longest = 0;
    for (const Item &it : items) {
      lens.push_back(it.proof.size());
      ms.push_back(it.m);
      longest = std::max(longest, it.proof.size());
    }
    stride = (longest + extra_stride + 7) & ~(size_t)7;
    proofs_n = (n - 1) * stride + lens[n - 1];
    const uint32_t last_m = std::min(ms[n - 1], m_stride);
    entries = (n - 1) * (size_t)m_stride + last_m;
    proofs = (uint8_t *)malloc(proofs_n ? proofs_n : 1);
    commits = (uint8_t *)malloc(entries * 32 + 1);
    memset(proofs, 0xff, proofs_n);
    memset(commits, 0xff, entries * 32);
    if (promises) {
      minv = (uint64_t *)malloc(entries * 8 + 8);
      present = (uint8_t *)malloc(entries + 1);
      for (size_t q = 0; q < entries; q++) {
        minv[q] = 1ull << 63;
        present[q] = 1;
      }
    }
    if (nonces != NO_NONCES) {
      seeds = (uint8_t *)malloc(32 * n);
      for (size_t q = 0; q < 32 * n; q++) seeds[q] = (uint8_t)(rng() | 1);
      if (nonces == NONCE_FLAGS) seed_present = (uint8_t *)malloc(n);
    }
    for (size_t i = 0; i < n; i++) {
      const Item &it = items[i];
      const uint32_t used = (i + 1 < n) ? std::min(it.m, m_stride) : last_m;
      if (lens[i]) memcpy(proofs + i * stride, it.proof.data(), lens[i]);
      for (size_t q = 0; q < 32 * (size_t)used; q++) commits[32 * i * m_stride + q] = (uint8_t)rng();
      if (promises)
        for (uint32_t j = 0; j < used; j++) {
          minv[i * m_stride + j] = it.minv.empty() ? 0 : it.minv[j % it.minv.size()];
          present[i * m_stride + j] = it.present.empty() ? 0 : it.present[j % it.present.size()];
        }
      if (seed_present) seed_present[i] = it.nonce ? 1 : 0;
      if (i + 1 < n) {
        POISON(proofs + i * stride + lens[i], stride - lens[i]);
        POISON(commits + 32 * (i * m_stride + used), 32 * (size_t)(m_stride - used));
        if (promises) {
          POISON(minv + i * m_stride + used, 8 * (size_t)(m_stride - used));
          POISON(present + i * m_stride + used, m_stride - used);
        }
      }
    }
    memset(&mx, 0, sizeof(mx));
    mx.n_items = n;
    mx.proofs = proofs;
    mx.proof_stride = stride;
    mx.proof_lens = lens.data();
    mx.m = ms.data();
    mx.m_stride = m_stride;
    mx.commitments32 = commits;
    mx.min_values = minv;
    mx.min_present = present;
    mx.seed_nonces32 = seeds;
    mx.seed_present = seed_present;
    mx.transcript_label = (const uint8_t *)"harness";
    mx.label_len = 7;
  }
  Case(const Case &) = delete;
  ~Case() {
    UNPOISON(proofs, proofs_n);
    UNPOISON(commits, entries * 32);
    if (minv) UNPOISON(minv, entries * 8);
    if (present) UNPOISON(present, entries);
    free(proofs);
    free(commits);
    free(minv);
    free(present);
    free(seeds);
    free(seed_present);
  }
  void bad_state() {
    state.assign(203, 0x5a);
    state[200] = (uint8_t)BPP_STROBE_R;  // pos >= rate
    mx.transcript_state = state.data();
  }
};

struct Outcome {
  int code = 0;
  std::string msg;
  uint32_t index = 0;
  bool fallback = false;  // (model only) the engine would stage the arrays and take the host form
  UploadPlan pl;
  std::vector<uint8_t> bytes, seeds;
  std::vector<uint64_t> minvals;
};

// the host form: the item form over views of the rows, as upload_mixed_impl drives it
void expected(const bpp_mixed_batch &mx, const ParamShape &P, Outcome &o) {
  try {
    upload_mixed_geometry(mx);
    std::vector<bpp_verify_item> items;
    upload_mixed_as_items(mx, items);
    upload_pass_a(items.data(), items.size(), o.pl);
    o.bytes.assign(o.pl.bytes_total + BPP_BYTES_SLACK, 0xcd);
    memset(o.bytes.data() + o.pl.bytes_total, 0, BPP_BYTES_SLACK);
    upload_pass_b(items.data(), P, o.pl, o.bytes.data(), serial_for);
    o.seeds = o.pl.seeds;
    o.minvals = o.pl.minvals;
  } catch (const ProofErr &e) {
    o.code = e.code;
    o.msg = e.msg;
    o.index = e.index;
  }
}

// the device form with the host standing in for the kernel: prelude, the one-item routines over items [0, h), the plan
void model(const bpp_mixed_batch &mx, const ParamShape &P, Outcome &o) {
  try {
    IngestMixedPrelude pre;
    if (!ingest_mixed_host_prelude(mx, P, pre)) {
      o.fallback = true;
      return;
    }
    const size_t n = mx.n_items, bytes_total = (size_t)(pre.proof_bytes + pre.sum_m * 32);
    if (pre.h == 0) ingest_mixed_throw_finding(pre, n, nullptr);
    // exact sizes: a write past the end of what the engine allocates is an ASan report
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[bytes_total + BPP_BYTES_SLACK]), seeds(new uint8_t[mx.seed_nonces32 ? n * 32 : 1]),
        info(new uint8_t[n]);
    std::unique_ptr<uint64_t[]> minvals(new uint64_t[pre.sum_m ? pre.sum_m : 1]);
    std::unique_ptr<IngestMixedRow[]> rows(new IngestMixedRow[n]);
    memcpy(rows.get(), pre.rows.data(), n * sizeof(IngestMixedRow));
    memset(bytes.get(), 0xcd, bytes_total + BPP_BYTES_SLACK);
    memset(seeds.get(), 0, mx.seed_nonces32 ? n * 32 : 1);
    uint32_t res[BPP_ING_RES_WORDS];
    const Ingest a = ingest_mixed_args(mx, P, pre, rows.get(), bytes.get(), minvals.get(), seeds.get(), info.get(), res);
    ingest_run_host<true>(a);
    if (res[BPP_ING_RES_DIFFERS]) {
      o.fallback = true;
      return;
    }
    ingest_mixed_finish_plan(mx, P, pre, res, ingest_needs_info(mx, res) ? info.get() : nullptr, o.pl);
    o.bytes.assign(bytes.get(), bytes.get() + bytes_total + BPP_BYTES_SLACK);
    o.minvals.assign(minvals.get(), minvals.get() + pre.sum_m);
    if (mx.seed_nonces32) o.seeds.assign(seeds.get(), seeds.get() + n * 32);
  } catch (const ProofErr &e) {
    o.code = e.code;
    o.msg = e.msg;
    o.index = e.index;
  }
}

const char *why = "";

bool same_plan(const Outcome &h, const Outcome &d, size_t n) {
  const UploadPlan &a = h.pl, &b = d.pl;
  // (pass A keeps a nonce array only when some item has a nonce; the device form has one whenever the caller gave the array, zeros
  // where no nonce is present)
  const bool seeds = h.seeds.empty() ? std::all_of(d.seeds.begin(), d.seeds.end(), [](uint8_t v) { return v == 0; }) : h.seeds == d.seeds;
  if (!(a.desc.size() == n && b.desc.size() == n && memcmp(a.desc.data(), b.desc.data(), n * sizeof(ProofDesc)) == 0))
    return why = "descriptors differ", false;
  if (h.bytes != d.bytes) return why = "bytes differ", false;
  if (h.minvals != d.minvals) return why = "promises differ", false;
  if (!seeds) return why = "nonces differ", false;
  if (a.defer != b.defer || a.rounds_bad != b.rounds_bad) return why = "defer / rounds_bad differ", false;
  if (!(a.states == b.states && a.total_dyn == b.total_dyn && a.rmax == b.rmax && a.max_mn == b.max_mn && a.any_seed == b.any_seed &&
        a.any_defer == b.any_defer && a.any_rounds_bad == b.any_rounds_bad && a.uniform_rounds == b.uniform_rounds && a.sum_m == b.sum_m &&
        a.proof_bytes == b.proof_bytes && a.bytes_total == b.bytes_total && a.tr_err_index == b.tr_err_index))
    return why = "plan sums differ", false;
  return true;
}

// item i of mx as a batch of its own (what the one-item routines are held to when the whole batch takes the host form)
bpp_mixed_batch single(const bpp_mixed_batch &mx, size_t i) {
  bpp_mixed_batch s = mx;
  s.n_items = 1;
  s.proofs = mx.proofs ? mx.proofs + i * mx.proof_stride : nullptr;
  s.proof_lens = mx.proof_lens + i;
  s.m = mx.m + i;
  s.commitments32 = mx.commitments32 ? mx.commitments32 + 32 * i * (size_t)mx.m_stride : nullptr;
  s.min_values = mx.min_values ? mx.min_values + i * (size_t)mx.m_stride : nullptr;
  s.min_present = mx.min_present ? mx.min_present + i * (size_t)mx.m_stride : nullptr;
  s.seed_nonces32 = mx.seed_nonces32 ? mx.seed_nonces32 + 32 * i : nullptr;
  s.seed_present = mx.seed_present ? mx.seed_present + i : nullptr;
  return s;
}

int fails = 0, checked = 0;

bool agree(const bpp_mixed_batch &mx, const ParamShape &P, int depth = 0) {
  Outcome h, d;
  expected(mx, P, h);
  model(mx, P, d);
  checked++;
  if (d.fallback) {
    // the engine takes the host form with the staged arrays: nothing of the device form decides the outcome.  It must be a batch
    // without a proofs array or one whose first bytes differ; its items, one at a time, still hold the one-item routines to the item form
    bool differ = !mx.proofs;
    for (size_t i = 1; i < mx.n_items && !differ; i++)
      differ = mx.proof_lens[i] && (!mx.proof_lens[0] || mx.proofs[i * mx.proof_stride] != mx.proofs[0]);
    if (!differ) return why = "model falls back on a batch of equal first bytes", false;
    if (depth == 0 && mx.proofs && mx.n_items > 1)
      for (size_t i = 0; i < mx.n_items; i++)
        if (!agree(single(mx, i), P, 1)) return false;
    return true;
  }
  if (h.code != d.code || h.msg != d.msg || h.index != d.index) {
    printf("   host {%d, \"%s\", %u}  model {%d, \"%s\", %u}\n", h.code, h.msg.c_str(), h.index, d.code, d.msg.c_str(), d.index);
    return why = "findings differ", false;
  }
  if (h.code == 0 && !same_plan(h, d, mx.n_items)) return false;
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

// what a case must come to on BOTH sides (so that a corpus that silently stopped failing is noticed); device = true: the model
// must have decided it without the fall-back
bool outcome_is(const bpp_mixed_batch &mx, const ParamShape &P, int code, const char *msg, uint32_t index, bool device = true) {
  Outcome h;
  expected(mx, P, h);
  if (h.code != code || h.index != index || (msg && h.msg != msg)) {
    printf("   host {%d, \"%s\", %u}, wanted {%d, \"%s\", %u}\n", h.code, h.msg.c_str(), h.index, code, msg ? msg : "", index);
    return why = "the host form's outcome is not the one the case is about", false;
  }
  if (device) {
    Outcome d;
    model(mx, P, d);
    if (d.fallback) return why = "the model fell back on a case meant for the device path", false;
  }
  return agree(mx, P);
}

// the m pattern of the tests, valid items under P
std::vector<Item> pattern(size_t n, const ParamShape &P) {
  static const uint32_t ms[7] = {4, 1, 2, 1, 1, 4, 2};
  std::vector<Item> v;
  for (size_t i = 0; i < n; i++) v.push_back(good(std::min(ms[i % 7], P.m_max), P.n_bits, P.t));
  return v;
}

}  // namespace

int main() {
  const ParamShape P8{8, 4, 1}, P8t2{8, 4, 2}, P64t3{64, 2, 3};
  const char *AGG = "Mask recovery is not supported with an aggregated statement";
  {  // valid batches of every shape of the GPU tests, promises and nonces on the m = 1 items; one item alone
    bool all = true;
    for (const ParamShape *P : {&P8, &P8t2, &P64t3})
      for (size_t n : {(size_t)1, (size_t)5, (size_t)17, (size_t)67}) {
        std::vector<Item> items = pattern(n, *P);
        for (Item &it : items) {
          it.nonce = it.m == 1;
          it.minv = {rng() & 0x7f, 0, 3};
          it.present = {1, 0, 1};
        }
        Case plain(items, NO_NONCES, false), full(items, NONCE_FLAGS, true, 3, 8), tight(items, NONCE_FLAGS, true, 0, P->m_max);
        all = all && outcome_is(plain.mx, *P, 0, nullptr, 0) && outcome_is(full.mx, *P, 0, nullptr, 0) && outcome_is(tight.mx, *P, 0, nullptr, 0);
      }
    EXPECT("valid_shapes", all);
    Case one({good(1, 8, 1)}, NONCE_ARRAY_ONLY, true), one4({good(4, 8, 1)}, NO_NONCES, true);
    EXPECT("one_item", outcome_is(one.mx, P8, 0, nullptr, 0) && outcome_is(one4.mx, P8, 0, nullptr, 0));
  }
  {  // every finding of ingest_check_item at index 3 of 7, between valid items of other m
    const uint32_t t = 1;
    auto with = [&](const std::function<void(Item &)> &f) {
      std::vector<Item> items = pattern(7, P8);
      f(items[3]);
      return items;
    };
    bool all = true;
    // every truncation of the item's proof, and a few surplus lengths
    const std::vector<uint8_t> full = good(1, 8, 1).proof;
    for (size_t len = 0; len <= full.size() + 70 && all; len += (len < 40 || len + 40 > full.size()) ? 1 : 13) {
      Case c(with([&](Item &it) {
               it.proof = full;
               it.proof.resize(len, (uint8_t)rng());
             }),
             NO_NONCES, false);
      all = agree(c.mx, P8);
      if (all && len >= 33 && len < full.size()) {  // a non-canonical d1[0] under the same cut beats a body too short for r1
        Case c2(with([&](Item &it) {
                  it.proof = full;
                  it.proof.resize(len);
                  group_order(&it.proof[1]);
                }),
                NO_NONCES, false);
        all = outcome_is(c2.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 3);
      }
    }
    EXPECT("lengths_at_index_3", all);
    Case cut(with([](Item &it) { it.proof.pop_back(); }), NO_NONCES, true), surplus(with([](Item &it) { it.proof.resize(it.proof.size() + 32, 1); }), NO_NONCES, false),
        empty(with([](Item &it) { it.proof.clear(); }), NO_NONCES, false), shortp(with([&](Item &it) { it.proof.resize(1 + 32 * (t + 5)); }), NO_NONCES, false);
    EXPECT("length_findings", outcome_is(cut.mx, P8, BPP_ERR_INVALID_LENGTH, "Unused data after deserialization", 3) &&
                                  outcome_is(surplus.mx, P8, BPP_ERR_INVALID_LENGTH, "Unused data after deserialization", 3) &&
                                  outcome_is(empty.mx, P8, BPP_ERR_INVALID_LENGTH, "Serialized proof is too short", 3) &&
                                  outcome_is(shortp.mx, P8, BPP_ERR_INVALID_LENGTH, "Serialized proof is too short", 3));
    bool parsing = true;
    for (uint32_t field : {0u, t + 3, t + 4}) {
      Case c(with([&](Item &it) { group_order(&it.proof[1 + 32 * field]); }), NONCE_FLAGS, true);
      parsing = parsing && outcome_is(c.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 3);
    }
    EXPECT("non_canonical_scalars", parsing);
    Case r65(with([](Item &it) { it.proof = make_proof(1, 65); }), NO_NONCES, false), r64(with([](Item &it) { it.proof = make_proof(1, 64); }), NO_NONCES, false);
    EXPECT("wire_rounds_64_and_65", outcome_is(r65.mx, P8, BPP_ERR_SIZE_OVERFLOW, "Internal size overflow (more than 64 (L, R) pairs)", 3) &&
                                        outcome_is(r64.mx, P8, 0, nullptr, 0));
    // first byte 0 and 7 in one item: the first bytes differ, the batch takes the host form, every item alone still agrees; in
    // every item: the finding is item 0's, on the device path
    bool degree = true;
    for (uint8_t b : {(uint8_t)0, (uint8_t)7}) {
      Case one(with([&](Item &it) { it.proof[0] = b; }), NO_NONCES, false);
      std::vector<Item> every = pattern(7, P8);
      for (Item &it : every) it.proof[0] = b;
      Case all7(every, NO_NONCES, false);
      degree = degree && outcome_is(one.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Extension degree not valid", 3, false) &&
               outcome_is(all7.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Extension degree not valid", 0);
    }
    EXPECT("first_byte_0_and_7", degree);
  }
  {  // a nonce on an m = 2 item (index 2 of the pattern), alone and behind / in front of a non-canonical s1
    std::vector<Item> items = pattern(7, P8);
    items[2].nonce = true;
    items[1].nonce = true;  // m = 1: fine
    Case alone(items, NONCE_FLAGS, false);
    std::vector<Item> below = items, above = items;
    group_order(&below[1].proof[1 + 32 * 5]);
    group_order(&above[4].proof[1 + 32 * 5]);
    Case cb(below, NONCE_FLAGS, false), ca(above, NONCE_FLAGS, false), every(pattern(7, P8), NONCE_ARRAY_ONLY, false);
    EXPECT("nonce_on_an_m2_item", outcome_is(alone.mx, P8, BPP_ERR_INVALID_ARGUMENT, AGG, 2) && outcome_is(cb.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 1) &&
                                      outcome_is(ca.mx, P8, BPP_ERR_INVALID_ARGUMENT, AGG, 2) && outcome_is(every.mx, P8, BPP_ERR_INVALID_ARGUMENT, AGG, 0));
  }
  {  // host-known findings at h: m = 3, m = 8 > m_max, m = 0; with a device finding below h (it wins) and above h (never looked at)
    bool all = true;
    struct {
      uint32_t m;
      const char *msg;
    } kinds[] = {{3, "Number of commitments must be a power of two"}, {0, "Number of commitments must be a power of two"},
                 {8, "Not enough generators for this statement"}};
    for (const auto &k : kinds) {
      std::vector<Item> items = pattern(7, P8);
      items[3].m = k.m;
      Case alone(items, NO_NONCES, true);
      std::vector<Item> below = items, above = items, both = items;
      group_order(&below[1].proof[1]);
      group_order(&above[5].proof[1]);
      above[6].proof.pop_back();
      group_order(&both[2].proof[1 + 32 * 4]);
      group_order(&both[4].proof[1 + 32 * 4]);
      Case cb(below, NO_NONCES, true), ca(above, NO_NONCES, true), cc(both, NONCE_FLAGS, false);
      all = all && outcome_is(alone.mx, P8, BPP_ERR_INVALID_ARGUMENT, k.msg, 3) && outcome_is(cb.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 1) &&
            outcome_is(ca.mx, P8, BPP_ERR_INVALID_ARGUMENT, k.msg, 3) && outcome_is(cc.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 2);
      // at item 0: nothing runs
      std::vector<Item> first = pattern(5, P8);
      first[0].m = k.m;
      first[1].proof.pop_back();
      Case c0(first, NO_NONCES, false);
      all = all && outcome_is(c0.mx, P8, BPP_ERR_INVALID_ARGUMENT, k.msg, 0);
    }
    EXPECT("host_known_findings", all);
    // the promises' null rule and a missing commitments array: every item has the finding, item 0 reports it
    Case nominv(pattern(5, P8), NO_NONCES, true), nocommit(pattern(5, P8), NO_NONCES, false), noproofs(pattern(5, P8), NONCE_FLAGS, false);
    nominv.mx.min_values = nullptr;
    nocommit.mx.commitments32 = nullptr;
    noproofs.mx.proofs = nullptr;
    Outcome np;
    model(noproofs.mx, P8, np);
    EXPECT("null_arrays", outcome_is(nominv.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Incorrect number of minimum value promises", 0) &&
                              outcome_is(nocommit.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Incorrect number of minimum value promises", 0) && np.fallback &&
                              outcome_is(noproofs.mx, P8, BPP_ERR_INVALID_LENGTH, "Serialized proof is too short", 0, false));
  }
  {  // the geometry refusals and the size limits: both forms, before anything is read
    Case c(pattern(5, P8), NO_NONCES, false);
    bpp_mixed_batch narrow = c.mx, thin = c.mx, nolens = c.mx, nom = c.mx;
    narrow.proof_stride = c.lens[0] - 1;
    thin.m_stride = 2;
    nolens.proof_lens = nullptr;
    nom.m = nullptr;
    Outcome a, b, e, f;
    model(narrow, P8, a);
    model(thin, P8, b);
    model(nolens, P8, e);
    model(nom, P8, f);
    EXPECT("geometry_refusals", a.code == BPP_ERR_INVALID_ARGUMENT && a.msg == "proof_stride is below a proof length" && b.code == BPP_ERR_INVALID_ARGUMENT &&
                                    b.msg == "m_stride is below an aggregation factor" && e.msg == "proof_lens is null" && f.msg == "m is null" &&
                                    agree(narrow, P8) && agree(thin, P8) && agree(nolens, P8) && agree(nom, P8));
    // sizes only: no array is read before the limit is reported
    const size_t n = 1u << 20;
    std::vector<size_t> lens(n, 4097);
    std::vector<uint32_t> ms(n, 1);
    bpp_mixed_batch big = c.mx;
    big.n_items = n;
    big.proof_lens = lens.data();
    big.m = ms.data();
    big.proof_stride = 4104;
    Outcome d;
    model(big, P8, d);
    EXPECT("size_limit", d.code == BPP_ERR_SIZE_OVERFLOW && d.msg == "batch too large for one call (4 GB of proof bytes)");
  }
  {  // promises at the capacity: 2^n - 1 fits, 2^n is a finding of its item (raised at verify time), per entry of an m = 4 item
    std::vector<Item> items = pattern(7, P8);
    for (Item &it : items) {
      it.minv = {255};
      it.present = {1};
    }
    items[5].minv = {1, 2, 256, 4};  // m = 4
    items[3].minv = {256};
    items[4].minv = {256};
    items[4].present = {0};
    Case c(items, NO_NONCES, true);
    Outcome d;
    model(c.mx, P8, d);
    EXPECT("promises_at_the_capacity", outcome_is(c.mx, P8, 0, nullptr, 0) && d.pl.any_defer &&
                                           d.pl.defer == std::vector<uint8_t>({0, 0, 0, BPP_DEFER_PROMISE, 0, BPP_DEFER_PROMISE, 0}));
    // parameters of t = 2 over t = 1 proofs: the degree on every item, beside the promise
    Outcome g;
    model(c.mx, P8t2, g);
    EXPECT("degree_and_promise", outcome_is(c.mx, P8t2, 0, nullptr, 0) && g.pl.defer == std::vector<uint8_t>({1, 1, 1, 3, 1, 3, 1}));
  }
  {  // rounds that do not fit the statement: an m = 2 proof under an m = 1 statement, recorded per item
    std::vector<Item> items = pattern(7, P8);
    items[3].proof = make_proof(1, 4);
    Case c(items, NO_NONCES, false);
    Outcome d;
    model(c.mx, P8, d);
    EXPECT("rounds_bad", outcome_is(c.mx, P8, 0, nullptr, 0) && d.pl.any_rounds_bad && d.pl.rounds_bad[3] == BPP_ERR_INVALID_LENGTH && d.pl.rounds_bad[2] == 0);
  }
  {  // a transcript state with pos >= rate: item 0's, once its proof has parsed
    std::vector<Item> items = pattern(5, P8), bad0 = items;
    group_order(&items[2].proof[1]);
    group_order(&bad0[0].proof[1]);
    Case a(items, NO_NONCES, false), b(bad0, NO_NONCES, false);
    a.bad_state();
    b.bad_state();
    EXPECT("bad_transcript_state", outcome_is(a.mx, P8, BPP_ERR_INVALID_ARGUMENT, "transcript state has pos >= rate", 0) &&
                                       outcome_is(b.mx, P8, BPP_ERR_INVALID_ARGUMENT, "Invalid parsing", 0));
  }
  {  // one proof of another extension degree: the first bytes differ, the batch takes the host form
    std::vector<Item> items = pattern(7, P8);
    items[4].proof = make_proof(2, 3);
    Case c(items, NONCE_FLAGS, true);
    Outcome d;
    model(c.mx, P8, d);
    EXPECT("mixed_first_bytes_fall_back", d.fallback && agree(c.mx, P8));
  }
  {  // random mutations of lengths, contents, aggregation factors, promises and nonces, batches of five
    bool all = true;
    for (int iter = 0; iter < 1500 && all; iter++) {
      const ParamShape &P = (iter & 1) ? P8t2 : P64t3;
      const uint32_t t = (rng() % 8) ? P.t : 1 + (uint32_t)(rng() % 3);
      std::vector<Item> items;
      for (int i = 0; i < 5; i++) {
        Item it;
        it.m = 1u << (rng() % 3);
        if (rng() % 23 == 0) it.m = (uint32_t)(rng() % 9);
        it.proof = make_proof(t, (rng() % 5) ? log2u(std::max(it.m, 1u) * P.n_bits) : 1 + (uint32_t)(rng() % 8));
        if (rng() % 7 == 0) it.proof.resize(rng() % (it.proof.size() + 70), (uint8_t)rng());
        for (int k = 0; k < (int)(rng() % 3) && !it.proof.empty(); k++)
          if (rng() % 5 == 0) it.proof[rng() % it.proof.size()] = (uint8_t)rng();
        it.nonce = rng() % 3 == 0 && (it.m == 1 || rng() % 4 == 0);
        it.minv = {rng() & 0x1ff, rng()};
        it.present = {(uint8_t)(rng() & 1), (uint8_t)(rng() % 9 == 0)};
        items.push_back(it);
      }
      Case c(items, (Nonces)(rng() % 3 == 0 ? NONCE_ARRAY_ONLY : (rng() & 1 ? NONCE_FLAGS : NO_NONCES)), (rng() & 3) != 0, rng() % 16, 8);
      all = agree(c.mx, P);
    }
    EXPECT("mutations", all);
  }
  {  // packed is the mixed form whose row is arithmetic: over a uniform batch (proof_stride > proof_len, m_stride = m) the run by the
     // table the prelude makes and the run by arithmetic leave the same bytes, promises, nonces, info, result words and plan -- with a
     // promise above the capacity and an absent nonce, and with a non-canonical scalar, whose finding both must throw
    bool all = true;
    for (uint32_t m : {1u, 2u})
      for (bool bad : {false, true}) {
        std::vector<Item> items;
        for (size_t i = 0; i < 7; i++) {
          Item it = good(m, P8.n_bits, P8.t);
          it.nonce = i != 4;
          it.minv = {i == 2 ? 256u : 255u};
          it.present = {1};
          items.push_back(it);
        }
        if (bad) group_order(&items[3].proof[1]);
        Case c(items, NONCE_FLAGS, true, 8, m);
        const size_t n = c.n, bytes_len = n * c.lens[0] + n * m * 32 + BPP_BYTES_SLACK;
        bpp_packed_batch pk;
        memset(&pk, 0, sizeof(pk));
        pk.n_items = n;
        pk.proofs = c.mx.proofs;
        pk.proof_len = c.lens[0];
        pk.proof_stride = c.mx.proof_stride;
        pk.m = m;
        pk.commitments32 = c.mx.commitments32;
        pk.min_values = c.mx.min_values;
        pk.min_present = c.mx.min_present;
        pk.seed_nonces32 = c.mx.seed_nonces32;
        pk.seed_present = c.mx.seed_present;
        pk.transcript_label = c.mx.transcript_label;
        pk.label_len = c.mx.label_len;
        struct Run {
          std::vector<uint8_t> bytes, seeds, info;
          std::vector<uint64_t> minvals;
          uint32_t res[BPP_ING_RES_WORDS];
          Outcome o;
        } rows, arith;
        for (Run *r : {&rows, &arith}) {
          r->bytes.assign(bytes_len, 0xcd);
          r->seeds.assign(n * 32, 0xcd);
          r->info.assign(n, 0xcd);
          r->minvals.assign(n * m, 0xcdcdcdcdcdcdcdcdull);
        }
        IngestMixedPrelude pre;
        all = all && pk.proof_stride > pk.proof_len && ingest_mixed_host_prelude(c.mx, P8, pre) && pre.h == n && ingest_host_prelude(pk, P8);
        if (!all) break;
        ingest_run_host<true>(ingest_mixed_args(c.mx, P8, pre, pre.rows.data(), rows.bytes.data(), rows.minvals.data(), rows.seeds.data(),
                                                rows.info.data(), rows.res));
        ingest_run_host<false>(ingest_args(pk, P8, arith.bytes.data(), arith.minvals.data(), arith.seeds.data(), arith.info.data(), arith.res));
        for (Run *r : {&rows, &arith}) {
          const uint8_t *info = ingest_needs_info(pk, r->res) ? r->info.data() : nullptr;
          try {
            if (r == &rows) ingest_mixed_finish_plan(c.mx, P8, pre, r->res, info, r->o.pl);
            else ingest_finish_plan(pk, P8, r->res, info, r->o.pl);
          } catch (const ProofErr &e) {
            r->o.code = e.code;
            r->o.msg = e.msg;
            r->o.index = e.index;
          }
          r->o.bytes = r->bytes;
          r->o.seeds = r->seeds;
          r->o.minvals = r->minvals;
        }
        const int want_code = (bad || m > 1) ? BPP_ERR_INVALID_ARGUMENT : 0;  // (m = 2: the nonce of item 0 is a finding of its own)
        all = all && rows.info == arith.info && memcmp(rows.res, arith.res, sizeof(rows.res)) == 0 && rows.bytes == arith.bytes &&
              rows.minvals == arith.minvals && rows.seeds == arith.seeds && rows.o.code == want_code && arith.o.code == want_code &&
              rows.o.msg == arith.o.msg && rows.o.index == arith.o.index && rows.res[BPP_ING_RES_ANY_PROMISE] == 1 &&
              (want_code || same_plan(rows.o, arith.o, n));
      }
    EXPECT("uniform_rows_equal_packed", all);
  }
  printf("%d comparisons\n", checked);
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
