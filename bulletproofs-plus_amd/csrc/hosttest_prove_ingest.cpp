// Sanitizer harness (CPU test suite only): the routines of prove_ingest.h -- what k_prove_ingest runs per item of a prove call whose
// openings lie in device memory -- and the host plan, run on the host lane by lane (16 lanes per item as the kernel has them, and
// one) over a corpus and held to ProvePack::pack and prove_item_check_host on the sorted equivalent items: d_bytes, every ProveDesc
// field, minvals, minpres and the states are equal, and every finding's {code, message} is what prove_item_check_host throws for
// that item.  An item with a finding is compared with the substitute the header describes.  The host's part -- findings, sort, row
// tables -- is prove_device_shape, the function the engine runs; the case group `shape` tests it alone.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_prove_ingest_host.py runs.
// The rows of an array share one allocation; it ends with the last byte the last row uses, and the slack of every other row is
// filled with 0xFF -- a value over the capacity, a promise above every value, a blinding factor and a nonce that are not canonical:
// each a finding if it were read -- in the first pass and poisoned with ASAN_POISON_MEMORY_REGION in the second.  Row strides are
// multiples of eight bytes (ASan poisons in granules of eight).  Prints one "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "prove_ingest.h"

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

std::mt19937_64 rng(20261020);
bool g_poison = false;
int g_failures = 0;

const uint8_t ORDER[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                           0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};

void canonical_scalar(uint8_t *p) {
  for (int i = 0; i < 32; i++) p[i] = (uint8_t)rng();
  p[31] &= 0x0f;  // < 2^252 < l
}

struct Item {
  uint32_t m = 1;
  std::vector<uint64_t> values, minv;
  std::vector<uint8_t> present, blind;  // blind: m x t x 32
  bool nonce = false;
  uint8_t seed[32];
};

Item good(uint32_t m, const ParamShape &P, bool nonce_if_single) {
  Item it;
  it.m = m;
  for (uint32_t j = 0; j < m; j++) {
    const uint64_t v = P.n_bits < 64 ? (rng() & ((1ull << P.n_bits) - 1)) : rng();
    it.values.push_back(v);
    it.present.push_back((uint8_t)(j & 1u));  // promises on alternate openings
    it.minv.push_back((j & 1u) ? v / 2 : ~0ull);  // (an absent promise's value is never looked at)
  }
  it.blind.resize((size_t)m * P.t * 32);
  for (uint32_t q = 0; q < m * P.t; q++) canonical_scalar(&it.blind[32 * (size_t)q]);
  it.nonce = nonce_if_single && m == 1;
  canonical_scalar(it.seed);
  return it;
}

enum Nonces { NO_NONCES, NONCE_ARRAY_ONLY, NONCE_FLAGS };

size_t rng_need(const ParamShape &P, uint32_t m) { return 32 * (size_t)(prove_rounds_host(P, m) + 3); }

// a call that owns its arrays: one allocation per array, exact to the last used byte, slack 0xFF or poisoned
struct Case {
  ParamShape P;
  size_t n;
  uint32_t ms;
  size_t rng_stride;
  std::vector<uint32_t> m;
  std::vector<uint32_t> used;  // the openings of row i anyone may read: m[i] for an item the host's part passes, else 0
  uint8_t *values = nullptr, *blind = nullptr, *commits = nullptr, *minv = nullptr, *present = nullptr, *seeds = nullptr, *seed_present = nullptr,
          *rngb = nullptr;
  size_t entries = 0, rng_n = 0;
  std::vector<uint8_t> state;
  bpp_prove_arrays in;
  std::vector<bpp_prove_item> items;  // the equivalent items: pointers into the same rows

  static uint8_t *filled(size_t bytes) {
    uint8_t *p = (uint8_t *)malloc(bytes ? bytes : 1);
    memset(p, 0xff, bytes);
    return p;
  }

  Case(const ParamShape &P_, const std::vector<Item> &its, Nonces nonces, bool promises, bool brought, size_t rng_stride_, bool use_state)
      : P(P_), n(its.size()), ms(8), rng_stride(rng_stride_) {
    const uint32_t t = P.t;
    for (const Item &it : its) m.push_back(it.m);
    ProveDeviceShape sh;
    if (!prove_device_shape(P, m.data(), n, ms, rng_stride, SIZE_MAX, SIZE_MAX, true, sh)) abort();  // (no case asks for an m above the stride)
    for (size_t i = 0; i < n; i++) used.push_back(sh.msg[i] ? 0 : m[i]);
    entries = (n - 1) * (size_t)ms + used[n - 1];
    rng_n = (n - 1) * rng_stride + (used[n - 1] ? rng_need(P, m[n - 1]) : 0);
    values = filled(entries * 8);
    blind = filled(entries * t * 32);
    if (brought) commits = filled(entries * 32);
    if (promises) {
      minv = filled(entries * 8);
      present = filled(entries);
    }
    if (nonces != NO_NONCES) {
      seeds = filled(32 * n);
      if (nonces == NONCE_FLAGS) seed_present = filled(n);
    }
    rngb = filled(rng_n);
    for (size_t i = 0; i < n; i++) {
      const Item &it = its[i];
      const size_t row = i * ms;
      for (uint32_t j = 0; j < used[i]; j++) {
        for (int k = 0; k < 8; k++) values[8 * (row + j) + k] = (uint8_t)(it.values[j] >> (8 * k));
        memcpy(blind + 32 * (row + j) * t, &it.blind[32 * (size_t)j * t], 32 * (size_t)t);
        if (brought)
          for (int k = 0; k < 32; k++) commits[32 * (row + j) + k] = (uint8_t)rng();
        if (promises) {
          for (int k = 0; k < 8; k++) minv[8 * (row + j) + k] = (uint8_t)(it.minv[j] >> (8 * k));
          present[row + j] = it.present[j];
        }
      }
      if (used[i])
        for (size_t k = 0; k < rng_need(P, it.m); k++) rngb[i * rng_stride + k] = (uint8_t)rng();
      if (seeds && (it.nonce || nonces == NONCE_ARRAY_ONLY)) memcpy(seeds + 32 * i, it.seed, 32);
      if (seed_present) seed_present[i] = it.nonce ? 1 : 0;
    }
    if (g_poison) poison(true);
    memset(&in, 0, sizeof(in));
    in.n_items = n;
    in.m = m.data();
    in.m_stride = ms;
    in.values = (const uint64_t *)values;
    in.blindings32 = blind;
    in.commitments32 = commits;
    in.min_values = (const uint64_t *)minv;
    in.min_present = present;
    in.seed_nonces32 = seeds;
    in.seed_present = seed_present;
    in.rng_bytes = rngb;
    in.rng_stride = rng_stride;
    if (use_state) {
      state.assign(203, 0);
      Strobe st;
      merlin_new(st, (const uint8_t *)"a state", 7);
      strobe_to_bytes(state.data(), st);
      in.transcript_state = state.data();
    } else {
      in.transcript_label = (const uint8_t *)"harness";
      in.label_len = 7;
    }
    items.assign(n, bpp_prove_item{});
    for (size_t i = 0; i < n; i++) {
      bpp_prove_item &o = items[i];
      const size_t row = i * ms;
      o.values = (const uint64_t *)(values + 8 * row);
      o.blindings32 = blind + 32 * row * t;
      o.commitments32 = commits ? commits + 32 * row : nullptr;
      o.m = m[i];
      o.min_values = minv ? (const uint64_t *)(minv + 8 * row) : nullptr;
      o.min_present = present ? present + row : nullptr;
      const bool seed = seeds && (!seed_present || seed_present[i]);
      o.seed_nonce32 = seed ? seeds + 32 * i : nullptr;
      o.transcript_state = in.transcript_state;
      o.transcript_label = in.transcript_label;
      o.label_len = in.label_len;
      o.rng_bytes = rngb + i * rng_stride;
      o.rng_len = rng_stride;
    }
  }
  void poison(bool on) {
    const uint32_t t = P.t;
    for (size_t i = 0; i + 1 < n; i++) {
      const size_t row = i * ms, at = row + used[i], gap = ms - used[i];
      const size_t rn = used[i] ? rng_need(P, m[i]) : 0;
      if (on) {
        POISON(values + 8 * at, 8 * gap);
        POISON(blind + 32 * at * t, 32 * gap * t);
        if (commits) POISON(commits + 32 * at, 32 * gap);
        if (minv) POISON(minv + 8 * at, 8 * gap);
        if (present && (at % 8) == 0) POISON(present + at, gap);
        if (rng_stride > rn) POISON(rngb + i * rng_stride + rn, rng_stride - rn);
      } else {
        UNPOISON(values + 8 * at, 8 * gap);
        UNPOISON(blind + 32 * at * t, 32 * gap * t);
        if (commits) UNPOISON(commits + 32 * at, 32 * gap);
        if (minv) UNPOISON(minv + 8 * at, 8 * gap);
        if (present) UNPOISON(present + at, gap);
        if (rng_stride > rn) UNPOISON(rngb + i * rng_stride + rn, rng_stride - rn);
      }
    }
  }
  Case(const Case &) = delete;
  ~Case() {
    if (g_poison) poison(false);
    free(values), free(blind), free(commits), free(minv), free(present), free(seeds), free(seed_present), free(rngb);
  }
};

struct Outcome {
  int code;
  std::string msg;
  bool operator==(const Outcome &o) const { return code == o.code && msg == o.msg; }
};

Outcome host_outcome(const ParamShape &P, const bpp_prove_item &it, size_t proof_stride = SIZE_MAX, size_t commit_stride = SIZE_MAX) {
  try {
    prove_item_check_host(P, it, proof_stride, true, commit_stride);
  } catch (const ProofErr &e) {
    return Outcome{e.code, e.msg};
  }
  return Outcome{BPP_OK, ""};
}

// the whole device form on the host, with `lanes` lanes per item, against the item form; expect[i] (optional): the message id item i
// must end with
bool run(const char *name, Case &c, uint32_t lanes, const std::vector<uint32_t> *expect = nullptr) {
  const ParamShape &P = c.P;
  const uint32_t t = P.t;
  std::vector<uint8_t> hg32((size_t)(t + 1) * 32);
  for (auto &b : hg32) b = (uint8_t)rng();
  auto bad = [&](const char *what, size_t i) {
    printf("FAIL %s: %s at %zu (lanes %u, poison %d)\n", name, what, i, lanes, (int)g_poison);
    g_failures++;
    return false;
  };
  // the host's part per item -- the engine's shape step -- against the item form on the equivalent item
  ProveDeviceShape sh;
  if (!prove_device_shape(P, c.m.data(), c.n, c.ms, c.rng_stride, SIZE_MAX, SIZE_MAX, true, sh)) return bad("m_stride is below", sh.m_stride_below);
  std::vector<uint32_t> msg = sh.msg;
  const std::vector<uint32_t> &m_sorted = sh.m_sorted;
  const std::vector<ProveDevRow> &rows = sh.rows;
  for (size_t i = 0; i < c.n; i++) {
    if (!msg[i]) continue;
    const Outcome want = host_outcome(P, c.items[i]), got{prove_msg_code(msg[i]), prove_msg_text(msg[i])};
    // the one precedence difference: a nonce on an aggregated item whose rng is also short reports the rng finding here
    const bool documented = msg[i] == BPP_PROVE_MSG_RNG_LEN && want.msg == prove_msg_text(BPP_PROVE_MSG_SEED_AGGREGATED);
    if (!(want == got) && !documented) return bad("host finding differs", i);
  }
  if (rows.empty()) return true;
  const uint32_t B = (uint32_t)rows.size();
  ProvePack plan;
  prove_plan_device(P, hg32.data(), m_sorted.data(), B, c.in.commitments32 != nullptr, c.in.transcript_state, c.in.transcript_label,
                    c.in.label_len, plan);
  // the sub-batches as ProveCall::carve cuts them (64 slots each), each with buffers of its own that end where its bytes end
  std::vector<ProveDesc> dev_desc = plan.desc;
  std::vector<uint8_t> dev_bytes;
  std::vector<uint64_t> dev_minvals((size_t)B * plan.m, 0);
  std::vector<uint8_t> dev_minpres((size_t)B * plan.m, 0);
  std::vector<uint32_t> finding(B, 0xdeadbeefu);
  for (uint32_t lo = 0; lo < B; lo += 64) {
    const uint32_t nb = std::min<uint32_t>(64, B - lo);
    const size_t bytes_lo = plan.desc[lo].wit_off, bytes_len = (lo + nb < B ? plan.desc[lo + nb].wit_off : plan.bytes_len) - bytes_lo;
    std::vector<ProveDesc> d(plan.desc.begin() + lo, plan.desc.begin() + lo + nb);
    for (uint32_t i = 0; i < nb; i++) {
      d[i].wit_off -= (uint32_t)bytes_lo, d[i].commit_off -= (uint32_t)bytes_lo, d[i].ext_off -= (uint32_t)bytes_lo, d[i].seed_off -= (uint32_t)bytes_lo;
      d[i].minval_idx = i * plan.m;
    }
    uint8_t *bytes = (uint8_t *)malloc(bytes_len);
    memset(bytes, 0xa5, bytes_len);
    ProveIngest a;
    memset(&a, 0, sizeof(a));
    a.values = c.values, a.blindings32 = c.blind, a.commitments32 = c.commits, a.min_values = c.minv, a.min_present = c.present;
    a.seed_nonces32 = c.seeds, a.seed_present = c.seed_present, a.rng_bytes = c.rngb, a.rng_stride = c.rng_stride;
    a.m_stride = c.ms, a.n_bits = P.n_bits, a.t = t, a.nb = nb, a.g0_32 = hg32.data() + 32;
    a.rows = rows.data() + lo, a.desc = d.data(), a.bytes = bytes;
    a.minvals = dev_minvals.data() + (size_t)lo * plan.m, a.minpres = dev_minpres.data() + (size_t)lo * plan.m, a.finding = finding.data() + lo;
    prove_ingest_run_host(a, lanes);
    dev_bytes.insert(dev_bytes.end(), bytes, bytes + bytes_len);
    free(bytes);
    for (uint32_t i = 0; i < nb; i++) dev_desc[lo + i].flags = d[i].flags;
  }
  // findings against the item form; the reference items: the equivalent ones, a failed one replaced by the substitute
  std::vector<bpp_prove_item> ref(B);
  const std::vector<uint64_t> zero_v(P.m_max, 0);
  std::vector<uint8_t> one_r((size_t)P.m_max * t * 32, 0), g0((size_t)P.m_max * 32), zero_rng(rng_need(P, P.m_max), 0);
  for (uint32_t j = 0; j < P.m_max; j++) {
    one_r[(size_t)j * t * 32] = 1;
    memcpy(&g0[32 * (size_t)j], hg32.data() + 32, 32);
  }
  for (uint32_t k = 0; k < B; k++) {
    const bpp_prove_item &it = c.items[rows[k].item];
    const Outcome want = host_outcome(P, it);
    const uint32_t id = prove_ingest_key_msg(finding[k]);
    const Outcome got{prove_msg_code(id), prove_msg_text(id)};
    if (!(want == got)) {
      printf("  want %d '%s' got %d '%s'\n", want.code, want.msg.c_str(), got.code, got.msg.c_str());
      return bad("device finding differs", rows[k].item);
    }
    msg[rows[k].item] = id;
    ref[k] = it;
    if (id) {
      bpp_prove_item &s = ref[k];
      s.values = zero_v.data(), s.blindings32 = one_r.data(), s.commitments32 = c.commits ? g0.data() : nullptr;
      s.min_values = nullptr, s.min_present = nullptr, s.seed_nonce32 = nullptr, s.rng_bytes = zero_rng.data(), s.rng_len = zero_rng.size();
    }
  }
  if (expect)
    for (size_t i = 0; i < c.n; i++)
      if (msg[i] != (*expect)[i]) {
        printf("  item %zu: message id %u, expected %u\n", i, msg[i], (*expect)[i]);
        return bad("not the expected finding", i);
      }
  ProvePack pk;
  pk.pack(P, hg32.data(), ref.data(), B, true, true);
  if (pk.bytes != dev_bytes) return bad("bytes differ", 0);
  if (pk.bytes_len != plan.bytes_len || pk.m != plan.m || pk.rounds != plan.rounds || pk.rounds_min != plan.rounds_min || pk.plen != plan.plen)
    return bad("call shape differs", 0);
  if (pk.states != plan.states) return bad("states differ", 0);
  if (pk.roff != plan.roff) return bad("roff differs", 0);
  if (pk.minvals != dev_minvals || pk.minpres != dev_minpres) return bad("promise rows differ", 0);
  for (uint32_t k = 0; k < B; k++) {
    const ProveDesc &x = pk.desc[k], &y = dev_desc[k];
    if (x.m != y.m || x.wit_off != y.wit_off || x.commit_off != y.commit_off || x.ext_off != y.ext_off || x.minval_idx != y.minval_idx ||
        x.state_idx != y.state_idx || x.flags != y.flags || x.seed_off != y.seed_off || x.roff != y.roff || x.mslot != y.mslot)
      return bad("descriptor differs", k);
  }
  return true;
}

std::vector<Item> pattern(size_t n, const ParamShape &P, bool nonces) {
  static const uint32_t ms[5] = {1, 4, 2, 8, 1};
  std::vector<Item> v;
  for (size_t i = 0; i < n; i++) v.push_back(good(ms[i % 5], P, nonces));
  return v;
}

size_t full_stride(const ParamShape &P) { return rng_need(P, P.m_max) + 8; }

bool both(const char *name, Case &c, const std::vector<uint32_t> *expect = nullptr) { return run(name, c, 16, expect) && run(name, c, 1, expect); }

void report(const char *name, bool ok) {
  if (ok && !g_poison) return;  // (one line per case, after its second pass)
  printf("%s %s\n", ok ? "ok" : "FAIL", name);
}

// every kind of device finding; `at`: the item, `where`: 0 the first, 1 a middle, 2 the last opening / blinding factor
enum Kind { K_VALUE, K_MINIMUM, K_BLINDING, K_SEED_NONCE, K_KINDS };
uint32_t kind_msg(Kind k) {
  return k == K_VALUE ? BPP_PROVE_MSG_VALUE : k == K_MINIMUM ? BPP_PROVE_MSG_MINIMUM : k == K_BLINDING ? BPP_PROVE_MSG_BLINDING : BPP_PROVE_MSG_SEED_NONCE;
}
void spoil(Item &it, Kind k, int where, const ParamShape &P) {
  const uint32_t j = where == 0 ? 0 : (where == 1 ? it.m / 2 : it.m - 1);
  if (k == K_VALUE) it.values[j] = 1ull << P.n_bits;
  if (k == K_MINIMUM) it.present[j] = 1, it.minv[j] = it.values[j] + 1;
  if (k == K_BLINDING) {
    const uint32_t q = where == 0 ? 0 : (where == 1 ? it.m * P.t / 2 : it.m * P.t - 1);
    memcpy(&it.blind[32 * (size_t)q], ORDER, 32);
  }
  if (k == K_SEED_NONCE) memset(it.seed, 0xff, 32);
}

void corpus() {
  for (uint32_t t : {1u, 3u}) {
    const ParamShape P{32, 8, t};
    bool ok = true;
    {
      Case c(P, {good(1, P, false)}, NO_NONCES, false, false, full_stride(P), false);
      ok = both("one_item", c);
      Case d(P, {good(1, P, true)}, NONCE_ARRAY_ONLY, true, true, rng_need(P, 1), true);
      ok = ok && both("one_item", d);
    }
    report("one_item", ok);
    for (size_t n : {(size_t)5, (size_t)17, (size_t)67}) {
      ok = true;
      for (int brought = 0; brought < 2; brought++) {
        Case c(P, pattern(n, P, true), NONCE_FLAGS, true, brought != 0, full_stride(P), brought != 0);
        ok = ok && both("valid_shapes", c);
      }
      Case e(P, pattern(n, P, false), NO_NONCES, false, false, full_stride(P), false);
      ok = ok && both("valid_shapes", e);
      report(n == 5 ? "pattern_5" : n == 17 ? "pattern_17" : "pattern_67", ok);
    }
    // every finding kind at the first, a middle and the last item and opening
    ok = true;
    for (int k = 0; k < K_KINDS; k++)
      for (size_t n : {(size_t)17, (size_t)67})
        for (int where = 0; where < 3; where++) {
          std::vector<Item> v = pattern(n, P, true);
          std::vector<uint32_t> expect(n, 0);
          // (a nonce finding needs an item that carries one: the m = 1 items do)
          const size_t at[3] = {0, k == K_SEED_NONCE ? (size_t)5 : (size_t)(n / 2) / 5 * 5 + 3, k == K_SEED_NONCE ? n - 2 - (n - 2) % 5 : n - 1};
          for (size_t i : at) {
            spoil(v[i], (Kind)k, where, P);
            expect[i] = kind_msg((Kind)k);
          }
          for (int brought = 0; brought < 2; brought++) {
            Case c(P, v, NONCE_FLAGS, true, brought != 0, full_stride(P), false);
            ok = ok && both("findings_first_middle_last", c, &expect);
          }
        }
    report("findings_first_middle_last", ok);
    {
      // two findings in one item: the earlier one in the host's order wins, whichever lane sees which
      std::vector<Item> v = pattern(7, P, true);
      std::vector<uint32_t> expect(7, 0);
      spoil(v[3], K_BLINDING, 0, P), spoil(v[3], K_VALUE, 2, P), expect[3] = BPP_PROVE_MSG_VALUE;            // a late value before an early blinding factor
      spoil(v[1], K_MINIMUM, 0, P), spoil(v[1], K_VALUE, 1, P), expect[1] = BPP_PROVE_MSG_MINIMUM;           // opening 0's promise before opening 2's value
      spoil(v[0], K_SEED_NONCE, 0, P), spoil(v[0], K_BLINDING, 2, P), expect[0] = BPP_PROVE_MSG_BLINDING;   // a blinding factor before the nonce
      v[2].values[1] = 1ull << 40, v[2].present[1] = 1, v[2].minv[1] = ~0ull, expect[2] = BPP_PROVE_MSG_VALUE;  // the value before its own promise
      Case c(P, v, NONCE_FLAGS, true, false, full_stride(P), false);
      report("two_findings", both("two_findings", c, &expect));
    }
    {
      std::vector<Item> v = pattern(5, P, false);
      std::vector<uint32_t> expect(5, 0);
      v[0].values[0] = (1ull << 32) - 1;                              // 2^n - 1: the largest value there is
      v[1].values[3] = 1ull << 32, expect[1] = BPP_PROVE_MSG_VALUE;  // 2^n
      v[3].values[7] = ~0ull, expect[3] = BPP_PROVE_MSG_VALUE;
      Case c(P, v, NO_NONCES, true, false, full_stride(P), false);
      report("value_edges", both("value_edges", c, &expect));
    }
    {
      std::vector<Item> v = pattern(5, P, false);
      std::vector<uint32_t> expect(5, 0);
      v[1].present[2] = 1, v[1].minv[2] = v[1].values[2];                                          // min == value
      v[3].present[7] = 1, v[3].minv[7] = v[3].values[7] + 1, expect[3] = BPP_PROVE_MSG_MINIMUM;  // min == value + 1
      v[4].present[0] = 0, v[4].minv[0] = ~0ull;                                                   // absent: not compared
      Case c(P, v, NO_NONCES, true, true, full_stride(P), false);
      report("minimum_edges", both("minimum_edges", c, &expect));
    }
    {
      std::vector<Item> v = pattern(5, P, false);
      std::vector<uint32_t> expect(5, 0);
      memcpy(&v[0].blind[0], ORDER, 32), v[0].blind[0] = 0xec;                                                   // l - 1
      memcpy(&v[1].blind[32 * (size_t)(4 * t - 1)], ORDER, 32), expect[1] = BPP_PROVE_MSG_BLINDING;              // l
      memset(&v[3].blind[32 * (size_t)(3 * t)], 0xff, 32), expect[3] = BPP_PROVE_MSG_BLINDING;                   // all ones
      Case c(P, v, NO_NONCES, false, false, full_stride(P), false);
      report("blinding_edges", both("blinding_edges", c, &expect));
    }
    {
      std::vector<Item> v = pattern(5, P, true);
      std::vector<uint32_t> expect(5, 0);
      v[2].nonce = true, expect[2] = BPP_PROVE_MSG_SEED_AGGREGATED;
      Case c(P, v, NONCE_FLAGS, true, false, full_stride(P), false);
      bool k = both("nonce_on_an_m2_item", c, &expect);
      // the array without flags: every item carries one, every aggregated item fails
      std::vector<uint32_t> all = {0, BPP_PROVE_MSG_SEED_AGGREGATED, BPP_PROVE_MSG_SEED_AGGREGATED, BPP_PROVE_MSG_SEED_AGGREGATED, 0};
      Case d(P, pattern(5, P, true), NONCE_ARRAY_ONLY, false, false, full_stride(P), false);
      report("nonce_on_an_m2_item", k && both("nonce_on_an_m2_item", d, &all));
    }
    {
      // seed_present = 0: the row is not read (it holds 0xFF: not canonical) and the slot gets zeros
      std::vector<Item> v = pattern(5, P, false);
      v[4].nonce = true;
      std::vector<uint32_t> expect(5, 0);
      Case c(P, v, NONCE_FLAGS, false, false, full_stride(P), false);
      report("nonce_with_seed_present_0", both("nonce_with_seed_present_0", c, &expect));
    }
    {
      // one byte short for the largest m only: the m = 8 item fails on the host, the others are packed
      std::vector<Item> v = pattern(7, P, true);
      std::vector<uint32_t> expect(7, 0);
      expect[3] = BPP_PROVE_MSG_RNG_LEN;
      Case c(P, v, NONCE_FLAGS, true, false, rng_need(P, 8) - 8, false);
      bool k = both("rng_stride_short_for_the_largest_m", c, &expect);
      Case d(P, v, NONCE_FLAGS, true, false, rng_need(P, 8) - 1, false);  // (one BYTE short)
      k = k && both("rng_stride_short_for_the_largest_m", d, &expect);
      // the documented precedence difference: a nonce on the m = 8 item as well
      v[3].nonce = true;
      Case e(P, v, NONCE_FLAGS, true, false, rng_need(P, 8) - 1, false);
      k = k && both("rng_stride_short_for_the_largest_m", e, &expect);
      report("rng_stride_short_for_the_largest_m", k);
    }
    {
      // aggregation factors no statement can have stay on the host; the rest is packed
      std::vector<Item> v = pattern(6, P, true);
      v[1].m = 3, v[2].m = 0, v[5].m = 16;
      std::vector<uint32_t> expect = {0, BPP_PROVE_MSG_POWER_OF_TWO, BPP_PROVE_MSG_POWER_OF_TWO, 0, 0, BPP_PROVE_MSG_GENERATORS};
      Case c(P, v, NONCE_FLAGS, true, true, full_stride(P), true);
      report("host_findings", both("host_findings", c, &expect));
    }
    {
      // every item fails
      std::vector<Item> v = pattern(5, P, true);
      std::vector<uint32_t> expect(5, BPP_PROVE_MSG_VALUE);
      for (Item &it : v) spoil(it, K_VALUE, 2, P);
      Case c(P, v, NONCE_FLAGS, true, true, full_stride(P), false);
      report("every_item_fails", both("every_item_fails", c, &expect));
    }
  }
}

// ---- the shape step itself (prove_device_shape: what the blocking calls and bpp_prove_plan_create run) over
// m[] = {1, 4, 3, 2, 0, 2 m_max, 1, 4}.  want_msg / want_zero: per item, the finding and (for a refused item) the zero flags.
struct ShapeCall {
  uint32_t m_stride;
  size_t rng_stride, proof_stride, commit_stride;
  bool fields_ok;
};

bool shape_holds(const ParamShape &P, const std::vector<uint32_t> &m, const ShapeCall &k, const std::vector<uint32_t> &want_msg,
                 const std::vector<uint32_t> &want_zero) {
  auto bad = [&](const char *what, size_t i) {
    printf("FAIL shape: %s at %zu (m_max %u, t %u, m_stride %u, rng %zu, proof %zu, commit %zu, fields %d)\n", what, i, P.m_max, P.t, k.m_stride,
           k.rng_stride, k.proof_stride, k.commit_stride, (int)k.fields_ok);
    g_failures++;
    return false;
  };
  ProveDeviceShape sh;
  if (!prove_device_shape(P, m.data(), m.size(), k.m_stride, k.rng_stride, k.proof_stride, k.commit_stride, k.fields_ok, sh))
    return bad("the step stopped", sh.m_stride_below);
  // the equivalent item: valid openings of its m (read only once every check of part one has passed), rng_stride bytes of randomness
  const std::vector<uint64_t> values(2 * P.m_max, 0);
  const std::vector<uint8_t> blind((size_t)2 * P.m_max * P.t * 32, 0), rngb(1, 0);
  std::vector<uint8_t> has_slot(m.size(), 0);
  size_t r = 0, slots = 0;
  for (size_t i = 0; i < m.size(); i++) {
    if (sh.proof_lens[i] != prove_item_len_host(P, m[i])) return bad("proof length differs", i);
    bpp_prove_item it{};
    it.m = m[i], it.values = k.fields_ok ? values.data() : nullptr, it.blindings32 = blind.data(), it.rng_bytes = rngb.data(), it.rng_len = k.rng_stride;
    const Outcome want = host_outcome(P, it, k.proof_stride, k.commit_stride), got{prove_msg_code(sh.msg[i]), prove_msg_text(sh.msg[i])};
    if (!(want == got)) return bad("finding differs from prove_item_check_host", i);
    if (sh.msg[i] != want_msg[i]) return bad("not the expected finding", i);
    if (!sh.msg[i]) {
      has_slot[i] = 1, slots++;
      continue;
    }
    if (r == sh.refused.size()) return bad("a refused item is missing from the table", i);
    const ProveDevRow &x = sh.refused[r++];
    if (x.item != i || x.m != m[i] || x.proof_len != sh.proof_lens[i] || x.msg != sh.msg[i]) return bad("refused row differs", i);
    if (x.zero != want_zero[i]) return bad("zero flags differ", i);
  }
  if (r != sh.refused.size()) return bad("the refused table holds more than the refused items", r);
  if (sh.rows.size() != slots || sh.m_sorted.size() != slots) return bad("the slots are not the items without a finding", slots);
  for (size_t s = 0; s < slots; s++) {
    const ProveDevRow &x = sh.rows[s];
    if (x.item >= m.size() || !has_slot[x.item]) return bad("not a permutation of the items without a finding", s);
    has_slot[x.item] = 0;
    if (x.m != m[x.item] || sh.m_sorted[s] != x.m || x.proof_len != sh.proof_lens[x.item] || x.msg != 0 ||
        x.zero != (BPP_PROVE_ROW_ZERO_PROOF | BPP_PROVE_ROW_ZERO_COMMIT))
      return bad("slot row differs", s);
    if (s && (sh.rows[s - 1].m < x.m || (sh.rows[s - 1].m == x.m && sh.rows[s - 1].item >= x.item))) return bad("not sorted", s);
  }
  return true;
}

void shape() {
  const uint32_t POW2 = BPP_PROVE_MSG_POWER_OF_TWO, GEN = BPP_PROVE_MSG_GENERATORS, PS = BPP_PROVE_MSG_PROOF_STRIDE, CS = BPP_PROVE_MSG_COMMIT_STRIDE;
  const uint32_t RNG = BPP_PROVE_MSG_RNG_LEN, ZP = BPP_PROVE_ROW_ZERO_PROOF, ZC = BPP_PROVE_ROW_ZERO_COMMIT, NUL = BPP_PROVE_MSG_NULL_FIELD;
  bool ok = true;
  for (const ParamShape &P : {ParamShape{64, 4, 1}, ParamShape{64, 8, 2}}) {
    const std::vector<uint32_t> m = {1, 4, 3, 2, 0, 2 * P.m_max, 1, 4};
    const uint32_t wide = 2 * P.m_max;
    const size_t full = rng_need(P, P.m_max), len2 = prove_item_len_host(P, 2);
    // every stride wide enough: 3, 0 and 2 m_max have no proof length and neither flag
    ok = shape_holds(P, m, {wide, full, SIZE_MAX, SIZE_MAX, true}, {0, 0, POW2, 0, POW2, GEN, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}) && ok;
    ok = prove_item_len_host(P, 3) == 0 && prove_item_len_host(P, 0) == 0 && prove_item_len_host(P, wide) == 0 && ok;
    // a proof_stride that holds m = 2: the m = 4 items lose ZERO_PROOF, the m = 2 item -- refused for its rng -- keeps it
    ok = shape_holds(P, m, {wide, rng_need(P, 2) - 1, len2, SIZE_MAX, true}, {0, PS, POW2, RNG, POW2, GEN, 0, PS}, {0, ZC, 0, ZP | ZC, 0, 0, 0, ZC}) && ok;
    // the same for a commit_stride of 32 x 2 and ZERO_COMMIT
    ok = shape_holds(P, m, {wide, rng_need(P, 2) - 1, SIZE_MAX, 64, true}, {0, CS, POW2, RNG, POW2, GEN, 0, CS}, {0, ZP, 0, ZP | ZC, 0, 0, 0, ZP}) && ok;
    // an rng_stride one byte short of what m = 4 needs: the m = 4 items alone, with the rng finding
    ok = shape_holds(P, m, {wide, rng_need(P, 4) - 1, SIZE_MAX, SIZE_MAX, true}, {0, RNG, POW2, 0, POW2, GEN, 0, RNG}, {0, ZP | ZC, 0, 0, 0, 0, 0, ZP | ZC}) && ok;
    // m_stride = 2 stops at the first m = 4 item, the lengths and findings in front of it written ...
    ProveDeviceShape sh;
    const bool stopped = !prove_device_shape(P, m.data(), m.size(), 2, full, SIZE_MAX, SIZE_MAX, true, sh) && sh.m_stride_below == 1 &&
                         sh.proof_lens[0] == prove_item_len_host(P, 1) && sh.proof_lens[1] == prove_item_len_host(P, 4) && sh.msg[0] == 0;
    if (!stopped) printf("FAIL shape: m_stride = 2 did not stop at item 1 (m_max %u)\n", P.m_max), g_failures++;
    // ... but not where the layout finding comes first: a proof_stride too short for m = 4
    ok = shape_holds(P, m, {2, full, len2, SIZE_MAX, true}, {0, PS, POW2, 0, POW2, GEN, 0, PS}, {0, ZC, 0, 0, 0, 0, 0, ZC}) && stopped && ok;
    // no fields: every item is refused with the layout finding it has then
    std::vector<uint32_t> none;
    for (uint32_t mi : m) none.push_back(prove_item_layout_finding(P, mi, SIZE_MAX, true, SIZE_MAX, false));
    ok = none == std::vector<uint32_t>{NUL, NUL, POW2, NUL, POW2, GEN, NUL, NUL} && ok;
    ok = shape_holds(P, m, {wide, full, SIZE_MAX, SIZE_MAX, false}, none, {ZP | ZC, ZP | ZC, 0, ZP | ZC, 0, 0, ZP | ZC, ZP | ZC}) && ok;
  }
  report("shape", ok);
}

}  // namespace

int main() {
  for (int pass = 0; pass < 2; pass++) {
    g_poison = pass == 1;
    rng.seed(20261020);
    corpus();
    shape();
  }
  if (g_failures) {
    printf("FAILED %d\n", g_failures);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
