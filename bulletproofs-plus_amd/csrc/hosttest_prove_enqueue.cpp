// Sanitizer harness (CPU test suite only): prove_ingest.h as bpp_prove_enqueue uses it.
//   1. The ingest routines under a LIVE MASK, run on the host lane by lane (16 lanes per item as the kernel has them, and one): all
//      live, all dead, alternating, only the first, only the last; 1, 5 and 67 items of the m pattern [1, 4, 2, 8, 1]; t = 1 and 3; one
//      transcript for the call and one row per item.  A live slot must equal ProvePack::pack on the equivalent item, a dead slot the
//      substitute, its finding word must carry BPP_PROVE_MSG_EMPTY, and its state row must be the fixed public one.
//      Every array ends behind the last live row.  The rows of dead items hold 0xFF in the first pass -- a value over the capacity, a
//      promise above every value, a blinding factor and a nonce that are not canonical, a nonce on an aggregated item, a state with pos
//      255: each a finding, or different bytes, if it were read -- and are poisoned with ASAN_POISON_MEMORY_REGION in the second: a
//      read of a dead row is an ASan report.
//   2. The emit routine's ok mask and outcome table, and the summary reduction (256 lanes as the kernel has them, and one), against a
//      straightforward host loop over outcome tables: a finding at the first, a middle and the last index, two findings, none,
//      refused items interleaved, all empty.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_prove_enqueue_host.py runs.  Prints one
// "ok <case>" line per case.
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

std::mt19937_64 rng(20261021);
bool g_poison = false;
int g_failures = 0;
const uint32_t PATTERN[5] = {1, 4, 2, 8, 1};
const uint32_t MS = 8;

size_t rng_need(const ParamShape &P, uint32_t m) { return 32 * (size_t)(prove_rounds_host(P, m) + 3); }

// one array of the call: rows of `row` bytes, of which row i uses used[i]; it ends with the last byte a LIVE row uses
struct Rows {
  uint8_t *p = nullptr;
  size_t row = 0, bytes = 0;
  std::vector<size_t> used;
  std::vector<uint8_t> live;

  void make(size_t row_bytes, const std::vector<size_t> &used_, const std::vector<uint8_t> &live_) {
    row = row_bytes, used = used_, live = live_;
    bytes = 0;
    for (size_t i = 0; i < used.size(); i++)
      if (live[i]) bytes = i * row + used[i];
    p = (uint8_t *)malloc(bytes ? bytes : 1);
    memset(p, 0xff, bytes);
  }
  uint8_t *at(size_t i) { return p + i * row; }
  // the rows of dead items in front of the last live row, and the slack of the live ones
  void poison(bool on) {
    for (size_t i = 0; i < used.size(); i++) {
      const size_t lo = i * row + (live[i] ? used[i] : 0), hi = std::min((i + 1) * row, bytes);
      if (lo >= hi) continue;
      if (on) POISON(p + lo, hi - lo);
      else UNPOISON(p + lo, hi - lo);
    }
  }
  ~Rows() { free(p); }
};

struct Case {
  ParamShape P;
  size_t n;
  bool brought, per_item;
  std::vector<uint32_t> m;
  std::vector<uint8_t> live;
  Rows values, blind, commits, minv, present, seeds, rngb, states;
  std::vector<uint8_t> seed_present;  // (one byte per item: not poisoned; a dead item's says "present" over a 0xFF nonce)
  std::vector<uint8_t> mask;          // the live mask as the routines read it
  std::vector<bpp_prove_item> items;

  Case(const ParamShape &P_, size_t n_, const std::vector<uint8_t> &live_, bool brought_, bool per_item_)
      : P(P_), n(n_), brought(brought_), per_item(per_item_), live(live_) {
    const uint32_t t = P.t;
    std::vector<size_t> u8(n), u32t(n), u32(n), u1(n), useed(n, 32), urng(n), ustate(n, 203);
    for (size_t i = 0; i < n; i++) {
      m.push_back(PATTERN[i % 5]);
      u8[i] = 8 * (size_t)m[i], u32t[i] = 32 * (size_t)m[i] * t, u32[i] = 32 * (size_t)m[i], u1[i] = m[i], urng[i] = rng_need(P, m[i]);
    }
    values.make(8 * MS, u8, live), blind.make(32 * (size_t)MS * t, u32t, live), commits.make(32 * MS, u32, live);
    minv.make(8 * MS, u8, live), present.make(MS, u1, live), seeds.make(32, useed, live);
    rngb.make(rng_need(P, P.m_max) + 8, urng, live), states.make(203, ustate, live);
    seed_present.assign(n, 0xff);
    mask.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
      if (!live[i]) continue;
      mask[i] = (uint8_t)(1 + (rng() % 255));  // (any non-zero byte is live)
      for (uint32_t j = 0; j < m[i]; j++) {
        const uint64_t v = rng() & ((1ull << P.n_bits) - 1);
        for (int k = 0; k < 8; k++) values.at(i)[8 * j + k] = (uint8_t)(v >> (8 * k));
        const uint64_t mv = v / 2;
        for (int k = 0; k < 8; k++) minv.at(i)[8 * j + k] = (uint8_t)(mv >> (8 * k));
        present.at(i)[j] = (uint8_t)(j & 1u);
        for (uint32_t q = 0; q < t; q++) {
          uint8_t *b = blind.at(i) + 32 * ((size_t)j * t + q);
          for (int k = 0; k < 32; k++) b[k] = (uint8_t)rng();
          b[31] &= 0x0f;
        }
        for (int k = 0; k < 32; k++) commits.at(i)[32 * j + k] = (uint8_t)rng();
      }
      for (size_t k = 0; k < rng_need(P, m[i]); k++) rngb.at(i)[k] = (uint8_t)rng();
      seed_present[i] = m[i] == 1 ? 1 : 0;
      for (int k = 0; k < 32; k++) seeds.at(i)[k] = (uint8_t)rng();
      seeds.at(i)[31] &= 0x0f;
      Strobe st;
      const std::string label = "item " + std::to_string(i);
      merlin_new(st, (const uint8_t *)label.data(), (uint32_t)label.size());
      strobe_to_bytes(states.at(i), st);
    }
    items.assign(n, bpp_prove_item{});
    for (size_t i = 0; i < n; i++) {
      if (!live[i]) continue;
      bpp_prove_item &o = items[i];
      o.values = (const uint64_t *)values.at(i), o.blindings32 = blind.at(i), o.commitments32 = brought ? commits.at(i) : nullptr;
      o.m = m[i], o.min_values = (const uint64_t *)minv.at(i), o.min_present = present.at(i);
      o.seed_nonce32 = seed_present[i] ? seeds.at(i) : nullptr;
      if (per_item) o.transcript_state = states.at(i);
      else o.transcript_label = (const uint8_t *)"harness", o.label_len = 7;
      o.rng_bytes = rngb.at(i), o.rng_len = rng_need(P, m[i]);
    }
    if (g_poison) poison(true);
  }
  void poison(bool on) {
    for (Rows *r : {&values, &blind, &commits, &minv, &present, &seeds, &rngb, &states}) r->poison(on);
  }
  Case(const Case &) = delete;
  ~Case() {
    if (g_poison) poison(false);
  }
};

bool run(const char *name, Case &c, uint32_t lanes) {
  const ParamShape &P = c.P;
  const uint32_t t = P.t;
  std::vector<uint8_t> hg32((size_t)(t + 1) * 32);
  for (auto &b : hg32) b = (uint8_t)rng();
  auto bad = [&](const char *what, size_t i) {
    printf("FAIL %s: %s at %zu (n %zu, t %u, lanes %u, poison %d)\n", name, what, i, c.n, t, lanes, (int)g_poison);
    g_failures++;
    return false;
  };
  // the sorted slots, from the engine's shape step: every item passes the host's part (the pattern's m are all legal)
  ProveDeviceShape sh;
  if (!prove_device_shape(P, c.m.data(), c.n, MS, c.rngb.row, SIZE_MAX, SIZE_MAX, true, sh) || sh.rows.size() != c.n)
    return bad("the host refused an item of the pattern", 0);
  const std::vector<ProveDevRow> &rows = sh.rows;
  const std::vector<uint32_t> &m_sorted = sh.m_sorted;
  const uint32_t B = (uint32_t)rows.size();
  const uint32_t sub = 64;
  ProvePack plan;
  prove_plan_device(P, hg32.data(), m_sorted.data(), B, c.brought, nullptr, c.per_item ? nullptr : (const uint8_t *)"harness", c.per_item ? 0 : 7, plan,
                    c.per_item ? sub : 0);
  std::vector<ProveDesc> dev_desc = plan.desc;
  std::vector<uint8_t> dev_bytes;
  std::vector<uint64_t> dev_minvals((size_t)B * plan.m, 0);
  std::vector<uint8_t> dev_minpres((size_t)B * plan.m, 0);
  std::vector<uint32_t> finding(B, 0xdeadbeefu);
  std::vector<uint8_t> dev_states((size_t)B * 203, 0xa5), ref_states((size_t)B * 203, 0x5a);
  // what the state kernel's model gives on rows that are all valid: a copy in which a dead item's row holds zeros, taken by flags
  std::vector<uint8_t> full_rows(c.n * 203, 0);
  for (size_t i = 0; i < c.n; i++)
    if (c.live[i]) memcpy(&full_rows[i * 203], c.states.at(i), 203);
  for (uint32_t lo = 0; lo < B; lo += sub) {
    const uint32_t nb = std::min<uint32_t>(sub, B - lo);
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
    a.values = c.values.p, a.blindings32 = c.blind.p, a.commitments32 = c.brought ? c.commits.p : nullptr, a.min_values = c.minv.p;
    a.min_present = c.present.p, a.seed_nonces32 = c.seeds.p, a.seed_present = c.seed_present.data(), a.rng_bytes = c.rngb.p;
    a.rng_stride = c.rngb.row, a.m_stride = MS, a.n_bits = P.n_bits, a.t = t, a.nb = nb, a.g0_32 = hg32.data() + 32;
    a.rows = rows.data() + lo, a.desc = d.data(), a.bytes = bytes;
    a.minvals = dev_minvals.data() + (size_t)lo * plan.m, a.minpres = dev_minpres.data() + (size_t)lo * plan.m, a.finding = finding.data() + lo;
    a.item_states = c.per_item ? c.states.p : nullptr;
    a.live = c.mask.data();
    prove_ingest_run_host(a, lanes);
    dev_bytes.insert(dev_bytes.end(), bytes, bytes + bytes_len);
    free(bytes);
    for (uint32_t i = 0; i < nb; i++) dev_desc[lo + i].flags = d[i].flags;
    if (c.per_item) {
      ProveItemStates s;
      memset(&s, 0, sizeof(s));
      s.src = c.states.p, s.rows = rows.data() + lo, s.desc = d.data(), s.finding = finding.data() + lo, s.hg32 = hg32.data();
      s.n_bits = P.n_bits, s.t = t, s.nb = nb, s.states = dev_states.data() + (size_t)lo * 203;
      prove_item_states_run_host(s);
      std::vector<uint32_t> flags(nb);
      for (uint32_t i = 0; i < nb; i++) flags[i] = c.live[rows[lo + i].item] ? 0u : 1u;
      s.src = full_rows.data(), s.finding = flags.data(), s.states = ref_states.data() + (size_t)lo * 203;
      prove_item_states_run_host(s);
    }
  }
  // the reference items: the equivalent ones, a dead one replaced by the substitute
  std::vector<bpp_prove_item> ref(B);
  const std::vector<uint64_t> zero_v(P.m_max, 0);
  std::vector<uint8_t> one_r((size_t)P.m_max * t * 32, 0), g0((size_t)P.m_max * 32), zero_rng(rng_need(P, P.m_max), 0), zero_state(203, 0);
  for (uint32_t j = 0; j < P.m_max; j++) {
    one_r[(size_t)j * t * 32] = 1;
    memcpy(&g0[32 * (size_t)j], hg32.data() + 32, 32);
  }
  const uint32_t empty_key = prove_ingest_key(BPP_PROVE_STAGE_LIVE_MASK, 0, BPP_PROVE_MSG_EMPTY);
  for (uint32_t k = 0; k < B; k++) {
    const bool live = c.live[rows[k].item] != 0;
    if (finding[k] != (live ? 0u : empty_key) || prove_ingest_key_msg(finding[k]) != (live ? BPP_PROVE_MSG_OK : BPP_PROVE_MSG_EMPTY))
      return bad("finding word differs", rows[k].item);
    ref[k] = c.items[rows[k].item];
    if (!live) {
      bpp_prove_item &s = ref[k];
      memset(&s, 0, sizeof(s));
      s.m = m_sorted[k];
      s.values = zero_v.data(), s.blindings32 = one_r.data(), s.commitments32 = c.brought ? g0.data() : nullptr;
      s.rng_bytes = zero_rng.data(), s.rng_len = zero_rng.size();
      if (c.per_item) s.transcript_state = zero_state.data();
      else s.transcript_label = (const uint8_t *)"harness", s.label_len = 7;
    }
  }
  ProvePack pk;
  pk.pack(P, hg32.data(), ref.data(), B, true, true);
  if (pk.bytes != dev_bytes) return bad("bytes differ", 0);
  if (pk.minvals != dev_minvals || pk.minpres != dev_minpres) return bad("promise rows differ", 0);
  for (uint32_t k = 0; k < B; k++) {
    const ProveDesc &x = pk.desc[k], &y = dev_desc[k];
    if (x.m != y.m || x.wit_off != y.wit_off || x.commit_off != y.commit_off || x.ext_off != y.ext_off || x.minval_idx != y.minval_idx ||
        x.flags != y.flags || x.seed_off != y.seed_off || x.roff != y.roff || x.mslot != y.mslot)
      return bad("descriptor differs", k);
  }
  if (c.per_item && dev_states != ref_states) return bad("state rows differ", 0);
  return true;
}

void report(const std::string &name, bool ok) {
  if (ok && !g_poison) return;  // (one line per case, after its second pass)
  printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
}

void live_masks() {
  const char *const forms[5] = {"all_live", "all_dead", "alternating", "only_first", "only_last"};
  for (int form = 0; form < 5; form++) {
    bool ok = true;
    for (uint32_t t : {1u, 3u})
      for (size_t n : {(size_t)1, (size_t)5, (size_t)67}) {
        std::vector<uint8_t> live(n, 0);
        for (size_t i = 0; i < n; i++)
          live[i] = form == 0 ? 1 : form == 1 ? 0 : form == 2 ? (uint8_t)(i % 2 == 0) : form == 3 ? (uint8_t)(i == 0) : (uint8_t)(i == n - 1);
        const ParamShape P{32, 8, t};
        for (int per_item = 0; per_item < 2; per_item++)
          for (int brought = 0; brought < 2; brought++) {
            Case c(P, n, live, brought != 0, per_item != 0);
            ok = run(forms[form], c, 16) && ok;
            ok = run(forms[form], c, 1) && ok;
          }
      }
    report(std::string("live_mask_") + forms[form], ok);
  }
}

// ---- the emit routine's by-item outputs and the summary against a plain loop
struct Table {
  std::vector<uint32_t> msg;      // per item: what it ends with
  std::vector<uint8_t> refused;   // per item: the host refused it (its row carries the finding)
};

bool summary_case(const char *name, const Table &tb) {
  const uint32_t n = (uint32_t)tb.msg.size();
  auto bad = [&](const char *what) {
    printf("FAIL %s: %s (poison %d)\n", name, what, (int)g_poison);
    g_failures++;
    return false;
  };
  // the rows: refused items in a table of their own, the others as slots in reverse order (a sort the summary must undo)
  std::vector<ProveDevRow> slot_rows, refused_rows;
  for (uint32_t i = n; i-- > 0;) {
    if (tb.refused[i]) refused_rows.push_back(ProveDevRow{i, 3, 0, tb.msg[i], 0});
    else slot_rows.push_back(ProveDevRow{i, 1, 40, 0, 3});
  }
  const uint32_t S = (uint32_t)slot_rows.size(), plen = 40;
  std::vector<uint32_t> finding(S, 0), status(S, 0);
  for (uint32_t k = 0; k < S; k++) {
    const uint32_t msg = tb.msg[slot_rows[k].item];
    if (msg == BPP_PROVE_MSG_EMPTY) finding[k] = prove_ingest_key(BPP_PROVE_STAGE_LIVE_MASK, 0, msg);
    else if (msg == BPP_PROVE_MSG_OPENING) status[k] = 2;
    else if (msg == BPP_PROVE_MSG_IDENTITY) status[k] = 1;
    else if (msg) finding[k] = prove_ingest_key(BPP_PROVE_STAGE_OPENINGS, 0, msg);
  }
  std::vector<uint8_t> proofs((size_t)S * plen + 1, 0x11), commit32((size_t)S * 32 + 1, 0x22), proofs_out((size_t)n * plen, 0xa5), commits_out((size_t)n * 32, 0xa5);
  std::vector<uint8_t> ok_mask(n, 0xa5);
  std::vector<bpp_device_prove_status> status_dev(n, bpp_device_prove_status{-99, 99}), outcome(n, bpp_device_prove_status{-99, 99});
  ProveEmit e;
  memset(&e, 0, sizeof(e));
  e.proofs_out = proofs_out.data(), e.proof_stride = plen, e.commitments_out = commits_out.data(), e.commit_stride = 32;
  e.status_dev = status_dev.data(), e.ok_mask = ok_mask.data(), e.outcome_item = outcome.data();
  e.rows = refused_rows.data(), e.n = (uint32_t)refused_rows.size(), e.slots = 0;
  for (uint32_t k = 0; k < e.n; k++)
    for (uint32_t lane = 0; lane < 16; lane++) prove_emit_row(e, k, lane, 16);
  e.rows = slot_rows.data(), e.n = S, e.slots = 1, e.finding = finding.data(), e.status = (const uint8_t *)status.data(), e.status_stride = 4;
  e.proofs = proofs.data(), e.plen = plen, e.commit32 = commit32.data(), e.mslot = 1;
  for (uint32_t k = 0; k < S; k++)
    for (uint32_t lane = 0; lane < 16; lane++) prove_emit_row(e, k, lane, 16);
  // the plain loop
  bpp_device_prove_summary want;
  memset(&want, 0, sizeof(want));
  want.flags = BPP_PROVE_SUMMARY_WRITTEN;
  bool found = false;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t msg = tb.msg[i];
    if (outcome[i].msg != msg || outcome[i].code != prove_msg_code(msg)) return bad("outcome record differs");
    if (status_dev[i].msg != msg || status_dev[i].code != prove_msg_code(msg)) return bad("status record differs");
    if (ok_mask[i] != (msg == BPP_PROVE_MSG_OK ? 1 : 0)) return bad("ok mask differs");
    if (msg == BPP_PROVE_MSG_OK) want.n_ok++;
    else if (msg == BPP_PROVE_MSG_EMPTY) want.n_empty++;
    else {
      want.n_failed++;
      if (!found) want.code = prove_msg_code(msg), want.msg = msg, want.index = i, found = true;
    }
    const bool zeroed = msg != BPP_PROVE_MSG_OK && !tb.refused[i];  // (a refused row here holds no lengths: nothing of it is touched)
    const uint8_t p0 = proofs_out[(size_t)i * plen], c0 = commits_out[(size_t)i * 32];
    if (msg == BPP_PROVE_MSG_OK ? (p0 != 0x11 || c0 != 0x22) : zeroed ? (p0 != 0 || c0 != 0) : (p0 != 0xa5 || c0 != 0xa5)) return bad("output rows differ");
  }
  for (uint32_t lanes : {(uint32_t)BPP_PROVE_SUMMARY_BLOCK, 1u}) {
    bpp_device_prove_summary got;
    memset(&got, 0xee, sizeof(got));
    prove_summary_run_host(outcome.data(), n, lanes, &got);
    if (memcmp(&got, &want, sizeof(got)) != 0) {
      printf("  want {%d %u %u %u %u %u %u} got {%d %u %u %u %u %u %u}\n", want.code, want.msg, want.index, want.flags, want.n_ok, want.n_failed,
             want.n_empty, got.code, got.msg, got.index, got.flags, got.n_ok, got.n_failed, got.n_empty);
      return bad("summary differs");
    }
  }
  return true;
}

void summaries() {
  for (uint32_t n : {1u, 5u, 67u, 700u}) {
    const std::string tag = "_" + std::to_string(n);
    auto table = [&] { return Table{std::vector<uint32_t>(n, 0), std::vector<uint8_t>(n, 0)}; };
    {
      Table t = table();
      report("summary_none" + tag, summary_case("summary_none", t));
    }
    for (uint32_t at : {0u, n / 2, n - 1}) {
      Table t = table();
      t.msg[at] = BPP_PROVE_MSG_VALUE;
      report("summary_finding_at_" + std::to_string(at) + tag, summary_case("summary_finding", t));
    }
    if (n >= 5) {
      Table t = table();
      t.msg[n - 2] = BPP_PROVE_MSG_BLINDING, t.msg[n / 2] = BPP_PROVE_MSG_OPENING;
      report("summary_two_findings" + tag, summary_case("summary_two_findings", t));
      Table r = table();
      for (uint32_t i = 1; i < n; i += 3) r.refused[i] = 1, r.msg[i] = BPP_PROVE_MSG_POWER_OF_TWO;
      r.msg[n - 1] = BPP_PROVE_MSG_IDENTITY, r.refused[n - 1] = 0;
      r.msg[0] = BPP_PROVE_MSG_EMPTY;
      report("summary_refused_interleaved" + tag, summary_case("summary_refused_interleaved", r));
    }
    {
      Table t = table();
      for (auto &x : t.msg) x = BPP_PROVE_MSG_EMPTY;
      report("summary_all_empty" + tag, summary_case("summary_all_empty", t));
    }
    {
      Table t = table();
      for (auto &x : t.msg) x = BPP_PROVE_MSG_MINIMUM;
      report("summary_all_fail" + tag, summary_case("summary_all_fail", t));
    }
  }
}

}  // namespace

int main() {
  for (int pass = 0; pass < 2; pass++) {
    g_poison = pass == 1;
    rng.seed(20261021);
    live_masks();
    summaries();
  }
  if (g_failures) {
    printf("FAILED %d\n", g_failures);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
