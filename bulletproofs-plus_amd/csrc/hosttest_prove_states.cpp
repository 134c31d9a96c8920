// Sanitizer harness (CPU test suite only): the per-item transcripts of bpp_prove_openings_device_transcripts as prove_ingest.h has
// them -- the finding stage of prove_ingest_check, the plan of prove_plan_device, the starting bytes and the call-wide head of
// k_prove_item_states (its host model: the same BPP_HD routines, the appends on merlin.h's sponge) and the out-row rule of
// prove_emit_row -- run on the host lane by lane (16 lanes per item as the kernels have them, and one) and held to ProvePack::pack and
// prove_item_check_host on the sorted equivalent items, each with transcript_state = its row.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_prove_states_host.py runs.
// The rows are n x 203 dense bytes (at an odd address whenever n is odd) inside a larger block whose other bytes are poisoned in the
// second pass: the bytes in front of row 0 and past row n - 1, and, of a row whose pos is bad, everything but byte 200 (as far
// as ASan's granules of eight allow; in the first pass those bytes hold 0xFF and the outputs must not depend on them).  The out rows
// end with the allocation.  Prints one "ok <case>" line per case.
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

const uint8_t ORDER[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                           0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
const uint32_t MS = 8, ROW = BPP_ITEM_STATE_BYTES, WORDS = 52;

size_t rng_need(const ParamShape &P, uint32_t m) { return 32 * (size_t)(prove_rounds_host(P, m) + 3); }

// what a case says about item i beyond its place in the m pattern
struct Spec {
  uint32_t m = 1;
  int pos = -1;            // >= 0: byte 200 of its row
  bool bad_blinding = false, bad_nonce = false, nonce = false;
};

std::vector<Spec> pattern(size_t n) {
  static const uint32_t ms[5] = {1, 4, 2, 8, 1};
  std::vector<Spec> v(n);
  for (size_t i = 0; i < n; i++) v[i].m = ms[i % 5];
  return v;
}

struct Case {
  ParamShape P;
  size_t n;
  std::vector<Spec> spec;
  std::vector<uint32_t> m;
  std::vector<uint8_t> values, blind, seeds, seed_present, rngb;
  size_t rng_stride;
  uint8_t *block = nullptr, *states = nullptr;  // states = block + lead: an odd address whenever n is odd, a granule in front
  size_t block_len = 0, lead = 0;
  std::vector<std::vector<uint8_t>> row_copy;   // what the equivalent items point to: copies, whole
  std::vector<bpp_prove_item> items;
  bpp_prove_arrays in;

  Case(const ParamShape &P_, const std::vector<Spec> &s) : P(P_), n(s.size()), spec(s), rng_stride(rng_need(P_, P_.m_max)) {
    const uint32_t t = P.t;
    values.assign(n * MS * 8, 0), blind.assign(n * MS * t * 32, 0), seeds.assign(n * 32, 0), seed_present.assign(n, 0), rngb.assign(n * rng_stride, 0);
    for (auto &b : rngb) b = (uint8_t)rng();
    lead = 8 + (8 - (n * ROW) % 8) % 8;  // the rows END with a granule, so every byte past row n - 1 can be poisoned
    block_len = lead + n * ROW + 16;
    block = (uint8_t *)malloc(block_len);
    memset(block, 0xff, block_len);
    states = block + lead;
    for (size_t i = 0; i < n; i++) {
      m.push_back(spec[i].m);
      const bool on_device = prove_item_layout_finding(P, spec[i].m, SIZE_MAX, true, SIZE_MAX, true) == 0;
      for (uint32_t j = 0; on_device && j < spec[i].m; j++) {
        const uint64_t v = rng() & 0xffffffffull;
        for (int k = 0; k < 8; k++) values[8 * (i * MS + j) + k] = (uint8_t)(v >> (8 * k));
        for (uint32_t q = 0; q < t; q++) {
          uint8_t *r = &blind[32 * ((i * MS + j) * t + q)];
          for (int k = 0; k < 32; k++) r[k] = (uint8_t)rng();
          r[31] &= 0x0f;
        }
      }
      if (spec[i].bad_blinding) memcpy(&blind[32 * (i * MS * t + (size_t)spec[i].m * t - 1)], ORDER, 32);  // the item's last one
      seed_present[i] = spec[i].nonce ? 1 : 0;
      for (int k = 0; k < 32; k++) seeds[32 * i + k] = spec[i].bad_nonce ? 0xff : (k == 31 ? 0x01 : (uint8_t)rng());
      // the row: a Merlin transcript under a label of its own with one message appended, then the byte the case asks for
      Strobe st;
      const std::string label = "item " + std::to_string(i);
      merlin_new(st, (const uint8_t *)label.data(), (uint32_t)label.size());
      std::vector<uint8_t> msg(1 + (7 * i) % 150, (uint8_t)i);
      merlin_append_message(st, (const uint8_t *)"ctx", 3, msg.data(), (uint32_t)msg.size());
      uint8_t *row = states + i * ROW;
      strobe_to_bytes(row, st);
      if (spec[i].pos >= 0) row[BPP_ITEM_STATE_POS] = (uint8_t)spec[i].pos;
      row_copy.push_back(std::vector<uint8_t>(row, row + ROW));
      if (row[BPP_ITEM_STATE_POS] >= BPP_STROBE_R || !on_device)  // nothing of it but byte 200 may matter (a refused item's: not even that)
        for (uint32_t q = 0; q < ROW; q++)
          if (q != BPP_ITEM_STATE_POS || !on_device) row[q] = 0xff;
      if (!on_device) row_copy.back().assign(ROW, 0);  // (the item form fails such an item before it looks at its state)
    }
    if (g_poison) poison(true);
    memset(&in, 0, sizeof(in));
    in.n_items = n, in.m = m.data(), in.m_stride = MS;
    in.values = (const uint64_t *)values.data(), in.blindings32 = blind.data(), in.seed_nonces32 = seeds.data(), in.seed_present = seed_present.data();
    in.rng_bytes = rngb.data(), in.rng_stride = rng_stride;
    items.assign(n, bpp_prove_item{});
    for (size_t i = 0; i < n; i++) {
      bpp_prove_item &o = items[i];
      o.values = (const uint64_t *)&values[8 * i * MS], o.blindings32 = &blind[32 * i * MS * t], o.m = m[i];
      o.seed_nonce32 = seed_present[i] ? &seeds[32 * i] : nullptr;
      o.transcript_state = row_copy[i].data();
      o.rng_bytes = &rngb[i * rng_stride], o.rng_len = rng_stride;
    }
  }
  void poison(bool on) {
    if (!on) {
      UNPOISON(block, block_len);
      return;
    }
    POISON(block, 8);  // (the granule in front)
    for (size_t i = 0; i < n; i++) {
      const uint8_t *row = states + i * ROW;
      const bool refused = prove_item_layout_finding(P, m[i], SIZE_MAX, true, SIZE_MAX, true) != 0;
      bool bad;
      {
        UNPOISON(row + BPP_ITEM_STATE_POS, 1);
        bad = row[BPP_ITEM_STATE_POS] >= BPP_STROBE_R;
      }
      if (!bad && !refused) continue;
      // the whole granules inside the row, but the one that holds byte 200 of a row that reaches the device
      for (size_t g = ((size_t)(row - block) + 7) / 8 * 8; g + 8 <= (size_t)(row + ROW - block); g += 8) {
        const size_t pos_at = (size_t)(row + BPP_ITEM_STATE_POS - block);
        if (!refused && g <= pos_at && pos_at < g + 8) continue;
        POISON(block + g, 8);
      }
    }
    POISON(block + lead + n * ROW, 16);
  }
  Case(const Case &) = delete;
  ~Case() {
    poison(false);
    free(block);
  }
};

struct Outcome {
  int code;
  std::string msg;
  bool operator==(const Outcome &o) const { return code == o.code && msg == o.msg; }
};
Outcome host_outcome(const ParamShape &P, const bpp_prove_item &it) {
  try {
    prove_item_check_host(P, it, SIZE_MAX, true, SIZE_MAX);
  } catch (const ProofErr &e) {
    return Outcome{e.code, e.msg};
  }
  return Outcome{BPP_OK, ""};
}

bool run(const char *name, Case &c, uint32_t lanes, const std::vector<uint32_t> &expect) {
  const ParamShape &P = c.P;
  const uint32_t t = P.t;
  std::vector<uint8_t> hg32((size_t)(t + 1) * 32);
  for (auto &b : hg32) b = (uint8_t)rng();
  auto bad = [&](const char *what, size_t i) {
    printf("FAIL %s: %s at %zu (t %u, lanes %u, poison %d)\n", name, what, i, t, lanes, (int)g_poison);
    g_failures++;
    return false;
  };
  // the engine's shape step (the rows hold rng_stride = what the largest m needs: no rng finding)
  ProveDeviceShape sh;
  if (!prove_device_shape(P, c.m.data(), c.n, MS, c.rng_stride, SIZE_MAX, SIZE_MAX, true, sh)) return bad("m_stride is below", sh.m_stride_below);
  std::vector<uint32_t> msg = sh.msg;
  const std::vector<ProveDevRow> &refused = sh.refused, &rows = sh.rows;
  const std::vector<uint32_t> &m_sorted = sh.m_sorted;
  for (size_t i = 0; i < c.n; i++) {
    if (!msg[i]) continue;
    const Outcome want = host_outcome(P, c.items[i]), got{prove_msg_code(msg[i]), prove_msg_text(msg[i])};
    if (!(want == got)) return bad("host finding differs", i);
  }
  const uint32_t B = (uint32_t)rows.size();
  // ---- the plan: no state table, slot k of a sub-batch reads row k of the sub-batch's own
  const uint32_t sub = prove_sub_size(B, 0);
  if (sub != 64) return bad("the sub-batch cut is not at 64", B);
  ProvePack plan;
  if (B) prove_plan_device(P, hg32.data(), m_sorted.data(), B, false, nullptr, nullptr, 0, plan, sub);
  if (!plan.states.empty()) return bad("the plan holds a state table", 0);
  for (uint32_t k = 0; k < B; k++)
    if (plan.desc[k].state_idx != k % 64) return bad("state_idx is not the slot's index in its sub-batch", k);
  // (and the call-level form is what it was: one state per distinct m)
  if (B) {
    ProvePack old;
    prove_plan_device(P, hg32.data(), m_sorted.data(), B, false, nullptr, (const uint8_t *)"x", 1, old);
    uint32_t distinct = 0;
    for (uint32_t k = 0; k < B; k++) distinct += k == 0 || m_sorted[k] != m_sorted[k - 1];
    if (old.states.size() != (size_t)distinct * ROW || prove_states_table_bytes(old, 0, 64) != old.states.size()) return bad("call-level plan changed", 0);
  }
  // ---- the sub-batches: ingest (the findings), then the states kernel into a table that ends where its rows end
  std::vector<uint32_t> finding(B, 0xdeadbeefu);
  std::vector<uint8_t> dev_states;
  for (uint32_t lo = 0; lo < B; lo += sub) {
    const uint32_t nb = std::min(sub, B - lo);
    if (prove_states_table_bytes(plan, sub, nb) != (size_t)nb * ROW) return bad("d_states is not nb x 203", lo);
    const size_t bytes_lo = plan.desc[lo].wit_off, bytes_len = (lo + nb < B ? plan.desc[lo + nb].wit_off : plan.bytes_len) - bytes_lo;
    std::vector<ProveDesc> d(plan.desc.begin() + lo, plan.desc.begin() + lo + nb);
    for (uint32_t i = 0; i < nb; i++) {
      d[i].wit_off -= (uint32_t)bytes_lo, d[i].commit_off -= (uint32_t)bytes_lo, d[i].ext_off -= (uint32_t)bytes_lo, d[i].seed_off -= (uint32_t)bytes_lo;
      d[i].minval_idx = i * plan.m;
    }
    std::vector<uint8_t> bytes(bytes_len, 0xa5), minpres((size_t)nb * plan.m, 0);
    std::vector<uint64_t> minvals((size_t)nb * plan.m, 0);
    ProveIngest a;
    memset(&a, 0, sizeof(a));
    a.values = c.values.data(), a.blindings32 = c.blind.data(), a.seed_nonces32 = c.seeds.data(), a.seed_present = c.seed_present.data();
    a.rng_bytes = c.rngb.data(), a.rng_stride = c.rng_stride, a.m_stride = MS, a.n_bits = P.n_bits, a.t = t, a.nb = nb, a.g0_32 = hg32.data() + 32;
    a.rows = rows.data() + lo, a.desc = d.data(), a.bytes = bytes.data(), a.minvals = minvals.data(), a.minpres = minpres.data();
    a.finding = finding.data() + lo;
    a.item_states = c.states;
    prove_ingest_run_host(a, lanes);
    uint8_t *table = (uint8_t *)malloc((size_t)nb * ROW);
    ProveItemStates s;
    memset(&s, 0, sizeof(s));
    s.src = c.states, s.rows = rows.data() + lo, s.desc = d.data(), s.finding = finding.data() + lo, s.hg32 = hg32.data();
    s.n_bits = P.n_bits, s.t = t, s.nb = nb, s.states = table;
    prove_item_states_run_host(s);
    dev_states.insert(dev_states.end(), table, table + (size_t)nb * ROW);
    free(table);
  }
  // ---- findings against the item form; the reference items: a failed one is the substitute under the fixed public state
  const std::vector<uint8_t> zero_state(ROW, 0), zero_rng(rng_need(P, P.m_max), 0);
  const std::vector<uint64_t> zero_v(P.m_max, 0);
  std::vector<uint8_t> one_r((size_t)P.m_max * t * 32, 0);
  for (uint32_t j = 0; j < P.m_max; j++) one_r[(size_t)j * t * 32] = 1;
  std::vector<bpp_prove_item> ref(B);
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
      s.values = zero_v.data(), s.blindings32 = one_r.data(), s.seed_nonce32 = nullptr, s.rng_bytes = zero_rng.data(), s.rng_len = zero_rng.size();
      s.transcript_state = zero_state.data();
    }
  }
  for (size_t i = 0; i < c.n; i++)
    if (msg[i] != expect[i]) {
      printf("  item %zu: message id %u, expected %u\n", i, msg[i], expect[i]);
      return bad("not the expected finding", i);
    }
  if (B) {
    ProvePack pk;
    pk.pack(P, hg32.data(), ref.data(), B, true, true);
    for (uint32_t k = 0; k < B; k++)
      if (memcmp(&pk.states[(size_t)pk.desc[k].state_idx * ROW], &dev_states[(size_t)k * ROW], ROW) != 0) return bad("state row differs from the packer's", k);
  }
  // ---- the out rows: an allocation that ends with row n - 1, at an odd address; the arena rows hold a pattern
  uint8_t *out_block = (uint8_t *)malloc(1 + c.n * ROW);
  memset(out_block, 0xa5, 1 + c.n * ROW);
  uint8_t *out = out_block + 1;
  std::vector<uint8_t> proofs_out(c.n * 1024, 0), commits_out(c.n * MS * 32, 0);
  auto emit = [&](const ProveDevRow *r, uint32_t cnt, bool slots, const uint32_t *fnd, const uint32_t *trows, const uint8_t *status,
                  const uint8_t *proofs, const uint8_t *commit32, uint32_t mslot) {
    ProveEmit e;
    memset(&e, 0, sizeof(e));
    e.rows = r, e.n = cnt, e.slots = slots ? 1 : 0, e.finding = fnd, e.status = status, e.status_stride = 4, e.proofs = proofs, e.plen = 1024;
    e.commit32 = commit32, e.mslot = mslot, e.proofs_out = proofs_out.data(), e.proof_stride = 1024, e.commitments_out = commits_out.data();
    e.commit_stride = MS * 32, e.tstates = trows, e.tstate_words = WORDS, e.states_out = out;
    for (uint32_t k = 0; k < cnt; k++)
      for (uint32_t lane = 0; lane < lanes; lane++) prove_emit_row(e, k, lane, lanes);
  };
  if (!refused.empty()) emit(refused.data(), (uint32_t)refused.size(), false, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  std::vector<uint32_t> trows((size_t)B * WORDS);
  for (auto &w : trows) w = (uint32_t)rng() | 0x01010101u;  // (no zero byte: a zeroed row cannot pass for a given one)
  std::vector<uint8_t> status((size_t)B * 4, 0), proofs((size_t)B * 1024, 0x11), commit32((size_t)B * P.m_max * 32, 0x22);
  if (B) emit(rows.data(), B, true, finding.data(), trows.data(), status.data(), proofs.data(), commit32.data(), P.m_max);
  std::vector<int> slot_of(c.n, -1);
  for (uint32_t k = 0; k < B; k++) slot_of[rows[k].item] = (int)k;
  bool rows_ok = out_block[0] == 0xa5;
  for (size_t i = 0; i < c.n; i++) {
    const uint8_t *got = out + i * ROW;
    if (msg[i] == 0) rows_ok = rows_ok && memcmp(got, (const uint8_t *)&trows[(size_t)slot_of[i] * WORDS], ROW) == 0;
    else
      for (uint32_t q = 0; q < ROW; q++) rows_ok = rows_ok && got[q] == 0;
  }
  free(out_block);
  if (!rows_ok) return bad("out rows: not give-or-zero", 0);
  return true;
}

bool both(const char *name, Case &c, const std::vector<uint32_t> &expect) { return run(name, c, 16, expect) && run(name, c, 1, expect); }

void report(const char *name, bool ok) {
  if (ok && !g_poison) return;  // (one line per case, after its second pass)
  printf("%s %s\n", ok ? "ok" : "FAIL", name);
}

void corpus() {
  const uint32_t T = BPP_PROVE_MSG_TRANSCRIPT_STATE;
  bool plan_ok = true, first_middle_last = true, edges = true, precedence = true, refused_ok = true, all_bad = true;
  for (uint32_t t : {1u, 3u}) {
    const ParamShape P{32, 8, t};
    for (size_t n : {(size_t)5, (size_t)17, (size_t)67}) {
      {
        Case c(P, pattern(n));
        plan_ok = both("plan_5_17_67", c, std::vector<uint32_t>(n, 0)) && plan_ok;
      }
      // a bad pos alone at the first, a middle and the last item
      for (size_t at : {(size_t)0, n / 2, n - 1}) {
        std::vector<Spec> v = pattern(n);
        std::vector<uint32_t> expect(n, 0);
        v[at].pos = 166, expect[at] = T;
        Case c(P, v);
        first_middle_last = both("bad_pos_first_middle_last", c, expect) && first_middle_last;
      }
    }
    {
      std::vector<Spec> v = pattern(7);
      std::vector<uint32_t> expect(7, 0);
      v[1].pos = 165;                   // the last position there is
      v[2].pos = 166, expect[2] = T;    // the rate
      v[4].pos = 255, expect[4] = T;
      v[5].pos = 0;
      Case c(P, v);
      edges = both("pos_165_166_255", c, expect) && edges;
    }
    {
      // the transcript finding is an item's LAST: behind a blinding factor, behind the nonce, behind a nonce on an aggregated item
      std::vector<Spec> v = pattern(10);
      std::vector<uint32_t> expect(10, 0);
      v[3].pos = 200, v[3].bad_blinding = true, expect[3] = BPP_PROVE_MSG_BLINDING;
      v[0].pos = 166, v[0].nonce = true, v[0].bad_nonce = true, expect[0] = BPP_PROVE_MSG_SEED_NONCE;
      v[2].pos = 255, v[2].nonce = true, expect[2] = BPP_PROVE_MSG_SEED_AGGREGATED;
      v[4].nonce = true;                // a good nonce beside a good row
      v[5].pos = 166, v[5].nonce = true, expect[5] = T;  // ... beside a bad one
      v[6].bad_blinding = true, expect[6] = BPP_PROVE_MSG_BLINDING;
      Case c(P, v);
      precedence = both("precedence", c, expect) && precedence;
    }
    {
      // items the host refuses: their rows are never read (0xFF / poisoned as a whole), their out rows are zeroed
      std::vector<Spec> v = pattern(6);
      v[1].m = 3, v[2].m = 0, v[5].m = 16, v[3].pos = 166;
      std::vector<uint32_t> expect = {0, BPP_PROVE_MSG_POWER_OF_TWO, BPP_PROVE_MSG_POWER_OF_TWO, T, 0, BPP_PROVE_MSG_GENERATORS};
      Case c(P, v);
      refused_ok = both("refused_rows", c, expect) && refused_ok;
      std::vector<Spec> w(3);
      w[0].m = 3, w[1].m = 0, w[2].m = 16;  // no item reaches the device: the rows are zeroed all the same
      Case d(P, w);
      refused_ok = both("refused_rows", d, {BPP_PROVE_MSG_POWER_OF_TWO, BPP_PROVE_MSG_POWER_OF_TWO, BPP_PROVE_MSG_GENERATORS}) && refused_ok;
    }
    {
      std::vector<Spec> v = pattern(5);
      for (Spec &s : v) s.pos = 166 + (int)(rng() % 90);
      Case c(P, v);
      all_bad = both("every_row_bad", c, std::vector<uint32_t>(5, T)) && all_bad;
    }
  }
  report("plan_5_17_67", plan_ok);
  report("bad_pos_first_middle_last", first_middle_last);
  report("pos_165_166_255", edges);
  report("precedence", precedence);
  report("refused_rows", refused_ok);
  report("every_row_bad", all_bad);
}

}  // namespace

int main() {
  for (int pass = 0; pass < 2; pass++) {
    g_poison = pass == 1;
    rng.seed(20261021);
    corpus();
  }
  if (g_failures) {
    printf("FAILED %d\n", g_failures);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
