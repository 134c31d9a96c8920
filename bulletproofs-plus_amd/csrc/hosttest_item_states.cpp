// Sanitizer harness (CPU test suite only): the one-lane host models of item_states.h -- k_item_states in its three forms (every
// row, a live count, a live mask) and the row rule of k_states_out -- held to what upload_host.h makes of the EQUIVALENT ITEM ARRAY:
// the live items in slot order, item k under transcript_state = the row of its slot.
//   clean rows            every live slot's row equals the row upload_pass_a's table holds for the item (through state_idx); dead
//                         slots hold 203 zero bytes; no finding
//   bad states            pos 166 and 255 at live and dead slots, at the first and the last slot, alone: the finding's index is the
//                         slot of tr_err_index, code and text are those upload_pass_b throws; the bad row's slot holds zeros, a bad
//                         state at a dead slot is no finding
//   with a bad scalar     at the same index the scalar's finding wins, at a higher index the transcript's
//   dead rows             poisoned with 0xff (a `pos` read there would be a finding), and the source array ENDS behind the last live
//                         row: an exact-size heap allocation, so a load from a dead row behind it is an ASan report
//   base address          the source at each of the four byte offsets
//   states out            a table of records and liveness views: only the exact Ok record hands a live slot's row out, the 203 bytes
//                         the blocking form makes of the row; zeros everywhere else; the caller's array at each byte offset
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_item_states_host.py runs.  One "ok <case>" line
// per case.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "item_states.h"

using namespace bpp;

namespace {

std::mt19937_64 rng(20261021);
const ParamShape SHAPE{32, 4, 1};
const uint32_t ROUNDS = 5;  // m = 1, n_bits = 32

#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                    \
      fprintf(stderr, "\n");                           \
      exit(1);                                         \
    }                                                  \
  } while (0)

void canonical_scalar(uint8_t *p) {
  for (int i = 0; i < 32; i++) p[i] = (uint8_t)rng();
  p[31] &= 0x0f;  // < 2^252 < l
}

// wire bytes with the structure of a proof: [t] d1[t] A A1 B r1 s1 (L R)*rounds
std::vector<uint8_t> make_proof() {
  const uint32_t t = SHAPE.t;
  std::vector<uint8_t> p(1 + 32 * (size_t)(t + 5 + 2 * (size_t)ROUNDS));
  p[0] = (uint8_t)t;
  for (size_t i = 1; i < p.size(); i++) p[i] = (uint8_t)rng();
  for (uint32_t k = 0; k < t; k++) canonical_scalar(&p[1 + 32 * k]);
  canonical_scalar(&p[1 + 32 * (t + 3)]);
  canonical_scalar(&p[1 + 32 * (t + 4)]);
  return p;
}

void make_state(uint8_t *row, uint8_t pos) {
  for (int k = 0; k < 200; k++) row[k] = (uint8_t)rng();
  row[200] = pos;
  row[201] = (uint8_t)(pos ? rng() % pos : 0);
  row[202] = 2;
}

enum Form { PLAIN, COUNT, MASK };

// one scenario: n slots, which are live, which states are bad (and how), which proofs carry a non-canonical r1
struct Scenario {
  size_t n;
  Form form;
  std::vector<uint8_t> live;           // per slot (PLAIN: all ones; COUNT: a prefix)
  std::vector<int> bad_pos;            // per slot: -1 a good state, else the pos byte (166, 255)
  std::vector<uint8_t> bad_scalar;     // per slot
  uint32_t base_offset;                // byte offset of the source array inside its allocation
};

// runs the scenario: the model against the item form of the live rows
void run(const Scenario &sc, const char *name) {
  const size_t n = sc.n;
  std::vector<std::vector<uint8_t>> proofs(n);
  for (size_t i = 0; i < n; i++) {
    proofs[i] = make_proof();
    if (sc.bad_scalar[i]) memset(&proofs[i][1 + 32 * (SHAPE.t + 3)], 0xff, 32);  // r1 >= l
  }
  const size_t len = proofs[0].size();
  size_t last_live = 0, n_live = 0;
  for (size_t i = 0; i < n; i++)
    if (sc.live[i]) last_live = i + 1, n_live++;
  // the caller's arrays END behind the last live row; dead rows in front of it are poisoned
  std::unique_ptr<uint8_t[]> pbuf(new uint8_t[last_live * len + 1]), cbuf(new uint8_t[last_live * 32 + 1]);
  const size_t src_bytes = last_live * (size_t)BPP_ITEM_STATE_BYTES;
  std::unique_ptr<uint8_t[]> sbuf(new uint8_t[sc.base_offset + src_bytes]);
  uint8_t *src = sbuf.get() + sc.base_offset;
  memset(sbuf.get(), 0xff, sc.base_offset + src_bytes);
  for (size_t i = 0; i < last_live; i++) {
    memcpy(pbuf.get() + i * len, proofs[i].data(), len);
    for (int k = 0; k < 32; k++) cbuf[32 * i + k] = (uint8_t)rng();
    if (sc.live[i]) make_state(src + i * BPP_ITEM_STATE_BYTES, sc.bad_pos[i] < 0 ? (uint8_t)(rng() % BPP_STROBE_R) : (uint8_t)sc.bad_pos[i]);
    else if (sc.bad_pos[i] >= 0) src[i * BPP_ITEM_STATE_BYTES + BPP_ITEM_STATE_POS] = (uint8_t)sc.bad_pos[i];  // (0xff everywhere else)
  }

  // ---- the reference: the item array of the live rows, in slot order
  std::vector<size_t> slot_of;
  std::vector<bpp_verify_item> items;
  for (size_t i = 0; i < n; i++) {
    if (!sc.live[i]) continue;
    bpp_verify_item it;
    memset(&it, 0, sizeof(it));
    it.proof = pbuf.get() + i * len;
    it.proof_len = len;
    it.commitments32 = cbuf.get() + 32 * i;
    it.m = 1;
    it.transcript_state = src + i * BPP_ITEM_STATE_BYTES;
    items.push_back(it);
    slot_of.push_back(i);
  }
  bool ref_threw = false;
  ProofErr ref_err{BPP_OK, ""};
  UploadPlan pl;
  if (n_live) {
    upload_pass_a(items.data(), items.size(), pl);
    std::vector<uint8_t> bytes(pl.bytes_total + BPP_BYTES_SLACK);
    const ParallelFor serial = [](uint32_t k, const std::function<void(uint32_t)> &fn) {
      for (uint32_t q = 0; q < k; q++) fn(q);
    };
    try {
      upload_pass_b(items.data(), SHAPE, pl, bytes.data(), serial);
    } catch (const ProofErr &e) {
      ref_threw = true;
      ref_err = e;
    }
  }

  // ---- the model: the proofs' findings as the refill kernel reduces them, then item_states_run_host into the same word
  std::unique_ptr<uint8_t[]> table(new uint8_t[n * BPP_ITEM_STATE_BYTES]);
  memset(table.get(), 0xcd, n * BPP_ITEM_STATE_BYTES);
  uint32_t finding = 0, count_word = 0;
  std::unique_ptr<uint8_t[]> mask(new uint8_t[n]);
  for (size_t i = 0; i < n; i++) mask[i] = sc.live[i] ? 1 : 0;  // (the batch's normalised copy)
  if (sc.form == COUNT) count_word = (uint32_t)n_live;
  for (size_t i = 0; i < n; i++) {
    if (!sc.live[i]) continue;
    const IngestFinding f = ingest_check_item(pbuf.get() + i * len, len, 1, false, false);
    if (f.msg) {
      const uint32_t key = ingest_key((uint32_t)i, f.msg);
      if (key > finding) finding = key;
    }
  }
  const ItemStates a{src, table.get(), (uint32_t)n, (uint32_t)n, &finding, sc.form == COUNT ? &count_word : nullptr,
                     sc.form == MASK ? mask.get() : nullptr};
  item_states_run_host(a);
  const bpp_device_refill rec = refill_record(finding, 0, sc.form == COUNT ? count_word : (uint32_t)n, (uint32_t)n);

  // ---- the finding
  if (ref_threw) {
    CHECK(rec.flags == (BPP_REFILL_WRITTEN | BPP_REFILL_FINDING), "%s: no finding, the item form throws \"%s\"", name, ref_err.msg.c_str());
    CHECK(rec.code == ref_err.code, "%s: code %d, item form %d", name, rec.code, ref_err.code);
    CHECK(rec.index == slot_of[ref_err.index], "%s: index %u, item form's item %u lies at slot %zu", name, rec.index, ref_err.index,
          slot_of[ref_err.index]);
    CHECK(ref_err.msg == ingest_message(rec.msg), "%s: text \"%s\", item form \"%s\"", name, ingest_message(rec.msg), ref_err.msg.c_str());
    if (rec.msg == BPP_ING_TRANSCRIPT) CHECK(slot_of[pl.tr_err_index] == rec.index, "%s: tr_err_index", name);
  } else {
    CHECK(rec.flags == BPP_REFILL_WRITTEN && rec.code == BPP_OK && rec.msg == 0, "%s: a finding (msg %u at %u) the item form does not have", name, rec.msg, rec.index);
    if (n_live) CHECK(pl.tr_err_index == items.size(), "%s: tr_err_index without a throw", name);
  }
  // ---- the table
  static const uint8_t zeros[BPP_ITEM_STATE_BYTES] = {0};
  size_t k = 0;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *row = table.get() + i * BPP_ITEM_STATE_BYTES;
    if (!sc.live[i]) {
      CHECK(memcmp(row, zeros, BPP_ITEM_STATE_BYTES) == 0, "%s: dead slot %zu is not zero", name, i);
      continue;
    }
    if (sc.bad_pos[i] >= 0) {
      CHECK(memcmp(row, zeros, BPP_ITEM_STATE_BYTES) == 0, "%s: the bad row of slot %zu was copied", name, i);
    } else {
      // (pass A fills its table whether or not pass B throws: the row the item form would verify item k under)
      const uint8_t *want = &pl.states[(size_t)pl.desc[k].state_idx * BPP_ITEM_STATE_BYTES];
      CHECK(memcmp(row, want, BPP_ITEM_STATE_BYTES) == 0, "%s: slot %zu differs from the item form's row %u", name, i, pl.desc[k].state_idx);
    }
    k++;
  }
  printf("ok %s\n", name);
}

Scenario scenario(size_t n, Form form, uint32_t off) {
  Scenario sc;
  sc.n = n;
  sc.form = form;
  sc.live.assign(n, 1);
  sc.bad_pos.assign(n, -1);
  sc.bad_scalar.assign(n, 0);
  sc.base_offset = off;
  return sc;
}

void item_states_cases() {
  const size_t n = 21;
  char name[128];
  for (int form = PLAIN; form <= MASK; form++) {
    for (uint32_t off = 0; off < 4; off++) {
      auto base = [&]() {
        Scenario sc = scenario(n, (Form)form, off);
        if (form == COUNT)
          for (size_t i = 13; i < n; i++) sc.live[i] = 0;
        if (form == MASK)
          for (size_t i : {0, 3, 4, 9, 17, 19, 20}) sc.live[i] = 0;
        return sc;
      };
      auto go = [&](const Scenario &sc, const char *what) {
        snprintf(name, sizeof(name), "item_states form=%d offset=%u %s", form, off, what);
        run(sc, name);
      };
      Scenario sc = base();
      go(sc, "clean");
      size_t first_live = 0, last_live = 0;
      for (size_t i = 0; i < n; i++)
        if (sc.live[i]) last_live = i;
      while (!sc.live[first_live]) first_live++;
      sc = base();
      sc.bad_pos[first_live] = 166;
      go(sc, "bad first");
      sc = base();
      sc.bad_pos[last_live] = 255;
      go(sc, "bad last");
      sc = base();
      sc.bad_pos[7] = 255;
      sc.bad_pos[11] = 166;
      go(sc, "two bad, the lower wins");
      sc = base();
      sc.bad_pos[7] = 166;
      sc.bad_scalar[7] = 1;
      go(sc, "bad scalar at the same index wins");
      sc = base();
      sc.bad_pos[7] = 166;
      sc.bad_scalar[11] = 1;
      go(sc, "bad scalar at a higher index loses");
      sc = base();
      sc.bad_pos[11] = 255;
      sc.bad_scalar[7] = 1;
      go(sc, "bad scalar at a lower index wins");
      if (form != PLAIN) {
        sc = base();
        for (size_t i = 0; i < n; i++)
          if (!sc.live[i]) sc.bad_pos[i] = (i & 1) ? 166 : 255;
        go(sc, "bad states at dead slots only");
        sc.bad_pos[last_live] = 166;
        go(sc, "bad states at dead slots and the last live one");
      }
    }
  }
  // alone; nothing live (a count of zero, an all-zero mask: the source array has no byte at all)
  Scenario one = scenario(1, PLAIN, 1);
  run(one, "item_states one item, clean");
  one.bad_pos[0] = 166;
  run(one, "item_states one item, bad");
  for (int form = COUNT; form <= MASK; form++) {
    Scenario none = scenario(5, (Form)form, 3);
    none.live.assign(5, 0);
    run(none, form == COUNT ? "item_states count 0" : "item_states mask of zeros");
  }
  // a count beyond the batch makes nothing live
  {
    const size_t m = 4;
    std::unique_ptr<uint8_t[]> table(new uint8_t[m * BPP_ITEM_STATE_BYTES]), src(new uint8_t[1]);
    memset(table.get(), 0xcd, m * BPP_ITEM_STATE_BYTES);
    uint32_t finding = 0, count_word = (uint32_t)m + 1;
    const ItemStates a{src.get(), table.get(), (uint32_t)m, (uint32_t)m, &finding, &count_word, nullptr};
    item_states_run_host(a);
    for (size_t q = 0; q < m * BPP_ITEM_STATE_BYTES; q++) CHECK(table[q] == 0, "count beyond the batch: byte %zu", q);
    CHECK(finding == 0, "count beyond the batch: a finding");
    printf("ok item_states count beyond the batch\n");
  }
  // n_run: rows at and beyond it are not read (the mixed upload stops at the host's finding)
  {
    const size_t m = 6, run_to = 2;
    std::unique_ptr<uint8_t[]> table(new uint8_t[m * BPP_ITEM_STATE_BYTES]), src(new uint8_t[run_to * BPP_ITEM_STATE_BYTES]);
    for (size_t i = 0; i < run_to; i++) make_state(src.get() + i * BPP_ITEM_STATE_BYTES, 17);
    uint32_t finding = 0;
    const ItemStates a{src.get(), table.get(), (uint32_t)m, (uint32_t)run_to, &finding, nullptr, nullptr};
    item_states_run_host(a);
    CHECK(memcmp(table.get(), src.get(), run_to * BPP_ITEM_STATE_BYTES) == 0, "n_run: the rows of the run");
    for (size_t q = run_to * BPP_ITEM_STATE_BYTES; q < m * BPP_ITEM_STATE_BYTES; q++) CHECK(table[q] == 0, "n_run: byte %zu", q);
    printf("ok item_states n_run\n");
  }
}

// ---- states out
void states_out_cases() {
  const uint32_t B = 23, G = 4;
  const uint32_t group_first[G + 1] = {0, 1, 9, 16, 23};
  const uint32_t W = 1, RD = 2, RF = 4, EM = 8;  // BPP_VERDICT_* flags
  static_assert(BPP_VERDICT_WRITTEN == 1 && BPP_VERDICT_REDRAW == 2 && BPP_VERDICT_REFILL == 4 && BPP_VERDICT_EMPTY == 8, "verdict flags");
  const bpp_device_verdict ok{BPP_OK, BPP_TIER_NONE, 0, W};
  const std::vector<bpp_device_verdict> others = {
      {BPP_ERR_VERIFICATION_FAILED, BPP_TIER_MSM, 0, W}, {BPP_ERR_VERIFICATION_FAILED, BPP_TIER_PASS1, 3, W}, {BPP_OK, BPP_TIER_NONE, 0, W | EM},
      {BPP_OK, BPP_TIER_NONE, 0, W | RD},                {BPP_OK, BPP_TIER_NONE, 0, W | RF},                {BPP_ERR_INVALID_ARGUMENT, BPP_TIER_CONSTRUCTION, 2, W | RF},
      {BPP_OK, BPP_TIER_NONE, 0, 0},                     {BPP_OK, BPP_TIER_NONE, 1, W},                     {BPP_OK, BPP_TIER_PASS2, 0, W}};
  std::vector<uint32_t> rows((size_t)B * 52);
  for (auto &w : rows) w = (uint32_t)rng();
  uint32_t count_word = 18;
  std::vector<uint8_t> mask(B);
  for (uint32_t i = 0; i < B; i++) mask[i] = (i % 3 != 1) ? 1 : 0;
  const LiveView views[3] = {{nullptr, nullptr}, {&count_word, nullptr}, {nullptr, mask.data()}};
  size_t cases = 0;
  for (int v = 0; v < 3; v++)
    for (size_t o = 0; o <= others.size(); o++)
      for (uint32_t off = 0; off < 4; off++) {
        // group g is Ok unless it is the one that takes `others[o]` (o == size: every group Ok)
        std::vector<bpp_device_verdict> recs(G, ok);
        const uint32_t odd = (uint32_t)((o + v) % G);
        if (o < others.size()) recs[odd] = others[o];
        std::unique_ptr<uint8_t[]> out(new uint8_t[off + (size_t)B * BPP_ITEM_STATE_BYTES]);
        memset(out.get(), 0xcd, off + (size_t)B * BPP_ITEM_STATE_BYTES);
        const StatesOut a{rows.data(), 52, out.get() + off, recs.data(), group_first, G, B, views[v]};
        states_out_run_host(a);
        for (uint32_t q = 0; q < off; q++) CHECK(out[q] == 0xcd, "states_out: a byte in front of the array");
        for (uint32_t i = 0; i < B; i++) {
          uint32_t g = 0;
          while (group_first[g + 1] <= i) g++;
          const bool live = v == 0 ? true : (v == 1 ? i < count_word : mask[i] != 0);
          const bool give = live && !(o < others.size() && g == odd);
          uint8_t want[BPP_ITEM_STATE_BYTES] = {0};
          if (give) {  // (state_row_to_bytes of the engine)
            const uint32_t *row = &rows[(size_t)i * 52];
            memcpy(want, row, 200);
            want[200] = (uint8_t)row[50];
            want[201] = (uint8_t)(row[50] >> 8);
            want[202] = (uint8_t)(row[50] >> 16);
          }
          CHECK(memcmp(out.get() + off + (size_t)i * BPP_ITEM_STATE_BYTES, want, BPP_ITEM_STATE_BYTES) == 0, "states_out: view %d record %zu offset %u row %u", v,
                o, off, i);
        }
        cases++;
      }
  printf("ok states_out %zu tables\n", cases);
}

}  // namespace

int main() {
  item_states_cases();
  states_out_cases();
  printf("all ok\n");
  return 0;
}
