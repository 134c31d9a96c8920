// Sanitizer harness (CPU test suite only): the job copy bpp_prove_submit takes of its caller's items (prove_job_host.h: the
// per-item check, the deep copy, the wipe) and the prover's witness packer (prove_pack_host.h), built with  g++ -fsanitize=address,undefined  into an executable that
// tests/test_prove_pipeline_host.py runs.  Everything an item points to is an exact-size heap allocation, so a read past what the
// item declares, or a look behind the pointer of an item that fails the check, is an ASan report (exit code != 0).  Prints one
// "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>

#include <sanitizer/asan_interface.h>

#include "prove_job_host.h"
#include "prove_pack_host.h"

using namespace bpp;

namespace {

std::mt19937_64 rng(20240229);

struct Owned {  // owns exact-size copies of everything a bpp_prove_item points to
  std::unique_ptr<uint64_t[]> values, minv;
  std::unique_ptr<uint8_t[]> blind, commits, present, seed, state, label, ext;
  uint32_t m = 1, t = 1;
  size_t label_len = 0, ext_len = 0;
  bpp_prove_item view() const {
    bpp_prove_item v;
    memset(&v, 0, sizeof(v));
    v.values = values.get();
    v.blindings32 = blind.get();
    v.commitments32 = commits.get();
    v.m = m;
    v.min_values = minv.get();
    v.min_present = present.get();
    v.seed_nonce32 = seed.get();
    v.transcript_state = state.get();
    v.transcript_label = label.get();
    v.label_len = label_len;
    v.rng_bytes = ext.get();
    v.rng_len = ext_len;
    return v;
  }
};

void fill(uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(rng() | 1);  // (never zero: the wipe has something to show)
}
void canonical_scalar(uint8_t *p) {
  fill(p, 32);
  p[31] &= 0x0f;  // < 2^252 < l
  p[31] |= 1;
}

uint32_t rounds_of(const ParamShape &P, uint32_t m) {
  uint32_t r = 0;
  while ((1u << r) < m * P.n_bits) r++;
  return r;
}

// opt bits: 1 commitments, 2 min_values, 4 min_present (with min_values), 8 seed nonce (m == 1), 16 transcript state (else label),
// 32 no transcript at all, 64 extra rng bytes beyond what is needed
Owned make(const ParamShape &P, uint32_t m, unsigned opt) {
  Owned o;
  o.m = m;
  o.t = P.t;
  const size_t mm = m ? m : 1;
  o.values.reset(new uint64_t[mm]);
  for (size_t j = 0; j < mm; j++) o.values[j] = 100 + (rng() % 100);  // (fits the 8-bit parameters too)
  o.blind.reset(new uint8_t[32 * mm * P.t]);
  for (size_t q = 0; q < mm * P.t; q++) canonical_scalar(o.blind.get() + 32 * q);
  if (opt & 1) {
    o.commits.reset(new uint8_t[32 * mm]);
    fill(o.commits.get(), 32 * mm);
  }
  if (opt & (2 | 4)) {
    o.minv.reset(new uint64_t[mm]);
    for (size_t j = 0; j < mm; j++) o.minv[j] = 7;
  }
  if (opt & 4) {
    o.present.reset(new uint8_t[mm]);
    for (size_t j = 0; j < mm; j++) o.present[j] = (uint8_t)(j & 1) ^ 1;
  }
  if ((opt & 8) && m == 1) {
    o.seed.reset(new uint8_t[32]);
    canonical_scalar(o.seed.get());
  }
  if (opt & 16) {
    o.state.reset(new uint8_t[203]);
    fill(o.state.get(), 203);
    o.state[200] = 5;
  } else if (!(opt & 32)) {
    o.label_len = 1 + rng() % 19;
    o.label.reset(new uint8_t[o.label_len]);
    fill(o.label.get(), o.label_len);
  }
  const bool valid_m = m && !(m & (m - 1)) && m <= P.m_max;
  o.ext_len = 32 * (size_t)((valid_m ? rounds_of(P, m) : 6) + 3) + ((opt & 64) ? 40 : 0);
  o.ext.reset(new uint8_t[o.ext_len]);
  fill(o.ext.get(), o.ext_len);
  return o;
}

// the copy of item k equals its source, field by field, and shares no address with it
bool equal_item(const ParamShape &P, const bpp_prove_item &a, const bpp_prove_item &b) {
  const size_t m = a.m, need = 32 * (size_t)(rounds_of(P, a.m) + 3);
  auto eq = [](const void *x, const void *y, size_t n, bool &ok) {
    if ((x == nullptr) != (y == nullptr)) ok = false;
    else if (x && (x == y || memcmp(x, y, n) != 0)) ok = false;
  };
  bool ok = a.m == b.m && b.rng_len == need;
  eq(a.values, b.values, 8 * m, ok);
  eq(a.blindings32, b.blindings32, 32 * m * P.t, ok);
  eq(a.commitments32, b.commitments32, 32 * m, ok);
  eq(a.min_values, b.min_values, 8 * m, ok);
  eq(a.min_present, b.min_present, m, ok);
  eq(a.seed_nonce32, b.seed_nonce32, 32, ok);
  eq(a.transcript_state, b.transcript_state, 203, ok);
  if (!a.transcript_state) {
    eq(a.transcript_label, b.transcript_label, a.label_len, ok);
    ok = ok && (!a.transcript_label || a.label_len == b.label_len);
  }
  eq(a.rng_bytes, b.rng_bytes, need, ok);
  return ok;
}

// what the packer laid down for item i equals its source, field by field (offsets into pk.bytes as a whole)
bool packed_item(const ParamShape &P, const ProvePack &pk, size_t i, const bpp_prove_item &it) {
  const ProveDesc &d = pk.desc[i];
  const size_t t = P.t, m = it.m, ext = 32 * (size_t)(rounds_of(P, it.m) + 3);
  bool ok = d.m == it.m && d.mslot == pk.m && d.roff == pk.rounds - rounds_of(P, it.m) && pk.roff[i] == d.roff && d.minval_idx == i * pk.m;
  ok = ok && d.commit_off == d.wit_off + m * (8 + 32 * t) && d.ext_off == d.commit_off + 32 * m && d.seed_off == d.ext_off + ext &&
       d.seed_off + 32 == (i + 1 < pk.desc.size() ? pk.desc[i + 1].wit_off : pk.bytes.size());
  ok = ok && d.flags == ((it.seed_nonce32 ? 1u : 0u) | (it.commitments32 ? 0u : PV_FLAG_MAKE_COMMITMENTS));
  if (!ok) return false;
  const uint8_t *b = pk.bytes.data();
  for (size_t j = 0; j < m; j++) {
    uint64_t v = 0;
    for (int k = 7; k >= 0; k--) v = (v << 8) | b[d.wit_off + j * (8 + 32 * t) + k];
    ok = ok && v == it.values[j] && memcmp(b + d.wit_off + j * (8 + 32 * t) + 8, it.blindings32 + 32 * t * j, 32 * t) == 0;
    const bool present = it.min_present && it.min_present[j];
    ok = ok && pk.minpres[i * pk.m + j] == (present ? 1 : 0) && pk.minvals[i * pk.m + j] == (present ? it.min_values[j] : 0);
  }
  const std::vector<uint8_t> zeros(32 * m + 32, 0);
  ok = ok && memcmp(b + d.commit_off, it.commitments32 ? it.commitments32 : zeros.data(), 32 * m) == 0;
  ok = ok && memcmp(b + d.ext_off, it.rng_bytes, ext) == 0;
  ok = ok && memcmp(b + d.seed_off, it.seed_nonce32 ? it.seed_nonce32 : zeros.data(), 32) == 0;
  return ok;
}

// the seven call-level appends on top of `st` (a label's Transcript::new, or the caller's state)
void call_appends(Strobe &st, const ParamShape &P, const uint8_t *hg32, uint32_t m) {
  merlin_append_message(st, (const uint8_t *)"dom-sep", 7, (const uint8_t *)"Bulletproofs+ Range Proof", 25);
  merlin_append_message(st, (const uint8_t *)"H", 1, hg32, 32);
  for (uint32_t k = 0; k < P.t; k++) merlin_append_message(st, (const uint8_t *)"G", 1, hg32 + 32 * (k + 1), 32);
  merlin_append_u64(st, (const uint8_t *)"N", 1, P.n_bits);
  merlin_append_u64(st, (const uint8_t *)"T", 1, P.t);
  merlin_append_u64(st, (const uint8_t *)"M", 1, m);
}
bool state_is(const ProvePack &pk, size_t i, const ParamShape &P, const uint8_t *hg32, const bpp_prove_item &it) {
  Strobe st;
  if (it.transcript_state) strobe_from_bytes(st, it.transcript_state);
  else merlin_new(st, it.transcript_label, (uint32_t)(it.transcript_label ? it.label_len : 0));
  call_appends(st, P, hg32, it.m);
  uint8_t want[203];
  strobe_to_bytes(want, st);
  return (size_t)pk.desc[i].state_idx * 203 + 203 <= pk.states.size() && memcmp(&pk.states[(size_t)pk.desc[i].state_idx * 203], want, 203) == 0;
}

int pack_code(const ParamShape &P, const uint8_t *hg32, const std::vector<bpp_prove_item> &v, bool mixed, bool openings, std::string *msg = nullptr) {
  ProvePack pk;
  try {
    pk.pack(P, hg32, v.data(), v.size(), mixed, openings);
  } catch (const ProofErr &e) {
    if (msg) *msg = e.msg;
    return e.code;
  }
  return BPP_OK;
}

int fails = 0;
#define EXPECT(name, cond)                           \
  do {                                               \
    if (cond) {                                      \
      printf("ok %s\n", name);                       \
    } else {                                         \
      printf("FAIL %s (line %d)\n", name, __LINE__); \
      fails++;                                       \
    }                                                \
  } while (0)

}  // namespace

int main() {
  const ParamShape P{64, 4, 3}, P8{8, 4, 1};
  {  // every optional field NULL or present, in every combination, as mixed-call items and as openings items
    bool all_ok = true;
    for (int openings = 0; openings < 2; openings++) {
      std::vector<Owned> own;
      for (unsigned opt = 0; opt < 128; opt++) own.push_back(make(P, 1u << (opt % 3), opt));
      std::vector<bpp_prove_item> v;
      for (auto &o : own) v.push_back(o.view());
      ProveJobCopy c;
      c.take(P, v.data(), v.size(), 4096, openings != 0, 128);
      size_t k = 0;
      for (size_t i = 0; i < v.size(); i++) {
        const bool want_ok = openings || v[i].commitments32;  // (an item without commitments passes as an openings item only)
        if ((c.code[i] == BPP_OK) != want_ok) all_ok = false;
        if (c.code[i] != BPP_OK) continue;
        if (k >= c.items.size() || c.index[k] != i || !equal_item(P, v[i], c.items[k])) all_ok = false;
        k++;
      }
      all_ok = all_ok && k == c.items.size();
    }
    EXPECT("optional_fields", all_ok);
  }
  {  // items that fail the check beside items that pass: none of the failing ones is looked at beyond what the check reads
    std::vector<Owned> own;
    own.push_back(make(P8, 1, 1 | 8));
    own.push_back(make(P8, 0, 1));  // m = 0
    own.push_back(make(P8, 2, 1 | 2 | 4));
    own.push_back(make(P8, 3, 1));  // m = 3
    own.push_back(make(P8, 8, 1));  // m above m_max
    own.push_back(make(P8, 4, 1));
    own.push_back(make(P8, 2, 1));  // values == NULL below
    own.push_back(make(P8, 4, 1));  // one draw short below
    own.push_back(make(P8, 1, 1));
    std::vector<bpp_prove_item> v;
    for (auto &o : own) v.push_back(o.view());
    v[1].values = nullptr;  // (an m of 0 or 3 says nothing about how much lies behind the pointers: poison them)
    v[1].blindings32 = (const uint8_t *)8;
    v[3].blindings32 = (const uint8_t *)8;
    v[3].rng_bytes = (const uint8_t *)8;
    v[4].values = (const uint64_t *)8;
    v[4].blindings32 = (const uint8_t *)8;
    v[6].values = nullptr;
    {  // exactly one draw short, in an exact-size buffer
      own[7].ext_len -= 32;
      std::unique_ptr<uint8_t[]> cut(new uint8_t[own[7].ext_len]);
      memcpy(cut.get(), own[7].ext.get(), own[7].ext_len);
      own[7].ext = std::move(cut);
      v[7] = own[7].view();
    }
    ProveJobCopy c;
    c.take(P8, v.data(), v.size(), 4096, false, 0);
    const int want[9] = {BPP_OK, BPP_ERR_INVALID_ARGUMENT, BPP_OK, BPP_ERR_INVALID_ARGUMENT, BPP_ERR_INVALID_ARGUMENT, BPP_OK,
                         BPP_ERR_INVALID_ARGUMENT, BPP_ERR_INVALID_LENGTH, BPP_OK};
    bool ok = c.items.size() == 4 && c.index == std::vector<uint32_t>{0, 2, 5, 8};
    for (size_t i = 0; i < 9; i++) ok = ok && c.code[i] == want[i] && (c.code[i] == BPP_OK) == c.msg[i].empty();
    ok = ok && c.msg[1] == "Number of commitments must be a power of two" && c.msg[4] == "Not enough generators for this statement" &&
         c.msg[6] == "null witness / statement field" && c.msg[7] == "not enough external randomness: need (rounds + 3) * 32 bytes";
    ok = ok && c.len[1] == 0 && c.len[3] == 0 && c.len[4] == 0 && c.len[0] == 1 + 32 * (size_t)(1 + 5 + 2 * 3) &&
         c.len[7] == 1 + 32 * (size_t)(1 + 5 + 2 * 5);
    for (size_t k = 0; ok && k < c.items.size(); k++) ok = equal_item(P8, v[c.index[k]], c.items[k]);
    // the blocking calls' own findings come out of the same routine: a stride too short, in the order of the checks
    ProveJobCopy d;
    d.take(P8, v.data(), 1, 10, true, 0);
    ok = ok && d.code[0] == BPP_ERR_INVALID_LENGTH && d.msg[0] == "proof_stride too small" && d.items.empty();
    d.take(P8, v.data(), 1, 4096, true, 31);
    ok = ok && d.code[0] == BPP_ERR_INVALID_LENGTH && d.msg[0] == "commit_stride too small";
    EXPECT("failing_items_beside_passing", ok);
  }
  {  // the copy equals the source byte for byte; the source is overwritten (and freed) and the copy does not change
    std::vector<Owned> own;
    own.push_back(make(P, 1, 1 | 2 | 4 | 8 | 64));
    own.push_back(make(P, 4, 1 | 16));
    own.push_back(make(P, 2, 2));
    std::vector<bpp_prove_item> v;
    for (auto &o : own) v.push_back(o.view());
    // two items on ONE label buffer: the copy keeps one source for both
    v.push_back(v[2]);
    ProveJobCopy c;
    c.take(P, v.data(), v.size(), 4096, true, 128);
    bool ok = c.items.size() == 4;
    for (size_t k = 0; ok && k < 4; k++) ok = equal_item(P, v[k], c.items[k]);
    ok = ok && c.items[3].transcript_label == c.items[2].transcript_label && c.items[3].values != c.items[2].values;
    const std::vector<uint64_t> before = c.store;
    const std::vector<bpp_prove_item> items_before = c.items;
    for (auto &o : own) {
      const size_t mm = o.m;
      memset(o.values.get(), 0xA5, 8 * mm);
      memset(o.blind.get(), 0xA5, 32 * mm * o.t);
      if (o.commits) memset(o.commits.get(), 0xA5, 32 * mm);
      if (o.minv) memset(o.minv.get(), 0xA5, 8 * mm);
      if (o.present) memset(o.present.get(), 0xA5, mm);
      if (o.seed) memset(o.seed.get(), 0xA5, 32);
      if (o.state) memset(o.state.get(), 0xA5, 203);
      if (o.label) memset(o.label.get(), 0xA5, o.label_len);
      memset(o.ext.get(), 0xA5, o.ext_len);
    }
    memset(v.data(), 0xA5, v.size() * sizeof(bpp_prove_item));
    own.clear();  // (freed: a copy that still pointed there would be a use after free below)
    ok = ok && c.store == before && memcmp(c.items.data(), items_before.data(), 4 * sizeof(bpp_prove_item)) == 0;
    uint64_t sum = 0;
    for (const bpp_prove_item &it : c.items) {  // every byte the prover would read is the copy's own
      for (uint32_t j = 0; j < it.m; j++) sum += it.values[j];
      for (size_t q = 0; q < 32 * (size_t)it.m * P.t; q++) sum += it.blindings32[q];
      for (size_t q = 0; q < it.rng_len; q++) sum += it.rng_bytes[q];
      if (it.transcript_label)
        for (size_t q = 0; q < it.label_len; q++) sum += it.transcript_label[q];
    }
    EXPECT("copy_survives_the_source", ok && sum != 0);
  }
  {  // after the wipe every byte of the copy reads zero, before it is freed; the outcomes stay
    std::vector<Owned> own;
    for (unsigned k = 0; k < 12; k++) own.push_back(make(P, 1u << (k % 3), 1 | 2 | 4 | 8 | (k & 1 ? 16 : 0)));
    own.push_back(make(P, 3, 1));
    std::vector<bpp_prove_item> v;
    for (auto &o : own) v.push_back(o.view());
    ProveJobCopy c;
    c.take(P, v.data(), v.size(), 4096, false, 0);
    bool ok = c.items.size() == 12 && c.store_bytes > 12 * (8 + 96 + 32 * 9);
    size_t nonzero = 0;
    for (size_t i = 0; i < c.store_bytes; i++) nonzero += c.bytes()[i] != 0;
    ok = ok && nonzero > c.store_bytes / 2;
    c.wipe();
    for (size_t i = 0; i < c.store.size() * sizeof(uint64_t); i++) ok = ok && c.bytes()[i] == 0;
    for (const bpp_prove_item &it : c.items) ok = ok && it.values == nullptr && it.rng_bytes == nullptr && it.m == 0;
    ok = ok && c.code[12] == BPP_ERR_INVALID_ARGUMENT && c.code[0] == BPP_OK && c.len[0] != 0 && c.m[2] == 4;
    EXPECT("wiped_before_freed", ok);
  }
  std::unique_ptr<uint8_t[]> hg(new uint8_t[32 * 4]);  // H and three G bases, exact size for P
  fill(hg.get(), 32 * 4);
  {  // a uniform and a mixed call, every optional field in some item: descriptors, bytes, minimum-value rows
    bool ok = true;
    for (int mixed = 0; mixed < 2; mixed++) {
      const uint32_t ms[2][6] = {{2, 2, 2, 2, 2, 2}, {4, 4, 2, 2, 1, 1}};
      std::vector<Owned> own;
      for (unsigned k = 0; k < 6; k++) own.push_back(make(P, ms[mixed][k], 1 | (k & 1 ? 2 | 4 : 0) | (k & 2 ? 2 : 0) | 8 | (k == 3 ? 64 : 0)));
      std::vector<bpp_prove_item> v;
      for (auto &o : own) v.push_back(o.view());
      ProvePack pk;
      pk.pack(P, hg.get(), v.data(), v.size(), mixed != 0, false);
      ok = ok && pk.m == ms[mixed][0] && pk.rounds == rounds_of(P, pk.m) && pk.rounds_min == rounds_of(P, ms[mixed][5]) &&
           pk.plen == prove_item_len_host(P, pk.m) && pk.desc.size() == 6 && pk.desc[0].wit_off == 0;
      for (size_t i = 0; ok && i < 6; i++) ok = packed_item(P, pk, i, v[i]) && state_is(pk, i, P, hg.get(), v[i]);
    }
    EXPECT("pack_uniform_and_mixed", ok);
  }
  {  // openings items with and without commitments; without the openings flag the item that brings none is refused, unread
    std::vector<Owned> own;
    own.push_back(make(P, 2, 1));
    own.push_back(make(P, 2, 0));
    own.push_back(make(P, 1, 8));
    own.push_back(make(P, 1, 1 | 8));
    std::vector<bpp_prove_item> v;
    for (auto &o : own) v.push_back(o.view());
    ProvePack pk;
    pk.pack(P, hg.get(), v.data(), v.size(), true, true);
    bool ok = pk.desc[0].flags == 0 && pk.desc[1].flags == PV_FLAG_MAKE_COMMITMENTS && pk.desc[2].flags == (1u | PV_FLAG_MAKE_COMMITMENTS) &&
              pk.desc[3].flags == 1u;
    for (size_t i = 0; ok && i < 4; i++) ok = packed_item(P, pk, i, v[i]);
    std::string msg;
    v[1].values = (const uint64_t *)8;
    v[1].blindings32 = v[1].rng_bytes = (const uint8_t *)8;
    ok = ok && pack_code(P, hg.get(), v, true, false, &msg) == BPP_ERR_INVALID_ARGUMENT && msg == "null witness / statement field";
    EXPECT("pack_openings", ok);
  }
  {  // labels and states, shared and distinct: one state per distinct (source bytes, m), each after the seven appends
    std::vector<Owned> own;
    own.push_back(make(P, 2, 1));       // a label
    own.push_back(make(P, 2, 1 | 16));  // a state
    own.push_back(make(P, 2, 1 | 32));  // no label at all
    own.push_back(make(P, 1, 1 | 16));
    std::vector<bpp_prove_item> v = {own[0].view(), own[0].view(), own[1].view(), own[2].view(), own[0].view(), own[3].view(), own[3].view()};
    v[1].values = own[1].values.get();  // (another witness on the SAME label buffer)
    v[4] = own[3].view();               // m = 1 items: the first label's bytes at ANOTHER address and under another m, a state twice
    v[4].transcript_state = nullptr;
    std::unique_ptr<uint8_t[]> label2(new uint8_t[own[0].label_len]);
    memcpy(label2.get(), own[0].label.get(), own[0].label_len);
    v[4].transcript_label = label2.get();
    v[4].label_len = own[0].label_len;
    std::unique_ptr<uint8_t[]> state2(new uint8_t[203]);
    memcpy(state2.get(), own[3].state.get(), 203);
    v[6].transcript_state = state2.get();
    ProvePack pk;
    pk.pack(P, hg.get(), v.data(), v.size(), true, false);
    const uint32_t want[7] = {0, 0, 1, 2, 3, 4, 4};
    bool ok = pk.states.size() == 5 * 203;
    for (size_t i = 0; i < 7; i++) ok = ok && pk.desc[i].state_idx == want[i] && state_is(pk, i, P, hg.get(), v[i]);
    EXPECT("pack_transcripts", ok);
  }
  {  // a failing item at every position of the check and of the call: the finding is the check's, and nothing behind a refused
     // pointer -- the failing item's or a later item's -- is read
    struct Bad {
      int code;
      const char *msg;
    };
    const Bad want[12] = {{BPP_ERR_INVALID_ARGUMENT, "Number of commitments must be a power of two"},
                          {BPP_ERR_INVALID_ARGUMENT, "Number of commitments must be a power of two"},
                          {BPP_ERR_INVALID_ARGUMENT, "Not enough generators for this statement"},
                          {BPP_ERR_INVALID_ARGUMENT, "null witness / statement field"},
                          {BPP_ERR_INVALID_ARGUMENT, "Mask recovery is not supported with an aggregated statement"},
                          {BPP_ERR_INVALID_LENGTH, "not enough external randomness: need (rounds + 3) * 32 bytes"},
                          {BPP_ERR_INVALID_LENGTH, "Value exceeds bit vector capacity!"},
                          {BPP_ERR_INVALID_ARGUMENT, "Minimum value is larger than value"},
                          {BPP_ERR_INVALID_ARGUMENT, "blinding factor is not canonical"},
                          {BPP_ERR_INVALID_ARGUMENT, "seed nonce is not canonical"},
                          {BPP_ERR_INVALID_ARGUMENT, "transcript state has pos >= rate"},
                          {BPP_ERR_INVALID_ARGUMENT, "all items of one prove batch must share the aggregation factor"}};
    bool ok = true;
    for (int kind = 0; kind < 12; kind++)
      for (size_t pos = 0; pos < 3; pos++) {
        if (kind == 11 && pos == 0) continue;  // (the call's m IS the first item's)
        const bool m1 = kind == 9;             // (a seed nonce needs m = 1)
        std::vector<Owned> own;
        for (size_t k = 0; k < 3; k++) own.push_back(make(P8, m1 ? 1 : 2, 1 | 2 | 4 | (k == pos && kind == 10 ? 16 : 0) | (m1 ? 8 : 0)));
        Owned &o = own[pos];
        std::vector<bpp_prove_item> v;
        for (auto &x : own) v.push_back(x.view());
        bpp_prove_item &b = v[pos];
        if (kind <= 2 || kind == 11) {  // an m that says nothing about what lies behind the pointers
          b.m = kind == 0 ? 0 : kind == 1 ? 3 : kind == 2 ? 8 : 4;
          b.values = (const uint64_t *)8;
          b.blindings32 = b.commitments32 = b.rng_bytes = (const uint8_t *)8;
        } else if (kind == 3) {
          b.rng_bytes = nullptr;
          b.values = (const uint64_t *)8;
        } else if (kind == 4) {
          o.seed.reset(new uint8_t[32]);
          canonical_scalar(o.seed.get());
          b.seed_nonce32 = o.seed.get();
          b.values = (const uint64_t *)8;
        } else if (kind == 5) {
          b.rng_len -= 1;
          b.values = (const uint64_t *)8;
        } else if (kind == 6) {
          o.values[1] = 256;
          b.blindings32 = (const uint8_t *)8;
        } else if (kind == 7) {
          o.values[0] = 3;  // (its promise is 7 and present)
          b.blindings32 = (const uint8_t *)8;
        } else if (kind == 8) {
          memset(o.blind.get() + 32, 0xff, 32);
        } else if (kind == 9) {
          memset(o.seed.get(), 0xff, 32);
        } else if (kind == 10) {
          o.state[200] = BPP_STROBE_R;
        }
        for (size_t k = pos + 1; k < 3; k++) {  // whatever comes after the finding is never looked at
          v[k].values = (const uint64_t *)8;
          v[k].blindings32 = v[k].commitments32 = v[k].rng_bytes = (const uint8_t *)8;
        }
        std::string msg;
        const int code = pack_code(P8, hg.get(), v, false, false, &msg);
        // (an m of another kind behind the first item meets the call's own rule first, as it always did)
        const Bad &w = kind <= 2 && pos > 0 ? want[11] : want[kind];
        if (code != w.code || msg != w.msg) {
          printf("  kind %d at %zu: %d %s\n", kind, pos, code, msg.c_str());
          ok = false;
        }
      }
    // the mixed call's own rule, in front of the check: an item larger than the one before it
    std::vector<Owned> own;
    own.push_back(make(P8, 2, 1));
    own.push_back(make(P8, 4, 1));
    std::vector<bpp_prove_item> v = {own[0].view(), own[1].view()};
    v[1].values = (const uint64_t *)8;
    std::string msg;
    ok = ok && pack_code(P8, hg.get(), v, true, false, &msg) == BPP_ERR_INVALID_ARGUMENT &&
         msg == "mixed prove batch: items must be sorted by aggregation factor";
    EXPECT("pack_failing_item_at_every_position", ok);
  }
  {  // every packed byte reads zero after wipe(), and after the destructor (read where the freed block still lies, which the
     // sanitizer keeps out of circulation: the destructor wipes BEFORE the vector gives its memory back)
    std::vector<Owned> own;
    for (unsigned k = 0; k < 8; k++) own.push_back(make(P, 2, 1 | 8));
    std::vector<bpp_prove_item> v;
    for (auto &o : own) v.push_back(o.view());
    bool ok = true;
    for (int how = 0; how < 2; how++) {
      std::unique_ptr<ProvePack> pk(new ProvePack);
      pk->pack(P, hg.get(), v.data(), v.size(), false, false);
      const uint8_t *p = pk->bytes.data();
      const size_t len = pk->bytes.size();
      size_t nonzero = 0;
      for (size_t i = 0; i < len; i++) nonzero += p[i] != 0;
      ok = ok && len == 8 * (2 * (8 + 96) + 64 + 32 * (rounds_of(P, 2) + 3) + 32) && nonzero > len / 2;
      if (how == 0) {
        pk->wipe();
      } else {
        pk.reset();
        ASAN_UNPOISON_MEMORY_REGION(p, len);
      }
      // (the sanitizer's allocator keeps a note of its own in the first 16 bytes of a block it has taken back)
      for (size_t i = how ? 16 : 0; i < len; i++) ok = ok && p[i] == 0;
      if (how == 1) ASAN_POISON_MEMORY_REGION(p, len);
    }
    // a call that fails half way leaves nothing either: the items packed before the finding are wiped with the rest
    v[5].rng_bytes = nullptr;
    ok = ok && pack_code(P, hg.get(), v, false, false) == BPP_ERR_INVALID_ARGUMENT;
    EXPECT("pack_wiped_by_wipe_and_by_the_destructor", ok);
  }
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
