// Sanitizer harness (CPU test suite only): the job copy bpp_prove_submit takes of its caller's items (prove_job_host.h: the
// per-item check, the deep copy, the wipe), built with  g++ -fsanitize=address,undefined  into an executable that
// tests/test_prove_pipeline_host.py runs.  Everything an item points to is an exact-size heap allocation, so a read past what the
// item declares, or a look behind the pointer of an item that fails the check, is an ASan report (exit code != 0).  Prints one
// "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>

#include "prove_job_host.h"

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
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
