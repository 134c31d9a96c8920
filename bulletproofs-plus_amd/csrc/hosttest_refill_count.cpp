// Sanitizer harness (CPU test suite only): a refill with a LIVE COUNT (bpp_batch_refill_enqueue_count).
//
// 1. The one-lane host model of the refill kernels (refill.h: refill_run_host with Refill::count) is held to what a fresh
//    device upload makes of the FIRST c ITEMS of the same arrays -- ingest_run_host + ingest_finish_plan of ingest.h -- over the
//    corpus of hosttest_refill.cpp's kinds (edge scalars in every field, two findings, foreign first bytes, nonces at m = 1 and
//    m = 2, promises at the capacity, a foreign degree, random mutations), for c in {0, 1, N - 1, N, N + 1}, the findings lying on
//    both sides of c:
//      record and state   what the upload of the first c items throws, FALLBACK for a foreign first byte below c, clean otherwise;
//                         c = N + 1: BPP_REFILL_COUNT alone, before either
//      live slots         as hosttest_refill.cpp holds them: the upload's bytes, or the sanitised slot of a stopped item
//      dead slots         byte for byte the sanitised slot: t0 and zeros, zero commitments, no promise, no nonce, no flag, the
//                         shape's degree bit, cleared status words, wiped mask rows
//      dead sources       are never read: the harness hands the model arrays whose items at and beyond c hold a poison pattern
//                         (and, for c < N, arrays that END behind item c - 1, so that a read is an ASan report), and searches
//                         everything the refill wrote for the pattern
//      the live word      min(c, N), 0 for c > N
// 2. The two live routines of verdict.h plus verdict_finish are held to check_deferred + check_chunk_errors (upload_host.h) on the
//    CUT batch, for groups cut in the middle, cut exactly at a boundary, and empty.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_refill_count_host.py runs.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "refill.h"

using namespace bpp;

static_assert(BPP_VERDICT_EMPTY != BPP_VERDICT_WRITTEN && BPP_VERDICT_EMPTY != BPP_VERDICT_REDRAW && BPP_VERDICT_EMPTY != BPP_VERDICT_REFILL, "verdict flags");
static_assert(BPP_REFILL_COUNT != BPP_REFILL_WRITTEN && BPP_REFILL_COUNT != BPP_REFILL_FINDING && BPP_REFILL_COUNT != BPP_REFILL_FALLBACK, "refill flags");

namespace {

std::mt19937_64 rng(20261021);
const uint8_t POISON[8] = {0xa7, 0x5c, 0x3e, 0x91, 0xd2, 0x4b, 0x68, 0xf3};

void canonical_scalar(uint8_t *p) {
  for (int i = 0; i < 32; i++) p[i] = (uint8_t)rng();
  p[31] &= 0x0f;  // < 2^252 < l
}
// wire bytes with the structure of a proof: [t] d1[t] A A1 B r1 s1 (L R)*rounds
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

// a caller's batch as plain vectors
struct Source {
  size_t n = 0, len = 0, stride = 0;
  uint32_t m = 1;
  std::vector<std::vector<uint8_t>> items;
  std::vector<uint8_t> commits, present, seeds, seed_present;
  std::vector<uint64_t> minv;
  bool has_promises = false, has_seeds = false, has_seed_present = false;

  Source(const std::vector<std::vector<uint8_t>> &it, uint32_t m_, size_t extra_stride = 0) : n(it.size()), m(m_), items(it) {
    len = items[0].size();
    stride = len + extra_stride;
    commits.resize(32 * n * m);
    for (auto &x : commits) x = (uint8_t)rng();
  }
  void promises(const std::vector<uint64_t> &v, const std::vector<uint8_t> &p) {
    has_promises = true;
    minv.resize(n * m);
    present.resize(n * m);
    for (size_t q = 0; q < n * m; q++) {
      minv[q] = v[q % v.size()];
      present[q] = p[q % p.size()];
    }
  }
  void nonces(const std::vector<uint8_t> *which) {  // null: every item has one
    has_seeds = true;
    seeds.resize(32 * n);
    for (auto &x : seeds) x = (uint8_t)(rng() | 1);
    if (which) {
      has_seed_present = true;
      seed_present.resize(n);
      for (size_t i = 0; i < n; i++) seed_present[i] = (*which)[i % which->size()];
    }
  }
};

// exact-size heap copies of the first `keep` items of a source, described as a packed batch of `claim` items: keep == claim is an
// ordinary batch; keep < claim is what a refill with count = keep is handed (the arrays END behind the last live item), keep ==
// claim with poison_from < claim overwrites the items from there on with the poison pattern
struct Arrays {
  std::unique_ptr<uint8_t[]> proofs, commits, present, seeds, seed_present;
  std::unique_ptr<uint64_t[]> minv;
  bpp_packed_batch pk;

  static void poison(uint8_t *p, size_t k) {
    for (size_t i = 0; i < k; i++) p[i] = POISON[i % 8];
  }
  Arrays(const Source &s, size_t keep, size_t claim, size_t poison_from) {
    const size_t n = keep, m = s.m;
    const size_t extent = n ? (n - 1) * s.stride + s.len : 0;
    proofs.reset(new uint8_t[extent ? extent : 1]);
    memset(proofs.get(), 0xee, extent);
    for (size_t i = 0; i < n; i++) {
      if (i >= poison_from) poison(proofs.get() + i * s.stride, s.len);
      else memcpy(proofs.get() + i * s.stride, s.items[i].data(), s.len);
    }
    commits.reset(new uint8_t[32 * n * m + 1]);
    memcpy(commits.get(), s.commits.data(), 32 * n * m);
    if (poison_from < n) poison(commits.get() + 32 * poison_from * m, 32 * (n - poison_from) * m);
    memset(&pk, 0, sizeof(pk));
    pk.n_items = claim;
    pk.proofs = proofs.get();
    pk.proof_len = s.len;
    pk.proof_stride = s.stride;
    pk.commitments32 = commits.get();
    pk.m = s.m;
    if (s.has_promises) {
      minv.reset(new uint64_t[n * m + 1]);
      present.reset(new uint8_t[n * m + 1]);
      memcpy(minv.get(), s.minv.data(), 8 * n * m);
      memcpy(present.get(), s.present.data(), n * m);
      if (poison_from < n) {
        poison((uint8_t *)(minv.get() + poison_from * m), 8 * (n - poison_from) * m);
        poison(present.get() + poison_from * m, (n - poison_from) * m);
      }
      pk.min_values = minv.get();
      pk.min_present = present.get();
    }
    if (s.has_seeds) {
      seeds.reset(new uint8_t[32 * n + 1]);
      memcpy(seeds.get(), s.seeds.data(), 32 * n);
      if (poison_from < n) poison(seeds.get() + 32 * poison_from, 32 * (n - poison_from));
      pk.seed_nonces32 = seeds.get();
      if (s.has_seed_present) {
        seed_present.reset(new uint8_t[n + 1]);
        memcpy(seed_present.get(), s.seed_present.data(), n);
        if (poison_from < n) poison(seed_present.get() + poison_from, n - poison_from);
        pk.seed_present = seed_present.get();
      }
    }
  }
};

// what the engine holds of a resident batch of N items of pk's shape: exact sizes, every byte a refill must write starts as `fill`
struct ModelBatch {
  size_t n, len, bytes_total;
  uint32_t m, t;
  std::unique_ptr<uint8_t[]> bytes, seeds, defer;
  std::unique_ptr<uint64_t[]> minvals;
  std::unique_ptr<ProofDesc[]> desc;
  std::unique_ptr<uint32_t[]> status0, status, masks;
  uint32_t red[BPP_REFILL_RED_WORDS] = {0, 0};
  uint64_t state = ~0ull;
  uint32_t live = 0xdddddddd;
  bpp_device_refill record;

  ModelBatch(size_t n_, const bpp_packed_batch &pk, const ParamShape &P, uint8_t fill)
      : n(n_), len(pk.proof_len), bytes_total(n * len + n * (size_t)pk.m * 32), m(pk.m), t(P.t) {
    bytes.reset(new uint8_t[bytes_total + BPP_BYTES_SLACK]);
    memset(bytes.get(), fill, bytes_total);
    memset(bytes.get() + bytes_total, 0, BPP_BYTES_SLACK);
    seeds.reset(new uint8_t[32 * n + 1]);
    memset(seeds.get(), fill, 32 * n + 1);
    defer.reset(new uint8_t[n + 1]);
    memset(defer.get(), fill, n + 1);
    minvals.reset(new uint64_t[n * m + 1]);
    memset(minvals.get(), fill, (n * m + 1) * 8);
    desc.reset(new ProofDesc[n + 1]);
    memset(desc.get(), fill, (n + 1) * sizeof(ProofDesc));
    status0.reset(new uint32_t[n + 1]);
    status.reset(new uint32_t[n + 1]);
    memset(status0.get(), fill, (n + 1) * 4);
    memset(status.get(), fill, (n + 1) * 4);
    masks.reset(new uint32_t[n * (size_t)t * 8 + 1]);
    memset(masks.get(), fill, (n * (size_t)t * 8 + 1) * 4);
    memset(&record, fill, sizeof(record));
  }
  void refill(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0, const uint32_t *count) {
    const Refill r = refill_args(pk, P, t0, bytes.get(), minvals.get(), seeds.get(), defer.get(), desc.get(),
                                       status0.get(), status.get(), masks.get(), red, count);
    refill_run_host<false>(r, &state, &record, &live);
  }
};

int fails = 0, checked = 0;
const char *why = "";

bool all_zero(const uint8_t *p, size_t k) {
  for (size_t i = 0; i < k; i++)
    if (p[i]) return false;
  return true;
}
// eight consecutive bytes of the poison pattern, at any phase
bool has_poison(const uint8_t *p, size_t k) {
  for (size_t i = 0; i + 8 <= k; i++)
    for (int ph = 0; ph < 8; ph++) {
      int q = 0;
      while (q < 8 && p[i + q] == POISON[(ph + q) % 8]) q++;
      if (q == 8) return true;
    }
  return false;
}

// the sanitised slot of item i, byte for byte
bool slot_is_sanitised(const ModelBatch &mb, size_t i, uint8_t t0, uint8_t degree, bool nonces) {
  const uint8_t *slot = mb.bytes.get() + i * mb.len, *cm = mb.bytes.get() + mb.n * mb.len + 32 * i * mb.m;
  if (slot[0] != t0 || !all_zero(slot + 1, mb.len - 1)) return why = "a slot is not t0 and zeros", false;
  if (!all_zero(cm, 32 * (size_t)mb.m)) return why = "commitments are not zero", false;
  for (uint32_t j = 0; j < mb.m; j++)
    if (mb.minvals[i * mb.m + j]) return why = "a promise is kept", false;
  if (nonces && !all_zero(mb.seeds.get() + 32 * i, 32)) return why = "a nonce is kept", false;
  if (mb.desc[i].flags) return why = "a flag is kept", false;
  if (mb.defer[i] != degree) return why = "defer is not the shape's degree bit alone", false;
  return true;
}

// one refill with count c of a model batch of src's shape, held to the fresh device upload of the first min(c, N) items
bool hold_count(const Source &src, const ParamShape &P, uint8_t t0, uint32_t c, bool shape_exists) {
  checked++;
  const size_t N = src.n, len = src.len;
  const uint32_t m = src.m;
  const bool bad_count = c > N;
  const size_t live = bad_count ? 0 : c;
  // what the model is handed: the arrays end behind the last live item (a bad count: no item at all may be read); a second run
  // takes full-length arrays whose dead items hold the poison pattern -- both must leave the same bytes
  const Arrays cut(src, live, N, live), poisoned(src, N, N, live);
  ModelBatch mb(N, cut.pk, P, 0xcd), mp(N, poisoned.pk, P, 0x37);
  mb.refill(cut.pk, P, t0, &c);
  mp.refill(poisoned.pk, P, t0, &c);
  const uint8_t degree = t0 != P.t ? BPP_DEFER_DEGREE : 0;
  const bool nonces = src.has_seeds;
  if (mb.live != live || mp.live != live) return why = "the live word is not the clamped count", false;
  if (memcmp(mb.bytes.get(), mp.bytes.get(), mb.bytes_total + BPP_BYTES_SLACK) || memcmp(mb.minvals.get(), mp.minvals.get(), N * m * 8) ||
      (nonces && memcmp(mb.seeds.get(), mp.seeds.get(), 32 * N)) || memcmp(mb.defer.get(), mp.defer.get(), N) ||
      memcmp(&mb.record, &mp.record, sizeof(mb.record)) || mb.state != mp.state)
    return why = "the outputs depend on the dead items' sources or on the old contents", false;
  if (has_poison(mp.bytes.get(), mp.bytes_total) || has_poison((const uint8_t *)mp.minvals.get(), N * m * 8) || (nonces && has_poison(mp.seeds.get(), 32 * N)))
    return why = "bytes of a dead item's source appear in the batch", false;
  for (size_t i = 0; i < N; i++)
    if (mp.desc[i].flags > 1) return why = "a dead item's source reached the flags", false;
  // (guard bytes behind every array: nothing is written past item N - 1)
  if (mb.defer[N] != 0xcd || mb.status[N] != 0xcdcdcdcdu || mb.status0[N] != 0xcdcdcdcdu || mb.masks[N * (size_t)mb.t * 8] != 0xcdcdcdcdu ||
      mb.minvals[N * m] != 0xcdcdcdcdcdcdcdcdull || mb.seeds[32 * N] != 0xcd)
    return why = "a write past the batch's last item", false;
  if (mb.red[0] || mb.red[1]) return why = "the reduction words are not left clear", false;
  const bpp_device_refill &rec = mb.record;
  if (mb.state != refill_state_make(rec.flags, rec.code, rec.msg, rec.index)) return why = "state word is not the record's", false;
  for (size_t i = 0; i < N; i++) {
    if (mb.status0[i] || mb.status[i]) return why = "status words not cleared", false;
    if (!all_zero((const uint8_t *)(mb.masks.get() + i * (size_t)mb.t * 8), (size_t)mb.t * 32)) return why = "mask rows not wiped", false;
  }
  if (!all_zero(mb.bytes.get() + mb.bytes_total, BPP_BYTES_SLACK)) return why = "slack not zero", false;
  // ---- dead slots
  for (size_t i = live; i < N; i++)
    if (!slot_is_sanitised(mb, i, t0, degree, nonces)) return false;
  if (bad_count) {
    if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_COUNT) || rec.code || rec.msg || rec.index) return why = "a bad count: COUNT alone expected", false;
    if (!(mb.state & BPP_REFILL_COUNT)) return why = "state word misses COUNT", false;
    const bpp_device_verdict v = verdict_finish(verdict_key_make(BPP_TIER_PASS1, 0, 0), true, BPP_VERIFY_ONLY, false, true, mb.state, 0);
    if (v.flags != (BPP_VERDICT_WRITTEN | BPP_VERDICT_REFILL) || v.code || v.tier || v.index) return why = "a bad count: the verdict claims something", false;
    return true;
  }
  if (live == 0) {
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "count 0: an empty record and a zero state expected", false;
    return true;
  }
  // ---- the fresh upload's kernel on the first c items, into buffers of its own
  const Arrays first(src, live, live, live);
  ModelBatch ref(live, first.pk, P, 0xab);
  std::unique_ptr<uint8_t[]> info(new uint8_t[live]);
  uint32_t res[BPP_ING_RES_WORDS];
  bpp_packed_batch plain = first.pk;
  plain.transcript_label = (const uint8_t *)"harness";
  plain.label_len = 7;
  const Ingest a = ingest_args(plain, P, ref.bytes.get(), ref.minvals.get(), ref.seeds.get(), info.get(), res);
  ingest_run_host<false>(a);
  bool foreign_any = false, finding_any = false;
  std::vector<uint8_t> stopped(live, 0);
  for (size_t i = 0; i < live; i++) {
    const uint8_t *p = plain.proofs + i * plain.proof_stride;
    const bool foreign = p[0] != t0;
    const bool finding = ingest_check_item(p, len, m, ingest_seed_present(a, i), false).msg != BPP_ING_OK;
    foreign_any = foreign_any || foreign;
    finding_any = finding_any || finding;
    stopped[i] = foreign || finding;
  }
  if (foreign_any) {
    if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK) || rec.code || rec.msg || rec.index) return why = "a foreign first byte below the count: FALLBACK alone expected", false;
  } else if (finding_any) {
    bool thrown = false;
    try {
      UploadPlan pl;
      ingest_finish_plan(plain, P, res, info.get(), pl);
    } catch (const ProofErr &e) {
      thrown = true;
      if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FINDING) || rec.code != e.code || rec.index != e.index || e.msg != ingest_message(rec.msg)) {
        printf("   upload {%d, \"%s\", %u}  refill {%d, \"%s\", %u} flags %u\n", e.code, e.msg.c_str(), e.index, rec.code, ingest_message(rec.msg), rec.index, rec.flags);
        return why = "the record is not the finding the upload of the first c items throws", false;
      }
    }
    if (!thrown) return why = "harness: a finding the upload does not throw", false;
  } else {
    // nothing below the count, whatever lies beyond it
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "clean below the count: an empty record and a zero state expected", false;
    UploadPlan pl;
    ingest_finish_plan(plain, P, res, info.get(), pl);  // (must not throw)
    for (size_t i = 0; i < live; i++) {
      if (mb.desc[i].flags != pl.desc[i].flags) return why = "flags differ from the plan's", false;
      if (mb.defer[i] != pl.defer[i]) return why = "defer[] differs from the plan's", false;
    }
  }
  // ---- live slots, item by item (the two layouts differ in their item counts: N here, c there)
  for (size_t i = 0; i < live; i++) {
    const uint8_t *slot = mb.bytes.get() + i * len, *cm = mb.bytes.get() + N * len + 32 * i * m;
    if ((mb.defer[i] & BPP_DEFER_DEGREE) != degree) return why = "degree bit is not the shape's", false;
    if (stopped[i]) {
      if (!slot_is_sanitised(mb, i, t0, degree, nonces)) return false;
      if (shape_exists && ingest_check_item(slot, len, m, false, false).msg != BPP_ING_OK) return why = "the sanitised slot does not pass ingest_check_item", false;
    } else {
      if (memcmp(slot, ref.bytes.get() + i * len, len) || memcmp(cm, ref.bytes.get() + live * len + 32 * i * m, 32 * (size_t)m))
        return why = "a taken item is not byte-equal to the upload's", false;
      if (memcmp(&mb.minvals[i * m], &ref.minvals[i * m], 8 * (size_t)m)) return why = "a taken item's promises differ", false;
      if (nonces && memcmp(mb.seeds.get() + 32 * i, ref.seeds.get() + 32 * i, 32)) return why = "a taken item's nonce differs", false;
      if (mb.desc[i].flags != (uint32_t)(info[i] & BPP_ING_INFO_SEED)) return why = "a taken item's nonce flag differs", false;
      if ((mb.defer[i] & BPP_DEFER_PROMISE) != (info[i] & BPP_ING_INFO_PROMISE)) return why = "a taken item's promise bit differs", false;
    }
  }
  return true;
}

// every count of the issue over one source; also: no count at all equals count = N
bool hold_counts(const Source &src, const ParamShape &P, uint8_t t0, bool shape_exists = true) {
  const uint32_t N = (uint32_t)src.n;
  for (uint32_t c : {0u, 1u, N - 1, N, N + 1, 0xffffffffu})
    if (!hold_count(src, P, t0, c, shape_exists)) {
      printf("   at count %u of %u\n", c, N);
      return false;
    }
  const Arrays all(src, N, N, N);
  ModelBatch a(N, all.pk, P, 0xcd), b(N, all.pk, P, 0xcd);
  const uint32_t n32 = N;
  a.refill(all.pk, P, t0, nullptr);
  b.refill(all.pk, P, t0, &n32);
  if (memcmp(a.bytes.get(), b.bytes.get(), a.bytes_total) || memcmp(&a.record, &b.record, 16) || a.state != b.state || a.live != N || b.live != N ||
      memcmp(a.defer.get(), b.defer.get(), N) || memcmp(a.minvals.get(), b.minvals.get(), 8 * N * src.m))
    return why = "no count is not count = N", false;
  return true;
}

#define EXPECT(name, cond)                                    \
  do {                                                        \
    if (cond) {                                               \
      printf("ok %s\n", name);                                \
    } else {                                                  \
      printf("FAIL %s (line %d): %s\n", name, __LINE__, why); \
      fails++;                                                \
    }                                                         \
  } while (0)

// ---- 2. the live routines and verdict_finish against the host rules on the cut batch
struct Want {
  int code = BPP_OK, tier = BPP_TIER_NONE;
  uint32_t index = 0;
  std::string msg;
};
Want host_finding(const std::vector<uint32_t> &status, const std::vector<uint8_t> &rounds_bad, const std::vector<uint8_t> &defer, uint32_t p0, uint32_t p1) {
  Want w;
  // the group as the verify() call of the cut batch sees it: its live proofs alone, counted from its first one
  const std::vector<uint32_t> st(status.begin() + p0, status.begin() + p1);
  const std::vector<uint8_t> rb(rounds_bad.begin() + p0, rounds_bad.begin() + p1), df(defer.begin() + p0, defer.begin() + p1);
  try {
    check_deferred(df, 0, p1 - p0);
    check_chunk_errors(st.data(), rb.data(), 0, p1 - p0);
  } catch (const ProofErr &e) {
    w.code = e.code;
    w.tier = e.tier;
    w.index = e.index;
    w.msg = e.msg;
  }
  return w;
}

void cut_groups() {
  std::mt19937_64 r(11);
  const uint8_t rb_of[3] = {0, BPP_ERR_INVALID_LENGTH, BPP_ERR_SIZE_OVERFLOW};
  bool ok = true;
  long empties = 0, middles = 0, at_boundary = 0;
  for (int it = 0; it < 4000 && ok; it++) {
    const uint32_t n = 2 + (uint32_t)(r() % 700), G = 1 + (uint32_t)(r() % (n < 6 ? n : 6));
    std::vector<uint32_t> bounds{0, n};
    while (bounds.size() < G + 1) {
      const uint32_t b = 1 + (uint32_t)(r() % (n - 1));
      bool dup = false;
      for (uint32_t x : bounds) dup = dup || x == b;
      if (!dup) bounds.push_back(b);
    }
    std::sort(bounds.begin(), bounds.end());
    // the count: exactly at a boundary (0 and n among them), or anywhere
    const uint32_t live = (it % 3 == 0) ? bounds[r() % bounds.size()] : (uint32_t)(r() % (n + 1));
    std::vector<uint32_t> status(n, 0);
    std::vector<uint8_t> rounds_bad(n, 0), defer(n, 0);
    // findings on both sides of the count; every dead slot carries the PASS-1 finding its sanitised bytes raise
    for (uint32_t f = 0, k = (uint32_t)(r() % 6); f < k; f++) {
      const uint32_t p = (uint32_t)(r() % n);
      switch (r() % 3) {
        case 0: status[p] |= 1u << (r() % 3); break;
        case 1: rounds_bad[p] = rb_of[1 + r() % 2]; break;
        default: defer[p] |= (uint8_t)(1u << (r() % 2)); break;
      }
    }
    for (uint32_t p = live; p < n; p++) status[p] |= BPP_ST_TRANSCRIPT_FAIL;
    for (uint32_t g = 0; g < G && ok; g++) {
      const uint32_t p0 = bounds[g], p1 = bounds[g + 1], len = verdict_group_live(p0, p1, live);
      // the group's live length is what clipping the boundaries to the count leaves
      const uint32_t c0 = p0 < live ? p0 : live, c1 = p1 < live ? p1 : live;
      ok = ok && len == c1 - c0;
      uint64_t key = BPP_VERDICT_KEY_NONE;
      for (uint32_t p = p0; p < p1; p++) {
        ok = ok && verdict_item_live(p, live) == (p < live);
        if (verdict_item_live(p, live)) key = verdict_min(key, verdict_key(defer[p], status[p], rounds_bad[p], p - p0));
      }
      empties += len == 0;
      middles += len != 0 && len != p1 - p0;
      at_boundary += live == p0 || live == p1;
      const Want found = len ? host_finding(status, rounds_bad, defer, p0, p0 + len) : Want();
      for (int want_msm = 0; want_msm < 2 && ok; want_msm++)
        for (int action = 0; action < 3; action++)
          for (int ident = 0; ident < 2; ident++)
            for (int zero = 0; zero < 2; zero++) {
              const bpp_device_verdict v = verdict_finish(key, want_msm != 0, action, ident != 0, zero != 0, 0ull, len);
              if (len == 0) {  // nothing is claimed, not even the redraw
                ok = ok && v.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_EMPTY) && v.code == BPP_OK && v.tier == BPP_TIER_NONE && v.index == 0;
                continue;
              }
              const bpp_device_verdict all_live = verdict_finish(key, want_msm != 0, action, ident != 0, zero != 0);
              ok = ok && memcmp(&v, &all_live, sizeof(v)) == 0;
              if (zero && want_msm && action != BPP_RECOVER_ONLY) {
                ok = ok && v.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_REDRAW) && v.code == BPP_OK && v.tier == BPP_TIER_NONE;
                continue;
              }
              Want w = found;
              if (w.tier == BPP_TIER_NONE && want_msm && action != BPP_RECOVER_ONLY && !ident) {
                w.code = BPP_ERR_VERIFICATION_FAILED;
                w.tier = BPP_TIER_MSM;
                w.msg = "Range proof batch not valid";
              }
              ok = ok && v.flags == BPP_VERDICT_WRITTEN && v.code == w.code && (int)v.tier == w.tier && v.index == w.index &&
                   w.msg == verdict_message(v.tier, v.code);
            }
      // a refill that did not take answers for empty groups too
      const bpp_device_verdict f = verdict_finish(key, true, 0, true, false, refill_state_make(BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK, 0, 0, 0), len);
      ok = ok && f.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_REFILL);
    }
    // a batch without a count word
    ok = ok && verdict_group_live(bounds[0], bounds[1], BPP_VERDICT_ALL_LIVE) == bounds[1] && verdict_item_live(n - 1, BPP_VERDICT_ALL_LIVE);
  }
  why = "the live routines and verdict_finish against the host rules on the cut batch";
  EXPECT("cut_groups", ok && empties > 100 && middles > 100 && at_boundary > 100);
}

}  // namespace

int main() {
  const ParamShape P64{64, 8, 1}, P64t3{64, 4, 3}, P8{8, 2, 1}, P16t2{16, 4, 2};
  for (uint32_t t : {1u, 3u}) {  // l, l - 1, 2^255, all ones in each of d1[k], r1, s1, at every index of a batch of five
    const ParamShape &P = t == 1 ? P64 : P64t3;
    std::vector<uint32_t> fields;
    for (uint32_t k = 0; k < t; k++) fields.push_back(k);
    fields.push_back(t + 3);
    fields.push_back(t + 4);
    bool all = true;
    for (size_t f = 0; f < fields.size() && all; f++)
      for (int v = 0; v < 4 && all; v++)
        for (size_t at = 0; at < 5 && all; at++) {
          std::vector<std::vector<uint8_t>> items;
          for (int i = 0; i < 5; i++) items.push_back(make_proof(t, 6));
          edge_scalar(v, &items[at][1 + 32 * fields[f]]);
          all = hold_counts(Source(items, 1, f), P, (uint8_t)t);
        }
    EXPECT(t == 1 ? "edge_scalars_t1" : "edge_scalars_t3", all);
  }
  {  // every truncation of a valid proof as the contents of a batch of that length
    const std::vector<uint8_t> full = make_proof(1, 6);
    bool all = true;
    for (size_t len = 1; len <= full.size() && all; len += (len < 40 || len + 40 > full.size()) ? 1 : 13) {
      std::vector<uint8_t> cut(full.begin(), full.begin() + len);
      all = hold_counts(Source({cut, cut, cut}, 1, 5), P64, 1, len == full.size());
    }
    EXPECT("truncations_t1", all);
  }
  {  // two findings, one on either side of most counts; a nonce with m = 2 in front of both
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 7; i++) items.push_back(make_proof(1, 7));
    edge_scalar(0, &items[5][1 + 32 * 4]);
    edge_scalar(3, &items[0][1 + 32 * 5]);
    Source c(items, 2, 3), d(items, 2);
    std::vector<uint8_t> only6{0, 0, 0, 0, 0, 0, 1};
    d.nonces(&only6);  // (the last item: dead at N - 1, a finding at N)
    EXPECT("two_findings", hold_counts(c, P64, 1) && hold_counts(d, P64, 1));
  }
  {  // a foreign first byte at the first, a middle and the last index; beside a finding on its other side
    bool all = true;
    for (size_t at : {0u, 3u, 6u}) {
      std::vector<std::vector<uint8_t>> items(7, make_proof(1, 6));
      items[at] = make_proof(3, 5);
      all = all && hold_counts(Source(items, 1, 7), P64, 1);
      items[at] = items[(at + 1) % 7];
      items[at][0] = 0;
      edge_scalar(0, &items[6 - at][1]);
      Source both(items, 1, 1);
      both.nonces(nullptr);
      all = all && hold_counts(both, P64, 1);
    }
    EXPECT("foreign_first_byte", all);
  }
  {  // nonces: at m = 2 on every item (a finding at index 0 for every count but 0), on the last item alone; at m = 1 on every other item
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 5; i++) items.push_back(make_proof(1, 7));
    Source every(items, 2), last(items, 2), alt(items, 1, 3), none(items, 1);
    std::vector<uint8_t> only4{0, 0, 0, 0, 1}, other{1, 0}, zero{0};
    every.nonces(nullptr);
    last.nonces(&only4);
    alt.nonces(&other);
    alt.promises({5, 0, 77}, {1, 0, 1});
    none.nonces(&zero);
    EXPECT("nonces", hold_counts(every, P64, 1) && hold_counts(last, P64, 1) && hold_counts(alt, P64, 1) && hold_counts(none, P64, 1));
  }
  {  // promises at the capacity, and parameters of t = 2 over t = 1 proofs: the degree bit on every slot, dead ones included
    std::vector<std::vector<uint8_t>> items, items2;
    for (int i = 0; i < 6; i++) items.push_back(make_proof(1, 3));
    for (int i = 0; i < 5; i++) items2.push_back(make_proof(1, 4));
    Source over(items, 1), deg(items2, 1);
    over.promises({255, 255, 256, 255, 256, 256}, {1});
    deg.promises({0, 1ull << 16, 0, 0, 1ull << 16}, {1});
    EXPECT("promises_and_degree", hold_counts(over, P8, 1) && hold_counts(deg, P16t2, 1));
  }
  {  // random mutations of content, batches of four
    bool all = true;
    for (int iter = 0; iter < 600 && all; iter++) {
      const uint32_t t = 1 + (uint32_t)(rng() % 3), r = 1 + (uint32_t)(rng() % 8), m = 1u << (rng() % 3);
      const size_t len = 1 + 32 * (size_t)(t + 5 + 2 * r);
      std::vector<std::vector<uint8_t>> items;
      for (int i = 0; i < 4; i++) {
        std::vector<uint8_t> p = make_proof(t, r);
        for (int k = 0; k < (int)(rng() % 3); k++) p[rng() % len] = (uint8_t)rng();
        if (rng() % 11 == 0) p[0] = (uint8_t)(rng() % 8);
        items.push_back(p);
      }
      Source c(items, m, rng() % 9);
      c.promises({rng(), rng() & 0xffff, 0}, {(uint8_t)(rng() & 1), 1, 0});
      if (rng() & 1) {
        std::vector<uint8_t> w{(uint8_t)(rng() & 1), (uint8_t)(rng() & 1), 1};
        c.nonces((rng() & 1) ? &w : nullptr);
      }
      all = hold_counts(c, (rng() & 1) ? P64t3 : P16t2, (uint8_t)t);
    }
    EXPECT("mutations", all);
  }
  cut_groups();
  printf("%d comparisons\n", checked);
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
