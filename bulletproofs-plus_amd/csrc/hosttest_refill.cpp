// Sanitizer harness (CPU test suite only): the one-lane host model of bpp_batch_refill_enqueue's kernels (refill.h: refill_run_host)
// is held to what a fresh device upload makes of the same arrays -- ingest_run_host + ingest_finish_plan of ingest.h, which
// hosttest_ingest.cpp in turn holds to the host packer -- over that harness's corpus (the cases a resident batch can meet: its
// shape exists), extended by batches with two findings and with one foreign first byte.
//   clean batch          bytes, promises, nonces equal ingest_run_host's output; flags and defer[] equal the plan's; state word 0
//   batch with findings  the record equals {code, message, index} that ingest_finish_plan throws
//   items with findings  the sanitised slot passes ingest_check_item; every other slot is byte-equal to the clean copy
//   foreign first byte   FALLBACK is set and no finding is claimed
//   two refills in a row the second refill's outputs do not depend on the first
//   verdict_finish       with a refill state: the specified record; with a zero state: the existing routine, over random groups
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_refill_host.py runs; every array is an exact-size
// heap allocation, so an access past what the engine allocates or the caller owns is an ASan report.  One "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "refill.h"

using namespace bpp;

static_assert(sizeof(bpp_device_refill) == 16, "the record is 16 bytes");
static_assert(BPP_VERDICT_REFILL != BPP_VERDICT_WRITTEN && BPP_VERDICT_REFILL != BPP_VERDICT_REDRAW, "verdict flags");

namespace {

std::mt19937_64 rng(20261020);

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

// a packed batch that owns exact-size copies of its arrays (the caller's side of a refill)
struct Case {
  size_t n = 0, len = 0, stride = 0;
  uint32_t m = 1;
  std::unique_ptr<uint8_t[]> proofs, commits, present, seeds, seed_present;
  std::unique_ptr<uint64_t[]> minv;
  bpp_packed_batch pk;

  Case(const std::vector<std::vector<uint8_t>> &items, uint32_t m_, size_t extra_stride = 0) : n(items.size()), m(m_) {
    len = items[0].size();
    stride = len + extra_stride;
    const size_t extent = (n - 1) * stride + len;
    proofs.reset(new uint8_t[extent]);
    memset(proofs.get(), 0xee, extent);
    for (size_t i = 0; i < n; i++) memcpy(proofs.get() + i * stride, items[i].data(), len);
    commits.reset(new uint8_t[32 * n * m]);
    for (size_t i = 0; i < 32 * n * m; i++) commits[i] = (uint8_t)rng();
    memset(&pk, 0, sizeof(pk));
    pk.n_items = n;
    pk.proofs = proofs.get();
    pk.proof_len = len;
    pk.proof_stride = stride;
    pk.commitments32 = commits.get();
    pk.m = m;
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
};

// what the engine holds of a resident batch of pk's shape: exact sizes, every byte the refill must write starts out as 0xcd (the
// "old contents"), the slack behind the bytes as zero (the upload left it so), the reduction words clear
struct ModelBatch {
  size_t n, len, bytes_total;
  uint32_t m, t;
  std::unique_ptr<uint8_t[]> bytes, seeds, defer;
  std::unique_ptr<uint64_t[]> minvals;
  std::unique_ptr<ProofDesc[]> desc;
  std::unique_ptr<uint32_t[]> status0, status, masks;
  uint32_t red[BPP_REFILL_RED_WORDS] = {0, 0};
  uint64_t state = ~0ull;
  bpp_device_refill record;

  ModelBatch(const bpp_packed_batch &pk, const ParamShape &P, uint8_t fill = 0xcd)
      : n(pk.n_items), len(pk.proof_len), bytes_total(n * len + n * (size_t)pk.m * 32), m(pk.m), t(P.t) {
    bytes.reset(new uint8_t[bytes_total + BPP_BYTES_SLACK]);
    memset(bytes.get(), fill, bytes_total);
    memset(bytes.get() + bytes_total, 0, BPP_BYTES_SLACK);
    seeds.reset(new uint8_t[pk.seed_nonces32 ? 32 * n : 1]);
    memset(seeds.get(), fill, pk.seed_nonces32 ? 32 * n : 1);
    defer.reset(new uint8_t[n]);
    memset(defer.get(), fill, n);
    minvals.reset(new uint64_t[n * m]);
    memset(minvals.get(), fill, n * m * 8);
    desc.reset(new ProofDesc[n]);
    memset(desc.get(), fill, n * sizeof(ProofDesc));
    status0.reset(new uint32_t[n]);
    status.reset(new uint32_t[n]);
    memset(status0.get(), fill, n * 4);
    memset(status.get(), fill, n * 4);
    masks.reset(new uint32_t[n * (size_t)t * 8]);
    memset(masks.get(), fill, n * (size_t)t * 32);
    memset(&record, fill, sizeof(record));
  }
  void refill(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0) {
    const Refill r = refill_args(pk, P, t0, bytes.get(), minvals.get(), seeds.get(), defer.get(), desc.get(), status0.get(), status.get(),
                                       masks.get(), red);
    refill_run_host<false>(r, &state, &record);
  }
  // everything a refill writes, as one string of bytes (flags of desc only: the other fields are the shape's)
  std::vector<uint8_t> outputs(bool nonces) const {
    std::vector<uint8_t> o(bytes.get(), bytes.get() + bytes_total + BPP_BYTES_SLACK);
    auto add = [&](const void *p, size_t k) { o.insert(o.end(), (const uint8_t *)p, (const uint8_t *)p + k); };
    if (nonces) add(seeds.get(), 32 * n);
    add(defer.get(), n);
    add(minvals.get(), n * m * 8);
    for (size_t i = 0; i < n; i++) add(&desc[i].flags, 4);
    add(status0.get(), n * 4);
    add(status.get(), n * 4);
    add(masks.get(), n * (size_t)t * 32);
    add(red, sizeof(red));
    add(&state, 8);
    add(&record, sizeof(record));
    return o;
  }
};

int fails = 0, checked = 0;
const char *why = "";

bool all_zero(const uint8_t *p, size_t k) {
  for (size_t i = 0; i < k; i++)
    if (p[i]) return false;
  return true;
}

// One refill of a model batch of pk's shape and first byte t0, held to the fresh device upload of the same arrays.  shape_exists:
// some clean proof of this (t0, length, m) exists, so a resident batch of the shape can (the sanitised slot must then pass the check).
bool hold(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0, bool shape_exists, ModelBatch *reuse = nullptr) {
  checked++;
  const size_t n = pk.n_items, len = pk.proof_len;
  const uint32_t m = pk.m;
  std::unique_ptr<ModelBatch> own;
  if (!reuse) own.reset(new ModelBatch(pk, P));
  ModelBatch &mb = reuse ? *reuse : *own;
  mb.refill(pk, P, t0);
  // the fresh upload's kernel on the same arrays, into buffers of its own
  ModelBatch ref(pk, P, 0xab);
  std::unique_ptr<uint8_t[]> info(new uint8_t[n]);
  uint32_t res[BPP_ING_RES_WORDS];
  bpp_packed_batch plain = pk;
  plain.transcript_label = (const uint8_t *)"harness";
  plain.label_len = 7;
  const Ingest a = ingest_args(plain, P, ref.bytes.get(), ref.minvals.get(), ref.seeds.get(), info.get(), res);
  ingest_run_host<false>(a);
  bool foreign_any = false, finding_any = false;
  std::vector<uint8_t> stopped(n, 0);
  for (size_t i = 0; i < n; i++) {
    const uint8_t *p = pk.proofs + i * pk.proof_stride;
    const bool foreign = p[0] != t0;
    const bool finding = ingest_check_item(p, len, m, ingest_seed_present(a, i), false).msg != BPP_ING_OK;
    foreign_any = foreign_any || foreign;
    finding_any = finding_any || finding;
    stopped[i] = foreign || finding;
  }
  // ---- the record and the state word
  const bpp_device_refill &rec = mb.record;
  if (mb.red[0] || mb.red[1]) return why = "the reduction words are not left clear", false;
  if (mb.state != refill_state_make(rec.flags, rec.code, rec.msg, rec.index)) return why = "state word is not the record's", false;
  if (foreign_any) {
    if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK) || rec.code || rec.msg || rec.index) return why = "a foreign first byte: FALLBACK alone expected", false;
    if (!(mb.state & BPP_REFILL_FALLBACK)) return why = "state word misses FALLBACK", false;
  } else if (finding_any) {
    // (all first bytes are t0: the blocking upload reaches ingest_finish_plan, which throws the lowest-index finding)
    if (res[BPP_ING_RES_DIFFERS]) return why = "harness: differs without a foreign byte", false;
    bool thrown = false;
    try {
      UploadPlan pl;
      ingest_finish_plan(plain, P, res, info.get(), pl);
    } catch (const ProofErr &e) {
      thrown = true;
      if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FINDING) || rec.code != e.code || rec.index != e.index || e.msg != ingest_message(rec.msg)) {
        printf("   upload {%d, \"%s\", %u}  refill {%d, \"%s\", %u} flags %u\n", e.code, e.msg.c_str(), e.index, rec.code, ingest_message(rec.msg), rec.index, rec.flags);
        return why = "the record is not the finding the upload throws", false;
      }
    }
    if (!thrown) return why = "harness: a finding the upload does not throw", false;
  } else {
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "a clean batch: an empty record and a zero state expected", false;
    UploadPlan pl;
    ingest_finish_plan(plain, P, res, info.get(), pl);  // (must not throw)
    for (size_t i = 0; i < n; i++) {
      if (mb.desc[i].flags != pl.desc[i].flags) return why = "flags differ from the plan's", false;
      if (mb.defer[i] != pl.defer[i]) return why = "defer[] differs from the plan's", false;
    }
    if (memcmp(mb.bytes.get(), ref.bytes.get(), mb.bytes_total + BPP_BYTES_SLACK)) return why = "bytes differ from the upload's", false;
    if (memcmp(mb.minvals.get(), ref.minvals.get(), n * m * 8)) return why = "promises differ from the upload's", false;
    if (pk.seed_nonces32 && memcmp(mb.seeds.get(), ref.seeds.get(), 32 * n)) return why = "nonces differ from the upload's", false;
  }
  // ---- item by item, whatever the record says
  const size_t proof_bytes = n * len;
  const uint8_t degree = t0 != P.t ? BPP_DEFER_DEGREE : 0;
  for (size_t i = 0; i < n; i++) {
    const uint8_t *slot = mb.bytes.get() + i * len, *cm = mb.bytes.get() + proof_bytes + 32 * i * m;
    if (mb.status0[i] || mb.status[i]) return why = "status words not cleared", false;
    if (!all_zero((const uint8_t *)(mb.masks.get() + i * (size_t)mb.t * 8), (size_t)mb.t * 32)) return why = "mask rows not wiped", false;
    if ((mb.defer[i] & BPP_DEFER_DEGREE) != degree) return why = "degree bit is not the shape's", false;
    if (stopped[i]) {
      if (slot[0] != t0 || !all_zero(slot + 1, len - 1)) return why = "a stopped item's slot is not t0 and zeros", false;
      if (shape_exists && ingest_check_item(slot, len, m, false, false).msg != BPP_ING_OK) return why = "the sanitised slot does not pass ingest_check_item", false;
      if (!all_zero(cm, 32 * (size_t)m)) return why = "a stopped item's commitments are not zero", false;
      for (uint32_t j = 0; j < m; j++)
        if (mb.minvals[i * m + j]) return why = "a stopped item keeps a promise", false;
      if (pk.seed_nonces32 && !all_zero(mb.seeds.get() + 32 * i, 32)) return why = "a stopped item keeps a nonce", false;
      if (mb.desc[i].flags || (mb.defer[i] & BPP_DEFER_PROMISE)) return why = "a stopped item keeps a flag", false;
    } else {
      if (memcmp(slot, ref.bytes.get() + i * len, len) || memcmp(cm, ref.bytes.get() + proof_bytes + 32 * i * m, 32 * (size_t)m))
        return why = "a taken item is not byte-equal to the clean copy", false;
      if (memcmp(&mb.minvals[i * m], &ref.minvals[i * m], 8 * (size_t)m)) return why = "a taken item's promises differ", false;
      if (pk.seed_nonces32 && memcmp(mb.seeds.get() + 32 * i, ref.seeds.get() + 32 * i, 32)) return why = "a taken item's nonce differs", false;
      if (mb.desc[i].flags != (uint32_t)(info[i] & BPP_ING_INFO_SEED)) return why = "a taken item's nonce flag differs", false;
      if ((mb.defer[i] & BPP_DEFER_PROMISE) != (info[i] & BPP_ING_INFO_PROMISE)) return why = "a taken item's promise bit differs", false;
    }
  }
  if (!all_zero(mb.bytes.get() + mb.bytes_total, BPP_BYTES_SLACK)) return why = "slack not zero", false;
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

bool record_is(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0, uint32_t flags, int code, uint32_t msg, uint32_t index) {
  ModelBatch mb(pk, P);
  mb.refill(pk, P, t0);
  const bpp_device_refill &r = mb.record;
  if (r.flags != flags || r.code != code || r.msg != msg || r.index != index) {
    printf("   record {%d, %u, %u, flags %u}, wanted {%d, %u, %u, flags %u}\n", r.code, r.msg, r.index, r.flags, code, msg, index, flags);
    return why = "the record is not the one the case is about", false;
  }
  return hold(pk, P, t0, true);
}

void verdict_with_state() {
  std::mt19937_64 r(7);
  bool ok = true;
  for (int it = 0; it < 20000 && ok; it++) {
    // a random group's key, as hosttest_verdict.cpp's random groups make them: a tier, an index, an order inside PASS 2 -- or none
    const uint32_t tier = (uint32_t)(r() % 7);
    const uint64_t key = tier < 2 ? BPP_VERDICT_KEY_NONE : verdict_key_make(tier, (uint32_t)(r() % 600), tier == BPP_TIER_PASS2 ? (uint32_t)(r() % 3) : 0);
    const bool want_msm = r() & 1, ident = r() & 1, zero = (r() % 4) == 0;
    const int action = (int)(r() % 3);
    const bpp_device_verdict a = verdict_finish(key, want_msm, action, ident, zero), b = verdict_finish(key, want_msm, action, ident, zero, 0ull);
    ok = memcmp(&a, &b, sizeof(a)) == 0;
    // a state word with WRITTEN alone is a refill that took
    const bpp_device_verdict c = verdict_finish(key, want_msm, action, ident, zero, refill_state_make(BPP_REFILL_WRITTEN, 0, 0, 0));
    ok = ok && memcmp(&a, &c, sizeof(a)) == 0;
    const uint32_t msg = 1 + (uint32_t)(r() % 8), index = (uint32_t)(r() % (1u << 24));
    const int code = ingest_finding(msg).code;  // (BPP_ERR_ENGINE, a negative one, among them)
    const bpp_device_verdict f =
        verdict_finish(key, want_msm, action, ident, zero, refill_state_make(BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, code, msg, index));
    ok = ok && f.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_REFILL) && f.code == code && f.tier == BPP_TIER_CONSTRUCTION && f.index == index;
    const bpp_device_verdict g = verdict_finish(key, want_msm, action, ident, zero, refill_state_make(BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK, 0, 0, 0));
    ok = ok && g.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_REFILL) && g.code == 0 && g.tier == BPP_TIER_NONE && g.index == 0;
  }
  why = "verdict_finish with a refill state";
  EXPECT("verdict_finish_with_refill_state", ok);
}

}  // namespace

int main() {
  const ParamShape P64{64, 8, 1}, P64t3{64, 4, 3}, P8{8, 2, 1}, P16t2{16, 4, 2};
  for (uint32_t t : {1u, 3u}) {  // every truncation of a valid proof as the new contents of a batch of that length (the upload's own corpus)
    const ParamShape &P = t == 1 ? P64 : P64t3;
    const std::vector<uint8_t> full = make_proof(t, 6);
    bool all = true;
    for (size_t len = 1; len <= full.size() && all; len++) {
      std::vector<uint8_t> cut(full.begin(), full.begin() + len);
      Case one({cut}, 1), three({cut, cut, cut}, 1, 5);
      all = hold(one.pk, P, (uint8_t)t, len == full.size()) && hold(three.pk, P, (uint8_t)t, len == full.size());
    }
    EXPECT(t == 1 ? "truncations_t1" : "truncations_t3", all);
  }
  for (uint32_t t : {1u, 3u}) {  // l, l - 1, 2^255, all ones in each of d1[k], r1, s1, alone and across two proofs
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
        Case c({good, good, bad, good}, 1, f);
        all = all && (v == 1 ? record_is(c.pk, P, (uint8_t)t, BPP_REFILL_WRITTEN, 0, 0, 0)
                             : record_is(c.pk, P, (uint8_t)t, BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, BPP_ERR_INVALID_ARGUMENT, BPP_ING_PARSING, 2));
      }
    EXPECT(t == 1 ? "edge_scalars_t1" : "edge_scalars_t3", all);
  }
  {  // two findings: the lowest index wins, whatever their kinds; both items are stopped
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 7; i++) items.push_back(make_proof(1, 7));
    edge_scalar(0, &items[5][1 + 32 * 4]);
    edge_scalar(3, &items[2][1 + 32 * 5]);
    Case c(items, 2, 3), d(items, 2);
    std::vector<uint8_t> only1{0, 1, 0, 0, 0, 0, 0};
    d.nonces(&only1);  // a nonce with m = 2 at item 1, in front of both
    EXPECT("two_findings", record_is(c.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, BPP_ERR_INVALID_ARGUMENT, BPP_ING_PARSING, 2) &&
                               record_is(d.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, BPP_ERR_INVALID_ARGUMENT, BPP_ING_SEED_AGGREGATED, 1));
  }
  {  // one foreign first byte (a valid proof of another degree in the same number of bytes; a byte no proof starts with), alone and
     // beside a finding at a lower index: FALLBACK, nothing else claimed
    std::vector<std::vector<uint8_t>> items(7, make_proof(1, 6));
    items[4] = make_proof(3, 5);
    Case c(items, 1, 7);
    items[4] = items[0];
    items[4][0] = 0;
    Case z(items, 1);
    edge_scalar(0, &items[1][1]);
    Case both(items, 1, 1);
    both.nonces(nullptr);
    EXPECT("foreign_first_byte", record_is(c.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK, 0, 0, 0) &&
                                     record_is(z.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK, 0, 0, 0) &&
                                     record_is(both.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK, 0, 0, 0));
  }
  {  // a seed nonce with m = 2: every item; only item 3, behind a non-canonical s1 in item 2; no item after all
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 5; i++) items.push_back(make_proof(1, 7));
    Case every(items, 2), nobody(items, 2), alone(items, 2);
    std::vector<uint8_t> only3{0, 0, 0, 1, 0}, none{0};
    every.nonces(nullptr);
    nobody.nonces(&none);
    alone.nonces(&only3);
    edge_scalar(0, &items[2][1 + 32 * 5]);
    Case mixed(items, 2);
    mixed.nonces(&only3);
    EXPECT("seed_with_m2", record_is(every.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, BPP_ERR_INVALID_ARGUMENT, BPP_ING_SEED_AGGREGATED, 0) &&
                               record_is(mixed.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, BPP_ERR_INVALID_ARGUMENT, BPP_ING_PARSING, 2) &&
                               record_is(alone.pk, P64, 1, BPP_REFILL_WRITTEN | BPP_REFILL_FINDING, BPP_ERR_INVALID_ARGUMENT, BPP_ING_SEED_AGGREGATED, 3) &&
                               record_is(nobody.pk, P64, 1, BPP_REFILL_WRITTEN, 0, 0, 0));
  }
  {  // nonces at m = 1: all, every other item (flags bit 0, zeros where absent), none; promises beside them
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 9; i++) items.push_back(make_proof(1, 6));
    Case all_(items, 1), alt(items, 1, 3), none(items, 1);
    std::vector<uint8_t> other{1, 0}, zero{0};
    all_.nonces(nullptr);
    alt.nonces(&other);
    none.nonces(&zero);
    alt.promises({5, 0, 77}, {1, 0, 1});
    EXPECT("nonces_m1", record_is(all_.pk, P64, 1, BPP_REFILL_WRITTEN, 0, 0, 0) && record_is(alt.pk, P64, 1, BPP_REFILL_WRITTEN, 0, 0, 0) &&
                            record_is(none.pk, P64, 1, BPP_REFILL_WRITTEN, 0, 0, 0));
  }
  {  // promises 2^n - 1 and 2^n at n = 8, at m = 1 and m = 2: a finding of verify time, the refill takes the item and sets its bit
    std::vector<std::vector<uint8_t>> items, items2;
    for (int i = 0; i < 6; i++) items.push_back(make_proof(1, 3));
    for (int i = 0; i < 3; i++) items2.push_back(make_proof(1, 4));
    Case fits(items, 1), over(items, 1), unset(items, 1), agg(items2, 2);
    fits.promises({255}, {1});
    over.promises({255, 255, 256, 255, 256, 255}, {1});
    unset.promises({256}, {0});
    agg.promises({1, 2, 3, 256, 5, 6}, {1});
    ModelBatch mb(over.pk, P8), ma(agg.pk, P8);
    mb.refill(over.pk, P8, 1);
    ma.refill(agg.pk, P8, 1);
    const bool bits = std::vector<uint8_t>(mb.defer.get(), mb.defer.get() + 6) == std::vector<uint8_t>({0, 0, BPP_DEFER_PROMISE, 0, BPP_DEFER_PROMISE, 0}) &&
                      std::vector<uint8_t>(ma.defer.get(), ma.defer.get() + 3) == std::vector<uint8_t>({0, BPP_DEFER_PROMISE, 0});
    why = "promise bits";
    EXPECT("promises_at_the_capacity", bits && record_is(fits.pk, P8, 1, BPP_REFILL_WRITTEN, 0, 0, 0) && record_is(over.pk, P8, 1, BPP_REFILL_WRITTEN, 0, 0, 0) &&
                                           record_is(unset.pk, P8, 1, BPP_REFILL_WRITTEN, 0, 0, 0) && record_is(agg.pk, P8, 1, BPP_REFILL_WRITTEN, 0, 0, 0));
  }
  {  // parameters of t = 2 over a batch of t = 1 proofs with an oversized promise: the degree bit on every item, the promise bit on one
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 5; i++) items.push_back(make_proof(1, 4));
    Case c(items, 1);
    c.promises({0, 1ull << 16, 0, 0, 0}, {1});
    ModelBatch mb(c.pk, P16t2);
    mb.refill(c.pk, P16t2, 1);
    why = "degree and promise bits";
    EXPECT("degree_and_promise", std::vector<uint8_t>(mb.defer.get(), mb.defer.get() + 5) == std::vector<uint8_t>({1, 3, 1, 1, 1}) &&
                                     record_is(c.pk, P16t2, 1, BPP_REFILL_WRITTEN, 0, 0, 0));
  }
  {  // two refills in a row on one model batch: findings and nonces first, then clean contents without nonces on any item -- the
     // second leaves what it leaves on a batch that never saw the first
    std::vector<std::vector<uint8_t>> dirty, clean;
    for (int i = 0; i < 6; i++) {
      dirty.push_back(make_proof(1, 6));
      clean.push_back(make_proof(1, 6));
    }
    edge_scalar(2, &dirty[1][1]);
    dirty[4][0] = 2;
    Case a(dirty, 1, 2), b(clean, 1);
    std::vector<uint8_t> none{0};
    a.nonces(nullptr);
    a.promises({1ull << 40}, {1});
    b.nonces(&none);
    b.promises({3}, {1, 0});
    ModelBatch twice(a.pk, P8), once(b.pk, P8, 0x37);
    bool ok = hold(a.pk, P8, 1, true, &twice) && (twice.state & BPP_REFILL_FALLBACK);
    ok = ok && hold(b.pk, P8, 1, true, &twice) && hold(b.pk, P8, 1, true, &once);
    if (ok && twice.outputs(true) != once.outputs(true)) {
      ok = false;
      why = "the second refill's outputs depend on the first";
    }
    ok = ok && twice.state == 0 && all_zero(twice.seeds.get(), 32 * 6);
    EXPECT("two_refills_in_a_row", ok);
  }
  {  // random mutations of content, batches of three, against a shape that exists
    bool all = true;
    for (int iter = 0; iter < 1500 && all; iter++) {
      const uint32_t t = 1 + (uint32_t)(rng() % 3), r = 1 + (uint32_t)(rng() % 8), m = 1u << (rng() % 3);
      const size_t len = 1 + 32 * (size_t)(t + 5 + 2 * r);
      std::vector<std::vector<uint8_t>> items;
      for (int i = 0; i < 3; i++) {
        std::vector<uint8_t> p = make_proof(t, r);
        for (int k = 0; k < (int)(rng() % 3); k++) p[rng() % len] = (uint8_t)rng();
        if (rng() % 11 == 0) p[0] = (uint8_t)(rng() % 8);
        items.push_back(p);
      }
      Case c(items, m, rng() % 9);
      c.promises({rng(), rng() & 0xffff, 0}, {(uint8_t)(rng() & 1), 1, 0});
      if (rng() & 1) {
        std::vector<uint8_t> w{(uint8_t)(rng() & 1), (uint8_t)(rng() & 1), 1};
        c.nonces((rng() & 1) ? &w : nullptr);
      }
      all = hold(c.pk, (rng() & 1) ? P64t3 : P16t2, (uint8_t)t, true);
    }
    EXPECT("mutations", all);
  }
  verdict_with_state();
  printf("%d comparisons\n", checked);
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
