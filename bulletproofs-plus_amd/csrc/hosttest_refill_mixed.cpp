// Sanitizer harness (CPU test suite only): a refill of a batch of MIXED aggregation factors (bpp_batch_refill_enqueue_mixed), plain,
// with a live count and under a live mask.
//
// The one-lane host model of the refill kernels (refill.h: refill_run_host<true>) runs over a batch whose shape vector
// (proof_lens[i], m[i]) comes from a sound corpus, and is held to what a fresh device upload makes of the rows in question -- all of
// them, the first c, the live ones alone in slot order: ingest_mixed_host_prelude + ingest_run_host<true> + ingest_mixed_finish_plan
// of ingest.h / ingest_mixed.h over a batch of those rows:
//   record and state   what the upload throws, its index k mapped to the slot of the k-th live row; FALLBACK for a foreign first byte
//                      at a live row, before any finding; BPP_REFILL_COUNT for a count beyond the batch; clean otherwise, whatever
//                      lies at dead rows
//   live slots         the upload's bytes, promises, nonce, nonce flag and deferred bits of the k-th row, at the SLOT's offsets
//   dead and refused   byte for byte the sanitised slot of ITS OWN lengths: t0 and proof_len[i] - 1 zeros, 32 * m[i] zero bytes, no
//                      promise, no nonce, no flag, the shape's degree bit; it passes ingest_check_item for (proof_len[i], m[i])
//   everywhere         cleared status words, wiped mask rows, zero slack, clear reduction words, nothing written past the batch
//   sources            the arrays the model is handed END behind the last live row; row slack and every dead row are poisoned for
//                      AddressSanitizer (a read is a report) and hold a byte pattern; a second run over full-length arrays and other
//                      old contents must leave the same bytes, none of them the pattern.  Source strides differ from the upload's.
// Findings and foreign first bytes are planted at the first and the last slot, in the shortest row (maximal slack) and in an m = 4 row,
// and fall on live and on dead slots under the masks.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_refill_mixed_host.py runs.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "refill.h"

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

std::mt19937_64 rng(20261023);
const uint8_t PATTERN[8] = {0xa7, 0x5c, 0x3e, 0x91, 0xd2, 0x4b, 0x68, 0xf3};

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
void group_order(uint8_t out[32]) {
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  memcpy(out, L, 32);
}
uint32_t log2u(uint32_t v) {
  uint32_t r = 0;
  while ((1u << r) < v) r++;
  return r;
}

struct Item {
  std::vector<uint8_t> proof;
  uint32_t m = 1;
  bool nonce = false;
  std::vector<uint64_t> minv;  // empty: no promise
  std::vector<uint8_t> present;
  std::vector<uint8_t> commits, seed;  // 32 * m bytes, 32 bytes: the row's contents whatever the strides of the arrays
};

// the m pattern of the tests: sound items of first byte t under n_bits, nonces on the m = 1 items, promises on every third
std::vector<Item> pattern(size_t n, uint32_t n_bits, uint32_t t, uint32_t m_max = 4) {
  static const uint32_t ms[7] = {4, 1, 2, 1, 1, 4, 2};
  std::vector<Item> v;
  for (size_t i = 0; i < n; i++) {
    Item it;
    it.m = std::min(ms[i % 7], m_max);
    it.proof = make_proof(t, log2u(it.m * n_bits));
    it.nonce = it.m == 1;
    it.commits.resize(32 * (size_t)it.m);
    it.seed.resize(32);
    for (auto &x : it.commits) x = (uint8_t)rng();
    for (auto &x : it.seed) x = (uint8_t)(rng() | 1);
    if (i % 3 == 0) {
      it.minv = {rng() & 0x7f, 0, 3, 1};
      it.present = {1, 0, 1, 1};
    }
    v.push_back(it);
  }
  return v;
}

// Rows [0, keep) of `items` as the six arrays of a bpp_mixed_batch that claims `claim` rows: one allocation per array, exact to the
// last byte row keep - 1 uses; the slack of every row and (hide) the whole of every dead row are poisoned for AddressSanitizer; dead
// rows hold the byte pattern.  proof_lens / m are the items' own.
struct Rows {
  size_t n, stride;
  uint32_t m_stride;
  std::vector<size_t> lens;
  std::vector<uint32_t> ms;
  uint8_t *proofs = nullptr, *commits = nullptr, *present = nullptr, *seeds = nullptr, *seed_present = nullptr;
  uint64_t *minv = nullptr;
  size_t proofs_n = 0, entries = 0;
  bpp_mixed_batch mx;

  static void pattern_fill(void *p, size_t k) {
    for (size_t i = 0; i < k; i++) ((uint8_t *)p)[i] = PATTERN[i % 8];
  }
  Rows(const std::vector<Item> &items, size_t keep, size_t claim, const std::vector<uint8_t> &dead, bool hide, size_t extra_stride, uint32_t m_stride_)
      : n(keep), m_stride(m_stride_) {
    size_t longest = 0;
    for (const Item &it : items) {
      lens.push_back(it.proof.size());
      ms.push_back(it.m);
      longest = std::max(longest, it.proof.size());
    }
    stride = (longest + extra_stride + 7) & ~(size_t)7;
    auto is_dead = [&](size_t i) { return !dead.empty() && dead[i] != 0; };
    proofs_n = n ? (n - 1) * stride + lens[n - 1] : 0;
    entries = n ? (n - 1) * (size_t)m_stride + ms[n - 1] : 0;
    proofs = (uint8_t *)malloc(proofs_n ? proofs_n : 1);
    commits = (uint8_t *)malloc(entries * 32 + 1);
    minv = (uint64_t *)malloc(entries * 8 + 8);
    present = (uint8_t *)malloc(entries + 1);
    seeds = (uint8_t *)malloc(32 * n + 1);
    seed_present = (uint8_t *)malloc(n + 1);
    memset(proofs, 0xff, proofs_n);
    memset(commits, 0xff, entries * 32);
    for (size_t q = 0; q < entries; q++) {  // slack that would change the outcome if it were used
      minv[q] = 1ull << 63;
      present[q] = 1;
    }
    for (size_t i = 0; i < n; i++) {
      const Item &it = items[i];
      const size_t row = i * (size_t)m_stride;
      const bool last = i + 1 == n;
      if (is_dead(i)) {
        pattern_fill(proofs + i * stride, lens[i]);
        pattern_fill(commits + 32 * row, 32 * (size_t)it.m);
        pattern_fill(minv + row, 8 * (size_t)it.m);
        pattern_fill(present + row, it.m);
        pattern_fill(seeds + 32 * i, 32);
        seed_present[i] = PATTERN[i % 8];
      } else {
        memcpy(proofs + i * stride, it.proof.data(), lens[i]);
        memcpy(commits + 32 * row, it.commits.data(), 32 * (size_t)it.m);
        memcpy(seeds + 32 * i, it.seed.data(), 32);
        for (uint32_t j = 0; j < it.m; j++) {
          minv[row + j] = it.minv.empty() ? 0 : it.minv[j % it.minv.size()];
          present[row + j] = it.present.empty() ? 0 : it.present[j % it.present.size()];
        }
        seed_present[i] = it.nonce ? 1 : 0;
      }
      const bool whole = hide && is_dead(i);
      const size_t p0 = whole ? 0 : lens[i], e0 = whole ? 0 : it.m;
      const size_t p1 = last ? lens[i] : stride, e1 = last ? it.m : m_stride;
      POISON(proofs + i * stride + p0, p1 - p0);
      POISON(commits + 32 * (row + e0), 32 * (e1 - e0));
      POISON(minv + row + e0, 8 * (e1 - e0));
      POISON(present + row + e0, e1 - e0);
      if (whole) POISON(seeds + 32 * i, 32);
    }
    memset(&mx, 0, sizeof(mx));
    mx.n_items = claim;
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
  }
  Rows(const Rows &) = delete;
  ~Rows() {
    UNPOISON(proofs, proofs_n);
    UNPOISON(commits, entries * 32);
    UNPOISON(minv, entries * 8);
    UNPOISON(present, entries);
    UNPOISON(seeds, 32 * n);
    free(proofs);
    free(commits);
    free(minv);
    free(present);
    free(seeds);
    free(seed_present);
  }
};

// what the engine holds of a resident mixed batch of the shape `pre`: exact sizes, every byte a refill must write starts as `fill`
struct ModelBatch {
  size_t n, bytes_total, sum_m;
  uint32_t t;
  std::unique_ptr<IngestMixedRow[]> rows;
  std::unique_ptr<uint8_t[]> bytes, seeds, defer, mask;
  std::unique_ptr<uint64_t[]> minvals;
  std::unique_ptr<ProofDesc[]> desc;
  std::unique_ptr<uint32_t[]> status0, status, masks;
  uint32_t red[BPP_REFILL_RED_WORDS] = {0, 0};
  uint64_t state = ~0ull, proof_bytes;
  uint32_t live = 0xdddddddd;
  bpp_device_refill record;

  ModelBatch(const IngestMixedPrelude &pre, const ParamShape &P, uint8_t fill)
      : n(pre.rows.size()), bytes_total((size_t)(pre.proof_bytes + 32 * pre.sum_m)), sum_m((size_t)pre.sum_m), t(P.t), proof_bytes(pre.proof_bytes) {
    rows.reset(new IngestMixedRow[n]);
    memcpy(rows.get(), pre.rows.data(), n * sizeof(IngestMixedRow));
    bytes.reset(new uint8_t[bytes_total + BPP_BYTES_SLACK]);
    memset(bytes.get(), fill, bytes_total);
    memset(bytes.get() + bytes_total, 0, BPP_BYTES_SLACK);
    seeds.reset(new uint8_t[32 * n + 1]);
    memset(seeds.get(), fill, 32 * n + 1);
    defer.reset(new uint8_t[n + 1]);
    memset(defer.get(), fill, n + 1);
    mask.reset(new uint8_t[n + 1]);
    memset(mask.get(), fill, n + 1);
    minvals.reset(new uint64_t[sum_m + 1]);
    memset(minvals.get(), fill, (sum_m + 1) * 8);
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
  // the call as the engine makes it: proof_lens, m and the transcript fields of `mx` are not passed on
  void refill(const bpp_mixed_batch &mx, const ParamShape &P, uint8_t t0, const uint32_t *count, const uint8_t *mask_bytes) {
    bpp_mixed_batch bare = mx;
    bare.proof_lens = nullptr;
    bare.m = nullptr;
    const Refill r = refill_mixed_args(bare, P, t0, rows.get(), n, proof_bytes, sum_m, bytes.get(), minvals.get(), seeds.get(), defer.get(),
                                            desc.get(), status0.get(), status.get(), masks.get(), red, count, mask_bytes, mask.get());
    refill_run_host<true>(r, &state, &record, &live);
  }
  // ... of a batch whose rows are uniform, by arithmetic: no table
  void refill_packed(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0, const uint32_t *count, const uint8_t *mask_bytes) {
    const Refill r = refill_args(pk, P, t0, bytes.get(), minvals.get(), seeds.get(), defer.get(), desc.get(), status0.get(), status.get(),
                                 masks.get(), red, count, mask_bytes, mask.get());
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
// eight consecutive bytes of the pattern, at any phase
bool has_pattern(const uint8_t *p, size_t k) {
  for (size_t i = 0; i + 8 <= k; i++)
    for (int ph = 0; ph < 8; ph++) {
      int q = 0;
      while (q < 8 && p[i + q] == PATTERN[(ph + q) % 8]) q++;
      if (q == 8) return true;
    }
  return false;
}

// the sanitised slot of item i, byte for byte, from ITS lengths; it must pass the walk
bool slot_is_sanitised(const ModelBatch &mb, size_t i, uint8_t t0, uint8_t degree) {
  const IngestMixedRow &r = mb.rows[i];
  const uint8_t *slot = mb.bytes.get() + r.proof_off, *cm = mb.bytes.get() + mb.proof_bytes + 32 * (size_t)r.minval_idx;
  if (slot[0] != t0 || !all_zero(slot + 1, r.proof_len - 1)) return why = "a slot is not t0 and zeros over its own length", false;
  if (!all_zero(cm, 32 * (size_t)r.m)) return why = "commitments are not zero", false;
  for (uint32_t j = 0; j < r.m; j++)
    if (mb.minvals[r.minval_idx + j]) return why = "a promise is kept", false;
  if (!all_zero(mb.seeds.get() + 32 * i, 32)) return why = "a nonce is kept", false;
  if (mb.desc[i].flags) return why = "a flag is kept", false;
  if (mb.defer[i] != degree) return why = "defer is not the shape's degree bit alone", false;
  if (ingest_check_item(slot, r.proof_len, r.m, false, false).msg != BPP_ING_OK) return why = "the sanitised slot does not pass ingest_check_item", false;
  return true;
}

enum Form { PLAIN, COUNT, MASK };

// One refill of a batch shaped by `shape` (sound items) with the contents `items` (the same lengths and factors), held to the fresh
// device upload of the live rows.  count: the live count (COUNT); mask: N bytes (MASK).
bool hold(const std::vector<Item> &shape, const std::vector<Item> &items, const ParamShape &P, Form form, uint32_t count, const std::vector<uint8_t> &mask) {
  checked++;
  const size_t N = shape.size();
  const uint8_t t0 = shape[0].proof[0], degree = t0 != P.t ? BPP_DEFER_DEGREE : 0;
  // ---- the shape, as the upload recorded it (its own strides)
  const Rows up(shape, N, N, {}, false, 8, 8);
  IngestMixedPrelude pre;
  if (!ingest_mixed_host_prelude(up.mx, P, pre) || pre.h != N) return why = "harness: the shape is not a sound batch", false;
  std::vector<size_t> slots;  // the live slots in slot order
  std::vector<uint8_t> dead(N, 0);
  for (size_t i = 0; i < N; i++) {
    const bool lv = form == MASK ? mask[i] != 0 : (form == COUNT ? (count <= N && i < count) : true);
    if (lv) slots.push_back(i);
    else dead[i] = 1;
  }
  const size_t L = slots.size(), end = L ? slots.back() + 1 : 0;
  // ---- the model: arrays that end behind the last live row, dead rows and slack unreadable; then full-length arrays, other contents
  const Rows cut(items, end, N, dead, true, 16, 4), full(items, N, N, dead, false, 0, 5);
  std::unique_ptr<uint8_t[]> mask_exact(new uint8_t[N]);
  if (form == MASK) memcpy(mask_exact.get(), mask.data(), N);
  std::unique_ptr<uint32_t> count_word(new uint32_t(count));
  const uint32_t *cw = form == COUNT ? count_word.get() : nullptr;
  const uint8_t *mw = form == MASK ? mask_exact.get() : nullptr;
  ModelBatch mb(pre, P, 0xcd), mp(pre, P, 0x37);
  mb.refill(cut.mx, P, t0, cw, mw);
  mp.refill(full.mx, P, t0, cw, mw);
  const size_t sum_m = mb.sum_m;
  if (form == MASK) {
    if (mb.live != 0xdddddddd) return why = "a mask refill wrote the count word", false;
    for (size_t i = 0; i < N; i++)
      if (mb.mask[i] != (mask[i] ? 1 : 0) || mp.mask[i] != mb.mask[i]) return why = "the batch's mask is not the normalised mask", false;
  } else {
    if (mb.live != refill_live(form == COUNT ? count : (uint32_t)N, (uint32_t)N)) return why = "the batch's count word is not the clamped count", false;
    for (size_t i = 0; i <= N; i++)
      if (mb.mask[i] != 0xcd) return why = "a refill without a mask wrote the batch's mask", false;
  }
  if (memcmp(mb.bytes.get(), mp.bytes.get(), mb.bytes_total + BPP_BYTES_SLACK) || memcmp(mb.minvals.get(), mp.minvals.get(), sum_m * 8) ||
      memcmp(mb.seeds.get(), mp.seeds.get(), 32 * N) || memcmp(mb.defer.get(), mp.defer.get(), N) || memcmp(&mb.record, &mp.record, sizeof(mb.record)) ||
      mb.state != mp.state)
    return why = "the outputs depend on the source strides, on dead rows or on the old contents", false;
  if (has_pattern(mp.bytes.get(), mp.bytes_total) || has_pattern((const uint8_t *)mp.minvals.get(), sum_m * 8) || has_pattern(mp.seeds.get(), 32 * N))
    return why = "bytes of a dead row appear in the batch", false;
  for (size_t i = 0; i < N; i++)
    if (mp.desc[i].flags > 1 || mp.desc[i].flags != mb.desc[i].flags) return why = "a dead row reached the flags", false;
  // (guard bytes behind every array: nothing is written past slot N - 1)
  if (mb.defer[N] != 0xcd || mb.status[N] != 0xcdcdcdcdu || mb.status0[N] != 0xcdcdcdcdu || mb.masks[N * (size_t)mb.t * 8] != 0xcdcdcdcdu ||
      mb.minvals[sum_m] != 0xcdcdcdcdcdcdcdcdull || mb.seeds[32 * N] != 0xcd)
    return why = "a write past the batch's last slot", false;
  if (mb.red[0] || mb.red[1]) return why = "the reduction words are not left clear", false;
  const bpp_device_refill &rec = mb.record;
  if (mb.state != refill_state_make(rec.flags, rec.code, rec.msg, rec.index)) return why = "state word is not the record's", false;
  for (size_t i = 0; i < N; i++) {
    if (mb.status0[i] || mb.status[i]) return why = "status words not cleared", false;
    if (!all_zero((const uint8_t *)(mb.masks.get() + i * (size_t)mb.t * 8), (size_t)mb.t * 32)) return why = "mask rows not wiped", false;
  }
  if (!all_zero(mb.bytes.get() + mb.bytes_total, BPP_BYTES_SLACK)) return why = "slack not zero", false;
  for (size_t i = 0; i < N; i++)
    if (dead[i] && !slot_is_sanitised(mb, i, t0, degree)) return false;
  if (form == COUNT && count > N) {
    if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_COUNT) || rec.code || rec.msg || rec.index) return why = "a count beyond the batch: COUNT alone expected", false;
    return true;
  }
  if (rec.flags & BPP_REFILL_COUNT) return why = "BPP_REFILL_COUNT without a count beyond the batch", false;
  if (L == 0) {
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "nothing live: an empty record and a zero state expected", false;
    return true;
  }
  // ---- the fresh upload of the live rows alone, in slot order, into buffers of its own
  std::vector<Item> comp;
  for (size_t s : slots) comp.push_back(items[s]);
  const Rows fresh(comp, L, L, {}, false, 3, 8);
  bpp_mixed_batch fmx = fresh.mx;
  fmx.transcript_label = (const uint8_t *)"harness";
  fmx.label_len = 7;
  IngestMixedPrelude fpre;
  if (!ingest_mixed_host_prelude(fmx, P, fpre) || fpre.h != L) return why = "harness: the live rows are not a batch for the device path", false;
  ModelBatch ref(fpre, P, 0xab);
  memset(ref.seeds.get(), 0, 32 * L);
  std::unique_ptr<uint8_t[]> info(new uint8_t[L]);
  uint32_t res[BPP_ING_RES_WORDS];
  const Ingest a = ingest_mixed_args(fmx, P, fpre, ref.rows.get(), ref.bytes.get(), ref.minvals.get(), ref.seeds.get(), info.get(), res);
  ingest_run_host<true>(a);
  bool foreign_any = false, finding_any = false;
  std::vector<uint8_t> stopped(L, 0);
  for (size_t k = 0; k < L; k++) {
    const uint8_t *p = fmx.proofs + k * fmx.proof_stride;
    const bool foreign = p[0] != t0;
    const bool finding = ingest_check_item(p, fresh.lens[k], fresh.ms[k], ingest_seed_present(a, k), false).msg != BPP_ING_OK;
    foreign_any = foreign_any || foreign;
    finding_any = finding_any || finding;
    stopped[k] = foreign || finding;
  }
  UploadPlan pl;
  if (foreign_any) {
    if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK) || rec.code || rec.msg || rec.index) return why = "a foreign first byte at a live row: FALLBACK alone expected", false;
  } else if (finding_any) {
    bool thrown = false;
    try {
      ingest_mixed_finish_plan(fmx, P, fpre, res, info.get(), pl);
    } catch (const ProofErr &e) {
      thrown = true;
      // the upload's index counts the live rows; the refill's is the slot
      if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FINDING) || rec.code != e.code || e.index >= L || rec.index != slots[e.index] ||
          e.msg != ingest_message(rec.msg)) {
        printf("   upload {%d, \"%s\", %u}  refill {%d, \"%s\", %u} flags %u\n", e.code, e.msg.c_str(), e.index, rec.code, ingest_message(rec.msg), rec.index, rec.flags);
        return why = "the record is not the finding the upload of the live rows throws, at its slot", false;
      }
    }
    if (!thrown) return why = "harness: a finding the upload does not throw", false;
  } else {
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "clean live rows: an empty record and a zero state expected", false;
    ingest_mixed_finish_plan(fmx, P, fpre, res, info.get(), pl);  // (must not throw)
    for (size_t k = 0; k < L; k++) {
      if (mb.desc[slots[k]].flags != pl.desc[k].flags) return why = "flags differ from the plan's", false;
      if (mb.defer[slots[k]] != pl.defer[k]) return why = "defer[] differs from the plan's", false;
    }
  }
  // ---- live slots, row by row (the two layouts differ in their offsets: the slot's here, the k-th row's there)
  for (size_t k = 0; k < L; k++) {
    const size_t i = slots[k];
    const IngestMixedRow &r = mb.rows[i], &q = ref.rows[k];
    if (r.proof_len != q.proof_len || r.m != q.m) return why = "harness: the contents do not keep the shape", false;
    if (stopped[k]) {
      if (!slot_is_sanitised(mb, i, t0, degree)) return false;
      continue;
    }
    if (memcmp(mb.bytes.get() + r.proof_off, ref.bytes.get() + q.proof_off, r.proof_len) ||
        memcmp(mb.bytes.get() + mb.proof_bytes + 32 * (size_t)r.minval_idx, ref.bytes.get() + ref.proof_bytes + 32 * (size_t)q.minval_idx, 32 * (size_t)r.m))
      return why = "a taken row is not byte-equal to the upload's", false;
    if (memcmp(&mb.minvals[r.minval_idx], &ref.minvals[q.minval_idx], 8 * (size_t)r.m)) return why = "a taken row's promises differ", false;
    if (memcmp(mb.seeds.get() + 32 * i, ref.seeds.get() + 32 * k, 32)) return why = "a taken row's nonce differs", false;
    if (mb.desc[i].flags != (uint32_t)(info[k] & BPP_ING_INFO_SEED)) return why = "a taken row's nonce flag differs", false;
    if (mb.defer[i] != (uint8_t)(degree | (info[k] & BPP_ING_INFO_PROMISE))) return why = "a taken row's deferred bits differ", false;
  }
  return true;
}

std::vector<std::pair<const char *, std::vector<uint8_t>>> masks_of(size_t N, const std::vector<Item> &shape) {
  std::vector<std::pair<const char *, std::vector<uint8_t>>> out;
  auto make = [&](const char *name, const std::function<int(size_t)> &f) {
    std::vector<uint8_t> mk(N);
    for (size_t i = 0; i < N; i++) mk[i] = (uint8_t)f(i);
    out.emplace_back(name, mk);
  };
  make("all dead", [](size_t) { return 0; });
  make("all live", [](size_t) { return 1; });
  make("only slot 0", [](size_t i) { return i == 0; });
  make("only slot N - 1", [=](size_t i) { return i == N - 1; });
  make("even slots", [](size_t i) { return i % 2 == 0; });
  make("odd slots", [](size_t i) { return i % 2 == 1; });
  make("a dead run in the middle", [=](size_t i) { return i < N / 3 || i >= N - (N + 2) / 3; });
  make("every m = 4 slot dead", [&](size_t i) { return shape[i].m != 4; });
  make("only the m = 4 slots", [&](size_t i) { return shape[i].m == 4; });
  make("byte values 2 and 255", [](size_t i) { return i % 3 == 0 ? 2 : (i % 3 == 1 ? 255 : 0); });
  return out;
}

// every form over one pair of shape and contents
bool hold_forms(const std::vector<Item> &shape, const std::vector<Item> &items, const ParamShape &P) {
  const size_t N = shape.size();
  if (!hold(shape, items, P, PLAIN, 0, {})) return printf("   plain, %zu slots\n", N), false;
  for (uint32_t c : {0u, 1u, (uint32_t)N / 2, (uint32_t)N - 1, (uint32_t)N, (uint32_t)N + 1, 0xffffffffu})
    if (!hold(shape, items, P, COUNT, c, {})) return printf("   count %u of %zu slots\n", c, N), false;
  for (const auto &mk : masks_of(N, shape))
    if (!hold(shape, items, P, MASK, 0, mk.second)) return printf("   under the mask \"%s\" of %zu slots\n", mk.first, N), false;
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

// the index of the first slot of factor m at or behind `from`
size_t slot_of(const std::vector<Item> &v, uint32_t m, size_t from = 0) {
  for (size_t i = from; i < v.size(); i++)
    if (v[i].m == m) return i;
  return 0;
}

}  // namespace

int main() {
  const ParamShape P8{8, 4, 1}, P8t2{8, 4, 2}, P64t3{64, 2, 3};
  {  // clean contents of another corpus: every form, several sizes, three parameter sets, a degree finding on every slot
    bool all = true;
    for (size_t n : {(size_t)1, (size_t)5, (size_t)9, (size_t)19}) {
      all = all && hold_forms(pattern(n, 8, 1), pattern(n, 8, 1), P8) && hold_forms(pattern(n, 8, 2), pattern(n, 8, 2), P8t2) &&
            hold_forms(pattern(n, 64, 3, 2), pattern(n, 64, 3, 2), P64t3) && hold_forms(pattern(n, 8, 1), pattern(n, 8, 1), P8t2);
    }
    EXPECT("clean_contents", all);
  }
  const size_t N = 15;
  const std::vector<Item> shape = pattern(N, 8, 1);
  const size_t first4 = slot_of(shape, 4), last2 = N - 1 - (shape[N - 1].m == 2 ? 0 : 1), short1 = slot_of(shape, 1, 8);
  {  // a non-canonical scalar: in an m = 4 row, at the first and the last slot, in a shortest row (maximal slack), each field
    bool all = true;
    for (size_t at : {first4, (size_t)0, N - 1, short1, slot_of(shape, 4, 3)})
      for (uint32_t field : {0u, 4u, 5u}) {
        std::vector<Item> items = pattern(N, 8, 1);
        group_order(&items[at].proof[1 + 32 * field]);
        all = all && hold_forms(shape, items, P8);
      }
    EXPECT("non_canonical_scalars", all);
  }
  {  // a nonce on an m = 2 slot and on an m = 4 slot; a promise above the capacity in an m = 4 row and in the last row
    std::vector<Item> nonce2 = pattern(N, 8, 1), nonce4 = pattern(N, 8, 1), prom = pattern(N, 8, 1), prom_last = pattern(N, 8, 1);
    nonce2[slot_of(shape, 2)].nonce = true;
    nonce4[slot_of(shape, 4, 3)].nonce = true;
    prom[first4].minv = {1, 2, 256, 4};
    prom[first4].present = {1};
    prom_last[N - 1].minv = {1ull << 32, 300};
    prom_last[N - 1].present = {1};
    EXPECT("nonce_on_aggregated_slots", hold_forms(shape, nonce2, P8) && hold_forms(shape, nonce4, P8));
    EXPECT("promises_above_the_capacity", hold_forms(shape, prom, P8) && hold_forms(shape, prom_last, P8) && hold_forms(shape, prom, P8t2));
  }
  {  // a foreign first byte at the first, a middle and the last slot, and in a shortest row; beside a finding of lower index
    bool all = true;
    for (size_t at : {(size_t)0, (size_t)7, N - 1, short1}) {
      std::vector<Item> items = pattern(N, 8, 1);
      items[at].proof[0] = 2;
      all = all && hold_forms(shape, items, P8);
      items[at].proof[0] = 0;
      group_order(&items[(at + 3) % N].proof[1]);
      all = all && hold_forms(shape, items, P8);
    }
    EXPECT("foreign_first_bytes", all);
  }
  {  // two findings: the lowest LIVE index wins
    std::vector<Item> items = pattern(N, 8, 1);
    group_order(&items[last2].proof[1 + 32 * 4]);
    group_order(&items[first4].proof[1 + 32 * 5]);
    items[slot_of(shape, 2)].nonce = true;
    EXPECT("several_findings", hold_forms(shape, items, P8));
  }
  {  // a shape with a slot whose proof does not fit its statement (an m = 2 proof under m = 1: rounds_bad at upload): the slot keeps ITS length
    std::vector<Item> odd = pattern(N, 8, 1);
    odd[3].proof = make_proof(1, 4);
    std::vector<Item> items = pattern(N, 8, 1);
    items[3].proof = make_proof(1, 4);
    group_order(&items[3].proof[1]);
    EXPECT("a_slot_of_unfitting_length", hold_forms(odd, odd, P8) && hold_forms(odd, items, P8));
  }
  {  // random mutations of contents under random forms
    bool all = true;
    for (int iter = 0; iter < 400 && all; iter++) {
      const bool t3 = (iter & 1) != 0;
      const ParamShape &P = t3 ? P64t3 : ((iter & 2) ? P8t2 : P8);
      const size_t n = 1 + rng() % 11;
      const std::vector<Item> sh = t3 ? pattern(n, 64, 3, 2) : pattern(n, 8, 1);
      std::vector<Item> items = t3 ? pattern(n, 64, 3, 2) : pattern(n, 8, 1);
      for (Item &it : items) {
        for (int k = 0; k < (int)(rng() % 3); k++)
          if (rng() % 4 == 0) it.proof[rng() % it.proof.size()] = (uint8_t)rng();
        if (rng() % 13 == 0) it.proof[0] = (uint8_t)(rng() % 8);
        it.nonce = rng() % 3 == 0 && (it.m == 1 || rng() % 4 == 0);
        it.minv = {rng() & 0x1ff, rng()};
        it.present = {(uint8_t)(rng() & 1), (uint8_t)(rng() % 9 == 0)};
      }
      std::vector<uint8_t> mk(n);
      for (auto &x : mk) x = (rng() & 1) ? (uint8_t)(1 + rng() % 255) : 0;
      const Form form = (Form)(rng() % 3);
      all = hold(sh, items, P, form, (uint32_t)(rng() % (n + 2)), mk);
    }
    EXPECT("mutations", all);
  }
  {  // packed is the mixed form whose row is arithmetic: a uniform batch (m = 2 everywhere, proof_stride > proof_len, m_stride = m)
     // refilled by its table and by arithmetic, plain, with a count c < N and under a mask, leaves the same slot bytes, defer, flags,
     // state word and record -- with a refused slot (a non-canonical scalar), with and without a foreign first byte, and with dead
     // slots whose sources are unreadable
    const size_t n = 9;
    auto uniform = [&] {
      std::vector<Item> v = pattern(n, 8, 1);
      for (size_t i = 0; i < n; i++) {
        v[i].m = 2;
        v[i].proof = make_proof(1, 4);
        v[i].nonce = false;
        v[i].commits.resize(64, (uint8_t)(i + 1));
      }
      return v;
    };
    const std::vector<Item> ushape = uniform();
    const Rows up(ushape, n, n, {}, false, 8, 2);
    IngestMixedPrelude pre;
    bool all = ingest_mixed_host_prelude(up.mx, P8, pre) && pre.h == n;
    for (bool foreign : {false, true})
      for (Form form : {PLAIN, COUNT, MASK}) {
        std::vector<Item> items = uniform();
        group_order(&items[4].proof[1]);
        items[0].minv = {1, 256};  // (a promise above the capacity, taken)
        items[0].present = {1};
        if (foreign) items[2].proof[0] = 2;
        const uint32_t count = 5;
        std::vector<uint8_t> mask(n), dead(n, 0);
        for (size_t i = 0; i < n; i++) {
          mask[i] = i % 2 == 0 ? (uint8_t)(1 + i) : 0;
          dead[i] = form == MASK ? !mask[i] : (form == COUNT ? i >= count : 0);
        }
        size_t end = n;
        while (end && dead[end - 1]) end--;
        const Rows src(items, end, n, dead, true, 16, 2);
        bpp_packed_batch pk;
        memset(&pk, 0, sizeof(pk));
        pk.n_items = n;
        pk.proofs = src.mx.proofs;
        pk.proof_len = src.lens[0];
        pk.proof_stride = src.mx.proof_stride;
        pk.m = 2;
        pk.commitments32 = src.mx.commitments32;
        pk.min_values = src.mx.min_values;
        pk.min_present = src.mx.min_present;
        pk.seed_nonces32 = src.mx.seed_nonces32;
        pk.seed_present = src.mx.seed_present;
        std::unique_ptr<uint32_t> count_word(new uint32_t(count));
        const uint32_t *cw = form == COUNT ? count_word.get() : nullptr;
        const uint8_t *mw = form == MASK ? mask.data() : nullptr;
        ModelBatch rows(pre, P8, 0xcd), arith(pre, P8, 0xcd);
        rows.refill(src.mx, P8, 1, cw, mw);
        arith.refill_packed(pk, P8, 1, cw, mw);
        checked++;
        bool same = pk.proof_stride > pk.proof_len && memcmp(rows.bytes.get(), arith.bytes.get(), rows.bytes_total + BPP_BYTES_SLACK) == 0 &&
                    memcmp(rows.minvals.get(), arith.minvals.get(), (rows.sum_m + 1) * 8) == 0 && memcmp(rows.seeds.get(), arith.seeds.get(), 32 * n + 1) == 0 &&
                    memcmp(rows.defer.get(), arith.defer.get(), n + 1) == 0 && memcmp(rows.mask.get(), arith.mask.get(), n + 1) == 0 &&
                    memcmp(rows.status.get(), arith.status.get(), (n + 1) * 4) == 0 && memcmp(rows.status0.get(), arith.status0.get(), (n + 1) * 4) == 0 &&
                    memcmp(rows.masks.get(), arith.masks.get(), (n * (size_t)P8.t * 8 + 1) * 4) == 0 && rows.state == arith.state && rows.live == arith.live &&
                    memcmp(&rows.record, &arith.record, sizeof(rows.record)) == 0 && !arith.red[0] && !arith.red[1];
        for (size_t i = 0; i < n && same; i++) same = rows.desc[i].flags == arith.desc[i].flags;
        // and the outcome is the one the case is about: the fall-back before the finding at slot 4, slot 4 and every dead slot sanitised
        const uint32_t want = BPP_REFILL_WRITTEN | (foreign ? BPP_REFILL_FALLBACK : BPP_REFILL_FINDING);
        same = same && arith.record.flags == want && (foreign || (arith.record.index == 4 && arith.record.msg == BPP_ING_PARSING)) &&
               arith.defer[0] == BPP_DEFER_PROMISE && slot_is_sanitised(arith, 4, 1, 0);
        for (size_t i = 0; i < n && same; i++)
          if (dead[i]) same = slot_is_sanitised(arith, i, 1, 0);
        if (!same) printf("   form %d, foreign %d\n", (int)form, (int)foreign);
        all = all && same;
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
