// Sanitizer harness (CPU test suite only): a refill under a per-item LIVE MASK (bpp_batch_refill_enqueue_live).
//
// 1. The one-lane host model of the refill kernels (refill.h: refill_run_host with Refill::mask) is held to what a fresh device
//    upload makes of the LIVE ITEMS ALONE, in slot order -- ingest_run_host + ingest_finish_plan of ingest.h on the compacted arrays
//    -- over the corpus of hosttest_refill_count.cpp's kinds, under the masks: all dead, all live, one live item at 0 / at N - 1,
//    alternating (both phases), a dead run in the middle, and the byte values 2 and 255 as "live"; findings and foreign first bytes
//    lie at live and at dead items:
//      record and state   what the upload of the live items throws, its index k mapped to the slot of the k-th live item; FALLBACK
//                         for a foreign first byte at a live item; clean otherwise, whatever lies at dead items
//      live slots         the upload's bytes of the k-th item, or the sanitised slot of a stopped item
//      dead slots         byte for byte the sanitised slot: t0 and zeros, zero commitments, no promise, no nonce, no flag, the
//                         shape's degree bit, cleared status words, wiped mask rows
//      dead sources       are never read: the arrays the model is handed END behind the last live item (a read beyond is an ASan
//                         report) and hold a poison pattern at every dead item; a second run over full-length arrays and other old
//                         contents must leave the same bytes, none of them the pattern
//      the batch's mask   the normalised bytes, 0 or 1; the count word is not touched
// 2. The live routines of verdict.h on a LiveView with a mask, plus verdict_finish, are held to check_deferred + check_chunk_errors
//    (upload_host.h) on the COMPACTED groups -- an empty group between two live ones among them -- with the reference's index k
//    mapped to the slot offset of the group's k-th live item.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_refill_live_host.py runs.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "refill.h"

using namespace bpp;

namespace {

std::mt19937_64 rng(20261022);
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
  // the items at `slots`, in that order, as a batch of their own: what the reference's caller would hand a fresh upload
  Source compacted(const std::vector<size_t> &slots) const {
    std::vector<std::vector<uint8_t>> it;
    for (size_t s : slots) it.push_back(items[s]);
    Source c(it, m, stride - len);
    c.has_promises = has_promises;
    c.has_seeds = has_seeds;
    c.has_seed_present = has_seed_present;
    for (size_t k = 0; k < slots.size(); k++) {
      const size_t s = slots[k];
      memcpy(&c.commits[32 * k * m], &commits[32 * s * m], 32 * (size_t)m);
      if (has_promises) {
        if (k == 0) c.minv.resize(slots.size() * m), c.present.resize(slots.size() * m);
        for (uint32_t j = 0; j < m; j++) c.minv[k * m + j] = minv[s * m + j], c.present[k * m + j] = present[s * m + j];
      }
      if (has_seeds) {
        if (k == 0) c.seeds.resize(32 * slots.size());
        memcpy(&c.seeds[32 * k], &seeds[32 * s], 32);
        if (has_seed_present) {
          if (k == 0) c.seed_present.resize(slots.size());
          c.seed_present[k] = seed_present[s];
        }
      }
    }
    return c;
  }
};

// exact-size heap copies of the first `keep` items of a source, described as a packed batch of `claim` items; items i with
// dead[i] != 0 hold the poison pattern in every array (dead empty: none).  keep < claim is what a refill under a mask whose last
// live item is keep - 1 may be handed: the arrays END there.
struct Arrays {
  std::unique_ptr<uint8_t[]> proofs, commits, present, seeds, seed_present;
  std::unique_ptr<uint64_t[]> minv;
  bpp_packed_batch pk;

  static void poison(uint8_t *p, size_t k) {
    for (size_t i = 0; i < k; i++) p[i] = POISON[i % 8];
  }
  Arrays(const Source &s, size_t keep, size_t claim, const std::vector<uint8_t> &dead) {
    const size_t n = keep, m = s.m;
    const size_t extent = n ? (n - 1) * s.stride + s.len : 0;
    auto is_dead = [&](size_t i) { return !dead.empty() && dead[i] != 0; };
    proofs.reset(new uint8_t[extent ? extent : 1]);
    memset(proofs.get(), 0xee, extent);
    for (size_t i = 0; i < n; i++) {
      if (is_dead(i)) poison(proofs.get() + i * s.stride, s.len);
      else memcpy(proofs.get() + i * s.stride, s.items[i].data(), s.len);
    }
    commits.reset(new uint8_t[32 * n * m + 1]);
    memcpy(commits.get(), s.commits.data(), 32 * n * m);
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
      pk.min_values = minv.get();
      pk.min_present = present.get();
    }
    if (s.has_seeds) {
      seeds.reset(new uint8_t[32 * n + 1]);
      memcpy(seeds.get(), s.seeds.data(), 32 * n);
      pk.seed_nonces32 = seeds.get();
      if (s.has_seed_present) {
        seed_present.reset(new uint8_t[n + 1]);
        memcpy(seed_present.get(), s.seed_present.data(), n);
        pk.seed_present = seed_present.get();
      }
    }
    for (size_t i = 0; i < n; i++) {
      if (!is_dead(i)) continue;
      poison(commits.get() + 32 * i * m, 32 * m);
      if (s.has_promises) {
        poison((uint8_t *)(minv.get() + i * m), 8 * m);
        poison(present.get() + i * m, m);
      }
      if (s.has_seeds) poison(seeds.get() + 32 * i, 32);
      if (s.has_seed_present) seed_present[i] = POISON[i % 8];
    }
  }
};

// what the engine holds of a resident batch of N items of pk's shape: exact sizes, every byte a refill must write starts as `fill`
struct ModelBatch {
  size_t n, len, bytes_total;
  uint32_t m, t;
  std::unique_ptr<uint8_t[]> bytes, seeds, defer, mask;
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
    mask.reset(new uint8_t[n + 1]);
    memset(mask.get(), fill, n + 1);
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
  // mask_bytes: exactly as many bytes as the caller's mask holds (null: no mask)
  void refill(const bpp_packed_batch &pk, const ParamShape &P, uint8_t t0, const uint8_t *mask_bytes) {
    const Refill r = refill_args(pk, P, t0, bytes.get(), minvals.get(), seeds.get(), defer.get(), desc.get(), status0.get(),
                                       status.get(), masks.get(), red, nullptr, mask_bytes, mask.get());
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

// one refill under `mask` (N bytes, any non-zero value live) of a model batch of src's shape, held to the fresh device upload of the
// live items alone
bool hold_mask(const Source &src, const ParamShape &P, uint8_t t0, const std::vector<uint8_t> &mask, bool shape_exists) {
  checked++;
  const size_t N = src.n, len = src.len;
  const uint32_t m = src.m;
  std::vector<size_t> slots;  // the live slots in slot order
  std::vector<uint8_t> dead(N, 0);
  for (size_t i = 0; i < N; i++) {
    if (mask[i]) slots.push_back(i);
    else dead[i] = 1;
  }
  const size_t L = slots.size(), end = L ? slots.back() + 1 : 0;
  // what the model is handed: arrays that end behind the last live item with every dead item poisoned, and, in a second run,
  // full-length arrays over other old contents -- both must leave the same bytes.  The mask itself is exactly N bytes.
  const Arrays cut(src, end, N, dead), poisoned(src, N, N, dead);
  std::unique_ptr<uint8_t[]> mask_exact(new uint8_t[N]);
  memcpy(mask_exact.get(), mask.data(), N);
  ModelBatch mb(N, cut.pk, P, 0xcd), mp(N, poisoned.pk, P, 0x37);
  mb.refill(cut.pk, P, t0, mask_exact.get());
  mp.refill(poisoned.pk, P, t0, mask_exact.get());
  const uint8_t degree = t0 != P.t ? BPP_DEFER_DEGREE : 0;
  const bool nonces = src.has_seeds;
  if (mb.live != 0xdddddddd || mp.live != 0xdddddddd) return why = "a mask refill wrote the count word", false;
  for (size_t i = 0; i < N; i++)
    if (mb.mask[i] != (mask[i] ? 1 : 0) || mp.mask[i] != mb.mask[i]) return why = "the batch's mask is not the normalised mask", false;
  if (memcmp(mb.bytes.get(), mp.bytes.get(), mb.bytes_total + BPP_BYTES_SLACK) || memcmp(mb.minvals.get(), mp.minvals.get(), N * m * 8) ||
      (nonces && memcmp(mb.seeds.get(), mp.seeds.get(), 32 * N)) || memcmp(mb.defer.get(), mp.defer.get(), N) ||
      memcmp(&mb.record, &mp.record, sizeof(mb.record)) || mb.state != mp.state)
    return why = "the outputs depend on the dead items' sources or on the old contents", false;
  if (has_poison(mp.bytes.get(), mp.bytes_total) || has_poison((const uint8_t *)mp.minvals.get(), N * m * 8) || (nonces && has_poison(mp.seeds.get(), 32 * N)))
    return why = "bytes of a dead item's source appear in the batch", false;
  for (size_t i = 0; i < N; i++)
    if (mp.desc[i].flags > 1) return why = "a dead item's source reached the flags", false;
  // (guard bytes behind every array: nothing is written past item N - 1)
  if (mb.defer[N] != 0xcd || mb.mask[N] != 0xcd || mb.status[N] != 0xcdcdcdcdu || mb.status0[N] != 0xcdcdcdcdu ||
      mb.masks[N * (size_t)mb.t * 8] != 0xcdcdcdcdu || mb.minvals[N * m] != 0xcdcdcdcdcdcdcdcdull || mb.seeds[32 * N] != 0xcd)
    return why = "a write past the batch's last item", false;
  if (mb.red[0] || mb.red[1]) return why = "the reduction words are not left clear", false;
  const bpp_device_refill &rec = mb.record;
  if (mb.state != refill_state_make(rec.flags, rec.code, rec.msg, rec.index)) return why = "state word is not the record's", false;
  if (rec.flags & BPP_REFILL_COUNT) return why = "a mask refill raised BPP_REFILL_COUNT", false;
  for (size_t i = 0; i < N; i++) {
    if (mb.status0[i] || mb.status[i]) return why = "status words not cleared", false;
    if (!all_zero((const uint8_t *)(mb.masks.get() + i * (size_t)mb.t * 8), (size_t)mb.t * 32)) return why = "mask rows not wiped", false;
  }
  if (!all_zero(mb.bytes.get() + mb.bytes_total, BPP_BYTES_SLACK)) return why = "slack not zero", false;
  // ---- dead slots
  for (size_t i = 0; i < N; i++)
    if (dead[i] && !slot_is_sanitised(mb, i, t0, degree, nonces)) return false;
  // ---- the view over the batch's mask
  const LiveView view{nullptr, mb.mask.get()};
  if (verdict_group_live(view, 0, (uint32_t)N) != L) return why = "verdict_group_live over the batch's mask", false;
  for (size_t i = 0; i < N; i++)
    if (verdict_item_live(view, (uint32_t)i) != (mask[i] != 0)) return why = "verdict_item_live over the batch's mask", false;
  if (L == 0) {
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "all dead: an empty record and a zero state expected", false;
    return true;
  }
  // ---- the fresh upload's kernel on the live items alone, into buffers of its own
  const Source comp = src.compacted(slots);
  const Arrays first(comp, L, L, {});
  ModelBatch ref(L, first.pk, P, 0xab);
  std::unique_ptr<uint8_t[]> info(new uint8_t[L]);
  uint32_t res[BPP_ING_RES_WORDS];
  bpp_packed_batch plain = first.pk;
  plain.transcript_label = (const uint8_t *)"harness";
  plain.label_len = 7;
  const Ingest a = ingest_args(plain, P, ref.bytes.get(), ref.minvals.get(), ref.seeds.get(), info.get(), res);
  ingest_run_host<false>(a);
  bool foreign_any = false, finding_any = false;
  std::vector<uint8_t> stopped(L, 0);
  for (size_t k = 0; k < L; k++) {
    const uint8_t *p = plain.proofs + k * plain.proof_stride;
    const bool foreign = p[0] != t0;
    const bool finding = ingest_check_item(p, len, m, ingest_seed_present(a, k), false).msg != BPP_ING_OK;
    foreign_any = foreign_any || foreign;
    finding_any = finding_any || finding;
    stopped[k] = foreign || finding;
  }
  if (foreign_any) {
    if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FALLBACK) || rec.code || rec.msg || rec.index) return why = "a foreign first byte at a live item: FALLBACK alone expected", false;
  } else if (finding_any) {
    bool thrown = false;
    try {
      UploadPlan pl;
      ingest_finish_plan(plain, P, res, info.get(), pl);
    } catch (const ProofErr &e) {
      thrown = true;
      // the upload's index counts the live items; the refill's is the slot
      if (rec.flags != (BPP_REFILL_WRITTEN | BPP_REFILL_FINDING) || rec.code != e.code || e.index >= L || rec.index != slots[e.index] ||
          e.msg != ingest_message(rec.msg)) {
        printf("   upload {%d, \"%s\", %u}  refill {%d, \"%s\", %u} flags %u\n", e.code, e.msg.c_str(), e.index, rec.code, ingest_message(rec.msg), rec.index, rec.flags);
        return why = "the record is not the finding the upload of the live items throws, at its slot", false;
      }
    }
    if (!thrown) return why = "harness: a finding the upload does not throw", false;
  } else {
    // nothing at live items, whatever lies at dead ones
    if (rec.flags != BPP_REFILL_WRITTEN || rec.code || rec.msg || rec.index || mb.state != 0) return why = "clean live items: an empty record and a zero state expected", false;
    UploadPlan pl;
    ingest_finish_plan(plain, P, res, info.get(), pl);  // (must not throw)
    for (size_t k = 0; k < L; k++) {
      if (mb.desc[slots[k]].flags != pl.desc[k].flags) return why = "flags differ from the plan's", false;
      if (mb.defer[slots[k]] != pl.defer[k]) return why = "defer[] differs from the plan's", false;
    }
  }
  // ---- live slots, item by item (the two layouts differ in their item counts: N here, L there)
  for (size_t k = 0; k < L; k++) {
    const size_t i = slots[k];
    const uint8_t *slot = mb.bytes.get() + i * len, *cm = mb.bytes.get() + N * len + 32 * i * m;
    if ((mb.defer[i] & BPP_DEFER_DEGREE) != degree) return why = "degree bit is not the shape's", false;
    if (stopped[k]) {
      if (!slot_is_sanitised(mb, i, t0, degree, nonces)) return false;
      if (shape_exists && ingest_check_item(slot, len, m, false, false).msg != BPP_ING_OK) return why = "the sanitised slot does not pass ingest_check_item", false;
    } else {
      if (memcmp(slot, ref.bytes.get() + k * len, len) || memcmp(cm, ref.bytes.get() + L * len + 32 * k * m, 32 * (size_t)m))
        return why = "a taken item is not byte-equal to the upload's", false;
      if (memcmp(&mb.minvals[i * m], &ref.minvals[k * m], 8 * (size_t)m)) return why = "a taken item's promises differ", false;
      if (nonces && memcmp(mb.seeds.get() + 32 * i, ref.seeds.get() + 32 * k, 32)) return why = "a taken item's nonce differs", false;
      if (mb.desc[i].flags != (uint32_t)(info[k] & BPP_ING_INFO_SEED)) return why = "a taken item's nonce flag differs", false;
      if ((mb.defer[i] & BPP_DEFER_PROMISE) != (info[k] & BPP_ING_INFO_PROMISE)) return why = "a taken item's promise bit differs", false;
    }
  }
  return true;
}

// the masks of the issue over a batch of N items
std::vector<std::pair<const char *, std::vector<uint8_t>>> masks_of(size_t N) {
  std::vector<std::pair<const char *, std::vector<uint8_t>>> out;
  auto make = [&](const char *name, auto f) {
    std::vector<uint8_t> mk(N);
    for (size_t i = 0; i < N; i++) mk[i] = (uint8_t)f(i);
    out.emplace_back(name, mk);
  };
  make("all dead", [](size_t) { return 0; });
  make("all live", [](size_t) { return 1; });
  make("only item 0", [](size_t i) { return i == 0; });
  make("only item N - 1", [=](size_t i) { return i == N - 1; });
  make("even items", [](size_t i) { return i % 2 == 0; });
  make("odd items", [](size_t i) { return i % 2 == 1; });
  make("a dead run in the middle", [=](size_t i) { return i < N / 3 || i >= N - (N + 2) / 3; });
  make("a live run in the middle", [=](size_t i) { return !(i < N / 3 || i >= N - (N + 2) / 3); });
  make("byte values 2 and 255", [](size_t i) { return i % 3 == 0 ? 2 : (i % 3 == 1 ? 255 : 0); });
  make("byte value 255 everywhere", [](size_t) { return 255; });
  return out;
}

// every mask of the issue over one source; also: no mask at all equals the all-live mask in everything but the batch's mask
bool hold_masks(const Source &src, const ParamShape &P, uint8_t t0, bool shape_exists = true) {
  const size_t N = src.n;
  for (const auto &mk : masks_of(N))
    if (!hold_mask(src, P, t0, mk.second, shape_exists)) {
      printf("   under the mask \"%s\" of %zu items\n", mk.first, N);
      return false;
    }
  const Arrays all(src, N, N, {});
  ModelBatch a(N, all.pk, P, 0xcd), b(N, all.pk, P, 0xcd);
  const std::vector<uint8_t> ones(N, 1);
  a.refill(all.pk, P, t0, nullptr);
  b.refill(all.pk, P, t0, ones.data());
  if (memcmp(a.bytes.get(), b.bytes.get(), a.bytes_total) || memcmp(&a.record, &b.record, 16) || a.state != b.state || a.live != N || b.live != 0xdddddddd ||
      memcmp(a.defer.get(), b.defer.get(), N) || memcmp(a.minvals.get(), b.minvals.get(), 8 * N * src.m))
    return why = "no mask is not the all-live mask", false;
  for (size_t i = 0; i <= N; i++)
    if (a.mask[i] != 0xcd) return why = "a refill without a mask wrote the batch's mask", false;
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

// ---- 2. the live routines and verdict_finish against the host rules on the compacted groups
struct Want {
  int code = BPP_OK, tier = BPP_TIER_NONE;
  uint32_t index = 0;
  std::string msg;
};
// the group as the verify() call of the fresh upload sees it: its live proofs alone, in slot order, counted from the first of them
Want host_finding(const std::vector<uint32_t> &status, const std::vector<uint8_t> &rounds_bad, const std::vector<uint8_t> &defer,
                  const std::vector<uint32_t> &slots) {
  Want w;
  std::vector<uint32_t> st;
  std::vector<uint8_t> rb, df;
  for (uint32_t p : slots) {
    st.push_back(status[p]);
    rb.push_back(rounds_bad[p]);
    df.push_back(defer[p]);
  }
  try {
    check_deferred(df, 0, (uint32_t)slots.size());
    check_chunk_errors(st.data(), rb.data(), 0, (uint32_t)slots.size());
  } catch (const ProofErr &e) {
    w.code = e.code;
    w.tier = e.tier;
    w.index = e.index;
    w.msg = e.msg;
  }
  return w;
}

void compacted_groups() {
  std::mt19937_64 r(12);
  const uint8_t rb_of[3] = {0, BPP_ERR_INVALID_LENGTH, BPP_ERR_SIZE_OVERFLOW};
  bool ok = true;
  long empties = 0, empty_between = 0, holes = 0, findings = 0, moved = 0;
  for (int it = 0; it < 4000 && ok; it++) {
    const uint32_t n = 3 + (uint32_t)(r() % 700), G = 1 + (uint32_t)(r() % (n < 7 ? n - 1 : 6));
    std::vector<uint32_t> bounds{0, n};
    while (bounds.size() < G + 1) {
      const uint32_t b = 1 + (uint32_t)(r() % (n - 1));
      bool dup = false;
      for (uint32_t x : bounds) dup = dup || x == b;
      if (!dup) bounds.push_back(b);
    }
    std::sort(bounds.begin(), bounds.end());
    // the mask: a density per batch, whole groups killed now and then (an empty group between two live ones), byte values beyond 1
    std::unique_ptr<uint8_t[]> mask(new uint8_t[n]);
    const uint32_t density = (uint32_t)(r() % 5);  // of 4
    for (uint32_t p = 0; p < n; p++) mask[p] = (r() % 4) < density ? (uint8_t)(1 + r() % 255) : 0;
    std::vector<uint8_t> killed(G, 0);
    for (uint32_t g = 0; g < G; g++)
      if (r() % 3 == 0) {
        killed[g] = 1;
        for (uint32_t p = bounds[g]; p < bounds[g + 1]; p++) mask[p] = 0;
      } else if (r() % 2) {
        mask[bounds[g] + r() % (bounds[g + 1] - bounds[g])] = 1;
      }
    const LiveView view{nullptr, mask.get()};
    std::vector<uint32_t> status(n, 0);
    std::vector<uint8_t> rounds_bad(n, 0), defer(n, 0);
    // findings at live and at dead slots; every dead slot carries the PASS-1 finding its sanitised bytes raise
    for (uint32_t f = 0, k = (uint32_t)(r() % 6); f < k; f++) {
      const uint32_t p = (uint32_t)(r() % n);
      switch (r() % 3) {
        case 0: status[p] |= 1u << (r() % 3); break;
        case 1: rounds_bad[p] = rb_of[1 + r() % 2]; break;
        default: defer[p] |= (uint8_t)(1u << (r() % 2)); break;
      }
    }
    for (uint32_t p = 0; p < n; p++)
      if (!mask[p]) status[p] |= BPP_ST_TRANSCRIPT_FAIL;
    std::vector<uint32_t> lens(G);
    for (uint32_t g = 0; g < G && ok; g++) {
      const uint32_t p0 = bounds[g], p1 = bounds[g + 1];
      std::vector<uint32_t> slots;
      uint64_t key = BPP_VERDICT_KEY_NONE;
      for (uint32_t p = p0; p < p1; p++) {
        ok = ok && verdict_item_live(view, p) == (mask[p] != 0);
        if (!verdict_item_live(view, p)) continue;
        slots.push_back(p);
        key = verdict_min(key, verdict_key(defer[p], status[p], rounds_bad[p], p - p0));  // what k_verdict_scan reduces
      }
      const uint32_t len = verdict_group_live(view, p0, p1);
      lens[g] = len;
      ok = ok && len == slots.size();
      empties += len == 0;
      holes += len != 0 && len != p1 - p0;
      const Want found = len ? host_finding(status, rounds_bad, defer, slots) : Want();
      findings += found.tier != BPP_TIER_NONE;
      for (int want_msm = 0; want_msm < 2 && ok; want_msm++)
        for (int action = 0; action < 3; action++)
          for (int ident = 0; ident < 2; ident++)
            for (int zero = 0; zero < 2; zero++) {
              const bpp_device_verdict v = verdict_finish(key, want_msm != 0, action, ident != 0, zero != 0, 0ull, len);
              if (len == 0) {  // nothing is claimed, not even the redraw
                ok = ok && v.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_EMPTY) && v.code == BPP_OK && v.tier == BPP_TIER_NONE && v.index == 0;
                continue;
              }
              if (zero && want_msm && action != BPP_RECOVER_ONLY) {
                ok = ok && v.flags == (BPP_VERDICT_WRITTEN | BPP_VERDICT_REDRAW) && v.code == BPP_OK && v.tier == BPP_TIER_NONE;
                continue;
              }
              Want w = found;
              if (w.tier != BPP_TIER_NONE) {  // the reference's k-th live item lies at slot offset slots[k] - p0
                ok = ok && w.index < len;
                if (!ok) break;
                moved += slots[w.index] - p0 != w.index;
                w.index = slots[w.index] - p0;
              } else if (want_msm && action != BPP_RECOVER_ONLY && !ident) {
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
    for (uint32_t g = 1; g + 1 < G; g++) empty_between += lens[g] == 0 && lens[g - 1] != 0 && lens[g + 1] != 0;
    // a view with neither form: every item is live; a view with a count word is the count form
    const LiveView none{nullptr, nullptr};
    const uint32_t c = (uint32_t)(r() % (n + 1));
    const LiveView counted{&c, nullptr};
    ok = ok && verdict_group_live(none, bounds[0], bounds[1]) == bounds[1] && verdict_item_live(none, n - 1);
    ok = ok && verdict_group_live(counted, bounds[0], bounds[1]) == verdict_group_live(bounds[0], bounds[1], c) &&
         verdict_item_live(counted, n - 1) == verdict_item_live(n - 1, c);
  }
  why = "the live routines and verdict_finish against the host rules on the compacted groups";
  EXPECT("compacted_groups", ok && empties > 100 && empty_between > 100 && holes > 100 && findings > 100 && moved > 100);
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
          all = hold_masks(Source(items, 1, f), P, (uint8_t)t);
        }
    EXPECT(t == 1 ? "edge_scalars_t1" : "edge_scalars_t3", all);
  }
  {  // every truncation of a valid proof as the contents of a batch of that length
    const std::vector<uint8_t> full = make_proof(1, 6);
    bool all = true;
    for (size_t len = 1; len <= full.size() && all; len += (len < 40 || len + 40 > full.size()) ? 1 : 13) {
      std::vector<uint8_t> cut(full.begin(), full.begin() + len);
      all = hold_masks(Source({cut, cut, cut, cut}, 1, 5), P64, 1, len == full.size());
    }
    EXPECT("truncations_t1", all);
  }
  {  // two findings, live or dead by the mask; a nonce with m = 2 in front of both
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 7; i++) items.push_back(make_proof(1, 7));
    edge_scalar(0, &items[5][1 + 32 * 4]);
    edge_scalar(3, &items[0][1 + 32 * 5]);
    Source c(items, 2, 3), d(items, 2);
    std::vector<uint8_t> only6{0, 0, 0, 0, 0, 0, 1};
    d.nonces(&only6);
    EXPECT("two_findings", hold_masks(c, P64, 1) && hold_masks(d, P64, 1));
  }
  {  // a foreign first byte at the first, a middle and the last index; beside a finding elsewhere
    bool all = true;
    for (size_t at : {0u, 3u, 6u}) {
      std::vector<std::vector<uint8_t>> items(7, make_proof(1, 6));
      items[at] = make_proof(3, 5);
      all = all && hold_masks(Source(items, 1, 7), P64, 1);
      items[at] = items[(at + 1) % 7];
      items[at][0] = 0;
      edge_scalar(0, &items[6 - at][1]);
      Source both(items, 1, 1);
      both.nonces(nullptr);
      all = all && hold_masks(both, P64, 1);
    }
    EXPECT("foreign_first_byte", all);
  }
  {  // nonces: at m = 2 on every item (a finding at the first live item), on the last item alone; at m = 1 on every other item
    std::vector<std::vector<uint8_t>> items;
    for (int i = 0; i < 6; i++) items.push_back(make_proof(1, 7));
    Source every(items, 2), last(items, 2), alt(items, 1, 3), none(items, 1);
    std::vector<uint8_t> only5{0, 0, 0, 0, 0, 1}, other{1, 0}, zero{0};
    every.nonces(nullptr);
    last.nonces(&only5);
    alt.nonces(&other);
    alt.promises({5, 0, 77}, {1, 0, 1});
    none.nonces(&zero);
    EXPECT("nonces", hold_masks(every, P64, 1) && hold_masks(last, P64, 1) && hold_masks(alt, P64, 1) && hold_masks(none, P64, 1));
  }
  {  // promises at the capacity, and parameters of t = 2 over t = 1 proofs: the degree bit on every slot, dead ones included
    std::vector<std::vector<uint8_t>> items, items2;
    for (int i = 0; i < 6; i++) items.push_back(make_proof(1, 3));
    for (int i = 0; i < 5; i++) items2.push_back(make_proof(1, 4));
    Source over(items, 1), deg(items2, 1);
    over.promises({255, 255, 256, 255, 256, 256}, {1});
    deg.promises({0, 1ull << 16, 0, 0, 1ull << 16}, {1});
    EXPECT("promises_and_degree", hold_masks(over, P8, 1) && hold_masks(deg, P16t2, 1));
  }
  {  // random mutations of content under random masks, batches of six
    bool all = true;
    for (int iter = 0; iter < 600 && all; iter++) {
      const uint32_t t = 1 + (uint32_t)(rng() % 3), r = 1 + (uint32_t)(rng() % 8), m = 1u << (rng() % 3);
      const size_t len = 1 + 32 * (size_t)(t + 5 + 2 * r);
      std::vector<std::vector<uint8_t>> items;
      for (int i = 0; i < 6; i++) {
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
      std::vector<uint8_t> mk(6);
      for (auto &x : mk) x = (rng() & 1) ? (uint8_t)(1 + rng() % 255) : 0;
      all = hold_mask(c, (rng() & 1) ? P64t3 : P16t2, (uint8_t)t, mk, true);
    }
    EXPECT("mutations", all);
  }
  compacted_groups();
  printf("%d comparisons\n", checked);
  if (fails) {
    printf("%d case(s) failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
