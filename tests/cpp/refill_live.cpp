// A compiled caller of bpp_batch_refill_enqueue_live (include/bpp.h) through Engine::batch_refill_enqueue_live of include/bpp.hpp,
// with arrays it allocated itself with hipMalloc -- no torch, no ctypes declarations that could hide a wrong prototype.  Six proofs
// (n = 64, m = 1, t = 1) are committed and proved through bpp.h and uploaded from device memory; the batch is then refilled under the
// mask {1, 0, 0, 0, 255, 2} from arrays whose dead items 1 and 3 hold a proof that does not verify and a non-canonical scalar, and
// verified in chunks of two proofs: group 0 runs over slot 0 alone, group 1 is empty between two live groups, group 2 is whole.  The
// reference is a fresh upload of items 0, 4 and 5 alone with the boundaries [0, 1, 3].  The program prints the records and holds the
// weights of the live slots to the reference's; tests/test_gpu_cpp_refill_live.py reads them.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bpp.hpp"

using namespace bpp_host;

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static uint64_t splitmix(uint64_t &s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

template <typename T>
static T *to_device(const std::vector<T> &v) {
  void *d = nullptr;
  CHECK(hipMalloc(&d, v.size() * sizeof(T)) == hipSuccess);
  CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  return static_cast<T *>(d);
}

// the items at `slots` of an array of `item` elements per item
template <typename T>
static std::vector<T> gather(const std::vector<T> &v, size_t item, const std::vector<size_t> &slots) {
  std::vector<T> out;
  for (size_t s : slots) out.insert(out.end(), v.begin() + s * item, v.begin() + (s + 1) * item);
  return out;
}

int main() {
  Engine eng(0);
  bpp_ctx *ctx = eng.ctx();
  auto params = RangeParameters::init(eng, 64, 1, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  const std::string label = "refill";
  const size_t N = 6, G = 3, rounds = 6, plen = 1 + 32 * (1 + 5 + 2 * rounds);
  uint64_t s = 20261022;
  std::vector<uint64_t> values(N), min_values(N);
  std::vector<uint8_t> blindings(32 * N), min_present(N, 1), commitments(32 * N), ext(N * 32 * (rounds + 3)), proofs(N * plen);
  for (size_t i = 0; i < N; i++) {
    values[i] = splitmix(s) >> 1;
    min_values[i] = values[i] / 3;
    for (int k = 0; k < 31; k++) blindings[32 * i + k] = (uint8_t)splitmix(s) | (k == 0);
  }
  for (auto &x : ext) x = (uint8_t)splitmix(s);
  char err[256] = {0};
  CHECK(bpp_pedersen_commit(ctx, params->handle(), values.data(), blindings.data(), 1, N, commitments.data()) == BPP_OK);
  std::vector<bpp_prove_item> items(N);
  for (size_t i = 0; i < N; i++) {
    memset(&items[i], 0, sizeof(items[i]));
    items[i].values = &values[i];
    items[i].blindings32 = &blindings[32 * i];
    items[i].commitments32 = &commitments[32 * i];
    items[i].m = 1;
    items[i].min_values = &min_values[i];
    items[i].min_present = &min_present[i];
    items[i].transcript_label = (const uint8_t *)label.data();
    items[i].label_len = label.size();
    items[i].rng_bytes = &ext[i * 32 * (rounds + 3)];
    items[i].rng_len = 32 * (rounds + 3);
  }
  size_t got_len = 0;
  CHECK(bpp_prove_batch(ctx, params->handle(), items.data(), N, proofs.data(), plen, &got_len, err, sizeof(err)) == BPP_OK && got_len == plen);
  // at dead slots: a proof that does not verify and a non-canonical scalar -- neither is looked at under the mask
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  std::vector<uint8_t> holes_bad = proofs;
  holes_bad[1 * plen + 1 + 32 * 4] ^= 1;
  memcpy(&holes_bad[3 * plen + 1 + 32 * 5], L, 32);

  bpp_packed_batch dev;
  memset(&dev, 0, sizeof(dev));
  dev.n_items = N;
  dev.proofs = to_device(proofs);
  dev.proof_len = dev.proof_stride = plen;
  dev.commitments32 = to_device(commitments);
  dev.m = 1;
  dev.min_values = to_device(min_values);
  dev.min_present = to_device(min_present);
  bpp_packed_batch first = dev, bad_dev = dev;
  first.transcript_label = (const uint8_t *)label.data();
  first.label_len = label.size();
  bad_dev.proofs = to_device(holes_bad);
  uint64_t h = 0;
  CHECK(bpp_batch_upload_packed_device(ctx, params->handle(), &first, &h, err, sizeof(err)) == BPP_OK);

  // the reference: the live items alone, in slot order, as a batch of their own with the boundaries mapped
  const std::vector<size_t> slots = {0, 4, 5};
  const std::vector<uint32_t> ref_bounds = {0, 1, 3};
  const size_t L_ITEMS = slots.size(), G_REF = 2;
  bpp_packed_batch ref = first;
  ref.n_items = L_ITEMS;
  ref.proofs = to_device(gather(proofs, plen, slots));
  ref.commitments32 = to_device(gather(commitments, 32, slots));
  ref.min_values = to_device(gather(min_values, 1, slots));
  ref.min_present = to_device(gather(min_present, 1, slots));
  uint64_t h_ref = 0;
  CHECK(bpp_batch_upload_packed_device(ctx, params->handle(), &ref, &h_ref, err, sizeof(err)) == BPP_OK);

  const std::vector<uint8_t> mask_host = {1, 0, 0, 0, 255, 2};
  uint8_t *mask = to_device(mask_host);
  void *out = nullptr;  // one refill record, G + G_REF verdict records, N + L_ITEMS weights
  const size_t out_bytes = sizeof(bpp_device_refill) + (G + G_REF) * sizeof(bpp_device_verdict) + (N + L_ITEMS) * 32;
  CHECK(hipMalloc(&out, out_bytes) == hipSuccess);
  CHECK(hipMemset(out, 0xff, out_bytes) == hipSuccess);
  bpp_device_refill *record = static_cast<bpp_device_refill *>(out);
  bpp_device_verdict *verdicts = reinterpret_cast<bpp_device_verdict *>(record + 1);
  uint8_t *weights = reinterpret_cast<uint8_t *>(verdicts + G + G_REF);
  eng.batch_refill_enqueue_live(h, bad_dev, mask, record);
  eng.verify_enqueue(h, nullptr, G, 2, nullptr, VerifyAction::VerifyOnly, verdicts);
  eng.enqueue_weights(h, weights);
  eng.verify_enqueue(h_ref, ref_bounds.data(), G_REF, 0, nullptr, VerifyAction::VerifyOnly, verdicts + G);
  Engine::EnqueueTicket last = eng.enqueue_weights(h_ref, weights + N * 32);
  last.wait();  // the one wait
  bpp_device_refill rec;
  std::vector<bpp_device_verdict> ver(G + G_REF);
  std::vector<uint8_t> w((N + L_ITEMS) * 32);
  CHECK(hipMemcpy(&rec, record, sizeof(rec), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(ver.data(), verdicts, ver.size() * sizeof(bpp_device_verdict), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(w.data(), weights, w.size(), hipMemcpyDeviceToHost) == hipSuccess);
  bpp_shard_result r;
  CHECK(bpp_refill_result(&rec, &r) == BPP_OK);
  printf("record %d %d %u %u %s\n", r.code, r.tier, r.index, rec.flags, r.msg);
  for (size_t g = 0; g < G + G_REF; g++) {
    bpp_shard_result v;
    CHECK(bpp_verdict_result(&ver[g], &v) == BPP_OK);
    printf("%s_%zu %d %u %u %u %s\n", g < G ? "verdict" : "reference", g < G ? g : g - G, ver[g].code, ver[g].tier, ver[g].index, ver[g].flags, v.msg);
  }
  printf("weights ");  // 1: a non-zero row
  for (size_t i = 0; i < N + L_ITEMS; i++) {
    bool any = false;
    for (int b = 0; b < 32; b++) any = any || w[i * 32 + b] != 0;
    printf("%d", any ? 1 : 0);
  }
  printf("\n");
  // the live slots carry the fresh upload's weights
  int same = 1;
  for (size_t k = 0; k < L_ITEMS; k++) same = same && memcmp(&w[slots[k] * 32], &w[(N + k) * 32], 32) == 0;
  printf("same_weights %d\n", same);
  const struct bpp_refill_stats st = eng.refill_stats();
  const struct bpp_enqueue_stats es = eng.enqueue_stats();
  printf("stats %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.first_calls, (unsigned long long)st.host_waits);
  // a mask in host memory is refused through the mirror as an exception, before anything is launched
  std::string what;
  try {
    eng.batch_refill_enqueue_live(h, dev, mask_host.data(), nullptr);
  } catch (const std::exception &e) {
    what = e.what();
  }
  printf("refused %s\n", what.c_str());
  CHECK(eng.refill_stats().calls == st.calls && eng.enqueue_stats().calls == es.calls);
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  CHECK(bpp_batch_destroy(ctx, h_ref) == BPP_OK);
  for (const void *p : {(const void *)dev.proofs, (const void *)dev.commitments32, (const void *)dev.min_values, (const void *)dev.min_present,
                        (const void *)bad_dev.proofs, (const void *)ref.proofs, (const void *)ref.commitments32, (const void *)ref.min_values,
                        (const void *)ref.min_present, (const void *)mask, (const void *)out})
    CHECK(hipFree(const_cast<void *>(p)) == hipSuccess);
  printf("refill live ok\n");
  return 0;
}
