// A compiled caller of bpp_batch_refill_enqueue_count and bpp_enqueue_weights (include/bpp.h) through the overload of
// Engine::batch_refill_enqueue that takes a count and Engine::enqueue_weights of include/bpp.hpp, with arrays it allocated itself
// with hipMalloc -- no torch, no ctypes declarations that could hide a wrong prototype.  Six proofs (n = 64, m = 1, t = 1) are
// committed and proved through bpp.h and uploaded from device memory; the batch is then refilled with count 4, count 7 (one more
// than it holds), count 6 and no count, each followed by an enqueued verification in chunks of two proofs and the weights call.
// The program prints the records and which weight rows are zero; tests/test_gpu_cpp_refill_count.py reads them.
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

int main() {
  Engine eng(0);
  bpp_ctx *ctx = eng.ctx();
  auto params = RangeParameters::init(eng, 64, 1, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  const std::string label = "refill";
  const size_t N = 6, G = 3, rounds = 6, plen = 1 + 32 * (1 + 5 + 2 * rounds), STEPS = 4;
  uint64_t s = 20261021;
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
  // beyond the first four: a proof that does not verify and a non-canonical scalar -- neither is looked at under count 4
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  std::vector<uint8_t> tail_bad = proofs;
  tail_bad[4 * plen + 1 + 32 * 4] ^= 1;
  memcpy(&tail_bad[5 * plen + 1 + 32 * 5], L, 32);

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
  bad_dev.proofs = to_device(tail_bad);
  uint64_t h = 0;
  CHECK(bpp_batch_upload_packed_device(ctx, params->handle(), &first, &h, err, sizeof(err)) == BPP_OK);

  const std::vector<uint32_t> counts_host = {4, 7, 6};
  uint32_t *counts = to_device(counts_host);
  void *out = nullptr;  // per step: one refill record, G verdict records, N weights
  const size_t step_bytes = sizeof(bpp_device_refill) + G * sizeof(bpp_device_verdict) + N * 32;
  CHECK(hipMalloc(&out, STEPS * step_bytes) == hipSuccess);
  CHECK(hipMemset(out, 0xff, STEPS * step_bytes) == hipSuccess);
  bpp_device_refill *records = static_cast<bpp_device_refill *>(out);
  bpp_device_verdict *verdicts = reinterpret_cast<bpp_device_verdict *>(records + STEPS);
  uint8_t *weights = reinterpret_cast<uint8_t *>(verdicts + STEPS * G);
  const bpp_packed_batch *src[STEPS] = {&bad_dev, &dev, &dev, &dev};
  const uint32_t *cnt[STEPS] = {counts, counts + 1, counts + 2, nullptr};
  Engine::EnqueueTicket last;
  for (size_t k = 0; k < STEPS; k++) {
    eng.batch_refill_enqueue(h, *src[k], cnt[k], &records[k]);
    eng.verify_enqueue(h, nullptr, G, 2, nullptr, VerifyAction::VerifyOnly, &verdicts[k * G]);
    last = eng.enqueue_weights(h, weights + k * N * 32);
  }
  last.wait();  // the one wait
  std::vector<bpp_device_refill> rec(STEPS);
  std::vector<bpp_device_verdict> ver(STEPS * G);
  std::vector<uint8_t> w(STEPS * N * 32);
  CHECK(hipMemcpy(rec.data(), records, STEPS * sizeof(bpp_device_refill), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(ver.data(), verdicts, STEPS * G * sizeof(bpp_device_verdict), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(w.data(), weights, w.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (size_t k = 0; k < STEPS; k++) {
    bpp_shard_result r;
    CHECK(bpp_refill_result(&rec[k], &r) == BPP_OK);
    printf("refill_%zu %d %d %u %u %s\n", k, r.code, r.tier, r.index, rec[k].flags, r.msg);
    for (size_t g = 0; g < G; g++) {
      bpp_shard_result v;
      CHECK(bpp_verdict_result(&ver[k * G + g], &v) == BPP_OK);
      printf("verdict_%zu_%zu %d %u %u %u %s\n", k, g, ver[k * G + g].code, ver[k * G + g].tier, ver[k * G + g].index, ver[k * G + g].flags, v.msg);
    }
    printf("weights_%zu ", k);  // 1: a non-zero row
    for (size_t i = 0; i < N; i++) {
      bool any = false;
      for (int b = 0; b < 32; b++) any = any || w[(k * N + i) * 32 + b] != 0;
      printf("%d", any ? 1 : 0);
    }
    printf("\n");
  }
  // the live proofs of steps 0, 2 and 3 are the same proofs in the same groups: the same weights
  printf("same_weights %d %d\n", memcmp(&w[0], &w[2 * N * 32], 4 * 32) == 0 ? 1 : 0, memcmp(&w[2 * N * 32], &w[3 * N * 32], N * 32) == 0 ? 1 : 0);
  const struct bpp_refill_stats st = eng.refill_stats();
  const struct bpp_enqueue_stats es = eng.enqueue_stats();
  printf("stats %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.first_calls, (unsigned long long)st.host_waits);
  // a count in host memory is refused through the mirror as an exception, before anything is launched
  std::string what;
  uint32_t host_count = 3;
  try {
    eng.batch_refill_enqueue(h, dev, &host_count, nullptr);
  } catch (const std::exception &e) {
    what = e.what();
  }
  printf("refused %s\n", what.c_str());
  CHECK(eng.refill_stats().calls == st.calls && eng.enqueue_stats().calls == es.calls);
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  for (const void *p : {(const void *)dev.proofs, (const void *)dev.commitments32, (const void *)dev.min_values, (const void *)dev.min_present,
                        (const void *)bad_dev.proofs, (const void *)counts, (const void *)out})
    CHECK(hipFree(const_cast<void *>(p)) == hipSuccess);
  printf("refill count ok\n");
  return 0;
}
