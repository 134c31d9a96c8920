// A compiled caller of bpp_batch_refill_enqueue, bpp_refill_result and bpp_refill_stats (include/bpp.h) through
// Engine::batch_refill_enqueue / Engine::refill_stats of include/bpp.hpp, with arrays it allocated itself with hipMalloc -- no torch,
// no ctypes declarations that could hide a wrong prototype.  Five proofs (n = 64, m = 1, t = 1) are committed and proved through
// bpp.h and uploaded from device memory; the batch is then refilled with the same proofs, with l in r1 of proof 3, and with the
// clean proofs again, each followed by an enqueued verification.  The program prints the records; tests/test_gpu_cpp_refill.py
// reads them.
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
  const size_t N = 5, rounds = 6, plen = 1 + 32 * (1 + 5 + 2 * rounds);
  uint64_t s = 20261020;
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
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  std::vector<uint8_t> bad = proofs;
  memcpy(&bad[3 * plen + 1 + 32 * 4], L, 32);

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
  first.transcript_label = (const uint8_t *)label.data();  // the upload sets the batch's transcript; a refill keeps it
  first.label_len = label.size();
  bad_dev.proofs = to_device(bad);
  uint64_t h = 0;
  CHECK(bpp_batch_upload_packed_device(ctx, params->handle(), &first, &h, err, sizeof(err)) == BPP_OK);

  void *out = nullptr;  // one refill record and one verdict record per step
  CHECK(hipMalloc(&out, 3 * (sizeof(bpp_device_refill) + sizeof(bpp_device_verdict))) == hipSuccess);
  bpp_device_refill *records = static_cast<bpp_device_refill *>(out);
  bpp_device_verdict *verdicts = reinterpret_cast<bpp_device_verdict *>(records + 3);
  const bpp_packed_batch *steps[3] = {&dev, &bad_dev, &dev};
  Engine::EnqueueTicket last;
  for (int k = 0; k < 3; k++) {
    eng.batch_refill_enqueue(h, *steps[k], &records[k]);
    last = eng.verify_enqueue(h, nullptr, 0, 0, nullptr, VerifyAction::VerifyOnly, &verdicts[k]);
  }
  last.wait();  // the one wait
  bpp_device_refill rec[3];
  bpp_device_verdict ver[3];
  CHECK(hipMemcpy(rec, records, sizeof(rec), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(ver, verdicts, sizeof(ver), hipMemcpyDeviceToHost) == hipSuccess);
  for (int k = 0; k < 3; k++) {
    bpp_shard_result r, v;
    CHECK(bpp_refill_result(&rec[k], &r) == BPP_OK && bpp_verdict_result(&ver[k], &v) == BPP_OK);
    printf("refill_%d %d %d %u %u %s\n", k, r.code, r.tier, r.index, rec[k].flags, r.msg);
    printf("verdict_%d %d %u %u %u\n", k, ver[k].code, ver[k].tier, ver[k].index, ver[k].flags);
  }
  const struct bpp_refill_stats st = eng.refill_stats();
  printf("stats %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.first_calls, (unsigned long long)st.host_waits);
  // a transcript field is refused through the mirror as an exception, before anything is launched
  std::string what;
  try {
    eng.batch_refill_enqueue(h, first);
  } catch (const std::exception &e) {
    what = e.what();
  }
  printf("refused %s\n", what.c_str());
  CHECK(eng.refill_stats().calls == st.calls);
  // a refilled batch takes enqueued calls only
  CHECK(bpp_verify_resident(ctx, h, BPP_VERIFY_ONLY, 0, nullptr, nullptr, err, sizeof(err)) == BPP_ERR_INVALID_ARGUMENT);
  printf("blocking %s\n", err);
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  for (const void *p : {(const void *)dev.proofs, (const void *)dev.commitments32, (const void *)dev.min_values, (const void *)dev.min_present,
                        (const void *)bad_dev.proofs, (const void *)out})
    CHECK(hipFree(const_cast<void *>(p)) == hipSuccess);
  printf("refill ok\n");
  return 0;
}
