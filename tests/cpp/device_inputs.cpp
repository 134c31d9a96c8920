// A compiled caller of the device-memory entry points of include/bpp.h (bpp_batch_upload_packed_device,
// bpp_verify_batch_packed_device, bpp_device_pointer_check, bpp_ingest_stats) and of the overload pair of include/bpp.hpp, with
// arrays it allocated itself with hipMalloc -- no torch, no ctypes declarations that could hide a wrong prototype.  Five proofs
// (n = 64, m = 1, t = 1) are committed and proved through bpp.h, copied to the device, and verified from there and from host memory;
// the program prints the codes, masks and BPP_TRACE_MSM_RESULT of both, tests/test_gpu_cpp_device_inputs.py compares them.
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

static void print_hex(const char *name, const uint8_t *p, size_t n) {
  printf("%s ", name);
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
  printf("\n");
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
  const std::string label = "device inputs";
  const size_t N = 5, rounds = 6, plen = 1 + 32 * (1 + 5 + 2 * rounds);
  uint64_t s = 20261020;
  std::vector<uint64_t> values(N), min_values(N);
  std::vector<uint8_t> blindings(32 * N), seeds(32 * N), min_present(N, 1), commitments(32 * N), ext(N * 32 * (rounds + 3)), proofs(N * plen);
  for (size_t i = 0; i < N; i++) {
    values[i] = splitmix(s) >> 1;
    min_values[i] = values[i] / 3;
    for (int k = 0; k < 31; k++) {
      blindings[32 * i + k] = (uint8_t)splitmix(s) | (k == 0);
      seeds[32 * i + k] = (uint8_t)splitmix(s) | (k == 0);
    }
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
    items[i].seed_nonce32 = &seeds[32 * i];
    items[i].transcript_label = (const uint8_t *)label.data();
    items[i].label_len = label.size();
    items[i].rng_bytes = &ext[i * 32 * (rounds + 3)];
    items[i].rng_len = 32 * (rounds + 3);
  }
  size_t got_len = 0;
  CHECK(bpp_prove_batch(ctx, params->handle(), items.data(), N, proofs.data(), plen, &got_len, err, sizeof(err)) == BPP_OK && got_len == plen);

  bpp_packed_batch host;
  memset(&host, 0, sizeof(host));
  host.n_items = N;
  host.proofs = proofs.data();
  host.proof_len = host.proof_stride = plen;
  host.commitments32 = commitments.data();
  host.m = 1;
  host.min_values = min_values.data();
  host.min_present = min_present.data();
  host.seed_nonces32 = seeds.data();
  host.transcript_label = (const uint8_t *)label.data();
  host.label_len = label.size();
  bpp_packed_batch dev = host;
  dev.proofs = to_device(proofs);
  dev.commitments32 = to_device(commitments);
  dev.min_values = to_device(min_values);
  dev.min_present = to_device(min_present);
  dev.seed_nonces32 = to_device(seeds);

  int kind = -1;
  CHECK(bpp_device_pointer_check(ctx, dev.proofs, &kind) == BPP_OK && kind == BPP_PTR_THIS_DEVICE);
  CHECK(bpp_device_pointer_check(ctx, proofs.data(), &kind) == BPP_OK && kind == BPP_PTR_HOST_OR_UNKNOWN);
  CHECK(hipGetLastError() == hipSuccess);  // the query of a pointer the runtime does not know left nothing behind

  // one blocking call each, straight off bpp.h
  std::vector<uint8_t> masks_h(32 * N), masks_d(32 * N), pres_h(N), pres_d(N);
  const int rc_h = bpp_verify_batch_packed(ctx, params->handle(), &host, BPP_RECOVER_AND_VERIFY, 0, masks_h.data(), pres_h.data(), err, sizeof(err));
  const int rc_d = bpp_verify_batch_packed_device(ctx, params->handle(), &dev, BPP_RECOVER_AND_VERIFY, 0, masks_d.data(), pres_d.data(), err, sizeof(err));
  printf("host_code %d\ndevice_code %d\n", rc_h, rc_d);
  print_hex("host_masks", masks_h.data(), masks_h.size());
  print_hex("device_masks", masks_d.data(), masks_d.size());
  print_hex("host_present", pres_h.data(), N);
  print_hex("device_present", pres_d.data(), N);
  CHECK(memcmp(masks_d.data(), blindings.data(), 32 * N) == 0);  // the blindings the prover was given

  // resident batches: the final check's point
  for (int on_device = 0; on_device < 2; on_device++) {
    uint64_t h = 0;
    const int rc = on_device ? bpp_batch_upload_packed_device(ctx, params->handle(), &dev, &h, err, sizeof(err))
                             : bpp_batch_upload_packed(ctx, params->handle(), &host, &h, err, sizeof(err));
    CHECK(rc == BPP_OK);
    CHECK(bpp_verify_resident(ctx, h, BPP_VERIFY_ONLY, 0, nullptr, nullptr, err, sizeof(err)) == BPP_OK);
    uint8_t point[32];
    size_t written = 0;
    memset(point, 0xff, sizeof(point));
    CHECK(bpp_batch_trace(ctx, h, BPP_TRACE_MSM_RESULT, point, sizeof(point), &written) == BPP_OK && written == 32);
    print_hex(on_device ? "device_msm" : "host_msm", point, 32);
    CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  }
  struct bpp_ingest_stats st;
  CHECK(bpp_ingest_stats(ctx, &st) == BPP_OK && st.device_calls == 2 && st.host_fallback_calls == 0 && st.fallback_bytes == 0);

  // the overload pair of bpp.hpp
  const auto mh = RangeProof::verify_batch(*params, host, VerifyAction::RecoverAndVerify, 0);
  const auto md = RangeProof::verify_batch(*params, DevicePackedBatch{dev}, VerifyAction::RecoverAndVerify, 0);
  CHECK(mh.size() == N && md.size() == N);
  for (size_t i = 0; i < N; i++) {
    CHECK(mh[i] && md[i] && mh[i]->blindings.size() == 1 && md[i]->blindings.size() == 1);
    printf("hpp_host_mask_%zu ", i);
    for (uint8_t b : mh[i]->blindings[0]) printf("%02x", b);
    printf("\nhpp_device_mask_%zu ", i);
    for (uint8_t b : md[i]->blindings[0]) printf("%02x", b);
    printf("\n");
  }
  // a finding travels through the overload as the same exception: l in r1 of proof 3
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  std::vector<uint8_t> bad = proofs;
  memcpy(&bad[3 * plen + 1 + 32 * 4], L, 32);
  bpp_packed_batch bad_h = host, bad_d = dev;
  bad_h.proofs = bad.data();
  bad_d.proofs = to_device(bad);
  std::string what_h, what_d;
  try {
    RangeProof::verify_batch(*params, bad_h, VerifyAction::VerifyOnly, 0);
  } catch (const ProofError &e) {
    what_h = std::to_string((int)e.kind) + " " + e.what();
  }
  try {
    RangeProof::verify_batch(*params, DevicePackedBatch{bad_d}, VerifyAction::VerifyOnly, 0);
  } catch (const ProofError &e) {
    what_d = std::to_string((int)e.kind) + " " + e.what();
  }
  printf("hpp_host_error %s\nhpp_device_error %s\n", what_h.c_str(), what_d.c_str());
  uint64_t nonzero = 1;
  CHECK(bpp_batch_secret_bytes(ctx, 0, &nonzero) == BPP_OK && nonzero == 0);
  for (const void *p : {(const void *)dev.proofs, (const void *)dev.commitments32, (const void *)dev.min_values, (const void *)dev.min_present,
                        (const void *)dev.seed_nonces32, (const void *)bad_d.proofs})
    CHECK(hipFree(const_cast<void *>(p)) == hipSuccess);
  printf("device_inputs ok\n");
  return 0;
}
