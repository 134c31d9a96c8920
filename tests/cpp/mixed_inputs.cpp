// A compiled caller of the mixed-aggregation array form of include/bpp.h (bpp_batch_upload_mixed, bpp_verify_batch_mixed and their
// _device forms) and of the overload pair of include/bpp.hpp, with arrays it allocated itself with hipMalloc -- no torch, no ctypes
// declarations that could hide a wrong prototype.  Five items (n = 8, m = 2, 1, 4, 1, 1, t = 1) are proved from their openings with
// bpp_prove_openings; what that call wrote -- proofs in rows of proof_stride, proof_lens, commitments in rows of commit_stride -- goes
// into a bpp_mixed_batch as it is, is copied to the device, and is verified as a bpp_verify_item array, from host memory and from
// device memory.  The program prints the codes, masks and BPP_TRACE_MSM_RESULT of the three, tests/test_gpu_cpp_mixed_inputs.py
// compares them.
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
  auto params = RangeParameters::init(eng, 8, 4, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  const std::string label = "mixed inputs";
  const size_t N = 5, M_STRIDE = 8, STRIDE = 1 + 32 * (1 + 5 + 2 * 5) + 3;  // the longest proof (m = 4: five rounds) and three bytes
  const uint32_t ms[N] = {2, 1, 4, 1, 1};
  uint64_t s = 20261021;
  std::vector<uint64_t> values(N * M_STRIDE), min_values(N * M_STRIDE, 1ull << 63);
  std::vector<uint8_t> blindings(32 * N * M_STRIDE), seeds(32 * N), seed_present(N), min_present(N * M_STRIDE, 1), ext(N * 32 * 8);
  std::vector<uint8_t> commitments(32 * N * M_STRIDE, 0xff), proofs(N * STRIDE, 0xff);  // (what the prover does not write stays 0xff: row slack)
  std::vector<size_t> lens(N);
  std::vector<uint32_t> m(ms, ms + N);
  std::vector<bpp_prove_item> items(N);
  for (auto &x : ext) x = (uint8_t)splitmix(s);
  for (size_t i = 0; i < N; i++) {
    for (size_t j = 0; j < ms[i]; j++) {
      values[i * M_STRIDE + j] = splitmix(s) & 0xff;
      min_values[i * M_STRIDE + j] = values[i * M_STRIDE + j] / 3;
      min_present[i * M_STRIDE + j] = (uint8_t)(j & 1);
      for (int k = 0; k < 31; k++) blindings[32 * (i * M_STRIDE + j) + k] = (uint8_t)splitmix(s) | (k == 0);
    }
    for (int k = 0; k < 31; k++) seeds[32 * i + k] = (uint8_t)splitmix(s) | (k == 0);
    seed_present[i] = ms[i] == 1;
    memset(&items[i], 0, sizeof(items[i]));
    items[i].values = &values[i * M_STRIDE];
    items[i].blindings32 = &blindings[32 * i * M_STRIDE];
    items[i].m = ms[i];
    items[i].min_values = &min_values[i * M_STRIDE];
    items[i].min_present = &min_present[i * M_STRIDE];
    items[i].seed_nonce32 = seed_present[i] ? &seeds[32 * i] : nullptr;
    items[i].transcript_label = (const uint8_t *)label.data();
    items[i].label_len = label.size();
    items[i].rng_bytes = &ext[i * 32 * 8];
    items[i].rng_len = 32 * 8;
  }
  char err[256] = {0};
  std::vector<int> status(N, -1);
  CHECK(bpp_prove_openings(ctx, params->handle(), items.data(), N, commitments.data(), 32 * M_STRIDE, proofs.data(), STRIDE, lens.data(),
                           status.data(), err, sizeof(err)) == BPP_OK);
  for (size_t i = 0; i < N; i++) CHECK(status[i] == BPP_OK && lens[i] == 1 + 32 * (size_t)(6 + 2 * (3 + (ms[i] > 1) + (ms[i] > 2))));

  // the prover's buffers as they are
  bpp_mixed_batch host;
  memset(&host, 0, sizeof(host));
  host.n_items = N;
  host.proofs = proofs.data();
  host.proof_stride = STRIDE;
  host.proof_lens = lens.data();
  host.m = m.data();
  host.m_stride = (uint32_t)M_STRIDE;
  host.commitments32 = commitments.data();
  host.min_values = min_values.data();
  host.min_present = min_present.data();
  host.seed_nonces32 = seeds.data();
  host.seed_present = seed_present.data();
  host.transcript_label = (const uint8_t *)label.data();
  host.label_len = label.size();
  bpp_mixed_batch dev = host;
  dev.proofs = to_device(proofs);
  dev.commitments32 = to_device(commitments);
  dev.min_values = to_device(min_values);
  dev.min_present = to_device(min_present);
  dev.seed_nonces32 = to_device(seeds);
  dev.seed_present = to_device(seed_present);
  // ... and as the bpp_verify_item array the two forms are held to
  std::vector<bpp_verify_item> vitems(N);
  for (size_t i = 0; i < N; i++) {
    memset(&vitems[i], 0, sizeof(vitems[i]));
    vitems[i].proof = &proofs[i * STRIDE];
    vitems[i].proof_len = lens[i];
    vitems[i].commitments32 = &commitments[32 * i * M_STRIDE];
    vitems[i].m = ms[i];
    vitems[i].min_values = &min_values[i * M_STRIDE];
    vitems[i].min_present = &min_present[i * M_STRIDE];
    vitems[i].seed_nonce32 = seed_present[i] ? &seeds[32 * i] : nullptr;
    vitems[i].transcript_label = (const uint8_t *)label.data();
    vitems[i].label_len = label.size();
  }

  // one blocking call each, straight off bpp.h
  std::vector<uint8_t> masks_i(32 * N), masks_h(32 * N), masks_d(32 * N), pres_i(N), pres_h(N), pres_d(N);
  const int rc_i = bpp_verify_batch(ctx, params->handle(), vitems.data(), N, BPP_RECOVER_AND_VERIFY, 2, masks_i.data(), pres_i.data(), err, sizeof(err));
  const int rc_h = bpp_verify_batch_mixed(ctx, params->handle(), &host, BPP_RECOVER_AND_VERIFY, 2, masks_h.data(), pres_h.data(), err, sizeof(err));
  const int rc_d = bpp_verify_batch_mixed_device(ctx, params->handle(), &dev, BPP_RECOVER_AND_VERIFY, 2, masks_d.data(), pres_d.data(), err, sizeof(err));
  printf("items_code %d\nhost_code %d\ndevice_code %d\n", rc_i, rc_h, rc_d);
  print_hex("items_masks", masks_i.data(), masks_i.size());
  print_hex("host_masks", masks_h.data(), masks_h.size());
  print_hex("device_masks", masks_d.data(), masks_d.size());
  print_hex("items_present", pres_i.data(), N);
  print_hex("host_present", pres_h.data(), N);
  print_hex("device_present", pres_d.data(), N);
  for (size_t i = 0; i < N; i++)
    if (ms[i] == 1) CHECK(pres_d[i] == 1 && memcmp(&masks_d[32 * i], &blindings[32 * i * M_STRIDE], 32) == 0);  // the blinding the prover was given

  // resident batches: the final check's point
  for (int form = 0; form < 3; form++) {
    uint64_t h = 0;
    const int rc = form == 0   ? bpp_batch_upload(ctx, params->handle(), vitems.data(), N, &h, err, sizeof(err))
                   : form == 1 ? bpp_batch_upload_mixed(ctx, params->handle(), &host, &h, err, sizeof(err))
                               : bpp_batch_upload_mixed_device(ctx, params->handle(), &dev, &h, err, sizeof(err));
    CHECK(rc == BPP_OK);
    CHECK(bpp_verify_resident(ctx, h, BPP_VERIFY_ONLY, 0, nullptr, nullptr, err, sizeof(err)) == BPP_OK);
    uint8_t point[32];
    size_t written = 0;
    memset(point, 0xff, sizeof(point));
    CHECK(bpp_batch_trace(ctx, h, BPP_TRACE_MSM_RESULT, point, sizeof(point), &written) == BPP_OK && written == 32);
    print_hex(form == 0 ? "items_msm" : form == 1 ? "host_msm" : "device_msm", point, 32);
    CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  }
  struct bpp_ingest_stats st;
  CHECK(bpp_ingest_stats(ctx, &st) == BPP_OK && st.device_calls == 2 && st.host_fallback_calls == 0 && st.fallback_bytes == 0);

  // the overload pair of bpp.hpp
  const auto mh = RangeProof::verify_batch(*params, host, VerifyAction::RecoverAndVerify, 0);
  const auto md = RangeProof::verify_batch(*params, DeviceMixedBatch{dev}, VerifyAction::RecoverAndVerify, 0);
  CHECK(mh.size() == N && md.size() == N);
  for (size_t i = 0; i < N; i++) {
    CHECK((bool)mh[i] == (ms[i] == 1) && (bool)md[i] == (ms[i] == 1));
    if (!mh[i]) continue;
    printf("hpp_host_mask_%zu ", i);
    for (uint8_t b : mh[i]->blindings[0]) printf("%02x", b);
    printf("\nhpp_device_mask_%zu ", i);
    for (uint8_t b : md[i]->blindings[0]) printf("%02x", b);
    printf("\n");
  }
  // findings travel through the overload as the same exception: l in r1 of proof 3 (the kernel finds it), m[1] = 3 (the host knows it)
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  std::vector<uint8_t> bad = proofs;
  memcpy(&bad[3 * STRIDE + 1 + 32 * 4], L, 32);
  std::vector<uint32_t> m3 = m;
  m3[1] = 3;
  bpp_mixed_batch bad_h = host, bad_d = dev;
  bad_h.proofs = bad.data();
  bad_d.proofs = to_device(bad);
  for (int round = 0; round < 2; round++) {
    if (round == 1) bad_h.m = bad_d.m = m3.data();
    std::string what_h, what_d;
    try {
      RangeProof::verify_batch(*params, bad_h, VerifyAction::VerifyOnly, 0);
    } catch (const ProofError &e) {
      what_h = std::to_string((int)e.kind) + " " + e.what();
    }
    try {
      RangeProof::verify_batch(*params, DeviceMixedBatch{bad_d}, VerifyAction::VerifyOnly, 0);
    } catch (const ProofError &e) {
      what_d = std::to_string((int)e.kind) + " " + e.what();
    }
    printf("hpp_host_error_%d %s\nhpp_device_error_%d %s\n", round, what_h.c_str(), round, what_d.c_str());
  }
  uint64_t nonzero = 1;
  CHECK(bpp_batch_secret_bytes(ctx, 0, &nonzero) == BPP_OK && nonzero == 0);
  for (const void *p : {(const void *)dev.proofs, (const void *)dev.commitments32, (const void *)dev.min_values, (const void *)dev.min_present,
                        (const void *)dev.seed_nonces32, (const void *)dev.seed_present, (const void *)bad_d.proofs})
    CHECK(hipFree(const_cast<void *>(p)) == hipSuccess);
  printf("mixed_inputs ok\n");
  return 0;
}
