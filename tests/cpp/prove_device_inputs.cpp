// A compiled caller of bpp_prove_openings_device (include/bpp.h) and of RangeProof::prove_openings over a DeviceProveArrays
// (include/bpp.hpp), with arrays it allocated itself with hipMalloc -- no torch, no ctypes declarations that could hide a wrong
// prototype.  Five items (n = 8, m = 2, 1, 4, 1, 1, t = 1) are proved twice: with bpp_prove_openings from host arrays, and from
// device copies of the same arrays -- the blinding factors at an ODD byte address -- into device rows prefilled with 0xff.  The
// device rows must equal the host call's rows byte for byte (slack included), the status records must read Ok, and the outputs go
// into bpp_verify_batch_mixed_device where they lie.  tests/test_gpu_cpp_prove_device.py compares what the program prints.
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

// a device copy of v that starts `skew` bytes into its allocation
template <typename T>
static T *to_device(const std::vector<T> &v, size_t skew = 0) {
  void *d = nullptr;
  CHECK(hipMalloc(&d, v.size() * sizeof(T) + skew) == hipSuccess);
  CHECK(hipMemcpy((uint8_t *)d + skew, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  return reinterpret_cast<T *>((uint8_t *)d + skew);
}

int main() {
  Engine eng(0);
  bpp_ctx *ctx = eng.ctx();
  auto params = RangeParameters::init(eng, 8, 4, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  const std::string label = "prove device inputs";
  const size_t N = 5, M_STRIDE = 8, STRIDE = 1 + 32 * (1 + 5 + 2 * 5) + 3, CSTRIDE = 32 * M_STRIDE, RNG = 32 * 8 + 5;
  const uint32_t ms[N] = {2, 1, 4, 1, 1};
  uint64_t s = 20261020;
  // row slack holds what would be a finding if it were read
  std::vector<uint64_t> values(N * M_STRIDE, ~0ull), min_values(N * M_STRIDE, ~0ull);
  std::vector<uint8_t> blindings(32 * N * M_STRIDE, 0xff), seeds(32 * N, 0xff), seed_present(N), min_present(N * M_STRIDE, 1), ext(N * RNG, 0xff);
  std::vector<uint32_t> m(ms, ms + N);
  std::vector<bpp_prove_item> items(N);
  for (size_t i = 0; i < N; i++) {
    for (size_t j = 0; j < ms[i]; j++) {
      values[i * M_STRIDE + j] = splitmix(s) & 0xff;
      min_values[i * M_STRIDE + j] = values[i * M_STRIDE + j] / 3;
      min_present[i * M_STRIDE + j] = (uint8_t)(j & 1);
      for (int k = 0; k < 32; k++) blindings[32 * (i * M_STRIDE + j) + k] = k < 31 ? (uint8_t)splitmix(s) | (k == 0) : 0;
    }
    seed_present[i] = ms[i] == 1;
    if (seed_present[i])
      for (int k = 0; k < 32; k++) seeds[32 * i + k] = k < 31 ? (uint8_t)splitmix(s) | (k == 0) : 0;
    const size_t need = 32 * (size_t)(3 + 3 + (ms[i] > 1) + (ms[i] > 2));
    for (size_t k = 0; k < need; k++) ext[i * RNG + k] = (uint8_t)splitmix(s);
    memset(&items[i], 0, sizeof(items[i]));
    items[i].values = &values[i * M_STRIDE];
    items[i].blindings32 = &blindings[32 * i * M_STRIDE];
    items[i].m = ms[i];
    items[i].min_values = &min_values[i * M_STRIDE];
    items[i].min_present = &min_present[i * M_STRIDE];
    items[i].seed_nonce32 = seed_present[i] ? &seeds[32 * i] : nullptr;
    items[i].transcript_label = (const uint8_t *)label.data();
    items[i].label_len = label.size();
    items[i].rng_bytes = &ext[i * RNG];
    items[i].rng_len = RNG;
  }
  char err[256] = {0};
  std::vector<uint8_t> commitments(N * CSTRIDE, 0xff), proofs(N * STRIDE, 0xff);
  std::vector<size_t> lens(N), lens_d(N);
  std::vector<int> status(N, -1), status_d(N, -1);
  CHECK(bpp_prove_openings(ctx, params->handle(), items.data(), N, commitments.data(), CSTRIDE, proofs.data(), STRIDE, lens.data(), status.data(),
                           err, sizeof(err)) == BPP_OK);

  // the same arrays in device memory, straight off bpp.h
  bpp_prove_arrays in;
  memset(&in, 0, sizeof(in));
  in.n_items = N;
  in.m = m.data();
  in.m_stride = (uint32_t)M_STRIDE;
  in.values = to_device(values);
  in.blindings32 = to_device(blindings, 1);  // an odd byte address
  in.min_values = to_device(min_values);
  in.min_present = to_device(min_present);
  in.seed_nonces32 = to_device(seeds);
  in.seed_present = to_device(seed_present);
  in.rng_bytes = to_device(ext, 3);
  in.rng_stride = RNG;
  in.transcript_label = (const uint8_t *)label.data();
  in.label_len = label.size();
  CHECK(((uintptr_t)in.blindings32 & 1) == 1);
  const std::vector<uint8_t> fill_c(N * CSTRIDE, 0xff), fill_p(N * STRIDE, 0xff);
  uint8_t *d_commit = to_device(fill_c), *d_proofs = to_device(fill_p);
  bpp_device_prove_status *d_status = to_device(std::vector<bpp_device_prove_status>(N, bpp_device_prove_status{-1, 99}));
  const int rc = bpp_prove_openings_device(ctx, params->handle(), &in, d_commit, CSTRIDE, d_proofs, STRIDE, lens_d.data(), d_status,
                                           status_d.data(), err, sizeof(err));
  printf("device_code %d %s\n", rc, err);
  std::vector<uint8_t> got_c(N * CSTRIDE), got_p(N * STRIDE);
  std::vector<bpp_device_prove_status> got_s(N);
  CHECK(hipMemcpy(got_c.data(), d_commit, got_c.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(got_p.data(), d_proofs, got_p.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(got_s.data(), d_status, N * sizeof(got_s[0]), hipMemcpyDeviceToHost) == hipSuccess);
  printf("proofs_equal %d\ncommitments_equal %d\nlens_equal %d\nstatus_equal %d\n", (int)(got_p == proofs), (int)(got_c == commitments),
         (int)(lens_d == lens), (int)(status_d == status));
  for (size_t i = 0; i < N; i++) {
    bpp_shard_result r;
    CHECK(bpp_prove_status_result(&got_s[i], &r) == BPP_OK);
    printf("record_%zu %d %u '%s'\n", i, r.code, got_s[i].msg, r.msg);
  }
  print_hex("proof_0", got_p.data(), lens_d[0]);

  // the outputs go into the verifier where they lie
  bpp_mixed_batch dev;
  memset(&dev, 0, sizeof(dev));
  dev.n_items = N;
  dev.proofs = d_proofs;
  dev.proof_stride = STRIDE;
  dev.proof_lens = lens_d.data();
  dev.m = m.data();
  dev.m_stride = (uint32_t)M_STRIDE;
  dev.commitments32 = d_commit;
  dev.min_values = in.min_values;
  dev.min_present = in.min_present;
  dev.seed_nonces32 = in.seed_nonces32;
  dev.seed_present = in.seed_present;
  dev.transcript_label = (const uint8_t *)label.data();
  dev.label_len = label.size();
  std::vector<uint8_t> masks(32 * N), pres(N);
  const int rc_v = bpp_verify_batch_mixed_device(ctx, params->handle(), &dev, BPP_RECOVER_AND_VERIFY, 0, masks.data(), pres.data(), err, sizeof(err));
  printf("verify_code %d %s\n", rc_v, err);
  print_hex("present", pres.data(), N);
  for (size_t i = 0; i < N; i++)
    if (ms[i] == 1) CHECK(pres[i] == 1 && memcmp(&masks[32 * i], &blindings[32 * i * M_STRIDE], 32) == 0);  // the blinding the prover was given

  // the overload of bpp.hpp: the same bytes again; a finding stays with its item and does not throw; a refusal throws
  CHECK(hipMemset(d_proofs, 0xff, N * STRIDE) == hipSuccess && hipMemset(d_commit, 0xff, N * CSTRIDE) == hipSuccess);
  const DeviceProveOutputs out{d_commit, CSTRIDE, d_proofs, STRIDE, d_status};
  const DeviceProveResult res = RangeProof::prove_openings(DeviceProveArrays{in}, out, params);
  CHECK(hipMemcpy(got_p.data(), d_proofs, got_p.size(), hipMemcpyDeviceToHost) == hipSuccess);
  printf("hpp_code %d\nhpp_proofs_equal %d\n", res.code, (int)(got_p == proofs && res.proof_lens == lens));
  std::vector<uint64_t> bad_v = values;
  bad_v[2 * M_STRIDE + 3] = 1ull << 8;  // item 2's last value: over the capacity of 8 bits
  bpp_prove_arrays bad = in;
  bad.values = to_device(bad_v);
  const DeviceProveResult res_bad = RangeProof::prove_openings(DeviceProveArrays{bad}, out, params);
  printf("hpp_finding %d %d%d%d%d%d '%s'\n", res_bad.code, res_bad.item_status[0], res_bad.item_status[1], res_bad.item_status[2],
         res_bad.item_status[3], res_bad.item_status[4], res_bad.message.c_str());
  bpp_prove_arrays refused = in;
  refused.values = values.data();  // host memory
  std::string what;
  try {
    RangeProof::prove_openings(DeviceProveArrays{refused}, out, params);
  } catch (const ProofError &e) {
    what = std::to_string((int)e.kind) + " " + e.what();
  }
  printf("hpp_refusal %s\n", what.c_str());
  struct bpp_prove_device_stats st;
  CHECK(bpp_prove_device_stats(ctx, &st) == BPP_OK);
  printf("stats %llu %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.items, (unsigned long long)st.device_findings,
         (unsigned long long)st.host_findings);
  uint64_t examined = 0, nonzero = 1;
  CHECK(bpp_prove_secret_bytes(ctx, &examined, &nonzero) == BPP_OK && examined > 0 && nonzero == 0);
  printf("prove_device_inputs ok\n");
  return 0;
}
