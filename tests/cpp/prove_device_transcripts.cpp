// A compiled caller of bpp_prove_openings_device_transcripts (include/bpp.h) through the overload of RangeProof::prove_openings over
// a DeviceProveArrays that takes the two device pointers (include/bpp.hpp), with arrays it allocated itself with hipMalloc -- no
// torch, no ctypes declarations that could hide a wrong prototype.  Three items (n = 8, m = 2, 1, 1, t = 1), every one under a
// transcript of its own: bpp_transcript_new plus one bpp_transcript_append_message whose length differs from item to item.  The rows
// going in start one byte into their allocation, the rows coming out three.  The program prints the commitments, the proofs and the
// advanced transcripts, which tests/test_gpu_cpp_prove_device_transcripts.py compares with bpp_prove_openings_states on the same
// openings; the outputs then go, where they lie and under the rows they continued, into bpp_batch_upload_mixed_device_transcripts and
// Engine::verify_enqueue_states, which must accept them.  Every input byte is a formula the test repeats.
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

static void print_hex(const char *name, size_t i, const uint8_t *p, size_t n) {
  printf("%s_%zu ", name, i);
  for (size_t k = 0; k < n; k++) printf("%02x", p[k]);
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
  const std::string label = "prove device transcripts", ctx_label = "tx";
  const size_t N = 3, M_STRIDE = 4, ROW = 203, STRIDE = 1 + 32 * (1 + 5 + 2 * 4) + 3, CSTRIDE = 32 * M_STRIDE, RNG = 32 * 7 + 5;
  const uint32_t ms[N] = {2, 1, 1};
  std::vector<uint64_t> values(N * M_STRIDE, ~0ull);  // row slack holds what would be a finding if it were read
  std::vector<uint8_t> blindings(32 * N * M_STRIDE, 0xff), ext(N * RNG, 0xff), rows(N * ROW, 0);
  std::vector<uint32_t> m(ms, ms + N);
  for (size_t i = 0; i < N; i++) {
    for (size_t j = 0; j < ms[i]; j++) {
      values[i * M_STRIDE + j] = 10 * i + j + 1;
      for (size_t k = 0; k < 32; k++) blindings[32 * (i * M_STRIDE + j) + k] = k < 31 ? (uint8_t)(7 * i + 3 * j + k + 1) : 0;
    }
    const size_t need = 32 * (size_t)(3 + 3 + (ms[i] > 1));
    for (size_t k = 0; k < need; k++) ext[i * RNG + k] = (uint8_t)(31 * i + 5 * k + 3);
    std::vector<uint8_t> context(5 + 11 * i, (uint8_t)(i + 1));
    CHECK(bpp_transcript_new((const uint8_t *)label.data(), label.size(), &rows[i * ROW]) == BPP_OK);
    CHECK(bpp_transcript_append_message(&rows[i * ROW], (const uint8_t *)ctx_label.data(), ctx_label.size(), context.data(), context.size()) == BPP_OK);
  }
  for (size_t i = 1; i < N; i++) CHECK(rows[i * ROW + 200] != rows[(i - 1) * ROW + 200]);  // the rows' pos differ

  DeviceProveArrays in;
  memset(&in.arrays, 0, sizeof(in.arrays));
  in.arrays.n_items = N;
  in.arrays.m = m.data();
  in.arrays.m_stride = (uint32_t)M_STRIDE;
  in.arrays.values = to_device(values);
  in.arrays.blindings32 = to_device(blindings);
  in.arrays.rng_bytes = to_device(ext);
  in.arrays.rng_stride = RNG;
  const uint8_t *d_rows = to_device(rows, 1);
  uint8_t *d_commit = to_device(std::vector<uint8_t>(N * CSTRIDE, 0xff)), *d_proofs = to_device(std::vector<uint8_t>(N * STRIDE, 0xff));
  uint8_t *d_states = to_device(std::vector<uint8_t>(3 + N * ROW + 13, 0xee)) + 3;
  bpp_device_prove_status *d_status = to_device(std::vector<bpp_device_prove_status>(N, bpp_device_prove_status{-1, 99}));
  CHECK(((uintptr_t)d_rows & 1) == 1 && ((uintptr_t)d_states & 3) == 3);
  const DeviceProveOutputs out{d_commit, CSTRIDE, d_proofs, STRIDE, d_status};
  const DeviceProveResult res = RangeProof::prove_openings(in, d_rows, out, d_states, params);
  printf("code %d '%s'\n", res.code, res.message.c_str());
  std::vector<uint8_t> got_c(N * CSTRIDE), got_p(N * STRIDE), got_s(3 + N * ROW + 13);
  CHECK(hipMemcpy(got_c.data(), d_commit, got_c.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(got_p.data(), d_proofs, got_p.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(got_s.data(), d_states - 3, got_s.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (int b = 0; b < 3; b++) CHECK(got_s[b] == 0xee);                  // the bytes in front of the rows
  for (int b = 0; b < 13; b++) CHECK(got_s[3 + N * ROW + b] == 0xee);  // ... and behind them
  for (size_t i = 0; i < N; i++) {
    CHECK(res.item_status[i] == BPP_OK);
    print_hex("commitments", i, &got_c[i * CSTRIDE], 32 * ms[i]);
    print_hex("proof", i, &got_p[i * STRIDE], res.proof_lens[i]);
    print_hex("state", i, &got_s[3 + i * ROW], ROW);
  }

  // a row whose pos is at the rate is its item's finding and does not throw; rows together with a label are refused and throw
  std::vector<uint8_t> bad_rows = rows;
  memset(&bad_rows[1 * ROW], 0xff, ROW);
  bad_rows[1 * ROW + 200] = 166;
  const DeviceProveResult res_bad = RangeProof::prove_openings(in, to_device(bad_rows, 1), out, d_states, params);
  printf("finding %d %d%d%d '%s'\n", res_bad.code, res_bad.item_status[0], res_bad.item_status[1], res_bad.item_status[2], res_bad.message.c_str());
  CHECK(hipMemcpy(got_s.data(), d_states - 3, got_s.size(), hipMemcpyDeviceToHost) == hipSuccess);
  bool zero = true;
  for (size_t b = 0; b < ROW; b++) zero = zero && got_s[3 + ROW + b] == 0;
  printf("finding_row_zero %d\n", (int)zero);
  DeviceProveArrays labelled = in;
  labelled.arrays.transcript_label = (const uint8_t *)label.data();
  labelled.arrays.label_len = label.size();
  std::string what;
  try {
    RangeProof::prove_openings(labelled, d_rows, out, d_states, params);
  } catch (const ProofError &e) {
    what = std::to_string((int)e.kind) + " " + e.what();
  }
  printf("refusal %s\n", what.c_str());

  // the outputs of the first call again, and into the verifier where they lie, every proof under the row it continued
  const DeviceProveResult again = RangeProof::prove_openings(in, d_rows, out, d_states, params);
  CHECK(again.code == BPP_OK);
  bpp_mixed_batch dev;
  memset(&dev, 0, sizeof(dev));
  dev.n_items = N;
  dev.proofs = d_proofs;
  dev.proof_stride = STRIDE;
  dev.proof_lens = again.proof_lens.data();
  dev.m = m.data();
  dev.m_stride = (uint32_t)M_STRIDE;
  dev.commitments32 = d_commit;
  char err[256] = {0};
  uint64_t h = 0;
  const int rc_u = bpp_batch_upload_mixed_device_transcripts(ctx, params->handle(), &dev, d_rows, &h, err, sizeof(err));
  printf("upload_code %d %s\n", rc_u, err);
  CHECK(rc_u == BPP_OK);
  bpp_device_verdict *d_verdict = to_device(std::vector<bpp_device_verdict>(1));
  uint8_t *d_verified = to_device(std::vector<uint8_t>(N * ROW, 0xee));
  auto ticket = eng.verify_enqueue_states(h, nullptr, 1, 0, nullptr, VerifyAction::VerifyOnly, d_verdict, d_verified);
  ticket.wait();
  bpp_device_verdict v;
  CHECK(hipMemcpy(&v, d_verdict, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess);
  const std::vector<bpp_shard_result> verdicts = ticket.results(&v);
  printf("verify_code %d '%s'\n", verdicts[0].code, verdicts[0].msg);
  std::vector<uint8_t> verified(N * ROW);
  CHECK(hipMemcpy(verified.data(), d_verified, verified.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(got_s.data(), d_states - 3, got_s.size(), hipMemcpyDeviceToHost) == hipSuccess);
  bool advanced = true;  // (the verifier appends r1, s1 and d1: its rows are neither zero nor the prover's)
  for (size_t i = 0; i < N; i++) {
    bool nonzero = false;
    for (size_t b = 0; b < ROW; b++) nonzero = nonzero || verified[i * ROW + b] != 0;
    advanced = advanced && nonzero && memcmp(&verified[i * ROW], &got_s[3 + i * ROW], ROW) != 0;
  }
  printf("verifier_rows_advanced %d\n", (int)advanced);
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  struct bpp_prove_device_stats st;
  CHECK(bpp_prove_device_stats(ctx, &st) == BPP_OK);
  printf("stats %llu %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.items, (unsigned long long)st.device_findings,
         (unsigned long long)st.host_findings);
  uint64_t examined = 0, nonzero = 1;
  CHECK(bpp_prove_secret_bytes(ctx, &examined, &nonzero) == BPP_OK && examined > 0 && nonzero == 0);
  printf("prove_device_transcripts ok\n");
  return 0;
}
