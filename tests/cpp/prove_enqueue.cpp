// A compiled caller of bpp_prove_plan_create / bpp_prove_enqueue (include/bpp.h) through Engine::prove_plan_create, Engine::ProvePlan
// and Engine::prove_enqueue of include/bpp.hpp, with arrays it allocated itself with hipMalloc -- no torch, no ctypes declarations that
// could hide a wrong prototype.  Four items (n = 8, m = 2, 1, 1, 1, t = 1), every one under a transcript of its own.
//   PARITY: an enqueue on a plan with per-item transcripts writes, byte for byte over whole buffers prefilled with 0xff, what the
//   blocking RangeProof::prove_openings over the same DeviceProveArrays writes: commitments, proofs, status records, state rows.
//   THE LOOP: prove_enqueue (one item fails on a blinding factor, one is switched off by the live mask) -> batch_refill_enqueue_mixed
//   with live_dev = the prover's ok mask -> verify_enqueue_states, on the engine's stream with no wait and no copy to the host in
//   between; only the last ticket is waited for.  The group must be Ok, the two enqueue paths must report zero host waits.
// Prints "prove_enqueue ok" at the end; tests/test_gpu_cpp_prove_enqueue.py builds and runs it.
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

template <typename T>
static T *to_device(const std::vector<T> &v) {
  void *d = nullptr;
  CHECK(hipMalloc(&d, v.size() * sizeof(T)) == hipSuccess);
  CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  return reinterpret_cast<T *>(d);
}
template <typename T>
static std::vector<T> to_host(const T *d, size_t n) {
  std::vector<T> v(n);
  CHECK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
  return v;
}

static const size_t N = 4, M_STRIDE = 4, ROW = 203, STRIDE = 1 + 32 * (1 + 5 + 2 * 4) + 3, CSTRIDE = 32 * M_STRIDE, RNG = 32 * 7 + 5;
static const uint32_t MS[N] = {2, 1, 1, 1};

struct Outputs {
  uint8_t *commit, *proofs, *states, *ok;
  bpp_device_prove_status *status;
  bpp_device_prove_summary *summary;
  Outputs() {
    commit = to_device(std::vector<uint8_t>(N * CSTRIDE, 0xff));
    proofs = to_device(std::vector<uint8_t>(N * STRIDE, 0xff));
    states = to_device(std::vector<uint8_t>(N * ROW, 0xff));
    ok = to_device(std::vector<uint8_t>(N, 0xff));
    status = to_device(std::vector<bpp_device_prove_status>(N, bpp_device_prove_status{-1, 99}));
    summary = to_device(std::vector<bpp_device_prove_summary>(1, bpp_device_prove_summary{-1, 99, 99, 0, 99, 99, 99, 99}));
  }
};

// the openings of one step; `salt` varies the values, `bad` (or N) is an item whose first blinding factor is not canonical
static bpp_prove_arrays openings(uint32_t salt, size_t bad, const std::vector<uint32_t> &m) {
  std::vector<uint64_t> values(N * M_STRIDE, ~0ull);  // row slack holds what would be a finding if it were read
  std::vector<uint8_t> blindings(32 * N * M_STRIDE, 0xff), ext(N * RNG, 0xff);
  for (size_t i = 0; i < N; i++) {
    for (size_t j = 0; j < MS[i]; j++) {
      values[i * M_STRIDE + j] = (10 * i + j + 1 + salt) & 0xff;
      for (size_t k = 0; k < 32; k++) blindings[32 * (i * M_STRIDE + j) + k] = (i == bad) ? 0xff : (k < 31 ? (uint8_t)(7 * i + 3 * j + k + 1 + salt) : 0);
    }
    const size_t need = 32 * (size_t)(3 + 3 + (MS[i] > 1));
    for (size_t k = 0; k < need; k++) ext[i * RNG + k] = (uint8_t)(31 * i + 5 * k + 3 + salt);
  }
  bpp_prove_arrays a;
  memset(&a, 0, sizeof(a));
  a.n_items = N;
  a.m = m.data();
  a.m_stride = (uint32_t)M_STRIDE;
  a.values = to_device(values);
  a.blindings32 = to_device(blindings);
  a.rng_bytes = to_device(ext);
  a.rng_stride = RNG;
  return a;
}

int main() {
  Engine eng(0);
  bpp_ctx *ctx = eng.ctx();
  auto params = RangeParameters::init(eng, 8, 4, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  const std::string label = "prove enqueue", ctx_label = "tx";
  const std::vector<uint32_t> m(MS, MS + N);
  std::vector<uint8_t> rows(N * ROW, 0);
  for (size_t i = 0; i < N; i++) {
    std::vector<uint8_t> context(5 + 11 * i, (uint8_t)(i + 1));
    CHECK(bpp_transcript_new((const uint8_t *)label.data(), label.size(), &rows[i * ROW]) == BPP_OK);
    CHECK(bpp_transcript_append_message(&rows[i * ROW], (const uint8_t *)ctx_label.data(), ctx_label.size(), context.data(), context.size()) == BPP_OK);
  }
  const uint8_t *d_rows = to_device(rows);

  // ---- the plan: the shape alone
  DeviceProveArrays first;
  first.arrays = openings(0, N, m);
  Engine::ProvePlan plan = eng.prove_plan_create(params->handle(), first.arrays, CSTRIDE, STRIDE, BPP_PROVE_PLAN_ITEM_STATES);
  std::vector<int> host_status;
  const std::vector<size_t> lens = plan.proof_lens(&host_status);
  CHECK(plan.n_items() == N && lens.size() == N);

  // ---- parity with the blocking call on the same arrays
  Outputs want, got;
  const DeviceProveOutputs blocking_out{want.commit, CSTRIDE, want.proofs, STRIDE, want.status};
  const DeviceProveResult ref = RangeProof::prove_openings(first, d_rows, blocking_out, want.states, params);
  CHECK(ref.code == BPP_OK);
  for (size_t i = 0; i < N; i++) CHECK(lens[i] == ref.proof_lens[i] && host_status[i] == 0);
  Engine::ProveEnqueueOutputs out;
  out.commitments = got.commit, out.proofs = got.proofs, out.states = got.states, out.status = got.status, out.ok_mask = got.ok, out.summary = got.summary;
  bpp_prove_arrays steady = first.arrays;
  steady.m = nullptr;  // the plan's own
  auto ticket = eng.prove_enqueue(plan, steady, out, d_rows);
  ticket.wait();
  CHECK(ticket.done());
  CHECK(to_host(got.commit, N * CSTRIDE) == to_host(want.commit, N * CSTRIDE));
  CHECK(to_host(got.proofs, N * STRIDE) == to_host(want.proofs, N * STRIDE));
  CHECK(to_host(got.states, N * ROW) == to_host(want.states, N * ROW));
  {
    const auto a = to_host(got.status, N), b = to_host(want.status, N);
    for (size_t i = 0; i < N; i++) CHECK(a[i].code == b[i].code && a[i].msg == b[i].msg && a[i].msg == BPP_PROVE_MSG_OK);
    const auto ok = to_host(got.ok, N);
    for (size_t i = 0; i < N; i++) CHECK(ok[i] == 1);
    const bpp_device_prove_summary s = to_host(got.summary, 1)[0];
    CHECK(s.code == 0 && s.msg == 0 && s.index == 0 && s.flags == BPP_PROVE_SUMMARY_WRITTEN && s.n_ok == N && s.n_failed == 0 && s.n_empty == 0);
    bpp_shard_result r;
    CHECK(bpp_prove_summary_result(&s, &r) == BPP_OK && r.code == 0 && r.msg[0] == 0);
  }
  printf("parity ok\n");

  // ---- a refusal throws and names the field
  std::string what;
  try {
    eng.prove_enqueue(plan, steady, out, nullptr);
  } catch (const ProofError &e) {
    what = std::to_string((int)e.kind) + " " + e.what();
  }
  printf("refusal %s\n", what.c_str());
  CHECK(what.find("item_states_dev") != std::string::npos);

  // ---- the loop: the resident batch first holds the outputs above; then one step without a wait in its middle
  bpp_mixed_batch dev;
  memset(&dev, 0, sizeof(dev));
  dev.n_items = N;
  dev.proofs = got.proofs;
  dev.proof_stride = STRIDE;
  dev.proof_lens = lens.data();
  dev.m = m.data();
  dev.m_stride = (uint32_t)M_STRIDE;
  dev.commitments32 = got.commit;
  char err[256] = {0};
  uint64_t h = 0;
  CHECK(bpp_batch_upload_mixed_device_transcripts(ctx, params->handle(), &dev, d_rows, &h, err, sizeof(err)) == BPP_OK);
  bpp_device_verdict *d_verdict = to_device(std::vector<bpp_device_verdict>(1));
  uint8_t *d_verified = to_device(std::vector<uint8_t>(N * ROW, 0xee));
  bpp_device_refill *d_record = to_device(std::vector<bpp_device_refill>(1));
  bpp_mixed_batch refill = dev;
  refill.proof_lens = nullptr, refill.m = nullptr;  // the batch's own
  // (a first round with every item live: the batch's first refill under a mask and its layout are made here)
  const uint8_t *d_all = to_device(std::vector<uint8_t>(N, 1));
  eng.batch_refill_enqueue_mixed(h, refill, d_rows, nullptr, d_all, d_record);
  eng.verify_enqueue_states(h, nullptr, 1, 0, nullptr, VerifyAction::VerifyOnly, d_verdict, d_verified).wait();

  const bpp_prove_arrays step = [&] {
    bpp_prove_arrays a = openings(40, 3, m);  // item 3 fails
    a.m = nullptr;
    return a;
  }();
  const uint8_t *d_live = to_device(std::vector<uint8_t>{1, 0, 7, 1});  // item 1 is switched off
  const auto p0 = eng.prove_enqueue_stats();
  const auto r0 = eng.refill_stats();
  const auto e0 = eng.enqueue_stats();
  auto proved = eng.prove_enqueue(plan, step, out, d_rows, d_live);
  auto filled = eng.batch_refill_enqueue_mixed(h, refill, d_rows, nullptr, got.ok, d_record);
  auto checked = eng.verify_enqueue_states(h, nullptr, 1, 0, nullptr, VerifyAction::VerifyOnly, d_verdict, d_verified);
  const auto p1 = eng.prove_enqueue_stats();
  const auto r1 = eng.refill_stats();
  const auto e1 = eng.enqueue_stats();
  checked.wait();  // the one wait of the step
  CHECK(p1.host_waits == 0 && p1.calls == p0.calls + 1 && p1.allocations == p0.allocations && p1.first_calls == p0.first_calls);
  CHECK(r1.host_waits == r0.host_waits && e1.host_waits == e0.host_waits);
  CHECK(proved.done() && filled.done());
  {
    const auto ok = to_host(got.ok, N);
    printf("ok_mask %d%d%d%d\n", ok[0], ok[1], ok[2], ok[3]);
    CHECK(ok[0] == 1 && ok[1] == 0 && ok[2] == 1 && ok[3] == 0);
    const auto st = to_host(got.status, N);
    CHECK(st[1].code == 0 && st[1].msg == BPP_PROVE_MSG_EMPTY && st[3].msg == BPP_PROVE_MSG_BLINDING && st[0].msg == 0 && st[2].msg == 0);
    const bpp_device_prove_summary s = to_host(got.summary, 1)[0];
    bpp_shard_result r;
    CHECK(bpp_prove_summary_result(&s, &r) == BPP_OK);
    printf("summary %d %u %u %u %u '%s'\n", s.code, s.index, s.n_ok, s.n_failed, s.n_empty, r.msg);
    CHECK(s.index == 3 && s.n_ok == 2 && s.n_failed == 1 && s.n_empty == 1 && r.code == s.code && r.index == 3);
    const auto proofs = to_host(got.proofs, N * STRIDE), states = to_host(got.states, N * ROW);
    for (size_t i : {(size_t)1, (size_t)3}) {
      for (size_t b = 0; b < lens[i]; b++) CHECK(proofs[i * STRIDE + b] == 0);
      for (size_t b = 0; b < ROW; b++) CHECK(states[i * ROW + b] == 0);
    }
    bpp_device_verdict v = to_host(d_verdict, 1)[0];
    const std::vector<bpp_shard_result> verdicts = checked.results(&v);
    printf("verify_code %d '%s'\n", verdicts[0].code, verdicts[0].msg);
    CHECK(verdicts[0].code == BPP_OK);
    const auto verified = to_host(d_verified, N * ROW);
    for (size_t i = 0; i < N; i++) {
      bool nonzero = false;
      for (size_t b = 0; b < ROW; b++) nonzero = nonzero || verified[i * ROW + b] != 0;
      CHECK(nonzero == (i == 0 || i == 2));  // the verifier's rows: advanced for the live slots, zero for the others
    }
  }
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  uint64_t examined = 0, nonzero = 1;
  CHECK(bpp_prove_secret_bytes(ctx, &examined, &nonzero) == BPP_OK && examined > 0 && nonzero == 0);
  plan.reset();
  CHECK(plan.handle() == 0);
  printf("prove_enqueue ok\n");
  return 0;
}
