// A compiled caller of bpp_rows_msm_enqueue and bpp_rows_scalar_enqueue (include/bpp.h) through Engine::rows_msm_enqueue and
// Engine::rows_scalar_enqueue of include/bpp.hpp, with arrays it allocated itself with hipMalloc -- no torch, no ctypes declarations that
// could hide a wrong prototype.  The commit / challenge / response step of a Schnorr proof of knowledge of x (X = x G) around a
// transcript, nine rows on the engine's stream with one wait at the end; row 4 is dead, row 6 has the identity as its X and is void
// from the APPEND_POINT on:
//   call 1: NEW("cpp rows step") + APPEND("txid") + RNG_BEGIN / RNG_REKEY("x") / RNG_FINALIZE(NullRng) / RNG_SCALARS(1) -> r
//   call 2: rows_msm_enqueue, K = 1, the shared base G                                                                  -> R = r G
//   call 3: APPEND_POINT("X"), APPEND_POINT("R"), CHALLENGE_SCALAR("c")                                                 -> c
//   call 4: rows_scalar_enqueue(c, x, r) under call 3's done mask                                                       -> s = c x + r
// The program holds r, c and the transcript rows to the host helpers of include/bpp.h, R to bpp_msm_ct, and checks s G == R + c X per
// row through bpp_msm_ct; it prints the records and the counters, which tests/test_gpu_cpp_rows_msm.py reads.
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
static T *to_device(const std::vector<T> &v, size_t skew = 0) {
  void *d = nullptr;
  CHECK(hipMalloc(&d, v.size() * sizeof(T) + skew) == hipSuccess);
  CHECK(hipMemcpy((uint8_t *)d + skew, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  return reinterpret_cast<T *>((uint8_t *)d + skew);
}
template <typename T>
static std::vector<T> to_host(const T *d, size_t count) {
  std::vector<T> v(count);
  CHECK(hipMemcpy(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
  return v;
}
static const uint8_t *bytes(const std::string &s) { return (const uint8_t *)s.data(); }

// the Ristretto basepoint's encoding
static const uint8_t kG[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                               0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};

int main() {
  Engine eng(0);
  const size_t N = 9, ROW = 203, DEAD = 4, IDENT = 6, TXID = 24, X_STRIDE = 35;
  const std::string proto = "cpp rows step", l_t = "txid", l_x = "x", l_X = "X", l_R = "R", l_c = "c";
  uint8_t live[N];
  std::vector<uint8_t> x(N * X_STRIDE, 0xee), X(N * 32), txid(N * TXID);
  for (size_t i = 0; i < N; i++) {
    live[i] = i == DEAD ? 0 : 1;
    for (size_t k = 0; k < 32; k++) x[i * X_STRIDE + k] = (uint8_t)(i == IDENT ? 0 : 37 * i + 5 * k + 1);
    x[i * X_STRIDE + 31] &= 0x0f;  // canonical
    for (size_t k = 0; k < TXID; k++) txid[i * TXID + k] = (uint8_t)(13 * i + 3 * k + 7);
    CHECK(bpp_msm_ct(eng.ctx(), &x[i * X_STRIDE], kG, 1, &X[i * 32]) == BPP_OK);
  }
  for (size_t k = 0; k < 32; k++) CHECK(X[IDENT * 32 + k] == 0);
  uint8_t *d_rows = to_device(std::vector<uint8_t>(3 + N * ROW, 0xee)) + 3;
  const uint8_t *d_x = to_device(x, 1), *d_X = to_device(X), *d_txid = to_device(txid, 1), *d_G = to_device(std::vector<uint8_t>(kG, kG + 32), 1);
  const uint8_t *d_live = to_device(std::vector<uint8_t>(live, live + N));
  uint8_t *d_r = to_device(std::vector<uint8_t>(N * 32, 0xff), 1), *d_R = to_device(std::vector<uint8_t>(N * 33, 0xff), 1);
  uint8_t *d_c = to_device(std::vector<uint8_t>(N * 32, 0xff)), *d_s = to_device(std::vector<uint8_t>(N * 32, 0xff), 3);
  uint8_t *d_done = to_device(std::vector<uint8_t>(3 * N, 0xa5));
  bpp_device_transcripts_record *d_trec = to_device(std::vector<bpp_device_transcripts_record>(1, bpp_device_transcripts_record{9, 9, 9, 9}));
  bpp_device_rows_record *d_rec = to_device(std::vector<bpp_device_rows_record>(2, bpp_device_rows_record{9, 9, 9, 9}));
  CHECK(((uintptr_t)d_x & 1) == 1 && ((uintptr_t)d_r & 1) == 1 && ((uintptr_t)d_R & 1) == 1 && ((uintptr_t)d_s & 3) == 3);

  auto t1 = eng.transcripts_enqueue(d_rows, N,
                                    {Engine::op_new(bytes(proto), (uint32_t)proto.size()),
                                     Engine::op_append(bytes(l_t), (uint32_t)l_t.size(), d_txid, TXID), Engine::op_rng_begin(),
                                     Engine::op_rng_rekey(bytes(l_x), (uint32_t)l_x.size(), d_x, 32, X_STRIDE), Engine::op_rng_finalize(),
                                     Engine::op_rng_scalars(d_r, 1)},
                                    d_live);
  bpp_rows_msm in{};
  in.n = N, in.K = 1, in.scalars_dev = d_r, in.scalar_stride = 32, in.points_dev = d_G, in.point_stride = 0;
  auto t2 = eng.rows_msm_enqueue(in, d_R, 33, d_live, d_done, d_rec);
  auto t3 = eng.transcripts_enqueue(d_rows, N,
                                    {Engine::op_append_point(bytes(l_X), (uint32_t)l_X.size(), d_X),
                                     Engine::op_append_point(bytes(l_R), (uint32_t)l_R.size(), d_R, 33),
                                     Engine::op_challenge_scalar(bytes(l_c), (uint32_t)l_c.size(), d_c)},
                                    d_live, d_done + N, d_trec);
  const bpp_scalar_rows a{d_c, 32}, b{d_x, X_STRIDE}, c{d_r, 32};
  auto t4 = eng.rows_scalar_enqueue(N, a, b, &c, d_s, 32, d_done + N, d_done + 2 * N, d_rec + 1);
  t4.wait();  // the one wait
  CHECK(t1.done() && t2.done() && t3.done() && t4.done());

  const std::vector<uint8_t> rows = to_host(d_rows, N * ROW), r = to_host(d_r, N * 32), R = to_host(d_R, N * 33), cc = to_host(d_c, N * 32),
                             s = to_host(d_s, N * 32), done = to_host(d_done, 3 * N);
  const std::vector<bpp_device_rows_record> rec = to_host(d_rec, 2);
  const std::vector<bpp_device_transcripts_record> trec = to_host(d_trec, 1);
  size_t verified = 0, void_rows = 0;
  const uint8_t zero[32] = {0};
  for (size_t i = 0; i < N; i++) {
    if (!live[i]) {  // dead: the row untouched, every output zero
      for (size_t k = 0; k < ROW; k++) CHECK(rows[i * ROW + k] == 0xee);
      CHECK(!memcmp(&r[i * 32], zero, 32) && !memcmp(&R[i * 33], zero, 32) && !memcmp(&cc[i * 32], zero, 32) && !memcmp(&s[i * 32], zero, 32));
      CHECK(done[i] == 0 && done[N + i] == 0 && done[2 * N + i] == 0);
      continue;
    }
    CHECK(R[i * 33 + 32] == 0xff);  // the slack of the output rows
    uint8_t want[ROW], rng[ROW], want_r[32], want_R[32], want_c[32];
    char err[128] = {0};
    CHECK(bpp_transcript_new(bytes(proto), proto.size(), want) == BPP_OK);
    CHECK(bpp_transcript_append_message(want, bytes(l_t), l_t.size(), &txid[i * TXID], TXID) == BPP_OK);
    CHECK(bpp_transcript_rng_begin(want, rng) == BPP_OK);
    CHECK(bpp_transcript_rng_rekey(rng, bytes(l_x), l_x.size(), &x[i * X_STRIDE], 32) == BPP_OK);
    CHECK(bpp_transcript_rng_finalize(rng, nullptr) == BPP_OK);
    CHECK(bpp_transcript_rng_scalar(rng, want_r, err, sizeof(err)) == BPP_OK);
    CHECK(!memcmp(&r[i * 32], want_r, 32));
    CHECK(bpp_msm_ct(eng.ctx(), want_r, kG, 1, want_R) == BPP_OK);
    CHECK(!memcmp(&R[i * 33], want_R, 32) && done[i] == 1);
    const int rc = bpp_transcript_validate_and_append_point(want, bytes(l_X), l_X.size(), &X[i * 32], err, sizeof(err));
    if (i == IDENT) {  // void from here on: the row, the challenge and the response are zero
      CHECK(rc == BPP_ERR_VERIFICATION_FAILED);
      for (size_t k = 0; k < ROW; k++) CHECK(rows[i * ROW + k] == 0);
      CHECK(!memcmp(&cc[i * 32], zero, 32) && !memcmp(&s[i * 32], zero, 32) && done[N + i] == 0 && done[2 * N + i] == 0);
      void_rows++;
      continue;
    }
    CHECK(rc == BPP_OK);
    CHECK(bpp_transcript_validate_and_append_point(want, bytes(l_R), l_R.size(), want_R, err, sizeof(err)) == BPP_OK);
    CHECK(bpp_transcript_challenge_scalar(want, bytes(l_c), l_c.size(), want_c, err, sizeof(err)) == BPP_OK);
    CHECK(!memcmp(&rows[i * ROW], want, ROW) && !memcmp(&cc[i * 32], want_c, 32) && done[N + i] == 1 && done[2 * N + i] == 1);
    // s G == R + c X
    uint8_t lhs[32], rhs[32], sc2[64] = {1}, pt2[64];
    memcpy(sc2 + 32, want_c, 32);
    memcpy(pt2, want_R, 32);
    memcpy(pt2 + 32, &X[i * 32], 32);
    CHECK(bpp_msm_ct(eng.ctx(), &s[i * 32], kG, 1, lhs) == BPP_OK);
    CHECK(bpp_msm_ct(eng.ctx(), sc2, pt2, 2, rhs) == BPP_OK);
    CHECK(!memcmp(lhs, rhs, 32) && memcmp(lhs, zero, 32));
    verified++;
  }
  printf("responses_verified %zu\n", verified);
  printf("void_rows_all_zero %zu\n", void_rows);
  printf("record_msm %u %u %u %u\n", rec[0].n_done, rec[0].n_void, rec[0].first_void, rec[0].flags);
  printf("record_transcripts %u %u %u %u\n", trec[0].n_done, trec[0].n_void, trec[0].first_void, trec[0].flags);
  printf("record_scalar %u %u %u %u\n", rec[1].n_done, rec[1].n_void, rec[1].first_void, rec[1].flags);

  std::string what;
  try {
    eng.rows_scalar_enqueue(N, a, b, &c, d_r, 32);  // out aliases c
  } catch (const ProofError &err) {
    what = std::to_string((int)err.kind) + " " + err.what();
  }
  printf("refusal %s\n", what.c_str());
  const struct bpp_rows_stats st = eng.rows_stats();
  printf("stats %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.first_calls, (unsigned long long)st.host_waits);
  printf("rows_msm ok\n");
  return 0;
}
