// A compiled caller of the transcript-protocol and transcript-RNG kinds of bpp_transcripts_enqueue (include/bpp.h) through
// Engine::transcripts_enqueue and the op builders of include/bpp.hpp, with arrays it allocated itself with hipMalloc -- no torch, no
// ctypes declarations that could hide a wrong prototype.  Eight rows under a live mask (rows 2 and 5 dead), the rows starting three
// bytes into their allocation:
//   call 1: NEW("cpp transcript rng") + APPEND_POINT("P", 32 bytes of row i, rows 33 bytes apart; row 6's point is the identity's
//           encoding and the row becomes void)
//   call 2: RNG_BEGIN, RNG_REKEY("witness", 40 bytes), RNG_FINALIZE(32 bytes of entropy), RNG_FILL32(96), RNG_SCALARS(5),
//           CHALLENGE_SCALAR("e")   (row 6, 203 zero bytes by now, stays void)
// The program holds every row and every output to the host helpers -- bpp_transcript_validate_and_append_point, _rng_begin,
// _rng_rekey, _rng_finalize, _rng_fill, _rng_scalar, _challenge_scalar, and their wrappers on bpp_host::Transcript -- on a host copy,
// the dead rows to the 0xEE they held, and prints the records and the counters, which tests/test_gpu_cpp_transcript_rng.py reads.
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

int main() {
  Engine eng(0);
  const size_t N = 8, ROW = 203, PT_STRIDE = 33, WIT = 40, FILL = 96, SCALARS = 5;
  const std::string proto = "cpp transcript rng", l_p = "P", l_w = "witness", l_e = "e";
  const uint8_t live[N] = {1, 1, 0, 1, 1, 0, 1, 1};
  std::vector<uint8_t> points(N * PT_STRIDE, 0xee), wit(N * WIT), ent(N * 32);
  for (size_t i = 0; i < N; i++) {
    for (size_t k = 0; k < 32; k++) points[i * PT_STRIDE + k] = (uint8_t)(i == 6 ? 0 : 17 * i + 3 * k + 1);
    for (size_t k = 0; k < WIT; k++) wit[i * WIT + k] = (uint8_t)(29 * i + 7 * k + 2);
    for (size_t k = 0; k < 32; k++) ent[i * 32 + k] = (uint8_t)(31 * i + 11 * k + 5);
  }
  uint8_t *d_rows = to_device(std::vector<uint8_t>(3 + N * ROW + 5, 0xee)) + 3;
  const uint8_t *d_points = to_device(points, 1), *d_wit = to_device(wit), *d_ent = to_device(ent, 1);
  const uint8_t *d_live = to_device(std::vector<uint8_t>(live, live + N));
  uint8_t *d_fill = to_device(std::vector<uint8_t>(N * FILL, 0xff)), *d_sc = to_device(std::vector<uint8_t>(N * 32 * SCALARS, 0xff), 1);
  uint8_t *d_e = to_device(std::vector<uint8_t>(N * 32, 0xff));
  uint8_t *d_done = to_device(std::vector<uint8_t>(N, 0xa5));
  bpp_device_transcripts_record *d_rec = to_device(std::vector<bpp_device_transcripts_record>(2, bpp_device_transcripts_record{9, 9, 9, 9}));
  CHECK(((uintptr_t)d_rows & 3) == 3 && ((uintptr_t)d_points & 1) == 1 && ((uintptr_t)d_sc & 1) == 1);

  auto t1 = eng.transcripts_enqueue(d_rows, N,
                                    {Engine::op_new(bytes(proto), (uint32_t)proto.size()),
                                     Engine::op_append_point(bytes(l_p), (uint32_t)l_p.size(), d_points, PT_STRIDE)},
                                    d_live, nullptr, d_rec);
  auto t2 = eng.transcripts_enqueue(d_rows, N,
                                    {Engine::op_rng_begin(), Engine::op_rng_rekey(bytes(l_w), (uint32_t)l_w.size(), d_wit, WIT),
                                     Engine::op_rng_finalize(d_ent), Engine::op_rng_fill32(d_fill, FILL), Engine::op_rng_scalars(d_sc, SCALARS),
                                     Engine::op_challenge_scalar(bytes(l_e), (uint32_t)l_e.size(), d_e)},
                                    d_live, d_done, d_rec + 1);
  t2.wait();  // the one wait
  CHECK(t1.done() && t2.done());

  const std::vector<uint8_t> rows = to_host(d_rows - 3, 3 + N * ROW + 5), fill = to_host(d_fill, N * FILL), sc = to_host(d_sc, N * 32 * SCALARS),
                             e = to_host(d_e, N * 32), done = to_host(d_done, N);
  const std::vector<bpp_device_transcripts_record> rec = to_host(d_rec, 2);
  for (int b = 0; b < 3; b++) CHECK(rows[b] == 0xee);
  for (int b = 0; b < 5; b++) CHECK(rows[3 + N * ROW + b] == 0xee);
  size_t same = 0, zero_rows = 0;
  for (size_t i = 0; i < N; i++) {
    const uint8_t *got = &rows[3 + i * ROW];
    auto outputs_zero = [&] {
      for (size_t b = 0; b < FILL; b++) CHECK(fill[i * FILL + b] == 0);
      for (size_t b = 0; b < 32 * SCALARS; b++) CHECK(sc[i * 32 * SCALARS + b] == 0);
      for (size_t b = 0; b < 32; b++) CHECK(e[i * 32 + b] == 0);
      CHECK(done[i] == 0);
    };
    if (!live[i]) {  // dead: the row untouched, its output rows zero
      for (size_t b = 0; b < ROW; b++) CHECK(got[b] == 0xee);
      outputs_zero();
      continue;
    }
    uint8_t want[ROW], rng[ROW], want_fill[FILL], want_sc[32 * SCALARS], want_e[32];
    char err[128] = {0};
    CHECK(bpp_transcript_new(bytes(proto), proto.size(), want) == BPP_OK);
    const int rc = bpp_transcript_validate_and_append_point(want, bytes(l_p), l_p.size(), &points[i * PT_STRIDE], err, sizeof(err));
    if (i == 6) {  // the identity: the reference's error on the host, a void row on the device
      CHECK(rc == BPP_ERR_VERIFICATION_FAILED && std::string(err) == "Identity element cannot be added to the transcript");
      for (size_t b = 0; b < ROW; b++) CHECK(got[b] == 0);
      outputs_zero();
      zero_rows++;
      continue;
    }
    CHECK(rc == BPP_OK && done[i] == 1);
    CHECK(bpp_transcript_rng_begin(want, rng) == BPP_OK);
    CHECK(bpp_transcript_rng_rekey(rng, bytes(l_w), l_w.size(), &wit[i * WIT], WIT) == BPP_OK);
    CHECK(bpp_transcript_rng_finalize(rng, &ent[i * 32]) == BPP_OK);
    for (size_t k = 0; k < FILL / 32; k++) CHECK(bpp_transcript_rng_fill(rng, want_fill + 32 * k, 32) == BPP_OK);
    for (size_t k = 0; k < SCALARS; k++) CHECK(bpp_transcript_rng_scalar(rng, want_sc + 32 * k, err, sizeof(err)) == BPP_OK);
    CHECK(bpp_transcript_challenge_scalar(want, bytes(l_e), l_e.size(), want_e, err, sizeof(err)) == BPP_OK);
    CHECK(memcmp(got, want, ROW) == 0);
    CHECK(memcmp(&fill[i * FILL], want_fill, FILL) == 0 && memcmp(&sc[i * 32 * SCALARS], want_sc, 32 * SCALARS) == 0 && memcmp(&e[i * 32], want_e, 32) == 0);
    // the same through the wrappers of bpp_host::Transcript
    Transcript tr = Transcript::create(proto);
    Bytes32 p;
    memcpy(p.data(), &points[i * PT_STRIDE], 32);
    tr.validate_and_append_point(l_p, p);
    Transcript::Rng r = tr.build_rng();
    r.rekey_with_witness_bytes(l_w, &wit[i * WIT], WIT).finalize(&ent[i * 32]);
    uint8_t f[FILL];
    for (size_t k = 0; k < FILL / 32; k++) r.fill_bytes(f + 32 * k, 32);
    CHECK(memcmp(f, want_fill, FILL) == 0 && memcmp(r.scalar().data(), want_sc, 32) == 0);
    CHECK(memcmp(tr.challenge_scalar(l_e).data(), want_e, 32) == 0 && memcmp(tr.state().data(), want, ROW) == 0);
    same++;
  }
  printf("rows_equal_to_the_host_helpers %zu\n", same);
  printf("void_rows_all_zero %zu\n", zero_rows);
  printf("record_1 %u %u %u %u\n", rec[0].n_done, rec[0].n_void, rec[0].first_void, rec[0].flags);
  printf("record_2 %u %u %u %u\n", rec[1].n_done, rec[1].n_void, rec[1].first_void, rec[1].flags);

  std::string what;
  try {
    eng.transcripts_enqueue(d_rows, N, {Engine::op_rng_begin(), Engine::op_rng_fill(d_fill, 32)});
  } catch (const ProofError &err) {
    what = std::to_string((int)err.kind) + " " + err.what();
  }
  printf("refusal %s\n", what.c_str());
  const struct bpp_transcripts_stats st = eng.transcripts_stats();
  printf("stats %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.first_calls, (unsigned long long)st.host_waits);
  printf("transcript_rng ok\n");
  return 0;
}
