// A compiled caller of bpp_transcripts_enqueue (include/bpp.h) through Engine::transcripts_enqueue and the op builders of
// include/bpp.hpp, with arrays it allocated itself with hipMalloc -- no torch, no ctypes declarations that could hide a wrong
// prototype.  Eight rows under a live mask (rows 2 and 5 dead), the rows starting three bytes into their allocation:
//   call 1: NEW("cpp transcript ops") + APPEND("txid", 32 bytes of row i, rows 33 bytes apart) + CHALLENGE("c", 32)
//   call 2: APPEND("more", lens[i] bytes under a cap of 48; row 6 asks for 49 and becomes void) + CHALLENGE("after", 64)
// The program holds every row and every challenge to bpp_transcript_new / bpp_transcript_append_message /
// bpp_transcript_challenge_bytes on a host copy, the dead rows to the 0xEE they held, and prints the records and the counters, which
// tests/test_gpu_cpp_transcript_ops.py reads.
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

// a device copy of v that starts `skew` bytes into its allocation
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
  const size_t N = 8, ROW = 203, TX = 32, TX_STRIDE = 33, CAP = 48;
  const std::string proto = "cpp transcript ops", l_txid = "txid", l_c = "c", l_more = "more", l_after = "after";
  const uint8_t live[N] = {1, 1, 0, 1, 1, 0, 1, 1};
  std::vector<uint8_t> txid(N * TX_STRIDE, 0xee), more(N * CAP, 0xee);
  std::vector<uint32_t> lens(N);
  for (size_t i = 0; i < N; i++) {
    for (size_t k = 0; k < TX; k++) txid[i * TX_STRIDE + k] = (uint8_t)(17 * i + 3 * k + 1);
    lens[i] = (uint32_t)(5 * i + 1);
    for (size_t k = 0; k < CAP; k++) more[i * CAP + k] = (uint8_t)(29 * i + 7 * k + 2);
  }
  lens[6] = CAP + 1;  // beyond the cap: the row is void in call 2
  uint8_t *d_rows = to_device(std::vector<uint8_t>(3 + N * ROW + 5, 0xee)) + 3;
  const uint8_t *d_txid = to_device(txid, 1), *d_more = to_device(more), *d_live = to_device(std::vector<uint8_t>(live, live + N));
  const uint32_t *d_lens = to_device(lens);
  uint8_t *d_c = to_device(std::vector<uint8_t>(N * 32, 0xff)), *d_after = to_device(std::vector<uint8_t>(N * 64, 0xff));
  uint8_t *d_done = to_device(std::vector<uint8_t>(N, 0xa5));
  bpp_device_transcripts_record *d_rec = to_device(std::vector<bpp_device_transcripts_record>(2, bpp_device_transcripts_record{9, 9, 9, 9}));
  CHECK(((uintptr_t)d_rows & 3) == 3 && ((uintptr_t)d_txid & 1) == 1);

  auto t1 = eng.transcripts_enqueue(d_rows, N,
                                    {Engine::op_new(bytes(proto), (uint32_t)proto.size()),
                                     Engine::op_append(bytes(l_txid), (uint32_t)l_txid.size(), d_txid, TX, TX_STRIDE),
                                     Engine::op_challenge(bytes(l_c), (uint32_t)l_c.size(), d_c, 32)},
                                    d_live, d_done, d_rec);
  auto t2 = eng.transcripts_enqueue(d_rows, N,
                                    {Engine::op_append(bytes(l_more), (uint32_t)l_more.size(), d_more, CAP, 0, d_lens),
                                     Engine::op_challenge(bytes(l_after), (uint32_t)l_after.size(), d_after, 64)},
                                    d_live, nullptr, d_rec + 1);
  t2.wait();  // the one wait
  CHECK(t1.done() && t2.done());

  const std::vector<uint8_t> rows = to_host(d_rows - 3, 3 + N * ROW + 5), c = to_host(d_c, N * 32), after = to_host(d_after, N * 64),
                             done = to_host(d_done, N);
  const std::vector<bpp_device_transcripts_record> rec = to_host(d_rec, 2);
  for (int b = 0; b < 3; b++) CHECK(rows[b] == 0xee);
  for (int b = 0; b < 5; b++) CHECK(rows[3 + N * ROW + b] == 0xee);
  size_t same = 0;
  for (size_t i = 0; i < N; i++) {
    const uint8_t *got = &rows[3 + i * ROW];
    uint8_t want[ROW], want_c[32], want_after[64];
    if (!live[i]) {  // dead: the row untouched, its challenge rows zero
      for (size_t b = 0; b < ROW; b++) CHECK(got[b] == 0xee);
      for (size_t b = 0; b < 32; b++) CHECK(c[i * 32 + b] == 0);
      for (size_t b = 0; b < 64; b++) CHECK(after[i * 64 + b] == 0);
      CHECK(done[i] == 0);
      continue;
    }
    CHECK(done[i] == 1);
    CHECK(bpp_transcript_new(bytes(proto), proto.size(), want) == BPP_OK);
    CHECK(bpp_transcript_append_message(want, bytes(l_txid), l_txid.size(), &txid[i * TX_STRIDE], TX) == BPP_OK);
    CHECK(bpp_transcript_challenge_bytes(want, bytes(l_c), l_c.size(), want_c, 32) == BPP_OK);
    CHECK(memcmp(&c[i * 32], want_c, 32) == 0);
    if (i == 6) {  // void in call 2
      for (size_t b = 0; b < ROW; b++) CHECK(got[b] == 0);
      for (size_t b = 0; b < 64; b++) CHECK(after[i * 64 + b] == 0);
      continue;
    }
    CHECK(bpp_transcript_append_message(want, bytes(l_more), l_more.size(), &more[i * CAP], lens[i]) == BPP_OK);
    CHECK(bpp_transcript_challenge_bytes(want, bytes(l_after), l_after.size(), want_after, 64) == BPP_OK);
    CHECK(memcmp(got, want, ROW) == 0 && memcmp(&after[i * 64], want_after, 64) == 0);
    same++;
  }
  printf("rows_equal_to_the_host_helpers %zu\n", same);
  printf("record_1 %u %u %u %u\n", rec[0].n_done, rec[0].n_void, rec[0].first_void, rec[0].flags);
  printf("record_2 %u %u %u %u\n", rec[1].n_done, rec[1].n_void, rec[1].first_void, rec[1].flags);

  std::string what;
  try {
    eng.transcripts_enqueue(d_rows, N, {Engine::op_challenge(bytes(l_c), (uint32_t)l_c.size(), d_rows + 10, 32)});
  } catch (const ProofError &e) {
    what = std::to_string((int)e.kind) + " " + e.what();
  }
  printf("refusal %s\n", what.c_str());
  const struct bpp_transcripts_stats st = eng.transcripts_stats();
  printf("stats %llu %llu %llu\n", (unsigned long long)st.calls, (unsigned long long)st.first_calls, (unsigned long long)st.host_waits);
  printf("transcript_ops ok\n");
  return 0;
}
