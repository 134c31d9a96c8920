// A compiled caller of the per-item transcript calls of include/bpp.h -- bpp_batch_upload_packed_device_transcripts,
// bpp_batch_refill_enqueue_transcripts, bpp_verify_enqueue_states -- with arrays it allocated itself with hipMalloc, on a context
// made with bpp_ctx_create_on_stream: no torch, no ctypes declarations that could hide a wrong prototype.  Two sets of six items
// (n = 8, m = 1, t = 1) are proved with bpp_prove_batch_mixed, every item under a transcript of its own: bpp_transcript_new plus one
// bpp_transcript_append_message whose length differs from item to item.  Set 0 is uploaded with its rows, set 1 refills the batch
// under a mask; each is followed by bpp_verify_enqueue_states with the boundaries [0, 2, 6], and nothing is waited for until the last
// call is in.  Engine::batch_refill_enqueue and Engine::verify_enqueue_states of include/bpp.hpp are called once each, on an engine
// of its own, for the prototypes and the refusal as an exception.  The state array starts one byte into its allocation, the
// output array three.  The program itself holds every (step, group) to a blocking bpp_verify_batch_states over the group's live
// items: codes, and the 203-byte rows of live slots; dead slots and rejected groups hold zero rows.  It prints one line per check
// for tests/test_gpu_cpp_item_transcripts.py.
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
static T *to_device(const std::vector<T> &v, size_t offset = 0) {
  void *d = nullptr;
  CHECK(hipMalloc(&d, offset + v.size() * sizeof(T)) == hipSuccess);
  CHECK(hipMemcpy(static_cast<uint8_t *>(d) + offset, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  return reinterpret_cast<T *>(static_cast<uint8_t *>(d) + offset);
}

static const size_t N = 6, SETS = 2, G = 2, ROW = 203;
static const size_t LEN = 1 + 32 * (1 + 5 + 2 * 3);  // t = 1, three rounds
static const uint32_t BOUNDS[G + 1] = {0, 2, 6};

struct Set {
  std::vector<uint64_t> values;
  std::vector<uint8_t> blindings, ext, commitments, proofs, states;
  bpp_packed_batch dev;
  const uint8_t *states_dev;
};

int main() {
  hipStream_t stream;
  CHECK(hipStreamCreate(&stream) == hipSuccess);
  bpp_ctx *ctx = nullptr;
  CHECK(bpp_ctx_create_on_stream(&ctx, 0, stream) == BPP_OK);
  uint64_t params = 0;
  CHECK(bpp_params_create(ctx, 8, 1, 1, nullptr, nullptr, &params) == BPP_OK);
  const std::string label = "item transcripts", ctx_label = "tx";
  char err[256] = {0};
  uint64_t s = 20261024;
  std::vector<Set> sets(SETS);
  for (size_t k = 0; k < SETS; k++) {
    Set &st = sets[k];
    st.values.assign(N, 0);
    st.blindings.assign(32 * N, 0);
    st.ext.resize(N * 32 * 6);
    st.commitments.assign(32 * N, 0);
    st.proofs.assign(N * LEN, 0);
    st.states.assign(N * ROW, 0);
    for (auto &x : st.ext) x = (uint8_t)splitmix(s);
    std::vector<bpp_prove_item> items(N);
    std::vector<size_t> lens(N, 0);
    for (size_t i = 0; i < N; i++) {
      st.values[i] = splitmix(s) & 0xff;
      for (int b = 0; b < 31; b++) st.blindings[32 * i + b] = (uint8_t)splitmix(s) | (b == 0);
      CHECK(bpp_pedersen_commit(ctx, params, &st.values[i], &st.blindings[32 * i], 1, 1, &st.commitments[32 * i]) == BPP_OK);
      // the item's own transcript: the label, then a context of 5 + 11 i + k bytes
      std::vector<uint8_t> context(5 + 11 * i + k);
      for (auto &x : context) x = (uint8_t)splitmix(s);
      uint8_t *row = &st.states[i * ROW];
      CHECK(bpp_transcript_new((const uint8_t *)label.data(), label.size(), row) == BPP_OK);
      CHECK(bpp_transcript_append_message(row, (const uint8_t *)ctx_label.data(), ctx_label.size(), context.data(), context.size()) == BPP_OK);
      memset(&items[i], 0, sizeof(items[i]));
      items[i].values = &st.values[i];
      items[i].blindings32 = &st.blindings[32 * i];
      items[i].commitments32 = &st.commitments[32 * i];
      items[i].m = 1;
      items[i].transcript_state = row;
      items[i].rng_bytes = &st.ext[i * 32 * 6];
      items[i].rng_len = 32 * 6;
    }
    std::vector<int> status(N, -1);
    CHECK(bpp_prove_batch_mixed(ctx, params, items.data(), N, st.proofs.data(), LEN, lens.data(), status.data(), err, sizeof(err)) == BPP_OK);
    for (size_t i = 0; i < N; i++) CHECK(status[i] == BPP_OK && lens[i] == LEN);
  }
  for (size_t i = 1; i < N; i++) CHECK(sets[0].states[i * ROW + 200] != sets[0].states[(i - 1) * ROW + 200]);  // the rows' pos differ
  // set 1 carries an invalid proof at the live slot 1 (group 0) and, at the DEAD slot 3, a state with pos = 166 and an invalid proof
  const uint8_t live[N] = {1, 255, 2, 0, 1, 1};
  sets[1].proofs[1 * LEN + 1 + 32 * 4] ^= 1;
  sets[1].proofs[3 * LEN + 1 + 32 * 4] ^= 1;
  sets[1].states[3 * ROW + 200] = 166;
  for (Set &st : sets) {
    memset(&st.dev, 0, sizeof(st.dev));
    st.dev.n_items = N;
    st.dev.proofs = to_device(st.proofs);
    st.dev.proof_len = LEN;
    st.dev.proof_stride = LEN;
    st.dev.commitments32 = to_device(st.commitments);
    st.dev.m = 1;
    st.states_dev = to_device(st.states, 1);  // (one byte into its allocation)
  }
  uint64_t h = 0;
  CHECK(bpp_batch_upload_packed_device_transcripts(ctx, params, &sets[0].dev, sets[0].states_dev, &h, err, sizeof(err)) == BPP_OK);

  // ---- two steps on the stream: [upload], enqueue_states; refill under the mask, enqueue_states.  One wait at the end.
  const size_t step_bytes = (16 + G * sizeof(bpp_device_verdict) + 16 + N * ROW + 13 + 15) & ~(size_t)15;  // record, verdicts, 3 bytes of offset, rows
  void *out = nullptr;
  CHECK(hipMalloc(&out, 2 * step_bytes) == hipSuccess);
  CHECK(hipMemset(out, 0xee, 2 * step_bytes) == hipSuccess);
  uint8_t *live_dev = to_device(std::vector<uint8_t>(live, live + N));
  auto record_at = [&](size_t k) { return reinterpret_cast<bpp_device_refill *>(static_cast<uint8_t *>(out) + k * step_bytes); };
  auto verdicts_at = [&](size_t k) { return reinterpret_cast<bpp_device_verdict *>(static_cast<uint8_t *>(out) + k * step_bytes + 16); };
  auto rows_at = [&](size_t k) { return static_cast<uint8_t *>(out) + k * step_bytes + 16 + G * 16 + 3; };
  uint64_t ticket = 0;
  CHECK(bpp_verify_enqueue_states(ctx, h, BOUNDS, G, 0, nullptr, BPP_VERIFY_ONLY, verdicts_at(0), nullptr, nullptr, rows_at(0), &ticket) == BPP_OK);
  {
    // (through bpp.hpp, on an Engine that shares nothing with ctx: only the prototypes are wanted, and the refusal as an exception)
    Engine other(0);
    std::string what;
    try {
      other.batch_refill_enqueue(h, sets[1].dev, sets[1].states_dev, nullptr, live_dev, nullptr);
    } catch (const std::exception &e) {
      what = e.what();
    }
    printf("refused %s\n", what.c_str());
    what.clear();
    try {
      other.verify_enqueue_states(h, BOUNDS, G, 0, nullptr, VerifyAction::VerifyOnly, verdicts_at(1), rows_at(1));
    } catch (const std::exception &e) {
      what = e.what();
    }
    printf("refused_states %s\n", what.c_str());
  }
  CHECK(bpp_batch_refill_enqueue_transcripts(ctx, h, &sets[1].dev, sets[1].states_dev, nullptr, live_dev, record_at(1), nullptr) == BPP_OK);
  CHECK(bpp_verify_enqueue_states(ctx, h, BOUNDS, G, 0, nullptr, BPP_VERIFY_ONLY, verdicts_at(1), nullptr, nullptr, rows_at(1), &ticket) == BPP_OK);
  struct bpp_refill_stats rs;
  struct bpp_enqueue_stats es;
  CHECK(bpp_refill_stats(ctx, &rs) == BPP_OK && bpp_enqueue_stats(ctx, &es) == BPP_OK);
  printf("stats %llu %llu %llu %llu\n", (unsigned long long)rs.calls, (unsigned long long)rs.host_waits, (unsigned long long)es.calls,
         (unsigned long long)es.host_waits);
  CHECK(bpp_enqueue_wait(ctx, ticket) == BPP_OK);  // the one wait
  std::vector<uint8_t> got(2 * step_bytes);
  CHECK(hipMemcpy(got.data(), out, got.size(), hipMemcpyDeviceToHost) == hipSuccess);

  // ---- the references: a blocking bpp_verify_batch_states over each group's live items, on a context of its own
  bpp_ctx *ref = nullptr;
  CHECK(bpp_ctx_create(&ref, 0) == BPP_OK);
  uint64_t ref_params = 0;
  CHECK(bpp_params_create(ref, 8, 1, 1, nullptr, nullptr, &ref_params) == BPP_OK);
  for (size_t k = 0; k < 2; k++) {
    const Set &st = sets[k];
    const uint8_t *base = got.data() + k * step_bytes;
    const uint8_t *rows = base + 16 + G * 16 + 3;
    for (int b = 0; b < 3; b++) CHECK(base[16 + G * 16 + b] == 0xee);  // the bytes in front of the rows
    for (int b = 0; b < 13; b++) CHECK(rows[N * ROW + b] == 0xee);  // ... and behind them
    if (k == 1) {
      bpp_device_refill rec;
      memcpy(&rec, base, 16);
      printf("record %d %u %u %u\n", rec.code, rec.msg, rec.index, rec.flags);
    }
    for (size_t g = 0; g < G; g++) {
      bpp_device_verdict v;
      memcpy(&v, base + 16 + g * 16, 16);
      std::vector<size_t> slots;
      for (size_t i = BOUNDS[g]; i < BOUNDS[g + 1]; i++)
        if (k == 0 || live[i]) slots.push_back(i);
      std::vector<bpp_verify_item> items(slots.size());
      for (size_t q = 0; q < slots.size(); q++) {
        const size_t i = slots[q];
        memset(&items[q], 0, sizeof(items[q]));
        items[q].proof = &st.proofs[i * LEN];
        items[q].proof_len = LEN;
        items[q].commitments32 = &st.commitments[32 * i];
        items[q].m = 1;
        items[q].transcript_state = &st.states[i * ROW];
      }
      std::vector<uint8_t> want(slots.size() * ROW, 0);
      const int rc = bpp_verify_batch_states(ref, ref_params, items.data(), items.size(), BPP_VERIFY_ONLY, 0, nullptr, nullptr, want.data(), err, sizeof(err));
      printf("group_%zu_%zu %d %u %u reference %d\n", k, g, v.code, v.tier, v.flags, rc);
      CHECK(v.code == rc && v.flags == BPP_VERDICT_WRITTEN);
      size_t q = 0;
      for (size_t i = BOUNDS[g]; i < BOUNDS[g + 1]; i++) {
        const bool is_live = k == 0 || live[i];
        bool zero = true, nonzero_want = false;
        for (size_t b = 0; b < ROW; b++) zero = zero && rows[i * ROW + b] == 0;
        if (is_live && rc == BPP_OK) {
          for (size_t b = 0; b < ROW; b++) nonzero_want = nonzero_want || want[q * ROW + b] != 0;
          CHECK(nonzero_want && memcmp(&rows[i * ROW], &want[q * ROW], ROW) == 0);
          CHECK(memcmp(&rows[i * ROW], &st.states[i * ROW], ROW) != 0);  // advanced, not handed back as it came
        } else {
          CHECK(zero);
        }
        if (is_live) q++;
      }
    }
  }
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  CHECK(bpp_params_destroy(ref, ref_params) == BPP_OK);
  bpp_ctx_destroy(ref);
  CHECK(hipFree(out) == hipSuccess);
  CHECK(hipFree(live_dev) == hipSuccess);
  for (Set &st : sets) {
    CHECK(hipFree(const_cast<uint8_t *>(st.dev.proofs)) == hipSuccess);
    CHECK(hipFree(const_cast<uint8_t *>(st.dev.commitments32)) == hipSuccess);
    CHECK(hipFree(const_cast<uint8_t *>(st.states_dev) - 1) == hipSuccess);
  }
  CHECK(bpp_params_destroy(ctx, params) == BPP_OK);
  bpp_ctx_destroy(ctx);
  CHECK(hipStreamDestroy(stream) == hipSuccess);
  printf("item transcripts ok\n");
  return 0;
}
