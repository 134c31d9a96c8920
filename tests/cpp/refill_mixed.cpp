// A compiled caller of bpp_batch_refill_enqueue_mixed (include/bpp.h), with arrays it allocated itself with hipMalloc -- no torch, no
// ctypes declarations that could hide a wrong prototype -- on a context made with bpp_ctx_create_on_stream.  Three sets of seven items
// (n = 8, m = 4, 1, 2, 1, 1, 4, 2, t = 1) are proved with bpp_prove_batch_mixed; what that call wrote -- proofs in rows of
// proof_stride, proof_lens -- goes into a ring of three device input sets as it is.  Set 0 is uploaded with
// bpp_batch_upload_mixed_device; then three steps run refill under a mask + bpp_verify_enqueue with the boundaries [0, 3, 7], nothing
// waited for in between.  The refills pass no proof_lens / m (the batch's own vectors).  Step 1 has a non-canonical scalar and a proof
// that does not verify at DEAD slots, step 2 a proof that does not verify at a LIVE slot.  The reference of every (step, group) is a
// blocking bpp_verify_batch_mixed over the group's live rows in host memory.  The program prints codes, masks and presence of both;
// tests/test_gpu_cpp_refill_mixed.py compares them.  Engine::batch_refill_enqueue_mixed of include/bpp.hpp is called once, on an
// engine of its own, for the prototype and the refusal as an exception.
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

static void print_hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

template <typename T>
static T *to_device(const std::vector<T> &v) {
  void *d = nullptr;
  CHECK(hipMalloc(&d, v.size() * sizeof(T)) == hipSuccess);
  CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
  return static_cast<T *>(d);
}

static const size_t N = 7, M_STRIDE = 4, SETS = 3, STEPS = 3, G = 2;
static const size_t STRIDE = 1 + 32 * (1 + 5 + 2 * 5) + 3;  // the longest proof (m = 4: five rounds) and three bytes
static const uint32_t MS[N] = {4, 1, 2, 1, 1, 4, 2};
static const uint32_t BOUNDS[G + 1] = {0, 3, 7};

// one input set as the prover left it
struct Set {
  std::vector<uint64_t> values, min_values;
  std::vector<uint8_t> blindings, seeds, seed_present, min_present, ext, commitments, proofs;
  std::vector<size_t> lens;
  bpp_mixed_batch dev;
};

int main() {
  hipStream_t stream;
  CHECK(hipStreamCreate(&stream) == hipSuccess);
  bpp_ctx *ctx = nullptr;
  CHECK(bpp_ctx_create_on_stream(&ctx, 0, stream) == BPP_OK);
  uint64_t params = 0;
  CHECK(bpp_params_create(ctx, 8, 4, 1, nullptr, nullptr, &params) == BPP_OK);
  const std::string label = "refill mixed";
  const std::vector<uint32_t> m(MS, MS + N);
  char err[256] = {0};
  uint64_t s = 20261023;
  std::vector<Set> sets(SETS);
  for (Set &st : sets) {
    st.values.assign(N * M_STRIDE, 0);
    st.min_values.assign(N * M_STRIDE, 1ull << 63);
    st.blindings.assign(32 * N * M_STRIDE, 0);
    st.seeds.assign(32 * N, 0);
    st.seed_present.assign(N, 0);
    st.min_present.assign(N * M_STRIDE, 1);
    st.ext.resize(N * 32 * 8);
    st.commitments.assign(32 * N * M_STRIDE, 0xff);  // (what is not written stays 0xff: row slack)
    st.proofs.assign(N * STRIDE, 0xff);
    st.lens.assign(N, 0);
    for (auto &x : st.ext) x = (uint8_t)splitmix(s);
    std::vector<bpp_prove_item> items(N);
    for (size_t i = 0; i < N; i++) {
      for (size_t j = 0; j < MS[i]; j++) {
        st.values[i * M_STRIDE + j] = splitmix(s) & 0xff;
        st.min_values[i * M_STRIDE + j] = st.values[i * M_STRIDE + j] / 3;
        st.min_present[i * M_STRIDE + j] = (uint8_t)(j & 1);
        for (int k = 0; k < 31; k++) st.blindings[32 * (i * M_STRIDE + j) + k] = (uint8_t)splitmix(s) | (k == 0);
      }
      for (int k = 0; k < 31; k++) st.seeds[32 * i + k] = (uint8_t)splitmix(s) | (k == 0);
      st.seed_present[i] = MS[i] == 1;
      CHECK(bpp_pedersen_commit(ctx, params, &st.values[i * M_STRIDE], &st.blindings[32 * i * M_STRIDE], 1, MS[i], &st.commitments[32 * i * M_STRIDE]) == BPP_OK);
      memset(&items[i], 0, sizeof(items[i]));
      items[i].values = &st.values[i * M_STRIDE];
      items[i].blindings32 = &st.blindings[32 * i * M_STRIDE];
      items[i].commitments32 = &st.commitments[32 * i * M_STRIDE];
      items[i].m = MS[i];
      items[i].min_values = &st.min_values[i * M_STRIDE];
      items[i].min_present = &st.min_present[i * M_STRIDE];
      items[i].seed_nonce32 = st.seed_present[i] ? &st.seeds[32 * i] : nullptr;
      items[i].transcript_label = (const uint8_t *)label.data();
      items[i].label_len = label.size();
      items[i].rng_bytes = &st.ext[i * 32 * 8];
      items[i].rng_len = 32 * 8;
    }
    std::vector<int> status(N, -1);
    CHECK(bpp_prove_batch_mixed(ctx, params, items.data(), N, st.proofs.data(), STRIDE, st.lens.data(), status.data(), err, sizeof(err)) == BPP_OK);
    for (size_t i = 0; i < N; i++) CHECK(status[i] == BPP_OK && st.lens[i] == sets[0].lens[i]);
  }
  // what the steps bring: step 1 a non-canonical scalar (slot 5) and an invalid proof (slot 2) at dead slots, step 2 an invalid proof
  // at the live slot 4
  static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
  const uint8_t masks_of[STEPS][N] = {{1, 1, 0, 1, 0, 1, 1}, {1, 255, 0, 0, 2, 0, 1}, {0, 0, 0, 1, 1, 1, 0}};
  const size_t set_of[STEPS] = {1, 2, 0};
  memcpy(&sets[2].proofs[5 * STRIDE + 1 + 32 * 5], L, 32);
  sets[2].proofs[2 * STRIDE + 1 + 32 * 4] ^= 1;
  std::vector<uint8_t> clean0 = sets[0].proofs;  // (the upload takes set 0 as it was proved)
  sets[0].proofs[4 * STRIDE + 1 + 32 * 4] ^= 1;
  for (size_t k = 0; k < SETS; k++) {
    Set &st = sets[k];
    memset(&st.dev, 0, sizeof(st.dev));
    st.dev.n_items = N;
    st.dev.proofs = to_device(st.proofs);
    st.dev.proof_stride = STRIDE;
    st.dev.m_stride = (uint32_t)M_STRIDE;
    st.dev.commitments32 = to_device(st.commitments);
    st.dev.min_values = to_device(st.min_values);
    st.dev.min_present = to_device(st.min_present);
    st.dev.seed_nonces32 = to_device(st.seeds);
    st.dev.seed_present = to_device(st.seed_present);
  }
  bpp_mixed_batch first = sets[0].dev;
  first.proofs = to_device(clean0);
  first.proof_lens = sets[0].lens.data();
  first.m = m.data();
  first.transcript_label = (const uint8_t *)label.data();
  first.label_len = label.size();
  uint64_t h = 0;
  CHECK(bpp_batch_upload_mixed_device(ctx, params, &first, &h, err, sizeof(err)) == BPP_OK);

  // ---- the steps: nothing is waited for until the last enqueue is in
  void *out = nullptr;  // per step: one refill record, G verdict records, N mask rows, N presence bytes (16-byte aligned pieces)
  const size_t step_bytes = 16 + G * sizeof(bpp_device_verdict) + N * 32 + 16;
  CHECK(sizeof(bpp_device_refill) == 16 && sizeof(bpp_device_verdict) == 16);
  CHECK(hipMalloc(&out, STEPS * step_bytes) == hipSuccess);
  CHECK(hipMemset(out, 0xff, STEPS * step_bytes) == hipSuccess);
  std::vector<uint8_t *> live_dev(STEPS);
  for (size_t k = 0; k < STEPS; k++) live_dev[k] = to_device(std::vector<uint8_t>(masks_of[k], masks_of[k] + N));
  const int actions[G] = {BPP_RECOVER_AND_VERIFY, BPP_RECOVER_AND_VERIFY};
  uint64_t ticket = 0;
  for (size_t k = 0; k < STEPS; k++) {
    uint8_t *base = static_cast<uint8_t *>(out) + k * step_bytes;
    CHECK(bpp_batch_refill_enqueue_mixed(ctx, h, &sets[set_of[k]].dev, nullptr, live_dev[k], reinterpret_cast<bpp_device_refill *>(base), nullptr) == BPP_OK);
    CHECK(bpp_verify_enqueue(ctx, h, BOUNDS, G, 0, actions, BPP_VERIFY_ONLY, reinterpret_cast<bpp_device_verdict *>(base + 16),
                             base + 16 + G * 16, base + 16 + G * 16 + N * 32, &ticket) == BPP_OK);
  }
  struct bpp_refill_stats rs;
  struct bpp_enqueue_stats es;
  CHECK(bpp_refill_stats(ctx, &rs) == BPP_OK && bpp_enqueue_stats(ctx, &es) == BPP_OK);
  printf("stats %llu %llu %llu\n", (unsigned long long)rs.calls, (unsigned long long)rs.first_calls, (unsigned long long)rs.host_waits);
  CHECK(es.calls == STEPS);
  CHECK(bpp_enqueue_wait(ctx, ticket) == BPP_OK);  // the one wait
  std::vector<uint8_t> got(STEPS * step_bytes);
  CHECK(hipMemcpy(got.data(), out, got.size(), hipMemcpyDeviceToHost) == hipSuccess);

  // ---- the references: a blocking call over each group's live rows, from host memory, on a context of its own
  Engine eng(0);
  auto ref_params = RangeParameters::init(eng, 8, 4, create_pedersen_gens_with_extension_degree(ExtensionDegree::DefaultPedersen));
  for (size_t k = 0; k < STEPS; k++) {
    const Set &st = sets[set_of[k]];
    const uint8_t *base = got.data() + k * step_bytes;
    bpp_device_refill rec;
    memcpy(&rec, base, 16);
    bpp_shard_result r;
    CHECK(bpp_refill_result(&rec, &r) == BPP_OK);
    printf("record_%zu %d %d %u %u\n", k, r.code, r.tier, r.index, rec.flags);
    const uint8_t *masks = base + 16 + G * 16, *present = masks + N * 32;
    for (size_t g = 0; g < G; g++) {
      bpp_device_verdict v;
      memcpy(&v, base + 16 + g * 16, 16);
      std::vector<size_t> slots;
      for (size_t i = BOUNDS[g]; i < BOUNDS[g + 1]; i++)
        if (masks_of[k][i]) slots.push_back(i);
      printf("verdict_%zu_%zu %d %u %u ", k, g, v.code, v.tier, v.flags);
      for (size_t i : slots) {
        printf("%d:", present[i]);
        print_hex(masks + 32 * i, 32);
        printf(",");
      }
      printf("\n");
      // the same rows gathered into a batch of their own
      const size_t n = slots.size();
      if (n == 0) {  // (a group without a live row: there is nothing to upload; its record must say so)
        printf("reference_%zu_%zu empty\n", k, g);
        continue;
      }
      std::vector<uint8_t> proofs(n * STRIDE), commitments(32 * n * M_STRIDE), min_present(n * M_STRIDE), seeds(32 * n), seed_present(n);
      std::vector<uint64_t> min_values(n * M_STRIDE);
      std::vector<size_t> lens(n);
      std::vector<uint32_t> ms(n);
      for (size_t q = 0; q < n; q++) {
        const size_t i = slots[q];
        memcpy(&proofs[q * STRIDE], &st.proofs[i * STRIDE], STRIDE);
        memcpy(&commitments[32 * q * M_STRIDE], &st.commitments[32 * i * M_STRIDE], 32 * M_STRIDE);
        memcpy(&min_values[q * M_STRIDE], &st.min_values[i * M_STRIDE], 8 * M_STRIDE);
        memcpy(&min_present[q * M_STRIDE], &st.min_present[i * M_STRIDE], M_STRIDE);
        memcpy(&seeds[32 * q], &st.seeds[32 * i], 32);
        seed_present[q] = st.seed_present[i];
        lens[q] = st.lens[i];
        ms[q] = MS[i];
      }
      bpp_mixed_batch host;
      memset(&host, 0, sizeof(host));
      host.n_items = n;
      host.proofs = proofs.data();
      host.proof_stride = STRIDE;
      host.proof_lens = lens.data();
      host.m = ms.data();
      host.m_stride = (uint32_t)M_STRIDE;
      host.commitments32 = commitments.data();
      host.min_values = min_values.data();
      host.min_present = min_present.data();
      host.seed_nonces32 = seeds.data();
      host.seed_present = seed_present.data();
      host.transcript_label = (const uint8_t *)label.data();
      host.label_len = label.size();
      std::vector<uint8_t> ref_masks(32 * n, 0), ref_present(n, 0);
      const int rc = bpp_verify_batch_mixed(eng.ctx(), ref_params->handle(), &host, BPP_RECOVER_AND_VERIFY, 0, ref_masks.data(), ref_present.data(), err, sizeof(err));
      // (a rejected blocking call hands out no masks; the enqueued call's rows of such a group are zero as well)
      printf("reference_%zu_%zu %d ", k, g, rc);
      for (size_t q = 0; q < n; q++) {
        printf("%d:", rc == BPP_OK ? ref_present[q] : 0);
        if (rc == BPP_OK) print_hex(&ref_masks[32 * q], 32);
        else print_hex(std::vector<uint8_t>(32, 0).data(), 32);
        printf(",");
      }
      printf("\n");
    }
    for (size_t i = 0; i < N; i++)
      if (!masks_of[k][i]) {
        CHECK(present[i] == 0);
        for (int b = 0; b < 32; b++) CHECK(masks[32 * i + b] == 0);
      }
  }
  // ---- the mirror of bpp.hpp: the prototype, and a refusal as an exception (a batch this engine does not know)
  std::string what;
  try {
    eng.batch_refill_enqueue_mixed(h, sets[0].dev, nullptr, live_dev[0], nullptr);
  } catch (const std::exception &e) {
    what = e.what();
  }
  printf("refused %s\n", what.c_str());
  // ... and count_dev together with live_dev, through bpp.h, before anything is launched
  CHECK(bpp_batch_refill_enqueue_mixed(ctx, h, &sets[0].dev, reinterpret_cast<const uint32_t *>(live_dev[0]), live_dev[1], nullptr, nullptr) == BPP_ERR_INVALID_ARGUMENT);
  printf("both %s\n", bpp_ctx_last_error(ctx));
  struct bpp_refill_stats rs2;
  CHECK(bpp_refill_stats(ctx, &rs2) == BPP_OK && rs2.calls == rs.calls);
  CHECK(bpp_batch_destroy(ctx, h) == BPP_OK);
  for (Set &st : sets)
    for (const void *p : {(const void *)st.dev.proofs, (const void *)st.dev.commitments32, (const void *)st.dev.min_values, (const void *)st.dev.min_present,
                          (const void *)st.dev.seed_nonces32, (const void *)st.dev.seed_present})
      CHECK(hipFree(const_cast<void *>(p)) == hipSuccess);
  for (uint8_t *p : live_dev) CHECK(hipFree(p) == hipSuccess);
  CHECK(hipFree(const_cast<uint8_t *>(first.proofs)) == hipSuccess);
  CHECK(hipFree(out) == hipSuccess);
  CHECK(bpp_params_destroy(ctx, params) == BPP_OK);
  bpp_ctx_destroy(ctx);
  CHECK(hipStreamDestroy(stream) == hipSuccess);
  printf("refill mixed ok\n");
  return 0;
}
