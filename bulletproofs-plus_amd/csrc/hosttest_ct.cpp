// Sanitizer harness (CPU test suite only): the one-lane model of the constant-time multiscalar multiplication (ct.h:
// ct_straus_model) and its chunk planner (ct_plan.h), built with  g++ -fsanitize=address,undefined  into an executable that
// tests/test_msm_ct_host.py runs as a child process.  Prints one "ok <case>" line per case and "all ok" at the end; a failed
// expectation prints its line and exits with 1.
#include <stdio.h>
#include <stdlib.h>

#include "hosttest.cpp"  // ht_ct_straus, ht_ct_chunk_plan and ht_scalarmult: same translation unit, so they run under the sanitizers too

namespace {

#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      fflush(stdout);                                       \
      exit(1);                                              \
    }                                                       \
  } while (0)

const uint8_t kEll[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                          0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};

uint64_t g_state = 0x243f6a8885a308d3ull;
uint8_t next_byte() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint8_t)(g_state >> 56);
}

// the edge scalars of the issue: 0, 1, l - 1, 2^252, 2^252 - 1, every digit 8, every digit 7, a random one
void edge_scalar(uint8_t s[32], size_t which) {
  memset(s, 0, 32);
  switch (which % 8) {
    case 0: break;
    case 1: s[0] = 1; break;
    case 2: memcpy(s, kEll, 32); s[0] -= 1; break;
    case 3: s[31] = 0x10; break;
    case 4: memset(s, 0xff, 31); s[31] = 0x0f; break;
    case 5: memset(s, 0x88, 31); s[31] = 0x08; break;
    case 6: memset(s, 0x77, 31); s[31] = 0x07; break;
    default:
      for (int k = 0; k < 32; k++) s[k] = next_byte();
      s[31] &= 0x0f;
  }
}

void random_point(uint8_t out[32]) {
  uint8_t u[64];
  for (int k = 0; k < 64; k++) u[k] = next_byte();
  ht_from_uniform(u, out);
}

// the model against the sum of the per-term products of the plain ladder (ht_scalarmult): the same group element
void model_case(size_t n) {
  std::vector<uint8_t> sc32(n * 32 + 32), pt32(n * 32 + 32);
  for (size_t i = 0; i < n; i++) {
    edge_scalar(&sc32[32 * i], i);
    if (i % 5 == 3) memset(&pt32[32 * i], 0, 32);                         // the identity encoding
    else if (i % 5 == 4) memcpy(&pt32[32 * i], &pt32[32 * (i - 2)], 32);  // a repeated point
    else random_point(&pt32[32 * i]);
  }
  uint8_t got[32];
  std::vector<uint8_t> trace(64 * 4 * 8 * n + 1);
  size_t tl = 0;
  CHECK(ht_ct_straus(sc32.data(), pt32.data(), n, got, trace.data(), trace.size(), &tl) == 1);
  CHECK(tl == 64 * 4 * 8 * n);
  ge want;
  ge_identity(want);
  for (size_t i = 0; i < n; i++) {
    niels e;
    CHECK(ristretto_decompress(e, &pt32[32 * i]));
    ge p, prod;
    ge_from_niels(p, e);
    sc s;
    sc_load_words(s, &sc32[32 * i]);
    ct_scalarmul(prod, p, s);
    ge_add(want, want, prod);
  }
  uint8_t w32[32];
  ristretto_compress(w32, want);
  CHECK(memcmp(got, w32, 32) == 0);
  // P and -P under equal scalars: 32 zero bytes
  if (n >= 2) {
    niels e;
    CHECK(ristretto_decompress(e, &pt32[0]));
    niels_cneg(e, true);
    ge m;
    ge_identity(m);
    ge_madd(m, m, e);
    ristretto_compress(&pt32[32], m);
    memcpy(&sc32[32], &sc32[0], 32);
    uint8_t pair[32], zero[32] = {0};
    CHECK(ht_ct_straus(sc32.data(), pt32.data(), 2, pair, nullptr, 0, nullptr) == 1);
    CHECK(memcmp(pair, zero, 32) == 0);
  }
  printf("ok model_%zu\n", n);
}

void plan_case(uint32_t K) {
  const uint32_t sizes[9] = {0, 1, 16, 17, 0, 32, 33, 65, 0};
  uint32_t off[10] = {0};
  for (int g = 0; g < 9; g++) off[g + 1] = off[g] + sizes[g];
  const size_t n = off[9];
  std::vector<uint32_t> chunks(3 * n + 3), choff(10);
  size_t nc = 0;
  CHECK(ht_ct_chunk_plan(off, 9, n, K, chunks.data(), n + 1, &nc, choff.data()) == 0);
  std::vector<int> seen(n, 0);
  for (size_t c = 0; c < nc; c++) {
    const uint32_t g = chunks[3 * c], first = chunks[3 * c + 1], cnt = chunks[3 * c + 2];
    CHECK(g < 9 && cnt >= 1 && cnt <= 16 * K);
    CHECK(first >= off[g] && first + cnt <= off[g + 1]);
    CHECK(c >= choff[g] && c < choff[g + 1]);
    for (uint32_t i = first; i < first + cnt; i++) seen[i]++;
  }
  for (size_t i = 0; i < n; i++) CHECK(seen[i] == 1);
  for (int g = 0; g < 9; g++) CHECK((choff[g + 1] == choff[g]) == (sizes[g] == 0));
  CHECK(choff[9] == nc);
  uint32_t bad[3] = {0, 5, 3};
  CHECK(ht_ct_chunk_plan(bad, 2, 5, K, nullptr, 0, &nc, nullptr) == -1);
  uint32_t past[3] = {0, 2, 6};
  CHECK(ht_ct_chunk_plan(past, 2, 5, K, nullptr, 0, &nc, nullptr) == -1);
  printf("ok plan_k%u\n", K);
}

}  // namespace

int main() {
  const size_t counts[6] = {1, 2, 3, 16, 17, 33};
  for (size_t n : counts) model_case(n);
  plan_case(1);
  plan_case(2);
  uint8_t s[32];
  memcpy(s, kEll, 32);
  CHECK(ht_ct_sc_canonical(s) == 0);
  s[0] -= 1;
  CHECK(ht_ct_sc_canonical(s) == 1);
  memset(s, 0xff, 32);
  CHECK(ht_ct_sc_canonical(s) == 0);
  printf("ok canonical\n");
  printf("all ok\n");
  return 0;
}
