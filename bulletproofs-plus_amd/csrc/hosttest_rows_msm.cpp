// Sanitizer harness (CPU test suite only): rows_msm.h, the per-row rules and the host models of k_rows_msm and k_rows_scalar
// (bpp_rows_msm_enqueue, bpp_rows_scalar_enqueue), built with  g++ -fsanitize=address,undefined  into an executable that
// tests/test_rows_msm_host.py runs as a child process.  The sum is held to ct_straus_model on the row's terms and to the sum of
// ct_scalarmul's products; the scalar operation to bit-serial big-integer arithmetic.  Dead rows' inputs and all row slack are
// POISONED (ASan) while the model runs: a read or write there ends the program.  Prints one "ok <case>" line per case and "all ok"
// at the end; a failed expectation prints its line and exits with 1.
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>

#include "hosttest.cpp"  // ht_rows_msm, ht_rows_scalar, ht_ct_straus: same translation unit, so they run under the sanitizers too

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

uint64_t g_state = 0x13198a2e03707344ull;
uint8_t next_byte() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint8_t)(g_state >> 56);
}
// 0, 1, l - 1, 2^252, 2^252 - 1, every digit 8, every digit 7, a random one
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

// n rows of `width` bytes, `stride` apart, `offset` bytes into an allocation; the slack behind every row can be poisoned
struct Rows {
  std::vector<uint8_t> mem;
  size_t n, width, stride, offset;
  Rows(size_t n_, size_t width_, size_t slack, size_t offset_) : mem(offset_ + n_ * (width_ + slack) + 8, 0xa5), n(n_), width(width_), stride(width_ + slack), offset(offset_) {}
  uint8_t *row(size_t i) { return mem.data() + offset + i * stride; }
  uint8_t *base() { return row(0); }
  void poison_slack(bool on) {
    for (size_t i = 0; i < n && stride > width; i++) {
      if (on) ASAN_POISON_MEMORY_REGION(row(i) + width, stride - width);
      else ASAN_UNPOISON_MEMORY_REGION(row(i) + width, stride - width);
    }
  }
  void poison_row(size_t i, bool on) {
    if (on) ASAN_POISON_MEMORY_REGION(row(i), width);
    else ASAN_UNPOISON_MEMORY_REGION(row(i), width);
  }
  bool slack_untouched() {
    for (size_t i = 0; i < n; i++)
      for (size_t k = width; k < stride; k++)
        if (row(i)[k] != 0xa5) return false;
    return true;
  }
};

// the row's sum by two other routes: ct_straus_model over the K terms, and the sum of ct_scalarmul's products
void reference_row(uint8_t want[32], const uint8_t *sc32, const uint8_t *pt32, uint32_t K) {
  CHECK(ht_ct_straus(sc32, pt32, K, want, nullptr, 0, nullptr) == 1);
  ge sum;
  ge_identity(sum);
  for (uint32_t k = 0; k < K; k++) {
    niels e;
    CHECK(ristretto_decompress(e, pt32 + 32 * k));
    ge p, prod;
    ge_from_niels(p, e);
    sc s;
    sc_load_words(s, sc32 + 32 * k);
    ct_scalarmul(prod, p, s);
    ge_add(sum, sum, prod);
  }
  uint8_t w2[32];
  ristretto_compress(w2, sum);
  CHECK(memcmp(want, w2, 32) == 0);
}

// rows with per-row points or shared bases, row 2 dead (its inputs poisoned), odd addresses, slack everywhere
void model_case(uint32_t K, bool shared) {
  const size_t n = 5, dead = 2;
  Rows sc(n, 32 * K, 5, 1), pt(shared ? 1 : n, 32 * K, 3, 3), out(n, 32, 7, 1);
  std::vector<uint8_t> live(n, 1), done(n, 9);
  live[dead] = 0;
  for (size_t i = 0; i < n; i++)
    for (uint32_t k = 0; k < K; k++) {
      edge_scalar(sc.row(i) + 32 * k, i * K + k);
      if (shared && i) continue;
      uint8_t *p = pt.row(i) + 32 * k;
      if ((i * K + k) % 5 == 3) memset(p, 0, 32);                               // the identity encoding
      else if (k >= 2 && (i * K + k) % 5 == 4) memcpy(p, pt.row(i) + 32 * (k - 2), 32);  // a repeated point
      else random_point(p);
    }
  sc.poison_slack(true), pt.poison_slack(true), out.poison_slack(true);
  sc.poison_row(dead, true);
  if (!shared) pt.poison_row(dead, true);
  uint32_t rec[4];
  std::vector<uint8_t> trace(64 * 4 * 8 * 16 * n + 1);
  size_t tl = 0;
  ht_rows_msm(sc.base(), sc.stride, pt.base(), shared ? 0 : pt.stride, n, K, out.base(), out.stride, live.data(), done.data(), rec, trace.data(),
              trace.size(), &tl);
  sc.poison_slack(false), pt.poison_slack(false), out.poison_slack(false);
  sc.poison_row(dead, false);
  if (!shared) pt.poison_row(dead, false);
  CHECK(tl == (size_t)64 * 4 * 8 * rows_kp(K) * (n - 1));  // every live row: Kp quads, padding included, each the full walk
  CHECK(rec[0] == n - 1 && rec[1] == 0 && rec[2] == 0xffffffffu && rec[3] == BPP_ROWS_WRITTEN);
  CHECK(out.slack_untouched());
  const uint8_t zero[32] = {0};
  for (size_t i = 0; i < n; i++) {
    if (i == dead) {
      CHECK(memcmp(out.row(i), zero, 32) == 0 && done[i] == 0);
      continue;
    }
    uint8_t want[32];
    reference_row(want, sc.row(i), pt.row(shared ? 0 : i), K);
    CHECK(memcmp(out.row(i), want, 32) == 0 && done[i] == 1);
  }
  printf("ok model_%s_%u\n", shared ? "shared" : "rows", K);
}

// P and -P under equal scalars: the identity, 32 zero bytes, and the row is DONE (not void)
void cancel_case() {
  uint8_t pt[64], sc[64], out[32], done = 9, zero[32] = {0};
  uint32_t rec[4];
  random_point(pt);
  niels e;
  CHECK(ristretto_decompress(e, pt));
  niels_cneg(e, true);
  ge m;
  ge_identity(m);
  ge_madd(m, m, e);
  ristretto_compress(pt + 32, m);
  for (size_t which = 1; which < 8; which++) {
    edge_scalar(sc, which);
    memcpy(sc + 32, sc, 32);
    ht_rows_msm(sc, 64, pt, 64, 1, 2, out, 32, nullptr, &done, rec, nullptr, 0, nullptr);
    CHECK(memcmp(out, zero, 32) == 0 && done == 1 && rec[0] == 1 && rec[1] == 0);
  }
  printf("ok cancel\n");
}

// void rows: a scalar >= l in the LAST term (row 1), an undecodable point (row 3), both (row 4); row 0 dead with both defects and
// poisoned; lowest index wins, both flags
void void_case() {
  const size_t n = 6;
  const uint32_t K = 3;
  Rows sc(n, 32 * K, 2, 1), pt(n, 32 * K, 0, 0), out(n, 32, 0, 3);
  std::vector<uint8_t> live(n, 1), done(n, 9);
  live[0] = 0;
  for (size_t i = 0; i < n; i++)
    for (uint32_t k = 0; k < K; k++) {
      edge_scalar(sc.row(i) + 32 * k, 7);
      random_point(pt.row(i) + 32 * k);
    }
  memcpy(sc.row(1) + 64, kEll, 32);
  memset(pt.row(3) + 32, 0xff, 32);
  memset(sc.row(4), 0xff, 32);
  memset(pt.row(4) + 64, 0xff, 32);
  sc.poison_row(0, true), pt.poison_row(0, true);
  uint32_t rec[4];
  ht_rows_msm(sc.base(), sc.stride, pt.base(), pt.stride, n, K, out.base(), out.stride, live.data(), done.data(), rec, nullptr, 0, nullptr);
  sc.poison_row(0, false), pt.poison_row(0, false);
  CHECK(rec[0] == 2 && rec[1] == 3 && rec[2] == 1 && rec[3] == (BPP_ROWS_WRITTEN | BPP_ROWS_SCALAR | BPP_ROWS_POINT));
  const uint8_t zero[32] = {0};
  const uint8_t want_done[6] = {0, 0, 1, 0, 0, 1};
  for (size_t i = 0; i < n; i++) {
    CHECK(done[i] == want_done[i]);
    CHECK((memcmp(out.row(i), zero, 32) == 0) == (want_done[i] == 0));
  }
  // one cause alone sets one flag
  live.assign(n, 0);
  live[1] = 1;
  ht_rows_msm(sc.base(), sc.stride, pt.base(), pt.stride, n, K, out.base(), out.stride, live.data(), done.data(), rec, nullptr, 0, nullptr);
  CHECK(rec[0] == 0 && rec[1] == 1 && rec[2] == 1 && rec[3] == (BPP_ROWS_WRITTEN | BPP_ROWS_SCALAR));
  live[1] = 0, live[3] = 1;
  ht_rows_msm(sc.base(), sc.stride, pt.base(), pt.stride, n, K, out.base(), out.stride, live.data(), done.data(), rec, nullptr, 0, nullptr);
  CHECK(rec[0] == 0 && rec[1] == 1 && rec[2] == 3 && rec[3] == (BPP_ROWS_WRITTEN | BPP_ROWS_POINT));
  // a shared base that does not decode voids every live row (row 2 is clean otherwise)
  live.assign(n, 1);
  live[1] = live[4] = 0;
  ht_rows_msm(sc.base(), sc.stride, pt.row(3), 0, n, K, out.base(), out.stride, live.data(), done.data(), rec, nullptr, 0, nullptr);
  CHECK(rec[0] == 0 && rec[1] == 4 && rec[2] == 0 && rec[3] == (BPP_ROWS_WRITTEN | BPP_ROWS_POINT));
  for (size_t i = 0; i < n; i++) CHECK(done[i] == 0 && memcmp(out.row(i), zero, 32) == 0);
  printf("ok void\n");
}

// the table-read trace of a call is the same for two different scalar rows (and for a void one)
void trace_case() {
  const uint32_t K = 3;
  uint8_t pt[32 * K], sa[32 * K], sb[32 * K], sv[32 * K], out[32];
  for (uint32_t k = 0; k < K; k++) {
    random_point(pt + 32 * k);
    edge_scalar(sa + 32 * k, 0);
    edge_scalar(sb + 32 * k, 7);
    memset(sv + 32 * k, 0xff, 32);
  }
  std::vector<uint8_t> ta(64 * 4 * 8 * 4 + 1), tb(ta.size()), tv(ta.size());
  size_t la = 0, lb = 0, lv = 0;
  uint32_t rec[4];
  ht_rows_msm(sa, 32 * K, pt, 32 * K, 1, K, out, 32, nullptr, nullptr, rec, ta.data(), ta.size(), &la);
  ht_rows_msm(sb, 32 * K, pt, 32 * K, 1, K, out, 32, nullptr, nullptr, rec, tb.data(), tb.size(), &lb);
  ht_rows_msm(sv, 32 * K, pt, 32 * K, 1, K, out, 32, nullptr, nullptr, rec, tv.data(), tv.size(), &lv);
  CHECK(rec[1] == 1);
  CHECK(la == (size_t)64 * 4 * 8 * 4 && lb == la && lv == la);
  CHECK(memcmp(ta.data(), tb.data(), la) == 0 && memcmp(ta.data(), tv.data(), la) == 0);
  for (size_t k = 0; k < la; k++) CHECK(ta[k] == k % 8);
  printf("ok trace\n");
}

// a * b + c mod l, bit-serially: for every bit of a from the top, r = 2 r (+ b), reduced by conditional subtraction
typedef unsigned __int128 u128;
struct Big {
  uint32_t w[9];
};
bool big_geq_l(const Big &x) {
  if (x.w[8]) return true;
  for (int i = 7; i >= 0; i--) {
    const uint32_t li = (uint32_t)kEll[4 * i] | (uint32_t)kEll[4 * i + 1] << 8 | (uint32_t)kEll[4 * i + 2] << 16 | (uint32_t)kEll[4 * i + 3] << 24;
    if (x.w[i] != li) return x.w[i] > li;
  }
  return true;
}
void big_sub_l(Big &x) {
  int64_t borrow = 0;
  for (int i = 0; i < 9; i++) {
    const uint32_t li = i < 8 ? ((uint32_t)kEll[4 * i] | (uint32_t)kEll[4 * i + 1] << 8 | (uint32_t)kEll[4 * i + 2] << 16 | (uint32_t)kEll[4 * i + 3] << 24) : 0;
    const int64_t t = (int64_t)x.w[i] - li - borrow;
    x.w[i] = (uint32_t)t;
    borrow = t < 0 ? 1 : 0;
  }
}
void big_add(Big &x, const Big &y) {
  uint64_t carry = 0;
  for (int i = 0; i < 9; i++) {
    const uint64_t t = (uint64_t)x.w[i] + y.w[i] + carry;
    x.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
  while (big_geq_l(x)) big_sub_l(x);
}
Big big_load(const uint8_t s[32]) {
  Big x{};
  for (int i = 0; i < 8; i++) x.w[i] = (uint32_t)s[4 * i] | (uint32_t)s[4 * i + 1] << 8 | (uint32_t)s[4 * i + 2] << 16 | (uint32_t)s[4 * i + 3] << 24;
  return x;
}
void big_muladd(uint8_t out[32], const uint8_t a[32], const uint8_t b[32], const uint8_t c[32]) {
  Big r{}, bb = big_load(b);
  for (int bit = 255; bit >= 0; bit--) {
    const Big twice = r;
    big_add(r, twice);
    if ((a[bit >> 3] >> (bit & 7)) & 1) big_add(r, bb);
  }
  if (c) big_add(r, big_load(c));
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(r.w[i] >> (8 * k));
}

void scalar_case() {
  // every pair of edge values under every edge value, rows at odd addresses with slack; then broadcasts, c = null, void and dead rows
  const size_t n = 64;
  Rows a(n, 32, 3, 1), b(n, 32, 1, 3), c(n, 32, 0, 1), out(n, 32, 5, 1);
  for (size_t i = 0; i < n; i++) {
    edge_scalar(a.row(i), i % 8);
    edge_scalar(b.row(i), i / 8);
    edge_scalar(c.row(i), (i * 5 + 2) % 8);
  }
  std::vector<uint8_t> live(n, 1), done(n, 9);
  live[9] = 0;
  memcpy(a.row(10), kEll, 32);      // l: void
  memset(b.row(11), 0xff, 32);      // 2^256 - 1: void
  memcpy(c.row(12), kEll, 32);
  c.row(12)[0] += 1;                // l + 1: void
  a.poison_slack(true), b.poison_slack(true), out.poison_slack(true);
  a.poison_row(9, true), b.poison_row(9, true), c.poison_row(9, true);
  uint32_t rec[4];
  ht_rows_scalar(a.base(), a.stride, b.base(), b.stride, c.base(), c.stride, n, out.base(), out.stride, live.data(), done.data(), rec);
  a.poison_slack(false), b.poison_slack(false), out.poison_slack(false);
  a.poison_row(9, false), b.poison_row(9, false), c.poison_row(9, false);
  CHECK(rec[0] == n - 4 && rec[1] == 3 && rec[2] == 10 && rec[3] == (BPP_ROWS_WRITTEN | BPP_ROWS_SCALAR));
  CHECK(out.slack_untouched());
  const uint8_t zero[32] = {0};
  for (size_t i = 0; i < n; i++) {
    if (i >= 9 && i <= 12) {
      CHECK(done[i] == 0 && memcmp(out.row(i), zero, 32) == 0);
      continue;
    }
    uint8_t want[32];
    big_muladd(want, a.row(i), b.row(i), c.row(i));
    CHECK(done[i] == 1 && memcmp(out.row(i), want, 32) == 0);
  }
  // broadcast operands in each position, and c = null (rows 41 .. 48: no operand row there is zero)
  const size_t at = 41;
  for (int which = 0; which < 4; which++) {
    ht_rows_scalar(a.row(at), which == 0 ? 0 : a.stride, b.row(at), which == 1 ? 0 : b.stride, which == 3 ? nullptr : c.row(at),
                   which == 2 ? 0 : c.stride, 8, out.base(), out.stride, nullptr, done.data(), rec);
    CHECK(rec[0] == 8 && rec[1] == 0);
    for (size_t i = 0; i < 8; i++) {
      uint8_t want[32];
      big_muladd(want, a.row(at + (which == 0 ? 0 : i)), b.row(at + (which == 1 ? 0 : i)), which == 3 ? nullptr : c.row(at + (which == 2 ? 0 : i)));
      CHECK(memcmp(out.row(i), want, 32) == 0);
    }
  }
  printf("ok scalar\n");
}

void refusal_case() {
  uint8_t buf[4096];
  char msg[256];
  auto msm = [&](size_t n, uint32_t K, const uint8_t *s, size_t ss, const uint8_t *p, size_t ps, const uint8_t *o, size_t os, const uint8_t *lv,
                 const uint8_t *dm, const void *rc) {
    ht_rows_msm_refusal(n, K, s, ss, p, ps, o, os, lv, dm, rc, msg, sizeof msg);
    return std::string(msg);
  };
  uint8_t *s = buf, *p = buf + 1024, *o = buf + 2048, *lv = buf + 3000, *dm = buf + 3100, *rc = buf + 3200;
  CHECK(msm(4, 2, s, 64, p, 64, o, 32, lv, dm, rc).empty());
  CHECK(msm(4, 2, s, 64, p, 0, o, 32, nullptr, nullptr, nullptr).empty());
  CHECK(msm(0, 2, s, 64, p, 64, o, 32, lv, dm, rc) == "n is 0");
  CHECK(msm((size_t)1 << 31, 2, s, 64, p, 64, o, 32, lv, dm, rc) == "n is above 2^31 - 1");
  CHECK(msm(4, 0, s, 64, p, 64, o, 32, lv, dm, rc) == "K must be 1 .. 16");
  CHECK(msm(4, 17, s, 32 * 17, p, 32 * 17, o, 32, lv, dm, rc) == "K must be 1 .. 16");
  CHECK(msm(4, 2, s, 63, p, 64, o, 32, lv, dm, rc) == "scalar_stride is below 32 K");
  CHECK(msm(4, 2, s, 64, p, 63, o, 32, lv, dm, rc) == "point_stride is below 32 K (and not 0)");
  CHECK(msm(4, 2, s, 64, p, 64, o, 31, lv, dm, rc) == "out_stride is below 32");
  CHECK(msm(4, 2, nullptr, 64, p, 64, o, 32, lv, dm, rc) == "scalars_dev is null");
  CHECK(msm(4, 2, s, 64, nullptr, 64, o, 32, lv, dm, rc) == "points_dev is null");
  CHECK(msm(4, 2, s, 64, p, 64, nullptr, 32, lv, dm, rc) == "out_dev is null");
  CHECK(msm(4, 2, s, 64, p, 64, s + 255, 32, lv, dm, rc) == "scalars_dev and out_dev overlap");
  CHECK(msm(4, 2, s, 64, p, 64, s + 256, 32, lv, dm, rc).empty());
  CHECK(msm(4, 2, s, 64, p, 64, p + 63, 32, lv, dm, rc) == "points_dev and out_dev overlap");
  CHECK(msm(4, 2, s, 64, p, 0, p + 64, 32, lv, dm, rc).empty());  // shared bases: one row
  CHECK(msm(4, 2, s, 64, p, 64, o, 32, lv, o + 127, rc) == "out_dev and done_mask_dev overlap");
  CHECK(msm(4, 2, s, 64, p, 64, o, 32, lv, lv + 3, rc) == "live_dev and done_mask_dev overlap");
  CHECK(msm(4, 2, s, 64, p, 64, o, 32, lv, dm, dm + 3) == "done_mask_dev and record_dev overlap");
  CHECK(msm(4, 2, s, 64, p, 64, o, 32, lv, dm, s + 240) == "scalars_dev and record_dev overlap");
  CHECK(msm(4, 2, s, 64, p, 64, o, 32, p + 10, dm, rc).empty());  // two ranges that are only read may overlap
  auto scl = [&](size_t n, const uint8_t *a, size_t as, const uint8_t *b, size_t bs, const uint8_t *c, size_t cs, const uint8_t *out, size_t os) {
    ht_rows_scalar_refusal(n, a, as, b, bs, c, cs, out, os, lv, dm, rc, msg, sizeof msg);
    return std::string(msg);
  };
  CHECK(scl(4, s, 32, p, 32, nullptr, 0, o, 32).empty());
  CHECK(scl(4, s, 0, p, 0, s, 0, o, 32).empty());
  CHECK(scl(4, nullptr, 32, p, 32, nullptr, 0, o, 32) == "a.dev is null");
  CHECK(scl(4, s, 31, p, 32, nullptr, 0, o, 32) == "a.stride is below 32 (and not 0)");
  CHECK(scl(4, s, 32, p, 16, nullptr, 0, o, 32) == "b.stride is below 32 (and not 0)");
  CHECK(scl(4, s, 32, p, 32, nullptr, 0, s, 32) == "a.dev and out_dev overlap");
  CHECK(scl(4, s, 32, p, 32, nullptr, 0, p + 127, 32) == "b.dev and out_dev overlap");
  CHECK(scl(4, s, 32, p, 32, o + 31, 0, o, 32) == "c.dev and out_dev overlap");
  CHECK(scl(0, s, 32, p, 32, nullptr, 0, o, 32) == "n is 0");
  printf("ok refusals\n");
}

}  // namespace

int main() {
  const uint32_t ks[8] = {1, 2, 3, 4, 5, 8, 9, 16};
  for (uint32_t K : ks) {
    model_case(K, false);
    model_case(K, true);
  }
  cancel_case();
  void_case();
  trace_case();
  scalar_case();
  refusal_case();
  printf("all ok\n");
  return 0;
}
