// Sanitizer harness (CPU test suite only): the verdict resolution of verdict.h -- what k_verdict_scan and k_verdict_finish run
// behind the final MSM of bpp_verify_enqueue -- on the host, held to the host rules of the blocking calls: check_deferred +
// check_chunk_errors (upload_host.h) and the final-check line of verify_flow_once, texts included.
//   exhaustive   groups of 1-3 proofs over every (status 0..7, rounds_bad in {0, InvalidLength, SizeOverflow}, defer 0..3) per proof
//                x identity flag x three actions x zero-weight flag (x whether the call ran the final MSM at all)
//   random       10 000 seeded groups of up to 600 proofs with sparse findings
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_verdict_host.py runs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "upload_host.h"
#include "verdict.h"

using namespace bpp;

static_assert(BPP_VERDICT_DEFER_DEGREE == BPP_DEFER_DEGREE && BPP_VERDICT_DEFER_PROMISE == BPP_DEFER_PROMISE, "deferred bits");
static_assert(sizeof(bpp_device_verdict) == 16, "the record is 16 bytes");

namespace {

struct Want {
  int code = BPP_OK, tier = BPP_TIER_NONE;
  uint32_t index = 0;
  std::string msg;
};

// the host rules over one group's proofs, as the blocking calls run them (no MSM line yet)
Want host_finding(const std::vector<uint32_t> &status, const std::vector<uint8_t> &rounds_bad, const std::vector<uint8_t> &defer) {
  Want w;
  try {
    check_deferred(defer, 0, (uint32_t)defer.size());
    check_chunk_errors(status.data(), rounds_bad.data(), 0, (uint32_t)status.size());
  } catch (const ProofErr &e) {
    w.code = e.code;
    w.tier = e.tier;
    w.index = e.index;
    w.msg = e.msg;
  }
  return w;
}

// ... and the final-check line behind them (engine.hip, verify_flow_once)
Want host_verdict(const Want &found, bool want_msm, int action, bool ident) {
  if (found.tier != BPP_TIER_NONE) return found;
  Want w;
  try {
    if (want_msm && action != BPP_RECOVER_ONLY && !ident)
      throw ProofErr{BPP_ERR_VERIFICATION_FAILED, "Range proof batch not valid", BPP_TIER_MSM, 0};
  } catch (const ProofErr &e) {
    w.code = e.code;
    w.tier = e.tier;
    w.index = e.index;
    w.msg = e.msg;
  }
  return w;
}

uint64_t group_key(const std::vector<uint32_t> &status, const std::vector<uint8_t> &rounds_bad, const std::vector<uint8_t> &defer, bool backwards) {
  uint64_t key = BPP_VERDICT_KEY_NONE;
  const size_t n = status.size();
  for (size_t k = 0; k < n; k++) {
    const size_t p = backwards ? n - 1 - k : k;  // (the device folds its keys in no particular order)
    key = verdict_min(key, verdict_key(defer[p], status[p], rounds_bad[p], (uint32_t)p));
  }
  return key;
}

long failures = 0;
void fail(const char *what, const Want &w, const bpp_device_verdict &v) {
  if (failures++ < 20)
    printf("FAIL %s: host %d/%d/%u '%s', shared %d/%u/%u flags %u '%s'\n", what, w.code, w.tier, w.index, w.msg.c_str(), v.code, v.tier, v.index,
           v.flags, verdict_message(v.tier, v.code));
}

// one group under every (want_msm, action, identity, zero weight)
void check_group(const char *what, const std::vector<uint32_t> &status, const std::vector<uint8_t> &rounds_bad, const std::vector<uint8_t> &defer) {
  const Want found = host_finding(status, rounds_bad, defer);
  const uint64_t key = group_key(status, rounds_bad, defer, false);
  if (key != group_key(status, rounds_bad, defer, true)) {
    failures++;
    printf("FAIL %s: the minimum depends on the order\n", what);
  }
  for (int want_msm = 0; want_msm < 2; want_msm++)
    for (int action = 0; action < 3; action++)
      for (int ident = 0; ident < 2; ident++)
        for (int zero = 0; zero < 2; zero++) {
          const bpp_device_verdict v = verdict_finish(key, want_msm != 0, action, ident != 0, zero != 0);
          if (!(v.flags & BPP_VERDICT_WRITTEN)) fail(what, found, v);
          if (zero && want_msm && action != BPP_RECOVER_ONLY) {  // a redraw claims nothing else
            if (v.flags != (BPP_VERDICT_WRITTEN | BPP_VERDICT_REDRAW) || v.code != BPP_OK || v.tier != BPP_TIER_NONE || v.index != 0) fail(what, found, v);
            continue;
          }
          const Want w = host_verdict(found, want_msm != 0, action, ident != 0);
          if (v.flags != BPP_VERDICT_WRITTEN || v.code != w.code || (int)v.tier != w.tier || v.index != w.index ||
              w.msg != verdict_message(v.tier, v.code))
            fail(what, w, v);
        }
}

void exhaustive() {
  const uint8_t rb_of[3] = {0, BPP_ERR_INVALID_LENGTH, BPP_ERR_SIZE_OVERFLOW};
  const uint32_t per = 8 * 3 * 4;
  for (uint32_t n = 1; n <= 3; n++) {
    uint32_t total = 1;
    for (uint32_t k = 0; k < n; k++) total *= per;
    std::vector<uint32_t> status(n);
    std::vector<uint8_t> rounds_bad(n), defer(n);
    for (uint32_t c = 0; c < total; c++) {
      uint32_t x = c;
      for (uint32_t p = 0; p < n; p++) {
        const uint32_t s = x % per;
        x /= per;
        status[p] = s % 8;
        rounds_bad[p] = rb_of[(s / 8) % 3];
        defer[p] = (uint8_t)(s / 24);
      }
      check_group("exhaustive", status, rounds_bad, defer);
    }
    printf("ok exhaustive_%u\n", n);
  }
}

void random_groups() {
  std::mt19937_64 rng(20261020);
  const uint8_t rb_of[3] = {0, BPP_ERR_INVALID_LENGTH, BPP_ERR_SIZE_OVERFLOW};
  for (int it = 0; it < 10000; it++) {
    const uint32_t n = 1 + (uint32_t)(rng() % 600);
    std::vector<uint32_t> status(n, 0);
    std::vector<uint8_t> rounds_bad(n, 0), defer(n, 0);
    const uint32_t findings = (uint32_t)(rng() % 5);  // sparse: none to four proofs with something
    for (uint32_t f = 0; f < findings; f++) {
      const uint32_t p = (uint32_t)(rng() % n);
      switch (rng() % 3) {
        case 0: status[p] |= 1u << (rng() % 3); break;
        case 1: rounds_bad[p] = rb_of[1 + rng() % 2]; break;
        default: defer[p] |= (uint8_t)(1u << (rng() % 2)); break;
      }
    }
    check_group("random", status, rounds_bad, defer);
  }
  printf("ok random_groups\n");
}

// every (tier, code) pair a check raises has its text; the record of an untouched key says Ok
void texts() {
  const bpp_device_verdict ok = verdict_finish(BPP_VERDICT_KEY_NONE, true, BPP_VERIFY_ONLY, true, false);
  if (ok.code != BPP_OK || ok.tier != BPP_TIER_NONE || strlen(verdict_message(ok.tier, ok.code)) != 0) failures++;
  for (uint32_t tier = BPP_TIER_DEGREE; tier <= BPP_TIER_MSM; tier++)
    for (uint32_t sub = 0; sub < (tier == BPP_TIER_PASS2 ? 3u : 1u); sub++)
      if (strlen(verdict_message(tier, verdict_code(tier, sub))) == 0) {
        failures++;
        printf("FAIL texts: tier %u sub %u has no text\n", tier, sub);
      }
  printf("ok texts\n");
}

}  // namespace

int main() {
  exhaustive();
  random_groups();
  texts();
  if (failures) {
    printf("FAIL %ld mismatches\n", failures);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
