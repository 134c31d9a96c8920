// Sanitizer harness (CPU test suite only): the host runtime of runtime_host.h (small-call gate, worker pool, wait schedule) and the
// chain scheduler of chain_host.h, built once with  g++ -fsanitize=thread  and once with  -fsanitize=address,undefined  into
// executables that tests/test_runtime_host.py runs.  A case that has to wait for another thread waits on a latch or on a counter
// of the code under test, never on a clock.  Prints one "ok <case>" line per case and "all ok" at the end; a failed expectation
// prints its line and exits with 1.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "chain_host.h"
#include "runtime_host.h"

using namespace bpp;

namespace {

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      fflush(stdout);                                             \
      exit(1);                                                    \
    }                                                             \
  } while (0)

struct Latch {
  std::mutex mu;
  std::condition_variable cv;
  bool open_ = false;
  void open() {
    {
      std::lock_guard<std::mutex> lk(mu);
      open_ = true;
    }
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return open_; });
  }
};

// ------------------------------------------------------------------------------------------------ gate
struct Counters {
  uint32_t limit, in_flight;
  uint64_t small_calls, queued;
  size_t waiting;
};
Counters counters(DeviceState &D) {
  std::lock_guard<std::mutex> lk(D.mu);
  return {D.limit, D.in_flight, D.small_calls, D.small_calls_queued, D.queue.size()};
}
template <class Pred>
void until(Pred p) {
  while (!p()) std::this_thread::yield();
}

// callers that take the gate, say so, and hold it until told to leave
struct Callers {
  DeviceState &D;
  std::mutex mu;
  std::vector<int> order;  // who got in, in that order
  int inside = 0, inside_max = 0;
  std::vector<std::unique_ptr<Latch>> leave;
  std::vector<std::thread> th;
  explicit Callers(DeviceState &d) : D(d) {}
  void start() {
    const int id = (int)th.size();
    leave.emplace_back(new Latch());
    Latch *l = leave.back().get();
    th.emplace_back([this, id, l] {
      GateHold hold(D, true);
      {
        std::lock_guard<std::mutex> lk(mu);
        order.push_back(id);
        inside_max = std::max(inside_max, ++inside);
      }
      l->wait();
      std::lock_guard<std::mutex> lk(mu);
      inside--;
    });
  }
  size_t entered() {
    std::lock_guard<std::mutex> lk(mu);
    return order.size();
  }
  void join() {
    for (auto &t : th) t.join();
  }
};

void gate_fifo_under_limit() {
  DeviceState D;
  D.limit = 2;
  Callers c(D);
  for (int i = 0; i < 6; i++) {
    c.start();
    if (i < 2) until([&] { return counters(D).in_flight == (uint32_t)i + 1; });
    else until([&] { return counters(D).queued == (uint64_t)i - 1; });  // it is in the queue before the next one arrives
  }
  CHECK(c.entered() == 2 && counters(D).waiting == 4);
  for (int i = 0; i < 6; i++) {
    c.leave[i]->open();  // one leaves, the oldest waiter comes in
    if (i < 4) until([&] { return c.entered() == (size_t)i + 3; });
    CHECK(counters(D).in_flight <= 2);
  }
  c.join();
  CHECK(c.inside_max <= 2);
  for (int i = 0; i < 6; i++) CHECK(c.order[i] == i);
  const Counters k = counters(D);
  CHECK(k.small_calls == 6 && k.queued == 4 && k.in_flight == 0 && k.waiting == 0);
  printf("ok gate_fifo_under_limit\n");
}

void gate_reentrant() {
  DeviceState D;
  D.limit = 1;
  {
    GateHold outer(D, true);
    CHECK(counters(D).small_calls == 1 && counters(D).in_flight == 1);
    {
      GateHold inner(D, true);  // would wait for ever if it queued
      CHECK(counters(D).small_calls == 1 && counters(D).in_flight == 1);
    }
    CHECK(counters(D).in_flight == 1);
  }
  CHECK(counters(D).in_flight == 0 && counters(D).queued == 0);
  {
    GateHold again(D, true);  // the depth is back at 0: a call of its own
    CHECK(counters(D).small_calls == 2 && counters(D).in_flight == 1);
  }
  CHECK(counters(D).in_flight == 0);
  printf("ok gate_reentrant\n");
}

void gate_off() {
  DeviceState D;
  D.limit = 0;
  Callers c(D);
  for (int i = 0; i < 3; i++) c.start();
  until([&] { return c.entered() == 3; });  // all three inside at once
  CHECK(counters(D).small_calls == 3 && counters(D).in_flight == 0 && counters(D).queued == 0);
  {
    GateHold a(D, true), b(D, true);  // one thread: counted each time, the depth is not kept
    CHECK(counters(D).small_calls == 5 && counters(D).in_flight == 0);
  }
  for (auto &l : c.leave) l->open();
  c.join();
  CHECK(counters(D).small_calls == 5 && counters(D).in_flight == 0 && counters(D).queued == 0);
  printf("ok gate_off\n");
}

void gate_large_passes() {
  DeviceState D;
  D.limit = 1;
  GateHold small_one(D, true);
  {
    GateHold a(D, false), b(D, false);  // the gate is full: a small call would wait
    const Counters k = counters(D);
    CHECK(k.small_calls == 1 && k.in_flight == 1 && k.queued == 0 && k.waiting == 0);
  }
  const Counters k = counters(D);
  CHECK(k.small_calls == 1 && k.in_flight == 1 && k.queued == 0);
  printf("ok gate_large_passes\n");
}

void gate_widen_and_remove() {
  DeviceState D;
  CHECK(D.set_limit(1) == 12);
  Callers c(D);
  c.start();
  until([&] { return counters(D).in_flight == 1; });
  for (int i = 1; i < 4; i++) {
    c.start();
    until([&] { return counters(D).queued == (uint64_t)i; });
  }
  CHECK(c.entered() == 1 && counters(D).waiting == 3);
  CHECK(D.set_limit(2) == 1);  // (set_limit itself counts the admitted in: the counters are right when it returns)
  CHECK(counters(D).in_flight == 2 && counters(D).waiting == 2);  // exactly one more
  until([&] { return c.entered() == 2; });
  CHECK(c.order[0] == 0 && c.order[1] == 1);  // the oldest waiter (the other two come in together below, in either order)
  CHECK(D.set_limit(-1) == 2 && counters(D).limit == 2);  // a negative limit only asks
  CHECK(D.set_limit(0) == 2);
  CHECK(counters(D).in_flight == 4 && counters(D).waiting == 0);
  until([&] { return c.entered() == 4; });
  CHECK(D.set_limit(-1) == 0);
  for (auto &l : c.leave) l->open();
  c.join();
  const Counters k = counters(D);
  CHECK(k.in_flight == 0 && k.small_calls == 4 && k.queued == 3);
  printf("ok gate_widen_and_remove\n");
}

void env_long() {
  long v = -7;
  CHECK(parse_env_long("0", 0, 100, &v) && v == 0);
  CHECK(parse_env_long("12", 0, 100, &v) && v == 12);
  CHECK(parse_env_long("100", 0, 100, &v) && v == 100);
  CHECK(parse_env_long("5", 5, 100, &v) && v == 5);
  v = -7;
  CHECK(!parse_env_long("", 0, 100, &v) && v == -7);
  CHECK(!parse_env_long(nullptr, 0, 100, &v) && v == -7);
  CHECK(!parse_env_long("12x", 0, 100, &v) && v == -7);
  CHECK(!parse_env_long("x", 0, 100, &v) && v == -7);
  CHECK(!parse_env_long("-1", 0, 100, &v) && v == -7);
  CHECK(!parse_env_long("4", 5, 100, &v) && v == -7);
  CHECK(!parse_env_long("101", 0, 100, &v) && v == -7);
  CHECK(!parse_env_long("99999999999999999999999", 0, 100, &v) && v == -7);
  printf("ok env_long\n");
}

// ------------------------------------------------------------------------------------------------ pool
void pool_size_from_env() {
  CHECK(HostPool::get().size() == 4 && host_pool_size() == 4);
  printf("ok pool_size_from_env\n");
}

void covers_once(uint32_t n) {
  std::vector<std::atomic<int>> hits(n);
  for (auto &h : hits) h = 0;
  host_parallel_for(n, [&](uint32_t i) {
    CHECK(i < n);
    hits[i]++;
  });
  for (auto &h : hits) CHECK(h.load() == 1);
}
void pool_covers_once() {
  const uint32_t sizes[] = {0, 1, 2, 3, 4, 5, 1000};
  for (uint32_t n : sizes) covers_once(n);
  std::vector<std::thread> th;
  for (int k = 0; k < 4; k++)
    th.emplace_back([&] {
      for (uint32_t n : sizes) covers_once(n);
    });
  for (auto &t : th) t.join();
  printf("ok pool_covers_once\n");
}

void pool_idle_not_busy() {
  HostPool &pool = HostPool::get();
  CHECK(pool.busy() == 0);
  std::atomic<uint32_t> seen{0};
  pool.parallel_for(4, [&](uint32_t) {
    const uint32_t b = pool.busy();
    uint32_t s = seen.load();
    while (b > s && !seen.compare_exchange_weak(s, b)) {
    }
  });
  CHECK(seen.load() >= 1);
  CHECK(pool.busy() == 0);
  printf("ok pool_idle_not_busy\n");
}

void pool_cpu_ns_counts() {
  const uint64_t before = host_pool_cpu_ns();
  host_parallel_for(2, [](uint32_t) {
    const uint64_t t0 = HostPool::thread_cpu_ns();
    while (HostPool::thread_cpu_ns() - t0 < 3000000ull) {
    }
  });
  CHECK(host_pool_cpu_ns() - before >= 3000000ull);  // (each of the two items alone spent that much inside a job)
  printf("ok pool_cpu_ns_counts\n");
}

void quota_cpus() {
  CHECK(cpus_from_quota(200000, 100000) == 2);
  CHECK(cpus_from_quota(150000, 100000) == 2);
  CHECK(cpus_from_quota(50000, 100000) == 1);
  CHECK(cpus_from_quota(10000, 100000) == 1);
  printf("ok cpus_from_quota\n");
}

// ------------------------------------------------------------------------------------------------ chain scheduler
void chain_width_rule() {
  CHECK(chain_bundle_width(64, 16, 0, 8, -1) == 8);
  CHECK(chain_bundle_width(32, 16, 0, 8, -1) == 1);
  CHECK(chain_bundle_width(32, 16, 1, 8, -1) == 8);
  CHECK(chain_bundle_width(15, 16, 1, 8, -1) == 1);
  CHECK(chain_bundle_width(16, 4, 0, 8, -1) == 8);
  CHECK(chain_bundle_width(8, 16, 1, 4, -1) == 1);  // 2 G > pool fails
  for (uint32_t G : {1u, 8u, 64u, 1000u})
    for (uint32_t pool : {1u, 4u, 16u, 256u})
      for (uint32_t busy : {0u, 3u}) {
        for (uint32_t simd : {1u, 4u, 8u}) {
          CHECK(chain_bundle_width(G, pool, busy, simd, 0) == 1);
          CHECK(chain_bundle_width(G, pool, busy, simd, 1) == simd);
        }
        CHECK(chain_bundle_width(G, pool, busy, 1, -1) == 1);
      }
  printf("ok chain_width_rule\n");
}

void chain_units_ragged() {
  const uint32_t first[6] = {0, 5, 10, 15, 18, 23};  // group sizes 5, 5, 5, 3, 5
  typedef std::vector<std::pair<uint32_t, uint32_t>> Units;
  CHECK((chain_units(first, 5, 4) == Units{{0, 3}, {3, 1}, {4, 1}}));
  CHECK((chain_units(first, 5, 1) == Units{{0, 1}, {1, 1}, {2, 1}, {3, 1}, {4, 1}}));
  CHECK(chain_units(first, 0, 4).empty());
  printf("ok chain_units_ragged\n");
}

void chains_lockstep_equals_scalar() {
  const uint32_t G = 19;
  std::vector<uint32_t> first(G + 1, 0);
  for (uint32_t g = 0; g < G; g++) first[g + 1] = first[g] + (g < 17 ? 7u : 3u);
  const uint32_t B = first[G];
  std::vector<uint8_t> rng((size_t)B * 32);
  uint64_t x = 0x243f6a8885a308d3ull;
  for (auto &b : rng) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    b = (uint8_t)(x >> 56);
  }
  const uint32_t simd = chain_simd_width();
  for (int wide = 0; wide < 2; wide++) {
    const size_t bytes = (size_t)B * (wide ? 64 : 32);
    std::vector<uint8_t> a(bytes, 0xaa), b(bytes, 0x55);
    run_weight_chains_width(rng.data(), a.data(), first.data(), G, wide != 0, 1);
    run_weight_chains_width(rng.data(), b.data(), first.data(), G, wide != 0, simd);
    CHECK(memcmp(a.data(), b.data(), bytes) == 0);
    if (!wide) {  // what the library's entry runs, whatever width it takes
      std::vector<uint8_t> c(bytes, 0x33);
      run_weight_chains_generic(rng.data(), c.data(), first.data(), G);
      CHECK(memcmp(a.data(), c.data(), bytes) == 0);
    }
  }
  printf("ok chains_lockstep_equals_scalar\n");
}

// ------------------------------------------------------------------------------------------------ wait schedule
// (waited us -> nap us) in the order given, on ONE schedule object
struct Step {
  long waited, nap;
};
void expect_naps(uint32_t hint, bool tail_spin, std::initializer_list<Step> steps) {
  WaitSchedule s{hint, tail_spin};
  for (const Step &st : steps) {
    const long got = s.next_nap_us(st.waited);
    if (got != st.nap) printf("hint %u tail_spin %d waited %ld: nap %ld, expected %ld\n", hint, (int)tail_spin, st.waited, got, st.nap);
    CHECK(got == st.nap);
  }
}

void wait_cold() {
  expect_naps(0, false, {{10, 0}, {30, 50}, {399, 50}, {400, 50}, {1600, 200}, {3200, 400}, {10000, 400}});
  printf("ok wait_cold\n");
}
void wait_remembered() {
  expect_naps(10000, false, {{40, 4960}, {5100, 50}, {12499, 50}, {12500, 400}});
  printf("ok wait_remembered\n");
}
void wait_late_first_look() {
  expect_naps(10000, false, {{6000, 400}});  // nothing was slept ahead: the naps grow
  printf("ok wait_late_first_look\n");
}
void wait_floor() {
  expect_naps(700, false, {{340, 50}});  // 350 - 340 = 10, raised to the floor
  printf("ok wait_floor\n");
}
void wait_tail_spin() {
  expect_naps(10000, true, {{40, 6960}, {7100, 0}, {9000, 0}, {12500, 0}, {100000, 0}});
  expect_naps(600, true, {{10, 0}, {40, 0}, {250, 0}, {400, 0}, {5000, 0}});
  expect_naps(601, true, {{40, 380}});
  expect_naps(0, true, {{10, 0}, {40, 0}, {400, 0}, {5000, 0}, {1000000, 0}});
  printf("ok wait_tail_spin\n");
}
void wait_hint_fold_case() {
  WaitHint h;
  wait_hint_fold(&h, 1234);
  CHECK(h.us == 1234);
  h.us = 1000;
  wait_hint_fold(&h, 2000);
  CHECK(h.us == 1250);
  wait_hint_begin(&h, 0);  // the key it has: kept
  CHECK(h.us == 1250 && h.key == 0);
  wait_hint_begin(&h, 77);
  CHECK(h.us == 0 && h.key == 77);
  wait_hint_fold(&h, 500);
  wait_hint_begin(&h, 77);
  CHECK(h.us == 500 && h.key == 77);
  wait_hint_begin(nullptr, 5);  // no memory: nothing to do
  wait_hint_fold(nullptr, 5);
  printf("ok wait_hint_fold\n");
}
void nap_timespec_case() {
  struct timespec a = nap_timespec(2500000), b = nap_timespec(50), c = nap_timespec(1000000);
  CHECK(a.tv_sec == 2 && a.tv_nsec == 500000000);
  CHECK(b.tv_sec == 0 && b.tv_nsec == 50000);
  CHECK(c.tv_sec == 1 && c.tv_nsec == 0);
  printf("ok nap_timespec\n");
}

}  // namespace

int main() {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  setenv("BPP_HOST_THREADS", "4", 1);  // before the pool is first touched
  gate_fifo_under_limit();
  gate_reentrant();
  gate_off();
  gate_large_passes();
  gate_widen_and_remove();
  env_long();
  pool_size_from_env();
  pool_covers_once();
  pool_idle_not_busy();
  pool_cpu_ns_counts();
  quota_cpus();
  chain_width_rule();
  chain_units_ragged();
  chains_lockstep_equals_scalar();
  wait_cold();
  wait_remembered();
  wait_late_first_look();
  wait_floor();
  wait_tail_spin();
  wait_hint_fold_case();
  nap_timespec_case();
  printf("all ok\n");
  return 0;
}
