// Sanitizer harness (CPU test suite only): the two concurrency protocols of lanes_host.h with integers for lanes and small structs
// for jobs and requests, built once with  g++ -fsanitize=thread  and once with  -fsanitize=address,undefined  into executables that
// tests/test_lanes_host.py runs.  A case that has to wait for an event waits on a latch, never on a clock.  Prints one "ok <case>"
// line per case and "all ok" at the end; a failed expectation prints its line and exits with 1.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <set>
#include <stdexcept>
#include <string>

#include "lanes_host.h"

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

uint64_t f(uint64_t x) { return x * 0x9e3779b97f4a7c15ull + 12345; }

// ------------------------------------------------------------------------------------------------ tickets
struct Job {
  uint64_t ticket = 0;
  bool done = false;
  uint64_t in = 0, out = 0;
  int lane = -1;
  int mode = 0;  // 1: run throws std::runtime_error, 2: run throws an int
  int code = 0;
  std::string msg;
  Latch *hold = nullptr;     // run waits for it
  Latch *started = nullptr;  // run opens it first
  std::atomic<bool> finished{false};
};
using Tickets = lanes::TicketLanes<int, Job>;

void job_run(int &lane, Job &j) {
  if (j.started) j.started->open();
  if (j.hold) j.hold->wait();
  j.lane = lane;
  if (j.mode == 1) throw std::runtime_error("boom");
  if (j.mode == 2) throw 42;
  j.out = f(j.in);
  j.finished = true;
}
void job_threw(Job &j, const char *what) {
  j.code = -1;
  j.msg = what ? what : "unexpected";
}
std::shared_ptr<Job> job_of(uint64_t in, int mode = 0, Latch *hold = nullptr, Latch *started = nullptr) {
  auto j = std::make_shared<Job>();
  j->in = in;
  j->mode = mode;
  j->hold = hold;
  j->started = started;
  return j;
}
uint64_t submit(Tickets &tl, std::shared_ptr<Job> j) {
  auto c = tl.claim();
  return tl.post(c, std::move(j));
}

void ticket_reverse_collect() {
  Tickets tl({0, 1}, 1, job_run, job_threw);
  uint64_t t[9];
  for (int k = 0; k < 9; k++) t[k] = submit(tl, job_of(100 + k));
  for (int k = 8; k >= 0; k--) {
    auto j = tl.take(t[k]);
    CHECK(j && j->done && j->ticket == t[k]);
    CHECK(j->out == f(100 + k));
    CHECK(j->lane == k % 2);
  }
  printf("ok ticket_reverse_collect\n");
}

void ticket_first_number() {
  for (uint64_t base : {(uint64_t)1, ((uint64_t)1 << 48) + 1}) {
    Tickets tl({0}, base, job_run, job_threw);
    CHECK(submit(tl, job_of(1)) == base);
    CHECK(submit(tl, job_of(2)) == base + 1);
    CHECK(tl.take(base + 1) && tl.take(base));
  }
  printf("ok ticket_first_number\n");
}

void ticket_dropped_claim() {
  Tickets tl({0}, 7, job_run, job_threw);
  CHECK(submit(tl, job_of(1)) == 7);
  {
    auto c = tl.claim();
    CHECK(c.lane() == 0);
  }  // dropped: with one lane the next claim would block for ever if the lane stayed busy
  try {
    auto c = tl.claim();
    throw std::runtime_error("a submit that fails after its claim");
  } catch (const std::runtime_error &) {
  }
  const uint64_t t = submit(tl, job_of(2));
  CHECK(t == 8);
  auto j = tl.take(t);
  CHECK(j && j->out == f(2) && j->lane == 0);
  CHECK(tl.take(7));
  printf("ok ticket_dropped_claim\n");
}

void ticket_run_throws() {
  Tickets tl({5}, 1, job_run, job_threw);
  const uint64_t a = submit(tl, job_of(1, 1)), b = submit(tl, job_of(2, 2)), c = submit(tl, job_of(3));
  auto ja = tl.take(a), jb = tl.take(b), jc = tl.take(c);
  CHECK(ja && ja->done && ja->code == -1 && ja->msg == "boom");
  CHECK(jb && jb->done && jb->code == -1 && jb->msg == "unexpected");
  CHECK(jc && jc->done && jc->code == 0 && jc->out == f(3) && jc->lane == 5);
  printf("ok ticket_run_throws\n");
}

void ticket_unknown() {
  Tickets tl({0, 1}, 1, job_run, job_threw);
  const uint64_t t = submit(tl, job_of(1));
  CHECK(!tl.take(t + 1) && !tl.peek(t + 1) && tl.done(t + 1) == lanes::TicketState::unknown);
  CHECK(!tl.take(0) && !tl.take((1ull << 48) + 1));
  CHECK(tl.take(t));
  CHECK(!tl.take(t) && tl.done(t) == lanes::TicketState::unknown);  // collected: unknown from now on
  printf("ok ticket_unknown\n");
}

void ticket_two_collectors() {
  for (int rep = 0; rep < 50; rep++) {
    Tickets tl({0}, 1, job_run, job_threw);
    Latch hold;
    const uint64_t t = submit(tl, job_of(rep, 0, &hold));
    std::atomic<int> at_take{0}, got{0};
    auto collector = [&] {
      at_take++;
      auto j = tl.take(t);
      if (j) {
        CHECK(j->done && j->out == f(rep));
        got++;
      }
    };
    std::thread x(collector), y(collector);
    while (at_take.load() < 2) std::this_thread::yield();
    for (int i = 0; i < 20; i++) std::this_thread::yield();  // (both are in take, or about to be: either way one of them wins)
    hold.open();
    x.join();
    y.join();
    CHECK(got.load() == 1);
    CHECK(!tl.take(t));
  }
  printf("ok ticket_two_collectors\n");
}

void ticket_done_states() {
  Tickets tl({0}, 1, job_run, job_threw);
  Latch hold, started;
  const uint64_t t = submit(tl, job_of(9, 0, &hold, &started));
  CHECK(tl.done(t) == lanes::TicketState::running);
  started.wait();
  CHECK(tl.done(t) == lanes::TicketState::running);
  hold.open();
  while (tl.done(t) == lanes::TicketState::running) std::this_thread::yield();
  CHECK(tl.done(t) == lanes::TicketState::done);
  CHECK(tl.take(t));
  printf("ok ticket_done_states\n");
}

void ticket_peek_then_refuse() {
  Tickets tl({0}, (1ull << 48) + 1, job_run, job_threw);
  const uint64_t t = submit(tl, job_of(4));
  {
    auto j = tl.peek(t);
    CHECK(j && j->in == 4);  // a collect looks at the job, finds its own arguments wanting and returns: the ticket stays
  }
  CHECK(tl.peek(t));
  auto j = tl.take(t);
  CHECK(j && j->out == f(4));
  CHECK(!tl.peek(t));
  printf("ok ticket_peek_then_refuse\n");
}

void ticket_shutdown() {
  Tickets tl({0, 1}, 1, job_run, job_threw);
  uint64_t t[4];
  for (int k = 0; k < 3; k++) t[k] = submit(tl, job_of(k));
  for (int k = 0; k < 3; k++)
    while (tl.done(t[k]) != lanes::TicketState::done) std::this_thread::yield();
  Latch hold, started;
  auto flying = job_of(3, 0, &hold, &started);
  t[3] = submit(tl, flying);
  started.wait();
  std::map<uint64_t, int> seen;
  bool all_finished = true;
  std::atomic<bool> returned{false};
  std::thread sd([&] {
    tl.shutdown([&](Job &j) {
      seen[j.ticket]++;
      all_finished = all_finished && j.done && j.finished.load() && flying->finished.load();
    });
    returned = true;
  });
  for (int i = 0; i < 20; i++) std::this_thread::yield();
  CHECK(!returned.load());  // a job is in flight
  hold.open();
  sd.join();
  CHECK(returned.load() && all_finished);
  CHECK(seen.size() == 4);
  for (int k = 0; k < 4; k++) CHECK(seen[t[k]] == 1);
  CHECK(!tl.take(t[0]));
  tl.shutdown([&](Job &) { CHECK(false); });  // nothing is left for a second one (the destructor's)
  printf("ok ticket_shutdown\n");
}

// ------------------------------------------------------------------------------------------------ leaders
struct Req : lanes::PoolReq {
  int id = 0;
  uint32_t weight = 1;
  int kind = 0;
  bool poolable = true;
  uint64_t in = 0, out = 0;
  int code = 0;
  Latch *queued = nullptr;  // opened from the poolable predicate: the request is in the queue once the pool's lock is free again
};
// GCC 11's ThreadSanitizer does not intercept pthread_cond_clockwait, which a steady-clock wait becomes: it would take the pool's
// mutex for held throughout a leader's wait for company and report every other thread that locks it.  So that build waits by the
// system clock (pthread_cond_timedwait); the steady-clock wait the engine instantiates runs in the ASan + UBSan build only.
#ifdef __SANITIZE_THREAD__
using Pool = lanes::LeaderPool<int, Req, std::chrono::system_clock>;
#else
using Pool = lanes::LeaderPool<int, Req>;
#endif

struct Group {
  int lane;
  std::vector<int> ids;
  size_t weight = 0;
  bool mixed = false;
};
struct Log {
  std::mutex mu;
  std::vector<Group> groups;
  void add(int lane, const std::vector<Req *> &reqs) {
    Group g;
    g.lane = lane;
    for (Req *r : reqs) {
      g.ids.push_back(r->id);
      g.weight += r->weight;
      g.mixed = g.mixed || r->kind != reqs[0]->kind;
    }
    std::lock_guard<std::mutex> lk(mu);
    groups.push_back(std::move(g));
  }
};

template <class Run>
void serve(Pool &p, Req &me, Run run) {
  p.serve(
      me,
      [&](uint32_t max_weight) {
        if (me.queued) me.queued->open();
        return me.poolable && me.weight <= max_weight;
      },
      [](const Req &r) { return (size_t)r.weight; }, [](const Req &a, const Req &b) { return a.kind == b.kind; }, run);
}
// (the request is queued, or has been and is being dealt with, once the pool's lock has been free after its predicate ran)
void wait_queued(Pool &p, Latch &l) {
  l.wait();
  (void)p.stats();
}

void leader_groups(uint32_t max_wait_us, const char *name) {
  const int T = 16, K = 50;
  Pool p({0, 1}, max_wait_us, 5, 12);
  Log log;
  auto run = [&](int &lane, const std::vector<Req *> &reqs) {
    log.add(lane, reqs);
    for (Req *r : reqs) r->out = f(r->in);
  };
  std::atomic<int> served{0};
  std::vector<std::thread> th;
  for (int k = 0; k < T; k++)
    th.emplace_back([&, k] {
      for (int c = 0; c < K; c++) {
        Req me;
        me.id = k * K + c;
        me.weight = 1 + (uint32_t)((k * 31 + c * 7) % 7);
        me.kind = (k + c / 3) % 2;
        me.in = (uint64_t)me.id * 3 + 1;
        serve(p, me, run);
        CHECK(me.out == f(me.in));  // the outcome of its own request
        served++;
      }
    });
  for (auto &x : th) x.join();
  p.drain();
  std::set<int> ids;
  size_t in_groups = 0, pooled = 0, solo = 0;
  for (const Group &g : log.groups) {
    CHECK(g.ids.size() >= 1 && g.ids.size() <= 5);
    CHECK(g.weight <= 12);
    CHECK(!g.mixed);
    for (int id : g.ids) ids.insert(id);
    in_groups += g.ids.size();
    (g.ids.size() > 1 ? pooled : solo) += g.ids.size();
  }
  CHECK(served.load() == T * K && in_groups == (size_t)T * K && ids.size() == (size_t)T * K);  // every request in exactly one group
  const lanes::PoolStats s = p.stats();
  CHECK(s.pooled_calls + s.solo_calls == (uint64_t)T * K);
  CHECK(s.pooled_calls == pooled && s.solo_calls == solo);
  CHECK(s.engine_calls == log.groups.size());
  CHECK(s.largest_pool_calls <= 5 && s.largest_pool_weight <= 12);
  printf("ok %s\n", name);
}

void leader_unpoolable_alone() {
  Pool p({0}, 0, 8, 100);
  Log log;
  Latch a_in_run, a_hold;
  auto run = [&](int &lane, const std::vector<Req *> &reqs) {
    log.add(lane, reqs);
    if (reqs[0]->id == 0) {
      a_in_run.open();
      a_hold.wait();
    }
    for (Req *r : reqs) r->out = f(r->in);
  };
  Req r[4];
  Latch q[4];
  for (int i = 0; i < 4; i++) {
    r[i].id = i;
    r[i].in = 10 + i;
    r[i].queued = &q[i];
  }
  r[3].poolable = false;
  std::vector<std::thread> th;
  th.emplace_back([&] { serve(p, r[0], run); });
  a_in_run.wait();  // the only lane is busy
  for (int i = 1; i < 4; i++) {
    th.emplace_back([&, i] { serve(p, r[i], run); });
    wait_queued(p, q[i]);  // 1 and 2 are pending when 3 arrives
  }
  a_hold.open();
  for (auto &x : th) x.join();
  for (int i = 0; i < 4; i++) CHECK(r[i].out == f(r[i].in));
  int with3 = 0;
  for (const Group &g : log.groups)
    for (int id : g.ids)
      if (id == 3) {
        with3++;
        CHECK(g.ids.size() == 1);
      }
  CHECK(with3 == 1);
  p.drain();
  printf("ok leader_unpoolable_alone\n");
}

// three requests and one lane under a wait of 20 s for up to 3 calls; `run` gets all three at once
template <class Run>
void three_at_once(Pool &p, Req (&r)[3], Run run, int *caught) {
  std::mutex mu;
  std::vector<std::thread> th;
  for (int i = 0; i < 3; i++) {
    r[i].id = i;
    r[i].in = 20 + i;
    th.emplace_back([&, i] {
      try {
        serve(p, r[i], run);
      } catch (...) {
        std::lock_guard<std::mutex> lk(mu);
        ++*caught;
      }
    });
  }
  for (auto &x : th) x.join();
}

void leader_woken_by_enqueue() {
  const uint32_t wait_us = 20u * 1000 * 1000;
  Pool p({0}, wait_us, 3, 100);
  Log log;
  auto run = [&](int &lane, const std::vector<Req *> &reqs) {
    log.add(lane, reqs);
    for (Req *q : reqs) q->out = f(q->in);
  };
  Req r[3];
  int caught = 0;
  const auto t0 = std::chrono::steady_clock::now();
  three_at_once(p, r, run, &caught);
  const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  CHECK(caught == 0);
  CHECK(log.groups.size() == 1 && log.groups[0].ids.size() == 3);
  for (auto &q : r) CHECK(q.out == f(q.in));
  CHECK(us < wait_us / 2);  // only the notification of the third enqueue ends the leader's wait this early
  printf("ok leader_woken_by_enqueue\n");
}

void leader_run_throws() {
  Pool p({0}, 20u * 1000 * 1000, 3, 100);
  size_t group = 0;
  auto run = [&](int &, const std::vector<Req *> &reqs) {
    group = reqs.size();
    for (Req *q : reqs) q->code = 7;  // (what a client's wrapper leaves before the failure gets past it)
    throw 42;
  };
  Req r[3];
  int caught = 0;
  three_at_once(p, r, run, &caught);
  CHECK(group == 3 && caught == 1);  // the leader's caller sees the exception; both followers came back
  for (auto &q : r) CHECK(q.code == 7);
  Req after;
  after.poolable = false;
  after.in = 5;
  serve(p, after, [&](int &, const std::vector<Req *> &reqs) { reqs[0]->out = f(reqs[0]->in); });  // the lane is free
  CHECK(after.out == f(5));
  p.drain();
  printf("ok leader_run_throws\n");
}

void leader_drain() {
  Pool p({0}, 0, 8, 100);
  Latch a_in_run, a_hold, b_queued;
  std::atomic<int> runs_done{0};
  auto run = [&](int &, const std::vector<Req *> &reqs) {
    if (reqs[0]->id == 0) {
      a_in_run.open();
      a_hold.wait();
    }
    for (Req *q : reqs) q->out = f(q->in);
    runs_done++;
  };
  { // nothing queued, nothing running: at once
    p.drain();
  }
  Req a, b;
  a.id = 0;
  b.id = 1;
  b.queued = &b_queued;
  std::thread ta([&] { serve(p, a, run); });
  a_in_run.wait();
  std::thread tb([&] { serve(p, b, run); });
  wait_queued(p, b_queued);  // a lane busy and a request pending
  int seen_at_return = -1;
  std::atomic<bool> returned{false};
  std::thread td([&] {
    p.drain();
    seen_at_return = runs_done.load();
    returned = true;
  });
  for (int i = 0; i < 20; i++) std::this_thread::yield();
  CHECK(!returned.load());
  a_hold.open();
  ta.join();
  tb.join();
  td.join();
  CHECK(seen_at_return == 2);  // both the running call and the queued one were over
  printf("ok leader_drain\n");
}

}  // namespace

int main() {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  ticket_reverse_collect();
  ticket_first_number();
  ticket_dropped_claim();
  ticket_run_throws();
  ticket_unknown();
  ticket_two_collectors();
  ticket_done_states();
  ticket_peek_then_refuse();
  ticket_shutdown();
  leader_groups(0, "leader_groups_no_wait");
  leader_groups(200, "leader_groups_wait_200us");
  leader_unpoolable_alone();
  leader_woken_by_enqueue();
  leader_run_throws();
  leader_drain();
  printf("all ok\n");
  return 0;
}
