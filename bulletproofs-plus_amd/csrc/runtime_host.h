// The host runtime around the engine's calls, with no HIP and no engine type in it: hosttest_runtime.cpp drives all of it on a CPU
// under ThreadSanitizer and ASan + UBSan.
//
//   DeviceState, GateHold   the per-device admission gate for small calls and the contexts' bookkeeping, under one mutex
//   HostPool                persistent host workers (weight chains, parsing), sized by the CPUs this process may really use
//   WaitHint, WaitSchedule  how long a caller naps between two looks at an event it waits for (the looking is the engine's)
#pragma once
#include <errno.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace bpp {

// a whole decimal number in [lo, hi] from an environment variable; false (and *out untouched) for anything else -- a typo must
// not silently become 0, which for a deadline means "none" and for the small-call gate "off"
inline bool parse_env_long(const char *text, long lo, long hi, long *out) {
  if (!text || !*text) return false;
  char *end = nullptr;
  errno = 0;
  const long v = strtol(text, &end, 10);
  while (end && (*end == ' ' || *end == '\t')) end++;
  if (errno || end == text || (end && *end) || v < lo || v > hi) return false;
  *out = v;
  return true;
}

// ------------------------------------------------------------------ per-device runtime state: admission gate, bookkeeping
// A SMALL call (one reference batch of up to a few hundred proofs: what separate callers of RangeProof::verify_batch issue,
// src/range_proof.rs:73-76,712-752) is a chain of about fifteen latency-bound kernels with tiny grids.  The chip runs about
// six such chains side by side; more callers than that add nothing, and many more take it away: 8-16 callers with a context
// each reached 5.3 k calls/s, 32 callers 2.6 k, 64 callers 1.6 k (profiles/r03_v10_calls_in_flight.jsonl) -- every context
// brings a stream and a side stream, the runtime multiplexes them onto its hardware queues (GPU_MAX_HW_QUEUES, 4 unless the
// host sets more) and streams that share a queue serialise behind each other's kernels.  So the library admits at most
// `limit` small calls per device at a time (BPP_SMALL_CALLS_IN_FLIGHT, default 12; bpp_small_call_limit); the others wait
// their turn in arrival order, on the host, holding nothing.  Large calls (they fill the chip by themselves) pass freely.
struct DeviceState {
  std::mutex mu;
  struct Waiter {
    std::condition_variable cv;
    bool go = false;
  };
  std::deque<Waiter *> queue;
  uint32_t limit = 12, in_flight = 0;
  uint64_t small_calls = 0, small_calls_queued = 0;
  uint32_t contexts = 0, contexts_peak = 0;
  bool warned = false;
  std::string env_note;  // a malformed BPP_SMALL_CALLS_IN_FLIGHT: said once, where bpp_ctx_last_error finds it

  // lets waiting calls in, oldest first, while the gate has room (or is off); `mu` is held.  The releasing thread counts the
  // call in: a woken waiter finds its place taken
  void admit_waiting() {
    while (!queue.empty() && (limit == 0 || in_flight < limit)) {
      Waiter *w = queue.front();
      queue.pop_front();
      in_flight++;
      w->go = true;
      w->cv.notify_one();
    }
  }
  // a new limit (0: no gate; negative: none, the call only asks); a wider or removed gate lets waiting calls in.  Returns the
  // limit before the call
  int set_limit(int new_limit) {
    std::lock_guard<std::mutex> lk(mu);
    const int before = (int)limit;
    if (new_limit >= 0) {
      limit = (uint32_t)new_limit;
      admit_waiting();
    }
    return before;
  }
};
inline DeviceState &device_state(int dev) {
  static std::mutex mu;
  static std::map<int, DeviceState *> *all = new std::map<int, DeviceState *>();  // leaked: contexts may outlive static destruction
  std::lock_guard<std::mutex> lk(mu);
  DeviceState *&d = (*all)[dev];
  if (!d) {
    d = new DeviceState();
    if (const char *e = getenv("BPP_SMALL_CALLS_IN_FLIGHT")) {  // 0: no gate
      long v = 0;
      if (parse_env_long(e, 0, 1 << 20, &v)) d->limit = (uint32_t)v;
      else d->env_note = std::string("note: BPP_SMALL_CALLS_IN_FLIGHT=\"") + e + "\" is not a number: the default gate (12 calls) stands";
    }
  }
  return *d;
}
// hardware queues the HIP runtime multiplexes this process' streams onto: read once at its start-up from GPU_MAX_HW_QUEUES
inline uint32_t runtime_hw_queues() {
  static const uint32_t q = [] {
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? (uint32_t)v : 4u;
  }();
  return q;
}
static thread_local int tl_gate_depth = 0;  // a thread that holds the gate passes it again (upload + verify of one call)
struct GateHold {
  DeviceState *d = nullptr;
  GateHold(DeviceState &D, bool small) {
    if (!small) return;
    if (tl_gate_depth++ > 0) {
      held_outer = true;
      return;
    }
    std::unique_lock<std::mutex> lk(D.mu);
    D.small_calls++;
    if (D.limit == 0) {  // gate switched off: counted, never held
      tl_gate_depth--;
      return;
    }
    d = &D;
    if (D.in_flight < D.limit && D.queue.empty()) {
      D.in_flight++;
      return;
    }
    D.small_calls_queued++;
    DeviceState::Waiter w;
    D.queue.push_back(&w);
    w.cv.wait(lk, [&] { return w.go; });  // the releasing thread has already counted this call in
  }
  ~GateHold() {
    if (held_outer) {
      tl_gate_depth--;
      return;
    }
    if (!d) return;
    tl_gate_depth--;
    std::lock_guard<std::mutex> lk(d->mu);
    d->in_flight--;
    d->admit_waiting();
  }
  GateHold(const GateHold &) = delete;
  GateHold &operator=(const GateHold &) = delete;

 private:
  bool held_outer = false;
};

// ------------------------------------------------------------------ host workers
// CPUs a cgroup's quota lets a process use: quota / period rounded to the nearest, one at least
inline long long cpus_from_quota(long long quota, long long period) { return std::max<long long>(1, (quota + period / 2) / period); }

// Persistent host workers for the weight chains (spawning threads per call costs more than a 1024-proof chain).
class HostPool {
 public:
  static HostPool &get() {
    static HostPool *p = new HostPool();  // leaked on purpose: detached workers may still wait at process exit
    return *p;
  }
  uint32_t size() const { return (uint32_t)workers_.size() + 1; }
  // calls that have work queued on the pool right now (a hint for the chain scheduler, nothing is promised)
  uint32_t busy() {
    std::lock_guard<std::mutex> lk(mu_);
    return (uint32_t)jobs_.size();
  }
  // run fn(i) for i in [0, n) on the pool + the calling thread; returns when all are done
  void parallel_for(uint32_t n, const std::function<void(uint32_t)> &fn) {
    if (n == 0) return;
    if (n == 1 || workers_.empty()) {
      CpuSpan span;
      for (uint32_t i = 0; i < n; i++) fn(i);
      return;
    }
    auto job = std::make_shared<Job>();
    job->fn = &fn;
    job->n = n;
    {
      std::lock_guard<std::mutex> lk(mu_);
      jobs_.push_back(job);
    }
    cv_.notify_all();
    work_on(*job);
    std::unique_lock<std::mutex> lk(job->mu);
    job->cv.wait(lk, [&] { return job->done.load() == n; });
    std::lock_guard<std::mutex> lk2(mu_);
    for (auto it = jobs_.begin(); it != jobs_.end(); ++it)
      if (it->get() == job.get()) {
        jobs_.erase(it);
        break;
      }
  }

 private:
  struct Job {
    const std::function<void(uint32_t)> *fn;
    uint32_t n;
    std::atomic<uint32_t> next{0}, done{0};
    std::mutex mu;
    std::condition_variable cv;
  };
  // host threads this process may really run at once: the affinity mask, capped by a cgroup CPU quota when there is one (a
  // 1-GPU box of the pool reports 256 logical CPUs and schedules 16: sized by hardware_concurrency() the pool had 32 workers
  // there, and the chain scheduler, which compares the number of chains with the pool, took 64 chains of 4096 proofs for
  // "few": scalar chains, 10 ms per call instead of 2 ms as eight lock-step bundles)
  static uint32_t usable_cpus() {
    uint32_t n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) n = std::min<uint32_t>(n, (uint32_t)CPU_COUNT(&set));
    auto read2 = [](const char *path, long long &a, long long &b, bool &a_is_max) {
      FILE *f = fopen(path, "r");
      if (!f) return false;
      char w[64] = {0};
      a_is_max = false;
      bool ok = false;
      if (fscanf(f, "%63s %lld", w, &b) == 2) {
        ok = true;
        if (strcmp(w, "max") == 0) a_is_max = true;
        else a = atoll(w);
      }
      fclose(f);
      return ok;
    };
    long long q = 0, per = 0;
    bool is_max = false;
    if (read2("/sys/fs/cgroup/cpu.max", q, per, is_max)) {  // cgroup v2: "<quota|max> <period>"
      if (!is_max && q > 0 && per > 0) n = std::min<uint32_t>(n, (uint32_t)cpus_from_quota(q, per));
    } else {  // cgroup v1
      FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"), *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
      if (fq && fp && fscanf(fq, "%lld", &q) == 1 && fscanf(fp, "%lld", &per) == 1 && q > 0 && per > 0)
        n = std::min<uint32_t>(n, (uint32_t)cpus_from_quota(q, per));
      if (fq) fclose(fq);
      if (fp) fclose(fp);
    }
    return std::max(1u, n);
  }
  HostPool() {
    uint32_t hw = usable_cpus();
    const char *e = getenv("BPP_HOST_THREADS");
    uint32_t want = e ? (uint32_t)atoi(e) : std::min(hw, 32u);
    want = std::max(1u, std::min(want, 256u));
    for (uint32_t i = 1; i < want; i++)
      workers_.emplace_back([this] {
        pthread_setname_np(pthread_self(), "bpp-chain");  // (who is busy: bench.py's host_cores_busy_by_thread)
        loop();
      });
    for (auto &t : workers_) t.detach();
  }
 public:
  // CPU time spent inside jobs (thread clocks, so a thread that was not scheduled is not counted): what bpp_host_pool_cpu_ns
  // reports -- with several ranks on one host it tells a host-bound step from a GPU-bound one
  static uint64_t thread_cpu_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
  }
  static std::atomic<uint64_t> &cpu_ns() {
    static std::atomic<uint64_t> v{0};
    return v;
  }
  // (the thread clock is a system call, ~1 us: read once per thread and JOB, never per item -- a 256-proof call parses 256 items)
  struct CpuSpan {
    uint64_t t0 = thread_cpu_ns();
    ~CpuSpan() { cpu_ns().fetch_add(thread_cpu_ns() - t0, std::memory_order_relaxed); }
  };

 private:
  static void work_on(Job &j) {
    if (j.next.load() >= j.n) return;  // nothing left: no clock reads either
    CpuSpan span;
    for (;;) {
      uint32_t i = j.next.fetch_add(1);
      if (i >= j.n) return;
      (*j.fn)(i);
      if (j.done.fetch_add(1) + 1 == j.n) {
        std::lock_guard<std::mutex> lk(j.mu);
        j.cv.notify_all();
      }
    }
  }
  void loop() {
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] {
          for (auto &j : jobs_)
            if (j->next.load() < j->n) return true;
          return false;
        });
        for (auto &j : jobs_)
          if (j->next.load() < j->n) {
            job = j;
            break;
          }
      }
      if (job) work_on(*job);
    }
  }
  std::vector<std::thread> workers_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<Job>> jobs_;
};

inline void host_parallel_for(uint32_t n, const std::function<void(uint32_t)> &fn) { HostPool::get().parallel_for(n, fn); }
inline uint32_t host_pool_size() { return HostPool::get().size(); }
inline uint64_t host_pool_cpu_ns() { return HostPool::cpu_ns().load(std::memory_order_relaxed); }

// ------------------------------------------------------------------ how long a waiting caller naps
// What a waiting site remembers: how long its wait took the last times (microseconds, a running mean) and for WHICH work -- a key the
// caller makes from the call's size.  A remembered time is only used for a call with the same key: a context that proved 8192
// proofs per call and then proves 1024 must not sleep through the shorter call on the longer one's memory (it did, for one
// build: 45 k proofs/s instead of 150 k in bench.py's prover leg, whose context had made the run's inputs before).
struct WaitHint {
  uint32_t us = 0;
  uint64_t key = 0;
};
// other work than last time: nothing is known about this wait
inline void wait_hint_begin(WaitHint *wh, uint64_t key) {
  if (wh && wh->key != key) {
    wh->us = 0;
    wh->key = key;
  }
}
// a wait that is over, into the running mean (the first one as it is)
inline void wait_hint_fold(WaitHint *wh, long waited_us) {
  if (wh) wh->us = wh->us ? (uint32_t)((3ul * wh->us + (unsigned long)waited_us) / 4ul) : (uint32_t)waited_us;
}

// One wait's naps between the looks at its event.  hint_us: what the caller remembers of this wait (0: nothing).  A call of a
// steady stream of calls waits about as long as the one before it: most of that is slept in ONE piece, and the looking starts
// when the wait is nearly over -- every look is a call into the runtime and every nap two context switches, which on a busy host
// (measured: the same build 0.3 or 1.2 cores for four waiting callers, box by box) is what a rank's idle callers cost.
// tail_spin: after the piece slept ahead, look without napping (a call at a time then ends as promptly as under the runtime's
// spinning wait, for ~30 % of a core instead of all of it; with nothing remembered yet the whole wait is looked through)
struct WaitSchedule {
  uint32_t hint_us;
  bool tail_spin;
  bool slept_ahead = false;
  // the nap after a look that found the event not ready, `waited_us` into the wait; 0: look again at once
  long next_nap_us(long waited_us) {
    // the first ~30 us by looking only: a wait for something that is (nearly) done must not cost a nap -- a nap is 60-100 us with
    // the kernel's timer slack, and a prover call has six waits in a row at its end (0.6 ms of a 6.5 ms call before this)
    if (waited_us < 30) return 0;
    if (tail_spin && (slept_ahead || hint_us <= 600)) return 0;
    if (!slept_ahead && hint_us > 600 && waited_us < (long)hint_us / 2) {
      // the bulk of an expected wait in one piece: HALF of what the last waits took when naps follow, 70 % when the rest is looked
      // through.  (70 % for the napping callers too overslept in short runs: between two synchronisations the steps in flight
      // start together and stay in step, their waits spread from 6 to 13 ms around the remembered 10, a caller that sleeps past
      // its step's end restarts its slot late and the steps in step with it all shift -- the driver's 20-step form of bench.py
      // read 25.1 M proofs/s with 70 %, 25.6 with 60 %, 25.8-26.2 with 50 %, 26.0 with 40 %, 25.9-26.0 under the runtime's
      // spinning wait; 256-step runs and the callers' CPU time do not change: profiles/r06_wait_ahead_ab.txt)
      slept_ahead = true;
      return std::max(50l, (long)hint_us * (tail_spin ? 7 : 5) / 10 - waited_us);
    }
    if (slept_ahead && waited_us < (long)hint_us * 5 / 4) return 50;  // the expected end is near: short naps (a call at a time wakes up within one of them)
    // naps grow with the wait: 50 us at first (a wait of a few hundred microseconds ends within a nap of its event), an eighth of
    // the time waited so far from 0.4 ms on, 400 us at most
    return waited_us < 400 ? 50 : std::min(400l, waited_us / 8);
  }
};

inline struct timespec nap_timespec(long us) {
  struct timespec ts;
  ts.tv_sec = us / 1000000;
  ts.tv_nsec = (us % 1000000) * 1000;  // (below 1e9: nanosleep refuses anything else at once, and the nap would be skipped)
  return ts;
}
inline void nap_us(long us) {
  const struct timespec ts = nap_timespec(us);
  nanosleep(&ts, nullptr);
}

}  // namespace bpp
