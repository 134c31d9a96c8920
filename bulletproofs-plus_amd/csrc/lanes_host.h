// The two concurrency protocols of the engine's host side, once: mutexes, a condition variable, a queue and a ticket map.  Nothing
// here knows the GPU or an engine type, so hosttest_lanes.cpp drives both on a CPU under ThreadSanitizer and ASan + UBSan.
//
//   TicketLanes<Lane, Job>  submit / collect: `depth` lanes, each with a worker thread; a submit claims the lane whose turn it is,
//                           posts a job and gets a ticket; a collect waits for the ticket's job and takes it.
//                           (bpp_verify_submit_packed / bpp_verify_collect, bpp_prove_submit / bpp_prove_collect)
//   LeaderPool<Lane, Req>   blocking callers, no thread of its own: whichever caller finds a lane free leads the next pooled call
//                           over what has queued up; the others wait for their outcome.  (bpp_batcher, bpp_prove_pool)
//
// A client supplies what a lane carries (for the engine: a context and its reusable buffers), what a job or request is, and the
// call that runs on a lane.  Lock order for clients: neither protocol calls the client with its own mutex held, except the
// predicates of LeaderPool::serve (poolable, weight, compatible), which must take no lock.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace lanes {

enum class TicketState { unknown, running, done };

// Job needs two fields: `uint64_t ticket` (set by post) and `bool done` (set by the worker, read under the lock).
template <class Lane, class Job>
class TicketLanes {
  struct Slot {
    Lane lane;
    std::thread th;
    std::shared_ptr<Job> job;  // posted by post(), taken by the worker
    bool busy = false;         // from claim() until the job is done (not: collected), or until the claim is dropped
  };

 public:
  using Run = std::function<void(Lane &, Job &)>;
  // what an exception out of `run` leaves in the job (its code and message fields); `what` is null for one that is no std::exception
  using OnThrow = std::function<void(Job &, const char *what)>;

  // a lane claimed by one submit; holds the submit lock, so lanes are claimed and tickets given in the same order
  class Claim {
   public:
    Claim(Claim &&o) noexcept : tl_(o.tl_), slot_(o.slot_), submit_(std::move(o.submit_)) { o.slot_ = nullptr; }
    Claim &operator=(Claim &&) = delete;
    ~Claim() {  // dropped without post: the lane is free again, no ticket number is used up
      if (!slot_) return;
      {
        std::lock_guard<std::mutex> lk(tl_->mu_);
        slot_->busy = false;
      }
      tl_->cv_.notify_all();
    }
    Lane &lane() { return slot_->lane; }

   private:
    friend class TicketLanes;
    Claim(TicketLanes *tl, Slot *slot, std::unique_lock<std::mutex> submit) : tl_(tl), slot_(slot), submit_(std::move(submit)) {}
    TicketLanes *tl_;
    Slot *slot_;
    std::unique_lock<std::mutex> submit_;
  };

  TicketLanes(std::vector<Lane> lanes, uint64_t first_ticket, Run run, OnThrow on_throw)
      : run_(std::move(run)), on_throw_(std::move(on_throw)), next_ticket_(first_ticket) {
    for (auto &l : lanes) slots_.emplace_back(new Slot{std::move(l)});
    try {
      for (auto &s : slots_) s->th = std::thread([this, p = s.get()] { work(p); });
    } catch (...) {  // a thread that could not be started: the ones that were are ended, not abandoned while joinable
      shutdown([](Job &) {});
      throw;
    }
  }
  ~TicketLanes() { shutdown([](Job &) {}); }

  // blocks while the lane whose turn it is (round-robin) is busy with an earlier ticket
  Claim claim() {
    std::unique_lock<std::mutex> submit(submit_mu_);
    std::unique_lock<std::mutex> lk(mu_);
    Slot *s = slots_[next_lane_].get();
    cv_.wait(lk, [&] { return !s->busy; });
    s->busy = true;
    next_lane_ = (next_lane_ + 1) % (uint32_t)slots_.size();
    return Claim(this, s, std::move(submit));
  }

  // the claimed lane's worker runs the job; the ticket collects it
  uint64_t post(Claim &c, std::shared_ptr<Job> job) {
    uint64_t t;
    {
      std::lock_guard<std::mutex> lk(mu_);
      t = job->ticket = next_ticket_++;
      tickets_[t] = job;
      c.slot_->job = std::move(job);
      c.slot_ = nullptr;
    }
    cv_.notify_all();
    return t;
  }

  // the ticket's job, running or done, or null; the ticket stays
  std::shared_ptr<Job> peek(uint64_t ticket) {
    std::lock_guard<std::mutex> lk(mu_);
    return find(ticket);
  }

  // waits for the ticket's job and hands it to exactly one caller; null for a ticket that is unknown or that another caller took
  std::shared_ptr<Job> take(uint64_t ticket) {
    std::unique_lock<std::mutex> lk(mu_);
    const std::shared_ptr<Job> job = find(ticket);  // (no iterator is kept across the wait: the lock is released in it)
    if (job) cv_.wait(lk, [&] { return job->done; });
    return job && tickets_.erase(ticket) ? job : nullptr;
  }

  TicketState done(uint64_t ticket) {
    std::lock_guard<std::mutex> lk(mu_);
    const std::shared_ptr<Job> job = find(ticket);
    return !job ? TicketState::unknown : job->done ? TicketState::done : TicketState::running;
  }

  // the lanes are fixed from construction on: no lock is held, `fn` may take any
  template <class F>
  void for_each_lane(F fn) {
    for (auto &s : slots_) fn(s->lane);
  }

  // waits for the jobs in flight, ends the workers, then hands every job nobody collected to `on_uncollected` once.  The lanes
  // themselves stay (for_each_lane) until the object dies.
  template <class F>
  void shutdown(F on_uncollected) {
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] {
        for (auto &s : slots_)
          if (s->busy) return false;
        return true;
      });
      quit_ = true;
    }
    cv_.notify_all();
    for (auto &s : slots_)
      if (s->th.joinable()) s->th.join();
    std::map<uint64_t, std::shared_ptr<Job>> left;
    {
      std::lock_guard<std::mutex> lk(mu_);
      left.swap(tickets_);
    }
    for (auto &kv : left) on_uncollected(*kv.second);
  }

 private:
  std::shared_ptr<Job> find(uint64_t ticket) {  // under mu_
    auto it = tickets_.find(ticket);
    return it == tickets_.end() ? nullptr : it->second;
  }

  void work(Slot *s) {
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return quit_ || s->job; });
        if (!s->job) return;  // quit with nothing posted
        job = std::move(s->job);
        s->job.reset();
      }
      try {  // nothing may escape a worker
        try {
          run_(s->lane, *job);
        } catch (const std::exception &e) {
          on_throw_(*job, e.what());
        } catch (...) {
          on_throw_(*job, nullptr);
        }
      } catch (...) {  // (the hook's own allocation)
      }
      {
        std::lock_guard<std::mutex> lk(mu_);
        job->done = true;
        s->busy = false;  // the lane is free now: the results wait in the job
      }
      cv_.notify_all();
    }
  }

  Run run_;
  OnThrow on_throw_;
  std::mutex mu_;  // lanes' state, tickets
  std::condition_variable cv_;
  std::mutex submit_mu_;  // one submit at a time
  std::vector<std::unique_ptr<Slot>> slots_;
  std::map<uint64_t, std::shared_ptr<Job>> tickets_;
  uint64_t next_ticket_;
  uint32_t next_lane_ = 0;
  bool quit_ = false;
};

// what LeaderPool keeps in a request; Req derives from it
struct PoolReq {
  bool taken = false;  // a leader has it in its pooled call
  bool done = false;
};

struct PoolStats {
  uint64_t pooled_calls = 0, engine_calls = 0, solo_calls = 0;  // requests served in a pool of two or more; runs; runs of one request
  uint32_t largest_pool_calls = 0, largest_pool_weight = 0;
};

// Clock: what a leader's wait for company goes by (the harness's ThreadSanitizer build names another: see hosttest_lanes.cpp)
template <class Lane, class Req, class Clock = std::chrono::steady_clock>
class LeaderPool {
  struct Slot {
    Lane lane;
    bool busy = false;
  };

 public:
  LeaderPool(std::vector<Lane> lanes, uint32_t max_wait_us, uint32_t max_calls, uint32_t max_weight)
      : max_wait_us_(max_wait_us), max_calls_(max_calls), max_weight_(max_weight) {
    for (auto &l : lanes) slots_.push_back(Slot{std::move(l)});
  }

  void set_limits(uint32_t max_calls, uint32_t max_weight) {  // 0: as it is
    std::lock_guard<std::mutex> lk(mu_);
    if (max_calls) max_calls_ = max_calls;
    if (max_weight) max_weight_ = max_weight;
  }

  PoolStats stats() {
    std::lock_guard<std::mutex> lk(mu_);
    return stats_;
  }

  template <class F>
  void for_each_lane(F fn) {  // (fixed from construction on: no lock is held)
    for (auto &s : slots_) fn(s.lane);
  }

  // One request, from its caller's thread; returns when somebody -- this thread or another request's -- has run it.
  //   poolable(max_weight) -> bool   may it share a run?  If not it runs alone, on the next free lane
  //   weight(req) -> size_t          what it adds to a pool's weight
  //   compatible(me, other) -> bool  may `other` share the run `me` leads?
  //   run(lane, reqs)                the pooled call, outside the lock; reqs[0] is `me`.  It leaves every request's outcome in the
  //                                  request.  Whatever it throws, the others are released and the lane is freed before it goes on
  //                                  to serve's caller
  template <class Poolable, class Weight, class Compatible, class Run>
  void serve(Req &me, Poolable poolable, Weight weight, Compatible compatible, Run run) {
    std::vector<Req *> mine{&me};
    Slot *slot = nullptr;
    {
      std::unique_lock<std::mutex> lk(mu_);
      const bool pool = poolable(max_weight_);
      if (pool) {
        pending_.push_back(&me);
        if (max_wait_us_) cv_.notify_all();  // (a leader waiting for company counts the queue)
      }
      auto free_slot = [&]() -> Slot * {
        for (auto &s : slots_)
          if (!s.busy) return &s;
        return nullptr;
      };
      // wait until somebody else has dealt with this request, or -- as long as nobody has taken it -- a lane is free and this
      // thread leads the next pooled call
      cv_.wait(lk, [&] { return me.done || (!me.taken && free_slot() != nullptr); });
      if (me.done) return;
      slot = free_slot();
      slot->busy = true;
      if (pool) {
        if (max_wait_us_ && pending_.size() < max_calls_)
          cv_.wait_until(lk, Clock::now() + std::chrono::microseconds(max_wait_us_),
                         [&] { return me.taken || pending_.size() >= max_calls_; });
        if (me.taken) {  // another leader took this thread's request while it waited for company: let that one finish it
          slot->busy = false;
          cv_.notify_all();
          cv_.wait(lk, [&] { return me.done; });
          return;
        }
        // The leader's own request goes first (it fits by itself: poolable), then whatever is queued, oldest first, as long as the
        // pool stays within max_calls requests and max_weight and is compatible with the leader's.  Requests that do not fit stay
        // where they are, for the next leader.
        pending_.erase(std::find(pending_.begin(), pending_.end(), &me));  // (untaken and poolable: it is there)
        me.taken = true;
        size_t w = weight(me);
        for (auto it = pending_.begin(); it != pending_.end() && mine.size() < max_calls_;) {
          Req *r = *it;
          if (!compatible(me, *r) || w + weight(*r) > max_weight_) {
            ++it;
            continue;
          }
          w += weight(*r);
          r->taken = true;
          mine.push_back(r);
          it = pending_.erase(it);
        }
        if (mine.size() > 1) {
          stats_.pooled_calls += mine.size();
          if (mine.size() > stats_.largest_pool_calls) stats_.largest_pool_calls = (uint32_t)mine.size();
          if (w > stats_.largest_pool_weight) stats_.largest_pool_weight = (uint32_t)w;
        }
      }
      stats_.engine_calls++;
      if (mine.size() == 1) stats_.solo_calls++;
    }
    auto finish = [&] {  // on every way out of run
      {
        std::lock_guard<std::mutex> lk(mu_);
        for (Req *r : mine)
          if (r != &me) r->done = true;  // (`me` lives on its caller's stack and is always part of `mine`)
        slot->busy = false;
      }
      cv_.notify_all();
    };
    struct Guard {
      decltype(finish) &f;
      ~Guard() { f(); }
    } guard{finish};
    run(slot->lane, static_cast<const std::vector<Req *> &>(mine));
  }

  // returns when nothing is queued and every lane is idle (what a destroy waits on)
  void drain() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] {
      for (auto &s : slots_)
        if (s.busy) return false;
      return pending_.empty();
    });
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<Req *> pending_;
  std::deque<Slot> slots_;
  uint32_t max_wait_us_, max_calls_, max_weight_;
  PoolStats stats_;
};

}  // namespace lanes
