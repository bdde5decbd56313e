// hvc_feed.h -- the hand-off between a batch pipeline's host workers and its orchestrating thread (internal).  Plain C++ over
// hvc_pool.h: no HIP, so the protocol runs on a CPU under ThreadSanitizer (tests/host_harness/feed_harness.cpp).
//
// A batch is `items` (files) cut into chunks; chunk k lives in ring slot k % ring.  Workers claim items in order, wait until
// the slot of an item's chunk is free, fill it and report; the orchestrator waits until a chunk is complete, consumes it and
// hands its slot to chunk k + ring.  The first error anybody raises ends everyone's waits.
//
// The feed waits for its pool tasks when it goes out of scope, however the call is left: whatever a task touches is
// declared BEFORE the feed (destroyed after it has waited).
#ifndef HVC_FEED_H
#define HVC_FEED_H

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <vector>

#include "hvc_pool.h"

namespace hvc {

class ChunkFeed {
  public:
    // on_leave (optional) runs under the lock when the scope ends, before everybody is woken: the place for a pipeline's
    // own stop flags (the GPU reader's downloader)
    ChunkFeed(WorkerPool &pool, int n_chunks, int ring, std::function<void()> on_leave = nullptr)
        : pool_(pool), done_in_chunk_((size_t)n_chunks, 0), ring_(ring), released_upto_(ring - 1), on_leave_(std::move(on_leave)),
          scope_(pool, [this] {
              std::lock_guard<std::mutex> lk(mu_);
              if (!completed_ && !error_.load()) error_.store(HVC_E_INTERNAL); // (the call was left before finish())
              if (on_leave_) on_leave_();
              cv_.notify_all();
          }) {}
    ChunkFeed(const ChunkFeed &) = delete;
    ChunkFeed &operator=(const ChunkFeed &) = delete;

    // ---- worker side
    int claim(int n = 1) { return next_.fetch_add(n); } // the first of the next n items (the caller compares with its item count)
    int error() const { return error_.load(); }
    bool wait_slot(int k) { // chunk k's slot may be written; false: an error ended the wait
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return k <= released_upto_ || error_.load(); });
        return !error_.load();
    }
    void report(int k, int n, int status) { // n items of chunk k are done; the first status that is not HVC_OK stays
        std::lock_guard<std::mutex> lk(mu_);
        if (status && !error_.load()) error_.store(status);
        done_in_chunk_[(size_t)k] += n;
        cv_.notify_all();
    }
    void raise(int e) { // an error that belongs to no item
        std::lock_guard<std::mutex> lk(mu_);
        error_.store(e);
        cv_.notify_all();
    }

    // ---- orchestrator side
    int wait_chunk(int k, int count) { // chunk k has `count` items done: HVC_OK, or the error that was raised
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return done_in_chunk_[(size_t)k] == count || error_.load(); });
        return error_.load();
    }
    void release(int k) { // chunk k has left its slot: chunks up to k + ring may be written
        std::lock_guard<std::mutex> lk(mu_);
        release_locked(k);
        cv_.notify_all();
    }
    // `threads` pool threads (WorkerPool::ensure first) run body(); nothing leaves a pool thread but through the error flag.
    // A refused submit is returned, and raised: the scope waits for the copies that were queued.
    int start(int threads, std::function<void()> body) {
        const int r = pool_.submit([this, body] {
            try {
                body();
            } catch (...) {
                raise(exception_code());
            }
        }, threads);
        if (r) raise(r);
        return r;
    }
    // The orchestrator is through with rc: everybody ends, the tasks are waited for.  Returns rc, else the code of an
    // exception that left a task, else the workers' error.
    int finish(int rc) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (rc != HVC_OK) error_.store(rc);
            else completed_ = true;
            cv_.notify_all();
        }
        const int te = scope_.finish();
        if (rc == HVC_OK && te) rc = te;
        if (rc == HVC_OK && error_.load()) rc = error_.load();
        return rc;
    }

    // A pipeline with state of its own beside the feed's (the GPU reader: verdicts, downloader) guards it with the feed's
    // mutex and waits on the feed's condition variable; release_locked: release() for a caller that holds the mutex and notifies.
    std::mutex &mutex() { return mu_; }
    std::condition_variable &cv() { return cv_; }
    void release_locked(int k) { released_upto_ = k + ring_; }

  private:
    WorkerPool &pool_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::atomic<int> next_{0}, error_{0};
    std::vector<int> done_in_chunk_;
    const int ring_;
    int released_upto_; // chunks 0 .. ring - 1 may be written at once
    bool completed_ = false;
    std::function<void()> on_leave_;
    PoolScope scope_; // (last: the first to go)
};

} // namespace hvc

#endif
