// Stand-alone driver of csrc/hvc_feed.h for tests/test_batch_feed.py: a real hvc::WorkerPool, the feed, and a fake
// orchestrator in place of the GPU.  Built by Makefile.feed twice (CPU only, no device code): under ThreadSanitizer, and
// under AddressSanitizer + UndefinedBehaviorSanitizer.
//   feed_harness SCENARIO [REPS]     REPS (default 200) runs of the scenario in one process, each followed by a plain batch
//                                    on the same pool; prints "ok SCENARIO REPS <ms> ms", or says what broke and aborts
// The ring is an array of plain ints (so that a write the protocol does not order is a data race the sanitizer sees): a worker
// aborts when it is let into slot k % RING before chunk k - RING was released, the orchestrator when a chunk it was told is
// complete lacks an item.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "hvc_feed.h"

namespace {

constexpr int RING = 3;

[[noreturn]] void broke(const char *what, int a = 0, int b = 0) {
    std::fprintf(stderr, "feed_harness: %s (%d, %d)\n", what, a, b);
    std::abort();
}

struct Batch {
    std::vector<int> counts;      // items per chunk
    int workers = 2, take = 1;    // pool threads; items claimed at a time
    int slow_until = 0;           // the orchestrator sleeps before releasing chunks below this one
    int fail_item = -1, fail_code = 0; // a worker reports fail_code for this item
    int throw_item = -1;          // a worker's body throws std::bad_alloc at this item
    int orch_fail_after = -1, orch_rc = 0; // the orchestrator gives up with orch_rc once this chunk is complete, releasing nothing
    bool leave_early = false;     // ... or leaves without finish() at that point
};

struct Outcome {
    int rc = 0;          // what finish() returned (leave_early: the error the workers saw)
    int wait_rc = 0;     // what the orchestrator's last wait returned
    int chunks_seen = 0; // chunks the orchestrator found complete
};

Outcome run(hvc::WorkerPool &pool, const Batch &b) {
    const int n_chunks = (int)b.counts.size();
    std::vector<int> chunk_of, pos_of, first_of;
    int most = 0;
    for (int k = 0; k < n_chunks; k++) {
        first_of.push_back((int)chunk_of.size());
        for (int p = 0; p < b.counts[(size_t)k]; p++) chunk_of.push_back(k), pos_of.push_back(p);
        most = b.counts[(size_t)k] > most ? b.counts[(size_t)k] : most;
    }
    const int n_items = (int)chunk_of.size();
    // everything a pool task touches: declared before the feed
    std::vector<int> ring((size_t)RING * (size_t)most, 0); // item + 1
    std::atomic<int> released{-1};                          // the last chunk the orchestrator released
    std::atomic<int> running{0}, seen_error{0}, ran{0};
    Outcome out;
    if (pool.ensure(b.workers)) broke("the pool refused its threads", b.workers);
    {
        hvc::ChunkFeed feed(pool, n_chunks, RING);
        auto body = [&] {
            running++;
            ran++;
            struct Leave {
                std::atomic<int> &n;
                ~Leave() { n--; }
            } leave{running};
            for (;;) {
                const int f0 = feed.claim(b.take);
                if (feed.error()) seen_error.store(feed.error());
                if (f0 >= n_items || feed.error()) return;
                const int cnt = f0 + b.take <= n_items ? b.take : n_items - f0;
                if (!feed.wait_slot(chunk_of[(size_t)(f0 + cnt - 1)])) {
                    seen_error.store(feed.error());
                    return;
                }
                for (int f = f0; f < f0 + cnt; f++) {
                    const int k = chunk_of[(size_t)f];
                    if (k - RING > released.load()) broke("a worker was let into a slot whose chunk was not released", k, released.load());
                    if (f == b.throw_item) throw std::bad_alloc();
                    int &cell = ring[(size_t)(k % RING) * (size_t)most + (size_t)pos_of[(size_t)f]];
                    if (cell != 0) broke("a worker found its slot still occupied", f, cell - 1);
                    cell = f + 1;
                    feed.report(k, 1, f == b.fail_item ? b.fail_code : HVC_OK);
                }
            }
        };
        if (feed.start(b.workers, body)) broke("submit was refused");
        int rc = HVC_OK;
        bool left = false;
        for (int k = 0; k < n_chunks && rc == HVC_OK; k++) {
            if ((out.wait_rc = rc = feed.wait_chunk(k, b.counts[(size_t)k]))) break;
            for (int p = 0; p < b.counts[(size_t)k]; p++) { // (the chunk is "uploaded": its slot is emptied)
                int &cell = ring[(size_t)(k % RING) * (size_t)most + (size_t)p];
                if (cell != first_of[(size_t)k] + p + 1) broke("a complete chunk lacks an item", k, p);
                cell = 0;
            }
            out.chunks_seen++;
            if (k == b.orch_fail_after) {
                std::this_thread::sleep_for(std::chrono::microseconds(200)); // (the workers run into the unreleased slots)
                left = b.leave_early;
                rc = b.orch_rc;
                break;
            }
            if (k < b.slow_until) std::this_thread::sleep_for(std::chrono::microseconds(100));
            released.store(k);
            feed.release(k);
        }
        if (!left) { // (else the feed goes out of scope without finish())
            out.rc = feed.finish(rc);
            if (running.load()) broke("finish() returned with a worker still running", running.load());
        }
    }
    if (running.load()) broke("the feed's scope ended with a worker still running", running.load());
    if (ran.load() != b.workers) broke("not every pool thread ran the body once", ran.load(), b.workers);
    if (b.leave_early) out.rc = seen_error.load();
    return out;
}

Batch chunks_of(int n_items, int per_chunk) {
    Batch b;
    for (int f = 0; f < n_items; f += per_chunk) b.counts.push_back(n_items - f < per_chunk ? n_items - f : per_chunk);
    return b;
}

void expect(const Outcome &o, int rc, int chunks, const char *what) {
    if (o.rc != rc) broke(what, o.rc, rc);
    if (chunks >= 0 && o.chunks_seen != chunks) broke(what, o.chunks_seen, chunks);
}

void plain_batch_after(hvc::WorkerPool &pool, int workers) { // the pool serves a second feed after whatever came before
    Batch b = chunks_of(10, 3);
    b.workers = workers;
    expect(run(pool, b), HVC_OK, 4, "a plain batch on the reused pool");
}

void scenario(const std::string &s, hvc::WorkerPool &pool) {
    if (s == "plain") { // 10 items in chunks of 3: four chunks, the last one ragged, more chunks than RING
        for (int w : {1, 2, 8, 16}) { // (16: more workers than items)
            Batch b = chunks_of(10, 3);
            b.workers = w;
            expect(run(pool, b), HVC_OK, 4, "plain");
        }
    } else if (s == "pairs") { // two items at a time, pairs that straddle a chunk boundary
        for (int w : {1, 2, 8}) {
            Batch b = chunks_of(10, 3);
            b.workers = w, b.take = 2;
            expect(run(pool, b), HVC_OK, 4, "pairs");
            Batch o = chunks_of(9, 1); // (every pair in two chunks, the last item alone)
            o.workers = w, o.take = 2;
            expect(run(pool, o), HVC_OK, 9, "pairs over chunks of one");
        }
    } else if (s == "unequal") {
        for (int w : {1, 2, 8}) {
            Batch b;
            b.counts = {1, 4, 1, 2, 5};
            b.workers = w;
            expect(run(pool, b), HVC_OK, 5, "unequal");
            b.take = 2;
            expect(run(pool, b), HVC_OK, 5, "unequal, in pairs");
        }
    } else if (s == "slow_fast") { // the orchestrator slow to release, then fast
        for (int w : {1, 2, 8}) {
            Batch b = chunks_of(24, 2);
            b.workers = w, b.slow_until = 6;
            expect(run(pool, b), HVC_OK, 12, "slow_fast");
        }
    } else if (s == "worker_error") { // an item of chunk 0, of chunk RING, of the last chunk
        for (int w : {1, 2, 8})
            for (int item : {1, 2 * RING, 9}) { // (five chunks of two)
                Batch b = chunks_of(10, 2);
                b.workers = w, b.fail_item = item, b.fail_code = HVC_E_BAD_JPEG;
                const Outcome o = run(pool, b);
                expect(o, HVC_E_BAD_JPEG, -1, "worker_error");
                if (o.wait_rc != HVC_E_BAD_JPEG) broke("the orchestrator's wait did not return the worker's code", o.wait_rc);
                if (o.chunks_seen > item / 2) broke("a chunk with a failed item was found complete", o.chunks_seen, item);
            }
        // the first error stays when another one follows
        hvc::ChunkFeed feed(pool, 2, RING);
        feed.report(0, 1, HVC_E_BAD_JPEG);
        feed.report(0, 1, HVC_E_RANGE);
        if (feed.wait_chunk(0, 2) != HVC_E_BAD_JPEG || feed.finish(HVC_OK) != HVC_E_BAD_JPEG) broke("a later error replaced the first one");
    } else if (s == "orchestrator_fails") { // while workers wait for a slot; rc wins
        for (int w : {1, 2, 8}) {
            Batch b = chunks_of(10, 1);
            b.workers = w, b.orch_fail_after = RING - 1, b.orch_rc = HVC_E_HIP;
            expect(run(pool, b), HVC_E_HIP, RING, "orchestrator_fails");
        }
        hvc::ChunkFeed feed(pool, 2, RING); // a worker's error beside it: rc still wins
        feed.report(0, 1, HVC_E_BAD_JPEG);
        if (feed.finish(HVC_E_HIP) != HVC_E_HIP) broke("a worker's error replaced the orchestrator's");
    } else if (s == "throws") {
        for (int w : {1, 2, 8})
            for (int item : {0, 4, 9}) {
                Batch b = chunks_of(10, 3);
                b.workers = w, b.throw_item = item;
                expect(run(pool, b), HVC_E_OUT_OF_MEMORY, -1, "throws");
            }
    } else if (s == "leaves_early") { // no finish(): the scope raises HVC_E_INTERNAL, the workers end
        for (int w : {1, 2, 8}) {
            Batch b = chunks_of(10, 1);
            b.workers = w, b.orch_fail_after = RING - 1, b.leave_early = true;
            expect(run(pool, b), HVC_E_INTERNAL, RING, "leaves_early");
        }
    } else if (s == "refused") { // HVC_POOL_FAIL_AFTER=2 in the environment: the third thread of the process is refused
        if (pool.ensure(2) != HVC_OK) broke("the first two threads were refused");
        const int r = pool.ensure(8);
        if (r != HVC_E_SYSTEM) broke("ensure(8) was not refused with HVC_E_SYSTEM", r);
        if (pool.size() != 2) broke("the threads that exist did not stay", pool.size());
        // (a pipeline returns here: no feed, no task)
    } else {
        broke("unknown scenario");
    }
}

} // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string s = argv[1];
    const int reps = argc > 2 ? std::atoi(argv[2]) : 200;
    const auto t0 = std::chrono::steady_clock::now();
    hvc::WorkerPool pool;
    for (int i = 0; i < reps; i++) {
        scenario(s, pool);
        plain_batch_after(pool, s == "refused" ? 2 : 4);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("ok %s %d %.0f ms\n", s.c_str(), reps, ms);
    return 0;
}
