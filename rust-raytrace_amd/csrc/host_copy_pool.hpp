#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace rtamd {

// Host threads that move pinned staging slices into the caller's pageable
// buffer (rt_render): created once per context, so a frame's copy does not pay
// thread start-up per slice.  run() shares any job of parts (the sparse copies'
// row scatter) the same way.  copy() splits one memcpy into kParts parts
// shared by the workers and the calling thread (one thread copies pinned ->
// pageable memory at ~20-28 GB/s, below the DMA's 56 GB/s).  Workers spin
// briefly for the next slice before sleeping, so consecutive slices of a frame
// do not pay a wake-up each.
//
// Each job is published as a snapshot under m_: a worker copies the job's
// fields under the mutex and counts itself in active_ before it takes parts,
// and copy() publishes (and resets the part counters) only once active_ is 0,
// i.e. no worker can still be inside the previous job's part loop.  So a
// worker never mixes two jobs' fields and never claims a part of a job it did
// not snapshot.
class HostCopyPool {
public:
    ~HostCopyPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        for (std::thread& t : th_) t.join();
    }
    void copy(void* to, const void* from, size_t len) {
        const size_t parts = std::max<size_t>(1, std::min<size_t>(kParts, len >> 20));   // >= 1 MiB each
        if (parts == 1) { std::memcpy(to, from, len); return; }
        post(Job{static_cast<uint8_t*>(to), static_cast<const uint8_t*>(from), len, parts, (len + parts - 1) / parts, nullptr});
    }
    // fn(0 .. parts-1), shared by the workers and the calling thread
    void run(size_t parts, const std::function<void(size_t)>& fn) {
        if (parts == 0) return;
        if (parts == 1) { fn(0); return; }
        post(Job{nullptr, nullptr, 0, parts, 0, &fn});
    }
    static constexpr size_t kParts = 8;

private:
    struct Job {
        uint8_t* to = nullptr;
        const uint8_t* from = nullptr;
        size_t len = 0, parts = 0, step = 0;
        const std::function<void(size_t)>* fn = nullptr;   // else a memcpy in parts
    };
    void post(const Job& j) {
        if (th_.empty()) start();
        if (th_.empty()) { next_.store(0, std::memory_order_relaxed); work(j); return; }
        const size_t parts = j.parts;
        {
            std::unique_lock<std::mutex> lk(m_);
            idle_.wait(lk, [&] { return active_ == 0; });    // every worker has left the previous job
            job_ = j;
            next_.store(0, std::memory_order_relaxed);
            done_.store(0, std::memory_order_relaxed);
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        work(j);
        while (done_.load(std::memory_order_acquire) != parts) std::this_thread::yield();
    }

    void start() {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const unsigned n = std::min<unsigned>(kParts - 1, hw > 1 ? hw - 1 : 1u);
        for (unsigned i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
    }
    void work(const Job& j) {           // take parts of job j until none is left
        for (;;) {
            const size_t q = next_.fetch_add(1, std::memory_order_relaxed);
            if (q >= j.parts) return;
            if (j.fn) {
                (*j.fn)(q);
            } else {
                const size_t a = q * j.step, b = std::min(j.len, a + j.step);
                if (a < b) std::memcpy(j.to + a, j.from + a, b - a);
            }
            done_.fetch_add(1, std::memory_order_release);
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            // spin at most ~200 us for the next slice (the DMA of one slice takes ~150 us), then sleep
            const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
            while (gen_.load(std::memory_order_acquire) == seen && std::chrono::steady_clock::now() < until)
                std::this_thread::yield();
            Job j;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_.load(std::memory_order_acquire) != seen; });
                if (stop_) return;
                seen = gen_.load(std::memory_order_acquire);
                j = job_;
                ++active_;
            }
            work(j);
            {
                std::lock_guard<std::mutex> g(m_);
                --active_;
            }
            idle_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, idle_;
    Job job_;                           // the current job (written and read under m_)
    int active_ = 0;                    // workers inside work() (under m_)
    bool stop_ = false;                 // (under m_)
    std::atomic<size_t> next_{0}, done_{0};
    std::atomic<uint64_t> gen_{0};
};

}  // namespace rtamd
