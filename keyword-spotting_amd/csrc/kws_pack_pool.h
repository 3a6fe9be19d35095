// The pack stage of the host ingest (kws_ingest.hip): a pool of host threads that copies one chunk of the caller's pageable
// memory into pinned staging.  Plain C++ with no HIP header, so that the one piece of hand-written thread code in the library
// also builds as host code under the thread and address sanitizers (tests/native/pack_pool_check.cpp).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <system_error>
#include <thread>
#include <vector>

namespace kws {

// A fixed set of host threads that copy one chunk in parallel (a single memcpy moves ~10-20 GB/s; the PCIe DMA behind it
// takes ~50): job = (dst, src, bytes), cut into equal 4 KiB-aligned slices.
class PackPool {
  public:
    explicit PackPool(int n) {
        // a host that refuses more threads (cgroup pids limit, RLIMIT_NPROC) still gets a pool: of the threads that did start,
        // or of none -- copy() then runs on the calling thread.  Nothing is thrown across the C ABI.
        try {
            for (int i = 0; i < n; ++i) workers_.emplace_back([this, i] { run(i); });
        } catch (const std::system_error&) {
        }
        n_started_ = workers_.size();
    }
    ~PackPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    int size() const { return (int)workers_.size(); }
    // blocks until the whole copy is done (the caller enqueues the DMA right after)
    void copy(void* dst, const void* src, size_t bytes) {
        if (workers_.empty() || bytes < (1u << 20)) {
            memcpy(dst, src, bytes);
            return;
        }
        std::unique_lock<std::mutex> g(m_);
        dst_ = static_cast<unsigned char*>(dst);
        src_ = static_cast<const unsigned char*>(src);
        bytes_ = bytes;
        pending_ = (int)n_started_;
        ++gen_;
        cv_.notify_all();
        done_.wait(g, [this] { return pending_ == 0; });
    }

  private:
    void run(int idx) {
        unsigned long seen = 0;
        for (;;) {
            unsigned char* dst;
            const unsigned char* src;
            size_t bytes;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                dst = dst_, src = src_, bytes = bytes_;
            }
            const size_t n = n_started_;
            const size_t slice = ((bytes + n - 1) / n + 4095) & ~(size_t)4095;
            const size_t lo = std::min(bytes, slice * idx), hi = std::min(bytes, lo + slice);
            if (hi > lo) memcpy(dst + lo, src + lo, hi - lo);
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> workers_;
    size_t n_started_ = 0;  // fixed before any job is posted (workers_.size() must not be read while the vector may still grow)
    std::mutex m_;
    std::condition_variable cv_, done_;
    unsigned char* dst_ = nullptr;
    const unsigned char* src_ = nullptr;
    size_t bytes_ = 0;
    int pending_ = 0;
    unsigned long gen_ = 0;
    bool stop_ = false;
};

}  // namespace kws
