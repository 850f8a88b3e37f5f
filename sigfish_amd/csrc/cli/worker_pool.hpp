// worker_pool.hpp -- the -t host threads of the command line, created once and woken per stage.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace cli {

// work_db() of the reference forks and joins `-t` threads for every stage of every batch (src/thread.c:119-132); here
// the workers are created once and woken per stage.  Items are handed out through an atomic counter,
// the calling thread works too.  Several threads may call run() (the loader and the output stage do): calls queue up.
class WorkerPool {
  public:
    explicit WorkerPool(int nthreads) {
        for (int t = 1; t < nthreads; ++t) workers_.emplace_back([this] { loop(); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &w : workers_) w.join();
    }
    template <typename F>
    void run(int64_t n, F fn) {
        if (workers_.empty() || n <= 1) {
            for (int64_t i = 0; i < n; ++i) fn(i);
            return;
        }
        std::lock_guard<std::mutex> one_job(submit_mu_);
        std::function<void(int64_t)> f = fn;
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &f;
            n_ = n;
            next_.store(0);
            busy_ = static_cast<int>(workers_.size());
            ++generation_;
        }
        cv_.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return busy_ == 0; });
        fn_ = nullptr;
    }

  private:
    void drain() {
        for (;;) {
            const int64_t i = next_.fetch_add(1);
            if (i >= n_) break;
            (*fn_)(i);
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
            }
            drain();
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--busy_ == 0) done_cv_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_, submit_mu_;
    std::condition_variable cv_, done_cv_;
    std::atomic<int64_t> next_{0};
    const std::function<void(int64_t)> *fn_ = nullptr;
    int64_t n_ = 0;
    int busy_ = 0;
    uint64_t generation_ = 0;
    bool stop_ = false;
};

}  // namespace cli
