// frame_loader.hpp -- a helper thread that frames the records of the next batches of a mapped file.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

#include "../host/blow5.hpp"

namespace cli {

// load_db() of the reference reads the records of a batch on the main thread, between two batches' worth of work (src/sigfish.c:
// 262-315).  Framing a mapped file is cheap -- a size prefix per record -- but it is a cache miss per record, 0.25 us x 1.6 M records
// = 0.4 s of a 2.3 s run during which the -t workers have nothing to do.  Here a helper frames batch i + 1 (and i + 2) while the main
// thread and the workers are in the host stages of batch i: the main thread only collects finished lists.
struct Frames {
    std::vector<const uint8_t *> view;
    std::vector<size_t> size;
    int32_t n = 0;
    int64_t bytes = 0;
    bool more = true;  // false: the file (or this process's part of it) ends with this batch
    bool failed = false;
};
class FrameLoader {
  public:
    FrameLoader(sfa::Blow5Reader &reader, int32_t batch_size, int64_t batch_bytes) : reader_(reader), batch_size_(batch_size), batch_bytes_(batch_bytes) {
        for (Frames &f : ring_) {
            f.view.resize(batch_size);
            f.size.resize(batch_size);
        }
        th_ = std::thread([this] { loop(); });
    }
    ~FrameLoader() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    // the next batch's list; valid until the call after the next one (three buffers: one with the caller, two ahead)
    const Frames &next() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return produced_ > consumed_; });
        const Frames &f = ring_[consumed_ % kDepth];
        ++consumed_;
        lk.unlock();
        cv_.notify_all();
        return f;
    }

  private:
    static constexpr uint64_t kDepth = 3;
    void loop() {
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                // the caller still reads the list it took last: keep one buffer behind `consumed_` untouched
                cv_.wait(lk, [this] { return quit_ || produced_ + 1 < consumed_ + kDepth; });
                if (quit_) return;
            }
            Frames &f = ring_[produced_ % kDepth];
            f.n = 0;
            f.bytes = 0;
            f.more = true;
            f.failed = false;
            while (f.n < batch_size_ && f.bytes < batch_bytes_) {
                const int rc = reader_.next_view(&f.view[f.n], &f.size[f.n]);
                if (rc < 0) f.failed = true;
                if (rc <= 0) {
                    f.more = false;
                    break;
                }
                f.bytes += static_cast<int64_t>(f.size[f.n]);
                ++f.n;
            }
            const bool last = !f.more;
            {
                std::lock_guard<std::mutex> lk(mu_);
                ++produced_;
            }
            cv_.notify_all();
            if (last) return;
        }
    }
    sfa::Blow5Reader &reader_;
    const int32_t batch_size_;
    const int64_t batch_bytes_;
    Frames ring_[kDepth];
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t produced_ = 0, consumed_ = 0;
    bool quit_ = false;
    std::thread th_;
};

}  // namespace cli
