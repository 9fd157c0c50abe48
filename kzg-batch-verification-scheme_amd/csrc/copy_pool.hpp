// Parallel memcpy for pageable -> pinned staging (api.hip h2d): one memcpy thread reaches
// ~10-20 GB/s, below PCIe Gen5's ~50 GB/s, so a copy of kCopyPoolMinBytes or more is split over
// `nthreads` - 1 workers plus the caller.  One job at a time (contexts on several host threads
// take turns).  Plain C++17, no HIP: tests/native/copy_pool_test.cpp runs it on its own.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace kzgmi {

// shorter copies are one memcpy on the calling thread
constexpr size_t kCopyPoolMinBytes = size_t(2) << 20;

class CopyPool {
 public:
  explicit CopyPool(int nthreads) : nthreads_(std::max(1, nthreads)) {}
  CopyPool(const CopyPool&) = delete;
  CopyPool& operator=(const CopyPool&) = delete;

  void copy(void* dst, const void* src, size_t len) {
    if (len < kCopyPoolMinBytes || nthreads_ <= 1) {
      memcpy(dst, src, len);
      return;
    }
    std::lock_guard<std::mutex> job(job_mu_);
    start();
    const int parts = (int)workers_.size() + 1;
    {
      std::lock_guard<std::mutex> lk(mu_);
      dst_ = (uint8_t*)dst;
      src_ = (const uint8_t*)src;
      len_ = len;
      parts_ = parts;
      left_ = parts - 1;
      ++gen_;
    }
    cv_.notify_all();
    part(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return left_ == 0; });
  }

  // [lo, hi) of part i when len bytes are cut into `parts`: 64-byte boundaries, and the parts
  // cover [0, len) for every len and part count (per is the rounded-up quotient, rounded up to 64)
  static void part_range(size_t len, int parts, int i, size_t& lo, size_t& hi) {
    const size_t per = ((len + parts - 1) / parts + 63) & ~size_t(63);
    lo = std::min(len, per * i);
    hi = std::min(len, per * (i + 1));
  }

 private:
  void start() {
    if (!workers_.empty()) return;
    for (int i = 1; i < nthreads_; ++i) {
      workers_.emplace_back([this, i] { loop(i); });
      workers_.back().detach();  // the pool lives as long as the process (never destroyed)
    }
  }
  void part(int i) {
    size_t lo, hi;
    part_range(len_, parts_, i, lo, hi);
    if (hi > lo) memcpy(dst_ + lo, src_ + lo, hi - lo);
  }
  void loop(int i) {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
      }
      part(i);
      std::lock_guard<std::mutex> lk(mu_);
      if (--left_ == 0) done_.notify_one();
    }
  }
  const int nthreads_;  // fixed by the constructor
  std::mutex job_mu_, mu_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  uint8_t* dst_ = nullptr;
  const uint8_t* src_ = nullptr;
  size_t len_ = 0;
  int parts_ = 1, left_ = 0;
  uint64_t gen_ = 0;
};

}  // namespace kzgmi
