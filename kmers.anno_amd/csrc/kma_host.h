// kma_host.h — host-side plumbing shared by the units of the C ABI (kma_host.cpp, kma_abi_*.cpp):
// the error string, HIP call checking, device scopes and buffers, the option store, the staging
// pool, and the batch-setup helpers of the one-shot operators (kma_abi_ops.cpp,
// kma_abi_sets.cpp). Private to the library, not installed. Per-process state (the options, the
// staging pool, the thread's error string and shard width) is defined once, in kma_host.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kmeranno.h"

namespace kma {
namespace host {

// ---- errors (kma_last_error) --------------------------------------------------------------------
extern thread_local std::string g_err;
// Sets the calling thread's error string; returns code.
int fail(int code, const char* fmt, ...);

#define KMA_HIP(call)                                                                  \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(e_ == hipErrorOutOfMemory ? KMA_E_NOMEM : KMA_E_DEVICE, "%s: %s (%s:%d)", \
                  #call, hipGetErrorString(e_), __FILE__, __LINE__);                    \
  } while (0)

// Make `device` current for the scope; restore the caller's device after (torch keeps its own).
struct DeviceScope {
  int prev = -1;
  int device;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int device) : device(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = hipSetDevice(device);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  // KMA_OK, or the operators' KMA_E_DEVICE failure (with the runtime's reason) when the device
  // could not be made current.
  int entered() const {
    return err == hipSuccess ? KMA_OK
                             : fail(KMA_E_DEVICE, "hipSetDevice(%d): %s", device,
                                    hipGetErrorString(err));
  }
};

// Device buffers freed on scope exit (one-shot builders only).
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class T>
  hipError_t alloc(T** out, size_t bytes) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
    if (e == hipSuccess) p.push_back(q);
    *out = static_cast<T*>(q);
    return e;
  }
};

// A device buffer that only grows (host contexts).
template <class T>
struct Grow {
  T* p = nullptr;
  size_t cap = 0;  // elements
  hipError_t reserve(size_t n) {
    if (p && n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(n + n / 4, 256);
    hipError_t e = hipMalloc(&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
// Pinned host staging that only grows.
struct Pinned {
  uint8_t* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (p && n <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(n + n / 4, 4096);
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// ---- small shared helpers (kma_host.cpp) --------------------------------------------------------
void standard_lut(uint8_t lut[256]);
int check_k(int k);
const char* ncbi_code(int gc);
std::vector<uint32_t> shard_bounds(const uint64_t* off, uint32_t n, int parts);

// ---- options (kma_option_set; include/kmeranno.h) -----------------------------------------------
constexpr int64_t kOptUnset = INT64_MIN;  // workspace override not set: the library default
bool option_valid(int opt, int64_t v);
int64_t opt(int o);

// ---- host CPUs and staging widths (kma_host.cpp) ------------------------------------------------
size_t host_cores();
size_t staging_width(int n_replicas);
size_t staging_threads();
extern thread_local size_t t_shard_width;
struct ShardWidth {
  explicit ShardWidth(size_t w) { t_shard_width = w; }
  ~ShardWidth() { t_shard_width = 0; }
};

// Library-wide pool of staging threads (grown on demand, never shrunk; threads sleep when idle).
// run(n, width, fn) calls fn(0..n-1) on the calling thread plus up to width - 1 pool threads and
// returns when every call has returned. Several host calls may run jobs at once (kma apply's
// workers each stage their own batch; a replicated table's host call stages every replica's
// share at once): pool threads take the oldest job with free width, and a caller always works on
// its own job, so every job finishes even when the pool is busy. The pool grows to the summed
// width of the jobs running at once (round 5 grew it to one job's width: 8 replicas' jobs of 16
// shared at most 63 threads). Round 3 and early round 4 spawned threads per staging piece: a c5
// host call spent milliseconds creating ~120 threads, and pieces of 5 chunks kept 5 of 16
// threads busy.
class StagingPool {
 public:
  template <class F>
  void run(uint64_t n, size_t width, F&& fn) {
    run_with(n, width, std::forward<F>(fn), [](auto& help) { while (help()) {} });
  }
  // run() whose calling thread runs caller(help) instead of draining the job: help() makes one
  // of the job's calls (in index order with the pool threads) on the calling thread and returns
  // false once every call has been taken. The calling thread can so act on the job's progress
  // (the host call issues each segment's copy as soon as its chunks are packed) and help
  // whenever it would otherwise wait. Returns after every call has returned.
  template <class F, class C>
  void run_with(uint64_t n, size_t width, F&& fn, C&& caller) {
    width = std::max<size_t>(1, std::min<size_t>(width, n));
    Job j;
    j.n = n;
    j.width = width;
    j.call = [](void* f, uint64_t i) { (*static_cast<std::remove_reference_t<F>*>(f))(i); };
    j.fn = (void*)&fn;
    if (width > 1) {
      std::lock_guard<std::mutex> g(mu_);
      demand_ += width - 1;
      while (threads_.size() < demand_ && threads_.size() < kMaxThreads)
        threads_.emplace_back([this] { worker(); });
      jobs_.push_back(&j);
      cv_.notify_all();
    }
    auto help = [&j]() {
      const uint64_t i = j.next.fetch_add(1);
      if (i >= j.n) return false;
      j.call(j.fn, i);
      return true;
    };
    caller(help);
    drain(j);
    if (width > 1) {
      std::unique_lock<std::mutex> lk(mu_);
      jobs_.erase(std::remove(jobs_.begin(), jobs_.end(), &j), jobs_.end());
      demand_ -= width - 1;
      done_cv_.wait(lk, [&] { return j.active == 0; });
    }
  }
  ~StagingPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
      cv_.notify_all();
    }
    for (auto& t : threads_) t.join();
  }

 private:
  static constexpr size_t kMaxThreads = 255;
  struct Job {
    uint64_t n = 0;
    size_t width = 1;
    size_t active = 0;  // pool threads inside drain() (guarded by mu_)
    std::atomic<uint64_t> next{0};
    void (*call)(void*, uint64_t) = nullptr;
    void* fn = nullptr;
  };
  static void drain(Job& j) {
    for (uint64_t i; (i = j.next.fetch_add(1)) < j.n;) j.call(j.fn, i);
  }
  void worker() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      Job* j = nullptr;
      cv_.wait(lk, [&] {
        if (stop_) return true;
        for (Job* c : jobs_)
          if (c->active + 1 < c->width && c->next.load() < c->n) return (j = c) != nullptr;
        return false;
      });
      if (stop_) return;
      ++j->active;
      lk.unlock();
      drain(*j);
      lk.lock();
      if (--j->active == 0) done_cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  std::vector<Job*> jobs_;
  std::vector<std::thread> threads_;
  size_t demand_ = 0;  // summed width - 1 of the jobs running (guarded by mu_)
  bool stop_ = false;
};

StagingPool& staging_pool();  // the process's one pool (never destroyed)
void rebase_offsets(uint64_t* dst, const uint64_t* src, uint64_t n, uint64_t base);
uint32_t offsets_decrease_at(const uint64_t* offsets, uint32_t n);
void pool_memcpy(void* dst, const void* src, size_t n);
// Host bytes -> pinned staging (on the pool) -> one copy on s (kma_abi_proteins.cpp).
hipError_t stage_h2d(uint8_t* d_dst, uint8_t* h_pinned, const uint8_t* src, size_t len,
                     hipStream_t s);

// Run f(i) for i in [0, n) on n threads (inline for one) and return the first failure, with
// its message moved to the calling thread (kma_last_error is thread-local).
template <class F>
int fan_out(int n, F f) {
  if (n == 1) return f(0);
  std::vector<int> rc(n, KMA_OK);
  std::vector<std::string> msg(n);
  std::vector<std::thread> th;
  for (int i = 0; i < n; ++i)
    th.emplace_back([&, i] {
      rc[i] = f(i);
      if (rc[i] != KMA_OK) msg[i] = g_err;
    });
  for (auto& x : th) x.join();
  for (int i = 0; i < n; ++i)
    if (rc[i] != KMA_OK) {
      g_err = msg[i];
      return rc[i];
    }
  return KMA_OK;
}

// ---- batch setup of the one-shot operators (kma_abi_ops.cpp, kma_abi_sets.cpp) ------------------
// The n + 1 offsets of a batch (n == 0: not read): KMA_E_INVALID "[<what> ]offsets decrease at
// <s>" at the first s with offsets[s + 1] < offsets[s] (what may be ""); then, with the message
// `too_long`, when offsets[n] - offsets[0] reaches limit (0: no limit).
int check_offsets(const uint64_t* offsets, uint32_t n, const char* what, uint64_t limit,
                  const char* too_long);

// A host batch on the device: the payload bytes [offsets[0], offsets[n]) with `pad` zero bytes
// after them, and the n + 1 offsets rebased to start at 0.
struct DevBatch {
  uint8_t* bytes = nullptr;
  uint64_t* off = nullptr;
  uint64_t total = 0;  // payload bytes
};
// Validates nothing. Allocates from b (total + pad bytes, then the offsets), then on the null
// stream copies the payload (when there is any), zeroes the pad and copies the offsets.
int upload_batch(DevBufs& b, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                 uint64_t pad, DevBatch* out);

// Scratch of the sort / scan launchers ("temp == nullptr: *temp_bytes = the need"): every size
// query writes through ask(), alloc() takes the largest need from b, and each real call gets p
// and, through bytes(), a fresh copy of the capacity.
struct Scratch {
  void* p = nullptr;
  size_t cap = 0, q = 0;
  size_t* ask() {
    cap = std::max(cap, q);
    q = 0;
    return &q;
  }
  hipError_t alloc(DevBufs& b) {
    ask();  // the last answer
    return b.alloc(&p, cap);
  }
  size_t* bytes() {
    q = cap;
    return &q;
  }
};

// The word a kernel sets when a counted window holds a byte outside the standard alphabet.
struct AlphabetFlag {
  uint32_t* d = nullptr;
  int init(DevBufs& b) {
    KMA_HIP(b.alloc(&d, 4));
    KMA_HIP(hipMemset(d, 0, 4));
    return KMA_OK;
  }
  int check() const {
    uint32_t alpha = 0;
    KMA_HIP(hipMemcpy(&alpha, d, 4, hipMemcpyDeviceToHost));
    if (alpha) return fail(KMA_E_ALPHABET, "a protein window holds a byte outside A-Z and '*'");
    return KMA_OK;
  }
};

}  // namespace host
}  // namespace kma
