// Device / pinned allocations of the library go through these wrappers so that one environment variable shows where
// every byte lives: HG_MEMLOG=<file> appends one line per allocation, free and scan call (name, base, end, size).
// A GPU memory fault reports only an address; this log is what maps it to a buffer (or to the gap right after one).
#pragma once
#include <hip/hip_runtime.h>

#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <utility>

namespace hgmem {

inline FILE *log_file() {
  static FILE *f = [] {
    const char *path = std::getenv("HG_MEMLOG");
    return path && *path ? std::fopen(path, "a") : nullptr;
  }();
  return f;
}
inline void note(const char *fmt, ...) {
  FILE *f = log_file();
  if (!f) return;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(f, fmt, ap);
  va_end(ap);
  std::fflush(f);  // the process may die in the next kernel
}

template <typename T>
inline hipError_t dev_alloc(T **ptr, size_t bytes, const char *name) {
  hipError_t e = hipMalloc(reinterpret_cast<void **>(ptr), bytes);
  if (log_file())
    note("alloc dev  %-14s %p .. %p  %zu  %s\n", name, static_cast<void *>(*ptr), static_cast<void *>(reinterpret_cast<char *>(*ptr) + bytes), bytes,
         e == hipSuccess ? "ok" : hipGetErrorString(e));
  return e;
}
template <typename T>
inline hipError_t host_alloc(T **ptr, size_t bytes, const char *name) {
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(ptr), bytes);
  if (log_file())
    note("alloc host %-14s %p .. %p  %zu  %s\n", name, static_cast<void *>(*ptr), static_cast<void *>(reinterpret_cast<char *>(*ptr) + bytes), bytes,
         e == hipSuccess ? "ok" : hipGetErrorString(e));
  return e;
}
inline void dev_free(void *p, const char *name) {
  if (!p) return;
  if (log_file()) note("free  dev  %-14s %p\n", name, p);
  (void)hipFree(p);
}
inline void host_free(void *p, const char *name) {
  if (!p) return;
  if (log_file()) note("free  host %-14s %p\n", name, p);
  (void)hipHostFree(p);
}

enum class Space { Host, Dev };  // pinned host memory, device memory

// The owner of one allocation: pointer, capacity in elements, log name, bytes of slack behind the elements (16 where kernels
// read whole 16-byte words up to the end; 0 for arrays that are written by index).  Not copyable.  The destructor frees, so
// every `alloc` line of the log gets its `free` line; reserve() is the only way to allocate.
template <typename T, Space S>
class Buf {
 public:
  explicit Buf(const char *name, size_t slack = 16) : name_(name), slack_(slack) {}
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() { release(); }
  T *get() const { return p_; }
  size_t cap() const { return cap_; }
  // Room for `need` elements: nothing to do if there is.  Else the buffer is freed and one of new_cap (>= need) elements plus
  // the slack allocated; contents are not kept.  false, with {nullptr, 0} left behind, if that fails.
  bool reserve(size_t need, size_t new_cap) {
    if (cap_ >= need) return true;
    assert(new_cap >= need);
    release();
    const size_t bytes = new_cap * sizeof(T) + slack_;
    if ((S == Space::Dev ? dev_alloc(&p_, bytes, name_) : host_alloc(&p_, bytes, name_)) != hipSuccess) {
      p_ = nullptr;
      return false;
    }
    cap_ = new_cap;
    return true;
  }
  // Room for `need` elements with the first `keep` (<= cap()) kept: nothing to do if there is.  Else a fresh allocation of
  // new_cap (>= need) elements plus the slack takes those elements (a copy on `stream`, waited for: work queued on the stream
  // may still read the old one) and is swapped in, and the old one is freed.  false, with the buffer as it was, if that fails.
  bool grow(size_t need, size_t new_cap, size_t keep, hipStream_t stream) {
    if (cap_ >= need) return true;
    assert(new_cap >= need && keep <= cap_);
    T *fresh = nullptr;
    const size_t bytes = new_cap * sizeof(T) + slack_;
    if ((S == Space::Dev ? dev_alloc(&fresh, bytes, name_) : host_alloc(&fresh, bytes, name_)) != hipSuccess) return false;
    if (log_file()) note("grow  %s  %-14s %p -> %p  keeps %zu\n", S == Space::Dev ? "dev " : "host", name_, static_cast<void *>(p_), static_cast<void *>(fresh), keep * sizeof(T));
    if ((keep && hipMemcpyAsync(fresh, p_, keep * sizeof(T), hipMemcpyDefault, stream) != hipSuccess) || hipStreamSynchronize(stream) != hipSuccess) {
      S == Space::Dev ? dev_free(fresh, name_) : host_free(fresh, name_);
      return false;
    }
    release();
    p_ = fresh, cap_ = new_cap;
    return true;
  }
  void swap(Buf &other) {  // (both of one element type and space; the log names stay with the objects)
    std::swap(p_, other.p_);
    std::swap(cap_, other.cap_);
  }

 private:
  void release() {
    S == Space::Dev ? dev_free(p_, name_) : host_free(p_, name_);
    p_ = nullptr, cap_ = 0;
  }
  T *p_ = nullptr;
  size_t cap_ = 0;
  const char *name_;
  size_t slack_;
};

}  // namespace hgmem
