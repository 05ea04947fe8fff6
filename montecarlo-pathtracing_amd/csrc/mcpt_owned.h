// mcpt_owned.h — the owners of what a context holds on the device: one allocation (DevBuf), its
// pinned-host twin (HostBuf), an event, a stream.  Move-only; each frees what it holds when it is
// destroyed, reset or assigned over, so a group of them (mcpt_ctx.h) ends its lifetime with
// `group = {}`.  An owner converts to the raw handle it holds.  Nothing here waits for a stream: a
// caller whose queued work still uses a buffer waits before it lets the buffer go.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace mcpt {

// one device allocation of size() elements of T
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {   // (what it held goes with t)
    DevBuf t(std::move(o));
    std::swap(p_, t.p_); std::swap(n_, t.n_);
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }
  void reset() {
    if (p_) (void)hipFree(std::exchange(p_, nullptr));
    n_ = 0;
  }
  // frees what it held, then allocates n elements; on failure it is empty
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    n_ = e == hipSuccess ? n : 0;   // (a failed call leaves p_ null)
    return e;
  }
  // at least n elements: no call when it holds them already (the contents are not kept otherwise)
  hipError_t ensure(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// the same in pinned host memory
template <class T>
class HostBuf {
 public:
  HostBuf() = default;
  HostBuf(HostBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  HostBuf& operator=(HostBuf&& o) noexcept {   // (what it held goes with t)
    HostBuf t(std::move(o));
    std::swap(p_, t.p_); std::swap(n_, t.n_);
    return *this;
  }
  ~HostBuf() { reset(); }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  void reset() {
    if (p_) (void)hipHostFree(std::exchange(p_, nullptr));
    n_ = 0;
  }
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), hipHostMallocDefault);
    n_ = e == hipSuccess ? n : 0;   // (a failed call leaves p_ null)
    return e;
  }
  hipError_t ensure(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// an event, created on first use with the flags of that use
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {   // (what it held goes with t)
    Event t(std::move(o));
    std::swap(e_, t.e_);
    return *this;
  }
  ~Event() { reset(); }
  operator hipEvent_t() const { return e_; }
  hipError_t ensure(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  void reset() { if (e_) (void)hipEventDestroy(std::exchange(e_, nullptr)); }

 private:
  hipEvent_t e_ = nullptr;
};

// a stream, created on first use with flags or, with_priority, flags and a priority
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept {   // (what it held goes with t)
    Stream t(std::move(o));
    std::swap(s_, t.s_);
    return *this;
  }
  ~Stream() { reset(); }
  operator hipStream_t() const { return s_; }
  hipError_t ensure(unsigned flags) { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, flags); }
  hipError_t ensure_with_priority(unsigned flags, int priority) {
    return s_ ? hipSuccess : hipStreamCreateWithPriority(&s_, flags, priority);
  }
  void reset() { if (s_) (void)hipStreamDestroy(std::exchange(s_, nullptr)); }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace mcpt
