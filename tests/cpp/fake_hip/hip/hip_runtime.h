// A stand-in for <hip/hip_runtime.h> on a machine without HIP (tests/cpp/owned_test.cpp,
// launch_seq_test.cpp): the types and the calls csrc/mcpt_owned.h and csrc/mcpt_launch_seq.h use.
// Creating and destroying is a counting fake on malloc / free, with a switch that makes the n-th
// allocation from now fail.  Events and streams carry a serial number (creation order: 1, 2, ...;
// the null stream is 0), and the calls on them — record, wait, synchronize, elapsed time — append
// (call, serial, serial) to a log, with a switch that makes the n-th logged call from now fail and a
// table of the elapsed times a test scripted per event pair.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
struct int4 { int x, y, z, w; };
struct fake_hip_stream { long id; };
struct fake_hip_event { long id; };
typedef fake_hip_stream* hipStream_t;
typedef fake_hip_event* hipEvent_t;
constexpr unsigned hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocDefault = 0;

namespace fake_hip {
struct Counts {
  long live_dev = 0, live_host = 0, live_events = 0, live_streams = 0;   // created and not yet destroyed
  long calls = 0;                                                        // every call of the fake
  long fail_in = 0;                                                      // n > 0: the n-th allocation from now fails
};
inline Counts& counts() {
  static Counts c;
  return c;
}
enum Call { kRecord, kWait, kSync, kElapsed };
struct Logged {
  Call call;
  long a, b;   // kRecord: event, stream; kWait: stream, event; kSync: event, 0; kElapsed: start, stop
  bool operator==(const Logged& o) const { return call == o.call && a == o.a && b == o.b; }
};
struct Log {
  std::vector<Logged> calls;
  long fail_in = 0;                                  // n > 0: the n-th logged call from now fails (it is logged)
  std::map<std::pair<long, long>, float> elapsed;    // (start, stop) -> ms; an unscripted pair fails
  long serials = 0;                                  // events and streams created so far
};
inline Log& log() {
  static Log l;
  return l;
}
template <class H>
inline long serial(H h) { return h ? h->id : 0; }
inline hipError_t logged(Call call, long a, long b) {
  Log& l = log();
  ++counts().calls;
  l.calls.push_back({call, a, b});
  return l.fail_in > 0 && --l.fail_in == 0 ? hipErrorInvalidValue : hipSuccess;
}
inline hipError_t allocate(void** p, size_t bytes, long& live) {
  Counts& c = counts();
  ++c.calls;
  if (c.fail_in > 0 && --c.fail_in == 0) return hipErrorOutOfMemory;   // (*p is left as it was, as HIP leaves it)
  *p = std::malloc(bytes ? bytes : 1);
  ++live;
  return hipSuccess;
}
template <class H>
inline hipError_t release(H h, long& live) {
  ++counts().calls;
  if (!h) return hipSuccess;
  std::free(h);   // (a second release of one handle is a double free: the sanitized build stops on it)
  --live;
  return hipSuccess;
}
// an event or a stream: allocated, then numbered
template <class H>
inline hipError_t create(H** h, long& live) {
  const hipError_t e = allocate(reinterpret_cast<void**>(h), sizeof(H), live);
  if (e == hipSuccess) (*h)->id = ++log().serials;
  return e;
}
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) { return fake_hip::allocate(p, bytes, fake_hip::counts().live_dev); }
inline hipError_t hipFree(void* p) { return fake_hip::release(p, fake_hip::counts().live_dev); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_hip::allocate(p, bytes, fake_hip::counts().live_host); }
inline hipError_t hipHostFree(void* p) { return fake_hip::release(p, fake_hip::counts().live_host); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_hip::create(e, fake_hip::counts().live_events); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::release(e, fake_hip::counts().live_events); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake_hip::create(s, fake_hip::counts().live_streams); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return fake_hip::create(s, fake_hip::counts().live_streams); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::release(s, fake_hip::counts().live_streams); }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return fake_hip::logged(fake_hip::kRecord, fake_hip::serial(e), fake_hip::serial(s)); }
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { return fake_hip::logged(fake_hip::kWait, fake_hip::serial(s), fake_hip::serial(e)); }
inline hipError_t hipEventSynchronize(hipEvent_t e) { return fake_hip::logged(fake_hip::kSync, fake_hip::serial(e), 0); }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t start, hipEvent_t stop) {
  const std::pair<long, long> key(fake_hip::serial(start), fake_hip::serial(stop));
  const hipError_t e = fake_hip::logged(fake_hip::kElapsed, key.first, key.second);
  const auto it = fake_hip::log().elapsed.find(key);
  if (e != hipSuccess || it == fake_hip::log().elapsed.end()) return hipErrorInvalidValue;
  *ms = it->second;
  return hipSuccess;
}
