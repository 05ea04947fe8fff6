// A stand-in for <hip/hip_runtime.h> on a machine without HIP (tests/cpp/owned_test.cpp): the types
// and the calls csrc/mcpt_owned.h uses, each call a counting fake on malloc / free, and a switch that
// makes the n-th allocation from now fail.
#pragma once
#include <cstddef>
#include <cstdlib>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
struct int4 { int x, y, z, w; };
typedef struct fake_hip_stream* hipStream_t;
typedef struct fake_hip_event* hipEvent_t;
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
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) { return fake_hip::allocate(p, bytes, fake_hip::counts().live_dev); }
inline hipError_t hipFree(void* p) { return fake_hip::release(p, fake_hip::counts().live_dev); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_hip::allocate(p, bytes, fake_hip::counts().live_host); }
inline hipError_t hipHostFree(void* p) { return fake_hip::release(p, fake_hip::counts().live_host); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  return fake_hip::allocate(reinterpret_cast<void**>(e), 1, fake_hip::counts().live_events);
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::release(e, fake_hip::counts().live_events); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  return fake_hip::allocate(reinterpret_cast<void**>(s), 1, fake_hip::counts().live_streams);
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) {
  return fake_hip::allocate(reinterpret_cast<void**>(s), 1, fake_hip::counts().live_streams);
}
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::release(s, fake_hip::counts().live_streams); }
