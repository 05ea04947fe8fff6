// Known answers for the owners of csrc/mcpt_owned.h (DevBuf, HostBuf, Event, Stream) against the
// counting stand-in tests/cpp/fake_hip: what each operation leaves live, that nothing is freed twice,
// and the way a group of owners is built (into a local group, moved in on success) with a failure
// injected at each allocation in turn.  Stand-alone: plain and AddressSanitizer + UBSan builds
// (tests/test_owned_host.py); the stand-in really allocates, so a leak fails the sanitized run at exit.
// The context's own groups (mcpt_ctx.h) need the whole HIP runtime's headers, so the pattern is
// checked on a group of the same shape defined here.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "mcpt_owned.h"

using mcpt::DevBuf;
using mcpt::Event;
using mcpt::HostBuf;
using mcpt::Stream;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

static fake_hip::Counts& C() { return fake_hip::counts(); }
static bool live(long dev, long host, long events, long streams) {
  return C().live_dev == dev && C().live_host == host && C().live_events == events && C().live_streams == streams;
}

static void test_devbuf() {
  {
    DevBuf<float4> a;
    CHECK(!a && a.size() == 0 && a.bytes() == 0 && live(0, 0, 0, 0));
    const long calls0 = C().calls;
    a.reset();   // (an empty owner makes no call)
    CHECK(C().calls == calls0);
    CHECK(a.alloc(10) == hipSuccess && a && a.size() == 10 && a.bytes() == 160 && live(1, 0, 0, 0));
    static_cast<float4*>(a)[9].w = 1.0f;   // (the memory is the size it says)
    const long calls = C().calls;
    float4* p = a;
    CHECK(a.ensure(10) == hipSuccess && a.ensure(3) == hipSuccess && a.ensure(0) == hipSuccess);
    CHECK(C().calls == calls && static_cast<float4*>(a) == p && a.size() == 10);   // n <= size(): no call
    CHECK(a.ensure(11) == hipSuccess && a.size() == 11 && live(1, 0, 0, 0));       // grown: the old one freed
    CHECK(a.alloc(4) == hipSuccess && a.size() == 4 && live(1, 0, 0, 0));          // alloc frees what it held
    DevBuf<float4> b(std::move(a));                                               // move-construct
    CHECK(!a && a.size() == 0 && b && b.size() == 4 && live(1, 0, 0, 0));
    DevBuf<float4> d;
    CHECK(d.alloc(7) == hipSuccess && live(2, 0, 0, 0));
    d = std::move(b);                                                             // move-assign over a live buffer
    CHECK(!b && d.size() == 4 && live(1, 0, 0, 0));
    d = std::move(d);                                                             // (onto itself: kept)
    CHECK(d && d.size() == 4 && live(1, 0, 0, 0));
    d.reset();
    CHECK(!d && d.size() == 0 && live(0, 0, 0, 0));
    d.reset();                                                                    // (twice: nothing freed twice)
    CHECK(live(0, 0, 0, 0));
    // a failed alloc: empty, size 0, nothing live, whether it held something or not
    C().fail_in = 1;
    CHECK(d.alloc(5) == hipErrorOutOfMemory && !d && d.size() == 0 && live(0, 0, 0, 0));
    CHECK(d.alloc(5) == hipSuccess && live(1, 0, 0, 0));
    C().fail_in = 1;
    CHECK(d.ensure(6) == hipErrorOutOfMemory && !d && d.size() == 0 && live(0, 0, 0, 0));
    CHECK(d.alloc(2) == hipSuccess && live(1, 0, 0, 0));
  }   // scope exit frees
  CHECK(live(0, 0, 0, 0));
  std::printf("devbuf: ok\n");
}

static void test_hostbuf() {
  {
    HostBuf<unsigned> h;
    CHECK(!h && h.size() == 0);
    CHECK(h.ensure(8) == hipSuccess && h && h.size() == 8 && live(0, 1, 0, 0));
    const long calls = C().calls;
    CHECK(h.ensure(8) == hipSuccess && C().calls == calls);
    HostBuf<unsigned> g(std::move(h));
    CHECK(!h && g.size() == 8 && live(0, 1, 0, 0));
    HostBuf<unsigned> k;
    CHECK(k.alloc(1) == hipSuccess && live(0, 2, 0, 0));
    k = std::move(g);
    CHECK(live(0, 1, 0, 0));
    C().fail_in = 1;
    CHECK(k.alloc(3) == hipErrorOutOfMemory && !k && k.size() == 0 && live(0, 0, 0, 0));
    CHECK(k.alloc(3) == hipSuccess);
  }
  CHECK(live(0, 0, 0, 0));
  std::printf("hostbuf: ok\n");
}

static void test_event_stream() {
  {
    Event e;
    Stream s, t;
    CHECK(!e && !s && live(0, 0, 0, 0));   // created lazily
    CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && e && live(0, 0, 1, 0));
    const hipEvent_t raw = e;
    const long calls = C().calls;
    CHECK(e.ensure() == hipSuccess && C().calls == calls && static_cast<hipEvent_t>(e) == raw);   // once
    CHECK(s.ensure(hipStreamNonBlocking) == hipSuccess && t.ensure_with_priority(hipStreamNonBlocking, -1) == hipSuccess);
    CHECK(live(0, 0, 1, 2));
    Event f(std::move(e));
    CHECK(!e && f && live(0, 0, 1, 2));
    Event g;
    CHECK(g.ensure() == hipSuccess && live(0, 0, 2, 2));
    g = std::move(f);
    CHECK(live(0, 0, 1, 2));
    s = std::move(t);
    CHECK(!t && s && live(0, 0, 1, 1));
    s.reset();
    s.reset();
    CHECK(!s && live(0, 0, 1, 0));
    C().fail_in = 1;
    CHECK(s.ensure(hipStreamNonBlocking) == hipErrorOutOfMemory && !s && live(0, 0, 1, 0));
    // arrays and vectors of events: the timing pairs and the per-call ring
    Event pair[2];
    std::vector<Event> ring;
    for (Event& p : pair) CHECK(p.ensure() == hipSuccess);
    for (int i = 0; i < 9; ++i) {   // (the vector grows: its elements move, none is destroyed twice)
      Event n;
      CHECK(n.ensure() == hipSuccess);
      ring.push_back(std::move(n));
    }
    CHECK(live(0, 0, 12, 0));
  }
  CHECK(live(0, 0, 0, 0));
  std::printf("event_stream: ok\n");
}

// a group of one lifetime, of the shape of mcpt_ctx's: owners and the plain state that ends with them
struct Group {
  DevBuf<float4> a;
  DevBuf<int> b[2];
  HostBuf<unsigned> h;
  Event ev[2];
  Stream st;
  bool on = false;
  long long passes = 0;
};
constexpr int kGroupAllocations = 7;
// built as the context's ensure_* functions build theirs: into a local group, moved in on success
static hipError_t ensure_group(Group& dst, size_t n) {
  if (dst.a) return hipSuccess;
  Group g;
  hipError_t e = g.a.alloc(n);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = g.b[k].alloc(n);
  if (e == hipSuccess) e = g.h.alloc(4);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = g.ev[k].ensure();
  if (e == hipSuccess) e = g.st.ensure(hipStreamNonBlocking);
  if (e != hipSuccess) return e;
  g.on = true;
  dst = std::move(g);
  return hipSuccess;
}
static bool group_empty(const Group& g) {
  return !g.a && !g.b[0] && !g.b[1] && !g.h && !g.ev[0] && !g.ev[1] && !g.st && !g.on && g.passes == 0 &&
         g.a.size() == 0 && g.b[0].size() == 0 && g.b[1].size() == 0 && g.h.size() == 0;
}

static void test_group() {
  Group g;
  for (int fail = 1; fail <= kGroupAllocations; ++fail) {   // a failure at each allocation in turn
    C().fail_in = fail;
    CHECK(ensure_group(g, 16) == hipErrorOutOfMemory);
    CHECK(C().fail_in == 0 && group_empty(g) && live(0, 0, 0, 0));
  }
  C().fail_in = kGroupAllocations + 1;   // (one past the last: the build succeeds)
  CHECK(ensure_group(g, 16) == hipSuccess && g.on && g.a.size() == 16 && live(3, 1, 2, 1));
  C().fail_in = 0;
  const long calls = C().calls;
  CHECK(ensure_group(g, 16) == hipSuccess && C().calls == calls);   // held: no call
  g.passes = 70;
  g = {};   // ending the lifetime
  CHECK(group_empty(g) && live(0, 0, 0, 0));
  CHECK(ensure_group(g, 5) == hipSuccess && live(3, 1, 2, 1));      // and beginning the next
  {
    Group other;
    CHECK(ensure_group(other, 3) == hipSuccess && live(6, 2, 4, 2));
    g = std::move(other);   // over a full group: its owners freed, the other's taken
    CHECK(g.a.size() == 3 && live(3, 1, 2, 1));
  }
  CHECK(live(3, 1, 2, 1));
  g = {};
  CHECK(live(0, 0, 0, 0));
  std::printf("group: ok\n");
}

int main() {
  test_devbuf();
  test_hostbuf();
  test_event_stream();
  test_group();
  CHECK(live(0, 0, 0, 0));
  std::printf("all: ok\n");
  return 0;   // (sanitized build: the leak check at exit is the last assertion)
}
