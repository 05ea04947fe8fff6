// The order of a render call on the device (csrc/mcpt_launch_seq.h: LaneSeq, TimingRing), replayed on
// the CPU against the logging stand-in tests/cpp/fake_hip.  render_call() below is launch()'s
// sub-launch loop without its kernels; every expected log is written out here, restated from the
// launch() and the timing entries this header was taken out of, and none comes from running the code
// under test.  An event or stream is named by its serial number (creation order): the context's
// stream first, then per lane its stream, `freed` and `tail`, then the ring's events as calls need
// them, four per sub-launch: 0 the timed interval's start, 1 the render's end, 2 the combine's end,
// 3 the render's own start.  Stand-alone: plain and AddressSanitizer + UBSan builds
// (tests/test_launch_seq_host.py); the leak check at exit is the last assertion.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "mcpt_launch_seq.h"

using fake_hip::kElapsed;
using fake_hip::kRecord;
using fake_hip::kSync;
using fake_hip::kWait;
using fake_hip::Logged;
using mcpt::kTimingRing;
using mcpt::LaneSeq;
using mcpt::TimingRing;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

// serial numbers: the context's stream; lane 0's stream, freed, tail; lane 1's; the ring's first event
constexpr long MAIN = 1, S0 = 2, F0 = 3, T0 = 4, S1 = 5, F1 = 6, T1 = 7, EV0 = 8;
// event i of sub-launch k of a call whose first event is `base`
constexpr long ev(long base, int k, int i) { return base + 4 * k + i; }

static fake_hip::Log& LOG() { return fake_hip::log(); }
static bool log_is(const std::vector<Logged>& want) {
  const std::vector<Logged>& got = LOG().calls;
  bool same = got.size() == want.size();
  for (size_t i = 0; same && i < got.size(); ++i) same = got[i] == want[i];
  if (!same) {
    const char* name[] = {"record", "wait", "sync", "elapsed"};
    std::printf("log: %zu calls, expected %zu\n", got.size(), want.size());
    for (size_t i = 0; i < got.size() || i < want.size(); ++i) {
      if (i < got.size()) std::printf("  got  %-7s %3ld %3ld", name[got[i].call], got[i].a, got[i].b);
      else std::printf("  got  %-15s", "-");
      if (i < want.size()) std::printf("   want %-7s %3ld %3ld", name[want[i].call], want[i].a, want[i].b);
      std::printf("%s\n", i < got.size() && i < want.size() && got[i] == want[i] ? "" : "   <--");
    }
  }
  LOG().calls.clear();
  return same;
}

// a context's stream, lanes and ring, created as mcpt_create creates them, with a fresh log
struct Ctx {
  mcpt::Stream own_stream;
  LaneSeq seq;
  TimingRing ring;
  hipStream_t main = nullptr;
  Ctx() {
    LOG() = {};
    CHECK(own_stream.ensure_with_priority(hipStreamNonBlocking, 0) == hipSuccess);
    main = own_stream;
    CHECK(seq.create(main) == hipSuccess);
    CHECK(log_is({{kRecord, F0, MAIN}, {kRecord, T0, S0}, {kRecord, F1, MAIN}, {kRecord, T1, S1}}));
    CHECK(LOG().serials == T1);
  }
};

#define OR_RETURN(call)                  \
  do {                                   \
    const hipError_t e_ = (call);        \
    if (e_ != hipSuccess) return e_;     \
  } while (0)

// launch()'s sub-launch loop: one entry of `lane` per sub-launch (lanes_ok && n_segments > 1)
static hipError_t render_call(Ctx& c, const std::vector<bool>& lane) {
  const int n_sub = (int)lane.size();
  OR_RETURN(c.ring.begin(n_sub));
  if (n_sub == 0) OR_RETURN(c.ring.record_empty(c.main));
  for (int k = 0; k < n_sub; ++k) {
    const LaneSeq::Sub s = c.seq.pick(k, lane[k], c.main);
    OR_RETURN(c.seq.acquire(s));
    OR_RETURN(c.seq.start(c.ring, s));          // (the render, on s.ws)
    OR_RETURN(c.seq.render_done(c.ring, s));    // (the combine, on the context's stream)
    OR_RETURN(c.seq.combine_done(c.ring, s));
    OR_RETURN(c.seq.release(s));
  }
  c.ring.commit();
  return hipSuccess;
}

// the calls of one lane sub-launch k on lane li (events from `base`), its start recorded on `start_on`
static void want_lane(std::vector<Logged>& w, long base, int k, int li, long start_on, bool period) {
  const long S = li ? S1 : S0, F = li ? F1 : F0, T = li ? T1 : T0;
  w.push_back({kWait, S, F});
  w.push_back({kRecord, ev(base, k, 0), start_on});
  w.push_back({kRecord, ev(base, k, 3), S});
  w.push_back({kRecord, ev(base, k, 1), S});
  w.push_back({kWait, MAIN, ev(base, k, 1)});
  if (period) w.push_back({kWait, MAIN, ev(base, k, 0)});
  w.push_back({kRecord, ev(base, k, 2), MAIN});
  w.push_back({kRecord, T, S});
  w.push_back({kWait, MAIN, T});
  w.push_back({kRecord, F, MAIN});
}

static void test_in_order() {
  Ctx c;
  CHECK(render_call(c, {false, false, false}) == hipSuccess);
  CHECK(log_is({{kRecord, ev(EV0, 0, 0), MAIN}, {kRecord, ev(EV0, 0, 1), MAIN}, {kRecord, ev(EV0, 0, 2), MAIN},
                {kRecord, ev(EV0, 1, 0), MAIN}, {kRecord, ev(EV0, 1, 1), MAIN}, {kRecord, ev(EV0, 1, 2), MAIN},
                {kRecord, ev(EV0, 2, 0), MAIN}, {kRecord, ev(EV0, 2, 1), MAIN}, {kRecord, ev(EV0, 2, 2), MAIN}}));
  CHECK(c.ring.n_sub() == 3 && c.ring.pos() == 1 && c.ring.n_timed() == 1);
  for (int k = 0; k < 3; ++k) CHECK(!c.ring.is_lane(1, k));
  CHECK(c.seq.lane[0].freed_stale && c.seq.lane[1].freed_stale);   // lanes 0, 1, 0 were used
  CHECK(c.seq.next_lane == 1 && c.seq.prev_lane == -1);
  std::printf("in_order: ok\n");
}

static void test_lanes_alternating() {
  Ctx c;
  CHECK(render_call(c, {true, true, true, true}) == hipSuccess);
  std::vector<Logged> w;
  want_lane(w, EV0, 0, 0, S0, false);   // the first: no period, its start on its own stream
  want_lane(w, EV0, 1, 1, S0, true);    // then each start on the other lane's stream
  want_lane(w, EV0, 2, 0, S1, true);
  want_lane(w, EV0, 3, 1, S0, true);
  CHECK(w.size() == 9 + 3 * 10 && log_is(w));
  for (int k = 0; k < 4; ++k) CHECK(c.ring.is_lane(1, k));
  CHECK(!c.seq.lane[0].freed_stale && !c.seq.lane[1].freed_stale);
  CHECK(c.seq.next_lane == 0 && c.seq.prev_lane == 1 && c.ring.n_sub() == 4);
  std::printf("lanes_alternating: ok\n");
}

static void test_lane_after_in_order() {
  Ctx c;
  CHECK(render_call(c, {false, false}) == hipSuccess);   // lanes 0 and 1 in order: both stale
  LOG().calls.clear();
  CHECK(c.seq.lane[0].freed_stale && c.seq.prev_lane == -1 && c.seq.next_lane == 0);
  const long B = EV0 + 8;
  CHECK(render_call(c, {true}) == hipSuccess);           // lane 0
  std::vector<Logged> w = {{kRecord, F0, MAIN}};         // the stale `freed` first, on the context's stream
  want_lane(w, B, 0, 0, S0, false);                      // prev_lane was -1: no period
  CHECK(log_is(w));
  CHECK(!c.seq.lane[0].freed_stale && c.seq.lane[1].freed_stale && c.seq.prev_lane == 0);
  // the stale flag is cleared only if the record succeeded (the wait follows either way)
  LOG().fail_in = 1;
  CHECK(c.seq.freed(1, c.main) != nullptr && c.seq.lane[1].freed_stale);
  CHECK(log_is({{kRecord, F1, MAIN}}));
  CHECK(c.seq.freed(1, c.main) != nullptr && !c.seq.lane[1].freed_stale);
  CHECK(log_is({{kRecord, F1, MAIN}}));
  CHECK(c.seq.freed(1, c.main) != nullptr && log_is({}));
  // work in order on the context's stream that used a lane's buffers (mcpt_render_adaptive)
  c.seq.used_in_order(0);
  CHECK(c.seq.lane[0].freed_stale);
  std::printf("lane_after_in_order: ok\n");
}

static void test_across_calls() {
  Ctx c;
  CHECK(render_call(c, {true, true}) == hipSuccess);   // call A ends on lane 1
  LOG().calls.clear();
  CHECK(c.seq.prev_lane == 1 && c.seq.next_lane == 0);
  CHECK(render_call(c, {true}) == hipSuccess);         // call B's first lane launch, on lane 0
  std::vector<Logged> w;
  want_lane(w, EV0 + 8, 0, 0, S1, true);   // its period starts on lane 1's stream, behind call A's render
  CHECK(log_is(w));
  // ... unless the lanes were switched in between (mcpt_set_render_lanes)
  c.seq.lanes_switched();
  CHECK(c.seq.prev_lane == -1);
  CHECK(render_call(c, {true}) == hipSuccess);         // lane 1
  w.clear();
  want_lane(w, EV0 + 12, 0, 1, S1, false);
  CHECK(log_is(w));
  std::printf("across_calls: ok\n");
}

static void test_empty_call() {
  Ctx c;
  CHECK(render_call(c, {}) == hipSuccess);
  CHECK(log_is({{kRecord, ev(EV0, 0, 0), MAIN}, {kRecord, ev(EV0, 0, 1), MAIN}, {kRecord, ev(EV0, 0, 2), MAIN},
                {kRecord, ev(EV0, 0, 3), MAIN}}));
  CHECK(c.ring.n_timed() == 1 && c.ring.n_sub() == 1 && !c.ring.is_lane(1, 0));
  CHECK(c.seq.next_lane == 0 && c.seq.prev_lane == -1);
  std::printf("empty_call: ok\n");
}

static void test_failure_part_way() {
  Ctx c;
  CHECK(c.ring.n_timed() == 0 && c.ring.n_sub() == 0);
  CHECK(render_call(c, {true, true}) == hipSuccess);
  const float trace[2] = {3.0f, 1.0f}, combine[2] = {0.5f, 0.25f};
  for (int k = 0; k < 2; ++k) {
    LOG().elapsed[{ev(EV0, k, 0), ev(EV0, k, 1)}] = trace[k];
    LOG().elapsed[{ev(EV0, k, 1), ev(EV0, k, 2)}] = combine[k];
  }
  float t = 0.0f, m = 0.0f;
  CHECK(c.ring.launch_ms(c.ring.pos(), &t, &m) == hipSuccess && t == 4.0f && m == 0.75f);
  const long events = fake_hip::counts().live_events;
  // A lane sub-launch makes 10 calls with a period, 9 without.  The first sub-launch of each attempt
  // runs on lane 0, with a period in the first attempt (call A ended on lane 1) and without in the
  // later ones (the attempt before released lane 0 last); the second has a period: calls 11 to 19
  // are the second sub-launch's in every attempt.
  for (int n = 11; n <= 19; ++n) {
    LOG().fail_in = n;
    CHECK(render_call(c, {true, true, true}) == hipErrorInvalidValue);
    CHECK(LOG().fail_in == 0);
    CHECK(c.ring.pos() == 1 && c.ring.n_timed() == 1 && c.ring.n_sub() == 2 && c.ring.slot_back(1) == -1);
    t = m = 0.0f;
    CHECK(c.ring.launch_ms(c.ring.slot_back(0), &t, &m) == hipSuccess && t == 4.0f && m == 0.75f);
    CHECK(c.seq.next_lane == 0 && c.seq.prev_lane == 0);   // two picks, one release
  }
  CHECK(fake_hip::counts().live_events == events + 12);   // slot 2's events, created once
  // a following complete call reuses the slot and its events
  CHECK(render_call(c, {false, false}) == hipSuccess);
  CHECK(c.ring.pos() == 2 && c.ring.n_timed() == 2 && c.ring.n_sub() == 2 && c.ring.slot_back(1) == 1);
  CHECK(fake_hip::counts().live_events == events + 12);
  // an event that cannot be created: the status, and nothing published
  fake_hip::counts().fail_in = 2;
  CHECK(render_call(c, {false}) == hipErrorOutOfMemory && c.ring.pos() == 2 && c.ring.n_timed() == 2);
  std::printf("failure_part_way: ok\n");
}

static void test_ring() {
  Ctx c;
  for (int back : {-1, 0, 1, kTimingRing}) CHECK(c.ring.slot_back(back) == -1);   // a fresh ring holds no call
  CHECK(render_call(c, {false, false, false}) == hipSuccess);                    // slot 1: three sub-launches
  CHECK(c.ring.slot_back(0) == 1 && c.ring.slot_back(1) == -1);
  for (int i = 1; i < kTimingRing + 3; ++i) CHECK(render_call(c, {false}) == hipSuccess);
  CHECK(c.ring.n_timed() == kTimingRing + 3 && c.ring.pos() == 3);
  std::set<int> seen;
  for (int back = 0; back < kTimingRing; ++back) {
    const int slot = c.ring.slot_back(back);
    CHECK(slot == (3 - back + kTimingRing) % kTimingRing && seen.insert(slot).second);
  }
  CHECK(c.ring.slot_back(kTimingRing) == -1 && c.ring.slot_back(-1) == -1);
  // slot 1 was reused by a call of one sub-launch: only that one is read
  LOG().calls.clear();
  LOG().elapsed[{ev(EV0, 0, 0), ev(EV0, 0, 1)}] = 2.0f;
  LOG().elapsed[{ev(EV0, 0, 1), ev(EV0, 0, 2)}] = 0.25f;
  float t = 0.0f, m = 0.0f;
  CHECK(c.ring.launch_ms(1, &t, &m) == hipSuccess && t == 2.0f && m == 0.25f);
  CHECK(log_is({{kSync, ev(EV0, 0, 2), 0}, {kElapsed, ev(EV0, 0, 0), ev(EV0, 0, 1)}, {kElapsed, ev(EV0, 0, 1), ev(EV0, 0, 2)}}));
  std::printf("ring: ok\n");
}

static void test_queries() {
  Ctx c;
  CHECK(render_call(c, {false, true, true}) == hipSuccess);   // in order (lane 0), lane 1, lane 0 with a period
  LOG().calls.clear();
  CHECK(!c.ring.is_lane(1, 0) && c.ring.is_lane(1, 1) && c.ring.is_lane(1, 2));
  const float trace[3] = {4.0f, 2.0f, 1.0f}, combine[3] = {0.5f, 0.25f, 0.125f}, span[3] = {4.0f, 8.0f, 16.0f};
  for (int k = 0; k < 3; ++k) {
    LOG().elapsed[{ev(EV0, k, 0), ev(EV0, k, 1)}] = trace[k];
    LOG().elapsed[{ev(EV0, k, 1), ev(EV0, k, 2)}] = combine[k];
    if (k > 0) LOG().elapsed[{ev(EV0, k, 3), ev(EV0, k, 1)}] = span[k];
  }
  LOG().elapsed[{ev(EV0, 0, 0), ev(EV0, 2, 2)}] = 64.0f;
  float t = 0.0f, m = 0.0f, s = 0.0f, ms = 0.0f;
  CHECK(c.ring.launch_ms(1, &t, &m) == hipSuccess && t == 7.0f && m == 0.875f);
  CHECK(log_is({{kSync, ev(EV0, 0, 2), 0}, {kElapsed, ev(EV0, 0, 0), ev(EV0, 0, 1)}, {kElapsed, ev(EV0, 0, 1), ev(EV0, 0, 2)},
                {kSync, ev(EV0, 1, 2), 0}, {kElapsed, ev(EV0, 1, 0), ev(EV0, 1, 1)}, {kElapsed, ev(EV0, 1, 1), ev(EV0, 1, 2)},
                {kSync, ev(EV0, 2, 2), 0}, {kElapsed, ev(EV0, 2, 0), ev(EV0, 2, 1)}, {kElapsed, ev(EV0, 2, 1), ev(EV0, 2, 2)}}));
  CHECK(c.ring.span_ms(1, &s) == hipSuccess && s == 28.0f);   // start -> render end in order, render start -> render end on a lane
  CHECK(log_is({{kSync, ev(EV0, 0, 1), 0}, {kElapsed, ev(EV0, 0, 0), ev(EV0, 0, 1)},
                {kSync, ev(EV0, 1, 1), 0}, {kElapsed, ev(EV0, 1, 3), ev(EV0, 1, 1)},
                {kSync, ev(EV0, 2, 1), 0}, {kElapsed, ev(EV0, 2, 3), ev(EV0, 2, 1)}}));
  CHECK(c.ring.call_ms(&ms) == hipSuccess && ms == 64.0f);    // first start -> last combine end
  CHECK(log_is({{kSync, ev(EV0, 2, 2), 0}, {kElapsed, ev(EV0, 0, 0), ev(EV0, 2, 2)}}));
  // a failing call: the status; the span is left as it was
  LOG().fail_in = 4;
  s = -1.0f;
  CHECK(c.ring.span_ms(1, &s) == hipErrorInvalidValue && s == -1.0f);
  LOG().fail_in = 5;
  CHECK(c.ring.launch_ms(1, &t, &m) == hipErrorInvalidValue);
  LOG().fail_in = 1;
  CHECK(c.ring.call_ms(&ms) == hipErrorInvalidValue);
  LOG().calls.clear();
  std::printf("queries: ok\n");
}

static void test_order_copy() {
  Ctx c;
  const LaneSeq::Sub s = c.seq.pick(0, true, c.main);   // a lane launch on lane 0 copies lane 1's order
  CHECK(s.li == 0 && s.lane && s.ws == (hipStream_t)c.seq.lane[0].stream && s.main == c.main);
  CHECK(c.seq.before_order_copy(s) == hipSuccess);      // (the two copies, on s.ws)
  CHECK(c.seq.after_order_copy(s) == hipSuccess);
  CHECK(log_is({{kWait, S0, T1}, {kWait, S0, F1}, {kRecord, T0, S0}, {kWait, S1, T0}}));
  // in order on the context's stream, on lane 1, from a lane 0 that was last used in order
  c.seq.used_in_order(0);
  const LaneSeq::Sub o = c.seq.pick(1, false, c.main);
  CHECK(o.li == 1 && !o.lane && o.ws == c.main);
  CHECK(c.seq.before_order_copy(o) == hipSuccess && c.seq.after_order_copy(o) == hipSuccess);
  CHECK(log_is({{kWait, MAIN, T0}, {kRecord, F0, MAIN}, {kWait, MAIN, F0}, {kRecord, T1, MAIN}, {kWait, S0, T1}}));
  CHECK(!c.seq.lane[0].freed_stale);
  LOG().fail_in = 2;
  CHECK(c.seq.before_order_copy(s) == hipErrorInvalidValue && log_is({{kWait, S0, T1}, {kWait, S0, F1}}));
  std::printf("order_copy: ok\n");
}

int main() {
  test_in_order();
  test_lanes_alternating();
  test_lane_after_in_order();
  test_across_calls();
  test_empty_call();
  test_failure_part_way();
  test_ring();
  test_queries();
  test_order_copy();
  const fake_hip::Counts& n = fake_hip::counts();
  CHECK(n.live_dev == 0 && n.live_host == 0 && n.live_events == 0 && n.live_streams == 0);
  std::printf("all: ok\n");
  return 0;   // (sanitized build: the leak check at exit is the last assertion)
}
