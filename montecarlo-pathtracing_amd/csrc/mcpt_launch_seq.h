// mcpt_launch_seq.h — the order of a render call on the device: which stream a sub-launch's render
// runs on, which events it records and waits for, when a lane's buffers count as free (LaneSeq), and
// which events the timing queries read later (TimingRing).  launch() (mcpt_capi.hip) calls the steps
// in the order they stand here, between its own kernel launches; every HIP call is made here, in
// that order, and tests/cpp/launch_seq_test.cpp replays them on the CPU against tests/cpp/fake_hip.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "mcpt_owned.h"

#define MCPT_SEQ_TRY(call) do { if (const hipError_t e_ = (call); e_ != hipSuccess) return e_; } while (0)

namespace mcpt {

// render calls whose events a context keeps (mcpt_kernel_ms_back)
constexpr int kTimingRing = 64;

// The events of the last kTimingRing render calls, four per sub-launch (a call is split into
// sub-launches at chunk boundaries), so a caller can time a run of calls without waiting after each.
// A call records into the slot after the last committed one (begin) and becomes the last call, the
// one the queries and AUTO read, only with commit(): a call that fails part-way leaves the previous
// call's complete timings in place.
class TimingRing {
 public:
  // kStart: the timed interval's start — for a lane launch that follows one on the other lane, that
  // launch's render end (LaneSeq::start), else the render's own start.  kRenderStart: the render's own
  // start on its stream, lane launches only: kRenderStart -> kRenderEnd is the kernel's whole span,
  // overlapped tails included.
  enum Ev { kStart, kRenderEnd, kCombineEnd, kRenderStart, kEvPerSub };

  // a call of n_sub sub-launches (0: an empty call, one empty interval) records into the next slot;
  // its events are created on demand
  hipError_t begin(int n_sub) {
    rec_ = (pos_ + 1) % kTimingRing; rec_n_ = n_sub > 0 ? n_sub : 1;
    Slot& s = slot_[rec_];
    if ((int)s.lane.size() < rec_n_) s.lane.resize(rec_n_, 0);
    for (Event e; (int)s.ev.size() < kEvPerSub * rec_n_; s.ev.push_back(std::move(e))) MCPT_SEQ_TRY(e.ensure());
    return hipSuccess;
  }
  // of the call being recorded: an event of its sub-launch k, whether k is a lane launch
  hipEvent_t event(int k, Ev which) const { return at(rec_, k, which); }
  void set_lane(int k, bool lane) { slot_[rec_].lane[k] = lane; }
  // no passes: an empty timed interval on stream s
  hipError_t record_empty(hipStream_t s) {
    for (int i = 0; i < kEvPerSub; ++i) MCPT_SEQ_TRY(hipEventRecord(event(0, Ev(i)), s));
    set_lane(0, false);
    return hipSuccess;
  }
  // every event of the call has been recorded: it is the last call now
  void commit() { pos_ = rec_; slot_[pos_].n_sub = rec_n_; ++n_timed_; }

  long long n_timed() const { return n_timed_; }       // render calls committed so far
  int pos() const { return pos_; }                     // the last call's slot
  int n_sub() const { return slot_[pos_].n_sub; }      // its sub-launches (0: no call yet)
  bool is_lane(int slot, int k) const { return slot_[slot].lane[k] != 0; }
  // slot of the call `back` calls before the last one; -1: no such call in the ring
  int slot_back(int back) const {
    return back < 0 || back >= kTimingRing || back >= n_timed_ ? -1 : (pos_ - back + kTimingRing) % kTimingRing;
  }
  // (path-tracing kernel ms, combine kernel ms) summed over the sub-launches of the call in `slot`
  // (waits for it)
  hipError_t launch_ms(int slot, float* trace_ms, float* combine_ms) const {
    *trace_ms = 0.0f; *combine_ms = 0.0f;
    for (int k = 0; k < slot_[slot].n_sub; ++k) {
      float a = 0.0f, b = 0.0f;
      MCPT_SEQ_TRY(hipEventSynchronize(at(slot, k, kCombineEnd)));
      MCPT_SEQ_TRY(hipEventElapsedTime(&a, at(slot, k, kStart), at(slot, k, kRenderEnd)));
      MCPT_SEQ_TRY(hipEventElapsedTime(&b, at(slot, k, kRenderEnd), at(slot, k, kCombineEnd)));
      *trace_ms += a; *combine_ms += b;
    }
    return hipSuccess;
  }
  // the path-tracing kernels' whole spans (own start -> end) summed likewise
  hipError_t span_ms(int slot, float* span) const {
    float tot = 0.0f, a = 0.0f;
    for (int k = 0; k < slot_[slot].n_sub; ++k, tot += a) {
      MCPT_SEQ_TRY(hipEventSynchronize(at(slot, k, kRenderEnd)));
      MCPT_SEQ_TRY(hipEventElapsedTime(&a, at(slot, k, is_lane(slot, k) ? kRenderStart : kStart), at(slot, k, kRenderEnd)));
    }
    *span = tot;
    return hipSuccess;
  }
  // the last call: its first sub-launch's start to its last combine's end (waits for it)
  hipError_t call_ms(float* ms) const {
    MCPT_SEQ_TRY(hipEventSynchronize(at(pos_, n_sub() - 1, kCombineEnd)));
    return hipEventElapsedTime(ms, at(pos_, 0, kStart), at(pos_, n_sub() - 1, kCombineEnd));
  }

 private:
  // a slot's events (kEvPerSub per sub-launch, kept when a later call has fewer), per sub-launch
  // whether it was a lane launch, and the sub-launches of the call committed there
  struct Slot { std::vector<Event> ev; std::vector<char> lane; int n_sub = 0; };
  hipEvent_t at(int slot, int k, Ev which) const { return slot_[slot].ev[kEvPerSub * k + which]; }
  Slot slot_[kTimingRing];
  int pos_ = 0, rec_ = 0, rec_n_ = 0;
  long long n_timed_ = 0;
};

// What orders a render lane (mcpt_ctx::Lane holds its buffers) against the context's stream.
// freed: recorded on the context's stream after the lane's last combine: its buffers are free.
// freed_stale: launches in order on the context's stream used the lane since (not recorded:
// launch-bound calls skip the record; the next waiter records it).  tail: recorded on the lane's
// stream after its last operation.
struct LaneSync { Stream stream; Event freed, tail; bool freed_stale = false; };

// The lane hand-off.  The sub-launches of render calls alternate between two lanes.  A lane launch
// (lanes on, schedule settled, several segments: the render writes only the lane's buffers) runs its
// set-up and render on the lane's stream once the lane's previous combine is done, so it can start
// while the previous launch's last workgroups still run; the combines stay in call order on `main`,
// the context's stream, which stays ordered after all of a lane's work.  Every other launch runs in
// order on `main`.  The steps of a sub-launch, in launch()'s order: pick, acquire, [set-up], start,
// [render], render_done, [combine], combine_done, [sort], release.
struct LaneSeq {
  LaneSync lane[2];
  int next_lane = 0;          // the lane of the next sub-launch
  // The lane of the previous sub-launch if it was a lane launch, else -1.  It is written by release()
  // and reset by lanes_switched() only, so it survives from one call to the next: a call's first lane
  // launch, on the lane other than the previous call's last, starts its timed period at an event
  // recorded on that lane's stream behind the previous call's render (ADVICE.md finding 2).
  int prev_lane = -1;
  // sub-launch k of the call on lane li; lane: a lane launch; ws: the stream of its render and set-up
  // (the lane's, else main); main: the context's stream
  struct Sub { int k, li; bool lane; hipStream_t ws, main; };

  // the lanes' streams and events; the events recorded once, so that the first waits on them are satisfied
  hipError_t create(hipStream_t main) {
    for (LaneSync& L : lane) {
      MCPT_SEQ_TRY(L.stream.ensure(hipStreamNonBlocking));
      MCPT_SEQ_TRY(L.freed.ensure(hipEventDisableTiming));
      MCPT_SEQ_TRY(L.tail.ensure(hipEventDisableTiming));
      MCPT_SEQ_TRY(hipEventRecord(L.freed, main));
      MCPT_SEQ_TRY(hipEventRecord(L.tail, L.stream));
    }
    return hipSuccess;
  }
  // the lanes were switched on or off behind a wait for `main`: no previous lane launch to overlap
  void lanes_switched() { prev_lane = -1; }
  // work in order on `main` used lane li's buffers (mcpt_render_adaptive)
  void used_in_order(int li) { lane[li].freed_stale = true; }

  // sub-launch k takes the next lane
  Sub pick(int k, bool lane_launch, hipStream_t main) {
    const int li = std::exchange(next_lane, next_lane ^ 1);
    return {k, li, lane_launch, lane_launch ? (hipStream_t)lane[li].stream : main, main};
  }
  // (a lane whose last launches ran in order on `main` is free once `main`'s work so far is)
  hipEvent_t freed(int li, hipStream_t main) {
    if (lane[li].freed_stale && hipEventRecord(lane[li].freed, main) == hipSuccess) lane[li].freed_stale = false;
    return lane[li].freed;
  }
  // a lane launch's set-up and render wait for the lane's previous combine
  hipError_t acquire(const Sub& s) { return s.lane ? hipStreamWaitEvent(s.ws, freed(s.li, s.main), 0) : hipSuccess; }
  // The timed interval of a lane launch that follows one on the other lane starts where that
  // launch's render ended (recorded on its stream): the launches overlap, and each is charged its
  // period, not its whole span (which would count the overlapped tails twice)
  bool period(const Sub& s) const { return s.lane && prev_lane >= 0 && prev_lane != s.li; }
  hipError_t start(TimingRing& ring, const Sub& s) {
    ring.set_lane(s.k, s.lane);
    MCPT_SEQ_TRY(hipEventRecord(ring.event(s.k, TimingRing::kStart), period(s) ? (hipStream_t)lane[prev_lane].stream : s.ws));
    return s.lane ? hipEventRecord(ring.event(s.k, TimingRing::kRenderStart), s.ws) : hipSuccess;
  }
  // the combine after the render; (the period's start too, so that the events a caller reads once
  // the combine's end has completed are all complete)
  hipError_t render_done(TimingRing& ring, const Sub& s) {
    MCPT_SEQ_TRY(hipEventRecord(ring.event(s.k, TimingRing::kRenderEnd), s.ws));
    if (s.lane) MCPT_SEQ_TRY(hipStreamWaitEvent(s.main, ring.event(s.k, TimingRing::kRenderEnd), 0));
    return period(s) ? hipStreamWaitEvent(s.main, ring.event(s.k, TimingRing::kStart), 0) : hipSuccess;
  }
  hipError_t combine_done(TimingRing& ring, const Sub& s) { return hipEventRecord(ring.event(s.k, TimingRing::kCombineEnd), s.main); }
  // `main` stays ordered after all of the lane's work (the order's sort too); the lane is free after it
  hipError_t release(const Sub& s) {
    LaneSync& L = lane[s.li];
    if (s.lane) {
      MCPT_SEQ_TRY(hipEventRecord(L.tail, L.stream));
      MCPT_SEQ_TRY(hipStreamWaitEvent(s.main, L.tail, 0));
      MCPT_SEQ_TRY(hipEventRecord(L.freed, s.main));
    }
    L.freed_stale = !s.lane;
    prev_lane = s.lane ? s.li : -1;
    return hipSuccess;
  }

  // prepare_order's copy of the other lane's work-item order on ws: after that lane's last sort and
  // combine; and that lane's next sort, which rewrites its order, waits for the copy
  hipError_t before_order_copy(const Sub& s) {
    MCPT_SEQ_TRY(hipStreamWaitEvent(s.ws, lane[s.li ^ 1].tail, 0));
    return hipStreamWaitEvent(s.ws, freed(s.li ^ 1, s.main), 0);
  }
  hipError_t after_order_copy(const Sub& s) {
    MCPT_SEQ_TRY(hipEventRecord(lane[s.li].tail, s.ws));
    return hipStreamWaitEvent(lane[s.li ^ 1].stream, lane[s.li].tail, 0);
  }
};

}  // namespace mcpt
#undef MCPT_SEQ_TRY
