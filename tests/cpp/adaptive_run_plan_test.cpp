// Known-answer tests of a queued adaptive run's schedule (csrc/mcpt_adaptive_run_plan.h) on the CPU:
// which rounds select, the grid that holds the list on entry, and the host loop's outcome from the
// list lengths the selects left.  Every expected value is written next to its assertion, worked out
// from the loop in mcpt.h (mcpt_adaptive_run), not taken from a run.  The host loops' step rule
// (until_next) and the C++ driver over it are checked against restatements of the loops they replaced.
#include <cstdio>
#include <vector>

#include "mcpt_adaptive_run_plan.h"
#include "../../include/mcpt.hpp"

namespace plan = mcpt::plan;

// This program links no library: the two entries mcpt.hpp's driver reaches.  The library's
// mcpt_adaptive_until_next is this call into the plan header (mcpt_capi_post.hip).  The price of
// testing the real driver: this test compiles the whole of mcpt.hpp, and links only while everything
// else in that header stays inline and unused here; a new out-of-line reference from
// adaptive_until needs a stand-in below.
int mcpt_adaptive_until_next(int done, int calls, int batch, int max_passes, int check_every, int queued_rounds,
                             int* rounds, int* n_passes, int* select) {
  return plan::until_next(done, calls, batch, max_passes, check_every, queued_rounds, rounds, n_passes, select)
             ? MCPT_OK
             : MCPT_ERR_INVALID_ARG;
}
const char* mcpt_error_string(int) { return "refused"; }

static int g_fails = 0, g_case_fails = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("  line %d: CHECK(%s) failed\n", __LINE__, #cond);       \
      ++g_case_fails;                                                      \
    }                                                                      \
  } while (0)
static void done(const char* name) {
  std::printf("%s: %s\n", name, g_case_fails ? "FAIL" : "ok");
  g_fails += g_case_fails;
  g_case_fails = 0;
}

// the rounds (0-based) that select, as a list
static std::vector<int> selecting(int rounds, int check_every, int batches) {
  std::vector<int> v;
  for (int i = 0; i < rounds; ++i)
    if (plan::run_round_selects(i, rounds, check_every, batches)) v.push_back(i);
  return v;
}

static void test_schedule() {
  // a fresh window (0 batches): round 0 leaves one batch, no select yet
  CHECK((selecting(4, 1, 0) == std::vector<int>{1, 2, 3}));
  CHECK((selecting(1, 1, 0) == std::vector<int>{}));
  CHECK((selecting(1, 1, 1) == std::vector<int>{0}));
  // every third round, and the run's last
  CHECK((selecting(8, 3, 0) == std::vector<int>{2, 5, 7}));
  CHECK((selecting(6, 3, 5) == std::vector<int>{2, 5}));
  // check_every above the run: its last round only
  CHECK((selecting(4, 16, 2) == std::vector<int>{3}));
  // two rounds from a fresh window, every second: round 1 is both a multiple and the last
  CHECK((selecting(2, 2, 0) == std::vector<int>{1}));
  CHECK(plan::run_select_count(4, 1, 0) == 3);
  CHECK(plan::run_select_count(8, 3, 0) == 3);
  CHECK(plan::run_select_count(1, 1, 0) == 0);
  CHECK(plan::run_select_count(256, 1, 7) == 256);
  CHECK(plan::run_select_count(plan::kAdaptiveRunMaxRounds, 1, 0) == 255);
  // outside the run, or no schedule
  CHECK(!plan::run_round_selects(-1, 4, 1, 5));
  CHECK(!plan::run_round_selects(4, 4, 1, 5));
  CHECK(!plan::run_round_selects(1, 4, 0, 5));
  done("schedule");
}

static bool same(const plan::RunOutcome& o, int rounds_run, int selects_run, int n_list) {
  return o.rounds_run == rounds_run && o.selects_run == selects_run && o.n_list == n_list;
}

static void test_outcome() {
  // 6 rounds, every second, 3 batches on entry: selects after rounds 1, 3, 5
  {
    const int ends_non_empty[3] = {9, 7, 2};
    CHECK(same(plan::run_outcome(6, 2, 3, 12, ends_non_empty, 3), 6, 3, 2));
    const int zero_first[3] = {0, 0, 0};      // the first select empties the list: rounds 0 and 1 ran
    CHECK(same(plan::run_outcome(6, 2, 3, 12, zero_first, 3), 2, 1, 0));
    const int zero_middle[3] = {5, 0, 0};     // the second: rounds 0..3
    CHECK(same(plan::run_outcome(6, 2, 3, 12, zero_middle, 3), 4, 2, 0));
    const int zero_last[3] = {5, 4, 0};       // the last: every round ran
    CHECK(same(plan::run_outcome(6, 2, 3, 12, zero_last, 3), 6, 3, 0));
    // an empty list on entry: nothing ran, whatever the ring holds
    CHECK(same(plan::run_outcome(6, 2, 3, 0, ends_non_empty, 3), 0, 0, 0));
    CHECK(same(plan::run_outcome(6, 2, 3, 0, nullptr, 0), 0, 0, 0));
  }
  // a fresh window: round 0 has no select, so the first length belongs to round 1
  {
    const int len[3] = {0, 0, 0};
    CHECK(same(plan::run_outcome(4, 1, 0, 5, len, 3), 2, 1, 0));
    const int len2[3] = {3, 0, 0};
    CHECK(same(plan::run_outcome(4, 1, 0, 5, len2, 3), 3, 2, 0));
  }
  // a run without selects (one round of a fresh window): the round ran, the list is as on entry
  CHECK(same(plan::run_outcome(1, 1, 0, 5, nullptr, 0), 1, 0, 5));
  // the last round selects although it is no multiple of check_every
  {
    const int len[2] = {4, 0};
    CHECK(same(plan::run_outcome(5, 3, 2, 6, len, 2), 5, 2, 0));
  }
  // fewer lengths than selects: stops at what is known, reads nothing past the array
  {
    const int len[1] = {4};
    CHECK(same(plan::run_outcome(6, 2, 3, 12, len, 1), 4, 1, 4));
  }
  done("outcome");
}

static void test_list_groups() {
  // one block per workgroup group at tile width 8, two at 16, four at 32
  CHECK(plan::run_list_groups(15, 8) == 15);
  CHECK(plan::run_list_groups(15, 16) == 8);
  CHECK(plan::run_list_groups(16, 16) == 8);
  CHECK(plan::run_list_groups(15, 32) == 4);
  CHECK(plan::run_list_groups(17, 32) == 5);
  CHECK(plan::run_list_groups(1, 32) == 1);
  CHECK(plan::run_list_groups(0, 16) == 0);
  CHECK(plan::run_list_groups(-3, 16) == 0);
  // 4K: 129,600 blocks
  CHECK(plan::run_list_groups(129600, 8) == 129600);
  CHECK(plan::run_list_groups(129600, 32) == 32400);
  // the groups of the entry length hold every shorter list
  for (int tw : {8, 16, 32})
    for (int n = 1; n <= 40; ++n) CHECK((long long)plan::run_list_groups(40, tw) * (tw / 8) >= n);
  CHECK(plan::run_list_groups(2147483647, 8) == 2147483647);   // (no overflow on the way)
  done("list_groups");
}

// ---- until: the host loop's step rule (plan::until_next) and the driver over it (mcpt::adaptive_until,
// mcpt.hpp) against restatements of the loops they replaced, on a fake device.

// The fake device: its list becomes empty at the k_empty-th select (0: never).  It logs every call;
// a queued run reports what plan::run_outcome derives from the lengths its selects would leave.
struct Event {
  char kind;   // 'r' render(first, n)   's' select   'q' run(first, rounds) -> selects it made
  int first, amount, selects;
  bool operator==(const Event& o) const {
    return kind == o.kind && first == o.first && amount == o.amount && selects == o.selects;
  }
};
struct FakeDevice {
  int k_empty;
  int selects = 0, n_list = 1, most_rounds = 0;
  std::vector<Event> log;
  void render(int first, int n) { log.push_back({'r', first, n, 0}); }
  long long select() {
    log.push_back({'s', 0, 0, 0});
    if (++selects == k_empty) n_list = 0;
    return n_list;
  }
  plan::RunOutcome run(int first, int rounds, int check_every, int batches_on_entry) {
    most_rounds = rounds > most_rounds ? rounds : most_rounds;
    std::vector<int> lengths;
    for (int j = 0; j < plan::run_select_count(rounds, check_every, batches_on_entry); ++j)
      lengths.push_back(selects + j + 1 >= k_empty && k_empty > 0 ? 0 : 1);
    const plan::RunOutcome o =
        plan::run_outcome(rounds, check_every, batches_on_entry, n_list, lengths.data(), (int)lengths.size());
    selects += o.selects_run;
    n_list = o.n_list;
    log.push_back({'q', first, rounds, o.selects_run});
    return o;
  }
};
struct Until {   // a render's arguments, and where it enters (a resume: done, calls > 0)
  int first_pass, batch, max_passes, check_every, queued_rounds, done, calls;
};
struct Trace {
  std::vector<Event> log;
  int done, calls, selects, most_rounds;
  bool operator==(const Trace& o) const {
    return log == o.log && done == o.done && calls == o.calls && selects == o.selects;
  }
};
static int min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

// Renderer.render_adaptive_until of the commit before the rule existed, statement for statement
static Trace parent_python_loop(const Until& p, FakeDevice dev) {
  int done = p.done, calls = p.calls;
  bool have = false;
  long long active = 1;
  while (done < p.max_passes) {
    const int full = (p.max_passes - done) / p.batch;
    int r = calls % p.check_every == 0 ? min3(p.queued_rounds, full, plan::kAdaptiveRunMaxRounds) : 0;
    if (r > 0 && !(r == full && done + r * p.batch == p.max_passes)) r -= r % p.check_every;
    if (r > 0) {
      const plan::RunOutcome got = dev.run(p.first_pass + done, r, p.check_every, calls);
      done += got.rounds_run * p.batch;
      calls += got.rounds_run;
      if (got.selects_run > 0) {
        have = true;
        active = got.n_list;
      }
      if (got.rounds_run < r || (have && active == 0)) break;
      continue;
    }
    const int n = p.batch < p.max_passes - done ? p.batch : p.max_passes - done;
    dev.render(p.first_pass + done, n);
    done += n;
    calls += 1;
    if (calls >= 2 && (calls % p.check_every == 0 || done >= p.max_passes)) {
      active = dev.select();
      have = true;
      if (active == 0) break;
    }
  }
  if (!have) dev.select();
  return {dev.log, done, calls, dev.selects, dev.most_rounds};
}

// mcpt_render's one-device loop of that commit (check_every 1, no select of its own at the end)
static Trace parent_program_loop(const Until& p, FakeDevice dev) {
  int done = p.done, calls = p.calls, rendered = p.done;
  bool converged = false;
  while (done < p.max_passes && !converged) {
    const int whole = (p.max_passes - done) / p.batch;
    if (p.queued_rounds > 0 && whole > 0) {
      const int k = p.queued_rounds < whole ? p.queued_rounds : whole;
      const plan::RunOutcome run = dev.run(p.first_pass + done, k, 1, calls);
      calls += run.rounds_run;
      done += run.rounds_run * p.batch;
      rendered = done;
      if (run.selects_run > 0) converged = run.n_list == 0;
      if (run.rounds_run < k) break;
      continue;
    }
    const int n = p.batch < p.max_passes - done ? p.batch : p.max_passes - done;
    dev.render(p.first_pass + done, n);
    rendered = done + n;
    if (++calls >= 2) converged = dev.select() == 0;
    done += p.batch;
  }
  return {dev.log, rendered, calls, dev.selects, dev.most_rounds};
}

// mcpt_render --temporal-target's frame loop of that commit: `rounds` whole chunks, runs of K rounds
// (0: one run)
static Trace parent_temporal_loop(int pass, int chunk, int rounds, int K, FakeDevice dev) {
  int done = 0;
  while (done < rounds) {
    const int q = (K > 0 ? K : rounds) < rounds - done ? (K > 0 ? K : rounds) : rounds - done;
    const plan::RunOutcome run = dev.run(pass + done * chunk, q, 1, done);
    done += run.rounds_run;
    if (run.rounds_run < q || (run.selects_run > 0 && run.n_list == 0)) break;
  }
  return {dev.log, done * chunk, done, dev.selects, dev.most_rounds};
}

// the driver on the same device; final_select: Renderer::render_adaptive_until's select of its own
// when none has run; only_runs: no render and no select callable, as mcpt_render --temporal-target
static Trace driver(const Until& p, FakeDevice dev, bool final_select, bool only_runs = false) {
  int calls = p.calls;   // (the window's batches on a run's entry: one per call so far)
  std::function<void(int, int)> render = [&](int first, int n) { dev.render(first, n); };
  std::function<long long()> select = [&] { return dev.select(); };
  const mcpt::AdaptiveUntil u = mcpt::adaptive_until(
      p.first_pass, p.batch, p.max_passes, p.check_every, p.queued_rounds, only_runs ? nullptr : render,
      only_runs ? nullptr : select,
      [&](int first, int rounds) {
        const plan::RunOutcome o = dev.run(first, rounds, p.check_every, calls);
        return mcpt::AdaptiveRan{o.rounds_run, o.selects_run, o.n_list};
      },
      [&](int, int calls_now) { calls = calls_now; }, p.done, p.calls);
  CHECK(u.selects == dev.selects);
  if (final_select && u.selects == 0) dev.select();
  return {dev.log, u.done, u.calls, dev.selects, dev.most_rounds};
}

static void test_until() {
  // known answers of the rule: {rounds, n_passes, select}
  auto next = [](int done, int calls, int batch, int max_passes, int check_every, int queued_rounds) {
    std::vector<int> v(3, -1);
    CHECK(plan::until_next(done, calls, batch, max_passes, check_every, queued_rounds, &v[0], &v[1], &v[2]));
    return v;
  };
  CHECK((next(0, 0, 8, 76, 1, 0) == std::vector<int>{0, 8, 0}));     // the first call: no select yet
  CHECK((next(8, 1, 8, 76, 1, 0) == std::vector<int>{0, 8, 1}));     // the second: a select
  CHECK((next(16, 2, 8, 76, 3, 0) == std::vector<int>{0, 8, 1}));    // every third call
  CHECK((next(24, 3, 8, 76, 3, 0) == std::vector<int>{0, 8, 0}));
  CHECK((next(72, 9, 8, 76, 1, 0) == std::vector<int>{0, 4, 1}));    // the short last batch
  CHECK((next(72, 10, 8, 76, 3, 4) == std::vector<int>{0, 4, 1}));   // ... is a single call, at the cap: a select
  CHECK((next(76, 10, 8, 76, 1, 4) == std::vector<int>{0, 0, 0}));   // finished
  CHECK((next(0, 0, 8, 76, 1, 4) == std::vector<int>{4, 0, 0}));     // a run of K
  CHECK((next(0, 0, 8, 76, 3, 4) == std::vector<int>{3, 0, 0}));     // trimmed to a multiple of check_every
  CHECK((next(48, 6, 8, 64, 3, 4) == std::vector<int>{2, 0, 0}));    // ends at the cap: not trimmed
  CHECK((next(48, 6, 8, 76, 3, 4) == std::vector<int>{3, 0, 0}));    // 3 whole batches left, not at the cap: 3
  CHECK((next(8, 1, 8, 76, 3, 4) == std::vector<int>{0, 8, 0}));     // calls no multiple of check_every: single
  CHECK((next(0, 0, 8, 76, 5, 4) == std::vector<int>{0, 8, 0}));     // K below check_every: single
  CHECK((next(0, 0, 1, 1000, 1, 1000) == std::vector<int>{plan::kAdaptiveRunMaxRounds, 0, 0}));
  int a = 7, b = 7, c = 7;
  CHECK(!plan::until_next(0, 0, 0, 76, 1, 0, &a, &b, &c) && !plan::until_next(0, 0, 8, 0, 1, 0, &a, &b, &c));
  CHECK(!plan::until_next(0, 0, 8, 76, 0, 0, &a, &b, &c) && !plan::until_next(-1, 0, 8, 76, 1, 0, &a, &b, &c));
  CHECK(!plan::until_next(0, -1, 8, 76, 1, 0, &a, &b, &c) && !plan::until_next(0, 0, 8, 76, 1, -1, &a, &b, &c));
  CHECK(!plan::until_next(0, 0, 8, 76, 1, 0, nullptr, &b, &c) && !plan::until_next(0, 0, 8, 76, 1, 0, &a, nullptr, &c));
  CHECK(!plan::until_next(0, 0, 8, 76, 1, 0, &a, &b, nullptr) && a == 7 && b == 7 && c == 7);

  // the driver against the loops it replaced
  long long cases = 0;
  for (int batch = 1; batch <= 4; ++batch)
    for (int max_passes = 1; max_passes <= 20; ++max_passes)
      for (int check_every = 1; check_every <= 4; ++check_every)
        for (int queued_rounds = 0; queued_rounds <= 6; ++queued_rounds)
          for (int k_empty : {0, 1, 2, 3, 5})
            for (int resumed = 0; resumed < 2; ++resumed) {
              const Until p = {5, batch, max_passes, check_every, queued_rounds, resumed ? 2 * batch : 0, resumed ? 2 : 0};
              const FakeDevice dev = {k_empty};
              CHECK(driver(p, dev, true) == parent_python_loop(p, dev));
              if (check_every == 1) CHECK(driver(p, dev, false) == parent_program_loop(p, dev));
              if (check_every == 1 && !resumed && max_passes % batch == 0 && max_passes / batch >= 2) {
                const int rounds = max_passes / batch;
                const Until t = {5, batch, max_passes, 1, queued_rounds > 0 ? queued_rounds : rounds, 0, 0};
                CHECK(driver(t, dev, false, true) == parent_temporal_loop(5, batch, rounds, queued_rounds, dev));
              }
              ++cases;
            }
  CHECK(cases == 4 * 20 * 4 * 7 * 5 * 2);
  // a run never exceeds the device's ring, whatever K asks for
  for (int check_every : {1, 3, 7}) {
    const Until p = {1, 1, 1000, check_every, 1000, 0, 0};
    const Trace t = driver(p, FakeDevice{0}, true);
    CHECK(t == parent_python_loop(p, FakeDevice{0}));
    CHECK(t.done == 1000 && t.most_rounds > 0 && t.most_rounds <= plan::kAdaptiveRunMaxRounds);
  }
  done("until");
}

int main() {
  test_schedule();
  test_outcome();
  test_list_groups();
  test_until();
  std::printf("%s\n", g_fails ? "FAILED" : "all ok");
  return g_fails ? 1 : 0;
}
