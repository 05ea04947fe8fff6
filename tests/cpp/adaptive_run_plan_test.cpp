// Known-answer tests of a queued adaptive run's schedule (csrc/mcpt_adaptive_run_plan.h) on the CPU:
// which rounds select, the grid that holds the list on entry, and the host loop's outcome from the
// list lengths the selects left.  Every expected value is written next to its assertion, worked out
// from the loop in mcpt.h (mcpt_adaptive_run), not taken from a run.
#include <cstdio>
#include <vector>

#include "mcpt_adaptive_run_plan.h"

namespace plan = mcpt::plan;

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

int main() {
  test_schedule();
  test_outcome();
  test_list_groups();
  std::printf("%s\n", g_fails ? "FAILED" : "all ok");
  return g_fails ? 1 : 0;
}
