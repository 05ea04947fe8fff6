// Known-answer tests of the frame gathers' row plan (csrc/mcpt_gather_plan.h) on the CPU: full-frame
// targets, shard sets that hold every frame row once, runs of consecutive rows, source rows of a
// packed buffer.  Every expected value is written next to its assertion, not taken from a run.
#include <cstdio>
#include <vector>

#include "mcpt_gather_plan.h"

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

static bool same_run(const plan::RowRun& r, int local_first, int global_first, int n) {
  return r.local_first == local_first && r.global_first == global_first && r.n == n;
}

static void test_row_runs() {
  CHECK(plan::row_runs({}).empty());
  const std::vector<plan::RowRun> a = plan::row_runs({0, 1, 2, 5, 6, 9});
  CHECK(a.size() == 3 && same_run(a[0], 0, 0, 3) && same_run(a[1], 3, 5, 2) && same_run(a[2], 5, 9, 1));
  const std::vector<plan::RowRun> one = plan::row_runs({7});
  CHECK(one.size() == 1 && same_run(one[0], 0, 7, 1));
  // descending rows are never one copy: local row 1 lies before local row 0 in the frame
  const std::vector<plan::RowRun> down = plan::row_runs({4, 3});
  CHECK(down.size() == 2 && same_run(down[0], 0, 4, 1) && same_run(down[1], 1, 3, 1));
  // a full frame in row order is one run
  const std::vector<plan::RowRun> full = plan::row_runs({0, 1, 2, 3});
  CHECK(full.size() == 1 && same_run(full[0], 0, 0, 4));
  done("row_runs");
}

static void test_is_full_frame() {
  CHECK(plan::is_full_frame({}, 0));
  CHECK(plan::is_full_frame({0, 1, 2}, 3));
  CHECK(!plan::is_full_frame({0, 2, 1}, 3));   // permuted
  CHECK(!plan::is_full_frame({0, 1}, 3));      // short
  CHECK(!plan::is_full_frame({1, 2, 3}, 3));   // the right length, shifted
  CHECK(!plan::is_full_frame({0}, 0));
  done("is_full_frame");
}

// mcpt_balanced_rows' partition of H = 53 with bands of 8 rows among 3 ranks: two whole periods
// (rows 0..47: rank of band b in period j is (b mod 3 - j mod 3) mod 3), then rows 48..52 dealt one
// at a time from rank (0 + 2) mod 3
static const std::vector<int> kRank0 = {0, 1, 2, 3, 4, 5, 6, 7, 32, 33, 34, 35, 36, 37, 38, 39, 49, 52};
static const std::vector<int> kRank1 = {8, 9, 10, 11, 12, 13, 14, 15, 40, 41, 42, 43, 44, 45, 46, 47, 50};
static const std::vector<int> kRank2 = {16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 48, 51};

static bool held_once(const std::vector<const std::vector<int>*>& lists, int H) {
  return plan::rows_held_once(lists.data(), (int)lists.size(), H);
}

static void test_rows_held_once() {
  const int H = 53;
  for (const std::vector<int>* r : {&kRank0, &kRank1, &kRank2}) {   // (the test's own data, for the Python side)
    std::printf("balanced 53 8 3:");
    for (int y : *r) std::printf(" %d", y);
    std::printf("\n");
  }
  CHECK(held_once({&kRank0, &kRank1, &kRank2}, H));
  CHECK(held_once({&kRank2, &kRank0, &kRank1}, H));            // any order of the shards
  CHECK(!held_once({&kRank0, &kRank2}, H));                    // a shard dropped: rows held by none
  CHECK(!held_once({&kRank0, &kRank1, &kRank2, &kRank1}, H));  // a shard twice: rows held twice
  CHECK(!held_once({}, H));
  CHECK(held_once({}, 0));
  // a row outside the frame: refused, and never used as an index
  const std::vector<int> past = {H}, before = {-1}, far = {1 << 30};
  CHECK(!held_once({&kRank0, &kRank1, &kRank2, &past}, H));
  CHECK(!held_once({&kRank0, &kRank1, &kRank2, &before}, H));
  CHECK(!held_once({&far}, H));
  CHECK(!held_once({&before}, 0));
  done("rows_held_once");
}

static void test_src_rows_in_range() {
  const long long src_rows = 36;   // three shards of 18 padded rows
  const int good[4] = {0, 35, 18, 17};
  CHECK(plan::src_rows_in_range(good, 4, src_rows));           // src_rows - 1 is the last row
  const int neg[4] = {0, -1, 18, 17}, past[4] = {0, 35, 36, 17};
  CHECK(!plan::src_rows_in_range(neg, 4, src_rows));
  CHECK(!plan::src_rows_in_range(past, 4, src_rows));
  CHECK(plan::src_rows_in_range(past, 2, src_rows));           // only the first H entries count
  CHECK(plan::src_rows_in_range(nullptr, 0, src_rows));
  CHECK(!plan::src_rows_in_range(good, 1, 0));                 // an empty buffer holds no row
  done("src_rows_in_range");
}

int main() {
  test_row_runs();
  test_is_full_frame();
  test_rows_held_once();
  test_src_rows_in_range();
  std::printf("%s\n", g_fails ? "FAILED" : "all ok");
  return g_fails ? 1 : 0;
}
