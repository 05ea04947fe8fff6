// Known-answer tests of the mesh rebuild's index arithmetic (csrc/mcpt_rebuild_plan.h) on the CPU:
// range bounds against kd_build's bounds vectors (restated here: every range halved at
// mid = (lo + hi) / 2, round by round), the range of a position, the leaf pairs and the float key map.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mcpt_rebuild_plan.h"

namespace rb = mcpt::rebuild;

static int g_fails = 0, g_case_fails = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_case_fails < 10) std::printf("  line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_case_fails;                                                      \
    }                                                                      \
  } while (0)
static void done(const char* name) {
  std::printf("%s: %s\n", name, g_case_fails ? "FAIL" : "ok");
  g_fails += g_case_fails;
  g_case_fails = 0;
}

// kd_build's loop: the bounds after each round
static std::vector<std::vector<int>> kd_bounds(int n, int rounds) {
  std::vector<std::vector<int>> all;
  std::vector<int> bounds{0, n}, next;
  all.push_back(bounds);
  for (int r = 0; r < rounds; ++r) {
    next.assign(1, bounds[0]);
    for (size_t s = 1; s < bounds.size(); ++s) {
      long long lo = bounds[s - 1], hi = bounds[s], mid = (lo + hi) / 2;
      next.push_back((int)mid);
      next.push_back((int)hi);
    }
    bounds.swap(next);
    all.push_back(bounds);
  }
  return all;
}

static std::vector<int> sizes() {
  std::vector<int> ns;
  for (int n = 1; n <= 1100; ++n) ns.push_back(n);
  for (int n : {(1 << 17) - 1, 1 << 17, (1 << 17) + 1, 140000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 998000}) ns.push_back(n);
  return ns;
}

static void test_depth() {
  CHECK(rb::depth_of(1) == 0 && rb::depth_of(2) == 1 && rb::depth_of(3) == 2 && rb::depth_of(4) == 2 && rb::depth_of(5) == 3);
  for (int n : sizes()) CHECK(rb::depth_of(n) == (int)std::ceil(std::log2((float)n)));   // kd_build's expression
  done("depth");
}

static void test_bounds() {
  for (int n : sizes()) {
    const int depth = rb::depth_of(n);
    const auto all = kd_bounds(n, depth > 0 ? depth - 1 : 0);
    const bool every_round = n <= 1100;
    for (int r = every_round ? 0 : (int)all.size() - 1; r < (int)all.size(); ++r) {
      const std::vector<int>& b = all[r];
      CHECK((int)b.size() == (1 << r) + 1);
      for (int s = 0; s < (1 << r); ++s) {
        int lo = -1, hi = -1;
        rb::range_bounds(n, r, s, lo, hi);
        CHECK(lo == b[s] && hi == b[s + 1]);
      }
    }
  }
  done("bounds");
}

static void test_range_of() {
  for (int n : sizes()) {
    const int depth = rb::depth_of(n);
    const int last = depth > 0 ? depth - 1 : 0;
    const bool every = n <= 1100;
    for (int r = every ? 0 : last; r <= last; ++r) {
      const int step = every ? 1 : 997;
      for (int pos = 0; pos < n; pos += step) {
        const int s = rb::range_of(n, r, pos);
        int lo, hi;
        rb::range_bounds(n, r, s, lo, hi);
        CHECK(s >= 0 && s < (1 << r) && lo <= pos && pos < hi);
      }
      CHECK(rb::range_of(n, r, n - 1) == (1 << r) - 1 && rb::range_of(n, r, 0) == 0);
    }
  }
  done("range_of");
}

static void test_leaf_pairs() {
  for (int n : sizes()) {
    if (n < 2) continue;
    const int depth = rb::depth_of(n);
    long long items = 0;
    int expect_first = 0;
    for (int s = 0; s < (1 << (depth - 1)); ++s) {
      int lo, hi, first, second;
      rb::range_bounds(n, depth - 1, s, lo, hi);
      CHECK(hi - lo == 1 || hi - lo == 2);   // every last-round range has one or two items
      rb::leaf_pair(n, depth, s, first, second);
      CHECK(first == lo && first == expect_first);
      CHECK(second == (hi - lo == 2 ? lo + 1 : -1));
      items += hi - lo;
      expect_first = hi;
    }
    CHECK(items == n);
  }
  done("leaf_pairs");
}

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static void test_float_key() {
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float> fs = {-inf, -3.4028235e38f, -1.0e10f, -2.5f, -1.0f, -0.5f, -1.1754944e-38f, from_bits(0x807fffffu),
                           from_bits(0x80000002u), from_bits(0x80000001u), -0.0f, 0.0f, from_bits(1u), from_bits(2u),
                           from_bits(0x007fffffu), 1.1754944e-38f, 0.5f, 1.0f, 1.0000001f, 2.5f, 1.0e10f, 3.4028235e38f, inf};
  for (uint32_t k = 0; k < 4000; ++k) {   // a spread of bit patterns of both signs (no NaNs)
    const uint32_t u = k * 1068397u;
    if ((u & 0x7f800000u) != 0x7f800000u) fs.push_back(from_bits(u));
  }
  for (float a : fs)
    for (float b : fs) {
      const uint32_t ka = rb::float_key(a), kb = rb::float_key(b);
      CHECK((a < b) == (ka < kb));     // monotone, and equal floats share a key
      CHECK((a == b) == (ka == kb));
    }
  CHECK(rb::float_key(-0.0f) == rb::float_key(0.0f));
  CHECK(rb::float_key(from_bits(0x80000001u)) < rb::float_key(0.0f) && rb::float_key(0.0f) < rb::float_key(from_bits(1u)));
  done("float_key");
}

int main() {
  test_depth();
  test_bounds();
  test_range_of();
  test_leaf_pairs();
  test_float_key();
  return g_fails ? 1 : 0;
}
