// mcpt_rebuild_plan.h — the index arithmetic of a mesh BVH rebuild, shared by the
// host specification (mcpt_scene.cpp: kd_build_stable) and the device sort (mcpt_rebuild.hip), and
// plain enough to be tested without a GPU (tests/cpp/rebuild_plan_test.cpp).
//
// kd_build halves [0, n) round by round at mid = (lo + hi) / 2: after r rounds there are 2^r ranges,
// and range s is reached from [0, n) by s's bits, most significant first (a set bit: the upper
// half).  A position never leaves its range, so the range is a function of the position alone.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCPT_RP_HD __host__ __device__ inline
#else
#define MCPT_RP_HD inline
#endif

namespace mcpt {
namespace rebuild {

// kd_build's depth: ceil(log2 n) (n >= 1); n_leaf = 2^depth, depth - 1 rounds of splits
MCPT_RP_HD int depth_of(int n) {
  int d = 0;
  while (((int64_t)1 << d) < n) ++d;
  return d;
}

// [lo, hi) of range s (0 .. 2^r - 1) after r rounds over n items
MCPT_RP_HD void range_bounds(int n, int r, int s, int& lo, int& hi) {
  int64_t a = 0, b = n;
  for (int bit = r - 1; bit >= 0; --bit) {
    const int64_t mid = (a + b) / 2;
    if ((s >> bit) & 1) a = mid; else b = mid;
  }
  lo = (int)a; hi = (int)b;
}

// the range (after r rounds over n items) that position pos (0 .. n - 1) lies in
MCPT_RP_HD int range_of(int n, int r, int pos) {
  int64_t a = 0, b = n;
  int s = 0;
  for (int k = 0; k < r; ++k) {
    const int64_t mid = (a + b) / 2;
    s *= 2;
    if (pos >= mid) { a = mid; s += 1; } else b = mid;
  }
  return s;
}

// the leaf pair of range s of the last round (r = depth - 1): leaves 2s and 2s + 1 hold the items
// at first and second (second = -1: a range of one, the right leaf stays empty)
MCPT_RP_HD void leaf_pair(int n, int depth, int s, int& first, int& second) {
  int lo, hi;
  range_bounds(n, depth - 1, s, lo, hi);
  first = lo;
  second = hi - lo >= 2 ? lo + 1 : -1;
}

// float -> uint32 whose unsigned order is the floats' `<` order; -0.0f and +0.0f share a key (they
// compare equal).  NaNs are not ordered by `<`: none reaches a build (the vertices are finite).
MCPT_RP_HD uint32_t float_key(float f) {
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(f);
#else
  std::memcpy(&u, &f, 4);
#endif
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace rebuild
}  // namespace mcpt
