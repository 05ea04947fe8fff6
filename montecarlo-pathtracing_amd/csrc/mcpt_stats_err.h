// mcpt_stats_err.h — the per-pixel error arithmetic of DESIGN.md §3.8, shared by the error kernel
// (mcpt_stats.hip) and the adaptive select kernel (mcpt_adaptive.hip; §3.9): one statement of it,
// so both write the same bits.  binary32 without contraction: + - * /, comparisons, sqrt_rn.
#pragma once
#include <hip/hip_runtime.h>

#include "mcpt_math.h"

namespace mcpt {

__device__ __forceinline__ bool finite32(float x) { return __builtin_fabsf(x) < __builtin_inff(); }   // (false for NaN)

// {se, r} of a pixel's statistics state {Yacc, S2, Ybase, 0} over a window of nf passes in
// bm1f + 1 batches; r clamped to 64 (an overflowed pixel counts 64)
__device__ __forceinline__ float2 pixel_error(const float4 s, float nf, float bm1f, float mu_floor) {
  const float s1 = s.x - s.z;
  float v = s.y - (s1 * s1) / nf;
  v = (0.0f < v) ? v : 0.0f;
  const float var = v / bm1f;
  const float se = sqrt_rn(var / nf);
  const float mu = s1 / nf;
  float r = se / (gmax(0.0f, mu) + mu_floor);
  if (!finite32(s.y) || !finite32(s1) || !(r <= 64.0f)) r = 64.0f;
  return make_float2(se, r);
}

// a pixel's share of the frame record: q = trunc(r * 2^16) (r <= 64: q <= 2^22)
__device__ __forceinline__ unsigned error_q(float r) { return (unsigned)(r * 65536.0f); }

}  // namespace mcpt
