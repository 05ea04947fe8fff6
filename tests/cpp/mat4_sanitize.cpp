// mat4_sanitize — the 4x4 inverse behind mcpt_mat4_inverse (csrc/mcpt_mat4.h) as a stand-alone
// program, built with -fsanitize=address,undefined by tests/test_temporal_orbit_counts.py: regular,
// ill-conditioned, singular, non-finite and overflowing inputs, and out aliasing the input.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../montecarlo-pathtracing_amd/csrc/mcpt_mat4.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s\n", what);
    ++failures;
  }
}

// |a * b - I| at most tol, in double
bool is_inverse(const float* a, const float* b, double tol) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += (double)a[k * 4 + r] * (double)b[c * 4 + k];
      if (!(std::fabs(s - (r == c ? 1.0 : 0.0)) <= tol)) return false;
    }
  return true;
}

unsigned lcg(unsigned& s) { return s = s * 1664525u + 1013904223u; }

}  // namespace

int main() {
  using mcpt::host::mat4_inverse;
  float out[16], keep[16];
  unsigned seed = 12345u;
  int inverted = 0;
  for (int n = 0; n < 2000; ++n) {
    float a[16];
    for (float& v : a) v = (float)((int)(lcg(seed) >> 8) % 2001 - 1000) / 250.0f;
    for (int i = 0; i < 16; ++i) out[i] = keep[i] = -7.0f;
    if (mat4_inverse(a, out)) {
      ++inverted;
      float scale = 0.0f;
      for (float v : out) scale = std::fmax(scale, std::fabs(v));
      expect(is_inverse(a, out, 1e-4 * (1.0 + scale) * 8.0), "random matrix: a * inverse(a) = I");
    } else {
      expect(std::memcmp(out, keep, sizeof(out)) == 0, "a refusal leaves out untouched");
    }
  }
  expect(inverted > 1900, "random matrices are regular");
  // a perspective-like matrix (the shape of a camera's P*V) and its round trip
  const float pv[16] = {1.3f, 0.0f, 0.0f, 0.0f, 0.0f, 0.4f, -0.98f, -0.98f, 0.0f, 2.3f, 0.17f, 0.17f, 10.0f, -20.0f, 140.0f, 145.0f};
  float inv[16], back[16];
  expect(mat4_inverse(pv, inv) && mat4_inverse(inv, back), "perspective matrix and its inverse are regular");
  for (int i = 0; i < 16; ++i) expect(std::fabs(back[i] - pv[i]) <= 1e-3f * (1.0f + std::fabs(pv[i])), "round trip");
  // in place
  float io[16];
  std::memcpy(io, pv, sizeof(io));
  expect(mat4_inverse(io, io) && std::memcmp(io, inv, sizeof(io)) == 0, "out may alias the input");
  // refused: zero, two equal rows, a zero column, NaN, inf, a determinant that underflows or overflows
  float bad[7][16];
  std::memset(bad, 0, sizeof(bad));
  for (int i = 0; i < 16; ++i) bad[1][i] = (float)(i * 7 % 11 + 1);
  for (int c = 0; c < 4; ++c) bad[1][c * 4 + 2] = bad[1][c * 4 + 1];
  for (int i = 0; i < 16; ++i) bad[2][i] = i % 4 == 3 ? 0.0f : (float)(i * i % 7 + 1);
  for (int k = 3; k < 7; ++k) bad[k][0] = bad[k][5] = bad[k][10] = bad[k][15] = 1.0f;
  bad[3][6] = std::numeric_limits<float>::quiet_NaN();
  bad[4][9] = std::numeric_limits<float>::infinity();
  for (int d = 0; d < 16; d += 5) bad[5][d] = 1e-39f;        // determinant 1e-156 in double: the inverse overflows binary32
  for (int d = 0; d < 16; d += 5) bad[6][d] = 3e38f;         // determinant 8e153, finite in double: the inverse is tiny, allowed
  for (int k = 0; k < 6; ++k) {
    for (int i = 0; i < 16; ++i) out[i] = keep[i] = -7.0f;
    expect(!mat4_inverse(bad[k], out), "singular, non-finite or overflowing input is refused");
    expect(std::memcmp(out, keep, sizeof(out)) == 0, "a refusal leaves out untouched");
  }
  expect(mat4_inverse(bad[6], out) && std::isfinite(out[0]) && out[1] == 0.0f, "a huge regular matrix inverts to small finite values");
  if (failures) return 1;
  std::printf("mat4_sanitize ok (%d inverted)\n", inverted);
  return 0;
}
