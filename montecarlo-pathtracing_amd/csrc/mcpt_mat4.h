// mcpt_mat4.h — the 4x4 inverse behind mcpt_mat4_inverse (host only, no dependencies: the C ABI
// and tests/cpp/mat4_sanitize.cpp include it).  Cofactors and determinant in double from the 16
// binary32 inputs, the result rounded to binary32 once.  The storage order does not matter: the
// inverse of a transpose is the transpose of the inverse.
#pragma once
#include <cmath>

namespace mcpt {
namespace host {

// false (out untouched): a non-finite input, a zero or non-finite determinant, a non-finite result
inline bool mat4_inverse(const float* a, float* out) {
  double m[16], inv[16];
  for (int i = 0; i < 16; ++i) {
    if (!std::isfinite(a[i])) return false;
    m[i] = (double)a[i];
  }
  // 2x2 minors of the lower two rows and of the upper two rows
  const double s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
  const double s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
  const double c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
  const double c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
  const double det = ((s0 * c5 - s1 * c4) + (s2 * c3 + s3 * c2)) + (s5 * c0 - s4 * c1);
  if (det == 0.0 || !std::isfinite(det)) return false;
  const double id = 1.0 / det;
  inv[0] = ((m[5] * c5 - m[6] * c4) + m[7] * c3) * id;
  inv[1] = ((-m[1] * c5 + m[2] * c4) - m[3] * c3) * id;
  inv[2] = ((m[13] * s5 - m[14] * s4) + m[15] * s3) * id;
  inv[3] = ((-m[9] * s5 + m[10] * s4) - m[11] * s3) * id;
  inv[4] = ((-m[4] * c5 + m[6] * c2) - m[7] * c1) * id;
  inv[5] = ((m[0] * c5 - m[2] * c2) + m[3] * c1) * id;
  inv[6] = ((-m[12] * s5 + m[14] * s2) - m[15] * s1) * id;
  inv[7] = ((m[8] * s5 - m[10] * s2) + m[11] * s1) * id;
  inv[8] = ((m[4] * c4 - m[5] * c2) + m[7] * c0) * id;
  inv[9] = ((-m[0] * c4 + m[1] * c2) - m[3] * c0) * id;
  inv[10] = ((m[12] * s4 - m[13] * s2) + m[15] * s0) * id;
  inv[11] = ((-m[8] * s4 + m[9] * s2) - m[11] * s0) * id;
  inv[12] = ((-m[4] * c3 + m[5] * c1) - m[6] * c0) * id;
  inv[13] = ((m[0] * c3 - m[1] * c1) + m[2] * c0) * id;
  inv[14] = ((-m[12] * s3 + m[13] * s1) - m[14] * s0) * id;
  inv[15] = ((m[8] * s3 - m[9] * s1) + m[10] * s0) * id;
  float r[16];
  for (int i = 0; i < 16; ++i) {
    r[i] = (float)inv[i];
    if (!std::isfinite(r[i])) return false;
  }
  for (int i = 0; i < 16; ++i) out[i] = r[i];
  return true;
}

}  // namespace host
}  // namespace mcpt
