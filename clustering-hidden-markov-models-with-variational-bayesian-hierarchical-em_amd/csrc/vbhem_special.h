// vbhem_special.h -- the special functions of the bounds and preludes, one copy each for
// host and device code (any C++ compiler: nothing here needs a device compiler).
//
// The two digamma forms share the series and differ in how they take the recurrence
// psi(x) = psi(x + n) - sum_{i<n} 1/(x + i) to x + n >= 8, so they differ in the last
// bits and a call site keeps the form it was validated with:
//   psi_recur    one division per step; the VHEM host loop (vbhem_em.hip) and the base
//                set built from learned HMMs (vbhem_h3m.hip)
//   psi_onediv   the sum as ONE division of a running numerator / denominator (fp64
//                division is a long dependent sequence on the GPU); the VHEM device
//                iteration (vbhem_em_dev.hip) and the VB-HMM EM (vbhmm_em_run.h)
//
// Include this header before any `#pragma clang fp contract`: the functions are compiled
// under the translation unit's default contraction, and the fma below is explicit.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBE_HD __host__ __device__
#else
#define VBE_HD
#endif

namespace vbhem {

// the asymptotic expansion ln x - 1/(2x) - sum B_2k / (2k x^2k) without its ln x, x >= 8
VBE_HD inline double psi_series(double r, double r2) {
  return r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 -
         r2 * (691.0 / 32760 - r2 * (1.0 / 12)))))));
}

// digamma for x > 0, the recurrence with one division per step
VBE_HD inline double psi_recur(double x) {
  if (!(x > 0.0 && x < INFINITY)) return x == INFINITY ? x : __builtin_nan("");
  double acc = 0.0;
  while (x < 8.0) {
    acc -= 1.0 / x;
    x += 1.0;
  }
  const double r = 1.0 / x, r2 = r * r;
  const double series = psi_series(r, r2);
  return acc + log(x) - 0.5 * r - series;
}

// digamma for x > 0, the recurrence as one division
VBE_HD inline double psi_onediv(double x) {
  if (!(x > 0.0 && x < INFINITY)) return x == INFINITY ? x : __builtin_nan("");
  double num = 0.0, den = 1.0;
  while (x < 8.0) {  // num / den = sum 1/(x_i) so far
    num = fma(num, x, den);
    den *= x;
    x += 1.0;
  }
  const double r = 1.0 / x, r2 = r * r;
  const double series = psi_series(r, r2);
  return log(x) - 0.5 * r - series - num / den;
}

// log Gamma for x > 0: lgamma(x) = lgamma(x + n) - log(prod_{i<n} (x + i)) with
// z = x + n >= 10, then Stirling's series (z - 1/2) ln z - z + ln(2 pi)/2 +
// sum B_2k / (2k (2k - 1) z^(2k-1)) through z^-15 (next term < 3e-18 at z = 10)
VBE_HD inline double lgamma_stirling(double x) {
  if (!(x > 0.0 && x < INFINITY)) return x == INFINITY ? x : __builtin_nan("");
  double prod = 1.0;
  while (x < 10.0) {
    prod *= x;
    x += 1.0;
  }
  const double r = 1.0 / x, r2 = r * r;
  const double series =
      r * (1.0 / 12 - r2 * (1.0 / 360 - r2 * (1.0 / 1260 - r2 * (1.0 / 1680 - r2 * (1.0 / 1188 -
      r2 * (691.0 / 360360 - r2 * (1.0 / 156 - r2 * (3617.0 / 122400))))))));
  return (x - 0.5) * log(x) - x + 0.91893853320467274178 + series - log(prod);
}

}  // namespace vbhem
