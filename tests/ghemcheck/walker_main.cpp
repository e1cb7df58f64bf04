// tests/ghemcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the serial walker of
// csrc/vbhem_ghem_run.h on seeded inputs, for a run under the address and undefined-behaviour
// sanitizers on the CPU (`make ghem_sanitize`; plain C++, no device compiler).  It walks the
// fit at the demo's size, at the limits d = 16, T = 32, at n = T, at a tile edge, with
// diagonal covariances, given centres, iterations = 0 and 1, all-zero covariances
// (SINGULAR), a far centre (NONFINITE), identical points (DEGENERATE), a non-finite
// coordinate and an out-of-range draw (BAD).
#include <cmath>
#include <cstdio>
#include <vector>

#include "ghem_walk.h"
#include "walker_input.h"

using namespace vbhem::ghemrun;
using walker::Lcg;

namespace {

// mode 0: ordinary; 1: every point the same; 2: a NaN coordinate; 3: j0 = n; 4: all-zero
// covariances; 5: given centres, one of them far away; 6: given centres
int one_case(int n, int d, bool full, int T, int iterations, unsigned long long seed, int mode, int want) {
  Lcg g{seed};
  const int cd = cov_len(d, full), R = 2;
  std::vector<double> X((size_t)n * d), C((size_t)n * cd, 0.0);
  for (int m = 0; m < n; ++m) {
    const int z = (int)(g.uni() * T);
    for (int a = 0; a < d; ++a) X[(size_t)m * d + a] = mode == 1 ? 3.0 : 6.0 * z + 2.0 * a + g.normal();
    if (mode == 4) continue;
    for (int a = 0; a < d; ++a) {
      const double v = 0.5 + g.uni();
      C[(size_t)m * cd + (full ? a * d + a : a)] = v;
      if (full && a > 0) C[(size_t)m * cd + a * d + a - 1] = C[(size_t)m * cd + (a - 1) * d + a] = 0.1 * v;
    }
  }
  if (mode == 2) X[(size_t)(n / 2) * d] = NAN;
  std::vector<double> u((size_t)R * (T - 1)), init((size_t)R * T * d);
  std::vector<int> j0(R);
  for (double &v : u) v = g.uni();
  for (int r = 0; r < R; ++r) j0[r] = mode == 3 ? n : (int)(g.uni() * n);
  for (int r = 0; r < R; ++r)
    for (int t = 0; t < T; ++t)
      for (int a = 0; a < d; ++a)
        init[((size_t)r * T + t) * d + a] = mode == 5 && t == 0 ? 1e4 : X[(size_t)((t * 7 + r) % n) * d + a] + 0.01 * t;
  std::vector<double> mx((size_t)R * T, -7.0), cen((size_t)R * T * d, -7.0), cov((size_t)R * T * cd, -7.0),
      lp((size_t)R * T * n, -7.0), logp(R, -7.0);
  std::vector<int> status(R, -7), iters(2 * R, -7);
  ghemwalk::fit_trials(n, d, full, T, R, X.data(), C.data(), 100.0 * n / 3.0, iterations, j0.data(), u.data(),
                       mode >= 5 ? init.data() : nullptr, mx.data(), cen.data(), cov.data(), lp.data(), logp.data(),
                       status.data(), iters.data());
  std::printf("n=%d d=%d full=%d T=%d it=%d mode=%d: status=%d,%d iters=%d,%d logp=%g\n", n, d, (int)full, T, iterations,
              mode, status[0], status[1], iters[0], iters[1], logp[0]);
  int bad = 0;
  for (int r = 0; r < R; ++r) {
    bad += status[r] != want;
    if (status[r] != kOk) {
      bad += !(mx[(size_t)r * T] == -7.0 && cen[(size_t)r * T * d] == -7.0 && lp[(size_t)r * T * n] == -7.0);
      continue;
    }
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += mx[(size_t)r * T + t];
    bad += !(std::fabs(s - 1.0) < 1e-9 && std::isfinite(cen[(size_t)r * T * d]) && iters[2 * r + 1] <= iterations);
  }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  bad += one_case(25, 2, true, 3, 30, 1, 0, kOk);
  bad += one_case(255, 3, false, 2, 30, 2, 0, kOk);
  bad += one_case(257, 8, true, 8, 30, 3, 0, kOk);
  bad += one_case(600, 16, true, 32, 5, 4, 0, kOk);
  bad += one_case(600, 16, false, 32, 5, 5, 0, kOk);
  bad += one_case(4, 2, true, 4, 30, 6, 0, kOk);
  bad += one_case(100, 2, true, 3, 0, 7, 0, kOk);
  bad += one_case(100, 2, false, 3, 1, 8, 0, kOk);
  bad += one_case(100, 2, true, 3, 30, 9, 6, kOk);
  bad += one_case(40, 2, true, 3, 30, 10, 1, kDegenerate);
  bad += one_case(40, 2, true, 3, 30, 11, 2, kBad);
  bad += one_case(40, 2, true, 3, 30, 12, 3, kBad);
  bad += one_case(40, 2, true, 3, 30, 13, 4, kSingular);
  bad += one_case(40, 2, false, 3, 30, 14, 4, kSingular);
  bad += one_case(40, 2, true, 3, 30, 15, 5, kNonfinite);
  std::printf(bad ? "FAILED %d\n" : "walker OK\n", bad);
  return bad != 0;
}
