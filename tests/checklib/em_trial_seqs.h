// tests/checklib/em_trial_seqs.h -- TEST-ONLY: hand-made bound sequences for the
// stopping rule of one EM trial (csrc/vbhem_em_trial_ctrl.h), shared by the check
// library (tests/emtrialscheck, read by tests/test_em_trials_ctrl.py) and the
// stand-alone sanitizer program (tests/emtrialscheck/walker_main.cpp).  Each has the
// outcome worked out by hand from vbhem_h3m_c_step_fc.m:311-374.
#pragma once
#include <cfloat>
#include <cmath>

namespace emtrialseqs {

constexpr int kMaxLen = 12;

struct Seq {
  const char *name;
  int n;  // bounds given (the trial stops at or before the last)
  double L[kMaxLen];
  int max_iter;
  double minDiff;
  int iters, stable;  // expected
};

constexpr double kTwoM18 = 1.0 / 262144.0, kTwoM20 = 1.0 / 1048576.0;

inline const Seq *table(int *count) {
  static const Seq seqs[] = {
      // relative changes 1e-2, 1e-3, ... : the first <= 1e-6 is at iteration 5
      {"converging", 6, {-1000.0, -990.0, -989.0, -988.9, -988.89, -988.8895}, 40, 1e-6, 6, 1},
      // no change at iteration 1 (not tested: it > 1), exactly minDiff = 2^-20 at 2
      {"exact_at_2", 3, {-4.0, -4.0, -4.0 + kTwoM18}, 40, kTwoM20, 3, 1},
      // 2^-53 above minDiff at iteration 2 (goes on), no change at 3 (stops)
      {"just_above_then_exact", 4, {-4.0, -4.0, -4.0 + kTwoM18 + 2 * DBL_EPSILON,
                                    (-4.0 + kTwoM18 + 2 * DBL_EPSILON)}, 40, kTwoM20, 4, 1},
      {"max_iter_0", 1, {-7.5}, 0, 1e-6, 1, 1},
      {"max_iter_1", 2, {-7.5, -3.25}, 1, 1e-6, 2, 1},
      {"max_iter_5_no_convergence", 6, {-60.0, -50.0, -40.0, -30.0, -20.0, -10.0}, 5, 1e-6, 6, 1},
      {"nan_at_0", 1, {NAN}, 40, 1e-6, 0, 0},
      {"nan_at_3", 4, {-9.0, -8.0, -7.0, NAN}, 40, 1e-6, 3, 0},
      // the first step divides by lastL = -DBL_MAX (and overflows in the numerator)
      {"huge_first", 3, {DBL_MAX, DBL_MAX, DBL_MAX}, 40, 1e-6, 3, 1},
      // lastL = 0: 0 / 0 = NaN and 1 / 0 = inf compare false, the trial goes on
      {"zero_lastL", 5, {-1.0, 0.0, 0.0, 1.0, 1.0}, 40, 1e-6, 5, 1},
      {"inf_bound", 4, {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, 3, 1e-6, 4, 1},
  };
  *count = (int)(sizeof(seqs) / sizeof(seqs[0]));
  return seqs;
}

}  // namespace emtrialseqs
