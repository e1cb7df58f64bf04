// tests/checklib/ghem_walk.h -- TEST-ONLY: the serial walker of csrc/vbhem_ghem_run.h over
// a list of trials with the C ABI's arrays (tests/ghemcheck: the check library and the
// stand-alone program; plain C++, no device compiler).
#pragma once
#include <algorithm>
#include <vector>

#include "vbhem_ghem_run.h"

namespace ghemwalk {

// Outputs of a trial that is not OK keep what the caller put there.  init, logpost: null
// or arrays.
inline void fit_trials(int n, int d, bool full, int T, int R, const double *X, const double *C, double vs,
                       int iterations, const int *j0, const double *u, const double *init, double *mxwt,
                       double *centres, double *covars, double *logpost, double *logp, int *status, int *iters) {
  using namespace vbhem::ghemrun;
  const int cd = cov_len(d, full), nu = std::max(T - 1, 1);
  const size_t big = (size_t)std::max(ea_len(T, d), T * cd);
  std::vector<double> vr0(cd), slot(slot_len(T, d, cd)), post((size_t)T * n), tot(big), part(big), A(cd), B(cd),
      cold((size_t)T * d), sums((size_t)T * (d + 1)), dmin(n);
  std::vector<int> lab(n);
  const bool fin = scan_serial(X, C, n, d, full, vr0.data(), part.data());
  for (int r = 0; r < R; ++r) {
    fit_serial(X, C, n, d, full, T, vs, iterations, init ? 0 : j0[r], init ? nullptr : u + (size_t)r * nu,
               init ? init + (size_t)r * T * d : nullptr, vr0.data(), fin, slot.data(), post.data(), tot.data(),
               part.data(), A.data(), B.data(), cold.data(), sums.data(), dmin.data(), lab.data());
    const Slot s = slot_at(slot.data(), T, d, cd);
    status[r] = s.flag[fStatus];
    if (status[r] != kOk) continue;
    std::copy(s.mx, s.mx + T, mxwt + (size_t)r * T);
    std::copy(s.cen, s.cen + (size_t)T * d, centres + (size_t)r * T * d);
    std::copy(s.vr, s.vr + (size_t)T * cd, covars + (size_t)r * T * cd);
    logp[r] = s.sc[1];
    iters[2 * r] = s.flag[fLloyd];
    iters[2 * r + 1] = s.flag[fEsteps];
    if (logpost) logpost_serial(X, C, n, d, full, T, vs, slot.data(), logpost + (size_t)r * T * n);
  }
}

}  // namespace ghemwalk
