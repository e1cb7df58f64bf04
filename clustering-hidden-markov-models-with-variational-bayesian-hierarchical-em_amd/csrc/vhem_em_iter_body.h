// vhem_em_iter_body.h -- the M-step and the next E-step constants of one (cluster k,
// state s) of one VHEM EM trial, one function for the host and the device.
//
// vhem_ks_body builds, from the trial's packed statistics (include/vbhem_estep.h, VHEM
// mode: Nj | N1 = new_prior | M = new_A | LogL 0 | U = Nr, Y, SC), what vhem.hem_mstep
// (hem_mstep_component.m:123-166) and host.vhem_cluster_constants form for (k, s):
//   prior[k][s], row s of A (with the S == 1 and tau == 1 substitutions of 1e-12),
//   emit_vcounts[k][s], the centre, the covariance plus reg_cov (full | diagonal);
//   logA row, logPi, m, P = inv(cov) | 1 / cov, c = log det cov | sum log cov;
//   and once per cluster (state 0) omega = Nj / Kb and logOmega = log omega.
// In prelude mode (a.stats == nullptr) the constants are those of the parameters GIVEN
// in the trial's arrays, which stay as they are.  Every sum over states follows numpy's
// order (np_sum below), the rest the expression order of hem_mstep.
//
// It returns the FALLBACK flag of (k, s), nonzero when the host engine has to take the
// trial: the new omega[k] == 0 or emit_vcounts[k][s] == 0 (the host's tests in
// vhem._apply_fixes; both are sums of non-negative terms, so the test does not depend
// on the summation order), or a new constant that is not finite other than a logA /
// logPi of -inf.  In prelude mode a logOmega of -inf passes too (the E-step takes it:
// Z = 0 exactly).
//
// The function is written once over a "wave" W: on the device the 64 lanes of a
// wavefront with the wave-private LDS elimination of vbhem_em_iter_body.h
// (gauss_jordan: no pivoting, the covariances are symmetric positive definite); on the
// host one lane and the same elimination entry by entry.  No lane reads what another
// lane stored to global memory: a value two lanes need is computed by both.  Internal.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#include "vbhem_em_iter_body.h"  // gauss_jordan, wsync, kWaves (arithmetic unchanged)
#define VHEM_BODY_HD __host__ __device__
#else
#define VHEM_BODY_HD
#endif

namespace vhem {

constexpr int kBodyMaxD = 16;  // d and S limit of the body (the elimination's)

// what one trial's (k, s) work reads and writes; every pointer addresses the trial
struct KsArgs {
  int K, S, d, covmode, NU;  // covmode 1: full; NU: doubles per (k, s) of U
  int Kb, tau;               // base HMMs (omega = Nj / Kb); tau == 1 substitutes A
  double reg_cov;
  const double *stats;  // nullptr: prelude of the given parameters
  // parameters (M-step outputs; prelude inputs)
  double *omega, *prior, *A, *centres, *covars, *vcounts;
  // E-step constants
  double *logA, *logPi, *cm, *P, *c, *logOmega;
};

// numpy's sum of n <= 16 doubles (pairwise_sum: below 8 a plain loop, else eight running
// sums over blocks of 8, combined as a tree, the rest added in order)
VHEM_BODY_HD inline double np_sum(const double *a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  for (int q = 0; q < 8; ++q) r[q] = a[q];
  int i = 8;
  for (; i + 8 <= n; i += 8)
    for (int q = 0; q < 8; ++q) r[q] += a[i + q];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

VHEM_BODY_HD inline bool is_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }
// finite, or the -inf a log of an exact zero gives
VHEM_BODY_HD inline bool log_ok(double x) { return is_finite(x) || x < 0; }

// ---- the host's wave: one lane; the elimination of vbhem_em_iter_body.h's gauss_jordan
// restated entry by entry (same pivots, same fma, every entry of a step computed from
// the matrix before the step) ----
struct HostWave {
  static constexpr int lanes = 1;
  int lane = 0;
  void sync() const {}
  bool any(bool b) const { return b; }
  double gauss_jordan(double *g, int d, int cols) const {
    const int w2 = 2 * d;
    double nv[2 * kBodyMaxD * kBodyMaxD];
    double det = 1.0;
    for (int k = 0; k < d; ++k) {
      const double piv = g[k * w2 + k], rp = 1.0 / piv;
      for (int r = 0; r < d; ++r)
        for (int c = 0; c < cols; ++c) {
          const double rk = g[k * w2 + c] * rp;
          nv[r * cols + c] = r == k ? rk : std::fma(-g[r * w2 + k], rk, g[r * w2 + c]);
        }
      det *= piv;
      for (int r = 0; r < d; ++r)
        for (int c = 0; c < cols; ++c) g[r * w2 + c] = nv[r * cols + c];
    }
    return det;
  }
};

#if defined(__HIPCC__)
struct DevWave {
  static constexpr int lanes = 64;
  int lane;
  __device__ void sync() const { vbhem::wsync(); }
  __device__ bool any(bool b) const { return __any(b) != 0; }
  __device__ double gauss_jordan(double *g, int d, int cols) const {
    return vbhem::gauss_jordan(g, d, cols, lane);
  }
};
#endif

// entry (r, c) of the new covariance of the (k, s) whose U block is u = Nr | Y | SC
// (hem_mstep_component.m:141-166 as vhem.hem_mstep writes it), reg_cov included
VHEM_BODY_HD inline double cov_entry(const double *u, int d, bool full, double reg, int r, int c) {
  const double wgt = u[0];
  const double *Y = u + 1, *SC = u + 1 + d;
  if (full) {
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    const double cr = Y[r] / wgt, cc = Y[c] / wgt;
    const double sc = SC[lo * d - lo * (lo - 1) / 2 + (hi - lo)];
    const double Sigma = sc - Y[r] * cc - Y[c] * cr + wgt * (cr * cc);
    return Sigma / wgt + (r == c ? reg : 0.0);
  }
  const double cx = Y[r] / wgt;
  const double Sigma = SC[r] - 2 * (Y[r] * cx) + (cx * cx) * wgt;
  return Sigma / wgt + reg;
}

// The work of one wave for cluster state ks = k S + s.  g: 2 d d doubles private to the
// wave.  Returns the fallback flag of (k, s), the same value in every lane.
template <class W>
VHEM_BODY_HD inline int vhem_ks_body(const KsArgs &a, const int ks, const W &w, double *g) {
  const int K = a.K, S = a.S, d = a.d, lane = w.lane;
  const int k = ks / S, s = ks - k * S;
  const bool full = a.covmode == 1, mstep = a.stats != nullptr;
  const int dd = full ? d * d : d, w2 = 2 * d;
  bool bad = false;
  double *Arow = a.A + (size_t)ks * S, *cen = a.centres + (size_t)ks * d;
  double *cov = a.covars + (size_t)ks * dd;
  // packed statistics: Nj | N1 | M | LogL 0 | U
  const double *Nj = a.stats, *N1 = nullptr, *M = nullptr, *u = nullptr;
  double prior, omega = 1.0, rowsum = 1.0;
  const bool oneA = S == 1 || a.tau == 1;  // hem_mstep_component.m:124, :129

  if (mstep) {
    N1 = Nj + K;
    M = N1 + (size_t)K * S;
    u = M + (size_t)K * S * S + 2 + (size_t)ks * a.NU;
    // prior, the row's sum and the counts: sums of <= 16 terms, every lane the same
    prior = N1[ks] / np_sum(N1 + (size_t)k * S, S);
    rowsum = oneA ? 1e-12 : np_sum(M + (size_t)ks * S, S);
    double colsum = 0.0;  // new_A.sum(1): down the column, row by row
    if (oneA) colsum = 1e-12;
    else for (int q = 0; q < S; ++q) colsum += M[((size_t)k * S + q) * S + s];
    const double vc = colsum + N1[ks];
    bad |= vc == 0.0;
    if (lane == 0) {
      a.prior[ks] = prior;
      a.vcounts[ks] = vc;
    }
    if (s == 0) {
      omega = Nj[k] / a.Kb;  // hem_h3m_c_step.m:430
      bad |= omega == 0.0;
      if (lane == 0) a.omega[k] = omega;
    }
  } else {
    prior = a.prior[ks];
    if (s == 0) omega = a.omega[k];
  }

  // ---- A row, centre, prior and omega with their constants ----
  for (int x = lane; x < S; x += W::lanes) {
    double av;
    if (mstep) {
      av = (oneA ? (x == s ? 1e-12 : 0.0) : M[(size_t)ks * S + x]) / rowsum;
      Arow[x] = av;
    } else {
      av = Arow[x];
    }
    const double la = log(av);
    a.logA[(size_t)ks * S + x] = la;
    bad |= !log_ok(la);
  }
  for (int x = lane; x < d; x += W::lanes) {
    double m;
    if (mstep) {
      m = u[1 + x] / u[0];
      cen[x] = m;
    } else {
      m = cen[x];
    }
    a.cm[(size_t)ks * d + x] = m;
    bad |= !is_finite(m);
  }
  {
    const double lp = log(prior);
    bad |= !log_ok(lp);
    if (lane == 0) a.logPi[ks] = lp;
  }
  if (s == 0) {
    const double lo = log(omega);
    bad |= mstep ? !is_finite(lo) : !log_ok(lo);
    if (lane == 0) a.logOmega[k] = lo;
  }

  // ---- covariance, P and c ----
  double c;
  if (full) {
    // [cov | I] -> [I | inv(cov)], det = the product of the pivots
    for (int x = lane; x < d * w2; x += W::lanes) {
      const int r = x / w2, q = x - r * w2;
      double v;
      if (q < d) {
        v = mstep ? cov_entry(u, d, true, a.reg_cov, r, q) : cov[r * d + q];
        if (mstep) cov[r * d + q] = v;
      } else {
        v = q - d == r ? 1.0 : 0.0;
      }
      g[x] = v;
    }
    w.sync();
    const double det = w.gauss_jordan(g, d, w2);
    c = log(det);
    for (int x = lane; x < dd; x += W::lanes) {
      const int r = x / d, q = x - r * d;
      const double p = g[r * w2 + d + q];
      a.P[(size_t)ks * dd + x] = p;
      bad |= !is_finite(p);
    }
  } else {
    double lg[kBodyMaxD];  // np.log(cov).sum(-1): numpy's order again, every lane the same
    for (int x = 0; x < kBodyMaxD; ++x)
      lg[x] = x < d ? log(mstep ? cov_entry(u, d, false, a.reg_cov, x, x) : cov[x]) : 0.0;
    c = np_sum(lg, d);
    for (int x = lane; x < d; x += W::lanes) {
      const double v = mstep ? cov_entry(u, d, false, a.reg_cov, x, x) : cov[x];
      if (mstep) cov[x] = v;
      const double p = 1.0 / v;
      a.P[(size_t)ks * dd + x] = p;
      bad |= !is_finite(p);
    }
  }
  bad |= !is_finite(c);
  if (lane == 0) a.c[ks] = c;
  return w.any(bad) ? 1 : 0;
}

}  // namespace vhem
