// vbhmm_gmm_run.h -- the arithmetic of one random-start GMM fit (include/vbhmm_gmm.h),
// written once for the device kernel (vbhmm_gmm.hip) and for a host build
// (tests/gmmcheck, and any C++ compiler: nothing here needs a device compiler).  A fit is
// one (subject, K, K start rows, reg); it restates vbhmm_em.py gmm_fit_randsample in the
// order of its steps:
//   start     means = K rows of X, proportions 1/K, every covariance diag(var(X, ddof=1))
//   factor    per state: L = chol(cov_k + reg I), sum log L_ii; a pivot that is not > 0
//             (NaN included) ends the fit as ill-conditioned (numpy raises LinAlgError)
//   E-step    per observation: logp_k = log pi_k - 1/2 |L^-1 (x - mu_k)|^2 - sum log L_ii
//             - dim/2 log 2 pi, the row log-sum-exp with its max, the responsibilities
//             (parked in the fit's workspace)
//   M-step    nk, pi, mu, then the CENTRED second moment about the new mu (a second
//             pass) + reg I, every sum over the observations in index order
//   stop      |ll - last| <= tolfun |ll| after the update, last = -inf at the start
// and the initial VB-HMM posterior of the fitted GMM (vbhmm_init.m:122-204) in the packed
// layout of include/vbhmm_em.h, its W by the Cholesky-based inverse of vbhmm_em_run.h.
//
// The units are one STATE (factor_state, init_posterior_state), one OBSERVATION
// (estep_obs) and one statistic ENTRY (start_var, stat_*).  Which units run in which
// order, when the loop ends and what an ill-conditioned fit leaves unwritten is run_fit
// below, written once: the device kernel walks it with a unit per lane, run_serial with
// plain loops (the lane policies of vbhmm_em_run.h).  Both read and write the same
// Fit<KM> (LDS on the device).
//
// Padding: a fit has K <= KM own states; every loop runs over K, so a fit's result does
// not depend on KM.  log(0) = -inf proportions, zero covariances and NaN flow through to
// the failing pivot of the next factor step; every loop is bounded by max_iter, N, K or
// dim whatever the values are.
#pragma once
#include <cmath>

#include "vbhmm_em_run.h"

// No fused multiply-add in the routines below.  Whether a collapsing component (a state
// left with one or two observations: a covariance of rank < dim) ends the fit at a pivot
// that is not > 0 is decided by the roundings of the M-step sums and of the pivot itself;
// the host fit rounds every product, so the device must too, or such a fit ends
// ill-conditioned on one side and converges on the other.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vbhem {
namespace gmmrun {

using emrun::kMaxDim;
using emrun::kMaxStates;
using emrun::Hyper;

// status of a fit (include/vbhmm_gmm.h)
constexpr int kConverged = 0, kMaxIter = 1, kIllConditioned = 2, kBadFit = 3;

// Per-observation doubles of a fit's workspace: the responsibilities KM and the row lse
VBE_HD constexpr int obs_len(int KM) { return KM + 1; }

// Everything of one fit that is not per observation.
template <int KM>
struct Fit {
  int K, dim, N;
  double reg;
  double pi[KM], mu[KM * kMaxDim], cov[KM * kMaxDim * kMaxDim];
  double L[KM * kMaxDim * kMaxDim];  // the factors; scratch of the initial posterior's W
  double hl[KM];                     // sum log L_ii
  double nk[KM], var[kMaxDim];
  int bad[KM];                       // a failed pivot of state k
  double ll, last;
  int flags;  // loop control of the current iteration: 1 break, 2 converged
};

// A fit's workspace.
struct Work {
  double *post;  // [N][KM]
  double *lse;   // [N]
};

// A fit the routines can run: 2 <= K <= KM, K < N <= max_obs, every start row inside the
// subject.  (Subject range and the subject's rows are the caller's to check first.)
VBE_HD inline bool fit_valid(int K, int KM, int N, int max_obs, const int *rows) {
  if (K < 2 || K > KM || N <= K || N > max_obs) return false;
  for (int k = 0; k < K; ++k)
    if (rows[k] < 0 || rows[k] >= N) return false;
  return true;
}

// ---- start: the variance of coordinate a over the N rows of x (ddof = 1)
template <int KM>
VBE_HD inline void start_var(Fit<KM> &f, const double *x, int a) {
  const int N = f.N, dim = f.dim;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s += x[(size_t)n * dim + a];
  const double mean = s / N;
  double q = 0.0;
  for (int n = 0; n < N; ++n) {
    const double d = x[(size_t)n * dim + a] - mean;
    q += d * d;
  }
  f.var[a] = q / (N - 1);
}

template <int KM>
VBE_HD inline void start_mean(Fit<KM> &f, const double *x, const int *rows, int k, int a) {
  f.mu[k * f.dim + a] = x[(size_t)rows[k] * f.dim + a];
  if (a == 0) f.pi[k] = 1.0 / f.K;
}

template <int KM>
VBE_HD inline void start_cov(Fit<KM> &f, int k, int a, int b) {
  f.cov[(k * f.dim + a) * f.dim + b] = a == b ? f.var[a] : 0.0;
}

// ---- factor of state k: L = chol(cov_k + reg I) into f.L, sum log L_ii into f.hl.  A
// pivot that is not > 0 sets f.bad[k] and leaves the rest of the factor unwritten.
template <int KM>
VBE_HD inline void factor_state(Fit<KM> &f, int k) {
  const int d = f.dim;
  double *a = f.L + k * d * d;
  const double *c = f.cov + k * d * d;
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) a[i * d + j] = c[i * d + j] + (i == j ? f.reg : 0.0);
  double hl = 0.0;
  int bad = 0;
  for (int j = 0; j < d && !bad; ++j) {
    double s = a[j * d + j];
    for (int q = 0; q < j; ++q) s -= a[j * d + q] * a[j * d + q];
    if (!(s > 0.0)) {
      bad = 1;
      break;
    }
    const double ljj = sqrt(s);
    a[j * d + j] = ljj;
    hl += log(ljj);
    for (int i = j + 1; i < d; ++i) {
      double t = a[i * d + j];
      for (int q = 0; q < j; ++q) t -= a[i * d + q] * a[j * d + q];
      a[i * d + j] = t / ljj;
    }
  }
  f.hl[k] = hl;
  f.bad[k] = bad;
}

template <int KM>
VBE_HD inline bool any_bad(const Fit<KM> &f) {
  int bad = 0;
  for (int k = 0; k < f.K; ++k) bad |= f.bad[k];
  return bad != 0;
}

// ---- E-step of one observation xn [dim]: its responsibilities prow [KM] and row lse.
// The loops are unrolled over the compile-time limits and guarded, so that z and logp
// stay in registers.
template <int KM>
VBE_HD inline void estep_obs(const Fit<KM> &f, const double *xn, double *prow, double *lse_out) {
  const int K = f.K, dim = f.dim;
  const double cden = 0.5 * dim * emrun::kLn2Pi;
  double lp[KM];
VBE_UNROLL
  for (int k = 0; k < KM; ++k) {
    lp[k] = 0.0;
    if (k < K) {
      const double *L = f.L + k * dim * dim, *mu = f.mu + k * dim;
      double z[kMaxDim];
      double q = 0.0;
VBE_UNROLL
      for (int i = 0; i < kMaxDim; ++i) {
        z[i] = 0.0;
        if (i < dim) {
          double t = xn[i] - mu[i];
VBE_UNROLL
          for (int j = 0; j < i; ++j) t -= L[i * dim + j] * z[j];
          z[i] = t / L[i * dim + i];
          q += z[i] * z[i];
        }
      }
      lp[k] = log(f.pi[k]) - 0.5 * q - f.hl[k] - cden;
    }
  }
  double mx = lp[0];
VBE_UNROLL
  for (int k = 1; k < KM; ++k)
    if (k < K && (lp[k] > mx || lp[k] != lp[k])) mx = lp[k];  // a NaN stays, as numpy's max
  double se = 0.0;
VBE_UNROLL
  for (int k = 0; k < KM; ++k)
    if (k < K) se += exp(lp[k] - mx);
  const double lse = mx + log(se);
VBE_UNROLL
  for (int k = 0; k < KM; ++k)
    if (k < K) prow[k] = exp(lp[k] - lse);
  *lse_out = lse;
}

// ---- the log-likelihood: the row lse in index order
template <int KM>
VBE_HD inline void stat_ll(Fit<KM> &f, const Work &w) {
  double acc = 0.0;
  for (int n = 0; n < f.N; ++n) acc += w.lse[n];
  f.ll = acc;
}

// ---- M-step, one entry each; x = the subject's first row
template <int KM>
VBE_HD inline void stat_nk(Fit<KM> &f, const Work &w, int k) {
  double acc = 0.0;
  for (int n = 0; n < f.N; ++n) acc += w.post[(size_t)n * KM + k];
  acc += 1e-300;
  f.nk[k] = acc;
  f.pi[k] = acc / f.N;
}

template <int KM>
VBE_HD inline void stat_mean(Fit<KM> &f, const double *x, const Work &w, int k, int a) {
  const int dim = f.dim;
  double acc = 0.0;
  for (int n = 0; n < f.N; ++n) acc += w.post[(size_t)n * KM + k] * x[(size_t)n * dim + a];
  f.mu[k * dim + a] = acc / f.nk[k];
}

// p (d_a d_b): the same bits for (a, b) and (b, a), so (C + C') / 2 changes nothing
template <int KM>
VBE_HD inline void stat_cov(Fit<KM> &f, const double *x, const Work &w, int k, int a, int b) {
  const int dim = f.dim;
  const double ma = f.mu[k * dim + a], mb = f.mu[k * dim + b];
  double acc = 0.0;
  for (int n = 0; n < f.N; ++n)
    acc += w.post[(size_t)n * KM + k] * ((x[(size_t)n * dim + a] - ma) * (x[(size_t)n * dim + b] - mb));
  f.cov[(k * dim + a) * dim + b] = acc / f.nk[k] + (a == b ? f.reg : 0.0);
}

// ---- loop control of iteration `it`, after the update.  Sets f.last, f.flags.
template <int KM>
VBE_HD inline void loop_control(Fit<KM> &f, int it, int max_iter, double tolfun) {
  int fl = 0;
  if (fabs(f.ll - f.last) <= tolfun * fabs(f.ll)) fl = 1 | 2;
  else if (it == max_iter) fl = 1;
  f.last = f.ll;
  f.flags = fl;
}

VBE_HD inline int status_of(int flags) { return (flags & 2) ? kConverged : kMaxIter; }

// ---- padding of a packed posterior (vbhmm_em.py pack_posterior): alpha, epsilon, beta, v
// with 1, m with 0, W with I; entry q of post [post_len(KM, dim)]
VBE_HD inline double post_padding(int KM, int dim, int q) {
  const int w0 = 3 * KM + KM * KM + KM * dim;
  if (q < 3 * KM + KM * KM) return 1.0;
  if (q < w0) return 0.0;
  const int e = (q - w0) % (dim * dim);
  return e / dim == e % dim ? 1.0 : 0.0;
}

// ---- the initial posterior of state k from the fitted GMM (vbhmm_init.m:122-204) into
// the packed post; W_k is formed and inverted in the state's factor slot f.L.
template <int KM>
VBE_HD inline void init_posterior_state(Fit<KM> &f, const Hyper &h, int k, double *post) {
  const int K = f.K, dim = f.dim;
  const double Nk2 = (double)f.N / K, Nk = f.N * f.pi[k];
  double *alpha = post, *eps = post + KM, *beta = post + KM + KM * KM, *v = beta + KM, *m = v + KM,
         *W = m + KM * dim;
  alpha[k] = h.alpha0 + Nk2;
  for (int j = 0; j < K; ++j) eps[k * KM + j] = h.epsilon0 + Nk2;
  const double bk = h.beta0 + Nk;
  beta[k] = bk;
  v[k] = h.v0 + Nk + 1;
  const double *xb = f.mu + k * dim, *S = f.cov + k * dim * dim;
  double *sc = f.L + k * dim * dim;
  const double mult1 = h.beta0 * Nk / (h.beta0 + Nk);
  for (int a = 0; a < dim; ++a) {
    m[k * dim + a] = (h.beta0 * h.m0[a] + Nk * xb[a]) / bk;
    for (int b = 0; b < dim; ++b)
      sc[a * dim + b] = (a == b ? h.W0inv[a] : 0.0) + Nk * S[a * dim + b] + mult1 * ((xb[a] - h.m0[a]) * (xb[b] - h.m0[b]));
  }
  emrun::spd_inverse_inplace(sc, dim);
  for (int e = 0; e < dim * dim; ++e) W[k * dim * dim + e] = sc[e];
}

// What a fit reports besides its parameters.
struct FitResult {
  double ll;
  int iters, status;
};

// ---- the schedule of one whole fit (emrun's lane policies): the device kernel walks it
// with WaveLanes, run_serial with SerialLanes.  f: the fit's state (LDS on the device),
// filled here; the fit is valid (fit_valid).  x: the subject's first row, N rows.  The
// outputs are this fit's own: prior [KM], mean [KM][dim], cov [KM][dim][dim], rows k < K
// written, and only for a fit that ends converged or at max_iter; lls (or null):
// [max_iter], entries past iters untouched; h / post_init (or null): the packed initial
// posterior, written under the same condition.
template <int KM, class Lanes>
VBE_HD inline FitResult run_fit(const Lanes lanes, Fit<KM> &f, int K, int dim, int N, const double *x,
                                const int *rows, double reg, int max_iter, double tolfun, double *prior,
                                double *mean, double *cov, double *lls, const Hyper *h, double *post_init,
                                const Work &w) {
  if (lanes.first()) {
    f.K = K;
    f.dim = dim;
    f.N = N;
    f.reg = reg;
    f.ll = __builtin_nan("");
    f.last = -INFINITY;
    f.flags = 0;
  }
  lanes.sync();
  lanes.once(dim, [&](int a) { start_var(f, x, a); });
  lanes.once(K * dim, [&](int e) { start_mean(f, x, rows, e / dim, e % dim); });
  lanes.sync();
  lanes.each(K * dim * dim, [&](int e) { start_cov(f, e / (dim * dim), (e / dim) % dim, e % dim); });
  lanes.sync();
  int it = 1;
  bool ill = false;
  for (; it <= max_iter; ++it) {
    lanes.once(K, [&](int k) { factor_state(f, k); });
    lanes.sync();
    if (any_bad(f)) {
      ill = true;
      break;
    }
    lanes.each(N, [&](int n) { estep_obs<KM>(f, x + (size_t)n * dim, w.post + (size_t)n * KM, w.lse + n); });
    lanes.sync();
    lanes.once(K + 1, [&](int k) {
      if (k < K) stat_nk(f, w, k);
      else stat_ll(f, w);
    });
    lanes.sync();
    lanes.once(K * dim, [&](int e) { stat_mean(f, x, w, e / dim, e % dim); });
    lanes.sync();
    lanes.each(K * dim * dim, [&](int e) { stat_cov(f, x, w, e / (dim * dim), (e / dim) % dim, e % dim); });
    if (lanes.first()) {
      loop_control(f, it, max_iter, tolfun);
      if (lls) lls[it - 1] = f.ll;
    }
    lanes.sync();
    if (f.flags & 1) break;
  }
  if (!ill) {
    lanes.once(K, [&](int k) { prior[k] = f.pi[k]; });
    lanes.once(K * dim, [&](int e) { mean[e] = f.mu[e]; });
    lanes.each(K * dim * dim, [&](int e) { cov[e] = f.cov[e]; });
    if (h && post_init) {
      lanes.each(emrun::post_len(KM, dim), [&](int q) { post_init[q] = post_padding(KM, dim, q); });
      lanes.sync();
      lanes.once(K, [&](int k) { init_posterior_state(f, *h, k, post_init); });
    }
  }
  return FitResult{f.ll, it > max_iter ? max_iter : it, ill ? kIllConditioned : status_of(f.flags)};
}

// ---- one whole fit, unit after unit (host builds only): max_obs bounds N as the
// workspace of a device call does.  A fit that is not valid returns kBadFit and writes
// nothing; the rest as run_fit's.
template <int KM>
inline FitResult run_serial(int K, int dim, int N, int max_obs, const double *x, const int *rows, double reg,
                            int max_iter, double tolfun, double *prior, double *mean, double *cov, double *lls,
                            const Hyper *h, double *post_init, const Work &w) {
  if (!fit_valid(K, KM, N, max_obs, rows)) return FitResult{__builtin_nan(""), 0, kBadFit};
  Fit<KM> f;
  return run_fit<KM>(emrun::SerialLanes{}, f, K, dim, N, x, rows, reg, max_iter, tolfun, prior, mean, cov, lls, h,
                     post_init, w);
}

}  // namespace gmmrun
}  // namespace vbhem
