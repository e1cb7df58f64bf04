// vbhem_em_deriv_terms.h -- the arithmetic of the bound's derivatives with respect to
// the hyperparameters (vbhemh3m_lb.m:202-345), one copy for the host and the device:
// trials_derivs_kernel (vbhem_em_trials_derivs.hip) runs it with one wavefront per
// (trial, k, s), the check library tests/emderivcheck runs it on the host.
//
// The raw derivatives, in the order of VBHEM_DLL_LEN (alpha0, eta0, epsilon0, v0,
// lambda0, W0[nW], m0[d]), are each a sum over the cluster states (k, s) of a term of
// the posterior plus a closed form of the hyperparameters alone:
//   alpha0    logOmega_k (state 0 only)        + K psi(K a0) - K psi(a0)
//   eta0      logPi_ks                         + K (S psi(S e0) - S psi(e0))
//   epsilon0  sum_s' logA_ks,s'                + K S (S psi(S ep0) - S psi(ep0))
//   v0        logLambdaTilde_ks / 2            + K S (log det W0^-1 / 2 - d ln 2 / 2
//                                                     - sum_q psi((v0 + 1 - q) / 2) / 2)
//   lambda0   (d / l0 - d / lam - v (m - m0)' W (m - m0)) / 2
//   W0        v w^2 tr W / 2 (one W0), v w_a^2 W_aa / 2 (one per dimension), w = W0^-1
//                                              - K S v0 d w / 2, - K S v0 w_a / 2
//   m0        l0 v W (m - m0)
// No clipping and no change of variables (host.transform_derivs applies those).
//
// Also the layout of the per-trial hyperparameter table the trials kernels read
// (vbhem_em_run_trials_hyp fills it once per call).  Internal.
#pragma once
#include <cmath>

#include "vbhem_special.h"

namespace vbhem {

// one trial's table: alpha0 eta0 epsilon0 lambda0 v0 | logCalpha0 logCeta0 logCepsilon0
// logB0 | m0 [d] | W0^-1 [d][d]
enum {
  kHypAlpha0 = 0, kHypEta0, kHypEpsilon0, kHypLambda0, kHypV0,
  kHypLogCalpha0, kHypLogCeta0, kHypLogCepsilon0, kHypLogB0,
  kHypM0
};
VBE_HD inline int hyp_table_len(int d) { return kHypM0 + d + d * d; }

// what row a of W contributes for (k, s): (m - m0)_a (W (m - m0))_a, W_aa and
// l0 v (W (m - m0))_a.  W is [d][d] (full) or the diagonal [d].
struct DerivRow {
  double mwm, wdiag, gm;
};

VBE_HD inline DerivRow deriv_row(const double *W, const double *mk, const double *m0, int d,
                                 bool full, int a, double l0, double v) {
  double wd = 0.0;  // (W (m - m0))[a]
  if (full) {
    for (int b = 0; b < d; ++b) wd += W[a * d + b] * (mk[b] - m0[b]);
  } else {
    wd = W[a] * (mk[a] - m0[a]);
  }
  DerivRow r;
  r.mwm = (mk[a] - m0[a]) * wd;
  r.wdiag = full ? W[a * d + a] : W[a];
  r.gm = l0 * v * wd;
  return r;
}

VBE_HD inline double deriv_lambda0_term(int d, double l0, double lam, double v, double mWm) {
  return 0.5 * (d / l0 - d / lam - v * mWm);
}

// wi: the entry of W0^-1; w: tr W (one W0) or W_aa
VBE_HD inline double deriv_w0_term(double v, double wi, double w) {
  return -0.5 * (-v * wi * wi * w);
}

// The hyperparameter-only part of derivative q of a trial with K clusters of S states;
// h: the trial's table, nW: the number of W0 entries (1 or d).
VBE_HD inline double deriv_closed_form(int q, int K, int S, int d, int nW, const double *h) {
  const double *W0inv = h + kHypM0 + d;
  if (q == 0) {
    const double a0 = h[kHypAlpha0];
    return K * psi_onediv(K * a0) - K * psi_onediv(a0);
  }
  if (q == 1) {
    const double e0 = h[kHypEta0];
    return K * (S * psi_onediv(S * e0) - S * psi_onediv(e0));
  }
  if (q == 2) {
    const double ep0 = h[kHypEpsilon0];
    return (double)K * S * (S * psi_onediv(S * ep0) - S * psi_onediv(ep0));
  }
  if (q == 3) {
    const double v0 = h[kHypV0];
    double logdetW0inv = 0.0, sp = 0.0;
    if (nW == 1) logdetW0inv = d * log(W0inv[0]);
    else for (int a = 0; a < d; ++a) logdetW0inv += log(W0inv[a * d + a]);
    for (int x = 1; x <= d; ++x) sp += psi_onediv(0.5 * (v0 + 1 - x));
    return (double)K * S * (0.5 * logdetW0inv - (d / 2.0) * log(2.0) - 0.5 * sp);
  }
  if (q >= 5 && q < 5 + nW) {
    const double v0 = h[kHypV0];
    if (nW == 1) return (double)K * S * (-0.5 * v0 * d * W0inv[0]);
    const int a = q - 5;
    return (double)K * S * (-0.5 * v0 * W0inv[a * d + a]);
  }
  return 0.0;  // lambda0, m0
}

// The 5 + nW + d terms of one (k, s), serially (the device spreads the rows and the
// terms over the lanes of a wavefront and calls the same functions).  logOmega_k is
// counted for state 0 only.
VBE_HD inline void deriv_ks_terms(int s, int d, bool full, int nW, double logOmega_k, double logPi,
                                  double sumLogA, double lLT, double v, double lam,
                                  const double *mk, const double *W, const double *h, double *out) {
  const double l0 = h[kHypLambda0];
  const double *m0 = h + kHypM0, *W0inv = h + kHypM0 + d;
  double mWm = 0.0, trW = 0.0;
  for (int a = 0; a < d; ++a) {
    const DerivRow r = deriv_row(W, mk, m0, d, full, a, l0, v);
    mWm += r.mwm;
    trW += r.wdiag;
    out[5 + nW + a] = r.gm;
    if (nW > 1) out[5 + a] = deriv_w0_term(v, W0inv[a * d + a], r.wdiag);
  }
  if (nW == 1) out[5] = deriv_w0_term(v, W0inv[0], trW);
  out[0] = s == 0 ? logOmega_k : 0.0;
  out[1] = logPi;
  out[2] = sumLogA;
  out[3] = 0.5 * lLT;
  out[4] = deriv_lambda0_term(d, l0, lam, v, mWm);
}

}  // namespace vbhem
