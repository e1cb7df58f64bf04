// tests/emderivcheck/emderivcheck.hip -- TEST-ONLY host build of the arithmetic of the
// bound's hyperparameter derivatives (csrc/vbhem_em_deriv_terms.h), the functions
// trials_derivs_kernel runs on the device, so tests/test_em_deriv_terms.py checks them
// against host.lower_bound_derivs on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <vector>

#include "vbhem_em_deriv_terms.h"

extern "C" {

int emderivcheck_table_len(int d) { return vbhem::hyp_table_len(d); }

// offsets into a trial's table: the five scalars, m0, W0^-1
void emderivcheck_table_layout(int d, int *out) {
  out[0] = vbhem::kHypAlpha0; out[1] = vbhem::kHypEta0; out[2] = vbhem::kHypEpsilon0;
  out[3] = vbhem::kHypLambda0; out[4] = vbhem::kHypV0; out[5] = vbhem::kHypM0;
  out[6] = vbhem::kHypM0 + d;
}

// The raw derivatives [5 + nW + d] of one trial: every (k, s)'s terms, summed in (k, s)
// order per derivative, plus the closed forms -- what the trial's last wave does.
// v, lam [K][S]; m [K][S][d]; W [K][S][d][d] (cov 1) or [K][S][d]; logOmega [K]; logPi,
// lLT [K][S]; logA [K][S][S]; h: the trial's table.
void emderivcheck_raw(int K, int S, int d, int cov, int nW, const double *v, const double *lam,
                      const double *m, const double *W, const double *logOmega, const double *logPi,
                      const double *logA, const double *lLT, const double *h, double *out) {
  const int n = 5 + nW + d;
  const size_t dd = cov == 1 ? (size_t)d * d : (size_t)d;
  std::vector<double> term((size_t)n);
  for (int q = 0; q < n; ++q) out[q] = 0.0;
  for (int k = 0; k < K; ++k)
    for (int s = 0; s < S; ++s) {
      const size_t ks = (size_t)k * S + s;
      double sla = 0.0;
      for (int s2 = 0; s2 < S; ++s2) sla += logA[ks * S + s2];
      vbhem::deriv_ks_terms(s, d, cov == 1, nW, logOmega[k], logPi[ks], sla, lLT[ks], v[ks], lam[ks],
                            m + ks * d, W + ks * dd, h, term.data());
      for (int q = 0; q < n; ++q) out[q] += term[(size_t)q];
    }
  for (int q = 0; q < n; ++q) out[q] += vbhem::deriv_closed_form(q, K, S, d, nW, h);
}

}  // extern "C"
