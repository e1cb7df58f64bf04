// tests/emderivcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the arithmetic of the
// bound's hyperparameter derivatives (csrc/vbhem_em_deriv_terms.h) over small made-up
// posteriors, for a run under the address and undefined-behaviour sanitizers on the CPU
// (`make emderiv_sanitize`; plain C++, no device compiler).  Every array has exactly the
// size the trials loop gives it (the table 9 + d + d d, the terms 5 + nW + d), so an index
// past an end is an error the sanitizer reports; the sums are compared with a direct
// restatement of vbhemh3m_lb.m:202-345 for the lambda0 and m0 derivatives.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vbhem_em_deriv_terms.h"

int main() {
  int bad = 0, cases = 0;
  for (int d : {1, 2, 3, 16})
    for (int full = 0; full < 2; ++full)
      for (int nW : {1, d}) {
        const int K = 2, S = 3, n = 5 + nW + d;
        const size_t dd = full ? (size_t)d * d : (size_t)d;
        std::vector<double> h((size_t)vbhem::hyp_table_len(d)), term((size_t)n), sum((size_t)n, 0.0);
        h[vbhem::kHypAlpha0] = 1.5; h[vbhem::kHypEta0] = 0.7; h[vbhem::kHypEpsilon0] = 1.2;
        h[vbhem::kHypLambda0] = 0.9; h[vbhem::kHypV0] = d + 2.5;
        for (int a = 0; a < d; ++a) {
          h[(size_t)vbhem::kHypM0 + a] = 0.1 * a - 0.3;
          h[(size_t)vbhem::kHypM0 + d + (size_t)a * d + a] = 1.0 / (nW == 1 ? 0.8 : 0.5 + 0.1 * a);
        }
        double lam0 = 0.0;
        std::vector<double> gm((size_t)d, 0.0);
        for (int k = 0; k < K; ++k)
          for (int s = 0; s < S; ++s) {
            std::vector<double> W(dd, 0.0), m((size_t)d);
            const double v = d + 3.0 + k + 0.5 * s, lam = 2.0 + s;
            for (int a = 0; a < d; ++a) {
              m[(size_t)a] = 0.2 * a + 0.1 * k - 0.05 * s;
              if (full) {
                for (int b = 0; b < d; ++b) W[(size_t)a * d + b] = (a == b ? 1.0 + 0.1 * a : 0.01) / v;
              } else {
                W[(size_t)a] = (1.0 + 0.1 * a) / v;
              }
            }
            vbhem::deriv_ks_terms(s, d, full != 0, nW, -0.4 - k, -1.0 - s, -3.0, 0.5 * k, v, lam, m.data(),
                                  W.data(), h.data(), term.data());
            for (int q = 0; q < n; ++q) sum[(size_t)q] += term[(size_t)q];
            double mWm = 0.0;
            for (int a = 0; a < d; ++a) {
              double wd = 0.0;
              for (int b = 0; b < d; ++b) {
                const double w = full ? W[(size_t)a * d + b] : (a == b ? W[(size_t)a] : 0.0);
                wd += w * (m[(size_t)b] - h[(size_t)vbhem::kHypM0 + b]);
              }
              mWm += (m[(size_t)a] - h[(size_t)vbhem::kHypM0 + a]) * wd;
              gm[(size_t)a] += h[vbhem::kHypLambda0] * v * wd;
            }
            lam0 += 0.5 * (d / h[vbhem::kHypLambda0] - d / lam - v * mWm);
          }
        for (int q = 0; q < n; ++q) {
          sum[(size_t)q] += vbhem::deriv_closed_form(q, K, S, d, nW, h.data());
          bad += !std::isfinite(sum[(size_t)q]);
        }
        bad += std::fabs(sum[4] - lam0) > 1e-12 * (1.0 + std::fabs(lam0));
        for (int a = 0; a < d; ++a)
          bad += std::fabs(sum[(size_t)(5 + nW + a)] - gm[(size_t)a]) > 1e-12 * (1.0 + std::fabs(gm[(size_t)a]));
        ++cases;
      }
  std::printf("emderiv walker: %d cases, %d errors\n", cases, bad);
  return bad ? 1 : 0;
}
