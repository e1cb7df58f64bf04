// vbhmm_dic_pair.h -- the arithmetic of the VHEM expected log-likelihood L(i, c) of one
// base HMM i under one group HMM c (include/vbhmm_dic.h), written once for the device
// kernel (vbhmm_dic.hip) and for a host build (tests/diccheck).  It is
// hem_hmm_bwd_fwd_mex.c in diag mode at smooth = 1, backward sweep and termination only
// (DESIGN.md 4.7, 4.13):
//   E[beta,sigma] = -1/2 (d ln 2pi + c_sigma + sum_a P_sigma,a (Sigma_beta,a + (mu_beta,a - m_sigma,a)^2))
//   L = 0;  t = T-1 .. 1, every rho:  s(rho,beta) = LSE_sigma(logA[rho,sigma] + E[beta,sigma] + L[beta,sigma])
//                                     L'[gamma,rho] = sum_beta Ab[gamma,beta] s(rho,beta)
//   L(i,c) = sum_beta pi_b[beta] LSE_sigma(logPi[sigma] + E[beta,sigma] + L[beta,sigma])
//
// The unit is one base-state COLUMN beta of a pair: it owns E[beta,.], L[beta,.] and
// s(., beta) (sigma / rho in registers); only the mixing with Ab crosses columns.  The
// device kernel gives a column to a lane and mixes by shuffles; pair_serial below walks
// the columns in a loop and is what the host build checks against the oracle.
//
// A step uses the factorised log-sum-exp of DESIGN.md 4.2: with amax(rho) = max_sigma
// logA, A' = exp(logA - amax) (prepared once per cluster), M = max_sigma v, G = exp(v - M):
//   s(rho,beta) = M + amax(rho) + log Z,   Z = sum_sigma A'(rho,sigma) G(sigma).
// A column whose Z falls below kZMin reports it; the pair is then recomputed in reference
// order (column_step_exact: S exps per (rho, beta), max first, sum in index order).
//
// Loops run over the cluster's own states (k.S) and the base's own states; padding is
// never read into a sum.  -inf in logA / logPi is a zero transition.  NaN, and the
// inf - inf of a row or column without any finite entry, propagate to L: the exps keep
// NaN (exp_nonpos alone would clamp it away).
#pragma once
#include <cmath>

#include "vbhem_math.h"

#define VBD_HD __host__ __device__

namespace vbhem {
namespace dic {

constexpr int kMaxStates = 16;         // S, SB
constexpr int kMaxDim = 16;            // d
constexpr int kMaxModelClusters = 64;  // clusters of one model
constexpr double kZMin = 1e-200;       // below: recompute the pair in reference order
constexpr double kLog2Pi = 1.83787706640934548356065947281123;

VBD_HD constexpr int state_bucket(int s) { return s <= 4 ? 4 : s <= 8 ? 8 : 16; }

// doubles of one prepared cluster block for bucket SP and dimension d:
// [ S | A' SP x SP | amax SP | logPi SP | c SP | m SP x d | P SP x d ]
VBD_HD constexpr int block_len(int SP, int d) { return 2 + SP * SP + 3 * SP + 2 * SP * d; }

// One cluster as the routines read it.  Aexp / amax are only read by column_step,
// logA only by column_step_exact.
struct Cluster {
  int S, d;            // own states, dimension
  int ldA;             // row stride of Aexp
  int ldlogA;          // row stride of logA
  const double *Aexp;  // exp(logA[rho][sigma] - amax[rho])
  const double *amax;
  const double *logPi;
  const double *c;
  const double *m;  // [S][d]
  const double *P;  // [S][d]
  const double *logA;
};

VBD_HD inline Cluster view_block(const double *blk, int SP, int d, const double *logA, int ldlogA) {
  Cluster k;
  k.S = (int)blk[0];
  k.d = d;
  k.ldA = SP;
  k.ldlogA = ldlogA;
  k.Aexp = blk + 2;
  k.amax = k.Aexp + SP * SP;
  k.logPi = k.amax + SP;
  k.c = k.logPi + SP;
  k.m = k.c + SP;
  k.P = k.m + SP * d;
  k.logA = logA;
  return k;
}

VBD_HD __forceinline__ double exp_keep_nan(double x) { return x != x ? x : exp_nonpos(x); }

// One cluster's block from its descriptor rows (logA [S][ld], logPi, c [ld], m, P [ld][d];
// own states n).  Padding is zero.
VBD_HD inline void prepare_block(double *blk, int SP, int d, int n, int ld, const double *logA,
                                 const double *logPi, const double *c, const double *m, const double *P) {
  const int len = block_len(SP, d);
  for (int q = 0; q < len; ++q) blk[q] = 0.0;
  blk[0] = (double)n;
  double *Aexp = blk + 2, *amax = Aexp + SP * SP, *lp = amax + SP, *cc = lp + SP, *mm = cc + SP,
         *PP = mm + SP * d;
  for (int r = 0; r < n; ++r) {
    double mx = logA[r * ld];
    for (int s = 1; s < n; ++s) mx = fmax(mx, logA[r * ld + s]);
    amax[r] = mx;
    for (int s = 0; s < n; ++s) Aexp[r * SP + s] = exp_keep_nan(logA[r * ld + s] - mx);
    lp[r] = logPi[r];
    cc[r] = c[r];
    for (int a = 0; a < d; ++a) {
      mm[r * d + a] = m[r * d + a];
      PP[r * d + a] = P[r * d + a];
    }
  }
}

// E[beta, .] of one base state (mean mu [d], variances cov [d]); 0 past k.S.
template <int SP>
VBD_HD __forceinline__ void column_emission(const Cluster &k, const double *mu, const double *cov,
                                            double (&E)[SP]) {
  double q[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) q[s] = 0.0;
  for (int a = 0; a < k.d; ++a) {
    const double xm = mu[a], xc = cov[a];
#pragma unroll
    for (int s = 0; s < SP; ++s)
      if (s < k.S) {
        const double x = xm - k.m[s * k.d + a];
        q[s] = fma(k.P[s * k.d + a], xc + x * x, q[s]);
      }
  }
#pragma unroll
  for (int s = 0; s < SP; ++s) E[s] = s < k.S ? -0.5 * ((double)k.d * kLog2Pi + k.c[s] + q[s]) : 0.0;
}

// Factorised step of one column: v[sigma] = E + L in, s[rho] out.  true: a Z fell below
// kZMin and s is not to be used.
template <int SP>
VBD_HD __forceinline__ bool column_step(const Cluster &k, const double (&v)[SP], double (&s)[SP]) {
  double M = v[0];
#pragma unroll
  for (int q = 1; q < SP; ++q)
    if (q < k.S) M = fmax(M, v[q]);
  double G[SP];
#pragma unroll
  for (int q = 0; q < SP; ++q) G[q] = q < k.S ? exp_keep_nan(v[q] - M) : 0.0;
  bool low = false;
#pragma unroll
  for (int r = 0; r < SP; ++r) {
    s[r] = 0.0;
    if (r < k.S) {
      double Z = 0.0;
#pragma unroll
      for (int q = 0; q < SP; ++q)
        if (q < k.S) Z = fma(k.Aexp[r * k.ldA + q], G[q], Z);
      low = low || Z < kZMin;
      s[r] = (M + k.amax[r]) + log_pos(Z < kZMin ? 1.0 : Z);
    }
  }
  return low;
}

// The same step in reference order (logtrick: max first, then the sum in index order).
template <int SP>
VBD_HD __forceinline__ void column_step_exact(const Cluster &k, const double (&E)[SP],
                                              const double (&L)[SP], double (&s)[SP]) {
#pragma unroll
  for (int r = 0; r < SP; ++r) {
    s[r] = 0.0;
    if (r < k.S) {
      double lt[SP];
      double mv = 0.0;
#pragma unroll
      for (int q = 0; q < SP; ++q)
        if (q < k.S) {
          lt[q] = (k.logA[r * k.ldlogA + q] + E[q]) + L[q];
          if (q == 0 || lt[q] > mv) mv = lt[q];
        }
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < SP; ++q)
        if (q < k.S) acc += exp_keep_nan(lt[q] - mv);
      s[r] = mv + log_pos(acc);
    }
  }
}

// Termination of one column: LSE_sigma(logPi + E + L), reference order.
template <int SP>
VBD_HD __forceinline__ double column_term(const Cluster &k, const double (&E)[SP], const double (&L)[SP]) {
  double lt[SP];
  double mv = 0.0;
#pragma unroll
  for (int q = 0; q < SP; ++q)
    if (q < k.S) {
      lt[q] = (k.logPi[q] + E[q]) + L[q];
      if (q == 0 || lt[q] > mv) mv = lt[q];
    }
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < SP; ++q)
    if (q < k.S) acc += exp_keep_nan(lt[q] - mv);
  return mv + log_pos(acc);
}

// The mixture term of one (base, cluster): each operation rounded as written.
VBD_HD __forceinline__ double mixture_term(double logw, double scale, double L) {
  const double t = scale * L;
  return logw + t;
}

// LSE over n mixture terms spaced by `stride`: max first, then the sum in index order.
VBD_HD inline double mixture_lse(const double *x, int n, int stride) {
  double mv = x[0];
  for (int j = 1; j < n; ++j)
    if (x[j * stride] > mv) mv = x[j * stride];
  double acc = 0.0;
  for (int j = 0; j < n; ++j) acc += exp_keep_nan(x[j * stride] - mv);
  return mv + log_pos(acc);
}

// One whole pair, column after column: Sb own base states, prior pi [Sb], Ab rows of
// stride ldb, means / variances [.][d].  *recomputed is incremented when the pair had to
// be redone in reference order; exact_only skips the factorised attempt.
template <int SP>
VBD_HD inline double pair_serial(const Cluster &k, int Sb, int ldb, const double *pi, const double *Ab,
                                 const double *mu, const double *cov, int T, bool exact_only,
                                 int *recomputed) {
  double E[kMaxStates][SP], L[kMaxStates][SP], s[kMaxStates][SP];
  for (int b = 0; b < Sb; ++b) column_emission<SP>(k, mu + b * k.d, cov + b * k.d, E[b]);
  for (int attempt = exact_only ? 1 : 0; attempt < 2; ++attempt) {
    for (int b = 0; b < Sb; ++b)
      for (int q = 0; q < SP; ++q) L[b][q] = 0.0;
    bool low = false;
    for (int t = T - 1; t >= 1 && !low; --t) {
      for (int b = 0; b < Sb; ++b) {
        if (attempt == 0) {
          double v[SP];
          for (int q = 0; q < SP; ++q) v[q] = E[b][q] + L[b][q];
          low = column_step<SP>(k, v, s[b]) || low;
        } else {
          column_step_exact<SP>(k, E[b], L[b], s[b]);
        }
      }
      if (low) break;
      for (int g = 0; g < Sb; ++g)
        for (int r = 0; r < k.S; ++r) {
          double acc = 0.0;
          for (int b = 0; b < Sb; ++b) acc = fma(Ab[g * ldb + b], s[b][r], acc);
          L[g][r] = acc;
        }
    }
    if (low) {
      if (recomputed) ++*recomputed;
      continue;
    }
    double LL = 0.0;
    for (int b = 0; b < Sb; ++b) LL += pi[b] * column_term<SP>(k, E[b], L[b]);
    return LL;
  }
  return NAN;  // not reached: the reference-order attempt never reports a low Z
}

}  // namespace dic
}  // namespace vbhem
