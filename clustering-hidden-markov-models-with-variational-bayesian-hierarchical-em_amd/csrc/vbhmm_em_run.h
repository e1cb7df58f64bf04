// vbhmm_em_run.h -- the arithmetic of one VB-HMM EM run (include/vbhmm_em.h), written
// once for the device kernel (vbhmm_em.hip) and for a host build (tests/vbhmmemcheck, and
// any C++ compiler: nothing here needs a device compiler).  A run is one (subject, K,
// initial posterior); its EM is vbhmm_em.m:112-414 with usegroups = 0 and fix_clusters,
// fix_cov unset:
//   prelude   logLambdaTilde, logATilde, logPiTilde and their exps     vbhmm_fb.m:54-93
//   phase A   per sequence: the scaled forward-backward of vbhmm_fb_mex.c in the MEX's
//             operation order, keeping gamma (parked in the run's
//             workspace), sum_t xi, sum_t sum_k gamma logrho, phi, sum_k gamma_1 logPi
//   phase B   Nk1, Nk, M, xbar and the CENTRED second moment t1_S about xbar (a second
//             pass over the parked gamma, vbhmm_em.m:241-246), every sum over (n, t) in
//             index order
//   bound     vbhmm_em_lb.m:74-257, per-state terms then one total in state order
//   M-step    vbhmm_em.m:352-383; W_k by a Cholesky-based inverse in place
//
// The units are one STATE (prelude_state, bound_state, mstep_state), one SEQUENCE
// (fb_sequence) and one statistic ENTRY (stat_*).  Which units run in which order, when
// the loop ends and what is captured when is run_em below, written once: the device
// kernel walks it with a unit per lane (WaveLanes), run_serial with plain loops
// (SerialLanes), which is what the host build checks against the oracle.  Both read and
// write the same Run<KM> (LDS on the device).
//
// Padding: a run has K <= KM own states; every loop runs over K, padding is never read
// into a sum, so a run's result does not depend on KM.  A NaN (log det of an indefinite
// W) propagates to the bound, which ends the run as unstable; every loop is bounded by
// max_iter, the sequence count or a sequence length whatever the values are.
#pragma once
#include <cmath>

#include "vbhem_special.h"  // VBE_HD, psi_onediv, lgamma_stirling

#if defined(__HIPCC__)
#define VBE_UNROLL _Pragma("unroll")
#else
#define VBE_UNROLL
#endif

namespace vbhem {
namespace emrun {

constexpr int kMaxDim = 8;
constexpr int kMaxStates = 8;
constexpr double kPi = 3.14159265358979323846;
constexpr double kLn2 = 0.69314718055994530942;
constexpr double kLnPi = 1.14472988584940017414;
constexpr double kLn2Pi = 1.83787706640934548356;

// status of a run (include/vbhmm_em.h)
constexpr int kConverged = 0, kMaxIter = 1, kUnstable = 2, kBadRun = 3;

VBE_HD constexpr int state_bucket(int K) { return K <= 4 ? 4 : 8; }

// Packed posterior of one run, KM-padded: [alpha KM | epsilon KM x KM | beta KM | v KM |
// m KM x dim | W KM x dim x dim]
VBE_HD constexpr int post_len(int KM, int dim) { return KM * (3 + KM + dim + dim * dim); }
// Packed statistics: [Nk1 KM | Nk KM | M KM x KM | xbar KM x dim | t1_S KM x dim x dim]
VBE_HD constexpr int stats_len(int KM, int dim) { return KM * (2 + KM + dim + dim * dim); }
// Per-sequence record kept by phase A: [xi KM x KM | phi | sum gamma logrho | sum_k gamma_1 logPi]
VBE_HD constexpr int seq_len(int KM) { return KM * KM + 3; }
// Per-observation doubles of a run's workspace: gamma KM, logrho KM, c, max
VBE_HD constexpr int obs_len(int KM) { return 2 * KM + 2; }

struct Hyper {
  double alpha0, epsilon0, beta0, v0;
  double m0[kMaxDim];
  double W0inv[kMaxDim];  // the diagonal of W0^-1
};

// per-state terms of the bound, summed over the states in state order by bound_total
enum { qLt1, qMlA, qSumlA, qLt51, qlLT, qvTrW0W, qAlPi, qLgAlpha, qLt72, qLt8a, qH, qlPi, kNQ };

// Everything of one run that is not per sequence or per observation.
template <int KM>
struct Run {
  int K, dim;
  double post[post_len(KM, kMaxDim)];
  double stats[stats_len(KM, kMaxDim)];
  double lLT[KM], logdetW[KM], logPi[KM], pz1[KM], db[KM], logA[KM * KM], A[KM * KM];
  double q[KM][kNQ];
  double L, lastL;
  int flags;  // loop control of the current iteration: 1 break, 2 converged, 4 unstable

  VBE_HD double *alpha() { return post; }
  VBE_HD double *eps() { return post + KM; }
  VBE_HD double *beta() { return post + KM + KM * KM; }
  VBE_HD double *v() { return post + 2 * KM + KM * KM; }
  VBE_HD double *m() { return post + 3 * KM + KM * KM; }
  VBE_HD double *W() { return post + 3 * KM + KM * KM + KM * dim; }
  VBE_HD double *Nk1() { return stats; }
  VBE_HD double *Nk() { return stats + KM; }
  VBE_HD double *M() { return stats + 2 * KM; }
  VBE_HD double *xbar() { return stats + 2 * KM + KM * KM; }
  VBE_HD double *S() { return stats + 2 * KM + KM * KM + KM * dim; }
};

// One subject's data as a run sees it: N sequences, sequence n's observations at rows
// off[n] .. off[n+1]-1 of x (absolute rows); base = off[0], so that observation row p of
// the subject sits at workspace position p - base.
struct Subject {
  int N;
  const int *off;   // [N+1]
  const double *x;  // [rows][dim]
};

// A run's workspace: obs[(p - base)] records of gamma | logrho, c and max per observation,
// and one record per sequence.
template <int KM>
struct Work {
  double *gamma;   // [obs][KM]
  double *logrho;  // [obs][KM]
  double *cs;      // [obs]
  double *mxs;     // [obs]
  double *seq;     // [N][seq_len(KM)]
};

// In-place Cholesky factor (lower triangle) of the d x d matrix a (row stride d).  Returns
// log det a = 2 sum log L_ii: NaN when a pivot is not positive (sqrt of a negative).
VBE_HD inline double chol_inplace(double *a, int d) {
  double logdet = 0.0;
  for (int j = 0; j < d; ++j) {
    double s = a[j * d + j];
    for (int k = 0; k < j; ++k) s -= a[j * d + k] * a[j * d + k];
    const double ljj = sqrt(s);
    a[j * d + j] = ljj;
    logdet += 2.0 * log(ljj);
    for (int i = j + 1; i < d; ++i) {
      double t = a[i * d + j];
      for (int k = 0; k < j; ++k) t -= a[i * d + k] * a[j * d + k];
      a[i * d + j] = t / ljj;
    }
  }
  return logdet;
}

// In-place inverse of a symmetric positive definite d x d matrix: a = L L', L^-1 in the
// lower triangle, then a^-1 = L^-T L^-1 (upper triangle first, the diagonal after it,
// mirrored): symmetric by construction, so (a^-1 + a^-T) / 2 changes nothing.
VBE_HD inline void spd_inverse_inplace(double *a, int d) {
  chol_inplace(a, d);
  for (int j = 0; j < d; ++j) {  // L^-1, column by column
    a[j * d + j] = 1.0 / a[j * d + j];
    for (int i = j + 1; i < d; ++i) {
      double t = 0.0;
      for (int k = j; k < i; ++k) t -= a[i * d + k] * a[k * d + j];
      a[i * d + j] = t / a[i * d + i];
    }
  }
  for (int i = 0; i < d; ++i)
    for (int j = i + 1; j < d; ++j) {
      double t = 0.0;
      for (int k = j; k < d; ++k) t += a[k * d + i] * a[k * d + j];
      a[i * d + j] = t;
    }
  for (int i = 0; i < d; ++i) {
    double t = 0.0;
    for (int k = i; k < d; ++k) t += a[k * d + i] * a[k * d + i];
    a[i * d + i] = t;
  }
  for (int i = 0; i < d; ++i)
    for (int j = i + 1; j < d; ++j) a[j * d + i] = a[i * d + j];
}

// ---- prelude of one state k (vbhmm_fb.m:54-93).  Uses the state's t1_S slot as scratch
// for the factor of W_k: the statistics are dead until phase B writes them again.
template <int KM>
VBE_HD inline void prelude_state(Run<KM> &r, int k) {
  const int K = r.K, dim = r.dim;
  const double v = r.v()[k];
  double t1 = 0.0;
  for (int q = 1; q <= dim; ++q) t1 += psi_onediv(0.5 * (v + 1.0) - 0.5 * q);
  double *sc = r.S() + k * dim * dim;
  const double *W = r.W() + k * dim * dim;
  for (int x = 0; x < dim * dim; ++x) sc[x] = W[x];
  const double logdet = chol_inplace(sc, dim);
  r.logdetW[k] = logdet;
  r.lLT[k] = t1 + dim * kLn2 + logdet;
  r.db[k] = dim / r.beta()[k];
  double se = 0.0, sa = 0.0;
  for (int j = 0; j < K; ++j) {
    se += r.eps()[k * KM + j];
    sa += r.alpha()[j];
  }
  const double pse = psi_onediv(se);
  for (int j = 0; j < K; ++j) {
    const double la = psi_onediv(r.eps()[k * KM + j]) - pse;
    r.logA[k * KM + j] = la;
    r.A[k * KM + j] = exp(la);
  }
  const double lp = psi_onediv(r.alpha()[k]) - psi_onediv(sa);
  r.logPi[k] = lp;
  r.pz1[k] = exp(lp);
}

// ---- phase A of one sequence: x [T][dim], its gamma / logrho rows [T][KM], c / max [T],
// and its record rec [seq_len(KM)] (T < 1: a record of zeros).  vbhmm_fb_kernel's
// operations in its order.
template <int KM>
VBE_HD inline void fb_sequence(const Run<KM> &r, const double *xn, int T, double *gam, double *lrho,
                               double *cs, double *mxs, double *rec) {
  const int K = r.K, dim = r.dim;
  const double cden = dim * kLn2Pi / 2.0;
  const double *sm = r.post + 3 * KM + KM * KM, *sW = sm + KM * dim, *sv = r.post + 2 * KM + KM * KM;
  // sum_t xi accumulates in the record itself (as vbhmm_fb_kernel does in its output):
  // KM x KM more registers per lane would halve the waves a SIMD holds
VBE_UNROLL
  for (int q = 0; q < KM * KM; ++q) rec[q] = 0.0;
  double phi = 0.0, glr = 0.0, g1 = 0.0;
  if (T >= 1) {
    double al[KM], px[KM];
    for (int t = 0; t < T; ++t) {
      double lr[KM];
VBE_UNROLL
      for (int k = 0; k < KM; ++k) {
        lr[k] = 0.0;
        if (k < K) {
          // diff is taken again where it is used (the same subtraction, the same value):
          // no per-lane array, the loops stay loops over dim
          double tmp = 0.0;
          for (int a = 0; a < dim; ++a) {
            double w = 0.0;  // (W(:,a,k) . diff), mex.c:371-383
            for (int b = 0; b < dim; ++b) w += sW[(k * dim + b) * dim + a] * (xn[t * dim + b] - sm[k * dim + b]);
            w *= xn[t * dim + a] - sm[k * dim + a];
            tmp += w;
          }
          const double delta = r.db[k] + sv[k] * tmp;
          lr[k] = 0.5 * (r.lLT[k] - delta) - cden;
          lrho[t * KM + k] = lr[k];
        }
      }
      double mx = lr[0];
VBE_UNROLL
      for (int k = 1; k < KM; ++k)
        if (k < K && lr[k] > mx) mx = lr[k];
VBE_UNROLL
      for (int k = 0; k < KM; ++k) px[k] = k < K ? exp(lr[k] - mx) : 0.0;
      double D[KM];
      if (t == 0) {
VBE_UNROLL
        for (int k = 0; k < KM; ++k) D[k] = k < K ? r.pz1[k] * px[k] : 0.0;
      } else {
VBE_UNROLL
        for (int j = 0; j < KM; ++j) {
          double tmp = 0.0;
VBE_UNROLL
          for (int i = 0; i < KM; ++i)
            if (i < K && j < K) tmp += al[i] * r.A[i * KM + j];
          D[j] = tmp * px[j];
        }
      }
      double c = 0.0;
VBE_UNROLL
      for (int k = 0; k < KM; ++k) c += k < K ? D[k] : 0.0;
VBE_UNROLL
      for (int k = 0; k < KM; ++k) {
        al[k] = k < K ? D[k] / c : 0.0;
        if (k < K) gam[t * KM + k] = al[k];  // alpha_t, parked
      }
      cs[t] = c;
      mxs[t] = mx;
      phi += log(c) + mx;
    }
    double be[KM];
VBE_UNROLL
    for (int k = 0; k < KM; ++k) be[k] = 1.0;
    for (int t = T - 2; t >= 0; --t) {
      const double c1 = cs[t + 1], mx1 = mxs[t + 1];
      double bpi[KM];
VBE_UNROLL
      for (int k = 0; k < KM; ++k) bpi[k] = k < K ? be[k] * exp(lrho[(t + 1) * KM + k] - mx1) : 0.0;
VBE_UNROLL
      for (int i = 0; i < KM; ++i) {
        double tmp = 0.0;
VBE_UNROLL
        for (int j = 0; j < KM; ++j)
          if (i < K && j < K) tmp += bpi[j] * r.A[i * KM + j];
        be[i] = i < K ? tmp / c1 : 0.0;
      }
      double a[KM];
VBE_UNROLL
      for (int k = 0; k < KM; ++k) {
        a[k] = k < K ? gam[t * KM + k] : 0.0;
        if (k < K) gam[t * KM + k] = a[k] * be[k];
      }
VBE_UNROLL
      for (int j = 0; j < KM; ++j)
VBE_UNROLL
        for (int i = 0; i < KM; ++i)
          if (i < K && j < K) rec[i * KM + j] += r.A[i * KM + j] * a[i] * bpi[j] / c1;
    }
    for (int t = 0; t < T; ++t)
VBE_UNROLL
      for (int k = 0; k < KM; ++k)
        if (k < K) glr += gam[t * KM + k] * lrho[t * KM + k];
VBE_UNROLL
    for (int k = 0; k < KM; ++k)
      if (k < K) g1 += gam[k] * r.logPi[k];
  }
  rec[KM * KM] = phi;
  rec[KM * KM + 1] = glr;
  rec[KM * KM + 2] = g1;
}

// ---- phase B, one entry each.  obs = the subject's observation count; gamma rows and x
// rows run over the subject's observations in index order.
template <int KM>
VBE_HD inline void stat_counts(Run<KM> &r, const Subject &s, const Work<KM> &w, int k) {
  const int base = s.off[0], obs = s.off[s.N] - base;
  double n1 = 0.0, nk = 0.0;
  for (int n = 0; n < s.N; ++n)
    if (s.off[n + 1] > s.off[n]) n1 += w.gamma[(size_t)(s.off[n] - base) * KM + k];
  for (int p = 0; p < obs; ++p) nk += w.gamma[(size_t)p * KM + k];
  r.Nk1()[k] = n1 + 1e-50;
  r.Nk()[k] = nk + 1e-50;
}

template <int KM>
VBE_HD inline void stat_trans(Run<KM> &r, const Subject &s, const Work<KM> &w, int i, int j) {
  double acc = 0.0;
  for (int n = 0; n < s.N; ++n) acc += w.seq[(size_t)n * seq_len(KM) + i * KM + j];
  r.M()[i * KM + j] = acc;
}

template <int KM>
VBE_HD inline void stat_mean(Run<KM> &r, const Subject &s, const Work<KM> &w, int k, int a) {
  const int base = s.off[0], obs = s.off[s.N] - base, dim = r.dim;
  const double *x = s.x + (size_t)base * dim;
  double acc = 0.0;
  for (int p = 0; p < obs; ++p) acc += w.gamma[(size_t)p * KM + k] * x[(size_t)p * dim + a];
  r.xbar()[k * dim + a] = acc / r.Nk()[k];
}

template <int KM>
VBE_HD inline void stat_cov(Run<KM> &r, const Subject &s, const Work<KM> &w, int k, int a, int b) {
  const int base = s.off[0], obs = s.off[s.N] - base, dim = r.dim;
  const double *x = s.x + (size_t)base * dim;
  const double xa = r.xbar()[k * dim + a], xb = r.xbar()[k * dim + b];
  double acc = 0.0;
  for (int p = 0; p < obs; ++p)
    acc += w.gamma[(size_t)p * KM + k] * ((x[(size_t)p * dim + a] - xa) * (x[(size_t)p * dim + b] - xb));
  // written after every lane of the wave is past the prelude's use of this slot
  r.S()[(k * dim + a) * dim + b] = acc / r.Nk()[k];
}

// ---- the bound's terms of one state (vbhmm_em_lb.m:74-257)
template <int KM>
VBE_HD inline void bound_state(Run<KM> &r, const Hyper &h, int k) {
  const int K = r.K, dim = r.dim;
  const double v = r.v()[k], beta = r.beta()[k], lLT = r.lLT[k], lPi = r.logPi[k];
  const double *W = r.W() + k * dim * dim, *m = r.m() + k * dim, *S = r.S() + k * dim * dim;
  const double *xb = r.xbar() + k * dim;
  double sg = 0.0;
  for (int q = 1; q <= dim; ++q) sg += lgamma_stirling(0.5 * (v + 1 - q));
  const double logBk = -(v / 2) * r.logdetW[k] - (v * dim / 2) * kLn2 - (dim * (dim - 1) / 4.0) * kLnPi - sg;
  double trSW = 0.0, xWx = 0.0, mWm = 0.0, trW0W = 0.0;
  for (int a = 0; a < dim; ++a) {
    double wx = 0.0, wm = 0.0;
    for (int b = 0; b < dim; ++b) {
      trSW += S[a * dim + b] * W[b * dim + a];
      wx += W[a * dim + b] * (xb[b] - m[b]);
      wm += W[a * dim + b] * (m[b] - h.m0[b]);
    }
    xWx += (xb[a] - m[a]) * wx;
    mWm += (m[a] - h.m0[a]) * wm;
    trW0W += h.W0inv[a] * W[a * dim + a];
  }
  double se = 0.0, sle = 0.0, MlA = 0.0, slA = 0.0, elA = 0.0;
  for (int j = 0; j < K; ++j) {
    const double e = r.eps()[k * KM + j], la = r.logA[k * KM + j];
    se += e;
    sle += lgamma_stirling(e);
    MlA += r.M()[k * KM + j] * la;
    slA += la;
    elA += (e - 1) * la;
  }
  double *q = r.q[k];
  q[qLt1] = r.Nk()[k] * (lLT - dim / beta - v * trSW - v * xWx - dim * kLn2Pi);
  q[qMlA] = MlA;
  q[qSumlA] = slA;
  q[qLt51] = dim * log(h.beta0 / (2 * kPi)) + lLT - dim * h.beta0 / beta - h.beta0 * v * mWm;
  q[qlLT] = lLT;
  q[qvTrW0W] = v * trW0W;
  q[qAlPi] = (r.alpha()[k] - 1) * lPi;
  q[qLgAlpha] = lgamma_stirling(r.alpha()[k]);
  q[qLt72] = elA + (lgamma_stirling(se) - sle);
  q[qLt8a] = lLT + dim * log(beta / (2 * kPi));
  q[qH] = -logBk - 0.5 * (v - dim - 1) * lLT + 0.5 * v * dim;
  q[qlPi] = lPi;
}

// ---- the bound from the states' terms and the sequences' records, in index order
template <int KM>
VBE_HD inline double bound_total(const Run<KM> &r, const Hyper &h, int N, const double *seq) {
  const int K = r.K, dim = r.dim;
  double t[kNQ];
  for (int x = 0; x < kNQ; ++x) t[x] = 0.0;
  double sa = 0.0;
  for (int k = 0; k < K; ++k) {
    for (int x = 0; x < kNQ; ++x) t[x] += r.q[k][x];
    sa += r.post[k];
  }
  double Lt2a = 0.0, Lt63 = 0.0, Lt64 = 0.0;
  for (int n = 0; n < N; ++n) {
    const double *rec = seq + (size_t)n * seq_len(KM) + KM * KM;
    Lt64 += rec[0];
    Lt63 += rec[1];
    Lt2a += rec[2];
  }
  double logdetW0inv = 0.0, sg0 = 0.0;
  for (int a = 0; a < dim; ++a) {
    logdetW0inv += log(h.W0inv[a]);
    sg0 += lgamma_stirling(0.5 * (h.v0 - a));
  }
  const double logCalpha0 = lgamma_stirling(K * h.alpha0) - K * lgamma_stirling(h.alpha0);
  const double logCeps0 = lgamma_stirling(K * h.epsilon0) - K * lgamma_stirling(h.epsilon0);
  const double logB0 = (h.v0 / 2) * logdetW0inv - (h.v0 * dim / 2) * kLn2 - (dim * (dim - 1) / 4.0) * kLnPi - sg0;
  const double logCalpha = lgamma_stirling(sa) - t[qLgAlpha];
  const double Lt1 = 0.5 * t[qLt1];
  const double Lt2b = t[qMlA];
  const double Lt2 = Lt2a + Lt2b;
  const double Lt3 = logCalpha0 + (h.alpha0 - 1) * t[qlPi];
  const double Lt4 = K * logCeps0 + (h.epsilon0 - 1) * t[qSumlA];
  const double Lt51 = 0.5 * t[qLt51];
  const double Lt52 = K * logB0 + 0.5 * (h.v0 - dim - 1) * t[qlLT] - 0.5 * t[qvTrW0W];
  const double Lt5 = Lt51 + Lt52;
  const double Lt6 = Lt2a + Lt2b + Lt63 - Lt64;
  const double Lt7 = t[qAlPi] + logCalpha + t[qLt72];
  const double Lt8 = 0.5 * t[qLt8a] - 0.5 * dim * K - t[qH];
  return Lt1 + Lt2 + Lt3 + Lt4 + Lt5 - Lt6 - Lt7 - Lt8;
}

// ---- loop control of iteration `it` (vbhmm_em.m:277-349): the bound is taken before the
// M-step, the relative change is tested from the second iteration on, a NaN bound ends
// the run as unstable with L = -inf.  Sets r.L, r.lastL, r.flags.
template <int KM>
VBE_HD inline void loop_control(Run<KM> &r, double L, int it, int max_iter, double min_diff) {
  if (it > 1) r.lastL = r.L;
  int fl = 0;
  if (it > 1 && fabs((L - r.lastL) / r.lastL) <= min_diff) fl |= 1 | 2;
  if (it == max_iter) fl |= 1;
  if (L != L) {
    fl = 1 | 4;
    L = -INFINITY;
  }
  r.L = L;
  r.flags = fl;
}

VBE_HD inline int status_of(int flags) { return (flags & 4) ? kUnstable : (flags & 2) ? kConverged : kMaxIter; }

// ---- M-step of one state (vbhmm_em.m:352-383)
template <int KM>
VBE_HD inline void mstep_state(Run<KM> &r, const Hyper &h, int k) {
  const int K = r.K, dim = r.dim;
  const double Nk = r.Nk()[k];
  r.alpha()[k] = h.alpha0 + r.Nk1()[k];
  for (int j = 0; j < K; ++j) r.eps()[k * KM + j] = h.epsilon0 + r.M()[k * KM + j];
  const double beta = h.beta0 + Nk;
  r.beta()[k] = beta;
  r.v()[k] = h.v0 + Nk + 1;
  const double *xb = r.xbar() + k * dim, *S = r.S() + k * dim * dim;
  double *m = r.m() + k * dim, *W = r.W() + k * dim * dim;
  const double mult1 = h.beta0 * Nk / (h.beta0 + Nk);
  for (int a = 0; a < dim; ++a) {
    m[a] = (h.beta0 * h.m0[a] + Nk * xb[a]) / beta;
    for (int b = 0; b < dim; ++b)
      W[a * dim + b] = (a == b ? h.W0inv[a] : 0.0) + Nk * S[a * dim + b] + mult1 * ((xb[a] - h.m0[a]) * (xb[b] - h.m0[b]));
  }
  spd_inverse_inplace(W, dim);
}

// What a run reports besides its posteriors.
struct RunResult {
  double LL;
  int iters, status;
};

// ---- who walks the units of a phase.  once(count, f): f(u) for every u < count, where
// count cannot pass the wave's 64 lanes; each(count, f): the same for any count; sync():
// between two phases, what one wrote the next may read; first(): true for the one walker
// that takes the run's scalar decisions.  Units of a phase are independent, so the order
// in which a policy visits them changes no bit.
struct SerialLanes {
  template <class F>
  VBE_HD void once(int count, F f) const {
    for (int u = 0; u < count; ++u) f(u);
  }
  template <class F>
  VBE_HD void each(int count, F f) const {
    for (int u = 0; u < count; ++u) f(u);
  }
  VBE_HD void sync() const {}
  VBE_HD bool first() const { return true; }
};

#if defined(__HIPCC__)
// A workgroup of ONE wavefront: a unit per lane.  The barrier is a memory fence and
// nothing to wait for.
struct WaveLanes {
  int lane;
  template <class F>
  __device__ __forceinline__ void once(int count, F f) const {
    if (lane < count) f(lane);
  }
  template <class F>
  __device__ __forceinline__ void each(int count, F f) const {
    for (int u = lane; u < count; u += 64) f(u);
  }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ bool first() const { return lane == 0; }
};
#endif

// ---- the schedule of one whole run: the device kernel walks it with WaveLanes, run_serial
// with SerialLanes.  r: the run's state (LDS on the device), filled here; post_in
// [post_len]: the initial posterior; post_out: the posterior after the last M-step (may be
// post_in); post_estep / stats (or null): the posterior at the last E-step and its
// statistics; LLs (or null): [max_iter], entries past the iteration count untouched.  w is
// sized for the subject; on return w.gamma holds the last E-step's gamma.  gamma_only:
// prelude + phase A once, nothing but w.gamma written.  Returns the iteration count; the
// bound and the status are r.L and status_of(r.flags).
template <int KM, class Lanes>
VBE_HD inline int run_em(const Lanes lanes, Run<KM> &r, int K, int dim, const Subject &s, const Hyper &h,
                         int max_iter, double min_diff, const double *post_in, double *post_out,
                         double *post_estep, double *stats, double *LLs, const Work<KM> &w, bool gamma_only) {
  const int PL = post_len(KM, dim), SL = stats_len(KM, dim), N = s.N, base = s.off[0];
  lanes.each(PL, [&](int x) { r.post[x] = post_in[x]; });
  lanes.each(SL, [&](int x) { r.stats[x] = 0.0; });
  if (lanes.first()) {
    r.K = K;
    r.dim = dim;
    r.L = r.lastL = -1.7976931348623157e308;
    r.flags = 0;
  }
  lanes.sync();
  int it = 1;
  for (; it <= max_iter; ++it) {
    lanes.once(K, [&](int k) { prelude_state(r, k); });
    lanes.sync();
    lanes.each(N, [&](int n) {
      const int q = s.off[n] - base, T = s.off[n + 1] - s.off[n];
      fb_sequence<KM>(r, s.x + (size_t)s.off[n] * dim, T, w.gamma + (size_t)q * KM, w.logrho + (size_t)q * KM,
                      w.cs + q, w.mxs + q, w.seq + (size_t)n * seq_len(KM));
    });
    if (gamma_only) return it;
    lanes.sync();
    lanes.once(K, [&](int k) { stat_counts(r, s, w, k); });
    lanes.once(KM * KM, [&](int e) {
      if (e / KM < K && e % KM < K) stat_trans(r, s, w, e / KM, e % KM);
    });
    lanes.sync();
    lanes.once(K * dim, [&](int e) { stat_mean(r, s, w, e / dim, e % dim); });
    lanes.sync();
    lanes.each(K * dim * dim, [&](int e) { stat_cov(r, s, w, e / (dim * dim), (e / dim) % dim, e % dim); });
    lanes.sync();
    lanes.once(K, [&](int k) { bound_state(r, h, k); });
    lanes.sync();
    if (lanes.first()) {
      loop_control(r, bound_total(r, h, N, w.seq), it, max_iter, min_diff);
      if (LLs) LLs[it - 1] = r.L;
    }
    lanes.sync();
    const int flags = r.flags;
    if (flags & 1) {  // the last E-step: its posterior and statistics
      if (post_estep) lanes.each(PL, [&](int x) { post_estep[x] = r.post[x]; });
      if (stats) lanes.each(SL, [&](int x) { stats[x] = r.stats[x]; });
    }
    if (flags & 4) break;
    lanes.sync();
    lanes.once(K, [&](int k) { mstep_state(r, h, k); });
    lanes.sync();
    if (flags & 1) break;
  }
  lanes.each(PL, [&](int x) { post_out[x] = r.post[x]; });
  return it > max_iter ? max_iter : it;
}

// ---- one whole run, unit after unit (host builds only).  post [post_len]: the initial
// posterior in, the posterior after the last M-step out; the rest as run_em's.
template <int KM>
inline RunResult run_serial(int K, int dim, const Subject &s, const Hyper &h, int max_iter, double min_diff,
                            double *post, double *post_estep, double *stats, double *LLs, const Work<KM> &w) {
  Run<KM> r;
  const int iters =
      run_em<KM>(SerialLanes{}, r, K, dim, s, h, max_iter, min_diff, post, post, post_estep, stats, LLs, w, false);
  return RunResult{r.L, iters, status_of(r.flags)};
}

}  // namespace emrun
}  // namespace vbhem
