// vbhmm_ppk_pair.h -- the arithmetic of the probability product kernel between two
// point HMMs (include/vbhmm_ppk.h; the reference's src/compare_mtds/ppk/elkernel.m
// and bhatt.m), written once for the device kernels (vbhmm_ppk.hip) and for a host
// build (tests/ppkcheck):
//   prepare_state   a state's regularised covariance C = cov + pad (every entry),
//                   C += 1e-5 trace(C) I, packed; 1/4 logdet C from its Cholesky
//                   factor; prior, prior^rho, trans^rho
//   state_pot       the Bhattacharyya affinity of two states in the difference form:
//                   C1 + C2 = R'R (one reciprocal root per column), y = R' \ (mu1 - mu2),
//                   pot = exp(d/2 ln 2 + 1/4 logdet C1 + 1/4 logdet C2
//                             - sum log diag R - |y|^2 / 4)
//   load_col / dot_col   one entry of (A^rho)' W and of Y (B^rho), the two small
//                   products of a step of elkernel.m:28-54, from a column of
//                   trans^rho kept in registers
//   pair_kernel     the whole recursion over plain arrays (the host loop; the kernel
//                   spreads the same calls over the lanes of a state-pair grid)
// Plain IEEE fp64, no log domain: far-apart HMMs underflow to tiny values or 0.
//
// A prepared HMM is one block of doubles (Layout): state count [1], prior [KM],
// prior^rho [KM], trans^rho [KM][KM], mean [KM][DB], packed upper triangle of C
// [KM][DB (DB + 1) / 2] (entry (i, j), i <= j, at j (j + 1) / 2 + i), 1/4 logdet C
// [KM].  Past the dimension d the means are 0 and C has 0.5 on the diagonal, so that
// C1 + C2 is the identity there and the unrolled loops over DB need no guard.  States
// past the HMM's own count hold zeros and are never read from the inputs.
#pragma once
#include <cmath>

#include "vbhmm_score_pair.h"

namespace vbhem {
namespace ppk {

using score::dim_bucket;
using score::kMaxDim;
using score::kMaxStates;
using score::packed_at;
using score::packed_len;
using score::state_bucket;

constexpr double kHalfLn2 = 0.34657359027997265470861606072909;
constexpr double kLn2 = 0.69314718055994530941723212145818;
constexpr double kTraceReg = 1e-5;  // bhatt.m:15-16

struct Layout {
  int KM, DB, NP;
  int nst, prior, prho, trho, mean, cov, qld, stride;  // offsets / block length in doubles
};

VBS_HD inline Layout make_layout(int KM, int d) {
  Layout L;
  L.KM = KM;
  L.DB = dim_bucket(d);
  L.NP = packed_len(L.DB);
  L.nst = 0;
  L.prior = 1;
  L.prho = L.prior + KM;
  L.trho = L.prho + KM;
  L.mean = L.trho + KM * KM;
  L.cov = L.mean + KM * L.DB;
  L.qld = L.cov + KM * L.NP;
  L.stride = (L.qld + KM + 1) / 2 * 2;
  return L;
}

// the largest block of a (state bucket, dimension bucket) pair
template <int KB, int DB>
struct BlockLen {
  static constexpr int value = (1 + 3 * KB + KB * KB + KB * DB + KB * packed_len(DB) + 1) / 2 * 2;
};

// x^rho with 0^rho = 0
VBS_HD inline double pow_rho(double x, double rho) { return x == 0.0 ? 0.0 : pow(x, rho); }

// 1 / sqrt(x) for a positive pivot
VBS_HD inline double rsqrt_pos(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return rsqrt(x);
#else
  return 1.0 / sqrt(x);
#endif
}

// Upper Cholesky factor of the packed matrix R (in place, columns in order).  Only
// the strict upper triangle is finished: the diagonal is left as the pivots s_j =
// R_jj^2 in pv, with ri[j] = 1 / R_jj (no square root or division is needed beyond
// one reciprocal root per column).  false: a pivot is not positive.
template <int DB>
VBS_HD inline bool chol_packed(double (&R)[packed_len(DB)], double (&ri)[DB], double (&pv)[DB]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < DB; ++j) {
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double s = R[packed_at(i, j)];
#pragma unroll
      for (int q = 0; q < i; ++q) s -= R[packed_at(q, i)] * R[packed_at(q, j)];
      if (i == j) {
        if (!(s > 0.0)) ok = false;
        pv[j] = s;
        ri[j] = rsqrt_pos(s);
      } else {
        R[packed_at(i, j)] = s * ri[i];
      }
    }
  }
  return ok;
}

// sum_{c < d} log R_cc = 1/2 log prod pv_c, with one log: the pivots' mantissas
// (in [0.5, 1), so their product cannot leave the range) and the sum of their exponents
template <int DB>
VBS_HD inline double sum_log_diag(const double (&pv)[DB], int d) {
  double m = 1.0;
  int E = 0;
#pragma unroll
  for (int c = 0; c < DB; ++c)
    if (c < d) {
      int e;
      m *= frexp(pv[c], &e);
      E += e;
    }
  return 0.5 * (log(m) + E * kLn2);
}

// State k of one HMM into its prepared block.  prior [KM], trans [KM][KM], mean
// [KM][d], cov [KM][d][d] (upper triangle read) or [KM][d] (diag) are that HMM's
// arrays.  false: the regularised covariance is not positive definite.
template <int DB>
VBS_HD inline bool prepare_state(const Layout &L, double *blk, int k, int K, int d, bool diag,
                                 double rho, double pad, const double *prior, const double *trans,
                                 const double *mean, const double *cov) {
  constexpr int NP = packed_len(DB);
  const int KM = L.KM;
  double *mu = blk + L.mean + k * DB, *cp = blk + L.cov + k * NP;
  if (k == 0) blk[L.nst] = (double)K;
  if (k >= K) {  // padding: never read from the inputs, kept finite
    blk[L.prior + k] = 0.0;
    blk[L.prho + k] = 0.0;
    blk[L.qld + k] = 0.0;
    for (int j = 0; j < KM; ++j) blk[L.trho + k * KM + j] = 0.0;
    for (int a = 0; a < DB; ++a) mu[a] = 0.0;
    for (int q = 0; q < NP; ++q) cp[q] = 0.0;
    return true;
  }
  blk[L.prior + k] = prior[k];
  blk[L.prho + k] = pow_rho(prior[k], rho);
  for (int j = 0; j < KM; ++j) blk[L.trho + k * KM + j] = j < K ? pow_rho(trans[k * KM + j], rho) : 0.0;
#pragma unroll
  for (int a = 0; a < DB; ++a) mu[a] = a < d ? mean[k * d + a] : 0.0;
  double C[NP], ri[DB], pv[DB], tr = 0.0;
#pragma unroll
  for (int j = 0; j < DB; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double c = i == j ? 0.5 : 0.0;
      if (j < d) {
        if (diag)
          c = (i == j ? cov[k * d + j] : 0.0) + pad;
        else
          c = cov[((size_t)k * d + i) * d + j] + pad;
        if (i == j) tr += c;
      }
      C[packed_at(i, j)] = c;
    }
  const double reg = kTraceReg * tr;
#pragma unroll
  for (int j = 0; j < DB; ++j)
    if (j < d) C[packed_at(j, j)] += reg;
#pragma unroll
  for (int q = 0; q < NP; ++q) cp[q] = C[q];
  const bool ok = chol_packed<DB>(C, ri, pv);
  blk[L.qld + k] = ok ? 0.5 * sum_log_diag<DB>(pv, d) : 0.0;  // logdet C = 2 sum log diag R
  return ok;
}

// a prepared block, as the pair routines read it (LDS on the device)
struct Hmm {
  const double *prior, *prho, *trho, *mean, *cov, *qld;
  int K, KM;
};

VBS_HD inline Hmm view(const Layout &L, const double *blk) {
  Hmm m;
  m.prior = blk + L.prior;
  m.prho = blk + L.prho;
  m.trho = blk + L.trho;
  m.mean = blk + L.mean;
  m.cov = blk + L.cov;
  m.qld = blk + L.qld;
  m.K = (int)blk[L.nst];
  m.KM = L.KM;
  return m;
}

// Bhattacharyya affinity of state i of a and state j of b (d the true dimension)
template <int DB>
VBS_HD inline double state_pot(const Hmm &a, int i, const Hmm &b, int j, int d) {
  constexpr int NP = packed_len(DB);
  const double *c1 = a.cov + i * NP, *c2 = b.cov + j * NP;
  const double *m1 = a.mean + i * DB, *m2 = b.mean + j * DB;
  double R[NP], ri[DB], pv[DB], y[DB];
#pragma unroll
  for (int q = 0; q < NP; ++q) R[q] = c1[q] + c2[q];
  chol_packed<DB>(R, ri, pv);
  double q4 = 0.0;
#pragma unroll
  for (int c = 0; c < DB; ++c) {  // R' y = mu1 - mu2
    double s = m1[c] - m2[c];
#pragma unroll
    for (int r = 0; r < c; ++r) s -= R[packed_at(r, c)] * y[r];
    y[c] = s * ri[c];
    q4 += y[c] * y[c];
  }
  return exp(d * kHalfLn2 + a.qld[i] + b.qld[j] - sum_log_diag<DB>(pv, d) - 0.25 * q4);
}

// Column c of m's trans^rho, v[q] = trans^rho(q, c) for q < K and 0 past it (off: all 0):
// what one entry of either product of a step needs of its HMM, kept for all T steps
template <int KB>
VBS_HD inline void load_col(const Hmm &m, int c, bool on, double (&v)[KB]) {
#pragma unroll
  for (int q = 0; q < KB; ++q) v[q] = on && q < m.K ? m.trho[q * m.KM + c] : 0.0;
}

// sum_q v[q] P[q stride]: with v a column of A^rho and P = &W(0, j), stride the row
// length, ((A^rho)' W)(ip, j); with v a column of B^rho and P = &Y(ip, 0), stride 1,
// (Y B^rho)(ip, jp).  Every P[q stride], q < KB, must be initialised (0 past the states).
template <int KB>
VBS_HD inline double dot_col(const double (&v)[KB], const double *P, int stride) {
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < KB; ++q) s += v[q] * P[q * stride];
  return s;
}

// sum of row i of W over the columns j < n, then of the row sums: the order of the
// kernel's final reduction
VBS_HD inline double row_sum(const double *W, int ld, int i, int n) {
  double s = 0.0;
  for (int j = 0; j < n; ++j) s += W[i * ld + j];
  return s;
}

// The kernel between two prepared HMMs over plain arrays: elkernel.m:19-54 with
// T + 1 factors of pot (T == 1: p' pot r, no rho).
template <int KB, int DB>
VBS_HD inline double pair_kernel(const Hmm &a, const Hmm &b, int d, int T) {
  double pot[KB * KB], X[KB * KB], Y[KB * KB], rs[KB], v[KB];
  const int M = a.K, N = b.K;
  for (int e = 0; e < KB * KB; ++e) pot[e] = X[e] = Y[e] = 0.0;
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      pot[i * KB + j] = state_pot<DB>(a, i, b, j, d);
      X[i * KB + j] = (T == 1 ? a.prior[i] * b.prior[j] : a.prho[i] * b.prho[j]) * pot[i * KB + j];
    }
  for (int t = 0; t < T && T > 1; ++t) {
    for (int i = 0; i < M; ++i) {
      load_col<KB>(a, i, true, v);
      for (int j = 0; j < N; ++j) Y[i * KB + j] = dot_col<KB>(v, X + j, KB);
    }
    for (int j = 0; j < N; ++j) {
      load_col<KB>(b, j, true, v);
      for (int i = 0; i < M; ++i) X[i * KB + j] = dot_col<KB>(v, Y + i * KB, 1) * pot[i * KB + j];
    }
  }
  for (int i = 0; i < M; ++i) rs[i] = row_sum(X, KB, i, N);
  return row_sum(rs, 0, 0, M);
}

// f.template operator()<KB, DB>() for the buckets of (KM, d)
template <class F>
inline auto dispatch(int KM, int d, F &&f) {
  return score::dispatch(KM, d, static_cast<F &&>(f));
}

}  // namespace ppk
}  // namespace vbhem
