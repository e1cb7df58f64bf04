// vbhmm_score_pair.h -- the arithmetic of scoring one observation sequence under
// one point HMM (include/vbhmm_score.h), written once for the device kernels
// (vbhmm_score.hip) and for a host build (tests/scorecheck):
//   prepare_state   Cholesky of a state's covariance, packed inverse factor,
//                   log-normaliser (MATLAB's mvnpdf: cov = R'R, q = |(x - mean) / R|^2,
//                   rho = exp(-q/2 - sum log diag R - d log(2 pi)/2))
//   densities       rho(t, .) of one observation, with vbhmm_ll.m:70-72's zero floor
//   pair_loglik     the scaled forward pass of vbhmm_ll.m:83-102
//   pair_viterbi    viterbi_path / normalize of vbhmm_map_state.m:41-138, back-pointers
//                   and backtrack included
// Plain IEEE fp64: no clamp, no log-domain rescue; denormals are kept.
//
// A prepared HMM is one block of doubles (Layout): prior [KM], trans [KM][KM],
// mean [KM][DB], packed upper-triangular R^-1 [KM][DB (DB + 1) / 2] (entry (i, j),
// i <= j, at j (j + 1) / 2 + i), log-normaliser [KM], state count [1]; KM = the
// padded state count of the set, DB = the dimension bucket (2, 4, 8).  Means and
// factors are zero past the dimension, so the unrolled loops over DB need no guard;
// states past the HMM's own count are never read (every loop is bounded by K).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBS_HD __host__ __device__
#else
#define VBS_HD
#endif

namespace vbhem {
namespace score {

constexpr int kMaxStates = 16;
constexpr int kMaxDim = 8;
constexpr double kHalfLog2Pi = 0.91893853320467274178032973640562;
// vbhmm_ll.m:71: the literal 4.9407e-323 read as a double = 10 * 2^-1074 (bits 0x...0A)
constexpr double kRhoFloor = 0x0.000000000000Ap-1022;

VBS_HD constexpr int state_bucket(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : 16; }
VBS_HD constexpr int dim_bucket(int d) { return d <= 2 ? 2 : d <= 4 ? 4 : 8; }
VBS_HD constexpr int packed_len(int db) { return db * (db + 1) / 2; }
VBS_HD constexpr int packed_at(int i, int j) { return j * (j + 1) / 2 + i; }  // i <= j

struct Layout {
  int KM, DB, NP;
  int prior, trans, mean, rinv, lnorm, nst, stride;  // offsets / block length in doubles
};

VBS_HD inline Layout make_layout(int KM, int d) {
  Layout L;
  L.KM = KM;
  L.DB = dim_bucket(d);
  L.NP = packed_len(L.DB);
  L.prior = 0;
  L.trans = L.prior + KM;
  L.mean = L.trans + KM * KM;
  L.rinv = L.mean + KM * L.DB;
  L.lnorm = L.rinv + KM * L.NP;
  L.nst = L.lnorm + KM;
  L.stride = (L.nst + 1 + 1) / 2 * 2;
  return L;
}

// the largest block of a (state bucket, dimension bucket) pair
template <int KB, int DB>
struct BlockLen {
  static constexpr int value = (2 * KB + KB * KB + KB * DB + KB * packed_len(DB) + 2) / 2 * 2;
};

// State k of one HMM into its prepared block.  prior [KM], trans [KM][KM], mean
// [KM][d], cov [KM][d][d] (upper triangle read, as chol does) or [KM][d] (diag) are
// that HMM's arrays.  false: the covariance is not positive definite.
VBS_HD inline bool prepare_state(const Layout &L, double *blk, int k, int K, int d, bool diag,
                                 const double *prior, const double *trans, const double *mean,
                                 const double *cov) {
  const int KM = L.KM;
  double *mu = blk + L.mean + k * L.DB, *rv = blk + L.rinv + k * L.NP;
  if (k == 0) blk[L.nst] = (double)K;
  for (int a = 0; a < L.DB; ++a) mu[a] = 0.0;
  for (int q = 0; q < L.NP; ++q) rv[q] = 0.0;
  if (k >= K) {  // padding: never read, kept finite
    blk[L.prior + k] = 0.0;
    blk[L.lnorm + k] = 0.0;
    for (int j = 0; j < KM; ++j) blk[L.trans + k * KM + j] = 0.0;
    return true;
  }
  blk[L.prior + k] = prior[k];
  for (int j = 0; j < KM; ++j) blk[L.trans + k * KM + j] = j < K ? trans[k * KM + j] : 0.0;
  for (int a = 0; a < d; ++a) mu[a] = mean[k * d + a];
  double logdet = 0.0;
  bool ok = true;
  if (diag) {
    const double *c = cov + k * d;
    for (int a = 0; a < d; ++a) {
      if (!(c[a] > 0.0)) ok = false;
      const double r = sqrt(c[a]);
      rv[packed_at(a, a)] = 1.0 / r;
      logdet += log(r);
    }
  } else {
    const double *C = cov + k * d * d;
    // upper Cholesky factor, column by column, into rv
    for (int j = 0; j < d; ++j)
      for (int i = 0; i <= j; ++i) {
        double s = C[i * d + j];
        for (int q = 0; q < i; ++q) s -= rv[packed_at(q, i)] * rv[packed_at(q, j)];
        if (i == j) {
          if (!(s > 0.0)) ok = false;
          rv[packed_at(j, j)] = sqrt(s);
        } else {
          rv[packed_at(i, j)] = s / rv[packed_at(i, i)];
        }
      }
    for (int j = 0; j < d; ++j) logdet += log(rv[packed_at(j, j)]);
    // R^-1 in place: column j needs the finished columns before it and R's column j
    // from row i down, so ascending i may overwrite as it goes
    for (int j = 0; j < d; ++j) {
      const double rjj = rv[packed_at(j, j)];
      for (int i = 0; i < j; ++i) {
        double s = 0.0;
        for (int q = i; q < j; ++q) s += rv[packed_at(i, q)] * rv[packed_at(q, j)];
        rv[packed_at(i, j)] = -s / rjj;
      }
      rv[packed_at(j, j)] = 1.0 / rjj;
    }
  }
  blk[L.lnorm + k] = -logdet - d * kHalfLog2Pi;
  return ok;
}

// a prepared block, as the recursions read it (LDS on the device)
struct Hmm {
  const double *prior, *trans, *mean, *rinv, *lnorm;
  int K, KM;
  bool diag;
};

VBS_HD inline Hmm view(const Layout &L, const double *blk, bool diag) {
  Hmm m;
  m.prior = blk + L.prior;
  m.trans = blk + L.trans;
  m.mean = blk + L.mean;
  m.rinv = blk + L.rinv;
  m.lnorm = blk + L.lnorm;
  m.K = (int)blk[L.nst];
  m.KM = L.KM;
  m.diag = diag;
  return m;
}

// rho(k) = mvnpdf(x, mean_k, cov_k) for k < K (0 past K); floor: exact zeros become kRhoFloor
template <int KB, int DB>
VBS_HD inline void densities(const Hmm &m, const double *x, int d, bool floor, double (&rho)[KB]) {
  double xs[DB];
#pragma unroll
  for (int a = 0; a < DB; ++a) xs[a] = a < d ? x[a] : 0.0;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    double r = 0.0;
    if (k < m.K) {
      const double *mu = m.mean + k * DB, *rv = m.rinv + k * packed_len(DB);
      double q = 0.0;
      if (m.diag) {
#pragma unroll
        for (int j = 0; j < DB; ++j) {
          const double y = (xs[j] - mu[j]) * rv[packed_at(j, j)];
          q += y * y;
        }
      } else {
        double df[DB];
#pragma unroll
        for (int a = 0; a < DB; ++a) df[a] = xs[a] - mu[a];
#pragma unroll
        for (int j = 0; j < DB; ++j) {
          double y = 0.0;
#pragma unroll
          for (int i = 0; i <= j; ++i) y += df[i] * rv[packed_at(i, j)];
          q += y * y;
        }
      }
      r = exp(-0.5 * q + m.lnorm[k]);
      if (floor && r == 0.0) r = kRhoFloor;
    }
    rho[k] = r;
  }
}

// sum_t log c_t of the scaled forward pass (0 for an empty sequence)
template <int KB, int DB>
VBS_HD inline double pair_loglik(const Hmm &m, const double *x, int T, int d) {
  const int K = m.K, KM = m.KM;
  double al[KB], ll = 0.0;
  for (int t = 0; t < T; ++t) {
    double rho[KB], D[KB];
    densities<KB, DB>(m, x + (size_t)t * d, d, true, rho);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k) D[k] = k < K ? m.prior[k] * rho[k] : 0.0;
    } else {
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < KB; ++i)
          if (i < K && j < K) s += al[i] * m.trans[i * KM + j];
        D[j] = s * rho[j];
      }
    }
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < K) c += D[k];
#pragma unroll
    for (int k = 0; k < KB; ++k) al[k] = D[k] / c;
    ll += log(c);
  }
  return ll;
}

// The scaled Viterbi recursion.  bp: T rows of KB bytes (4-byte aligned), row t the
// best predecessor of every state at step t (row 0 unused); path: T 0-based states.
// Returns -sum_t log(1 / z_t).  Ties go to the lowest index (MATLAB's max).
template <int KB, int DB>
VBS_HD inline double pair_viterbi(const Hmm &m, const double *x, int T, int d, unsigned char *bp,
                                  int *path) {
  const int K = m.K, KM = m.KM;
  if (T < 1) return 0.0;
  double de[KB], ll = 0.0;
  for (int t = 0; t < T; ++t) {
    double rho[KB], D[KB];
    densities<KB, DB>(m, x + (size_t)t * d, d, false, rho);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k) D[k] = k < K ? m.prior[k] * rho[k] : 0.0;
    } else {
      uint32_t w[KB / 4];
#pragma unroll
      for (int q = 0; q < KB / 4; ++q) w[q] = 0u;
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        double best = 0.0;
        uint32_t arg = 0u;
        if (j < K) {
          best = de[0] * m.trans[j];
#pragma unroll
          for (int i = 1; i < KB; ++i)
            if (i < K) {
              const double v = de[i] * m.trans[i * KM + j];
              if (v > best) {
                best = v;
                arg = (uint32_t)i;
              }
            }
        }
        D[j] = best * rho[j];
        w[j / 4] |= arg << (8 * (j % 4));
      }
      uint32_t *row = reinterpret_cast<uint32_t *>(bp + (size_t)t * KB);
#pragma unroll
      for (int q = 0; q < KB / 4; ++q) row[q] = w[q];
    }
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < K) z += D[k];
    const double s = z + (z == 0.0 ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < KB; ++k) de[k] = D[k] / s;
    ll -= log(1.0 / z);
  }
  int cur = 0;
  double best = de[0];
#pragma unroll
  for (int k = 1; k < KB; ++k)
    if (k < K && de[k] > best) {
      best = de[k];
      cur = k;
    }
  path[T - 1] = cur;
  for (int t = T - 1; t >= 1; --t) {
    cur = bp[(size_t)t * KB + cur];
    path[t - 1] = cur;
  }
  return ll;
}

// f.template operator()<KB, DB>() for the buckets of (KM, d)
template <class F>
inline auto dispatch(int KM, int d, F &&f) {
  const int kb = state_bucket(KM), db = dim_bucket(d);
#define VBS_CASE(KB, DB) \
  if (kb == KB && db == DB) return f.template operator()<KB, DB>();
  VBS_CASE(4, 2) VBS_CASE(4, 4) VBS_CASE(4, 8)
  VBS_CASE(8, 2) VBS_CASE(8, 4) VBS_CASE(8, 8)
  VBS_CASE(16, 2) VBS_CASE(16, 4)
#undef VBS_CASE
  return f.template operator()<16, 8>();
}

}  // namespace score
}  // namespace vbhem
