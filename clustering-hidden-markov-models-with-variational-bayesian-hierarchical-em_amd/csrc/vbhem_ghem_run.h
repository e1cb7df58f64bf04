// vbhem_ghem_run.h -- the arithmetic of the hierarchical EM behind the 'gmmNew'
// initialisation (include/vbhem_init.h), written once for the device kernels
// (vbhem_ghem.hip) and for a host build (tests/ghemcheck, and any C++ compiler: the serial
// part needs no device compiler).  It restates h3m.gmm_mix_hier_em for T >= 2:
//   seeding   kmeans_pp over all n points for T centres from injected draws
//             (wtkrun::kmeans_pp_serial / block_kmeans_pp), or given centres
//   start     vr_t = the mean (full) or the maximum (diagonal) of the points' covariances
//             (scan_*: once per call, the same for every trial), mxwt_t = 1 / T
//   E-step    xpt[t][n] in the reference's forms (estep_point), the column log-sum-exp
//             with its maximum, logpost = xpt - lx, logp = (sum_n lx) / n
//   stop      logp not finite, or logp - last < 1e-6: the parameters stay, the trial ends
//             with THIS E-step's logpost; otherwise last = logp and the M-step runs
//   M-step    mxwt = (sum_n post) / n; with wp = post * (1 / n): cent_t = (sum_n wp x_n) /
//             (sum_n wp), then vr_t = (sum_n wp ((x_n - c_t)(x_n - c_t)' + C_n)) / (sum_n wp)
//             about the NEW centre (a second pass over the points; never the expanded
//             second-moment form).  The reference divides wp by its sum before it sums;
//             here the sums are divided: a rounding apart.
//   prepare   ivr_t and log|vr_t| by Cholesky (emrun::chol_inplace, spd_inverse_inplace);
//             diagonal: 1 / vr and nrm_t = sum_a (c c ivr + log vr).  A pivot <= 0 ends the
//             trial SINGULAR; a non-finite vr_t is passed on as NaN (numpy's inverse does
//             the same), so the next E-step ends the trial NONFINITE.  After the last of
//             `iterations` rounds nothing is prepared, as in the reference.
// Every n-term sum runs over point tiles of tile_points(n, d) points and the tile partials
// are added in tile order.  The units are one POINT of one trial (estep_point, cov_term)
// and one COMPONENT (prepare_component); the serial walker (fit_serial) sums a tile's points
// in point order.  The kernels sum the E-step's statistics of 256 points in a fixed tree
// and the covariance terms in point order, so a trial's result depends on its own inputs
// alone; it differs from the walker's by the order of n-term sums and by exp and log.
#pragma once
#include "vbhmm_em_run.h"  // emrun::chol_inplace, spd_inverse_inplace (before the pragma below)
#include "vbhem_wtk_run.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vbhem {
namespace ghemrun {

using wtkrun::finite_d;
using wtkrun::kBlock;
using wtkrun::kWaves;

constexpr int kMaxDim = 16, kMaxT = 32;
constexpr int kOk = 0, kDegenerate = 1, kBad = 2, kNonfinite = 3, kSingular = 4;
constexpr int kGroup = 8;  // the trials a pass block loops over with its tile's points
constexpr int kAcc = 8;    // covariance entries a thread accumulates per walk of its tile
constexpr double kStop = 1e-6;
constexpr double kLn2Pi = 1.83787706640934548356;

// the point tile of every n-term sum: a function of (n, d) only.  256 points (one per
// thread of the E-step) while that makes at most 1,024 tiles, whose partials the finish
// kernels add serially; 1,024 points beyond.
WTK_HD constexpr int tile_points(int n, int /*d*/) { return n <= 262144 ? 256 : 1024; }
WTK_HD constexpr int tiles_of(int n, int d) { return (n + tile_points(n, d) - 1) / tile_points(n, d); }
WTK_HD constexpr int cov_len(int d, bool full) { return full ? d * d : d; }
// the E-step's sums of one trial: [t][0..d-1] sum wp x, [t][d] sum wp, [t][d+1] sum post;
// the last entry: sum lx
WTK_HD constexpr int ea_len(int T, int d) { return T * (d + 2) + 1; }

// A trial's state: the parameters (mx, cen, vr), what the E-step reads (logmx, ecen, ivr,
// cst: log|vr| or nrm), sum wp, (last, logp) and four ints (done, status, E-steps, Lloyd).
WTK_HD constexpr size_t slot_len(int T, int d, int cd) { return (size_t)T * (5 + 2 * d + 2 * cd) + 4; }
struct Slot {
  double *mx, *cen, *vr, *logmx, *ecen, *ivr, *cst, *sw, *sc;
  int *flag;
};
enum { fDone, fStatus, fEsteps, fLloyd };
WTK_HD inline Slot slot_at(double *p, int T, int d, int cd) {
  Slot s;
  s.mx = p;
  s.cen = s.mx + T;
  s.vr = s.cen + (size_t)T * d;
  s.logmx = s.vr + (size_t)T * cd;
  s.ecen = s.logmx + T;
  s.ivr = s.ecen + (size_t)T * d;
  s.cst = s.ivr + (size_t)T * cd;
  s.sw = s.cst + T;
  s.sc = s.sw + T;
  s.flag = reinterpret_cast<int *>(s.sc + 2);
  return s;
}

struct EParams {
  int T, d;
  bool full;
  double coef;
  const double *logmx, *cen, *ivr, *cst;
};
WTK_HD inline EParams eparams_of(const Slot &s, int T, int d, bool full) {
  return EParams{T, d, full, -(d / 2.0) * kLn2Pi, s.logmx, s.ecen, s.ivr, s.cst};
}

// One point's column of the E-step: logpost[t] into out[t * stride], lx returned.
WTK_HD inline double estep_point(const EParams &m, const double *x, const double *C, double dpp, double *out,
                                 size_t stride) {
  const int d = m.d;
  double mv = -INFINITY;
  for (int t = 0; t < m.T; ++t) {
    const double *c = m.cen + (size_t)t * d;
    double v;
    if (m.full) {
      const double *iv = m.ivr + (size_t)t * d * d;
      double trc = 0.0, quad = 0.0;
      for (int a = 0; a < d; ++a) {
        const double da = c[a] - x[a];
        double row = 0.0;
        for (int b = 0; b < d; ++b) {
          trc += iv[a * d + b] * C[a * d + b];
          row += iv[a * d + b] * (c[b] - x[b]);
        }
        quad += da * row;
      }
      v = m.logmx[t] + dpp * (m.coef - 0.5 * ((trc + quad) + m.cst[t]));
    } else {
      const double *iv = m.ivr + (size_t)t * d;
      double A = 0.0, B = 0.0, trc = 0.0;
      for (int a = 0; a < d; ++a) {
        A += iv[a] * (x[a] * x[a]);
        B += (c[a] * iv[a]) * x[a];
        trc += iv[a] * C[a];
      }
      v = m.logmx[t] + dpp * (m.coef - 0.5 * (((A - 2.0 * B) + m.cst[t]) + trc));
    }
    out[(size_t)t * stride] = v;
    if (v > mv) mv = v;
  }
  double s = 0.0;
  for (int t = 0; t < m.T; ++t) s += exp(out[(size_t)t * stride] - mv);
  const double lx = mv + log(s);
  for (int t = 0; t < m.T; ++t) out[(size_t)t * stride] -= lx;
  return lx;
}

// One term of vr_t[a][b] (diagonal: a == b, ab = a): wp ((x - c)(x - c)' + C)
WTK_HD inline double cov_term(double wp, const double *x, const double *C, double ca, double cb, int a, int b, int ab) {
  return wp * ((x[a] - ca) * (x[b] - cb) + C[ab]);
}

// The stopping rule on a trial's sum of lx.  Returns true when the trial ends here.
WTK_HD inline bool stop_rule(const Slot &s, double sumlx, int n) {
  const double logp = sumlx / n;
  s.sc[1] = logp;
  s.flag[fEsteps] += 1;
  if (!finite_d(logp) || logp - s.sc[0] < kStop) {
    s.flag[fStatus] = finite_d(logp) ? kOk : kNonfinite;
    s.flag[fDone] = 1;
    return true;
  }
  s.sc[0] = logp;
  return false;
}

// Component t of `prepare`; A, B: scratch [cd].  Returns 1 on a pivot <= 0.
WTK_HD inline int prepare_component(const Slot &s, int t, int d, bool full, double *A, double *B) {
  const int cd = cov_len(d, full);
  const double *vr = s.vr + (size_t)t * cd;
  double *ivr = s.ivr + (size_t)t * cd;
  s.logmx[t] = log(s.mx[t]);
  for (int a = 0; a < d; ++a) s.ecen[(size_t)t * d + a] = s.cen[(size_t)t * d + a];
  bool fin = true;
  for (int e = 0; e < cd; ++e) fin = fin && finite_d(vr[e]);
  if (!fin) {
    for (int e = 0; e < cd; ++e) ivr[e] = NAN;
    s.cst[t] = NAN;
    return 0;
  }
  if (!full) {
    for (int a = 0; a < d; ++a)
      if (!(vr[a] > 0.0)) return 1;
    double nrm = 0.0;
    for (int a = 0; a < d; ++a) {
      const double c = s.cen[(size_t)t * d + a];
      ivr[a] = 1.0 / vr[a];
      nrm += (c * c) * ivr[a] + log(vr[a]);
    }
    s.cst[t] = nrm;
    return 0;
  }
  for (int e = 0; e < cd; ++e) A[e] = B[e] = vr[e];
  const double logdet = emrun::chol_inplace(B, d);
  if (!finite_d(logdet)) return 1;  // sqrt or log of a pivot that is not > 0
  emrun::spd_inverse_inplace(A, d);
  for (int e = 0; e < cd; ++e) ivr[e] = A[e];
  s.cst[t] = logdet;
  return 0;
}

// ---------------------------------------------------------------------------------------
// the serial walkers
// ---------------------------------------------------------------------------------------
// vr0 [cd] and whether every coordinate and covariance entry is finite; part: scratch [cd]
WTK_HD inline bool scan_serial(const double *X, const double *C, int n, int d, bool full, double *vr0, double *part) {
  const int cd = cov_len(d, full), P = tile_points(n, d);
  bool fin = true;
  for (size_t e = 0; e < (size_t)n * d; ++e) fin = fin && finite_d(X[e]);
  for (size_t e = 0; e < (size_t)n * cd; ++e) fin = fin && finite_d(C[e]);
  for (int e = 0; e < cd; ++e) vr0[e] = full ? 0.0 : -INFINITY;
  for (int p0 = 0; p0 < n; p0 += P) {
    const int p1 = p0 + P < n ? p0 + P : n;
    for (int e = 0; e < cd; ++e) {
      double v = full ? 0.0 : -INFINITY;
      for (int p = p0; p < p1; ++p) {
        const double c = C[(size_t)p * cd + e];
        v = full ? v + c : (c > v ? c : v);
      }
      part[e] = v;
    }
    for (int e = 0; e < cd; ++e) vr0[e] = full ? vr0[e] + part[e] : (part[e] > vr0[e] ? part[e] : vr0[e]);
  }
  if (full)
    for (int e = 0; e < cd; ++e) vr0[e] /= n;
  return fin;
}

// The start of a trial from the centres in s.cen: mxwt, vr, last and the counters.
WTK_HD inline void start_values(const Slot &s, int T, int d, int cd, const double *vr0, int lloyd) {
  for (int t = 0; t < T; ++t) {
    s.mx[t] = 1.0 / T;
    for (int e = 0; e < cd; ++e) s.vr[(size_t)t * cd + e] = vr0[e];
  }
  s.sc[0] = -1.7976931348623157e308;
  s.sc[1] = 0.0;
  s.flag[fDone] = 0;
  s.flag[fStatus] = kOk;
  s.flag[fEsteps] = 0;
  s.flag[fLloyd] = lloyd;
}

// `prepare` of every component; true (and the trial ended SINGULAR) on a failed pivot
WTK_HD inline bool prepare_serial(const Slot &s, int T, int d, bool full, double *A, double *B) {
  int sing = 0;
  for (int t = 0; t < T; ++t) sing |= prepare_component(s, t, d, full, A, B);
  if (sing) {
    s.flag[fStatus] = kSingular;
    s.flag[fDone] = 1;
  }
  return sing != 0;
}

// One trial.  slot: slot_len doubles; post [T][n]; tot, part [max(ea_len, T cd)]; A, B [cd];
// cold [T][d], sums [T][d+1], dmin [n], lab [n]: the seeding's scratch.  init: given centres
// [T][d] or null.  The trial's state is left in the slot; post holds the last E-step's
// posteriors (logpost_serial gives the log-posteriors).
WTK_HD inline void fit_serial(const double *X, const double *C, int n, int d, bool full, int T, double virtual_samples,
                              int iterations, int j0, const double *u, const double *init, const double *vr0,
                              bool finite, double *slot, double *post, double *tot, double *part, double *A, double *B,
                              double *cold, double *sums, double *dmin, int *lab) {
  const int cd = cov_len(d, full), P = tile_points(n, d), EA = ea_len(T, d), EB = T * cd;
  const Slot s = slot_at(slot, T, d, cd);
  s.flag[fDone] = 1;
  if (!finite || (!init && (j0 < 0 || j0 >= n))) {
    s.flag[fStatus] = kBad;
    return;
  }
  int lloyd = 0;
  if (init) {
    for (int e = 0; e < T * d; ++e) s.cen[e] = init[e];
  } else {
    const wtkrun::PPResult pp =
        wtkrun::kmeans_pp_serial(X, d, nullptr, n, T, j0, u, wtkrun::kLloydMax, s.cen, cold, sums, dmin, lab);
    if (pp.status != wtkrun::kOk) {
      s.flag[fStatus] = pp.status;
      return;
    }
    lloyd = pp.iters;
  }
  start_values(s, T, d, cd, vr0, lloyd);
  if (iterations < 1) {
    s.flag[fDone] = 1;
    return;
  }
  if (prepare_serial(s, T, d, full, A, B)) return;
  const double prior = 1.0 / n, dpp = prior * virtual_samples;
  for (int it = 0; it < iterations; ++it) {
    const EParams m = eparams_of(s, T, d, full);
    for (int e = 0; e < EA; ++e) tot[e] = 0.0;
    for (int p0 = 0; p0 < n; p0 += P) {
      const int p1 = p0 + P < n ? p0 + P : n;
      for (int e = 0; e < EA; ++e) part[e] = 0.0;
      for (int p = p0; p < p1; ++p) {
        const double *x = X + (size_t)p * d;
        part[EA - 1] += estep_point(m, x, C + (size_t)p * cd, dpp, post + p, (size_t)n);
        for (int t = 0; t < T; ++t) {
          const double po = exp(post[(size_t)t * n + p]), wp = po * prior;
          post[(size_t)t * n + p] = po;
          double *q = part + t * (d + 2);
          for (int a = 0; a < d; ++a) q[a] += wp * x[a];
          q[d] += wp;
          q[d + 1] += po;
        }
      }
      for (int e = 0; e < EA; ++e) tot[e] += part[e];
    }
    if (stop_rule(s, tot[EA - 1], n)) return;
    for (int t = 0; t < T; ++t) {
      const double *q = tot + t * (d + 2);
      s.mx[t] = q[d + 1] / n;
      s.sw[t] = q[d];
      for (int a = 0; a < d; ++a) s.cen[(size_t)t * d + a] = q[a] / q[d];
    }
    for (int e = 0; e < EB; ++e) tot[e] = 0.0;
    for (int p0 = 0; p0 < n; p0 += P) {
      const int p1 = p0 + P < n ? p0 + P : n;
      for (int e = 0; e < EB; ++e) {
        const int t = e / cd, ab = e % cd, a = full ? ab / d : ab, b = full ? ab % d : ab;
        const double ca = s.cen[(size_t)t * d + a], cb = s.cen[(size_t)t * d + b];
        double v = 0.0;
        for (int p = p0; p < p1; ++p)
          v += cov_term(post[(size_t)t * n + p] * prior, X + (size_t)p * d, C + (size_t)p * cd, ca, cb, a, b, ab);
        tot[e] += v;
      }
    }
    for (int e = 0; e < EB; ++e) s.vr[e] = tot[e] / s.sw[e / cd];
    if (it == iterations - 1) {
      s.flag[fDone] = 1;
      return;
    }
    if (prepare_serial(s, T, d, full, A, B)) return;
  }
}

// The log-posteriors [T][n] of an OK trial: the E-step the trial ended with, evaluated
// again from what it read (zeros when no E-step was evaluated).
WTK_HD inline void logpost_serial(const double *X, const double *C, int n, int d, bool full, int T,
                                  double virtual_samples, double *slot, double *logpost) {
  const int cd = cov_len(d, full);
  const Slot s = slot_at(slot, T, d, cd);
  const EParams m = eparams_of(s, T, d, full);
  const double dpp = (1.0 / n) * virtual_samples;
  for (int p = 0; p < n; ++p) {
    if (s.flag[fEsteps] > 0)
      estep_point(m, X + (size_t)p * d, C + (size_t)p * cd, dpp, logpost + p, (size_t)n);
    else
      for (int t = 0; t < T; ++t) logpost[(size_t)t * n + p] = 0.0;
  }
}

}  // namespace ghemrun
}  // namespace vbhem
