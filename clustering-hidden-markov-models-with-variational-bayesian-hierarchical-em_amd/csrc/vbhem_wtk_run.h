// vbhem_wtk_run.h -- the arithmetic of the 'wtkmeans' initialisation (include/vbhem_init.h),
// written once for the device kernels (vbhem_wtk.hip) and for a host build (tests/wtkcheck,
// and any C++ compiler: the serial part needs no device compiler).  It restates h3m.py:
//   (a) kmeans_pp on a subset of the points (all of them, or the members of one cluster in
//       point order) with every draw injected: the first centre is member j0, centre c is
//       the first member whose running sum of d2 exceeds u[c-1] * total (numpy's
//       choice(n, p = d2 / total): one uniform draw and a right-sided search of the cdf);
//       total == 0 ends the run DEGENERATE.  Then at most max_iter Lloyd updates, stopped
//       when the labels repeat, an emptied cluster re-seeded with the member farthest from
//       its centre: by the distances of this iteration (the stale `dist`), the first of
//       equal maxima, the member's label changed in place so that later clusters of the
//       sweep and the next iteration's comparison see it.
//   (b) weighted_kmeans (my_weighted_kmeans.m): the first assignment by plain distance,
//       gcentroids (a weightless cluster: zero centre, cw = 0), genergy with cw / (cw - w),
//       the sweep with f for a member and dist * cw / (cw + w) for the others, the minimum
//       as h3m._nanargmin0 takes it (NaN counts as +Inf, the first of equal minima, all NaN:
//       cluster 0); x/0 and 0/0 are kept.  Stop on |dE| < 1e-6 or after it_max sweeps.
// The units are one POINT (dist2, nearest, wk_assign, wk_member_f); the serial walkers
// (kmeans_pp_serial, weighted_serial) loop over them and sum in point order.  The block
// routines (block_kmeans_pp, block_weighted; device compiler only) give the points to the
// kBlock threads of a workgroup in block strides and reduce in a fixed tree, so a run's
// result depends on its own inputs alone; it differs from the walker's by the order of the
// n-term sums.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WTK_HD __host__ __device__
#define WTK_UNROLL _Pragma("unroll")
#else
#define WTK_HD
#define WTK_UNROLL
#endif

// Products are rounded before they are summed, on the host and on the device alike.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vbhem {
namespace wtkrun {

constexpr int kMaxDim = 16, kMaxK = 32, kMaxS = 16;
constexpr int kLloydMax = 100, kWkMax = 100;
constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kOk = 0, kDegenerate = 1, kBad = 2;
constexpr double kWkTol = 1e-6;
constexpr int kNone = 0x7fffffff;

// the dimension bucket of a kernel instantiation and the clusters it sums at a time
WTK_HD constexpr int dim_bucket(int d) { return d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : 16; }
WTK_HD constexpr int group_of(int DB) { return DB <= 4 ? 8 : DB <= 8 ? 4 : 2; }

struct PPResult {
  int status, iters;
};
struct WKResult {
  int status, iters;  // iters: the sweeps counted by the reference's `it`
  double energy;      // the last energy computed
};

WTK_HD inline bool finite_d(double v) { return v - v == 0.0; }

// member m of a subset: point idx[m], or point m without a list
WTK_HD inline const double *point_of(const double *X, const int *idx, int m, int d) {
  return X + (size_t)(idx ? idx[m] : m) * d;
}

WTK_HD inline double dist2(const double *x, const double *c, int d) {
  double s = 0.0;
  for (int a = 0; a < d; ++a) {
    const double t = x[a] - c[a];
    s += t * t;
  }
  return s;
}

// np.argmin over the K centres: the first of equal minima
WTK_HD inline int nearest(const double *x, const double *cen, int K, int d, double *dmin) {
  int best = 0;
  double bv = dist2(x, cen, d);
  for (int j = 1; j < K; ++j) {
    const double v = dist2(x, cen + (size_t)j * d, d);
    if (v < bv) {
      bv = v;
      best = j;
    }
  }
  *dmin = bv;
  return best;
}

// genergy: a member's distance scaled by cw / (cw - w)
WTK_HD inline double wk_member_f(double fm, double cw, double w) { return fm * cw / (cw - w); }

// one column of the sweep matrix and its minimum (h3m._nanargmin0)
WTK_HD inline int wk_assign(const double *x, double w, int lab, double f, const double *cen, const double *cw, int K,
                            int d) {
  int best = 0;
  double bv = 0.0;
  for (int j = 0; j < K; ++j) {
    double v = j == lab ? f : dist2(x, cen + (size_t)j * d, d) * (cw[j] / (cw[j] + w));
    if (v != v) v = INFINITY;
    if (j == 0 || v < bv) {
      bv = v;
      best = j;
    }
  }
  return best;
}

// ---------------------------------------------------------------------------------------
// the serial walkers
// ---------------------------------------------------------------------------------------
WTK_HD inline bool points_finite_serial(const double *X, const int *idx, int n, int d, const double *w) {
  for (int m = 0; m < n; ++m) {
    const double *p = point_of(X, idx, m, d);
    for (int a = 0; a < d; ++a)
      if (!finite_d(p[a])) return false;
    if (w && !finite_d(w[idx ? idx[m] : m])) return false;
  }
  return true;
}

// sums[c][0..d-1] and the member count sums[c][d] of cluster c alone
WTK_HD inline void pp_sum_cluster(const double *X, const int *idx, int n, int d, const int *lab, int c, double *sums) {
  double *s = sums + (size_t)c * (d + 1);
  for (int a = 0; a <= d; ++a) s[a] = 0.0;
  for (int m = 0; m < n; ++m) {
    if (lab[m] != c) continue;
    const double *p = point_of(X, idx, m, d);
    for (int a = 0; a < d; ++a) s[a] += p[a];
    s[d] += 1.0;
  }
}

// (a) on the n members of a subset.  cen, cold [k][d]; sums [k][d+1]; dmin, lab [n].
// The caller has checked 1 <= k <= kMaxK, 1 <= d, 0 <= j0 < n and finite points.
WTK_HD inline PPResult kmeans_pp_serial(const double *X, int d, const int *idx, int n, int k, int j0, const double *u,
                                        int max_iter, double *cen, double *cold, double *sums, double *dmin,
                                        int *lab) {
  for (int a = 0; a < d; ++a) cen[a] = point_of(X, idx, j0, d)[a];
  for (int m = 0; m < n; ++m) dmin[m] = dist2(point_of(X, idx, m, d), cen, d);
  for (int c = 1; c < k; ++c) {
    double tot = 0.0;
    for (int m = 0; m < n; ++m) tot += dmin[m];
    if (!(tot > 0.0) || !finite_d(tot)) return PPResult{kDegenerate, 0};
    const double target = u[c - 1] * tot;
    int pick = n - 1;
    double run = 0.0;
    for (int m = 0; m < n; ++m) {
      run += dmin[m];
      if (run > target) {
        pick = m;
        break;
      }
    }
    double *cc = cen + (size_t)c * d;
    for (int a = 0; a < d; ++a) cc[a] = point_of(X, idx, pick, d)[a];
    for (int m = 0; m < n; ++m) {
      const double v = dist2(point_of(X, idx, m, d), cc, d);
      if (v < dmin[m]) dmin[m] = v;
    }
  }
  bool have = false;
  int iters = 0;
  for (int it = 0; it < max_iter; ++it) {
    for (int e = 0; e < k * d; ++e) cold[e] = cen[e];
    bool changed = !have;
    for (int m = 0; m < n; ++m) {
      double dm;
      const int l = nearest(point_of(X, idx, m, d), cen, k, d, &dm);
      if (have && l != lab[m]) changed = true;
      lab[m] = l;
      dmin[m] = dm;
    }
    ++iters;
    if (!changed) break;
    have = true;
    for (int c = 0; c < k; ++c) pp_sum_cluster(X, idx, n, d, lab, c, sums);
    for (int c = 0; c < k; ++c) {
      const double *s = sums + (size_t)c * (d + 1);
      double *cc = cen + (size_t)c * d;
      if (s[d] > 0.0) {
        for (int a = 0; a < d; ++a) cc[a] = s[a] / s[d];
        continue;
      }
      int far = 0;
      for (int m = 1; m < n; ++m)
        if (dmin[m] > dmin[far]) far = m;
      const int p = lab[far];
      const double *x = point_of(X, idx, far, d);
      for (int a = 0; a < d; ++a) cc[a] = x[a];
      lab[far] = c;
      dmin[far] = dist2(x, cold + (size_t)c * d, d);
      if (p > c) pp_sum_cluster(X, idx, n, d, lab, p, sums);
    }
  }
  return PPResult{kOk, iters};
}

// gcentroids of every cluster, cw in cw[K]; sums [K][d+1] is scratch
WTK_HD inline void wk_centroids_serial(const double *X, int d, int n, const double *w, const int *lab, int K,
                                       double *cen, double *cw, double *sums) {
  for (int e = 0; e < K * (d + 1); ++e) sums[e] = 0.0;
  for (int m = 0; m < n; ++m) {
    double *s = sums + (size_t)lab[m] * (d + 1);
    const double *p = X + (size_t)m * d;
    for (int a = 0; a < d; ++a) s[a] += p[a] * w[m];
    s[d] += w[m];
  }
  for (int c = 0; c < K; ++c) {
    const double *s = sums + (size_t)c * (d + 1);
    cw[c] = s[d];
    for (int a = 0; a < d; ++a) cen[(size_t)c * d + a] = s[d] > 0.0 ? s[a] / s[d] : s[a];
  }
}

// genergy: f [n], the energies per cluster in sums[0..K-1], their sum returned
WTK_HD inline double wk_energy_serial(const double *X, int d, int n, const double *w, const int *lab, int K,
                                      const double *cen, const double *cw, double *f, double *sums) {
  for (int c = 0; c < K; ++c) sums[c] = 0.0;
  for (int m = 0; m < n; ++m) {
    const int l = lab[m];
    const double fm = dist2(X + (size_t)m * d, cen + (size_t)l * d, d);
    sums[l] += w[m] * fm;
    f[m] = wk_member_f(fm, cw[l], w[m]);
  }
  double e = 0.0;
  for (int c = 0; c < K; ++c) e += sums[c];
  return e;
}

// (b) on all n points from the centres in cen [K][d] (replaced by the final ones).
// cw [K]; sums [K][d+1]; f, lab [n]; energies: [it_max + 1] or null, entry i the energy
// after i counted sweeps.
WTK_HD inline WKResult weighted_serial(const double *X, int d, int n, const double *w, int K, int it_max, double *cen,
                                       double *cw, double *sums, double *f, int *lab, double *energies) {
  for (int m = 0; m < n; ++m) {
    double dm;
    lab[m] = nearest(X + (size_t)m * d, cen, K, d, &dm);
  }
  wk_centroids_serial(X, d, n, w, lab, K, cen, cw, sums);
  double old = wk_energy_serial(X, d, n, w, lab, K, cen, cw, f, sums);
  if (energies) energies[0] = old;
  int it = 0;
  double last = old;
  while (it < it_max) {
    for (int m = 0; m < n; ++m) lab[m] = wk_assign(X + (size_t)m * d, w[m], lab[m], f[m], cen, cw, K, d);
    wk_centroids_serial(X, d, n, w, lab, K, cen, cw, sums);
    last = wk_energy_serial(X, d, n, w, lab, K, cen, cw, f, sums);
    if (std::fabs(last - old) < kWkTol) break;
    old = last;
    ++it;
    if (energies) energies[it] = last;
  }
  return WKResult{kOk, it, last};
}

// One trial of the first stage: (a) over all points for K centres, then (b).  Outputs
// (labels [n], counts [K], iters [2]) are written for an OK trial only.  Scratch: cen, cold
// [K][d], sums [K][d+1], cw [K], dwork [n], lwork [n].
WTK_HD inline int cluster_trial_serial(const double *X, const double *w, int n, int d, int K, int j0, const double *u,
                                       double *cen, double *cold, double *sums, double *cw, double *dwork, int *lwork,
                                       int *labels, int *counts, int *iters) {
  if (j0 < 0 || j0 >= n || !points_finite_serial(X, nullptr, n, d, w)) return kBad;
  const PPResult pp = kmeans_pp_serial(X, d, nullptr, n, K, j0, u, kLloydMax, cen, cold, sums, dwork, lwork);
  if (pp.status != kOk) return pp.status;
  const WKResult wk = weighted_serial(X, d, n, w, K, kWkMax, cen, cw, sums, dwork, lwork, nullptr);
  for (int c = 0; c < K; ++c) counts[c] = 0;
  for (int m = 0; m < n; ++m) {
    labels[m] = lwork[m];
    ++counts[lwork[m]];
  }
  iters[0] = pp.iters;
  iters[1] = wk.iters;
  return kOk;
}

// One item of the second stage: (a) on the nmem members of cluster c for S centres, written
// to out [S][d] for an OK item only.  Scratch: idx, lwork [nmem], dwork [nmem], cen, cold
// [S][d], sums [S][d+1].
WTK_HD inline int states_item_serial(const double *X, int n, int d, const int *labels, int c, int nmem, int S, int j0,
                                     const double *u, int *idx, double *cen, double *cold, double *sums, double *dwork,
                                     int *lwork, double *out, int *iters) {
  int cnt = 0;
  for (int m = 0; m < n; ++m)
    if (labels[m] == c) {
      if (cnt < nmem) idx[cnt] = m;
      ++cnt;
    }
  if (cnt != nmem || j0 < 0 || j0 >= nmem || !points_finite_serial(X, idx, nmem, d, nullptr)) return kBad;
  const PPResult pp = kmeans_pp_serial(X, d, idx, nmem, S, j0, u, kLloydMax, cen, cold, sums, dwork, lwork);
  if (pp.status != kOk) return pp.status;
  for (int e = 0; e < S * d; ++e) out[e] = cen[e];
  *iters = pp.iters;
  return kOk;
}

// ---------------------------------------------------------------------------------------
// the block routines: one workgroup of kBlock threads, every argument uniform
// ---------------------------------------------------------------------------------------
#if defined(__HIPCC__)

// A workgroup's LDS.  Centres and sums use the run's own strides (d and d + 1).
template <int DB>
struct Block {
  double cen[kMaxK * DB], cold[kMaxK * DB], sums[kMaxK * (DB + 1)], cw[kMaxK];
  double wred[kWaves * group_of(DB) * (DB + 1)];
  double scan[kBlock + 1];
  double rv[kWaves];
  int ri[kWaves];
  int cnt[kWaves * kMaxK];
  int pick;
};

__device__ inline double wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the sum of v over the workgroup: a butterfly per wave, then the waves in order
template <int DB>
__device__ inline double block_sum(Block<DB> &b, double v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) b.rv[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = b.rv[0];
  for (int q = 1; q < kWaves; ++q) r += b.rv[q];
  __syncthreads();
  return r;
}

// the least index over the workgroup (kNone: a thread without one)
template <int DB>
__device__ inline int block_min_index(Block<DB> &b, int i) {
  for (int m = 32; m >= 1; m >>= 1) {
    const int o = __shfl_xor(i, m, 64);
    i = o < i ? o : i;
  }
  if ((threadIdx.x & 63) == 0) b.ri[threadIdx.x >> 6] = i;
  __syncthreads();
  int r = b.ri[0];
  for (int q = 1; q < kWaves; ++q) r = b.ri[q] < r ? b.ri[q] : r;
  __syncthreads();
  return r;
}

// np.argmax over the workgroup's (value, index) pairs: the greatest value, the least index
// among equal ones (kNone: a thread without a pair)
template <int DB>
__device__ inline int block_argmax_first(Block<DB> &b, double v, int i) {
  for (int m = 32; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (oi != kNone && (i == kNone || ov > v || (ov == v && oi < i))) {
      v = ov;
      i = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    b.rv[threadIdx.x >> 6] = v;
    b.ri[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = b.rv[0];
  i = b.ri[0];
  for (int q = 1; q < kWaves; ++q) {
    const double ov = b.rv[q];
    const int oi = b.ri[q];
    if (oi != kNone && (i == kNone || ov > v || (ov == v && oi < i))) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();
  return i;
}

// every member's coordinates (and weight) finite
template <int DB>
__device__ inline bool block_points_finite(Block<DB> &b, const double *X, const int *idx, int n, int d,
                                           const double *w) {
  int bad = 0;
  for (int m = threadIdx.x; m < n; m += kBlock) {
    const double *p = point_of(X, idx, m, d);
    for (int a = 0; a < d; ++a) bad |= !finite_d(p[a]);
    if (w) bad |= !finite_d(w[idx ? idx[m] : m]);
  }
  return !__syncthreads_or(bad);
}

// b.sums[c][0..d] of the clusters c_begin <= c < c_end: coordinate sums (times the weight
// with wt) and the count (the weight sum), group_of(DB) clusters per pass over the members.
// A thread sums its members in order into registers; the workgroup adds the threads' sums
// by block_sum's tree.
template <int DB>
__device__ inline void block_accumulate(Block<DB> &b, const double *X, int d, const int *idx, const double *wt,
                                        const int *lab, int n, int c_begin, int c_end) {
  constexpr int G = group_of(DB), E = G * (DB + 1);
  const int tid = threadIdx.x;
  for (int c0 = c_begin; c0 < c_end; c0 += G) {
    const int gc = c_end - c0 < G ? c_end - c0 : G;
    double acc[G][DB + 1];
    WTK_UNROLL
    for (int g = 0; g < G; ++g) {
      WTK_UNROLL
      for (int a = 0; a <= DB; ++a) acc[g][a] = 0.0;
    }
    for (int m = tid; m < n; m += kBlock) {
      const int l = lab[m] - c0;
      if (l < 0 || l >= gc) continue;
      const int pi = idx ? idx[m] : m;
      const double *p = X + (size_t)pi * d;
      const double w = wt ? wt[pi] : 1.0;
      double xw[DB];
      WTK_UNROLL
      for (int a = 0; a < DB; ++a) xw[a] = a < d ? (wt ? p[a] * w : p[a]) : 0.0;
      WTK_UNROLL
      for (int g = 0; g < G; ++g) {
        const bool on = l == g;
        WTK_UNROLL
        for (int a = 0; a < DB; ++a) acc[g][a] += on ? xw[a] : 0.0;
        acc[g][DB] += on ? w : 0.0;
      }
    }
    WTK_UNROLL
    for (int g = 0; g < G; ++g) {
      WTK_UNROLL
      for (int a = 0; a <= DB; ++a) {
        const double v = wave_sum(acc[g][a]);
        if ((tid & 63) == 0) b.wred[(tid >> 6) * E + g * (DB + 1) + a] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < E; e += kBlock) {
      const int g = e / (DB + 1), a = e % (DB + 1);
      if (g >= gc || (a >= d && a != DB)) continue;
      double r = b.wred[e];
      for (int q = 1; q < kWaves; ++q) r += b.wred[q * E + e];
      b.sums[(c0 + g) * (d + 1) + (a == DB ? d : a)] = r;
    }
    __syncthreads();
  }
}

// The D2 draw.  Every thread sums a contiguous chunk of dmin; thread 0 adds the chunk sums
// in order (b.scan: exclusive prefixes, b.scan[kBlock]: the total, returned).
template <int DB>
__device__ inline double block_chunk_scan(Block<DB> &b, const double *dmin, int n) {
  const int tid = threadIdx.x, L = (n + kBlock - 1) / kBlock;
  const long long lo = (long long)tid * L;
  const int hi = lo + L < n ? (int)(lo + L) : n;
  double s = 0.0;
  for (long long m = lo; m < hi; ++m) s += dmin[m];
  b.scan[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int t = 0; t < kBlock; ++t) {
      const double v = b.scan[t];
      b.scan[t] = run;
      run += v;
    }
    b.scan[kBlock] = run;
  }
  __syncthreads();
  return b.scan[kBlock];
}

// ... and the first member whose running sum exceeds target (the last member if rounding
// leaves none), after block_chunk_scan.
template <int DB>
__device__ inline int block_pick(Block<DB> &b, const double *dmin, int n, double target) {
  const int tid = threadIdx.x, L = (n + kBlock - 1) / kBlock;
  const long long lo = (long long)tid * L;
  const int hi = lo + L < n ? (int)(lo + L) : n;
  int pick = kNone;
  double run = b.scan[tid];
  for (long long m = lo; m < hi; ++m) {
    run += dmin[m];
    if (run > target) {
      pick = (int)m;
      break;
    }
  }
  pick = block_min_index(b, pick);
  return pick == kNone ? n - 1 : pick;
}

// The members of cluster c among labels [n], in point order, into idx (at most cap of them
// are written); returns how many there are.
template <int DB>
__device__ inline int block_members(Block<DB> &b, const int *labels, int n, int c, int *idx, int cap) {
  const int tid = threadIdx.x, L = (n + kBlock - 1) / kBlock;
  const long long lo = (long long)tid * L;
  const int hi = lo + L < n ? (int)(lo + L) : n;
  int cnt = 0;
  for (long long m = lo; m < hi; ++m) cnt += labels[m] == c;
  b.scan[tid] = (double)cnt;
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int t = 0; t < kBlock; ++t) {
      const double v = b.scan[t];
      b.scan[t] = run;
      run += v;
    }
    b.scan[kBlock] = run;
  }
  __syncthreads();
  int pos = (int)b.scan[tid];
  const int total = (int)b.scan[kBlock];
  for (long long m = lo; m < hi; ++m)
    if (labels[m] == c) {
      if (pos < cap) idx[pos] = (int)m;
      ++pos;
    }
  __syncthreads();
  return total;
}

// counts [K] of the labels, written by the first K threads
template <int DB>
__device__ inline void block_counts(Block<DB> &b, const int *lab, int n, int K, int *counts) {
  const int tid = threadIdx.x;
  int cnt[kMaxK];
  WTK_UNROLL
  for (int c = 0; c < kMaxK; ++c) cnt[c] = 0;
  for (int m = tid; m < n; m += kBlock) {
    const int l = lab[m];
    WTK_UNROLL
    for (int c = 0; c < kMaxK; ++c) cnt[c] += l == c;
  }
  WTK_UNROLL
  for (int c = 0; c < kMaxK; ++c) {
    int v = cnt[c];
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((tid & 63) == 0) b.cnt[(tid >> 6) * kMaxK + c] = v;
  }
  __syncthreads();
  if (tid < K) {
    int r = 0;
    for (int q = 0; q < kWaves; ++q) r += b.cnt[q * kMaxK + tid];
    counts[tid] = r;
  }
  __syncthreads();
}

// (a): kmeans_pp_serial's steps; the centres end in b.cen [k][d].  dmin, lab: [n], global.
template <int DB>
__device__ inline PPResult block_kmeans_pp(Block<DB> &b, const double *X, int d, const int *idx, int n, int k, int j0,
                                           const double *u, int max_iter, double *dmin, int *lab) {
  const int tid = threadIdx.x;
  if (tid < d) b.cen[tid] = point_of(X, idx, j0, d)[tid];
  __syncthreads();
  for (int m = tid; m < n; m += kBlock) dmin[m] = dist2(point_of(X, idx, m, d), b.cen, d);
  __syncthreads();
  for (int c = 1; c < k; ++c) {
    const double tot = block_chunk_scan(b, dmin, n);
    if (!(tot > 0.0) || !finite_d(tot)) return PPResult{kDegenerate, 0};
    const int pick = block_pick(b, dmin, n, u[c - 1] * tot);
    if (tid < d) b.cen[c * d + tid] = point_of(X, idx, pick, d)[tid];
    __syncthreads();
    for (int m = tid; m < n; m += kBlock) {
      const double v = dist2(point_of(X, idx, m, d), b.cen + c * d, d);
      if (v < dmin[m]) dmin[m] = v;
    }
    __syncthreads();
  }
  bool have = false;
  int iters = 0;
  for (int it = 0; it < max_iter; ++it) {
    for (int e = tid; e < k * d; e += kBlock) b.cold[e] = b.cen[e];
    int ch = !have;
    for (int m = tid; m < n; m += kBlock) {
      double dm;
      const int l = nearest(point_of(X, idx, m, d), b.cen, k, d, &dm);
      if (have && l != lab[m]) ch = 1;
      lab[m] = l;
      dmin[m] = dm;
    }
    ++iters;
    if (!__syncthreads_or(ch)) break;
    have = true;
    block_accumulate<DB>(b, X, d, idx, nullptr, lab, n, 0, k);
    bool empty = false;
    for (int c = 0; c < k; ++c) empty = empty || !(b.sums[c * (d + 1) + d] > 0.0);
    if (!empty) {
      for (int e = tid; e < k * d; e += kBlock) {
        const int c = e / d, a = e % d;
        b.cen[e] = b.sums[c * (d + 1) + a] / b.sums[c * (d + 1) + d];
      }
      __syncthreads();
      continue;
    }
    for (int c = 0; c < k; ++c) {  // the reference's sweep, a cluster at a time
      const double cnt = b.sums[c * (d + 1) + d];
      if (cnt > 0.0) {
        if (tid < d) b.cen[c * d + tid] = b.sums[c * (d + 1) + tid] / cnt;
        __syncthreads();
        continue;
      }
      double bv = 0.0;
      int bi = kNone;
      for (int m = tid; m < n; m += kBlock) {
        const double v = dmin[m];
        if (bi == kNone || v > bv) {
          bv = v;
          bi = m;
        }
      }
      const int far = block_argmax_first(b, bv, bi);
      const double *x = point_of(X, idx, far, d);
      if (tid == 0) {
        b.pick = lab[far];
        lab[far] = c;
        dmin[far] = dist2(x, b.cold + c * d, d);
      }
      if (tid < d) b.cen[c * d + tid] = x[tid];
      __syncthreads();
      const int p = b.pick;
      __syncthreads();
      if (p > c) block_accumulate<DB>(b, X, d, idx, nullptr, lab, n, p, p + 1);
    }
  }
  return PPResult{kOk, iters};
}

template <int DB>
__device__ inline void block_wk_centroids(Block<DB> &b, const double *X, int d, int n, const double *w, const int *lab,
                                          int K) {
  block_accumulate<DB>(b, X, d, nullptr, w, lab, n, 0, K);
  for (int e = threadIdx.x; e < K * d; e += kBlock) {
    const int c = e / d, a = e % d;
    const double cw = b.sums[c * (d + 1) + d], s = b.sums[c * (d + 1) + a];
    b.cen[e] = cw > 0.0 ? s / cw : s;
  }
  if (threadIdx.x < K) b.cw[threadIdx.x] = b.sums[threadIdx.x * (d + 1) + d];
  __syncthreads();
}

template <int DB>
__device__ inline double block_wk_energy(Block<DB> &b, const double *X, int d, int n, const double *w, const int *lab,
                                         double *f) {
  double e = 0.0;
  for (int m = threadIdx.x; m < n; m += kBlock) {
    const int l = lab[m];
    const double fm = dist2(X + (size_t)m * d, b.cen + l * d, d);
    e += w[m] * fm;
    f[m] = wk_member_f(fm, b.cw[l], w[m]);
  }
  return block_sum(b, e);
}

// (b): weighted_serial's steps from the centres in b.cen [K][d], which end as the final
// ones, b.cw with them.  f, lab: [n], global.  energies: global [it_max + 1] or null.
template <int DB>
__device__ inline WKResult block_weighted(Block<DB> &b, const double *X, int d, int n, const double *w, int K,
                                          int it_max, double *f, int *lab, double *energies) {
  const int tid = threadIdx.x;
  for (int m = tid; m < n; m += kBlock) {
    double dm;
    lab[m] = nearest(X + (size_t)m * d, b.cen, K, d, &dm);
  }
  __syncthreads();
  block_wk_centroids(b, X, d, n, w, lab, K);
  double old = block_wk_energy(b, X, d, n, w, lab, f);
  if (energies && tid == 0) energies[0] = old;
  int it = 0;
  double last = old;
  while (it < it_max) {
    for (int m = tid; m < n; m += kBlock)
      lab[m] = wk_assign(X + (size_t)m * d, w[m], lab[m], f[m], b.cen, b.cw, K, d);
    __syncthreads();
    block_wk_centroids(b, X, d, n, w, lab, K);
    last = block_wk_energy(b, X, d, n, w, lab, f);
    if (fabs(last - old) < kWkTol) break;
    old = last;
    ++it;
    if (energies && tid == 0) energies[it] = last;
  }
  return WKResult{kOk, it, last};
}

#endif  // __HIPCC__

}  // namespace wtkrun
}  // namespace vbhem
