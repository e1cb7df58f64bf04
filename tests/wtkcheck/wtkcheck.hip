// tests/wtkcheck/wtkcheck.hip -- TEST-ONLY exports of the batched 'wtkmeans' initialisation:
// the serial walkers of csrc/vbhem_wtk_run.h on host arrays (where = 0), so the arithmetic
// is checked on a machine without a GPU, and the same calls on device 0 (where = 1):
// wtkcheck_pp and wtkcheck_wk run (a) and (b) alone through thin kernels over the block
// routines, from given draws and centres; wtkcheck_cluster and wtkcheck_states go through
// the library (include/vbhem_init.h).  Arrays are host arrays; outputs of runs that are not
// OK keep what the caller put there.  Returns 0, -2 outside the limits, the library's
// status, or a positive hipError_t.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_pool.h"
#include "vbhem_init.h"
#include "vbhem_wtk_run.h"

namespace {

using namespace vbhem::wtkrun;
using checklib::Pool;

bool in_limits(int n, int d, int K) { return n >= 1 && d >= 1 && d <= kMaxDim && K >= 1 && K <= kMaxK; }

template <int DB>
__global__ __launch_bounds__(kBlock) void pp_kernel(const double *X, int d, const int *idx, int n, int k, int j0,
                                                    const double *u, int max_iter, double *dmin, int *lab, double *cen,
                                                    int *iters, int *status) {
  __shared__ Block<DB> b;
  if (j0 < 0 || j0 >= n || !block_points_finite(b, X, idx, n, d, nullptr)) {
    if (threadIdx.x == 0) *status = kBad;
    return;
  }
  const PPResult r = block_kmeans_pp(b, X, d, idx, n, k, j0, u, max_iter, dmin, lab);
  if (threadIdx.x == 0) *status = r.status;
  if (r.status != kOk) return;
  for (int e = threadIdx.x; e < k * d; e += kBlock) cen[e] = b.cen[e];
  if (threadIdx.x == 0) *iters = r.iters;
}

template <int DB>
__global__ __launch_bounds__(kBlock) void wk_kernel(const double *X, int d, int n, const double *w, int K, int it_max,
                                                    double *f, int *lab, double *cen, double *energies, double *last,
                                                    int *iters, int *status) {
  __shared__ Block<DB> b;
  bool ok = block_points_finite(b, X, nullptr, n, d, w);
  int bad = 0;
  for (int e = threadIdx.x; e < K * d; e += kBlock) bad |= !finite_d(cen[e]);
  ok = !__syncthreads_or(bad) && ok;
  if (!ok) {
    if (threadIdx.x == 0) *status = kBad;
    return;
  }
  for (int e = threadIdx.x; e < K * d; e += kBlock) b.cen[e] = cen[e];
  __syncthreads();
  const WKResult r = block_weighted(b, X, d, n, w, K, it_max, f, lab, energies);
  for (int e = threadIdx.x; e < K * d; e += kBlock) cen[e] = b.cen[e];
  if (threadIdx.x == 0) {
    *status = r.status;
    *iters = r.iters;
    *last = r.energy;
  }
}

}  // namespace

extern "C" {

// (a) on the nsub members idx (null: all n points, nsub = n) for k centres.
int wtkcheck_pp(int where, int n, int d, const double *X, int nsub, const int *idx, int k, int j0, const double *u,
                int max_iter, double *cen, int *lab, int *iters, int *status) {
  if (!in_limits(n, d, k) || nsub < 1 || nsub > n || max_iter < 1) return -2;
  if (idx)
    for (int m = 0; m < nsub; ++m)
      if (idx[m] < 0 || idx[m] >= n) return -2;
  if (where == 0) {
    if (j0 < 0 || j0 >= nsub || !points_finite_serial(X, idx, nsub, d, nullptr)) {
      *status = kBad;
      return 0;
    }
    std::vector<double> c((size_t)k * d), cold((size_t)k * d), sums((size_t)k * (d + 1)), dmin(nsub);
    std::vector<int> l(nsub);
    const PPResult r =
        kmeans_pp_serial(X, d, idx, nsub, k, j0, u, max_iter, c.data(), cold.data(), sums.data(), dmin.data(), l.data());
    *status = r.status;
    if (r.status != kOk) return 0;
    std::copy(c.begin(), c.end(), cen);
    std::copy(l.begin(), l.end(), lab);
    *iters = r.iters;
    return 0;
  }
  Pool pool;
  const int nu = std::max(k - 1, 1);
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const int *didx = idx ? static_cast<const int *>(pool.put(idx, (size_t)nsub * 4)) : nullptr;
  const double *du = static_cast<const double *>(pool.put(u, (size_t)nu * 8));
  double *dmin = static_cast<double *>(pool.put(nullptr, (size_t)nsub * 8));
  int *dlab = static_cast<int *>(pool.put(lab, (size_t)nsub * 4));
  double *dcen = static_cast<double *>(pool.put(cen, (size_t)k * d * 8));
  int *dit = static_cast<int *>(pool.put(iters, 4));
  int *dst = static_cast<int *>(pool.put(status, 4));
  if (pool.e != hipSuccess) return (int)pool.e;
  const dim3 grid(1), block(kBlock);
  switch (dim_bucket(d)) {
    case 2: hipLaunchKernelGGL(pp_kernel<2>, grid, block, 0, nullptr, dX, d, didx, nsub, k, j0, du, max_iter, dmin, dlab, dcen, dit, dst); break;
    case 4: hipLaunchKernelGGL(pp_kernel<4>, grid, block, 0, nullptr, dX, d, didx, nsub, k, j0, du, max_iter, dmin, dlab, dcen, dit, dst); break;
    case 8: hipLaunchKernelGGL(pp_kernel<8>, grid, block, 0, nullptr, dX, d, didx, nsub, k, j0, du, max_iter, dmin, dlab, dcen, dit, dst); break;
    default: hipLaunchKernelGGL(pp_kernel<16>, grid, block, 0, nullptr, dX, d, didx, nsub, k, j0, du, max_iter, dmin, dlab, dcen, dit, dst); break;
  }
  pool.e = hipGetLastError();
  if (pool.e == hipSuccess) pool.e = hipDeviceSynchronize();
  pool.get(status, dst, 4);
  if (pool.e == hipSuccess && *status == kOk) {
    pool.get(cen, dcen, (size_t)k * d * 8);
    pool.get(lab, dlab, (size_t)nsub * 4);
    pool.get(iters, dit, 4);
  }
  return (int)pool.e;
}

// (b) from the centres in cen [K][d] (replaced by the final ones); energies [it_max + 1].
int wtkcheck_wk(int where, int n, int d, const double *X, const double *w, int K, int it_max, double *cen, int *lab,
                double *energies, double *last, int *iters, int *status) {
  if (!in_limits(n, d, K) || it_max < 0) return -2;
  if (where == 0) {
    bool ok = points_finite_serial(X, nullptr, n, d, w);
    for (int e = 0; e < K * d; ++e) ok = ok && finite_d(cen[e]);
    if (!ok) {
      *status = kBad;
      return 0;
    }
    std::vector<double> cw(K), sums((size_t)K * (d + 1)), f(n);
    const WKResult r = weighted_serial(X, d, n, w, K, it_max, cen, cw.data(), sums.data(), f.data(), lab, energies);
    *status = r.status;
    *iters = r.iters;
    *last = r.energy;
    return 0;
  }
  Pool pool;
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const double *dw = static_cast<const double *>(pool.put(w, (size_t)n * 8));
  double *df = static_cast<double *>(pool.put(nullptr, (size_t)n * 8));
  int *dlab = static_cast<int *>(pool.put(lab, (size_t)n * 4));
  double *dcen = static_cast<double *>(pool.put(cen, (size_t)K * d * 8));
  double *den = static_cast<double *>(pool.put(energies, (size_t)(it_max + 1) * 8));
  double *dla = static_cast<double *>(pool.put(last, 8));
  int *dit = static_cast<int *>(pool.put(iters, 4));
  int *dst = static_cast<int *>(pool.put(status, 4));
  if (pool.e != hipSuccess) return (int)pool.e;
  const dim3 grid(1), block(kBlock);
  switch (dim_bucket(d)) {
    case 2: hipLaunchKernelGGL(wk_kernel<2>, grid, block, 0, nullptr, dX, d, n, dw, K, it_max, df, dlab, dcen, den, dla, dit, dst); break;
    case 4: hipLaunchKernelGGL(wk_kernel<4>, grid, block, 0, nullptr, dX, d, n, dw, K, it_max, df, dlab, dcen, den, dla, dit, dst); break;
    case 8: hipLaunchKernelGGL(wk_kernel<8>, grid, block, 0, nullptr, dX, d, n, dw, K, it_max, df, dlab, dcen, den, dla, dit, dst); break;
    default: hipLaunchKernelGGL(wk_kernel<16>, grid, block, 0, nullptr, dX, d, n, dw, K, it_max, df, dlab, dcen, den, dla, dit, dst); break;
  }
  pool.e = hipGetLastError();
  if (pool.e == hipSuccess) pool.e = hipDeviceSynchronize();
  pool.get(status, dst, 4);
  if (pool.e == hipSuccess && *status == kOk) {
    pool.get(cen, dcen, (size_t)K * d * 8);
    pool.get(lab, dlab, (size_t)n * 4);
    pool.get(energies, den, (size_t)(it_max + 1) * 8);
    pool.get(last, dla, 8);
    pool.get(iters, dit, 4);
  }
  return (int)pool.e;
}

// The first stage of R trials: cluster_trial_serial per trial, or vbhem_wtk_cluster_batch.
int wtkcheck_cluster(int where, int n, int d, int K, int R, const double *X, const double *w, const int *j0,
                     const double *u, int chunk_trials, int *labels, int *counts, int *status, int *iters) {
  const int nu = std::max(K - 1, 1);
  if (where == 0) {
    if (!in_limits(n, d, K) || R < 0) return -2;
    std::vector<double> cen((size_t)K * d), cold((size_t)K * d), sums((size_t)K * (d + 1)), cw(K), dw(n);
    std::vector<int> lw(n);
    for (int r = 0; r < R; ++r)
      status[r] = cluster_trial_serial(X, w, n, d, K, j0[r], u + (size_t)r * nu, cen.data(), cold.data(), sums.data(),
                                       cw.data(), dw.data(), lw.data(), labels + (size_t)r * n, counts + (size_t)r * K,
                                       iters + 2 * (size_t)r);
    return 0;
  }
  if (n < 1 || d < 1 || K < 1 || R < 0) return -1;
  Pool pool;
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const double *dwt = static_cast<const double *>(pool.put(w, (size_t)n * 8));
  const int *dj = static_cast<const int *>(pool.put(j0, (size_t)R * 4));
  const double *du = static_cast<const double *>(pool.put(u, (size_t)R * nu * 8));
  int *dl = static_cast<int *>(pool.put(labels, (size_t)R * n * 4));
  int *dc = static_cast<int *>(pool.put(counts, (size_t)R * K * 4));
  int *ds = static_cast<int *>(pool.put(status, (size_t)R * 4));
  int *di = static_cast<int *>(pool.put(iters, (size_t)R * 2 * 4));
  const size_t wb = vbhem_wtk_cluster_workspace_bytes(n, d, K, R, chunk_trials);
  void *ws = pool.put(nullptr, wb);
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhem_wtk_cluster_batch(n, d, K, R, dX, dwt, dj, du, chunk_trials, dl, dc, ds, di, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(labels, dl, (size_t)R * n * 4);
  pool.get(counts, dc, (size_t)R * K * 4);
  pool.get(status, ds, (size_t)R * 4);
  pool.get(iters, di, (size_t)R * 2 * 4);
  return (int)pool.e;
}

// The second stage of I items: states_item_serial per item, or vbhem_wtk_states_batch.
int wtkcheck_states(int where, int n, int d, int K, int S, int R, const double *X, const int *labels, int I,
                    const int *trial, const int *cluster, const int *nmem, const int *j0, const double *u,
                    double *centres, int *status, int *iters) {
  const int nu = std::max(S - 1, 1);
  std::vector<long long> off(I + 1, 0);
  for (int q = 0; q < I; ++q) {
    if (nmem[q] < 0) return -1;
    off[q + 1] = off[q] + nmem[q];
  }
  if (where == 0) {
    if (!in_limits(n, d, K) || S < 1 || S > kMaxS || R < 0) return -2;
    std::vector<double> cen((size_t)S * d), cold((size_t)S * d), sums((size_t)S * (d + 1)), dw(n);
    std::vector<int> idx(n), lw(n);
    for (int q = 0; q < I; ++q) {
      const int r = trial[q], c = cluster[q];
      if (r < 0 || r >= R || c < 0 || c >= K || nmem[q] < 1 || nmem[q] > n) {
        status[q] = kBad;
        continue;
      }
      status[q] = states_item_serial(X, n, d, labels + (size_t)r * n, c, nmem[q], S, j0[q], u + (size_t)q * nu,
                                     idx.data(), cen.data(), cold.data(), sums.data(), dw.data(), lw.data(),
                                     centres + ((size_t)r * K + c) * S * d, iters + q);
    }
    return 0;
  }
  if (n < 1 || d < 1 || K < 1 || S < 1 || R < 0 || I < 0) return -1;
  Pool pool;
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const int *dl = static_cast<const int *>(pool.put(labels, (size_t)R * n * 4));
  const int *dt = static_cast<const int *>(pool.put(trial, (size_t)I * 4));
  const int *dc = static_cast<const int *>(pool.put(cluster, (size_t)I * 4));
  const int *dn = static_cast<const int *>(pool.put(nmem, (size_t)I * 4));
  const long long *dof = static_cast<const long long *>(pool.put(off.data(), (size_t)I * 8));
  const int *dj = static_cast<const int *>(pool.put(j0, (size_t)I * 4));
  const double *du = static_cast<const double *>(pool.put(u, (size_t)I * nu * 8));
  double *dce = static_cast<double *>(pool.put(centres, (size_t)R * K * S * d * 8));
  int *ds = static_cast<int *>(pool.put(status, (size_t)I * 4));
  int *di = static_cast<int *>(pool.put(iters, (size_t)I * 4));
  const size_t wb = vbhem_wtk_states_workspace_bytes(off[I]);
  void *ws = pool.put(nullptr, wb);
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhem_wtk_states_batch(n, d, K, S, R, dX, dl, I, dt, dc, dn, dof, off[I], dj, du, dce, ds, di, ws, wb,
                                        nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(centres, dce, (size_t)R * K * S * d * 8);
  pool.get(status, ds, (size_t)I * 4);
  pool.get(iters, di, (size_t)I * 4);
  return (int)pool.e;
}

}  // extern "C"
