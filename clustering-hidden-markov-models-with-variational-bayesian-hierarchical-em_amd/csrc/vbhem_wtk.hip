// vbhem_wtk.hip -- the batched 'wtkmeans' initialisation (include/vbhem_init.h).  The
// arithmetic is vbhem_wtk_run.h, shared with the host check build.
//
// wtk_cluster_kernel<DB>: a workgroup of 256 threads owns ONE trial: kmeans_pp over all n
// points for K centres, then weighted_kmeans.  wtk_states_kernel<DB>: a workgroup owns ONE
// (trial, cluster): it lists the cluster's members in point order and runs kmeans_pp over
// them for S centres.  DB is the dimension bucket (2, 4, 8, 16).
//
// Points and weights stay in global memory and are read in block strides (the chunked D2
// scan and member listing aside); the per-point state (the running d2 / f, the labels) is
// the workgroup's workspace slot; centres, their sums and the reductions' scratch are LDS
// (Block<DB>).  Centroid sums: a thread keeps group_of(DB) clusters' (d + 1) sums in
// registers per pass over the points (8, 8, 4 and 2 clusters for DB = 2, 4, 8 and 16: what
// fits 256 VGPRs without scratch), and the threads' sums are added in a fixed tree.  No
// atomics; every loop is bounded by n, K, S, d or the iteration limits.  A trial that is not OK writes its status alone: labels are
// worked on in the workspace and copied out at the end.
//
// This is the BLOCK schedule.  The tiled schedule (vbhem_wtk_tiled.hip) launches
// wtk_cluster_kernel through wtk_block_rerun for the trials whose Lloyd update emptied a
// cluster: the kernel then reads a per-trial flag first and leaves where it is clear.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_init.h"
#include "vbhem_internal.h"
#include "vbhem_wtk_run.h"
#include "vbhem_wtk_tiled_run.h"

namespace vbhem {
namespace {

using namespace wtkrun;

struct ClusterArgs {
  int R0, n, d, K, ustride;
  const double *x, *w, *u;
  const int *j0;
  int *labels, *counts, *status, *iters;
  double *wd;  // [chunk][n]
  int *wl;     // [chunk][n]
  // the tiled schedule's re-seed hand-over (vbhem_wtk_tiled.hip): a workgroup whose trial's
  // flag only[block * only_stride] is clear leaves at once; null: every trial runs
  const int *only;
  int only_stride;
};

template <int DB>
__global__ __launch_bounds__(kBlock) void wtk_cluster_kernel(const ClusterArgs p) {
  __shared__ Block<DB> b;
  const int tid = threadIdx.x, r = p.R0 + blockIdx.x, n = p.n, d = p.d, K = p.K;
  if (p.only && !p.only[(size_t)blockIdx.x * p.only_stride]) return;
  double *dwork = p.wd + (size_t)blockIdx.x * n;
  int *lwork = p.wl + (size_t)blockIdx.x * n;
  const int j0 = p.j0[r];
  const bool fin = block_points_finite(b, p.x, nullptr, n, d, p.w);
  if (!fin || j0 < 0 || j0 >= n) {
    if (tid == 0) p.status[r] = kBad;
    return;
  }
  const PPResult pp =
      block_kmeans_pp(b, p.x, d, nullptr, n, K, j0, p.u + (size_t)r * p.ustride, kLloydMax, dwork, lwork);
  if (pp.status != kOk) {
    if (tid == 0) p.status[r] = pp.status;
    return;
  }
  const WKResult wk = block_weighted(b, p.x, d, n, p.w, K, kWkMax, dwork, lwork, nullptr);
  int *lab = p.labels + (size_t)r * n;
  for (int m = tid; m < n; m += kBlock) lab[m] = lwork[m];
  block_counts(b, lwork, n, K, p.counts + (size_t)r * K);
  if (tid == 0) {
    p.status[r] = kOk;
    p.iters[2 * r] = pp.iters;
    p.iters[2 * r + 1] = wk.iters;
  }
}

struct StatesArgs {
  int n, d, K, S, R, ustride;
  long long total;
  const double *x, *u;
  const int *labels, *trial, *cluster, *nmem, *j0;
  const long long *off;
  double *centres;
  int *status, *iters;
  double *wd;      // [total]
  int *widx, *wl;  // [total] each
};

template <int DB>
__global__ __launch_bounds__(kBlock) void wtk_states_kernel(const StatesArgs p) {
  __shared__ Block<DB> b;
  const int tid = threadIdx.x, q = blockIdx.x, n = p.n, d = p.d, S = p.S;
  const int r = p.trial[q], c = p.cluster[q], nm = p.nmem[q], j0 = p.j0[q];
  const long long off = p.off[q];
  // the item's slot lies inside the workspace, its draw inside its members (uniform)
  bool ok = r >= 0 && r < p.R && c >= 0 && c < p.K && nm >= 1 && nm <= n && off >= 0 && off + nm <= p.total &&
            j0 >= 0 && j0 < nm;
  int *idx = p.widx + (ok ? off : 0);
  if (ok) ok = block_members(b, p.labels + (size_t)r * n, n, c, idx, nm) == nm;
  if (ok) ok = block_points_finite(b, p.x, idx, nm, d, nullptr);
  if (!ok) {
    if (tid == 0) p.status[q] = kBad;
    return;
  }
  const PPResult pp =
      block_kmeans_pp(b, p.x, d, idx, nm, S, j0, p.u + (size_t)q * p.ustride, kLloydMax, p.wd + off, p.wl + off);
  if (pp.status != kOk) {
    if (tid == 0) p.status[q] = pp.status;
    return;
  }
  double *out = p.centres + ((size_t)r * p.K + c) * S * d;
  for (int e = tid; e < S * d; e += kBlock) out[e] = b.cen[e];
  if (tid == 0) {
    p.status[q] = kOk;
    p.iters[q] = pp.iters;
  }
}

size_t slot_bytes(int n) { return (size_t)n * sizeof(double) + (((size_t)n * sizeof(int) + 7) & ~(size_t)7); }

int chunk_of(int chunk_trials, int n, int R) {
  if (chunk_trials > 0) return std::min(chunk_trials, std::max(R, 1));
  const size_t fit = (size_t)VBHEM_WTK_DEFAULT_WORKSPACE / slot_bytes(n);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(R, 1), fit));
}

int launch_cluster(const ClusterArgs &a, int trials, hipStream_t st) {
  const dim3 grid((unsigned)trials), block(kBlock);
  switch (dim_bucket(a.d)) {
    case 2: hipLaunchKernelGGL(wtk_cluster_kernel<2>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(wtk_cluster_kernel<4>, grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(wtk_cluster_kernel<8>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(wtk_cluster_kernel<16>, grid, block, 0, st, a); break;
  }
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e, "wtk_cluster_kernel") : VBHEM_OK;
}

int check_sizes(const char *what, int n, int d, int K, int S, int R) {
  if (n < 1 || d < 1 || K < 1 || S < 1 || R < 0)
    return set_error(VBHEM_ERR_ARG, std::string(what) + ": need n, d, K, S >= 1 and R >= 0");
  if (d > kMaxDim) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": d <= 16 supported");
  if (K > kMaxK) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": K <= 32 supported");
  if (S > kMaxS) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": S <= 16 supported");
  return VBHEM_OK;
}

}  // namespace

// The block schedule over the trials R0 .. R0 + trials - 1 whose flag is set (see
// ClusterArgs::only), from scratch, for the tiled schedule's emptied-cluster trials.
int wtk_block_rerun(int n, int d, int K, int R0, int trials, const double *x, const double *w, const int *j0,
                    const double *u, int *labels, int *counts, int *status, int *iters, double *wd, int *wl,
                    const int *only, int only_stride, hipStream_t st) {
  ClusterArgs a{};
  a.R0 = R0; a.n = n; a.d = d; a.K = K; a.ustride = std::max(K - 1, 1);
  a.x = x; a.w = w; a.u = u; a.j0 = j0;
  a.labels = labels; a.counts = counts; a.status = status; a.iters = iters;
  a.wd = wd; a.wl = wl; a.only = only; a.only_stride = only_stride;
  return launch_cluster(a, trials, st);
}

}  // namespace vbhem

extern "C" {

size_t vbhem_wtk_cluster_workspace_bytes(int n, int d, int K, int R, int chunk_trials) {
  using namespace vbhem;
  if (check_sizes("vbhem_wtk_cluster", n, d, K, 1, R) != VBHEM_OK || chunk_trials < 0) return 0;
  return std::max<size_t>(256, (size_t)chunk_of(chunk_trials, n, R) * slot_bytes(n));
}

int vbhem_wtk_cluster_batch(int n, int d, int K, int R, const double *x_dev, const double *weight_dev,
                            const int *j0_dev, const double *u_dev, int chunk_trials, int *labels_dev,
                            int *counts_dev, int *status_dev, int *iters_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  const int rc = check_sizes("vbhem_wtk_cluster_batch", n, d, K, 1, R);
  if (rc != VBHEM_OK) return rc;
  if (chunk_trials < 0) return set_error(VBHEM_ERR_ARG, "vbhem_wtk_cluster_batch: chunk_trials >= 0");
  if (R == 0) return VBHEM_OK;
  if (!x_dev || !weight_dev || !j0_dev || !u_dev || !labels_dev || !counts_dev || !status_dev || !iters_dev)
    return set_error(VBHEM_ERR_ARG, "vbhem_wtk_cluster_batch: null array");
  const int chunk = chunk_of(chunk_trials, n, R);
  const size_t need = (size_t)chunk * slot_bytes(n);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  ClusterArgs a{};
  a.n = n; a.d = d; a.K = K; a.ustride = std::max(K - 1, 1);
  a.x = x_dev; a.w = weight_dev; a.u = u_dev; a.j0 = j0_dev;
  a.labels = labels_dev; a.counts = counts_dev; a.status = status_dev; a.iters = iters_dev;
  a.wd = static_cast<double *>(workspace_dev);
  a.wl = reinterpret_cast<int *>(a.wd + (size_t)chunk * n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int r0 = 0; r0 < R; r0 += chunk) {
    a.R0 = r0;
    const int lrc = launch_cluster(a, std::min(chunk, R - r0), st);
    if (lrc != VBHEM_OK) return lrc;
  }
  return VBHEM_OK;
}

size_t vbhem_wtk_states_workspace_bytes(long long total_members) {
  if (total_members < 0) return 0;
  return std::max<size_t>(256, (size_t)total_members * (sizeof(double) + 2 * sizeof(int)) + 16);
}

int vbhem_wtk_states_batch(int n, int d, int K, int S, int R, const double *x_dev, const int *labels_dev, int I,
                           const int *trial_dev, const int *cluster_dev, const int *nmem_dev,
                           const long long *off_dev, long long total_members, const int *j0_dev,
                           const double *u_dev, double *centres_dev, int *status_dev, int *iters_dev,
                           void *workspace_dev, size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  const int rc = check_sizes("vbhem_wtk_states_batch", n, d, K, S, R);
  if (rc != VBHEM_OK) return rc;
  if (I < 0 || total_members < 0) return set_error(VBHEM_ERR_ARG, "vbhem_wtk_states_batch: negative count");
  if (I == 0) return VBHEM_OK;
  if (!x_dev || !labels_dev || !trial_dev || !cluster_dev || !nmem_dev || !off_dev || !j0_dev || !u_dev ||
      !centres_dev || !status_dev || !iters_dev)
    return set_error(VBHEM_ERR_ARG, "vbhem_wtk_states_batch: null array");
  const size_t need = vbhem_wtk_states_workspace_bytes(total_members);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  StatesArgs a{};
  a.n = n; a.d = d; a.K = K; a.S = S; a.R = R; a.ustride = std::max(S - 1, 1);
  a.total = total_members;
  a.x = x_dev; a.u = u_dev; a.labels = labels_dev; a.trial = trial_dev; a.cluster = cluster_dev;
  a.nmem = nmem_dev; a.j0 = j0_dev; a.off = off_dev;
  a.centres = centres_dev; a.status = status_dev; a.iters = iters_dev;
  a.wd = static_cast<double *>(workspace_dev);
  a.widx = reinterpret_cast<int *>(a.wd + total_members);
  a.wl = a.widx + total_members;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)I), block(kBlock);
  switch (dim_bucket(d)) {
    case 2: hipLaunchKernelGGL(wtk_states_kernel<2>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(wtk_states_kernel<4>, grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(wtk_states_kernel<8>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(wtk_states_kernel<16>, grid, block, 0, st, a); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "wtk_states_kernel");
  return VBHEM_OK;
}

}  // extern "C"
