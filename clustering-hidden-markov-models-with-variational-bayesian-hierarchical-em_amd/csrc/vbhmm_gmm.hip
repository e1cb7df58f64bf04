// vbhmm_gmm.hip -- the batched random-start GMM fit (include/vbhmm_gmm.h): every fit of a
// list, from its start rows to its last M-step, in one call; optionally the initial VB-HMM
// posterior of each fitted GMM.  The arithmetic of a fit is vbhmm_gmm_run.h, shared with
// the host check build.
//
// vbhmm_gmm_kernel<KM>: a workgroup is ONE wavefront and owns ONE fit (fit = chunk start +
// blockIdx.x) for its whole EM; the fit's small state (pi, mu, cov, the factors L and their
// log-determinants: Fit<KM>) lives in the workgroup's LDS, the responsibilities [N][KM] and
// the row log-sum-exps [N] in the workspace slot of the workgroup.  Per iteration:
//   factor    a lane per state; a failed pivot ends the fit (wave-uniform: every lane reads
//             the states' flags after the barrier)
//   E-step    a lane per observation, in rounds of 64 (estep_obs)
//   M-step    a lane per statistic entry -- (k) and the log-likelihood, then (k,a), then
//             (k,a,b) -- each walking the subject's observations in index order, so the
//             serial walker is the same sums in the same order
//   stop      lane 0
// The phases are separated by the workgroup barrier, which for a one-wave workgroup is a
// memory fence and nothing to wait for: no wave ever waits on another wave.  Every loop is
// bounded by max_iter, N, K or dim; there are no atomics.  A fit's result depends on its
// own inputs only: not on its position, the chunking or KM.  The observations are read
// where the subjects' sequences already lie; nothing is copied.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_gmm.h"
#include "vbhmm_gmm_run.h"

namespace vbhem {
namespace {

using namespace gmmrun;

struct GmmArgs {
  int R0, S, Ntot, dim, max_obs, max_iter;
  double tolfun;
  const int *offsets, *seq_first, *subject, *K, *rows;
  const double *x, *reg;
  double *prior, *mean, *cov, *ll, *lls, *post_init;
  int *iters, *status;
  Hyper h;
  double *ws;
  size_t slot;  // doubles per workgroup
};

template <int KM>
__global__ __launch_bounds__(64, KM == 4 ? 2 : 1) void vbhmm_gmm_kernel(const GmmArgs p) {
  __shared__ Fit<KM> f;
  const int lane = threadIdx.x;
  const int fit = p.R0 + blockIdx.x;
  const int dim = p.dim;
  // the fit's subject and start rows, checked against the sizes the workspace was made
  // for (uniform)
  const int sub = p.subject[fit], K = p.K[fit];
  const int *rows = p.rows + (size_t)fit * KM;
  bool ok = sub >= 0 && sub < p.S;
  int row0 = 0, N = 0;
  if (ok) {
    const int n0 = p.seq_first[sub], n1 = p.seq_first[sub + 1];
    ok = n0 >= 0 && n1 >= n0 && n1 <= p.Ntot;
    if (ok) {
      row0 = p.offsets[n0];
      N = p.offsets[n1] - row0;
      ok = row0 >= 0 && fit_valid(K, KM, N, p.max_obs, rows);
    }
  }
  if (!ok) {
    if (lane == 0) p.status[fit] = kBadFit;
    return;
  }
  const double *x = p.x + (size_t)row0 * dim;
  double *slot = p.ws + (size_t)blockIdx.x * p.slot;
  const Work w{slot, slot + (size_t)p.max_obs * KM};

  if (lane == 0) {
    f.K = K;
    f.dim = dim;
    f.N = N;
    f.reg = p.reg[fit];
    f.ll = __builtin_nan("");
    f.last = -INFINITY;
    f.flags = 0;
  }
  __syncthreads();
  if (lane < dim) start_var(f, x, lane);
  if (lane < K * dim) start_mean(f, x, rows, lane / dim, lane % dim);
  __syncthreads();
  for (int e = lane; e < K * dim * dim; e += 64) start_cov(f, e / (dim * dim), (e / dim) % dim, e % dim);
  __syncthreads();

  int it = 1;
  bool ill = false;
  for (; it <= p.max_iter; ++it) {
    if (lane < K) factor_state(f, lane);
    __syncthreads();
    if (any_bad(f)) {
      ill = true;
      break;
    }
    for (int n = lane; n < N; n += 64) estep_obs<KM>(f, x + (size_t)n * dim, w.post + (size_t)n * KM, w.lse + n);
    __syncthreads();
    if (lane < K) stat_nk(f, w, lane);
    else if (lane == K) stat_ll(f, w);
    __syncthreads();
    if (lane < K * dim) stat_mean(f, x, w, lane / dim, lane % dim);
    __syncthreads();
    for (int e = lane; e < K * dim * dim; e += 64) stat_cov(f, x, w, e / (dim * dim), (e / dim) % dim, e % dim);
    if (lane == 0) {
      loop_control(f, it, p.max_iter, p.tolfun);
      if (p.lls) p.lls[(size_t)fit * p.max_iter + (it - 1)] = f.ll;
    }
    __syncthreads();
    if (f.flags & 1) break;
  }
  if (lane == 0) {
    p.ll[fit] = f.ll;
    p.iters[fit] = it > p.max_iter ? p.max_iter : it;
    p.status[fit] = ill ? kIllConditioned : status_of(f.flags);
  }
  if (ill) return;
  if (lane < K) p.prior[(size_t)fit * KM + lane] = f.pi[lane];
  if (lane < K * dim) p.mean[(size_t)fit * KM * dim + lane] = f.mu[lane];
  for (int e = lane; e < K * dim * dim; e += 64) p.cov[(size_t)fit * KM * dim * dim + e] = f.cov[e];
  if (p.post_init) {
    const int PL = emrun::post_len(KM, dim);
    double *post = p.post_init + (size_t)fit * PL;
    for (int q = lane; q < PL; q += 64) post[q] = post_padding(KM, dim, q);
    __syncthreads();
    if (lane < K) init_posterior_state(f, p.h, lane, post);
  }
}

size_t slot_doubles(int KM, int max_obs) { return (size_t)std::max(max_obs, 1) * obs_len(KM); }

// Fits per launch: the caller's, or the default -- VBHMM_EM_DEFAULT_CHUNK fits, fewer where
// their workspace would pass VBHMM_EM_DEFAULT_WORKSPACE bytes.
int chunk_of(int chunk_runs, size_t slot) {
  if (chunk_runs > 0) return chunk_runs;
  const size_t fit = (size_t)VBHMM_EM_DEFAULT_WORKSPACE / (slot * sizeof(double));
  return (int)std::max<size_t>(1, std::min<size_t>(VBHMM_EM_DEFAULT_CHUNK, fit));
}

int check_sizes(const vbhmm_em_subjects_t *sb, int R, int KM) {
  if (!sb) return set_error(VBHEM_ERR_ARG, "vbhmm_gmm: null subjects");
  if (sb->S < 1 || sb->seqs.N < 0 || sb->seqs.dim < 1 || sb->max_obs < 0 || R < 0 || KM < 1)
    return set_error(VBHEM_ERR_ARG, "vbhmm_gmm: need S >= 1, dim >= 1, KM >= 1 and non-negative counts");
  if (sb->seqs.dim > kMaxDim || KM > kMaxStates)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_gmm: K <= 8 and dim <= 8 supported");
  if (KM != 4 && KM != 8) return set_error(VBHEM_ERR_ARG, "vbhmm_gmm: KM is 4 or 8");
  return VBHEM_OK;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_gmm_fit_workspace_bytes(const vbhmm_em_subjects_t *sb, int R, int KM, int chunk_runs) {
  using namespace vbhem;
  if (check_sizes(sb, R, KM) != VBHEM_OK) return 0;
  const size_t slot = slot_doubles(KM, sb->max_obs);
  return std::max<size_t>(256, (size_t)std::min(R, chunk_of(chunk_runs, slot)) * slot * sizeof(double));
}

int vbhmm_gmm_fit_batch(const vbhmm_em_subjects_t *sb, const vbhmm_gmm_fits_t *fits, const vbhmm_gmm_opt_t *opt,
                        double *prior_dev, double *mean_dev, double *cov_dev, double *ll_dev, int *iters_dev,
                        int *status_dev, double *lls_dev, const vbhmm_em_hyper_t *hyper, double *post_init_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  if (!fits || !opt) return set_error(VBHEM_ERR_ARG, "vbhmm_gmm_fit_batch: null descriptor");
  const int rc = check_sizes(sb, fits->R, fits->KM);
  if (rc != VBHEM_OK) return rc;
  if (opt->max_iter < 1 || opt->chunk_runs < 0)
    return set_error(VBHEM_ERR_ARG, "vbhmm_gmm_fit_batch: need max_iter >= 1 and chunk_runs >= 0");
  if ((hyper == nullptr) != (post_init_dev == nullptr))
    return set_error(VBHEM_ERR_ARG, "vbhmm_gmm_fit_batch: hyper and post_init go together");
  if (fits->R == 0) return VBHEM_OK;
  if (!sb->seqs.offsets || !sb->seqs.x || !sb->seq_first || !fits->subject || !fits->K || !fits->rows ||
      !fits->reg || !prior_dev || !mean_dev || !cov_dev || !ll_dev || !iters_dev || !status_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_gmm_fit_batch: null array");
  GmmArgs a{};
  a.S = sb->S; a.Ntot = sb->seqs.N; a.dim = sb->seqs.dim; a.max_obs = sb->max_obs;
  a.offsets = sb->seqs.offsets; a.x = sb->seqs.x; a.seq_first = sb->seq_first;
  a.subject = fits->subject; a.K = fits->K; a.rows = fits->rows; a.reg = fits->reg;
  a.max_iter = opt->max_iter;
  a.tolfun = opt->tolfun;
  a.prior = prior_dev; a.mean = mean_dev; a.cov = cov_dev; a.ll = ll_dev; a.lls = lls_dev;
  a.iters = iters_dev; a.status = status_dev; a.post_init = post_init_dev;
  if (hyper) {
    a.h.alpha0 = hyper->alpha0; a.h.epsilon0 = hyper->epsilon0; a.h.beta0 = hyper->beta0; a.h.v0 = hyper->v0;
    for (int q = 0; q < kMaxDim; ++q) {
      a.h.m0[q] = q < a.dim ? hyper->m0[q] : 0.0;
      a.h.W0inv[q] = q < a.dim ? hyper->W0inv_diag[q] : 1.0;
    }
  }
  const int R = fits->R, KM = fits->KM;
  a.slot = slot_doubles(KM, a.max_obs);
  const int chunk = chunk_of(opt->chunk_runs, a.slot);
  const size_t need = (size_t)std::min(R, chunk) * a.slot * sizeof(double);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  a.ws = static_cast<double *>(workspace_dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int r0 = 0; r0 < R; r0 += chunk) {
    a.R0 = r0;
    const unsigned n = (unsigned)std::min(chunk, R - r0);
    if (KM == 4)
      hipLaunchKernelGGL(vbhmm_gmm_kernel<4>, dim3(n), dim3(64), 0, st, a);
    else
      hipLaunchKernelGGL(vbhmm_gmm_kernel<8>, dim3(n), dim3(64), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "vbhmm_gmm_kernel");
  }
  return VBHEM_OK;
}

}  // extern "C"
