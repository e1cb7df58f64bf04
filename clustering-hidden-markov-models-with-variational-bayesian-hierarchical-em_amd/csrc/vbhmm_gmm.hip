// vbhmm_gmm.hip -- the batched random-start GMM fit (include/vbhmm_gmm.h): every fit of a
// list, from its start rows to its last M-step, in one call; optionally the initial VB-HMM
// posterior of each fitted GMM.  The arithmetic of a fit AND its schedule (run_fit) are
// vbhmm_gmm_run.h, shared with the host check build; the kernel's own are the check of the
// fit against the workspace sizes, the carving of the slot and the fit's ll / iters / status.
//
// vbhmm_gmm_kernel<KM>: a workgroup is ONE wavefront and owns ONE fit (fit = chunk start +
// blockIdx.x) for its whole EM; the fit's small state (pi, mu, cov, the factors L and their
// log-determinants: Fit<KM>) lives in the workgroup's LDS, the responsibilities [N][KM] and
// the row log-sum-exps [N] in the workspace slot of the workgroup.  run_fit with a unit per
// lane (emrun::WaveLanes) is, per iteration:
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
#include "vbhmm_batch_launch.h"
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

// <4> runs at 3 waves per SIMD and sits a few registers under the step to 2: its bound
// says so.
template <int KM>
__global__ __launch_bounds__(64, KM == 4 ? 3 : 1) void vbhmm_gmm_kernel(const GmmArgs p) {
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

  const FitResult res = run_fit<KM>(
      emrun::WaveLanes{lane}, f, K, dim, N, x, rows, p.reg[fit], p.max_iter, p.tolfun, p.prior + (size_t)fit * KM,
      p.mean + (size_t)fit * KM * dim, p.cov + (size_t)fit * KM * dim * dim,
      p.lls ? p.lls + (size_t)fit * p.max_iter : nullptr, &p.h,
      p.post_init ? p.post_init + (size_t)fit * emrun::post_len(KM, dim) : nullptr, w);
  if (lane == 0) {
    p.ll[fit] = res.ll;
    p.iters[fit] = res.iters;
    p.status[fit] = res.status;
  }
}

size_t slot_doubles(int KM, int max_obs) { return (size_t)std::max(max_obs, 1) * obs_len(KM); }

int check_sizes(const vbhmm_em_subjects_t *sb, int R, int KM) {
  return batch::check_sizes("vbhmm_gmm", sb, 0, R, KM);
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_gmm_fit_workspace_bytes(const vbhmm_em_subjects_t *sb, int R, int KM, int chunk_runs) {
  using namespace vbhem;
  if (check_sizes(sb, R, KM) != VBHEM_OK) return 0;
  return batch::workspace_bytes(R, chunk_runs, slot_doubles(KM, sb->max_obs));
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
  if (hyper) a.h = batch::to_hyper(hyper, a.dim);
  a.slot = slot_doubles(fits->KM, a.max_obs);
  return batch::launch_chunks(a, fits->R, fits->KM, opt->chunk_runs, workspace_dev, workspace_bytes,
                              static_cast<hipStream_t>(stream), vbhmm_gmm_kernel<4>, vbhmm_gmm_kernel<8>,
                              "vbhmm_gmm_kernel");
}

}  // extern "C"
