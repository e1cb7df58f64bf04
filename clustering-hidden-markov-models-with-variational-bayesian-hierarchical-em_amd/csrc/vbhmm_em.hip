// vbhmm_em.hip -- the fused, batched VB-HMM EM (include/vbhmm_em.h): the whole EM of every
// run of a list in one call, no host round trip inside the loop.  The arithmetic of a run
// AND its schedule (run_em) are vbhmm_em_run.h, shared with the host check build; the
// kernel's own are the check of the run against the workspace sizes, the carving of the
// slot (or of the caller's gamma array) and the run's LL / iters / status.
//
// vbhmm_em_kernel<KM>: a workgroup is ONE wavefront and owns ONE run (run = chunk start +
// blockIdx.x) for its whole EM; the run's small state (posterior, prelude, statistics,
// bound terms: Run<KM>) lives in the workgroup's LDS, its per-observation and per-sequence
// records in the workspace slot of the workgroup.  run_em with a unit per lane (WaveLanes)
// is, per iteration:
//   prelude   a lane per state
//   phase A   a lane per sequence, in rounds of 64 sequences (fb_sequence): gamma, logrho,
//             c_t, max_t to the slot, the sequence's record (sum xi, phi, sum gamma logrho,
//             sum_k gamma_1 logPi) after them
//   phase B   a lane per statistic entry -- (k), (i,j), then (k,a), then (k,a,b) -- each
//             walking the subject's observations (or sequences) in index order
//   bound     a lane per state, then lane 0 adds the states' terms and the sequences'
//             records in index order and takes the loop decision
//   M-step    a lane per state (Cholesky-based inverse in the state's own LDS slot)
// The phases are separated by the workgroup barrier, which for a one-wave workgroup is a
// memory fence and nothing to wait for: no wave ever waits on another wave.  Every loop is
// bounded by max_iter, a sequence count or a sequence length; there are no atomics.  A
// run's result depends on its own inputs only: not on its position, the chunking or KM.
//
// The gamma-only mode runs prelude + phase A once with gamma written to the caller's array.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_batch_launch.h"
#include "vbhmm_em.h"
#include "vbhmm_em_run.h"

namespace vbhem {
namespace {

using namespace emrun;

struct EmArgs {
  int R0, S, Ntot, dim, max_seqs, max_obs, max_iter;
  double min_diff;
  const int *offsets, *seq_first, *subject, *K;
  const double *x, *post;
  Hyper h;
  double *post_out, *post_estep, *stats, *LL, *LLs;
  int *iters, *status;
  double *ws;
  size_t slot;  // doubles per workgroup
  double *gamma_out;           // gamma-only mode when set
  const long long *gamma_row;  // [R]: first row of run r in gamma_out
};

template <int KM>
__global__ __launch_bounds__(64, KM == 4 ? 2 : 1) void vbhmm_em_kernel(const EmArgs p) {
  __shared__ Run<KM> r;
  const int lane = threadIdx.x;
  const int run = p.R0 + blockIdx.x;
  const int dim = p.dim;
  const bool gamma_only = p.gamma_out != nullptr;
  // the run's subject, checked against the sizes the workspace was made for (uniform)
  const int sub = p.subject[run], K = p.K[run];
  bool ok = sub >= 0 && sub < p.S && K >= 1 && K <= KM;
  int n0 = 0, N = 0, obs = 0;
  if (ok) {
    n0 = p.seq_first[sub];
    N = p.seq_first[sub + 1] - n0;
    ok = n0 >= 0 && N >= 0 && N <= p.max_seqs && n0 + N <= p.Ntot;
    if (ok) {
      obs = p.offsets[n0 + N] - p.offsets[n0];
      ok = p.offsets[n0] >= 0 && obs >= 0 && obs <= p.max_obs;
    }
  }
  if (!ok) {
    if (lane == 0) {
      if (p.status) p.status[run] = kBadRun;
      if (!gamma_only) {
        p.LL[run] = __builtin_nan("");
        p.iters[run] = 0;
      }
    }
    return;
  }
  const Subject s{N, p.offsets + n0, p.x};
  double *slot = p.ws + (size_t)blockIdx.x * p.slot;
  Work<KM> w;
  w.gamma = gamma_only ? p.gamma_out + (size_t)p.gamma_row[run] * KM : slot;
  w.logrho = slot + (size_t)p.max_obs * KM;
  w.cs = w.logrho + (size_t)p.max_obs * KM;
  w.mxs = w.cs + p.max_obs;
  w.seq = w.mxs + p.max_obs;

  const size_t PL = post_len(KM, dim), SL = stats_len(KM, dim);
  const int iters = run_em<KM>(WaveLanes{lane}, r, K, dim, s, p.h, p.max_iter, p.min_diff, p.post + run * PL,
                               gamma_only ? nullptr : p.post_out + run * PL,
                               p.post_estep ? p.post_estep + run * PL : nullptr,
                               p.stats ? p.stats + run * SL : nullptr,
                               p.LLs ? p.LLs + (size_t)run * p.max_iter : nullptr, w, gamma_only);
  if (lane != 0) return;
  if (gamma_only) {
    if (p.status) p.status[run] = kConverged;
    return;
  }
  p.LL[run] = r.L;
  p.iters[run] = iters;
  p.status[run] = status_of(r.flags);
}

size_t slot_doubles(int KM, int max_seqs, int max_obs) {
  return (size_t)std::max(max_obs, 1) * obs_len(KM) + (size_t)std::max(max_seqs, 1) * seq_len(KM);
}

int check_sizes(const vbhmm_em_subjects_t *sb, int R, int KM) {
  return batch::check_sizes("vbhmm_em", sb, sb ? sb->max_seqs : 0, R, KM);
}

int launch_chunks(EmArgs &a, int R, int KM, int chunk_runs, void *workspace_dev, size_t workspace_bytes,
                  hipStream_t st) {
  a.slot = slot_doubles(KM, a.max_seqs, a.max_obs);
  return batch::launch_chunks(a, R, KM, chunk_runs, workspace_dev, workspace_bytes, st, vbhmm_em_kernel<4>,
                              vbhmm_em_kernel<8>, "vbhmm_em_kernel");
}

void fill_common(EmArgs &a, const vbhmm_em_subjects_t *sb, const vbhmm_em_runs_t *runs) {
  a.S = sb->S; a.Ntot = sb->seqs.N; a.dim = sb->seqs.dim; a.max_seqs = sb->max_seqs; a.max_obs = sb->max_obs;
  a.offsets = sb->seqs.offsets; a.x = sb->seqs.x; a.seq_first = sb->seq_first;
  a.subject = runs->subject; a.K = runs->K; a.post = runs->post;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_em_post_len(int KM, int dim) { return (size_t)vbhem::emrun::post_len(KM, dim); }
size_t vbhmm_em_stats_len(int KM, int dim) { return (size_t)vbhem::emrun::stats_len(KM, dim); }

size_t vbhmm_em_batch_workspace_bytes(const vbhmm_em_subjects_t *sb, int R, int KM, int chunk_runs) {
  using namespace vbhem;
  if (check_sizes(sb, R, KM) != VBHEM_OK) return 0;
  return batch::workspace_bytes(R, chunk_runs, slot_doubles(KM, sb->max_seqs, sb->max_obs));
}

int vbhmm_em_batch(const vbhmm_em_subjects_t *sb, const vbhmm_em_runs_t *runs, const vbhmm_em_hyper_t *hyper,
                   const vbhmm_em_opt_t *opt, double *post_out_dev, double *post_estep_dev, double *stats_dev,
                   double *LL_dev, int *iters_dev, int *status_dev, double *LLs_dev, void *workspace_dev,
                   size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  if (!runs || !hyper || !opt) return set_error(VBHEM_ERR_ARG, "vbhmm_em_batch: null descriptor");
  const int rc = check_sizes(sb, runs->R, runs->KM);
  if (rc != VBHEM_OK) return rc;
  if (opt->max_iter < 1 || opt->chunk_runs < 0) return set_error(VBHEM_ERR_ARG, "vbhmm_em_batch: need max_iter >= 1");
  if (runs->R == 0) return VBHEM_OK;
  if (!sb->seqs.offsets || !sb->seqs.x || !sb->seq_first || !runs->subject || !runs->K || !runs->post ||
      !post_out_dev || !LL_dev || !iters_dev || !status_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_em_batch: null array");
  EmArgs a{};
  fill_common(a, sb, runs);
  a.max_iter = opt->max_iter;
  a.min_diff = opt->min_diff;
  a.h = batch::to_hyper(hyper, a.dim);
  a.post_out = post_out_dev; a.post_estep = post_estep_dev; a.stats = stats_dev;
  a.LL = LL_dev; a.iters = iters_dev; a.status = status_dev; a.LLs = LLs_dev;
  return launch_chunks(a, runs->R, runs->KM, opt->chunk_runs, workspace_dev, workspace_bytes,
                       static_cast<hipStream_t>(stream));
}

int vbhmm_em_gamma(const vbhmm_em_subjects_t *sb, const vbhmm_em_runs_t *runs, double *gamma_dev,
                   const long long *gamma_row_dev, int *status_dev, int chunk_runs, void *workspace_dev,
                   size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  if (!runs) return set_error(VBHEM_ERR_ARG, "vbhmm_em_gamma: null descriptor");
  const int rc = check_sizes(sb, runs->R, runs->KM);
  if (rc != VBHEM_OK) return rc;
  if (chunk_runs < 0) return set_error(VBHEM_ERR_ARG, "vbhmm_em_gamma: negative chunk");
  if (runs->R == 0) return VBHEM_OK;
  if (!sb->seqs.offsets || !sb->seqs.x || !sb->seq_first || !runs->subject || !runs->K || !runs->post ||
      !gamma_dev || !gamma_row_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_em_gamma: null array");
  EmArgs a{};
  fill_common(a, sb, runs);
  a.max_iter = 1;
  a.status = status_dev;
  a.gamma_out = gamma_dev;
  a.gamma_row = gamma_row_dev;
  return launch_chunks(a, runs->R, runs->KM, chunk_runs, workspace_dev, workspace_bytes,
                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
