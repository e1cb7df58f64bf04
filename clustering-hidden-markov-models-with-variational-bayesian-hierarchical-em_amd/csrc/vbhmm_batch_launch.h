// vbhmm_batch_launch.h -- the host side that the wave-per-item routines share
// (vbhmm_em.hip: a run per wavefront; vbhmm_gmm.hip: a fit per wavefront): the check of
// the subjects descriptor, the items per launch, the workspace check and the chunked
// launch loop over the <4> / <8> instantiations of a kernel, and the hyperparameters as
// the run routines take them.  Not part of the public interface.
#pragma once
#include <algorithm>
#include <string>

#include "vbhem_internal.h"
#include "vbhmm_em.h"
#include "vbhmm_em_run.h"

namespace vbhem {
namespace batch {

// `who` names the caller in the message; max_seqs: the descriptor's, where the routine
// sizes its workspace by it (else 0)
inline int check_sizes(const std::string &who, const vbhmm_em_subjects_t *sb, int max_seqs, int R, int KM) {
  if (!sb) return set_error(VBHEM_ERR_ARG, who + ": null subjects");
  if (sb->S < 1 || sb->seqs.N < 0 || sb->seqs.dim < 1 || max_seqs < 0 || sb->max_obs < 0 || R < 0 || KM < 1)
    return set_error(VBHEM_ERR_ARG, who + ": need S >= 1, dim >= 1, KM >= 1 and non-negative counts");
  if (sb->seqs.dim > emrun::kMaxDim || KM > emrun::kMaxStates)
    return set_error(VBHEM_ERR_UNSUPPORTED, who + ": K <= 8 and dim <= 8 supported");
  if (KM != 4 && KM != 8) return set_error(VBHEM_ERR_ARG, who + ": KM is 4 or 8");
  return VBHEM_OK;
}

// Items per launch: the caller's, or the default -- VBHMM_EM_DEFAULT_CHUNK items (a launch
// of that many EM runs at 25 sequences x 50 observations takes 0.13 s),
// fewer where their workspace (slot doubles each) would pass VBHMM_EM_DEFAULT_WORKSPACE
// bytes.
inline int chunk_of(int chunk_runs, size_t slot) {
  if (chunk_runs > 0) return chunk_runs;
  const size_t fit = (size_t)VBHMM_EM_DEFAULT_WORKSPACE / (slot * sizeof(double));
  return (int)std::max<size_t>(1, std::min<size_t>(VBHMM_EM_DEFAULT_CHUNK, fit));
}

inline size_t workspace_bytes(int R, int chunk_runs, size_t slot) {
  return std::max<size_t>(256, (size_t)std::min(R, chunk_of(chunk_runs, slot)) * slot * sizeof(double));
}

// The R items of a (a.slot set) in launches of one wavefront per item: a.ws, then a.R0
// per launch.  k4 / k8: the kernel's instantiations for KM = 4 and 8.
template <class Args>
inline int launch_chunks(Args &a, int R, int KM, int chunk_runs, void *workspace_dev, size_t workspace_bytes,
                         hipStream_t st, void (*k4)(const Args), void (*k8)(const Args), const char *kernel) {
  const int chunk = chunk_of(chunk_runs, a.slot);
  const size_t need = (size_t)std::min(R, chunk) * a.slot * sizeof(double);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  a.ws = static_cast<double *>(workspace_dev);
  for (int r0 = 0; r0 < R; r0 += chunk) {
    a.R0 = r0;
    const unsigned n = (unsigned)std::min(chunk, R - r0);
    hipLaunchKernelGGL(KM == 4 ? k4 : k8, dim3(n), dim3(64), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, kernel);
  }
  return VBHEM_OK;
}

// entries past dim: m0 0, W0inv 1 (never read into a result)
inline emrun::Hyper to_hyper(const vbhmm_em_hyper_t *hy, int dim) {
  emrun::Hyper h;
  h.alpha0 = hy->alpha0; h.epsilon0 = hy->epsilon0; h.beta0 = hy->beta0; h.v0 = hy->v0;
  for (int q = 0; q < emrun::kMaxDim; ++q) {
    h.m0[q] = q < dim ? hy->m0[q] : 0.0;
    h.W0inv[q] = q < dim ? hy->W0inv_diag[q] : 1.0;
  }
  return h;
}

}  // namespace batch
}  // namespace vbhem
