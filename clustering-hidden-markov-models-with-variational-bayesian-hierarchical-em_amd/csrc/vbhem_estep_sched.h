// vbhem_estep_sched.h -- what the C ABI (vbhem_capi.hip) calls of the E-step's
// scheduler (vbhem_estep_sched.hip): workspace sizes and the two calls' schedules,
// entered after the argument checks.
#pragma once
#include <cstddef>

#include "vbhem_estep.h"

namespace vbhem {

// bytes of workspace (need_tnu: sum_t_nu is not an output and lives in the workspace)
size_t pairs_workspace_bytes(const vbhem_base_t *b, const vbhem_cluster_t *c, int T, bool need_tnu);
size_t fused_workspace_bytes(const vbhem_base_t *b, const vbhem_cluster_t *c, int T, int R);

// vbhem_estep_pairs / vhem_estep_pairs (smooth) on checked arguments, N > 0
int sched_estep_pairs(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T, double smooth,
                      double *LL_elbo_dev, double *sum_nu_1_dev, double *emit_pr_dev,
                      double *emit_mu_dev, double *emit_Mu_dev, double *sum_xi_dev,
                      double *sum_t_nu_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

// the VHEM mode of the fused call (vhem_estep_fused*): null for VBHEM
struct VhemIn {
  double smooth, inf_norm;
  const double *omegaB;
};
// vbhem_estep_fused_trials / vhem_estep_fused_trials on checked arguments; done_word
// (optional): the completion word armed for this call (vbhem_arm_done_word)
int sched_estep_fused(const vbhem_base_t *base, const vbhem_cluster_t *clus, int R, int T,
                      const double *tildeN_dev, const double *logOmega_dev, double *stats_dev,
                      double *hatZ_dev, double *LL_elbo_dev, void *workspace_dev,
                      size_t workspace_bytes, void *stream, const VhemIn *vh,
                      unsigned long long *done_word, unsigned long long done_val);

// vbhem_last_kernel
const char *last_kernel(int pass);

}  // namespace vbhem

// (exported for the tests, not part of the public interface) where the fused call of R
// trials carves its gated schedule's buffers in the workspace: out [5] = bases per group,
// then the byte offsets of the gate lists ([K][group] ints), their totals ([K] ints), the
// gate masks ([group] 64-bit words; -1: none, K > 64) and the exact fallback's scratch,
// which comes last; returns the workspace's bytes (0: bad arguments)
extern "C" size_t vbhem_fused_workspace_layout(const vbhem_base_t *base, const vbhem_cluster_t *clus,
                                               int T, int R, long long *out);

// (exported for the tests) fb_bwd4_kernel's persistent grid for K clusters of nbases bases on
// the current device: out [3] = bases per quad (one wave's tile), waves per block, blocks per
// cluster.  A wave takes every (blocks per cluster x waves per block)-th quad of its cluster.
extern "C" int vbhem_bwd4_launch_plan(int K, int nbases, int *out);
