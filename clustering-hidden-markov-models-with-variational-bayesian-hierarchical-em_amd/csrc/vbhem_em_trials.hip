// vbhem_em_trials.hip -- the per-iteration math of R EM trials in one launch, with
// the stopping rule on the device (vbhem_em_run_trials, vbhem_em.hip).
//
// vbhem_h3m_c.m:28-67 runs `trials` EM runs from their own initialisations; the
// batched E-step (vbhem_estep_fused_trials) already takes the R trials of a (K, S)
// cell as one launch over R K clusters.  Here the rest of an iteration does too:
//
// em_iter_trials_kernel: one WAVEFRONT per (trial r, cluster k, state s), R K S in
// all, each running em_ks_body (vbhem_em_iter_body.h: the arithmetic of
// em_iter_kernel, vbhem_em_dev.hip) on pointers that address its trial: the
// statistics at stats + r stats_len, the posterior buffer ctrl[r].cur, the M-step
// into the trial's other buffer, the prelude into the trial's slices of the
// trial-major cluster constants and of logOmega, and the trial's OWN hyperparameters
// (its table at hyp + r hyp_stride, vbhem_em_deriv_terms.h; vbhem_em_run_trials fills
// R copies of one, vbhem_em_run_trials_hyp one per trial).  The last wave of a trial to
// finish (a ticket per trial) sums that trial's K S partials in em_iter_kernel's
// order, forms the bound and runs trial_ctrl_step (vbhem_em_trial_ctrl.h): record
// the bound, accept the M-step (flip cur), or stop.  The waves of a trial whose
// record says done leave before any write: its posterior, its constants and its
// record never change again, while its clusters ride along in the later E-steps.
// Blocks of 4 waves straddle trial boundaries; no wave waits for another (wave-private
// LDS and wave-level synchronisation only, no block barrier, no spinning).
//
// trials_latch_kernel, after it, with the iteration number j: a trial that stopped
// at j gets its K columns of hat_Z and L_elbo and its statistics copied aside (later
// E-steps overwrite them); a trial still running gets its E-step constants saved,
// and a trial whose bound was NaN at j gets the saved ones put back -- its M-step was
// not accepted, and the prelude of a NaN posterior must not reach the next E-step,
// whose emission GEMM shifts by the mean of ALL clusters' means.  One wave then
// writes the number of running trials and j + 1 to mapped host memory.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vbhem_em_deriv_terms.h"
#include "vbhem_em_dev.h"
#include "vbhem_em_iter_body.h"
#include "vbhem_em_trial_ctrl.h"
#include "vbhem_special.h"

namespace vbhem {

namespace {

__global__ __launch_bounds__(64 * kWaves) void em_iter_trials_kernel(const EmTrialsArgs t,
                                                                     int mode) {
  __shared__ double glds[kWaves][2 * kEmDevMaxD * kEmDevMaxD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = t.a.K, S = t.a.S, d = t.a.d, KS = K * S;
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wave);  // wave-uniform
  if (w >= t.R * KS) return;
  const int r = w / KS, ks = w - r * KS;
  TrialCtrl *cp = t.ctrl + r;
  // read before this wave's ticket, so before the trial's last wave can write it
  const int done = cp->done, cur = cp->cur;
  if (done) return;  // frozen
  const bool iterate = mode == kEmIterate;
  const size_t dd = t.a.covmode == 1 ? (size_t)d * d : (size_t)d;
  // this trial's view of the arguments
  EmDevArgs a = t.a;
  const size_t in = ((size_t)cur * t.R + r) * t.postn, out = ((size_t)(cur ^ 1) * t.R + r) * t.postn;
  a.alpha = t.a.alpha + in; a.eta = t.a.eta + in; a.eps = t.a.eps + in; a.lam = t.a.lam + in;
  a.v = t.a.v + in; a.m = t.a.m + in; a.W = t.a.W + in;
  a.alpha_o = const_cast<double *>(t.a.alpha) + out; a.eta_o = const_cast<double *>(t.a.eta) + out;
  a.eps_o = const_cast<double *>(t.a.eps) + out; a.lam_o = const_cast<double *>(t.a.lam) + out;
  a.v_o = const_cast<double *>(t.a.v) + out; a.m_o = const_cast<double *>(t.a.m) + out;
  a.W_o = const_cast<double *>(t.a.W) + out;
  a.stats = t.a.stats + (size_t)r * t.stats_len;
  a.logA = t.a.logA + (size_t)r * KS * S; a.logPi = t.a.logPi + (size_t)r * KS;
  a.cm = t.a.cm + (size_t)r * KS * d; a.P = t.a.P + (size_t)r * KS * dd;
  a.c = t.a.c + (size_t)r * KS; a.lLT = t.a.lLT + (size_t)r * KS;
  a.logOmega = t.a.logOmega + (size_t)r * K; a.logdetW = t.a.logdetW + (size_t)r * KS;
  a.part = t.a.part + (size_t)r * kNQ * KS;
  // ... and its own hyperparameters (wave-uniform reads of the trial's table)
  const double *h = t.hyp + (size_t)r * t.hyp_stride;
  a.alpha0 = h[kHypAlpha0]; a.eta0 = h[kHypEta0]; a.epsilon0 = h[kHypEpsilon0];
  a.lambda0 = h[kHypLambda0]; a.v0 = h[kHypV0];
  a.logCalpha0 = h[kHypLogCalpha0]; a.logCeta0 = h[kHypLogCeta0];
  a.logCepsilon0 = h[kHypLogCepsilon0]; a.logB0 = h[kHypLogB0];
  a.m0 = h + kHypM0; a.W0inv = h + kHypM0 + d;
  const StatsView st(a.stats, K, S);
  em_ks_body(a, iterate, ks, lane, glds[wave], st);

  // ---- the bound and the decision: the trial's last wave ----
  if (iterate) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int last = 0;
    if (lane == 0) last = atomicAdd(t.ticket + r, 1) == KS - 1;
    last = __shfl(last, 0, 64);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const double L = em_bound_total(a, st, lane);
      if (lane == 0) {
        TrialCtrl c = *cp;
        const int slot = trial_ctrl_step(&c, L, t.max_iter, t.minDiff);
        if (slot >= 0 && slot < t.ldL) t.LogLs[(size_t)r * t.ldL + slot] = L;
        *cp = c;
        t.ticket[r] = 0;  // ready for the next launch
      }
    }
  }
}

constexpr int kLatchThreads = 256;

__global__ __launch_bounds__(kLatchThreads) void trials_latch_kernel(const EmTrialsArgs t, int j) {
  const int K = t.a.K, S = t.a.S, d = t.a.d, R = t.R, r = blockIdx.y;
  const size_t tid = (size_t)blockIdx.x * kLatchThreads + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * kLatchThreads;
  const TrialCtrl *cp = t.ctrl + r;
  const int done = cp->done, stable = cp->stable, stop_iter = cp->stop_iter;
  if (done && stop_iter == j) {
    // the E-step of the trial's own stopping iteration
    const size_t RK = (size_t)R * K;
    for (size_t x = tid; x < (size_t)t.N * K; x += stride) {
      const size_t i = x / K, k = x - i * K, o = i * RK + (size_t)r * K + k;
      t.hz_out[o] = t.hz[o];
      t.ll_out[o] = t.ll[o];
    }
    for (size_t x = tid; x < t.stats_len; x += stride)
      t.stats_out[(size_t)r * t.stats_len + x] = t.a.stats[(size_t)r * t.stats_len + x];
  }
  const bool restore = done && stop_iter == j && !stable;
  if (restore || !done) {
    // logA | logPi | cm | P | c | logOmega, each [R] slices of n[q] doubles
    const size_t dd = t.a.covmode == 1 ? (size_t)d * d : (size_t)d, KS = (size_t)K * S;
    const size_t n[6] = {KS * S, KS, KS * d, KS * dd, KS, (size_t)K};
    double *live = t.a.logA;
    size_t base = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const size_t o = base + (size_t)r * n[q];
      for (size_t x = tid; x < n[q]; x += stride) {
        if (restore) live[o + x] = t.backup[o + x];
        else t.backup[o + x] = live[o + x];
      }
      base += (size_t)R * n[q];
    }
  }
  // the word the host waits for (it reads results only after the stream has drained;
  // the count depends on the records alone, which the kernel before this one wrote)
  if (j >= 0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
    int nrun = 0;
    for (int q = threadIdx.x; q < R; q += 64) nrun += t.ctrl[q].done ? 0 : 1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nrun += __shfl_xor(nrun, o, 64);
    if (threadIdx.x == 0) {
      t.active[j & 1] = nrun;
      __threadfence_system();
      __hip_atomic_store(t.flag + (j & 1), j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

hipError_t launch_em_trials(const EmTrialsArgs &t, int mode, hipStream_t st) {
  if (!em_dev_supported(t.a.d, t.a.S) || t.R < 1 || !t.ctrl || !t.ticket || !t.LogLs || !t.a.part ||
      !t.hyp || t.hyp_stride < (size_t)hyp_table_len(t.a.d) || t.ldL < t.max_iter + 1)
    return hipErrorInvalidValue;
  const int nw = t.R * t.a.K * t.a.S;
  hipLaunchKernelGGL(em_iter_trials_kernel, dim3((nw + kWaves - 1) / kWaves), dim3(64 * kWaves), 0,
                     st, t, mode);
  return hipGetLastError();
}

hipError_t launch_trials_latch(const EmTrialsArgs &t, int j, hipStream_t st) {
  if (t.R < 1 || !t.ctrl || !t.backup || !t.hz || !t.ll || !t.hz_out || !t.ll_out || !t.stats_out ||
      (j >= 0 && (!t.flag || !t.active)))
    return hipErrorInvalidValue;
  // enough blocks per trial for its longest copy, at most 32
  const int d = t.a.d, KS = t.a.K * t.a.S;
  const size_t dd = t.a.covmode == 1 ? (size_t)d * d : (size_t)d;
  size_t longest = (size_t)t.N * t.a.K;
  if (t.stats_len > longest) longest = t.stats_len;
  if ((size_t)KS * dd > longest) longest = (size_t)KS * dd;
  size_t nb = (longest + kLatchThreads - 1) / kLatchThreads;
  nb = nb < 1 ? 1 : nb > 32 ? 32 : nb;
  hipLaunchKernelGGL(trials_latch_kernel, dim3((unsigned)nb, (unsigned)t.R), dim3(kLatchThreads), 0,
                     st, t, j);
  return hipGetLastError();
}

}  // namespace vbhem
