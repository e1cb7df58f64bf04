// vhem_em_trials.hip -- what follows the batched VHEM E-step in one EM iteration of R
// trials, with the stopping rule on the device (vhem_em_run_trials, vhem_em.hip).
//
// hem_h3m_c.m runs `trials` EM runs from their own initialisations; the batched E-step
// (vhem_estep_fused_trials) already takes the R trials of a chunk as one launch over
// R K clusters.  Here the rest of an iteration does too:
//
// vhem_iter_trials_kernel: one WAVEFRONT per (trial r, cluster k, state s), R K S in
// all, in blocks of 4 waves that straddle trial boundaries.  A wave reads its trial's
// record first and leaves if the trial is done (stopped or frozen) before any write.
// It then takes the trial's decision itself (trial_ctrl_decide, vhem_em_trial_ctrl.h:
// the record and the LogL slot of the statistics are all it needs): at a stop or a
// non-finite LogL it writes no parameter -- a stopping trial keeps the parameters that
// produced its stopping E-step -- otherwise it runs vhem_ks_body (vhem_em_iter_body.h):
// the M-step of (k, s) into the trial's parameters and the next E-step constants into
// the trial's slices of the trial-major cluster constants and of logOmega.  The last
// wave of a trial to finish (a ticket per trial, reset for the next launch) combines
// the waves' fallback flags and writes the record and the LogLs slot.  No wave waits
// for another (wave-private LDS and wave-level synchronisation only, no block barrier,
// no spinning).  The device never draws a random number: a trial that would need one of
// the degenerate fixes is flagged and frozen, and the host engine reruns it.
//
// vhem_trials_latch_kernel, after it, with the iteration number j: a trial that stopped
// at j gets its K columns of Z and L_elbo and its statistics copied aside (later E-steps
// overwrite them); a trial still running gets its E-step constants saved; a trial
// flagged at j gets the saved ones put back -- its clusters ride along in every later
// E-step, whose emission GEMM shifts by the mean of ALL clusters' means, so a frozen
// trial must always carry finite constants.  One wave then writes the number of running
// trials and j + 1 to mapped host memory, the sequence word last.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vhem_em_dev.h"
#include "vhem_em_iter_body.h"
#include "vhem_em_trial_ctrl.h"

namespace vhem {

namespace {

using vbhem::kWaves;

// trial r's view of the arguments
__device__ __forceinline__ KsArgs trial_view(const EmTrialsArgs &t, int r) {
  KsArgs a = t.a;
  const size_t K = (size_t)t.a.K, KS = K * t.a.S, d = (size_t)t.a.d;
  const size_t dd = t.a.covmode == 1 ? d * d : d;
  a.omega += r * K; a.prior += r * KS; a.vcounts += r * KS; a.A += r * KS * t.a.S;
  a.centres += r * KS * d; a.covars += r * KS * dd;
  a.logA += r * KS * t.a.S; a.logPi += r * KS; a.cm += r * KS * d; a.P += r * KS * dd;
  a.c += r * KS; a.logOmega += r * K;
  return a;
}

__global__ __launch_bounds__(64 * kWaves) void vhem_iter_trials_kernel(const EmTrialsArgs t,
                                                                       int j) {
  __shared__ double glds[kWaves][2 * kBodyMaxD * kBodyMaxD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = t.a.K, S = t.a.S, KS = K * S;
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wave);  // wave-uniform
  if (w >= t.R * KS) return;
  const int r = w / KS, ks = w - r * KS;
  TrialCtrl *cp = t.ctrl + r;
  // read before this wave's ticket, so before the trial's last wave can write it
  const TrialCtrl c0 = *cp;
  if (c0.done) return;  // stopped or frozen
  KsArgs a = trial_view(t, r);
  int what = kTrialContinue;
  double new_LL = 0.0;
  if (j >= 0) {
    a.stats = t.a.stats + (size_t)r * t.stats_len;
    new_LL = a.stats[(size_t)K + KS + (size_t)KS * S];  // LogL, the Lt1 slot
    what = trial_ctrl_decide(&c0, new_LL, t.max_iter, t.min_iter, t.termvalue);
  } else {
    a.stats = nullptr;  // the constants of the given parameters
  }
  int bad = 0;
  if (what == kTrialContinue) {
    DevWave dw;
    dw.lane = lane;
    bad = vhem_ks_body(a, ks, dw, glds[wave]);
  }

  // ---- the record: the trial's last wave ----
  if (lane == 0 && bad) atomicOr(t.flags + r, 1);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  int last = 0;
  if (lane == 0) last = atomicAdd(t.ticket + r, 1) == KS - 1;
  last = __shfl(last, 0, 64);
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (lane == 0) {
      const int anybad = atomicExch(t.flags + r, 0);  // ready for the next launch
      TrialCtrl c = c0;
      if (j < 0) {
        if (anybad) {
          c.done = 1;
          c.fallback = 1;
        }
      } else {
        if (what == kTrialContinue && anybad) what = kTrialFallback;
        const int slot = trial_ctrl_record(&c, what, new_LL, j);
        if (slot < t.ldL) t.LogLs[(size_t)r * t.ldL + slot] = new_LL;
      }
      *cp = c;
      t.ticket[r] = 0;  // ready for the next launch
    }
  }
}

constexpr int kLatchThreads = 256;

__global__ __launch_bounds__(kLatchThreads) void vhem_trials_latch_kernel(const EmTrialsArgs t,
                                                                          int j) {
  const int K = t.a.K, S = t.a.S, d = t.a.d, R = t.R, r = blockIdx.y;
  const size_t tid = (size_t)blockIdx.x * kLatchThreads + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * kLatchThreads;
  const TrialCtrl *cp = t.ctrl + r;
  const int done = cp->done, fallback = cp->fallback, stop_iter = cp->stop_iter;
  const int fb_iter = cp->fb_iter;
  if (done && !fallback && stop_iter == j) {
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
  const bool restore = done && fallback && fb_iter == j;
  if (restore || !done) {
    // logA | logPi | cm | P | c | logOmega, each [R] slices of n[q] doubles
    const bool full = t.a.covmode == 1;
    const size_t dd = full ? (size_t)d * d : (size_t)d, KS = (size_t)K * S;
    const size_t n[6] = {KS * S, KS, KS * d, KS * dd, KS, (size_t)K};
    // a trial flagged before its first E-step has nothing saved: uniform A and prior,
    // centres 0, unit covariances, equal weights
    const double neutral[6] = {-log((double)S), -log((double)S), 0.0, 1.0, 0.0, -log((double)K)};
    double *live = t.a.logA;
    size_t base = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const size_t o = base + (size_t)r * n[q];
      for (size_t x = tid; x < n[q]; x += stride) {
        if (!restore) {
          t.backup[o + x] = live[o + x];
        } else if (j >= 0) {
          live[o + x] = t.backup[o + x];
        } else {
          double v = neutral[q];
          if (q == 3 && full) {
            const size_t e = x % dd;
            v = e / d == e % d ? 1.0 : 0.0;
          }
          live[o + x] = v;
        }
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

hipError_t launch_em_trials(const EmTrialsArgs &t, int j, hipStream_t st) {
  const KsArgs &a = t.a;
  if (a.d < 1 || a.d > kBodyMaxD || a.S < 1 || a.S > kBodyMaxD || a.K < 1 || t.R < 1 || !t.ctrl ||
      !t.ticket || !t.flags || !t.LogLs || t.ldL < t.max_iter + 2 || !a.omega || !a.prior || !a.A ||
      !a.centres || !a.covars || !a.vcounts || !a.logA || !a.logPi || !a.cm || !a.P || !a.c ||
      !a.logOmega || (j >= 0 && !a.stats))
    return hipErrorInvalidValue;
  const int nw = t.R * a.K * a.S;
  hipLaunchKernelGGL(vhem_iter_trials_kernel, dim3((nw + kWaves - 1) / kWaves), dim3(64 * kWaves), 0,
                     st, t, j);
  return hipGetLastError();
}

hipError_t launch_trials_latch(const EmTrialsArgs &t, int j, hipStream_t st) {
  if (t.R < 1 || !t.ctrl || !t.backup || !t.hz || !t.ll || !t.hz_out || !t.ll_out || !t.stats_out ||
      !t.a.logA || (j >= 0 && (!t.flag || !t.active || !t.a.stats)))
    return hipErrorInvalidValue;
  // enough blocks per trial for its longest copy, at most 32
  const int d = t.a.d, KS = t.a.K * t.a.S;
  const size_t dd = t.a.covmode == 1 ? (size_t)d * d : (size_t)d;
  size_t longest = (size_t)t.N * t.a.K;
  if (t.stats_len > longest) longest = t.stats_len;
  if ((size_t)KS * dd > longest) longest = (size_t)KS * dd;
  size_t nb = (longest + kLatchThreads - 1) / kLatchThreads;
  nb = nb < 1 ? 1 : nb > 32 ? 32 : nb;
  hipLaunchKernelGGL(vhem_trials_latch_kernel, dim3((unsigned)nb, (unsigned)t.R), dim3(kLatchThreads),
                     0, st, t, j);
  return hipGetLastError();
}

}  // namespace vhem
