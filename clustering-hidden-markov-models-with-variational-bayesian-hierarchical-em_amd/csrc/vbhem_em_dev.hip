// vbhem_em_dev.hip -- the per-iteration host math of the EM loop, on the device.
//
// vbhem_h3m_c_step_fc.m runs, between two E-steps, the lower bound (vbhemh3m_lb.m:
// 64-186), the M-step (vbhem_compute_Statistics.m:57-82, vbhem_mstep_component.m:
// 42-70, :396) and the next iteration's psi prelude (:118-165, 180-191, 271-273).
// vbhem_em.hip has them in C++ on the host; here the same arithmetic is ONE kernel on
// the E-step's stream, so an EM iteration never leaves the GPU: the packed
// statistics are read where the statistics kernel (and the all-reduce) left them,
// the prelude writes the next E-step's cluster constants in place, and only the
// bound (one double) goes to the host, for the convergence test.
//
// em_iter_kernel: one WAVEFRONT per cluster state (k, s).  Each does, with its
// lanes working in parallel:
//   1. the (k, s) terms of the bound for the current posterior (lgammas over the
//      lanes, the quadratic forms over lanes = matrix entries), written as partial
//      sums; the last wave to finish (a ticket counter) reduces all of them in a
//      fixed order and writes L (deterministic);
//   2. the M-step of (k, s) into the other posterior buffer: the d x d inverse of
//      W0^-1 + Nr SC + mult1 dd' by Gauss-Jordan elimination without row exchanges
//      (the operand is symmetric positive definite; see gauss_jordan) in
//      wave-private LDS, lanes = entries of [A | I];
//   3. the prelude of the new (k, s): logLambdaTilde (psi over the lanes, det W by
//      the same elimination), c, P = v W, m, its logATilde row, logPiTilde and (one
//      wave per cluster) logOmega -- the sums over a cluster's states or over all
//      clusters are recomputed by every wave that needs them, in one fixed order.
// A prelude-only launch (no bound, no M-step) starts the loop.
// The per-(k, s) arithmetic is in vbhem_em_iter_body.h, shared with the batched-trials
// kernel (vbhem_em_trials.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "vbhem_em_dev.h"
#include "vbhem_special.h"

#ifdef EMDEV_TIMING
namespace vbhem {
namespace {
__device__ long long emdev_t[8][1024];  // [phase][wave]: s_memrealtime (100 MHz)
}
}  // namespace vbhem
#define EMDEV_MARK(ph)                                                  \
  if (lane == 0 && ks < 1024) emdev_t[ph][ks] = __builtin_amdgcn_s_memrealtime()
#endif
#include "vbhem_em_iter_body.h"

namespace vbhem {

namespace {

__global__ __launch_bounds__(64 * kWaves) void em_iter_kernel(const EmDevArgs a, int mode,
                                                              double *L_out) {
  __shared__ double glds[kWaves][2 * kEmDevMaxD * kEmDevMaxD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K, S = a.S;
  const int ks = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wave);  // wave-uniform
  if (ks >= K * S) return;
  const bool iterate = mode == kEmIterate;
  // (the view is built in both modes: a.stats is always a valid buffer, so a load
  // the compiler hoists out of an `iterate ? stats : posterior` select cannot fault)
  const StatsView st(a.stats, K, S);
  EMDEV_MARK(0);
  em_ks_body(a, iterate, ks, lane, glds[wave], st);

  EMDEV_MARK(6);
  // ---- the bound: the last wave reduces every (k, s)'s partial sums ----
  if (iterate) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int last = 0;
    if (lane == 0) last = atomicAdd(a.ticket, 1) == K * S - 1;
    last = __shfl(last, 0, 64);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const double L = em_bound_total(a, st, lane);
      if (lane == 0) {
        *L_out = L;
        *a.ticket = 0;  // ready for the next launch
        EMDEV_MARK(7);
        if (a.flag) {   // the host polls this word (mapped memory) instead of syncing
          __threadfence_system();
          __hip_atomic_store(a.flag, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  }
}

}  // namespace

bool em_dev_supported(int d, int S) { return d >= 1 && d <= kEmDevMaxD && S >= 1 && S <= 32; }

hipError_t launch_em_dev(const EmDevArgs &a, int mode, double *L_out, hipStream_t st) {
  if (!em_dev_supported(a.d, a.S) || (mode == kEmIterate && (!L_out || !a.ticket || !a.part)))
    return hipErrorInvalidValue;
  const int nw = a.K * a.S;
  hipLaunchKernelGGL(em_iter_kernel, dim3((nw + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, st, a,
                     mode, L_out);
  return hipGetLastError();
}

}  // namespace vbhem
