// vbhem_em_trials_derivs.hip -- the bound's derivatives with respect to the
// hyperparameters (vbhemh3m_lb.m:202-345) of R EM trials in one launch, after the
// trials loop has stopped every trial (vbhem_em_run_trials_hyp, vbhem_em.hip).
//
// trials_derivs_kernel: one WAVEFRONT per (trial r, cluster k, state s), as
// em_iter_trials_kernel.  vbhem_h3m_c_step_fc.m:356-360 takes the derivatives at the
// posterior before the last accepted M-step: buffer cur ^ 1 of a stable trial with at
// least one accepted iteration.  Its prelude quantities are not recomputed: the
// trial's stopping iteration left, in its slices of `part` (frozen since), logOmega,
// logPi, the logA row sum and logLambdaTilde of exactly that posterior -- the numbers
// its last bound was formed from.  The rows of W (m - m0) go to lanes a < d, the
// 5 + W0_len + d terms to lanes q (vbhem_em_deriv_terms.h has the arithmetic, shared
// with the host check); the trial's last wave (the per-trial ticket of the iterate
// kernel) sums the K S terms of every derivative in one fixed order and adds the
// hyperparameter-only closed forms.  A trial that is unstable, inactive or stopped
// before any accepted iteration is left alone: the host writes its NaN.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vbhem_em_deriv_terms.h"
#include "vbhem_em_dev.h"
#include "vbhem_em_iter_body.h"
#include "vbhem_em_trial_ctrl.h"

namespace vbhem {

namespace {

__global__ __launch_bounds__(64 * kWaves) void trials_derivs_kernel(const EmTrialsArgs t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = t.a.K, S = t.a.S, d = t.a.d, KS = K * S, nW = t.W0_len, n = 5 + nW + d;
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wave);  // wave-uniform
  if (w >= t.R * KS) return;
  const int r = w / KS, ks = w - r * KS, k = ks / S, s = ks - k * S;
  const TrialCtrl *cp = t.ctrl + r;
  if (!cp->stable || cp->it < 1) return;
  const bool full = t.a.covmode == 1;
  const size_t dd = full ? (size_t)d * d : (size_t)d;
  const size_t in = ((size_t)(cp->cur ^ 1) * t.R + r) * t.postn;  // before the last M-step
  const double *h = t.hyp + (size_t)r * t.hyp_stride;
  const double *part = t.a.part + (size_t)r * kNQ * KS;  // 1 lLT, 6 logPi, 7 sum logA row, 9 logOmega
  const double v = t.a.v[in + ks], lam = t.a.lam[in + ks], l0 = h[kHypLambda0];
  DerivRow row = {0.0, 0.0, 0.0};
  if (lane < d)
    row = deriv_row(t.a.W + in + (size_t)ks * dd, t.a.m + in + (size_t)ks * d, h + kHypM0, d, full,
                    lane, l0, v);
  const double mWm = wsum(row.mwm), trW = wsum(row.wdiag);
  // lane q's row: W0 entry q - 5 (one per dimension), m0 entry q - 5 - nW
  const int a = lane >= 5 + nW ? lane - 5 - nW : (lane >= 5 && nW > 1 ? lane - 5 : 0);
  const int src = a < d ? a : 0;
  const double wdg = __shfl(row.wdiag, src, 64), gm = __shfl(row.gm, src, 64);
  double *terms = t.dterms + (size_t)r * n * KS;
  if (lane < n) {
    const double *W0inv = h + kHypM0 + d;
    double q;
    if (lane == 0) q = s == 0 ? part[(size_t)9 * KS + ks] : 0.0;
    else if (lane == 1) q = part[(size_t)6 * KS + ks];
    else if (lane == 2) q = part[(size_t)7 * KS + ks];
    else if (lane == 3) q = 0.5 * part[(size_t)1 * KS + ks];
    else if (lane == 4) q = deriv_lambda0_term(d, l0, lam, v, mWm);
    else if (lane < 5 + nW) q = nW == 1 ? deriv_w0_term(v, W0inv[0], trW) : deriv_w0_term(v, W0inv[a * d + a], wdg);
    else q = gm;
    terms[(size_t)lane * KS + ks] = q;  // quantity-major: one strided sum each below
  }

  // ---- the sums and the closed forms: the trial's last wave ----
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  int last = 0;
  if (lane == 0) last = atomicAdd(t.ticket + r, 1) == KS - 1;
  last = __shfl(last, 0, 64);
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double mine = 0.0;
  for (int q = 0; q < n; ++q) {
    double acc = 0.0;
    for (int j = lane; j < KS; j += 64) acc += terms[(size_t)q * KS + j];
    const double tot = wsum(acc);
    if (lane == q) mine = tot;
  }
  if (lane < n) t.dLL[(size_t)r * n + lane] = mine + deriv_closed_form(lane, K, S, d, nW, h);
  if (lane == 0) t.ticket[r] = 0;  // ready for the next launch
}

}  // namespace

hipError_t launch_trials_derivs(const EmTrialsArgs &t, hipStream_t st) {
  if (!em_dev_supported(t.a.d, t.a.S) || t.R < 1 || !t.ctrl || !t.ticket || !t.a.part || !t.hyp ||
      t.hyp_stride < (size_t)hyp_table_len(t.a.d) || !t.dterms || !t.dLL ||
      (t.W0_len != 1 && t.W0_len != t.a.d))
    return hipErrorInvalidValue;
  const int nw = t.R * t.a.K * t.a.S;
  hipLaunchKernelGGL(trials_derivs_kernel, dim3((nw + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, st,
                     t);
  return hipGetLastError();
}

}  // namespace vbhem
