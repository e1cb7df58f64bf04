// vhem_em.hip -- the VHEM EM loop of a chunk of trials on the device
// (include/vhem_em.h), host C++ around vhem_estep_fused_trials and the two kernels of
// vhem_em_trials.hip.
//
// Mirrors vhem.hem_h3m_c_trials (hem_h3m_c_step.m) without its per-iteration return to
// the host: the statistics stay on the device, the M-step and vhem_cluster_constants run
// there per (cluster, state), and the host reads one word per iteration -- the number
// of trials still running -- from mapped memory, with the next iteration already
// queued.  A stopped or frozen trial's waves leave before any write, so the iteration
// queued ahead cannot change a result.  The bounded wait and the mapped-memory pool are
// the VBHEM loop's (vbhem_em_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "vbhem_em_host.h"
#include "vbhem_internal.h"
#include "vhem_em.h"
#include "vhem_em_dev.h"
#include "vhem_em_trial_ctrl.h"

namespace {

// why a shape is outside vhem_em_run_trials (nullptr: supported)
const char *trials_unsupported(const vbhem_base_t *base, int K, int S, int R) {
  if (R < 1 || K < 1 || S < 1) return "R, KT and S must be positive";
  if ((long long)R * K > 256) return "R * KT > 256 (vhem_estep_fused_trials)";
  if (S > 16) return "S > 16 (vhem_estep_fused_trials)";
  if (base->SB > S) return "Sb > S (vhem_estep_fused_trials)";
  if (base->d < 1 || base->d > vhem::kBodyMaxD) return "d > 16 (the device-side EM math)";
  return nullptr;
}

struct Sizes {
  size_t nA, nPi, nm, nP, nc, nO;  // per trial: logA | logPi | m | P | c | logOmega
  size_t consts, params, slen;
};

Sizes sizes_of(int K, int S, int d, int cov) {
  const size_t KS = (size_t)K * S, dd = cov == VBHEM_COV_FULL ? (size_t)d * d : (size_t)d;
  Sizes z;
  z.nA = KS * S; z.nPi = KS; z.nm = KS * d; z.nP = KS * dd; z.nc = KS; z.nO = (size_t)K;
  z.consts = z.nA + z.nPi + z.nm + z.nP + z.nc + z.nO;
  // omega | prior | A | centres | covars | vcounts
  z.params = (size_t)K + KS + KS * S + KS * d + KS * dd + KS;
  z.slen = vbhem_stats_len(K, S, d, cov);
  return z;
}

// the doubles of the loop's workspace after the E-step's own
size_t ws_doubles(int N, int K, int R, const Sizes &z) {
  return (size_t)R * (2 * z.consts + z.params + 2 * z.slen + 2 * (size_t)N * K) +
         ((size_t)R * sizeof(vhem::TrialCtrl) + 7) / 8 + 2 * (((size_t)R * sizeof(int) + 7) / 8);
}

}  // namespace

extern "C" {

size_t vhem_em_trials_workspace_bytes(const vbhem_base_t *base, int KT, int S, int R, int T) {
  if (!base || trials_unsupported(base, KT, S, R)) return 0;
  vbhem_cluster_t c = {R * KT, S, nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t fused = vhem_fused_trials_workspace_bytes(base, &c, R, T);
  if (fused == 0) return 0;
  const Sizes z = sizes_of(KT, S, base->d, base->covmode);
  return (fused + 255) / 256 * 256 + ws_doubles(base->N, KT, R, z) * sizeof(double) + 256;
}

int vhem_em_run_trials(const vbhem_base_t *base, const double *Ni_dev, const double *omegaB_dev,
                       int R, int T, const vhem_em_opt_t *opt, vhem_mix_trials_t *mix,
                       double *LogLs, int *num_iter, double *LogL, int *fallback,
                       int *fallback_iter, double *stats_out, double *Z_dev, double *LL_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream) {
  const char *fn = "vhem_em_run_trials";
  const std::string who = std::string(fn) + ": ";
  if (!base || !Ni_dev || !omegaB_dev || !opt || !mix || !mix->omega || !mix->prior || !mix->A ||
      !mix->centres || !mix->covars || !mix->emit_vcounts || !LogLs || !num_iter || !LogL ||
      !fallback || !fallback_iter || !stats_out || !Z_dev || !LL_dev || R < 1)
    return vbhem::set_error(VBHEM_ERR_ARG, who + "null or invalid argument");
  const int K = mix->K, S = mix->S, d = mix->d, cov = mix->covmode;
  if (d != base->d || cov != base->covmode)
    return vbhem::set_error(VBHEM_ERR_ARG, who + "d / covmode differ from the base set's");
  if (!(opt->inf_norm > 0) || !(opt->smooth > 0) || opt->tau < 1 || !(opt->reg_cov >= 0))
    return vbhem::set_error(VBHEM_ERR_ARG, who + "inf_norm, smooth, tau or reg_cov out of range");
  if (const char *why = trials_unsupported(base, K, S, R))
    return vbhem::set_error(VBHEM_ERR_UNSUPPORTED, who + why);
  if (opt->max_iter < 0 || opt->max_iter > (1 << 24))
    return vbhem::set_error(VBHEM_ERR_UNSUPPORTED, who + "max_iter < 0 (or above 2^24)");
  if (opt->min_iter < 0 || opt->min_iter > opt->max_iter + 1)
    return vbhem::set_error(VBHEM_ERR_UNSUPPORTED,
                            who + "min_iter outside [0, max_iter + 1]: more than max_iter + 2 E-steps");
  const size_t need = vhem_em_trials_workspace_bytes(base, K, S, R, T);
  if (need == 0)
    return vbhem::set_error(VBHEM_ERR_UNSUPPORTED, who + "no batched E-step for this shape");
  if (!workspace_dev || workspace_bytes < need) return VBHEM_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = base->N, RK = R * K;
  const size_t KS = (size_t)K * S, dd = cov == VBHEM_COV_FULL ? (size_t)d * d : (size_t)d;
  const Sizes z = sizes_of(K, S, d, cov);
  vbhem_cluster_t c0 = {RK, S, nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t fused = (vhem_fused_trials_workspace_bytes(base, &c0, R, T) + 255) / 256 * 256;
  double *p = reinterpret_cast<double *>(static_cast<char *>(workspace_dev) + fused);
  double *dc = p; p += (size_t)R * z.consts;
  double *dbackup = p; p += (size_t)R * z.consts;
  double *dpar = p; p += (size_t)R * z.params;
  double *dstats = p; p += (size_t)R * z.slen;
  double *dstats_out = p; p += (size_t)R * z.slen;
  double *dhz = p; p += (size_t)N * RK;
  double *dll = p; p += (size_t)N * RK;
  vhem::TrialCtrl *dctrl = reinterpret_cast<vhem::TrialCtrl *>(p);
  p += ((size_t)R * sizeof(vhem::TrialCtrl) + 7) / 8;
  int *dticket = reinterpret_cast<int *>(p);
  p += ((size_t)R * sizeof(int) + 7) / 8;
  int *dflags = reinterpret_cast<int *>(p);
  // the constants, array by array, each trial-major (what the batched E-step reads)
  double *dlogA = dc, *dlogPi = dlogA + R * z.nA, *dcm = dlogPi + R * z.nPi, *dP = dcm + R * z.nm;
  double *dcc = dP + R * z.nP, *dlogOmega = dcc + R * z.nc;
  vbhem_cluster_t cl = {RK, S, dlogA, dlogPi, dcm, dP, dcc};
  // the parameters, likewise: omega | prior | A | centres | covars | vcounts
  const size_t pn[6] = {(size_t)K, KS, KS * S, KS * d, KS * dd, KS};
  double *dparq[6];
  {
    double *q = dpar;
    for (int x = 0; x < 6; ++x) {
      dparq[x] = q;
      q += (size_t)R * pn[x];
    }
  }
  double *hpar[6] = {mix->omega, mix->prior, mix->A, mix->centres, mix->covars, mix->emit_vcounts};

  const int ldL = vhem::trial_ctrl_slots(opt->max_iter);
  vhem::EmTrialsArgs t{};
  vhem::KsArgs &a = t.a;
  a.K = K; a.S = S; a.d = d; a.covmode = cov; a.NU = (int)vbhem_stats_nu(d, cov);
  a.Kb = N; a.tau = opt->tau; a.reg_cov = opt->reg_cov;
  a.stats = dstats;
  a.omega = dparq[0]; a.prior = dparq[1]; a.A = dparq[2]; a.centres = dparq[3];
  a.covars = dparq[4]; a.vcounts = dparq[5];
  a.logA = dlogA; a.logPi = dlogPi; a.cm = dcm; a.P = dP; a.c = dcc; a.logOmega = dlogOmega;
  t.R = R; t.N = N; t.stats_len = z.slen; t.ctrl = dctrl; t.ticket = dticket; t.flags = dflags;
  t.ldL = ldL; t.max_iter = opt->max_iter; t.min_iter = opt->min_iter; t.termvalue = opt->termvalue;
  t.backup = dbackup; t.hz = dhz; t.ll = dll; t.hz_out = Z_dev; t.ll_out = LL_dev;
  t.stats_out = dstats_out;

  std::vector<vhem::TrialCtrl> ctrl((size_t)R);
  for (int r = 0; r < R; ++r) vhem::trial_ctrl_init(&ctrl[(size_t)r]);
  // mapped host memory: flag[2] | active[2] | (64 bytes in) LogLs [R][max_iter + 2]
  vbhem::EmMappedBuf mb;
  const size_t nL = (size_t)R * ldL;
  hipError_t e = vbhem::em_acquire_mapped_buf(64 + nL * sizeof(double), mb);
  int *flag_h = reinterpret_cast<int *>(mb.h), *act_h = flag_h ? flag_h + 2 : nullptr;
  double *L_h = mb.h ? reinterpret_cast<double *>(mb.h + 64) : nullptr;
  if (e == hipSuccess) {
    flag_h[0] = flag_h[1] = 0;
    act_h[0] = act_h[1] = 0;
    std::fill(L_h, L_h + nL, 0.0);
    t.flag = reinterpret_cast<int *>(mb.d);
    t.active = t.flag + 2;
    t.LogLs = reinterpret_cast<double *>(mb.d + 64);
  }
  for (int x = 0; x < 5 && e == hipSuccess; ++x)  // the initial mixtures; vcounts: zeros
    e = hipMemcpyAsync(dparq[x], hpar[x], (size_t)R * pn[x] * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(dparq[5], 0, (size_t)R * pn[5] * sizeof(double), st);
  if (e == hipSuccess) e = hipMemsetAsync(dstats_out, 0, (size_t)R * z.slen * sizeof(double), st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(dctrl, ctrl.data(), ctrl.size() * sizeof(vhem::TrialCtrl), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(dticket, 0, (size_t)R * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(dflags, 0, (size_t)R * sizeof(int), st);
  if (e == hipSuccess) e = vhem::launch_em_trials(t, -1, st);
  if (e == hipSuccess) e = vhem::launch_trials_latch(t, -1, st);
  int rc = VBHEM_OK;
  // iteration j: the E-step of all R K clusters, every running trial's decision, M-step
  // and constants, the latch and the word
  auto enqueue = [&](int j) -> bool {
    rc = vhem_estep_fused_trials(base, &cl, R, T, opt->smooth, Ni_dev, omegaB_dev, opt->inf_norm,
                                 dlogOmega, dstats, dhz, dll, workspace_dev, fused, st);
    if (rc != VBHEM_OK) return false;
    e = vhem::launch_em_trials(t, j, st);
    if (e == hipSuccess) e = vhem::launch_trials_latch(t, j, st);
    return e == hipSuccess;
  };
  const int last_j = opt->max_iter + 1;  // E-step number max_iter + 1 stops every trial
  bool ok = e == hipSuccess && enqueue(0);
  bool finished = false;
  for (int j = 0; ok; ++j) {
    // the next iteration is queued before this one's word is read; it changes nothing
    // of a trial that this one stopped.  Never more than max_iter + 2 in all.
    if (j + 1 <= last_j && !enqueue(j + 1)) break;
    e = vbhem::em_wait_flag(flag_h + (j & 1), j + 1, st);
    if (e != hipSuccess) break;
    if (__atomic_load_n(act_h + (j & 1), __ATOMIC_ACQUIRE) == 0) {
      finished = true;
      break;
    }
    if (j == last_j) break;  // not reached: every trial is done by then
  }
  hipError_t e2 = hipStreamSynchronize(st);  // the iteration queued ahead drains
  if (e == hipSuccess) e = e2;
  for (int x = 0; x < 6 && e == hipSuccess && rc == VBHEM_OK; ++x)
    e = hipMemcpyAsync(hpar[x], dparq[x], (size_t)R * pn[x] * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == VBHEM_OK)
    e = hipMemcpyAsync(ctrl.data(), dctrl, ctrl.size() * sizeof(vhem::TrialCtrl), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == VBHEM_OK)
    e = hipMemcpyAsync(stats_out, dstats_out, (size_t)R * z.slen * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == VBHEM_OK) e = hipStreamSynchronize(st);
  if (e == hipSuccess && rc == VBHEM_OK) std::copy(L_h, L_h + nL, LogLs);
  if (e == hipSuccess) vbhem::em_release_mapped_buf(mb);  // a failed stream may still write it: not reused
  if (rc != VBHEM_OK) return rc;
  if (e != hipSuccess) return vbhem::hip_fail(e, fn);
  if (!finished)
    return vbhem::set_error(VBHEM_ERR_HIP, who + "trials still running after max_iter + 2 iterations");
  for (int r = 0; r < R; ++r) {
    const vhem::TrialCtrl &c = ctrl[(size_t)r];
    num_iter[r] = c.num_iter;
    LogL[r] = c.LogL;
    fallback[r] = c.fallback;
    fallback_iter[r] = c.fb_iter;
  }
  return VBHEM_OK;
}

}  // extern "C"
