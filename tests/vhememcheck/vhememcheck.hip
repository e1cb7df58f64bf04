// tests/vhememcheck/vhememcheck.hip -- TEST-ONLY exports of the host builds of the VHEM EM
// loop's shared functions: the stopping rule of one trial (csrc/vhem_em_trial_ctrl.h) and
// the M-step + E-step constants of one (cluster, state) (csrc/vhem_em_iter_body.h, run
// here over every (k, s) of one trial with the host's one-lane wave), so
// tests/test_vhem_em_trials_ctrl.py and tests/test_vhem_em_body.py check them on a
// machine without a GPU.
#include <hip/hip_runtime.h>

#include "vhem_em_iter_body.h"
#include "vhem_em_trial_ctrl.h"

extern "C" {

int vhem_trial_ctrl_size() { return (int)sizeof(vhem::TrialCtrl); }
void vhem_trial_ctrl_init(vhem::TrialCtrl *c) { vhem::trial_ctrl_init(c); }
int vhem_trial_ctrl_slots(int max_iter) { return vhem::trial_ctrl_slots(max_iter); }
int vhem_trial_ctrl_ends(const vhem::TrialCtrl *c, double new_LL, int max_iter, int min_iter,
                         double termvalue) {
  return vhem::trial_ctrl_ends(c, new_LL, max_iter, min_iter, termvalue) ? 1 : 0;
}
int vhem_trial_ctrl_decide(const vhem::TrialCtrl *c, double new_LL, int max_iter, int min_iter,
                           double termvalue) {
  return vhem::trial_ctrl_decide(c, new_LL, max_iter, min_iter, termvalue);
}
int vhem_trial_ctrl_record(vhem::TrialCtrl *c, int what, double new_LL, int j) {
  return vhem::trial_ctrl_record(c, what, new_LL, j);
}

// One trial's M-step and constants from its packed statistics (stats == nullptr: the
// constants of the given parameters).  Returns the trial's fallback flag (the OR over
// its (k, s)), or -1 for a shape outside the body's limits.
int vhememcheck_body(int K, int S, int d, int covmode, int Kb, int tau, double reg_cov,
                     const double *stats, double *omega, double *prior, double *A, double *centres,
                     double *covars, double *vcounts, double *logA, double *logPi, double *cm,
                     double *P, double *c, double *logOmega) {
  if (K < 1 || S < 1 || S > vhem::kBodyMaxD || d < 1 || d > vhem::kBodyMaxD) return -1;
  vhem::KsArgs a{};
  a.K = K; a.S = S; a.d = d; a.covmode = covmode;
  a.NU = covmode == 1 ? 1 + d + d * (d + 1) / 2 : 1 + 2 * d;
  a.Kb = Kb; a.tau = tau; a.reg_cov = reg_cov; a.stats = stats;
  a.omega = omega; a.prior = prior; a.A = A; a.centres = centres; a.covars = covars;
  a.vcounts = vcounts;
  a.logA = logA; a.logPi = logPi; a.cm = cm; a.P = P; a.c = c; a.logOmega = logOmega;
  double g[2 * vhem::kBodyMaxD * vhem::kBodyMaxD];
  int flag = 0;
  const vhem::HostWave w;
  for (int ks = 0; ks < K * S; ++ks) flag |= vhem::vhem_ks_body(a, ks, w, g);
  return flag;
}

}  // extern "C"
