// vbhem_em_trial_ctrl.h -- the stopping rule of one EM trial, one function for the
// host and the device (vbhem_em_trials.hip's last wave per trial calls it; the
// check library tests/emtrialscheck and the loop's tests call it on the host).
//
// It restates the decision lines of vbhem_h3m_c_step_fc.m:311-374 as the loops in
// vbhem_em.hip (vbhem_em_run_ext) and vbhem_amd/em.py (vbhem_h3m_c_trials) have
// them, in plain fp64 and in the same expression order, so that given the same
// bound the decision is the same.  Internal.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VBHEM_CTRL_HD __host__ __device__
#else
#define VBHEM_CTRL_HD
#endif

namespace vbhem {

struct TrialCtrl {
  int it;         // accepted iterations so far (= M-steps taken)
  int done;       // the trial has stopped: nothing of it changes any more
  int stable;     // 0 once a bound was NaN
  int cur;        // which of the trial's two posterior buffers is current
  int stop_iter;  // the loop iteration at which the trial stopped (-1 while running)
  int pad_;
  double lastL;    // the previous accepted bound (-DBL_MAX before the first)
  double L_final;  // the last bound (-inf when unstable, and before the first)
};

VBHEM_CTRL_HD inline void trial_ctrl_init(TrialCtrl *c) {
  c->it = 0;
  c->done = 0;
  c->stable = 1;
  c->cur = 0;
  c->stop_iter = -1;
  c->pad_ = 0;
  c->lastL = -DBL_MAX;
  c->L_final = -INFINITY;
}

// One iteration's decision from its bound L.  Returns the LogLs slot that takes L
// (the caller stores it), or -1 when the bound is NaN (nothing recorded, no M-step
// accepted).  An accepted M-step flips `cur`.  Not to be called on a done trial.
VBHEM_CTRL_HD inline int trial_ctrl_step(TrialCtrl *c, double L, int max_iter, double minDiff) {
  const int it = c->it;
  if (L != L) {  // step_fc.m:338-374: unstable model, stop before the M-step
    c->L_final = -INFINITY;
    c->stable = 0;
    c->done = 1;
    c->stop_iter = it;
    return -1;
  }
  bool do_break = false;
  if (it > 1 && fabs((L - c->lastL) / c->lastL) <= minDiff) do_break = true;
  if (it == max_iter) do_break = true;
  c->cur ^= 1;
  c->it = it + 1;
  c->lastL = L;
  c->L_final = L;
  if (do_break) {
    c->done = 1;
    c->stop_iter = it;
  }
  return it;
}

}  // namespace vbhem
