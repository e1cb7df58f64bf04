// vhem_em_trial_ctrl.h -- the stopping rule of one VHEM EM trial, one function for the
// host and the device (vhem_em_trials.hip: every wave of a trial takes the decision, the
// trial's last wave records it; the check library tests/vhememcheck and the stand-alone
// walker call it on the host).
//
// It restates the decision lines of vhem.hem_h3m_c_trials (hem_h3m_c_step.m) in plain
// fp64 and in the same expression order.  It is NOT the VBHEM rule of
// vbhem_em_trial_ctrl.h:
//   * change = (new_LL - old_LL) / |old_LL| is signed, +inf while num_iter <= 1, and
//     old_LL starts at -inf;
//   * stop = change < termvalue || num_iter > max_iter, with num_iter the count BEFORE
//     the increment: a falling likelihood stops, a NaN one never passes the change test;
//   * the trial ends only if stop && num_iter >= min_iter;
//   * at a stop no M-step is accepted: the trial keeps the parameters that produced the
//     stopping E-step and LogL = new_LL.
// So a trial runs at most max_iter + 2 E-steps (given min_iter <= max_iter + 1), E-step
// number e has num_iter == e, and LogLs needs max_iter + 2 slots.  Internal.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VHEM_CTRL_HD __host__ __device__
#else
#define VHEM_CTRL_HD
#endif

namespace vhem {

struct TrialCtrl {
  int num_iter;   // M-steps accepted so far = the number of the next E-step
  int done;       // stopped or frozen: nothing of the trial changes any more
  int fallback;   // frozen for the host engine (degenerate or non-finite), not stopped
  int stop_iter;  // the loop iteration at which the trial stopped (-1 while running)
  int fb_iter;    // the loop iteration at which the fallback was raised (-1: none)
  int pad_;
  double LogL;    // the last E-step's log-likelihood (-inf before the first)
};

enum { kTrialContinue = 0, kTrialStop = 1, kTrialFallback = 2 };

VHEM_CTRL_HD inline void trial_ctrl_init(TrialCtrl *c) {
  c->num_iter = 0;
  c->done = 0;
  c->fallback = 0;
  c->stop_iter = -1;
  c->fb_iter = -1;
  c->pad_ = 0;
  c->LogL = -INFINITY;
}

// The number of LogLs slots of one trial.
VHEM_CTRL_HD inline int trial_ctrl_slots(int max_iter) { return max_iter + 2; }

// The rule as vhem.hem_h3m_c_trials has it: true when the trial ends at the E-step whose
// log-likelihood is new_LL.  It depends on the record and new_LL alone, both known before
// the M-step, and changes nothing.
VHEM_CTRL_HD inline bool trial_ctrl_ends(const TrialCtrl *c, double new_LL, int max_iter,
                                         int min_iter, double termvalue) {
  const double old_LL = c->LogL;
  const double change = c->num_iter > 1 ? (new_LL - old_LL) / fabs(old_LL) : (double)INFINITY;
  const bool stop = change < termvalue || c->num_iter > max_iter;
  return stop && c->num_iter >= min_iter;
}

// What the device loop does with that E-step.  A non-finite new_LL is a fallback whatever
// the rule says (the host engine reruns the trial), so nothing downstream of it is ever
// computed on the device.
VHEM_CTRL_HD inline int trial_ctrl_decide(const TrialCtrl *c, double new_LL, int max_iter,
                                          int min_iter, double termvalue) {
  if (!(fabs(new_LL) <= 1.79769313486231570815e308)) return kTrialFallback;  // NaN, +-inf
  return trial_ctrl_ends(c, new_LL, max_iter, min_iter, termvalue) ? kTrialStop : kTrialContinue;
}

// Record iteration j's outcome: `what` from trial_ctrl_decide, or kTrialFallback raised
// by the M-step of a continuing trial.  Returns the LogLs slot that takes new_LL (the
// caller stores it when the slot is below trial_ctrl_slots).  Not to be called on a done
// trial.
VHEM_CTRL_HD inline int trial_ctrl_record(TrialCtrl *c, int what, double new_LL, int j) {
  const int slot = c->num_iter;
  c->LogL = new_LL;
  if (what == kTrialStop) {
    c->done = 1;
    c->stop_iter = j;
  } else if (what == kTrialFallback) {
    c->done = 1;
    c->fallback = 1;
    c->fb_iter = j;
  } else {
    c->num_iter = slot + 1;
  }
  return slot;
}

}  // namespace vhem
