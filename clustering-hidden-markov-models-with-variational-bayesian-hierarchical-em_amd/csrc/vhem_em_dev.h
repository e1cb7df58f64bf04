// vhem_em_dev.h -- the VHEM EM loop's per-iteration kernels (vhem_em_trials.hip), used
// by vhem_em_run_trials (vhem_em.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "vhem_em_iter_body.h"

namespace vhem {

struct TrialCtrl;  // vhem_em_trial_ctrl.h

// `a` holds the shapes (K = clusters of ONE trial), the M-step's options and the
// pointers of trial 0 into the trial-major arrays, trial r lying r times its slice
// further: the parameters omega [R][K], prior, vcounts [R][K S], A [R][K S][S], centres
// [R][K S][d], covars [R][K S][dd]; the E-step constants logA [R K][S][S], logPi, cm, P,
// c (what the batched E-step reads) and logOmega [R K]; the statistics [R][stats_len].
struct EmTrialsArgs {
  KsArgs a;
  int R, N;          // trials; base HMMs (rows of Z)
  size_t stats_len;  // doubles of one trial's packed statistics
  TrialCtrl *ctrl;   // [R]
  int *ticket;       // [R], 0 between launches
  int *flags;        // [R], 0 between launches: the waves' fallback flags of one launch
  double *LogLs;     // [R][ldL] (device, or mapped host memory)
  int ldL, max_iter, min_iter;  // ldL >= max_iter + 2
  double termvalue;
  // the latch: a copy of every running trial's E-step constants (logA | logPi | cm | P |
  // c | logOmega, laid out as the live ones), the E-step's outputs and where a stopping
  // trial's columns and statistics are kept
  double *backup;
  const double *hz, *ll;    // [N][R K], overwritten by every E-step
  double *hz_out, *ll_out;  // [N][R K]
  double *stats_out;        // [R][stats_len]
  int *flag, *active;       // [2] each (mapped host memory), slot j % 2
};

// j = -1: the constants of every trial's GIVEN parameters (a trial whose constants are
// not finite is flagged, fb_iter -1).  j >= 0: for every trial not done, the decision on
// iteration j's E-step (vhem_em_trial_ctrl.h) and, if the trial continues, its M-step
// and next constants (vhem_em_iter_body.h).
hipError_t launch_em_trials(const EmTrialsArgs &t, int j, hipStream_t st);
// After that kernel: keeps Z, L_elbo and the statistics of every trial that stopped at
// j, saves the constants of every running trial, gives a trial flagged at j its saved
// constants back (j = -1: neutral finite ones), then (j >= 0) writes active[j % 2] =
// trials not done and flag[j % 2] = j + 1.
hipError_t launch_trials_latch(const EmTrialsArgs &t, int j, hipStream_t st);

}  // namespace vhem
