// vbhem_em_dev.h -- the EM loop's per-iteration host math as device kernels
// (vbhem_em_dev.hip), used by vbhem_em_run (vbhem_em.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>

namespace vbhem {

constexpr int kEmDevMaxD = 16;  // register-resident d x d factorisations (padded to 2/4/8/16)

enum { kEmPrelude = 0, kEmIterate = 1 };

struct EmDevArgs {
  int K, S, d, covmode, NU;
  // posterior read (device; mode kEmPrelude / kEmBound)
  const double *alpha, *eta, *eps, *lam, *v, *m, *W;
  // posterior written by the M-step (kEmMstepPrelude; the prelude then reads it)
  double *alpha_o, *eta_o, *eps_o, *lam_o, *v_o, *m_o, *W_o;
  const double *stats;  // packed E-step statistics (device)
  // hyperparameters and their precomputed constants (host side, once per run)
  double alpha0, eta0, epsilon0, lambda0, v0;
  double logCalpha0, logCeta0, logCepsilon0, logB0;
  const double *m0;     // [d]
  const double *W0inv;  // [d][d]
  // prelude outputs: the E-step's cluster constants, and for the bound
  // logLambdaTilde and log det W of every (k, s)
  double *logA, *logPi, *cm, *P, *c, *lLT, *logOmega, *logdetW;
  double *part;  // [K S][13] bound partial sums
  int *ticket;   // 0 between launches (the last wave of a launch resets it)
  int *flag;     // optional (mapped host memory): set to seq after *L_out is written
  int seq;
};

bool em_dev_supported(int d, int S);
// kEmPrelude: prelude of (alpha .. W); kEmIterate: the bound of (alpha .. W) with
// this iteration's prelude outputs and stats, written to *L_out (device or mapped
// host), then the M-step of (stats) into (alpha_o .. W_o) and its prelude.
hipError_t launch_em_dev(const EmDevArgs &a, int mode, double *L_out, hipStream_t st);

// ---- R trials in one launch, stopped on the device (vbhem_em_trials.hip) ----
struct TrialCtrl;  // vbhem_em_trial_ctrl.h

// `a` holds the shapes (K = clusters of ONE trial), the hyperparameters and the
// pointers of trial 0: its posterior buffer 0 in (alpha .. W) -- buffer b of trial r
// lies (b R + r) postn doubles further, the M-step outputs are not used -- and its
// slices of the trial-major arrays, trial r lying r times the slice further: the
// cluster constants logA [R K][S][S], logPi, cm, P, c (what the batched E-step
// reads), logOmega [R K], lLT, logdetW [R K S], part [R][13][K S] and the statistics
// [R][stats_len].  a.ticket, a.flag and a.seq are not used.
struct EmTrialsArgs {
  EmDevArgs a;
  int R, N;           // trials; base HMMs (rows of hat_Z)
  size_t postn;       // doubles of one posterior
  size_t stats_len;   // doubles of one trial's packed statistics
  TrialCtrl *ctrl;    // [R]
  int *ticket;        // [R], 0 between launches
  double *LogLs;      // [R][ldL]: the accepted bounds (device, or mapped host memory)
  int ldL, max_iter;  // ldL >= max_iter + 1
  double minDiff;
  // the latch: a copy of every running trial's E-step constants (logA | logPi | cm |
  // P | c | logOmega, laid out as the live ones), the E-step's outputs and where a
  // stopping trial's columns and statistics are kept
  double *backup;
  const double *hz, *ll;            // [N][R K], overwritten by every E-step
  double *hz_out, *ll_out;          // [N][R K]
  double *stats_out;                // [R][stats_len]
  int *flag, *active;               // [2] each (mapped host memory), slot j % 2
  // the hyperparameters, per trial: trial r's table (vbhem_em_deriv_terms.h: the five
  // scalars, the bound's four constants, m0, W0^-1) lies at hyp + r hyp_stride; the
  // kernels read them from there, a.alpha0 .. a.W0inv are not used
  const double *hyp;
  size_t hyp_stride;
  // the bound's derivatives (launch_trials_derivs): W0 entries, the per-(k, s) terms
  // [R][5 + W0_len + d][K S] and the result [R][5 + W0_len + d] (device)
  int W0_len;
  double *dterms, *dLL;
};

// kEmPrelude: the prelude of every trial's buffer 0.  kEmIterate: for every trial
// not done, the bound of its current posterior, the M-step into its other buffer,
// that one's prelude, and trial_ctrl_step on the bound.
hipError_t launch_em_trials(const EmTrialsArgs &t, int mode, hipStream_t st);
// After iteration j (j = -1 after the prelude: no word): keeps the E-step outputs
// and statistics of every trial that stopped at j, saves the constants of every
// running trial and puts back those of a trial whose bound was NaN, then writes
// active[j % 2] = trials not done and flag[j % 2] = j + 1.
hipError_t launch_trials_latch(const EmTrialsArgs &t, int j, hipStream_t st);
// After the loop (every trial done): the raw derivatives of every stable trial's last
// accepted bound (vbhemh3m_lb.m:202-345), at the posterior before its last M-step
// (buffer cur ^ 1), into dLL.  A trial that is unstable or took no iteration is left
// alone (the caller writes its NaN).  vbhem_em_trials_derivs.hip.
hipError_t launch_trials_derivs(const EmTrialsArgs &t, hipStream_t st);

}  // namespace vbhem
