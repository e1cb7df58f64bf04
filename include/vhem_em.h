/*
 * vhem_em.h -- the VHEM EM loop of a chunk of trials (hem_h3m_c_step.m, as
 * vhem.hem_h3m_c_trials runs it) kept on the device: per iteration one
 * vhem_estep_fused_trials launch over the R * KT clusters, one kernel with the stopping
 * rule, the M-step (hem_mstep_component.m:123-166) and the next E-step constants of
 * every trial, and one that keeps what the stopping trials leave
 * (csrc/vhem_em_trials.hip).  The host waits for one word per iteration.
 *
 * The rule (csrc/vhem_em_trial_ctrl.h) is hem_h3m_c_step.m's, not the VBHEM one:
 * change = (new_LL - old_LL) / |old_LL| signed, stop = change < termvalue ||
 * num_iter > max_iter with num_iter counted before the increment, the trial ends only
 * with num_iter >= min_iter, and at a stop NO M-step is accepted: the trial keeps the
 * parameters that produced its stopping E-step.  A trial runs at most max_iter + 2
 * E-steps; never more than that many iterations are queued.
 *
 * The degenerate fixes (hem_fix_degenerate_component / _hmm) draw random numbers and
 * stay on the host.  A trial whose M-step gives an omega == 0 or an emit_vcounts == 0
 * (the host's tests), a constant that is not finite (a logA / logPi of -inf is), or a
 * LogL that is not finite, is frozen on the device and FLAGGED: fallback[r] = 1 and
 * fallback_iter[r] = the iteration (-1: the initial mixture's constants).  Its other
 * outputs are then unspecified; the caller reruns it with the host engine from its
 * initial mixture.  The device never draws a random number.
 *
 * All arrays are HOST arrays, row-major, unless named *_dev.  Status codes as in
 * vbhem_estep.h.
 */
#ifndef VHEM_EM_H
#define VHEM_EM_H

#include <stddef.h>

#include "vbhem_estep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* R reduced mixtures of KT clusters and S states, trial-major. */
typedef struct {
  int K, S, d, covmode; /* K = KT, the clusters of ONE trial                        */
  double *omega;        /* [R][K]                                                   */
  double *prior;        /* [R][K][S]                                                */
  double *A;            /* [R][K][S][S]                                             */
  double *centres;      /* [R][K][S][d]                                             */
  double *covars;       /* [R][K][S][d][d] (full) | [R][K][S][d] (diag)             */
  double *emit_vcounts; /* [R][K][S], output only (hem_mstep_component.m:138)       */
} vhem_mix_trials_t;

typedef struct {
  double inf_norm;  /* hem_h3m_c_step.m:110-119                                    */
  double smooth;    /* E /= smooth                                                 */
  double reg_cov;   /* added to every new covariance (diagonal)                    */
  double termvalue; /* the change below which a trial stops (strict)               */
  int tau;          /* virtual sample length; tau == 1 substitutes A               */
  int max_iter;     /* >= 0                                                        */
  int min_iter;     /* 0 <= min_iter <= max_iter + 1                               */
} vhem_em_opt_t;

/* Shapes: those of vhem_estep_fused_trials (S <= 16, Sb <= S, R * KT <= 256) with
 * d <= 16.  vhem_em_trials_workspace_bytes returns 0 for any other, and
 * vhem_em_run_trials VBHEM_ERR_UNSUPPORTED (vbhem_last_error names the limit).
 *
 * mix: in, the R initial mixtures WITH reg_cov already added to the covariances
 * (hem_h3m_c_step.m:98-108); out, per trial the parameters that produced its stopping
 * E-step and their emit_vcounts.  Ni_dev [N] = Nv * omega_b * Kb, omegaB_dev [N]
 * (device).  LogLs [R][max_iter + 2]: every E-step's log-likelihood (the slots a trial
 * did not reach are 0); num_iter, LogL, fallback, fallback_iter [R].  stats_out
 * [R][vbhem_stats_len(KT, ...)]: the packed statistics of each trial's stopping E-step.
 * Z_dev / LL_dev [N][R * KT] (device): trial r's columns [r KT, (r + 1) KT) hold Z and
 * the undivided L_elbo of ITS stopping E-step. */
size_t vhem_em_trials_workspace_bytes(const vbhem_base_t *base, int KT, int S, int R, int T);
int vhem_em_run_trials(const vbhem_base_t *base, const double *Ni_dev, const double *omegaB_dev,
                       int R, int T, const vhem_em_opt_t *opt, vhem_mix_trials_t *mix,
                       double *LogLs, int *num_iter, double *LogL, int *fallback,
                       int *fallback_iter, double *stats_out, double *Z_dev, double *LL_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VHEM_EM_H */
