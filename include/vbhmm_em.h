/*
 * vbhmm_em.h -- C-ABI of the fused, batched VB-HMM EM on MI355X: the whole EM of
 * src/hmm/vbhmm_em.m:112-414 (usegroups = 0; fix_clusters, fix_cov unset) for a list of
 * independent RUNS in one call.  A run is one (subject, K, initial posterior); one
 * wavefront owns a run from its first prelude to its last M-step, so no iteration leaves
 * the device and the per-iteration [K][N][maxT] arrays of vbhmm_fb are never written.
 *
 * Layouts (row-major, DEVICE pointers; status codes and stream of vbhem_estep.h):
 *   subjects: every subject's sequences in one vbhmm_seqs_t (include/vbhmm_fb.h) plus
 *             seq_first[S+1]: subject s owns sequences seq_first[s] .. seq_first[s+1]-1.
 *             max_seqs / max_obs: the largest sequence / observation count of one subject
 *             (they size the workspace; a subject beyond them fails its runs, see status).
 *   runs:     subject[R], K[R] (1 <= K <= KM), post[R][PL]: the packed posterior of a run,
 *             PL = vbhmm_em_post_len(KM, dim):
 *               [alpha KM | epsilon KM x KM | beta KM | v KM | m KM x dim | W KM x dim x dim]
 *             with states and epsilon rows padded to KM (padding is never read).
 *             KM is 4 or 8.
 *   hyper:    one set per call; W0inv_diag is the diagonal of W0^-1 (W0mode iid and diag).
 *   outputs:  post_out[R][PL]    posterior after the last M-step (an unstable run: the
 *                                posterior of its last E-step, no M-step)
 *             post_estep[R][PL]  posterior at the last E-step (NULL: not kept)
 *             stats[R][SL]       the last E-step's statistics, SL = vbhmm_em_stats_len:
 *               [Nk1 KM | Nk KM | M KM x KM | xbar KM x dim | t1_S KM x dim x dim] (NULL ok)
 *             LL[R], iters[R], status[R]
 *             LLs[R][max_iter]   the bound trajectory (NULL: not kept); entries past
 *                                iters[r] are not written
 * Limits: K <= 8 and dim <= 8; larger: VBHEM_ERR_UNSUPPORTED.
 *
 * The call splits R into launches of opt->chunk_runs runs (0: the library's default,
 * VBHMM_EM_DEFAULT_CHUNK runs or as many as fit VBHMM_EM_DEFAULT_WORKSPACE); a run's
 * result does not depend on the chunking, on its position in the list or on the other
 * runs.
 */
#ifndef VBHMM_EM_H
#define VBHMM_EM_H

#include <stddef.h>

#include "vbhem_estep.h"
#include "vbhmm_fb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBHMM_EM_CONVERGED 0 /* relative change of the bound <= min_diff             */
#define VBHMM_EM_MAX_ITER 1  /* stopped at max_iter                                  */
#define VBHMM_EM_UNSTABLE 2  /* NaN bound: LL = -inf, no further M-step               */
#define VBHMM_EM_BAD_RUN 3   /* subject / K out of range or beyond max_seqs / max_obs */

#define VBHMM_EM_DEFAULT_CHUNK 16384
#define VBHMM_EM_DEFAULT_WORKSPACE (2ull << 30) /* the default chunk shrinks to stay below */

typedef struct {
  vbhmm_seqs_t seqs;    /* all subjects' sequences, packed */
  int S;                /* subjects */
  const int *seq_first; /* [S+1] */
  int max_seqs, max_obs;
} vbhmm_em_subjects_t;

typedef struct {
  int R, KM;
  const int *subject;  /* [R] */
  const int *K;        /* [R] */
  const double *post;  /* [R][PL] */
} vbhmm_em_runs_t;

typedef struct {
  double alpha0, epsilon0, beta0, v0;
  double m0[8];
  double W0inv_diag[8];
} vbhmm_em_hyper_t;

typedef struct {
  int max_iter;
  double min_diff;
  int chunk_runs; /* runs per launch; 0 = the default */
} vbhmm_em_opt_t;

size_t vbhmm_em_post_len(int KM, int dim);
size_t vbhmm_em_stats_len(int KM, int dim);

/* Workspace of a call with up to R runs (0 on invalid / unsupported sizes). */
size_t vbhmm_em_batch_workspace_bytes(const vbhmm_em_subjects_t *subjects, int R, int KM, int chunk_runs);

int vbhmm_em_batch(const vbhmm_em_subjects_t *subjects, const vbhmm_em_runs_t *runs,
                   const vbhmm_em_hyper_t *hyper, const vbhmm_em_opt_t *opt, double *post_out_dev,
                   double *post_estep_dev, double *stats_dev, double *LL_dev, int *iters_dev, int *status_dev,
                   double *LLs_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* gamma of the E-step at each run's posterior (phase A alone, no M-step) into the packed
 * gamma_dev[sum of the runs' observation counts][KM]: run r writes rows gamma_row_dev[r]
 * .. gamma_row_dev[r] + (its subject's observation count) - 1, row p = observation p of
 * the subject, columns k < K (the caller lays the rows out; columns past K are not
 * written).  status_dev[r] (or NULL): VBHMM_EM_CONVERGED, or VBHMM_EM_BAD_RUN with nothing
 * written.  Workspace: vbhmm_em_batch_workspace_bytes. */
int vbhmm_em_gamma(const vbhmm_em_subjects_t *subjects, const vbhmm_em_runs_t *runs, double *gamma_dev,
                   const long long *gamma_row_dev, int *status_dev, int chunk_runs, void *workspace_dev,
                   size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_EM_H */
