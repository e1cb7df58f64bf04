/*
 * vbhmm_gmm.h -- C-ABI of the batched random-start GMM fit on MI355X: the starting GMMs
 * of VB-HMM learning's random trials (src/hmm/vbhmm_init.m:59-60, gmdistribution.fit with
 * 'Start' 'randSample', as vbhmm_em.py gmm_fit_randsample restates it) for a list of
 * independent FITS in one call, and optionally the initial variational posterior of each
 * fitted GMM (vbhmm_init.m:122-204), ready to be the `post` of vbhmm_em_batch.  A fit is
 * one (subject, K, K start rows, reg); one wavefront owns a fit from its start to its
 * last M-step.
 *
 * Layouts (row-major, DEVICE pointers; status codes and stream of vbhem_estep.h):
 *   subjects: as include/vbhmm_em.h.  The observations of subject s are rows
 *             offsets[seq_first[s]] .. offsets[seq_first[s+1]]-1 of x: N of them.
 *   fits:     subject[R], K[R] (2 <= K <= KM < N), rows[R][KM]: the K start rows of a fit,
 *             indices into its subject's N observations; reg[R]: added to every
 *             covariance's diagonal (0, or 1e-10 for the regularised refit).  KM is 4 or 8.
 *   outputs:  prior[R][KM], mean[R][KM][dim], cov[R][KM][dim][dim]: states k < K
 *             ll[R]             the log-likelihood of the last E-step
 *             iters[R], status[R]
 *             lls[R][max_iter]  the log-likelihood trajectory (NULL: not kept); entries
 *                               past iters[r] are not written (an ill-conditioned fit
 *                               fails at the factorisation that opens iteration iters[r]
 *                               and has iters[r] - 1 entries)
 *             post_init[R][PL]  with hyper (both or neither NULL): the packed initial
 *                               posterior, PL = vbhmm_em_post_len(KM, dim), padded as the
 *                               host packs it
 *             prior, mean, cov and post_init are written only for fits that end
 *             VBHMM_GMM_CONVERGED or VBHMM_GMM_MAX_ITER; a VBHMM_GMM_BAD_FIT writes its
 *             status alone.
 * Limits: K <= 8 and dim <= 8; larger: VBHEM_ERR_UNSUPPORTED.
 *
 * The call splits R into launches of opt->chunk_runs fits (0: the library's default,
 * VBHMM_EM_DEFAULT_CHUNK fits or as many as fit VBHMM_EM_DEFAULT_WORKSPACE); a fit's
 * result does not depend on the chunking, on its position in the list, on KM or on the
 * other fits.
 */
#ifndef VBHMM_GMM_H
#define VBHMM_GMM_H

#include <stddef.h>

#include "vbhmm_em.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBHMM_GMM_CONVERGED 0       /* |ll - last| <= tolfun |ll|                        */
#define VBHMM_GMM_MAX_ITER 1        /* stopped at max_iter                               */
#define VBHMM_GMM_ILL_CONDITIONED 2 /* a Cholesky pivot was not > 0 (NaN included)       */
#define VBHMM_GMM_BAD_FIT 3         /* subject / K / a row out of range, N <= K, K < 2,  */
                                    /* or a subject beyond max_obs                       */

typedef struct {
  int R, KM;
  const int *subject; /* [R] */
  const int *K;       /* [R] */
  const int *rows;    /* [R][KM] */
  const double *reg;  /* [R] */
} vbhmm_gmm_fits_t;

typedef struct {
  int max_iter;
  double tolfun;
  int chunk_runs; /* fits per launch; 0 = the default */
} vbhmm_gmm_opt_t;

/* Workspace of a call with up to R fits (0 on invalid / unsupported sizes). */
size_t vbhmm_gmm_fit_workspace_bytes(const vbhmm_em_subjects_t *subjects, int R, int KM, int chunk_runs);

int vbhmm_gmm_fit_batch(const vbhmm_em_subjects_t *subjects, const vbhmm_gmm_fits_t *fits,
                        const vbhmm_gmm_opt_t *opt, double *prior_dev, double *mean_dev, double *cov_dev,
                        double *ll_dev, int *iters_dev, int *status_dev, double *lls_dev,
                        const vbhmm_em_hyper_t *hyper, double *post_init_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_GMM_H */
