/*
 * vbhmm_score.h -- C-ABI for scoring observation sequences under point HMMs on
 * MI355X: the computations of the reference's
 *     src/hmm/vbhmm_ll.m:40-116         (scaled forward log-likelihood)
 *     src/hmm/vbhmm_map_state.m:28-103  (scaled Viterbi path)
 * for every (HMM, sequence) pair of H HMMs x N sequences in one launch, fp64,
 * one lane per pair.
 *
 * A set of H HMMs is given as plain padded device arrays (the layouts a packed
 * base set keeps on the device):
 *   nstates [H] (int, 1 <= nstates[h] <= KM), prior [H][KM], trans [H][KM][KM]
 *   (trans[h][i][j] = p(j | i)), mean [H][KM][dim], cov [H][KM][dim][dim]
 *   (VBHEM_COV_FULL; the upper triangle is read) or [H][KM][dim] (VBHEM_COV_DIAG).
 * States k >= nstates[h] are padding: their entries are never used, whatever
 * they hold.  Limits: 1 <= KM <= 16, 1 <= dim <= 8 (else VBHEM_ERR_UNSUPPORTED).
 *
 * vbhmm_score_prepare turns the set into a resident prepared buffer (per state
 * the Cholesky factor's packed inverse and the log-normaliser of MATLAB's
 * mvnpdf); the scoring calls read only that buffer and the sizes H, KM, dim,
 * covmode of the descriptor.  Sequences are a vbhmm_seqs_t (include/vbhmm_fb.h).
 * Status codes and vbhem_last_error() as include/vbhem_estep.h.  Only
 * vbhmm_score_prepare synchronises the stream (to read the positive-definite flag).
 */
#ifndef VBHMM_SCORE_H
#define VBHMM_SCORE_H

#include <stddef.h>

#include "vbhem_estep.h"
#include "vbhmm_fb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int H, KM, dim, covmode;
  const int *nstates;
  const double *prior, *trans, *mean, *cov;
} vbhmm_score_hmms_t;

/* Bytes of the prepared buffer (0: invalid or unsupported sizes). */
size_t vbhmm_score_prepared_bytes(const vbhmm_score_hmms_t *hmms);
/* Builds the prepared buffer from the device arrays of `hmms`.  A covariance that
 * is not positive definite: VBHEM_ERR_ARG, vbhem_last_error() names the first
 * (HMM, state), as MATLAB's mvnpdf errors.  Synchronises `stream`. */
int vbhmm_score_prepare(const vbhmm_score_hmms_t *hmms_dev, void *prepared_dev,
                        size_t prepared_bytes, void *stream);
/* Viterbi back-pointer workspace for sequences of total_steps observations in all. */
size_t vbhmm_score_workspace_bytes(const vbhmm_score_hmms_t *hmms, long long total_steps);
/* loglik [H][N] = sum_t log c_t (not normalised by the length; 0 for an empty
 * sequence).  Emission densities that are exactly 0 are set to 10 * 2^-1074
 * (vbhmm_ll.m:70-72). */
int vbhmm_score_ll(const vbhmm_score_hmms_t *hmms, const void *prepared_dev,
                   const vbhmm_seqs_t *seqs_dev, double *loglik_dev, void *stream);
/* path [H][total_steps] (int, 0-based states; sequence n of HMM h at
 * path[h * total_steps + offsets[n] + t]), loglik [H][N] = -sum_t log(1 / z_t) of
 * the scaled recursion.  total_steps >= offsets[N].  No zero floor. */
int vbhmm_score_viterbi(const vbhmm_score_hmms_t *hmms, const void *prepared_dev,
                        const vbhmm_seqs_t *seqs_dev, long long total_steps, int *path_dev,
                        double *loglik_dev, void *workspace_dev, size_t workspace_bytes,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_SCORE_H */
