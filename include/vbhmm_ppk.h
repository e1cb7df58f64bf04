/*
 * vbhmm_ppk.h -- C-ABI for the probability product kernel (PPK) between point
 * HMMs on MI355X: the Gram matrix of the reference's PPK spectral clustering,
 *     src/compare_mtds/ppk/ppk_sc.m:17-22  (the N x N double loop)
 *     src/compare_mtds/ppk/elkernel.m      (the kernel of two HMMs)
 *     src/compare_mtds/ppk/bhatt.m         (the affinity of two Gaussians)
 * for every pair of two HMM sets in one launch, fp64.
 *
 * For HMM a (M states, prior p, trans A) and HMM b (N states, prior r, trans B):
 *   C = cov + pad on every entry, then C += 1e-5 trace(C) I (a vector cov is a
 *   diagonal matrix first);
 *   pot[i][j] = 2^(d/2) det(C1)^(1/4) det(C2)^(1/4) det(C1 + C2)^(-1/2)
 *               exp(-(mu1 - mu2)' (C1 + C2)^-1 (mu1 - mu2) / 4);
 *   T == 1: K = p' pot r (no rho);  otherwise sep = (A^rho)' ((p r')^rho o pot) (B^rho),
 *   T - 1 times sep = (A^rho)' (sep o pot) (B^rho), K = sum(sep o pot).
 * ^rho is elementwise with 0^rho = 0.  No log domain: far-apart HMMs give tiny
 * values or 0; values are not bounded by 1.
 *
 * HMM sets are vbhmm_score_hmms_t (include/vbhmm_score.h: padded device arrays,
 * states k >= nstates[h] never read).  Limits: KM <= 16, dim <= 8 (else
 * VBHEM_ERR_UNSUPPORTED).  Status codes and vbhem_last_error() as
 * include/vbhem_estep.h.  Only vbhmm_ppk_prepare synchronises the stream (to read
 * the positive-definite flag).
 */
#ifndef VBHMM_PPK_H
#define VBHMM_PPK_H

#include <stddef.h>

#include "vbhmm_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBHMM_PPK_RECT 0 /* out [Ha][Hb]                                         */
#define VBHMM_PPK_SYM 1  /* a and b are one set: out [H][H], bitwise symmetric    */
#define VBHMM_PPK_DIAG 2 /* Ha == Hb: out [H], the (i, i) pairs only              */

/* Bytes of the prepared buffer (0: invalid or unsupported sizes). */
size_t vbhmm_ppk_prepared_bytes(const vbhmm_score_hmms_t *hmms);
/* Builds the prepared buffer (per HMM: state count, prior, prior^rho, trans^rho,
 * means, packed regularised covariances, 1/4 logdet).  rho <= 0 or pad < 0:
 * VBHEM_ERR_ARG.  A regularised covariance that is not positive definite:
 * VBHEM_ERR_ARG, vbhem_last_error() names the first (HMM, state).  Synchronises
 * `stream`. */
int vbhmm_ppk_prepare(const vbhmm_score_hmms_t *hmms_dev, double rho, double pad, void *prepared_dev,
                      size_t prepared_bytes, void *stream);
/* The Gram matrix of the sets a and b (prepared with the same rho and pad) in
 * `mode`.  VBHMM_PPK_SYM computes the pairs i <= j only and stores each value to
 * out[i][j] and out[j][i]; it and VBHMM_PPK_DIAG need Ha == Hb (SYM: the same
 * prepared buffer).  T < 1 or different dimensions: VBHEM_ERR_ARG. */
int vbhmm_ppk_gram(const vbhmm_score_hmms_t *hmms_a, const void *prepared_a,
                   const vbhmm_score_hmms_t *hmms_b, const void *prepared_b, int T, int mode,
                   double *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_PPK_H */
