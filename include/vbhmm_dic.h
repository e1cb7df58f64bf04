/*
 * vbhmm_dic.h -- C-ABI of the DIC likelihood on MI355X: for every model of a K x S
 * grid, the VHEM expected log-likelihood of all N subject HMMs under the model's group
 * HMMs, mixed over the model's clusters and summed over the subjects, as the
 * reference's
 *     src/compare_mtds/dic/myDIC.m:160-170
 * computes it (hem_hmm_bwd_fwd_mex in diag mode at smooth = 1, then logtrick and sum).
 * Backward sweep and termination only; clusters of different sizes in one launch; the
 * mixture log-sum-exp and the sum over subjects are taken where the values are
 * produced, so no [N][clusters] buffer exists unless the caller asks for L_pairs.
 *
 * The base set is a vbhem_base_t (include/vbhem_estep.h) in VBHEM_COV_DIAG; its U is
 * ignored.  All pointers inside the descriptors and every *_dev argument are device
 * pointers.  Status codes and vbhem_last_error() as include/vbhem_estep.h.
 */
#ifndef VBHMM_DIC_H
#define VBHMM_DIC_H

#include <stddef.h>

#include "vbhem_estep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G models of group HMMs: C clusters laid model after model, model g owning clusters
 * model_off[g] .. model_off[g + 1] - 1 (model_off[0] = 0, model_off[G] = C).  Cluster c
 * has nstates_r[c] <= S own states; arrays are padded to S and padding is never read.
 * Per cluster, the constants of vhem_estep_pairs in diag mode:
 *   logA = log(A_r) (-inf = a zero transition), logPi = log(prior_r), m = centres,
 *   P = 1 ./ covars, c = sum(log(covars)).
 * max_model_clusters: the caller's bound on model_off[g + 1] - model_off[g] (the host
 * never reads model_off); a model with more clusters than that, or with none, gets
 * LL = NaN. */
typedef struct {
  int G;                   /* models                                              */
  int C;                   /* clusters in all                                     */
  int S;                   /* padded states per cluster                           */
  int d;                   /* emission dimension (the base set's)                 */
  int max_model_clusters;  /* 1 .. 64                                             */
  const int *model_off;    /* [G + 1]                                             */
  const int *nstates_r;    /* [C]      own states, 1 .. S                         */
  const double *logw;      /* [C]      log mixture weight (-inf allowed)          */
  const double *scale;     /* [G]      the model's N~ (multiplies L)              */
  const double *logA;      /* [C][S][S]                                           */
  const double *logPi;     /* [C][S]                                              */
  const double *m;         /* [C][S][d]                                           */
  const double *P;         /* [C][S][d]                                           */
  const double *c;         /* [C][S]                                              */
} vbhmm_dic_models_t;

/* Workspace of vbhmm_dic_loglik: the prepared cluster blocks (C of them) and one
 * partial sum per (tile of 64 bases, model).  Nothing in it scales with N * C.
 * 0: unsupported or invalid descriptor. */
size_t vbhmm_dic_workspace_bytes(const vbhem_base_t *base, const vbhmm_dic_models_t *models, int T);

/*   L(i, c)  = the VHEM expected log-likelihood of base HMM i under cluster c, tau = T
 *   LL[g]    = sum_i  LSE_{c in model g} ( logw[c] + scale[g] * L(i, c) )
 * LL_dev [G]; L_pairs_dev [N][C] or NULL.  The LSE takes the maximum first and adds in
 * cluster order; the sum over i adds the bases of a tile in index order and the tiles
 * in a fixed order that depends on N alone, so LL[g] is bit for bit the same whether
 * model g is submitted alone or at any position of a grid.  No atomics.  A pair whose
 * factorised log-sum-exp underflows is recomputed in reference order inside the call.
 * Non-finite inputs make the L of the pairs that read them NaN and leave the others
 * alone.  Enqueue-only on `stream`: no allocation, no host synchronisation.
 * Supported: SB, S, d <= 16, T >= 1, at most 64 clusters per model, diag covariances;
 * anything else returns VBHEM_ERR_UNSUPPORTED.  The workspace is 16-byte aligned. */
int vbhmm_dic_loglik(const vbhem_base_t *base, const vbhmm_dic_models_t *models, int T,
                     double *LL_dev, double *L_pairs_dev, void *workspace_dev,
                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_DIC_H */
