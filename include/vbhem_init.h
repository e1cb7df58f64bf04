/*
 * vbhem_init.h -- C-ABI of the batched clustering initialisations on MI355X: 'wtkmeans'
 * here, 'gmmNew' (vbhem_ghem_fit_batch) further down.  The batched 'wtkmeans' initialisation
 * (vbhemhmm_init.m:294-425 as h3m.py wtkmeans_init restates it): the k-means++ seeding with
 * Lloyd updates (h3m.kmeans_pp) and the weighted k-means (my_weighted_kmeans.m,
 * h3m.weighted_kmeans) of every TRIAL of a list in two calls.  Every random draw is an
 * input, so the host keeps the generators and their order.
 *
 *   vbhem_wtk_cluster_batch  one workgroup per trial: kmeans_pp over all n points for K
 *                            centres, then weighted_kmeans from them
 *   vbhem_wtk_states_batch   one workgroup per ITEM = (trial, cluster) with more than S
 *                            members: kmeans_pp over the cluster's members (in point order)
 *                            for S centres
 * The second call's first draw of an item is an index into the cluster's members, so the
 * host reads counts between the calls.
 *
 * Layouts (row-major, DEVICE pointers; return codes and stream of vbhem_estep.h):
 *   points:  x[n][d], weight[n]
 *   draws:   j0[.]: the first centre, an index into the members (all points in the first
 *            call); u[.][max(k - 1, 1)]: the uniform draw of centre c at [c - 1]
 *   cluster: labels[R][n], counts[R][K], status[R], iters[R][2] (Lloyd passes, sweeps)
 *   states:  trial[I], cluster[I], nmem[I] (the cluster's member count, as counts gave it),
 *            off[I] (the item's first slot in the workspace: the exclusive prefix sums of
 *            nmem, total_members their sum); centres[R][K][S][d]: the rows of the items;
 *            status[I], iters[I]
 * Status: VBHEM_WTK_OK; VBHEM_WTK_DEGENERATE: a D2 total of zero (fewer distinct points
 * than centres), where the host's generator would take another branch; VBHEM_WTK_BAD: a
 * non-finite coordinate or weight, or an index, count or slot out of range.  A trial or
 * item that is not OK writes its status alone.
 * Limits: d <= 16, K <= 32, S <= 16; beyond: VBHEM_ERR_UNSUPPORTED.
 *
 * Every sum, scan and tie is taken in a fixed order: a trial's or item's result depends on
 * its own inputs only -- not on R, its place in the list or chunk_trials (trials per
 * launch; 0: as many as fit VBHEM_WTK_DEFAULT_WORKSPACE bytes).
 */
#ifndef VBHEM_INIT_H
#define VBHEM_INIT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBHEM_WTK_OK 0
#define VBHEM_WTK_DEGENERATE 1
#define VBHEM_WTK_BAD 2

#define VBHEM_WTK_MAX_DIM 16
#define VBHEM_WTK_MAX_K 32
#define VBHEM_WTK_MAX_S 16
#define VBHEM_WTK_DEFAULT_WORKSPACE ((size_t)1 << 30)

/* Workspace of a first-stage call (0 on invalid / unsupported sizes). */
size_t vbhem_wtk_cluster_workspace_bytes(int n, int d, int K, int R, int chunk_trials);

int vbhem_wtk_cluster_batch(int n, int d, int K, int R, const double *x_dev, const double *weight_dev,
                            const int *j0_dev, const double *u_dev, int chunk_trials, int *labels_dev,
                            int *counts_dev, int *status_dev, int *iters_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream);

/* Workspace of a second-stage call over items with total_members members in all. */
size_t vbhem_wtk_states_workspace_bytes(long long total_members);

int vbhem_wtk_states_batch(int n, int d, int K, int S, int R, const double *x_dev, const int *labels_dev, int I,
                           const int *trial_dev, const int *cluster_dev, const int *nmem_dev,
                           const long long *off_dev, long long total_members, const int *j0_dev,
                           const double *u_dev, double *centres_dev, int *status_dev, int *iters_dev,
                           void *workspace_dev, size_t workspace_bytes, void *stream);

/*
 * The TILED schedule of the same k-means (csrc/vbhem_wtk_tiled.hip).  The calls above give
 * a trial to one workgroup (the BLOCK schedule); these spread every pass of every trial over
 * a grid of (point tile, group of trials) and let a small per-trial kernel add the tile
 * partials in tile order and apply the rule, round after round, with no host read.  The
 * number of launches is fixed by K and the pass caps: 2 ((K - 1) + 100 + 1 + 101) + 2 for the
 * first entry, 2 ((K - 1) + 100) + 2 for the second, per chunk of trials.
 *
 *   vbhem_wtk_cluster_tiled_batch  vbhem_wtk_cluster_batch's arguments, layouts, statuses and
 *                                  limits
 *   vbhem_wtk_seed_tiled_batch     kmeans_pp alone over all n points for K centres:
 *                                  centres[R][K][d], status[R], iters[R] (Lloyd passes); the
 *                                  start centres of vbhem_ghem_fit_batch's init_centres.
 *                                  Limits: d <= 16, 2 <= K <= VBHEM_GHEM_MAX_T; beyond:
 *                                  VBHEM_ERR_UNSUPPORTED (K < 2: VBHEM_ERR_ARG)
 * Per-point values are the block schedule's bit for bit; the n-term sums run over point
 * tiles whose size depends on (n, d) only (256 points up to n = 262,144, 1,024 beyond), in
 * point order inside a tile and in tile order across tiles, so the discrete outputs equal
 * the block schedule's wherever no decision is within rounding, and a trial's result depends
 * on its own inputs only -- not on R, its place in the list or chunk_trials (0: as many as
 * fit VBHEM_WTK_DEFAULT_WORKSPACE bytes).  A trial whose Lloyd update empties a cluster is
 * computed by the block schedule inside the same call (the re-seed is sequential and rare).
 * A trial that is not OK writes its status alone.
 */
size_t vbhem_wtk_cluster_tiled_workspace_bytes(int n, int d, int K, int R, int chunk_trials);

int vbhem_wtk_cluster_tiled_batch(int n, int d, int K, int R, const double *x_dev, const double *weight_dev,
                                  const int *j0_dev, const double *u_dev, int chunk_trials, int *labels_dev,
                                  int *counts_dev, int *status_dev, int *iters_dev, void *workspace_dev,
                                  size_t workspace_bytes, void *stream);

size_t vbhem_wtk_seed_tiled_workspace_bytes(int n, int d, int K, int R, int chunk_trials);

int vbhem_wtk_seed_tiled_batch(int n, int d, int K, int R, const double *x_dev, const int *j0_dev, const double *u_dev,
                               int chunk_trials, double *centres_dev /* [R][K][d] */, int *status_dev,
                               int *iters_dev /* [R]: Lloyd passes */, void *workspace_dev, size_t workspace_bytes,
                               void *stream);

/*
 * The batched 'gmmNew' initialisation (vbhemhmm_init.m:103-293, GMM_MixHierEM.m as
 * h3m.gmm_mix_hier_em restates it for T >= 2): the mixture of all n base-state Gaussians
 * reduced to T components by hierarchical EM, every TRIAL of a list in one call.  A trial
 * is its k-means++ draws (j0, u: as above, over all n points) or, with init_centres given,
 * its start centres (no seeding, no draws read).
 *
 * Layouts (row-major, DEVICE pointers):
 *   points:  x[n][d]; cov[n][d][d] (full != 0) or cov[n][d]
 *   draws:   j0[R], u[R][max(T - 1, 1)]; init_centres[R][T][d] or NULL
 *   outputs: mxwt[R][T], centres[R][T][d], covars[R][T][d][d] or [R][T][d], logpost[R][T][n]
 *            or NULL (not wanted), logp[R] (of the last E-step evaluated), status[R],
 *            iters[R][2] (Lloyd passes of the seeding, E-steps evaluated)
 * Status: VBHEM_WTK_OK, VBHEM_WTK_DEGENERATE (the seeding's D2 total is zero),
 * VBHEM_WTK_BAD (a non-finite coordinate or covariance entry, a draw out of range),
 * VBHEM_GHEM_NONFINITE (a logp that is not finite), VBHEM_GHEM_SINGULAR (a pivot of a
 * covariance's Cholesky factor that is not > 0).  A trial that is not OK writes its status
 * alone.
 * Limits: d <= 16, 2 <= T <= 32; beyond: VBHEM_ERR_UNSUPPORTED (T < 2: VBHEM_ERR_ARG).
 *
 * Every n-term sum runs over point tiles whose size depends on (n, d) only, and the tile
 * partials are added in tile order: a trial's result depends on its own inputs only -- not
 * on R, its place in the list or chunk_trials (trials per round of launches; 0: as many as
 * fit VBHEM_GHEM_DEFAULT_WORKSPACE bytes).
 */
#define VBHEM_GHEM_NONFINITE 3
#define VBHEM_GHEM_SINGULAR 4

#define VBHEM_GHEM_MAX_DIM 16
#define VBHEM_GHEM_MAX_T 32
#define VBHEM_GHEM_DEFAULT_WORKSPACE ((size_t)1 << 30)

/* Workspace of a call (0 on invalid / unsupported sizes). */
size_t vbhem_ghem_workspace_bytes(int n, int d, int full, int T, int R, int chunk_trials);

int vbhem_ghem_fit_batch(int n, int d, int full, int T, int R, const double *x_dev, const double *cov_dev,
                         double virtual_samples, int iterations, const int *j0_dev, const double *u_dev,
                         const double *init_centres_dev, int chunk_trials, double *mxwt_dev, double *centres_dev,
                         double *covars_dev, double *logpost_dev, double *logp_dev, int *status_dev, int *iters_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHEM_INIT_H */
