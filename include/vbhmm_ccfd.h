/*
 * vbhmm_ccfd.h -- C-ABI of CCFD clustering of point HMMs on MI355X: the distance
 * matrix of the reference's
 *     src/compare_mtds/ccfd/myccfd.m:14-30   (symmetrised vbhmm_kld of every pair)
 * computed without the [H][N_total] log-likelihood matrix, and the O(N^2) sweeps of
 *     src/compare_mtds/ccfd/CCFD.m:36-60, :194-206
 * over that matrix (local density, distance to the nearest denser point, border
 * density).  The O(N) rest of CCFD.m runs on the host (vbhem_amd/ccfd.py).
 *
 * HMM sets and their prepared buffer are those of include/vbhmm_score.h
 * (vbhmm_score_prepare); sequences are a vbhmm_seqs_t (include/vbhmm_fb.h).  All
 * pointers but the descriptors are device pointers.  Status codes and
 * vbhem_last_error() as include/vbhem_estep.h.
 */
#ifndef VBHMM_CCFD_H
#define VBHMM_CCFD_H

#include <stddef.h>

#include "vbhmm_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vbhmm_ccfd_distance for H HMMs and N_total sequences in all:
 * the own-likelihood vector and the two tile tables (0: invalid sizes). */
size_t vbhmm_ccfd_distance_workspace_bytes(int H, long long n_total);

/* D [H][H]: D[i][j] = D[j][i] = 0.5 (KL[i][j] + KL[j][i]) for i < j, D[i][i] = 0,
 *   KL[i][j] = (1 / c_i) sum_n (ll_i(n) / T_n - ll_j(n) / T_n)
 * over the c_i sequences n = seg_offsets[i] .. seg_offsets[i + 1] - 1 of HMM i, in
 * index order, ll as vbhmm_score_ll (zero-density floor, no other rescue).  An empty
 * segment or an empty sequence gives NaN.  seqs->N must equal seg_offsets[H].
 * rowmin / rowmax [H]: the minimum and maximum of D[i][j] over j > i (+inf / -inf
 * for the last row), NaN entries skipped.  The workspace is 16-byte aligned.
 * Reads seg_offsets back to build the tile tables: synchronises `stream` once,
 * before the first launch. */
int vbhmm_ccfd_distance(const vbhmm_score_hmms_t *hmms, const void *prepared_dev,
                        const vbhmm_seqs_t *seqs_dev, const int *seg_offsets_dev,
                        void *workspace_dev, size_t workspace_bytes, double *D_dev,
                        double *rowmin_dev, double *rowmax_dev, void *stream);

/* rowmin / rowmax [N] of any D [N][N] over j > i, as vbhmm_ccfd_distance emits them. */
int vbhmm_ccfd_rowstats(const double *D_dev, int N, double *rowmin_dev, double *rowmax_dev,
                        void *stream);

/* rho_out [C][N] (int): rho[c][i] = #{ j != i : D[i][j] < dc[c] }; dc is a host
 * array of 1 <= C <= 3 cut-offs, all evaluated in one read of D. */
int vbhmm_ccfd_rho(const double *D_dev, int N, const double *dc, int C, int *rho_out_dev,
                   void *stream);

/* rank [C][N] (int): the position of every point in the stable descending sort of
 * rho[c] (a permutation of 0 .. N - 1).  Row i looks at the points j with
 * rank[j] < rank[i] and takes the lexicographic minimum of (D[i][j], rank[j]); when
 * that D is < maxd, delta = D and nneigh = j, otherwise delta = maxd and nneigh = -1.
 * The row of rank 0 gets delta = -1 and nneigh = -1.  1 <= C <= 3, one read of D. */
int vbhmm_ccfd_delta(const double *D_dev, int N, const int *rank_dev, int C, double maxd,
                     double *delta_out_dev, int *nneigh_out_dev, void *stream);

/* rowmax_out [N]: the largest (rho[i] + rho[j]) / 2 over j with cl[j] != cl[i] and
 * D[i][j] <= dc, or 0 when there is none. */
int vbhmm_ccfd_border(const double *D_dev, int N, double dc, const int *cl_dev,
                      const int *rho_dev, double *rowmax_out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_CCFD_H */
