/*
 * vbhmm_kld.h -- C-ABI of KL jobs over gathered sequence lists on MI355X: many
 * vbhmm_kld values (src/hmm/vbhmm_kld.m with 'n') in one call, each over its own
 * list of sequences, without a log-likelihood matrix.  What the Dunn index of the
 * reference's
 *     Synthetic_experiment/compute_hmms_dist.m:47-65
 *     Synthetic_experiment/compute_inter_Centhmms_dist.m:40-54
 * needs: every centre against its members and against the other centres, each pair
 * on the data of one side only.
 *
 * HMM sets and their prepared buffer are those of include/vbhmm_score.h
 * (vbhmm_score_prepare); sequences are a vbhmm_seqs_t (include/vbhmm_fb.h).  The HMM
 * descriptor's arrays, the prepared buffer, the sequences' arrays, the workspace and
 * kl are device pointers; list_offsets, list_items and jobs are HOST arrays.  Status
 * codes and vbhem_last_error() as include/vbhem_estep.h.
 */
#ifndef VBHMM_KLD_H
#define VBHMM_KLD_H

#include <stddef.h>

#include "vbhmm_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vbhmm_kld_jobs for these lists and jobs: the own-likelihood table (one
 * double per item of every unique (a, list) of the jobs) and the planner's tables
 * (4 bytes per own slot, a few words per job and per tile).  0: invalid counts,
 * offsets or job indices. */
size_t vbhmm_kld_jobs_workspace_bytes(int n_lists, const int *list_offsets, int n_jobs,
                                      const int *jobs);

/* kl [n_jobs]: for job p = (a, b, list) over the c items n_0 .. n_{c-1} of its list
 *   kl[p] = (1 / c) sum_q (ll_a(n_q) / T_q - ll_b(n_q) / T_q),
 * the terms added one after the other in list order from 0.0; ll as vbhmm_score_ll
 * (zero-density floor).  List l is list_items[list_offsets[l] .. list_offsets[l + 1]):
 * indices into seqs, in any order, non-contiguous, repeated.  An empty list, or an
 * empty sequence in the list, gives NaN.  a == b is computed like any other job.
 * A job's value is the same chain of additions whatever other jobs the call holds.
 *
 * Checked on the host before anything is uploaded or launched: list_offsets starts at
 * >= 0 and does not decrease, every a and b lies in [0, H), every list in
 * [0, n_lists), every item of a list that a job uses in [0, seqs->N); else
 * VBHEM_ERR_ARG and vbhem_last_error() names the first offender.  n_jobs == 0
 * succeeds and launches nothing.  The workspace is 16-byte aligned.  Uploads the
 * planner's tables and synchronises `stream` once, before the first launch. */
int vbhmm_kld_jobs(const vbhmm_score_hmms_t *hmms, const void *prepared_dev,
                   const vbhmm_seqs_t *seqs_dev, int n_lists, const int *list_offsets,
                   const int *list_items, int n_jobs, const int *jobs, void *workspace_dev,
                   size_t workspace_bytes, double *kl_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBHMM_KLD_H */
