// tests/vbhmmemcheck/vbhmmemcheck.hip -- TEST-ONLY exports of the batched VB-HMM EM: the
// serial walker over the run routines the kernel calls (csrc/vbhmm_em_run.h) on host
// arrays, so the arithmetic is checked on a machine without a GPU, and the same call
// through the library's kernels on device 0.  Arrays are host arrays in the layouts of
// include/vbhmm_em.h; hyper = [alpha0, epsilon0, beta0, v0, m0[8], W0inv_diag[8]].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device_pool.h"
#include "hyper_vec.h"
#include "vbhmm_batch_launch.h"
#include "vbhmm_em.h"
#include "vbhmm_em_run.h"

namespace {

using namespace vbhem::emrun;

using checklib::Pool;

void subject_maxima(int S, const int *offsets, const int *seq_first, int *max_seqs, int *max_obs) {
  *max_seqs = *max_obs = 0;
  for (int s = 0; s < S; ++s) {
    *max_seqs = std::max(*max_seqs, seq_first[s + 1] - seq_first[s]);
    *max_obs = std::max(*max_obs, offsets[seq_first[s + 1]] - offsets[seq_first[s]]);
  }
}

template <int KM>
void host_runs(int dim, const int *offsets, const double *x, const int *seq_first, int R, const int *subject,
               const int *K, const double *post_in, const Hyper &h, int max_iter, double min_diff,
               double *post_out, double *post_estep, double *stats, double *LL, int *iters, int *status,
               double *LLs, int max_seqs, int max_obs) {
  const int PL = post_len(KM, dim), SL = stats_len(KM, dim);
  std::vector<double> g((size_t)max_obs * KM + 1), lr((size_t)max_obs * KM + 1), cs(max_obs + 1), mx(max_obs + 1),
      sq((size_t)max_seqs * seq_len(KM) + 1);
  const Work<KM> w{g.data(), lr.data(), cs.data(), mx.data(), sq.data()};
  for (int r = 0; r < R; ++r) {
    const int n0 = seq_first[subject[r]];
    const Subject s{seq_first[subject[r] + 1] - n0, offsets + n0, x};
    for (int q = 0; q < PL; ++q) post_out[(size_t)r * PL + q] = post_in[(size_t)r * PL + q];
    const RunResult res = run_serial<KM>(K[r], dim, s, h, max_iter, min_diff, post_out + (size_t)r * PL,
                                         post_estep ? post_estep + (size_t)r * PL : nullptr,
                                         stats ? stats + (size_t)r * SL : nullptr,
                                         LLs ? LLs + (size_t)r * max_iter : nullptr, w);
    LL[r] = res.LL;
    iters[r] = res.iters;
    status[r] = res.status;
  }
}

}  // namespace

extern "C" {

// Every run by run_serial.  -2: outside the routines' limits.
int vbhmmemcheck_host(int S, int dim, const int *offsets, const double *x, const int *seq_first, int R, int KM,
                      const int *subject, const int *K, const double *post_in, const double *hyper, int max_iter,
                      double min_diff, double *post_out, double *post_estep, double *stats, double *LL, int *iters,
                      int *status, double *LLs) {
  if ((KM != 4 && KM != 8) || dim < 1 || dim > kMaxDim || max_iter < 1) return -2;
  for (int r = 0; r < R; ++r)
    if (K[r] < 1 || K[r] > KM || subject[r] < 0 || subject[r] >= S) return -2;
  int max_seqs, max_obs;
  subject_maxima(S, offsets, seq_first, &max_seqs, &max_obs);
  const vbhmm_em_hyper_t hy = checklib::hyper_struct(hyper);
  const Hyper h = vbhem::batch::to_hyper(&hy, dim);
  if (KM == 4)
    host_runs<4>(dim, offsets, x, seq_first, R, subject, K, post_in, h, max_iter, min_diff, post_out, post_estep,
                 stats, LL, iters, status, LLs, max_seqs, max_obs);
  else
    host_runs<8>(dim, offsets, x, seq_first, R, subject, K, post_in, h, max_iter, min_diff, post_out, post_estep,
                 stats, LL, iters, status, LLs, max_seqs, max_obs);
  return 0;
}

// vbhmm_em_batch on device 0.  Returns the library's status, or a positive hipError_t of
// the copies.
int vbhmmemcheck_device(int S, int dim, const int *offsets, const double *x, const int *seq_first, int R, int KM,
                        const int *subject, const int *K, const double *post_in, const double *hyper, int max_iter,
                        double min_diff, int chunk_runs, double *post_out, double *post_estep, double *stats,
                        double *LL, int *iters, int *status, double *LLs) {
  if (KM < 1 || dim < 1 || S < 1 || R < 0) return -1;
  Pool pool;
  const int Ntot = seq_first[S], rows = offsets[Ntot];
  const size_t PL = vbhmm_em_post_len(KM, dim), SL = vbhmm_em_stats_len(KM, dim);
  vbhmm_em_subjects_t sb{};
  sb.seqs.N = Ntot; sb.seqs.dim = dim; sb.seqs.maxT = 0;
  sb.seqs.offsets = static_cast<const int *>(pool.put(offsets, (size_t)(Ntot + 1) * sizeof(int)));
  sb.seqs.x = static_cast<const double *>(pool.put(x, (size_t)rows * dim * 8));
  sb.S = S;
  sb.seq_first = static_cast<const int *>(pool.put(seq_first, (size_t)(S + 1) * sizeof(int)));
  subject_maxima(S, offsets, seq_first, &sb.max_seqs, &sb.max_obs);
  vbhmm_em_runs_t rn{R, KM, static_cast<const int *>(pool.put(subject, (size_t)R * sizeof(int))),
                     static_cast<const int *>(pool.put(K, (size_t)R * sizeof(int))),
                     static_cast<const double *>(pool.put(post_in, (size_t)R * PL * 8))};
  const vbhmm_em_hyper_t hy = checklib::hyper_struct(hyper);
  const vbhmm_em_opt_t opt{max_iter, min_diff, chunk_runs};
  const size_t wb = vbhmm_em_batch_workspace_bytes(&sb, R, KM, chunk_runs);
  void *ws = pool.put(nullptr, wb);
  double *dpo = static_cast<double *>(pool.put(nullptr, (size_t)R * PL * 8));
  double *dpe = static_cast<double *>(pool.put(nullptr, (size_t)R * PL * 8));
  double *dst = static_cast<double *>(pool.put(nullptr, (size_t)R * SL * 8));
  double *dLL = static_cast<double *>(pool.put(nullptr, (size_t)R * 8));
  int *dit = static_cast<int *>(pool.put(nullptr, (size_t)R * sizeof(int)));
  int *dss = static_cast<int *>(pool.put(nullptr, (size_t)R * sizeof(int)));
  double *dLLs = LLs ? static_cast<double *>(pool.put(nullptr, (size_t)R * std::max(max_iter, 1) * 8)) : nullptr;
  if (pool.e != hipSuccess) return (int)pool.e;
  if (dLLs) pool.e = hipMemset(dLLs, 0, (size_t)R * std::max(max_iter, 1) * 8);
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhmm_em_batch(&sb, &rn, &hy, &opt, dpo, dpe, dst, dLL, dit, dss, dLLs, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(post_out, dpo, (size_t)R * PL * 8);
  pool.get(post_estep, dpe, (size_t)R * PL * 8);
  pool.get(stats, dst, (size_t)R * SL * 8);
  pool.get(LL, dLL, (size_t)R * 8);
  pool.get(iters, dit, (size_t)R * sizeof(int));
  pool.get(status, dss, (size_t)R * sizeof(int));
  if (LLs) pool.get(LLs, dLLs, (size_t)R * max_iter * 8);
  return (int)pool.e;
}

}  // extern "C"
