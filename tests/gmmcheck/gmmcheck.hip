// tests/gmmcheck/gmmcheck.hip -- TEST-ONLY exports of the batched GMM fit: the serial
// walker over the fit routines the kernel calls (csrc/vbhmm_gmm_run.h) on host arrays, so
// the arithmetic is checked on a machine without a GPU, and the same call through the
// library's kernels on device 0.  Arrays are host arrays in the layouts of
// include/vbhmm_gmm.h; hyper (or null) = [alpha0, epsilon0, beta0, v0, m0[8],
// W0inv_diag[8]], post_init (or null) with it.  Output rows of fits that write nothing keep
// what the caller put there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device_pool.h"
#include "hyper_vec.h"
#include "vbhmm_batch_launch.h"
#include "vbhmm_gmm.h"
#include "vbhmm_gmm_run.h"

namespace {

using namespace vbhem::gmmrun;

using checklib::Pool;

int max_obs_of(int S, const int *offsets, const int *seq_first) {
  int m = 0;
  for (int s = 0; s < S; ++s) m = std::max(m, offsets[seq_first[s + 1]] - offsets[seq_first[s]]);
  return m;
}

template <int KM>
void host_fits(int S, int dim, const int *offsets, const double *x, const int *seq_first, int R, const int *subject,
               const int *K, const int *rows, const double *reg, int max_iter, double tolfun, const Hyper *h,
               double *prior, double *mean, double *cov, double *ll, int *iters, int *status, double *lls,
               double *post_init) {
  const int max_obs = max_obs_of(S, offsets, seq_first), PL = vbhem::emrun::post_len(KM, dim);
  std::vector<double> post((size_t)max_obs * KM + 1), lse(max_obs + 1);
  const Work w{post.data(), lse.data()};
  for (int r = 0; r < R; ++r) {
    if (subject[r] < 0 || subject[r] >= S) {
      status[r] = kBadFit;
      continue;
    }
    const int row0 = offsets[seq_first[subject[r]]], N = offsets[seq_first[subject[r] + 1]] - row0;
    const FitResult res = run_serial<KM>(K[r], dim, N, max_obs, x + (size_t)row0 * dim, rows + (size_t)r * KM, reg[r],
                                         max_iter, tolfun, prior + (size_t)r * KM, mean + (size_t)r * KM * dim,
                                         cov + (size_t)r * KM * dim * dim, lls ? lls + (size_t)r * max_iter : nullptr,
                                         h, h && post_init ? post_init + (size_t)r * PL : nullptr, w);
    status[r] = res.status;
    if (res.status == kBadFit) continue;
    ll[r] = res.ll;
    iters[r] = res.iters;
  }
}

}  // namespace

extern "C" {

// Every fit by run_serial.  -2: outside the routines' limits.
int gmmcheck_host(int S, int dim, const int *offsets, const double *x, const int *seq_first, int R, int KM,
                  const int *subject, const int *K, const int *rows, const double *reg, int max_iter, double tolfun,
                  const double *hyper, double *prior, double *mean, double *cov, double *ll, int *iters, int *status,
                  double *lls, double *post_init) {
  if ((KM != 4 && KM != 8) || dim < 1 || dim > kMaxDim || max_iter < 1 || S < 1) return -2;
  Hyper h{};
  if (hyper) {
    const vbhmm_em_hyper_t hy = checklib::hyper_struct(hyper);
    h = vbhem::batch::to_hyper(&hy, dim);
  }
  if (KM == 4)
    host_fits<4>(S, dim, offsets, x, seq_first, R, subject, K, rows, reg, max_iter, tolfun, hyper ? &h : nullptr, prior,
                 mean, cov, ll, iters, status, lls, post_init);
  else
    host_fits<8>(S, dim, offsets, x, seq_first, R, subject, K, rows, reg, max_iter, tolfun, hyper ? &h : nullptr, prior,
                 mean, cov, ll, iters, status, lls, post_init);
  return 0;
}

// vbhmm_gmm_fit_batch on device 0: the output arrays go up as the caller filled them and
// come back as the kernels left them.  Returns the library's status, or a positive
// hipError_t of the copies.
int gmmcheck_device(int S, int dim, const int *offsets, const double *x, const int *seq_first, int R, int KM,
                    const int *subject, const int *K, const int *rows, const double *reg, int max_iter, double tolfun,
                    const double *hyper, int chunk_runs, double *prior, double *mean, double *cov, double *ll,
                    int *iters, int *status, double *lls, double *post_init) {
  if (KM < 1 || dim < 1 || S < 1 || R < 0 || max_iter < 1) return -1;
  Pool pool;
  const int Ntot = seq_first[S], nrows = offsets[Ntot];
  const size_t PL = vbhmm_em_post_len(KM, dim);
  vbhmm_em_subjects_t sb{};
  sb.seqs.N = Ntot; sb.seqs.dim = dim; sb.seqs.maxT = 0;
  sb.seqs.offsets = static_cast<const int *>(pool.put(offsets, (size_t)(Ntot + 1) * sizeof(int)));
  sb.seqs.x = static_cast<const double *>(pool.put(x, (size_t)nrows * dim * 8));
  sb.S = S;
  sb.seq_first = static_cast<const int *>(pool.put(seq_first, (size_t)(S + 1) * sizeof(int)));
  sb.max_obs = max_obs_of(S, offsets, seq_first);
  for (int s = 0; s < S; ++s) sb.max_seqs = std::max(sb.max_seqs, seq_first[s + 1] - seq_first[s]);
  const vbhmm_gmm_fits_t ft{R, KM, static_cast<const int *>(pool.put(subject, (size_t)R * sizeof(int))),
                            static_cast<const int *>(pool.put(K, (size_t)R * sizeof(int))),
                            static_cast<const int *>(pool.put(rows, (size_t)R * KM * sizeof(int))),
                            static_cast<const double *>(pool.put(reg, (size_t)R * 8))};
  vbhmm_em_hyper_t hy{};
  if (hyper) hy = checklib::hyper_struct(hyper);
  const vbhmm_gmm_opt_t opt{max_iter, tolfun, chunk_runs};
  const size_t wb = vbhmm_gmm_fit_workspace_bytes(&sb, R, KM, chunk_runs);
  void *ws = pool.put(nullptr, wb);
  double *dpr = static_cast<double *>(pool.put(prior, (size_t)R * KM * 8));
  double *dme = static_cast<double *>(pool.put(mean, (size_t)R * KM * dim * 8));
  double *dco = static_cast<double *>(pool.put(cov, (size_t)R * KM * dim * dim * 8));
  double *dll = static_cast<double *>(pool.put(ll, (size_t)R * 8));
  int *dit = static_cast<int *>(pool.put(iters, (size_t)R * sizeof(int)));
  int *dss = static_cast<int *>(pool.put(status, (size_t)R * sizeof(int)));
  double *dlls = lls ? static_cast<double *>(pool.put(lls, (size_t)R * max_iter * 8)) : nullptr;
  double *dpi = hyper && post_init ? static_cast<double *>(pool.put(post_init, (size_t)R * PL * 8)) : nullptr;
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhmm_gmm_fit_batch(&sb, &ft, &opt, dpr, dme, dco, dll, dit, dss, dlls, dpi ? &hy : nullptr, dpi, ws,
                                     wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(prior, dpr, (size_t)R * KM * 8);
  pool.get(mean, dme, (size_t)R * KM * dim * 8);
  pool.get(cov, dco, (size_t)R * KM * dim * dim * 8);
  pool.get(ll, dll, (size_t)R * 8);
  pool.get(iters, dit, (size_t)R * sizeof(int));
  pool.get(status, dss, (size_t)R * sizeof(int));
  if (lls) pool.get(lls, dlls, (size_t)R * max_iter * 8);
  if (dpi) pool.get(post_init, dpi, (size_t)R * PL * 8);
  return (int)pool.e;
}

}  // extern "C"
