// tests/ccfdcheck/ccfdcheck.hip -- TEST-ONLY exports of the CCFD arithmetic: host
// loops over the routines the kernels call (csrc/vbhmm_ccfd_row.h for the passes,
// pair_loglik of csrc/vbhmm_score_pair.h for the distance), so the logic is checked
// on a machine without a GPU, and the same calls through the library's kernels on
// device 0.  Arrays are host arrays in the layouts of include/vbhmm_score.h and
// include/vbhmm_ccfd.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "device_pool.h"
#include "host_prepare.h"
#include "vbhmm_ccfd.h"
#include "vbhmm_ccfd_row.h"
#include "vbhmm_score_pair.h"

namespace {

using namespace vbhem::score;
using namespace vbhem::ccfd;

struct HostDistance {
  const Layout &L;
  const std::vector<double> &blocks;
  int H, d;
  bool diag;
  const int *offsets, *seg;
  const double *x;
  double *D;
  template <int KB, int DB>
  int operator()() const {
    std::vector<double> KL((size_t)H * H, 0.0), own;
    for (int i = 0; i < H; ++i) {
      const Hmm mi = view(L, blocks.data() + (size_t)i * L.stride, diag);
      const int c = seg[i + 1] - seg[i];
      own.assign((size_t)c, 0.0);
      for (int q = 0; q < c; ++q) {
        const int off = offsets[seg[i] + q], T = offsets[seg[i] + q + 1] - off;
        own[q] = pair_loglik<KB, DB>(mi, x + (size_t)off * d, T, d) / (double)T;
      }
      for (int j = 0; j < H; ++j) {
        const Hmm mj = view(L, blocks.data() + (size_t)j * L.stride, diag);
        double sum = 0.0;
        for (int q = 0; q < c; ++q) {
          const int off = offsets[seg[i] + q], T = offsets[seg[i] + q + 1] - off;
          sum += kl_term(own[q], pair_loglik<KB, DB>(mj, x + (size_t)off * d, T, d), T);
        }
        KL[(size_t)i * H + j] = sum / (double)c;
      }
    }
    for (int i = 0; i < H; ++i) {
      D[(size_t)i * H + i] = 0.0;
      for (int j = i + 1; j < H; ++j) {
        const double v = 0.5 * (KL[(size_t)i * H + j] + KL[(size_t)j * H + i]);
        D[(size_t)i * H + j] = v;
        D[(size_t)j * H + i] = v;
      }
    }
    return 0;
  }
};

using checklib::Pool;

}  // namespace

extern "C" {

// D [H][H].  0, or 1 + (h KM + k) of the first covariance that is not positive definite.
long long ccfdcheck_distance_host(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                                  const double *trans, const double *mean, const double *cov, int N,
                                  const int *offsets, const double *x, const int *seg, double *D) {
  const Layout L = make_layout(KM, d);
  std::vector<double> blocks;
  const long long bad = checklib::host_prepare(L, H, KM, d, covmode, nstates, prior, trans, mean, cov, blocks);
  if (bad) return bad;
  (void)N;
  return dispatch(KM, d, HostDistance{L, blocks, H, d, covmode == VBHEM_COV_DIAG, offsets, seg, x, D});
}

// The same through vbhmm_score_prepare / vbhmm_ccfd_distance on device 0; rowmin and
// rowmax [H] too.  Returns the library's status, or a positive hipError_t of the copies.
int ccfdcheck_distance_device(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                              const double *trans, const double *mean, const double *cov, int N,
                              const int *offsets, const double *x, const int *seg, double *D, double *rowmin,
                              double *rowmax) {
  const size_t cs = covmode == VBHEM_COV_DIAG ? (size_t)d : (size_t)d * d;
  const long long total = N > 0 ? offsets[N] : 0;
  Pool pool;
  vbhmm_score_hmms_t m = {H, KM, d, covmode,
                          static_cast<const int *>(pool.put(nstates, (size_t)H * sizeof(int))),
                          static_cast<const double *>(pool.put(prior, (size_t)H * KM * 8)),
                          static_cast<const double *>(pool.put(trans, (size_t)H * KM * KM * 8)),
                          static_cast<const double *>(pool.put(mean, (size_t)H * KM * d * 8)),
                          static_cast<const double *>(pool.put(cov, (size_t)H * KM * cs * 8))};
  vbhmm_seqs_t s = {N, d, 0, static_cast<const int *>(pool.put(offsets, (size_t)(N + 1) * sizeof(int))),
                    static_cast<const double *>(pool.put(x, (size_t)total * d * 8))};
  const int *dseg = static_cast<const int *>(pool.put(seg, (size_t)(H + 1) * sizeof(int)));
  const size_t pb = vbhmm_score_prepared_bytes(&m), wb = vbhmm_ccfd_distance_workspace_bytes(H, N);
  void *prep = pool.put(nullptr, pb), *ws = pool.put(nullptr, wb);
  double *dD = static_cast<double *>(pool.put(nullptr, (size_t)H * H * 8));
  double *dmin = static_cast<double *>(pool.put(nullptr, (size_t)H * 8));
  double *dmax = static_cast<double *>(pool.put(nullptr, (size_t)H * 8));
  if (pool.e != hipSuccess) return (int)pool.e;
  int rc = vbhmm_score_prepare(&m, prep, pb, nullptr);
  if (rc == 0) rc = vbhmm_ccfd_distance(&m, prep, &s, dseg, ws, wb, dD, dmin, dmax, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(D, dD, (size_t)H * H * 8);
  pool.get(rowmin, dmin, (size_t)H * 8);
  pool.get(rowmax, dmax, (size_t)H * 8);
  return (int)pool.e;
}

// The passes of include/vbhmm_ccfd.h in host loops over the rows, j ascending.
void ccfdcheck_rowstats_host(const double *D, int N, double *rowmin, double *rowmax) {
  for (int i = 0; i < N; ++i) {
    double mn = INFINITY, mx = -INFINITY;
    for (int j = i + 1; j < N; ++j) {
      mn = std::fmin(mn, D[(size_t)i * N + j]);
      mx = std::fmax(mx, D[(size_t)i * N + j]);
    }
    rowmin[i] = mn;
    rowmax[i] = mx;
  }
}

void ccfdcheck_rho_host(const double *D, int N, const double *dc, int C, int *rho) {
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < N; ++i) {
      int cnt = 0;
      for (int j = 0; j < N; ++j)
        if (j != i && rho_hit(D[(size_t)i * N + j], dc[c])) ++cnt;
      rho[(size_t)c * N + i] = cnt;
    }
}

void ccfdcheck_delta_host(const double *D, int N, const int *rank, int C, double maxd, double *delta,
                          int *nneigh) {
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < N; ++i) {
      const int *rk = rank + (size_t)c * N;
      Best b = best_none();
      for (int j = 0; j < N; ++j) best_take(b, D[(size_t)i * N + j], rk[j], rk[i], j);
      best_finish(b, rk[i], maxd, delta[(size_t)c * N + i], nneigh[(size_t)c * N + i]);
    }
}

void ccfdcheck_border_host(const double *D, int N, double dc, const int *cl, const int *rho, double *out) {
  for (int i = 0; i < N; ++i) {
    double mx = 0.0;
    for (int j = 0; j < N; ++j)
      if (border_hit(D[(size_t)i * N + j], dc, cl[i], cl[j])) mx = std::fmax(mx, border_value(rho[i], rho[j]));
    out[i] = mx;
  }
}

// All four passes through the kernels on device 0 (cl / rho_for_border: the border
// pass's inputs; rho_out [C][N] is the rho pass's own result).
int ccfdcheck_passes_device(const double *D, int N, const double *dc, int C, const int *rank, double maxd,
                            const int *cl, const int *rho_for_border, double *rowmin, double *rowmax,
                            int *rho_out, double *delta, int *nneigh, double *border) {
  Pool pool;
  const size_t n8 = (size_t)N * 8, n4 = (size_t)N * sizeof(int);
  const double *dD = static_cast<const double *>(pool.put(D, (size_t)N * N * 8));
  const int *drank = static_cast<const int *>(pool.put(rank, n4 * C));
  const int *dcl = static_cast<const int *>(pool.put(cl, n4));
  const int *drb = static_cast<const int *>(pool.put(rho_for_border, n4));
  double *dmin = static_cast<double *>(pool.put(nullptr, n8)), *dmax = static_cast<double *>(pool.put(nullptr, n8));
  int *drho = static_cast<int *>(pool.put(nullptr, n4 * C)), *dnn = static_cast<int *>(pool.put(nullptr, n4 * C));
  double *ddelta = static_cast<double *>(pool.put(nullptr, n8 * C));
  double *dborder = static_cast<double *>(pool.put(nullptr, n8));
  if (pool.e != hipSuccess) return (int)pool.e;
  int rc = vbhmm_ccfd_rowstats(dD, N, dmin, dmax, nullptr);
  if (rc == 0) rc = vbhmm_ccfd_rho(dD, N, dc, C, drho, nullptr);
  if (rc == 0) rc = vbhmm_ccfd_delta(dD, N, drank, C, maxd, ddelta, dnn, nullptr);
  if (rc == 0) rc = vbhmm_ccfd_border(dD, N, dc[0], dcl, drb, dborder, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(rowmin, dmin, n8);
  pool.get(rowmax, dmax, n8);
  pool.get(rho_out, drho, n4 * C);
  pool.get(delta, ddelta, n8 * C);
  pool.get(nneigh, dnn, n4 * C);
  pool.get(border, dborder, n8);
  return (int)pool.e;
}

}  // extern "C"
