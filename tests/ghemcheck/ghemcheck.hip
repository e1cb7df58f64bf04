// tests/ghemcheck/ghemcheck.hip -- TEST-ONLY exports of the batched 'gmmNew' initialisation:
// the serial walker of csrc/vbhem_ghem_run.h on host arrays (where = 0), so the arithmetic
// is checked on a machine without a GPU, and the library's call (include/vbhem_init.h) on
// device 0 (where = 1).  Arrays are host arrays; outputs of trials that are not OK keep
// what the caller put there.  Returns 0, -2 outside the limits, the library's status, or a
// positive hipError_t.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_pool.h"
#include "vbhem_init.h"
#include "ghem_walk.h"

using checklib::Pool;

extern "C" {

// the point tile of the n-term sums
int ghemcheck_tile_points(int n, int d) { return vbhem::ghemrun::tile_points(n, d); }

// R trials: ghemwalk::fit_trials, or vbhem_ghem_fit_batch.  init, logpost: null or arrays.
int ghemcheck_fit(int where, int n, int d, int full, int T, int R, const double *X, const double *C, double vs,
                  int iterations, const int *j0, const double *u, const double *init, int chunk_trials, double *mxwt,
                  double *centres, double *covars, double *logpost, double *logp, int *status, int *iters) {
  using namespace vbhem::ghemrun;
  const int cd = cov_len(d, full != 0), nu = std::max(T - 1, 1);
  if (where == 0) {
    if (n < 1 || d < 1 || d > kMaxDim || T < 2 || T > kMaxT || R < 0 || iterations < 0) return -2;
    ghemwalk::fit_trials(n, d, full != 0, T, R, X, C, vs, iterations, j0, u, init, mxwt, centres, covars, logpost, logp,
                         status, iters);
    return 0;
  }
  if (n < 1 || d < 1 || T < 1 || R < 0) return -1;
  Pool pool;
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const double *dC = static_cast<const double *>(pool.put(C, (size_t)n * cd * 8));
  const int *dj = init ? nullptr : static_cast<const int *>(pool.put(j0, (size_t)R * 4));
  const double *du = init ? nullptr : static_cast<const double *>(pool.put(u, (size_t)R * nu * 8));
  const double *di = init ? static_cast<const double *>(pool.put(init, (size_t)R * T * d * 8)) : nullptr;
  double *dm = static_cast<double *>(pool.put(mxwt, (size_t)R * T * 8));
  double *dce = static_cast<double *>(pool.put(centres, (size_t)R * T * d * 8));
  double *dco = static_cast<double *>(pool.put(covars, (size_t)R * T * cd * 8));
  double *dlp = logpost ? static_cast<double *>(pool.put(logpost, (size_t)R * T * n * 8)) : nullptr;
  double *dl = static_cast<double *>(pool.put(logp, (size_t)R * 8));
  int *ds = static_cast<int *>(pool.put(status, (size_t)R * 4));
  int *dit = static_cast<int *>(pool.put(iters, (size_t)R * 2 * 4));
  const size_t wb = vbhem_ghem_workspace_bytes(n, d, full, T, R, chunk_trials);
  void *ws = pool.put(nullptr, wb);
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhem_ghem_fit_batch(n, d, full, T, R, dX, dC, vs, iterations, dj, du, di, chunk_trials, dm, dce, dco,
                                      dlp, dl, ds, dit, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(mxwt, dm, (size_t)R * T * 8);
  pool.get(centres, dce, (size_t)R * T * d * 8);
  pool.get(covars, dco, (size_t)R * T * cd * 8);
  pool.get(logpost, dlp, (size_t)R * T * n * 8);
  pool.get(logp, dl, (size_t)R * 8);
  pool.get(status, ds, (size_t)R * 4);
  pool.get(iters, dit, (size_t)R * 2 * 4);
  return (int)pool.e;
}

}  // extern "C"
