// tests/wtktilecheck/wtktilecheck.hip -- TEST-ONLY exports of the TILED schedule of the
// initialisations' k-means: the serial tiled walker of csrc/vbhem_wtk_tiled_run.h on host
// arrays (where = 0: the same phases, the same tile order, one lane), so the schedule is
// checked on a machine without a GPU, and the library's tiled entries on device 0
// (where = 1).  A trial whose re-seed flag the walker sets is handed to the block schedule's
// serial walker (csrc/vbhem_wtk_run.h), as the device call hands it to the block kernel.
// Arrays are host arrays; outputs of trials that are not OK keep what the caller put there.
// reseed [R] and rounds [R] (the rounds a trial used) are the walker's; the device leaves
// them.  Returns 0, -2 outside the limits, the library's status, or a positive hipError_t.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_pool.h"
#include "vbhem_init.h"
#include "vbhem_wtk_tiled_run.h"

namespace {

using namespace vbhem::wtktile;
using checklib::Pool;

bool in_limits(int n, int d, int K, int kmin) {
  return n >= 1 && d >= 1 && d <= kMaxDim && K >= kmin && K <= kMaxK;
}

struct Scratch {
  std::vector<double> rec, part, tot, dw, cen, cold, sums, cw;
  std::vector<int> lw;
  Scratch(int n, int d, int K)
      : rec(rec_len(K, d)), part((size_t)tiles_of(n, d) * part_len(K, d)), tot(part_len(K, d)), dw(n),
        cen((size_t)K * d), cold((size_t)K * d), sums((size_t)K * (d + 1)), cw(K), lw(n) {}
};

}  // namespace

extern "C" {

int wtktilecheck_tile_points(int n, int d) { return tile_points(n, d); }

int wtktilecheck_rounds(int K, int seed_only) { return rounds_of(K, seed_only != 0); }

// The first stage of R trials: tiled_trial_serial per trial, or vbhem_wtk_cluster_tiled_batch.
int wtktilecheck_cluster(int where, int n, int d, int K, int R, const double *X, const double *w, const int *j0,
                         const double *u, int chunk_trials, int *labels, int *counts, int *status, int *iters,
                         int *reseed, int *rounds) {
  const int nu = std::max(K - 1, 1);
  if (where == 0) {
    if (!in_limits(n, d, K, 1) || R < 0) return -2;
    Scratch s(n, d, K);
    for (int r = 0; r < R; ++r) {
      const WalkOut o = tiled_trial_serial(X, w, n, d, K, j0[r], u + (size_t)r * nu, false, s.rec.data(), s.part.data(),
                                           s.tot.data(), s.dw.data(), s.lw.data(), labels + (size_t)r * n,
                                           counts + (size_t)r * K, nullptr, iters + 2 * (size_t)r);
      reseed[r] = o.reseed;
      rounds[r] = o.rounds;
      status[r] = o.status;
      if (o.reseed)
        status[r] = cluster_trial_serial(X, w, n, d, K, j0[r], u + (size_t)r * nu, s.cen.data(), s.cold.data(),
                                         s.sums.data(), s.cw.data(), s.dw.data(), s.lw.data(), labels + (size_t)r * n,
                                         counts + (size_t)r * K, iters + 2 * (size_t)r);
    }
    return 0;
  }
  if (n < 1 || d < 1 || K < 1 || R < 0) return -1;
  Pool pool;
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const double *dwt = static_cast<const double *>(pool.put(w, (size_t)n * 8));
  const int *dj = static_cast<const int *>(pool.put(j0, (size_t)R * 4));
  const double *du = static_cast<const double *>(pool.put(u, (size_t)R * nu * 8));
  int *dl = static_cast<int *>(pool.put(labels, (size_t)R * n * 4));
  int *dc = static_cast<int *>(pool.put(counts, (size_t)R * K * 4));
  int *ds = static_cast<int *>(pool.put(status, (size_t)R * 4));
  int *di = static_cast<int *>(pool.put(iters, (size_t)R * 2 * 4));
  const size_t wb = vbhem_wtk_cluster_tiled_workspace_bytes(n, d, K, R, chunk_trials);
  void *ws = pool.put(nullptr, std::max<size_t>(wb, 16));
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc =
      vbhem_wtk_cluster_tiled_batch(n, d, K, R, dX, dwt, dj, du, chunk_trials, dl, dc, ds, di, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(status, ds, (size_t)R * 4);
  pool.get(labels, dl, (size_t)R * n * 4);
  pool.get(counts, dc, (size_t)R * K * 4);
  pool.get(iters, di, (size_t)R * 2 * 4);
  return (int)pool.e;
}

// kmeans_pp alone of R trials: tiled_trial_serial per trial, or vbhem_wtk_seed_tiled_batch.
int wtktilecheck_seed(int where, int n, int d, int K, int R, const double *X, const int *j0, const double *u,
                      int chunk_trials, double *centres, int *status, int *iters, int *reseed, int *rounds) {
  const int nu = std::max(K - 1, 1);
  if (where == 0) {
    if (!in_limits(n, d, K, 2) || R < 0) return -2;
    Scratch s(n, d, K);
    for (int r = 0; r < R; ++r) {
      const WalkOut o = tiled_trial_serial(X, nullptr, n, d, K, j0[r], u + (size_t)r * nu, true, s.rec.data(),
                                           s.part.data(), s.tot.data(), s.dw.data(), s.lw.data(), nullptr, nullptr,
                                           centres + (size_t)r * K * d, iters + r);
      reseed[r] = o.reseed;
      rounds[r] = o.rounds;
      status[r] = o.status;
      if (!o.reseed) continue;
      const PPResult pp = kmeans_pp_serial(X, d, nullptr, n, K, j0[r], u + (size_t)r * nu, kLloydMax, s.cen.data(),
                                           s.cold.data(), s.sums.data(), s.dw.data(), s.lw.data());
      status[r] = pp.status;
      if (pp.status != kOk) continue;
      std::copy(s.cen.begin(), s.cen.end(), centres + (size_t)r * K * d);
      iters[r] = pp.iters;
    }
    return 0;
  }
  if (n < 1 || d < 1 || K < 2 || R < 0) return -1;
  Pool pool;
  const double *dX = static_cast<const double *>(pool.put(X, (size_t)n * d * 8));
  const int *dj = static_cast<const int *>(pool.put(j0, (size_t)R * 4));
  const double *du = static_cast<const double *>(pool.put(u, (size_t)R * nu * 8));
  double *dc = static_cast<double *>(pool.put(centres, (size_t)R * K * d * 8));
  int *ds = static_cast<int *>(pool.put(status, (size_t)R * 4));
  int *di = static_cast<int *>(pool.put(iters, (size_t)R * 4));
  const size_t wb = vbhem_wtk_seed_tiled_workspace_bytes(n, d, K, R, chunk_trials);
  void *ws = pool.put(nullptr, std::max<size_t>(wb, 16));
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhem_wtk_seed_tiled_batch(n, d, K, R, dX, dj, du, chunk_trials, dc, ds, di, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(centres, dc, (size_t)R * K * d * 8);
  pool.get(status, ds, (size_t)R * 4);
  pool.get(iters, di, (size_t)R * 4);
  return (int)pool.e;
}

}  // extern "C"
