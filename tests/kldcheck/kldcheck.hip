// tests/kldcheck/kldcheck.hip -- TEST-ONLY exports of the KL-job planner
// (csrc/vbhmm_kld_plan.h): the plan's counts and its refusals, a host walk of the planned
// tiles with the routines the kernels call (tests/checklib/kld_walk.h), so planner and
// arithmetic are checked on a machine without a GPU, and the same call through the
// library's kernels on device 0.  Arrays are host arrays in the layouts of
// include/vbhmm_score.h and include/vbhmm_kld.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "device_pool.h"
#include "host_prepare.h"
#include "kld_walk.h"
#include "vbhmm_kld.h"

namespace {

using checklib::Pool;
using vbhem::kld::Plan;

void copy_message(const std::string &s, char *msg, int msg_len) {
  if (!msg || msg_len < 1) return;
  std::strncpy(msg, s.c_str(), (size_t)msg_len - 1);
  msg[msg_len - 1] = 0;
}

}  // namespace

extern "C" {

// The planner alone.  counts [6]: own slots, own tiles, (job, item) lanes, cross tiles,
// the most passes of a tile, workspace bytes.  Returns the planner's status; msg gets
// its message.
int kldcheck_plan(int H, int N, int n_lists, const int *list_offsets, const int *list_items, int n_jobs,
                  const int *jobs, long long *counts, char *msg, int msg_len) {
  Plan p;
  const int rc = vbhem::kld::make_plan(H, N, n_lists, list_offsets, list_items, n_jobs, jobs, p);
  copy_message(p.error, msg, msg_len);
  if (rc != VBHEM_OK) return rc;
  long long passes = 0;
  for (const auto &t : p.cross_tiles) passes = std::max(passes, (long long)(t.y + vbhem::kld::kLanes - 1) / vbhem::kld::kLanes);
  counts[0] = p.own_len;
  counts[1] = (long long)p.own_tiles.size();
  counts[2] = p.n_lanes;
  counts[3] = (long long)p.cross_tiles.size();
  counts[4] = passes;
  counts[5] = (long long)vbhem::kld::ws_layout(p).total;
  return rc;
}

// kl [n_jobs] by the host walk of the planned tiles; own_hits [own slots] and pair_hits
// [(job, item) in the caller's job order] count the writes and visits.  The planner's
// status (msg: its message), or 1 + (h KM + k) of a covariance that is not positive definite.
long long kldcheck_jobs_host(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                             const double *trans, const double *mean, const double *cov, int N, const int *offsets,
                             const double *x, int n_lists, const int *list_offsets, const int *list_items,
                             int n_jobs, const int *jobs, double *kl, int *own_hits, int *pair_hits, char *msg,
                             int msg_len) {
  using namespace vbhem::score;
  Plan p;
  const int rc = vbhem::kld::make_plan(H, N, n_lists, list_offsets, list_items, n_jobs, jobs, p);
  copy_message(p.error, msg, msg_len);
  if (rc != VBHEM_OK || n_jobs == 0) return rc;
  const Layout L = make_layout(KM, d);
  std::vector<double> blocks;
  const long long bad = checklib::host_prepare(L, H, KM, d, covmode, nstates, prior, trans, mean, cov, blocks);
  if (bad) return bad;
  std::vector<int> first;
  kldwalk::pair_firsts(n_jobs, jobs, list_offsets, first);
  return dispatch(KM, d, kldwalk::Walk{L, blocks, d, covmode == VBHEM_COV_DIAG, offsets, x, p, first.data(), kl,
                                       own_hits, pair_hits});
}

// The same through vbhmm_score_prepare / vbhmm_kld_jobs on device 0.  Returns the
// library's status, or a positive hipError_t of the copies.
int kldcheck_jobs_device(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                         const double *trans, const double *mean, const double *cov, int N, const int *offsets,
                         const double *x, int n_lists, const int *list_offsets, const int *list_items, int n_jobs,
                         const int *jobs, double *kl) {
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
  const size_t pb = vbhmm_score_prepared_bytes(&m);
  const size_t wb = vbhmm_kld_jobs_workspace_bytes(n_lists, list_offsets, n_jobs, jobs);
  void *prep = pool.put(nullptr, pb), *ws = pool.put(nullptr, wb);
  double *dkl = static_cast<double *>(pool.put(nullptr, (size_t)n_jobs * 8));
  if (pool.e != hipSuccess) return (int)pool.e;
  int rc = vbhmm_score_prepare(&m, prep, pb, nullptr);
  if (rc == 0)
    rc = vbhmm_kld_jobs(&m, prep, &s, n_lists, list_offsets, list_items, n_jobs, jobs, ws, wb, dkl, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(kl, dkl, (size_t)n_jobs * 8);
  return (int)pool.e;
}

}  // extern "C"
