// tests/scorecheck/scorecheck.hip -- TEST-ONLY exports of the sequence-scoring
// arithmetic (csrc/vbhmm_score_pair.h): a host loop over (HMM, sequence) pairs
// calling the routines the kernels call, so the logic is checked on a machine
// without a GPU, and the same call through the library's kernels on device 0.
// Arrays are host arrays in the layouts of include/vbhmm_score.h.
#include <hip/hip_runtime.h>

#include <vector>

#include "device_pool.h"
#include "host_prepare.h"
#include "vbhmm_score.h"
#include "vbhmm_score_pair.h"

namespace {

using namespace vbhem::score;

struct HostPairs {
  const Layout &L;
  const std::vector<double> &blocks;
  int H, N, d;
  bool diag;
  const int *offsets;
  const double *x;
  long long total;
  double *ll, *vll;
  int *path;
  template <int KB, int DB>
  int operator()() const {
    std::vector<uint32_t> bp((size_t)(total + 1) * KB / 4 + 1);
    for (int h = 0; h < H; ++h) {
      const Hmm m = view(L, blocks.data() + (size_t)h * L.stride, diag);
      for (int n = 0; n < N; ++n) {
        const int off = offsets[n], T = offsets[n + 1] - off;
        const double *xn = x + (size_t)off * d;
        ll[(size_t)h * N + n] = pair_loglik<KB, DB>(m, xn, T, d);
        vll[(size_t)h * N + n] =
            pair_viterbi<KB, DB>(m, xn, T, d, reinterpret_cast<unsigned char *>(bp.data()),
                                 path + (size_t)h * total + off);
      }
    }
    return 0;
  }
};

}  // namespace

extern "C" {

// 0, or 1 + (h KM + k) of the first covariance that is not positive definite.
// ll / vll [H][N], path [H][total] (total = offsets[N]).
long long scorecheck_host(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                          const double *trans, const double *mean, const double *cov, int N,
                          const int *offsets, const double *x, double *ll, double *vll, int *path) {
  const Layout L = make_layout(KM, d);
  std::vector<double> blocks;
  const long long bad = checklib::host_prepare(L, H, KM, d, covmode, nstates, prior, trans, mean, cov, blocks);
  if (bad) return bad;
  const long long total = N > 0 ? offsets[N] : 0;
  return dispatch(KM, d,
                  HostPairs{L, blocks, H, N, d, covmode == VBHEM_COV_DIAG, offsets, x, total, ll, vll, path});
}

// The same through vbhmm_score_prepare / _ll / _viterbi on device 0.  Returns the
// library's status, or a positive hipError_t of the copies.
int scorecheck_device(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                      const double *trans, const double *mean, const double *cov, int N,
                      const int *offsets, const double *x, double *ll, double *vll, int *path) {
  const size_t cs = covmode == VBHEM_COV_DIAG ? (size_t)d : (size_t)d * d;
  const long long total = N > 0 ? offsets[N] : 0;
  checklib::Pool pool;
  vbhmm_score_hmms_t m = {H, KM, d, covmode,
                          static_cast<const int *>(pool.put(nstates, (size_t)H * sizeof(int))),
                          static_cast<const double *>(pool.put(prior, (size_t)H * KM * 8)),
                          static_cast<const double *>(pool.put(trans, (size_t)H * KM * KM * 8)),
                          static_cast<const double *>(pool.put(mean, (size_t)H * KM * d * 8)),
                          static_cast<const double *>(pool.put(cov, (size_t)H * KM * cs * 8))};
  vbhmm_seqs_t s = {N, d, 0, static_cast<const int *>(pool.put(offsets, (size_t)(N + 1) * sizeof(int))),
                    static_cast<const double *>(pool.put(x, (size_t)total * d * 8))};
  const size_t pb = vbhmm_score_prepared_bytes(&m), wb = vbhmm_score_workspace_bytes(&m, total);
  void *prep = pool.put(nullptr, pb), *ws = pool.put(nullptr, wb);
  double *dll = static_cast<double *>(pool.put(nullptr, (size_t)H * N * 8));
  double *dvll = static_cast<double *>(pool.put(nullptr, (size_t)H * N * 8));
  int *dpath = static_cast<int *>(pool.put(nullptr, (size_t)H * total * sizeof(int)));
  if (pool.e != hipSuccess) return (int)pool.e;
  int rc = vbhmm_score_prepare(&m, prep, pb, nullptr);
  if (rc == 0) rc = vbhmm_score_ll(&m, prep, &s, dll, nullptr);
  if (rc == 0) rc = vbhmm_score_viterbi(&m, prep, &s, total, dpath, dvll, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(ll, dll, (size_t)H * N * 8);
  pool.get(vll, dvll, (size_t)H * N * 8);
  pool.get(path, dpath, (size_t)H * total * sizeof(int));
  return (int)pool.e;
}

}  // extern "C"
