// tests/scorecheck/scorecheck.hip -- TEST-ONLY exports of the sequence-scoring
// arithmetic (csrc/vbhmm_score_pair.h): a host loop over (HMM, sequence) pairs
// calling the routines the kernels call, so the logic is checked on a machine
// without a GPU, and the same call through the library's kernels on device 0.
// Arrays are host arrays in the layouts of include/vbhmm_score.h.
#include <hip/hip_runtime.h>

#include <vector>

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
  const bool diag = covmode == VBHEM_COV_DIAG;
  const size_t cs = diag ? (size_t)d : (size_t)d * d;
  std::vector<double> blocks((size_t)H * L.stride, 0.0);
  long long bad = 0;
  for (int h = 0; h < H; ++h)
    for (int k = 0; k < KM; ++k)
      if (!prepare_state(L, blocks.data() + (size_t)h * L.stride, k, nstates[h], d, diag,
                         prior + (size_t)h * KM, trans + (size_t)h * KM * KM,
                         mean + (size_t)h * KM * d, cov + (size_t)h * KM * cs) &&
          !bad)
        bad = 1 + (long long)h * KM + k;
  if (bad) return bad;
  const long long total = N > 0 ? offsets[N] : 0;
  return dispatch(KM, d, HostPairs{L, blocks, H, N, d, diag, offsets, x, total, ll, vll, path});
}

// The same through vbhmm_score_prepare / _ll / _viterbi on device 0.  Returns the
// library's status, or a positive hipError_t of the copies.
int scorecheck_device(int H, int KM, int d, int covmode, const int *nstates, const double *prior,
                      const double *trans, const double *mean, const double *cov, int N,
                      const int *offsets, const double *x, double *ll, double *vll, int *path) {
  const bool diag = covmode == VBHEM_COV_DIAG;
  const size_t cs = diag ? (size_t)d : (size_t)d * d;
  const long long total = N > 0 ? offsets[N] : 0;
  vbhmm_score_hmms_t m = {H, KM, d, covmode, nullptr, nullptr, nullptr, nullptr, nullptr};
  vbhmm_seqs_t s = {N, d, 0, nullptr, nullptr};
  const size_t pb = vbhmm_score_prepared_bytes(&m), wb = vbhmm_score_workspace_bytes(&m, total);
  const size_t in_bytes[] = {(size_t)H * sizeof(int), (size_t)H * KM * 8, (size_t)H * KM * KM * 8,
                             (size_t)H * KM * d * 8, (size_t)H * KM * cs * 8,
                             (size_t)(N + 1) * sizeof(int), (size_t)total * d * 8};
  const void *in_host[] = {nstates, prior, trans, mean, cov, offsets, x};
  const size_t out_bytes[] = {(size_t)H * N * 8, (size_t)H * N * 8, (size_t)H * total * sizeof(int)};
  void *out_host[] = {ll, vll, path};
  void *din[7] = {nullptr}, *dout[3] = {nullptr}, *prep = nullptr, *ws = nullptr;
  hipError_t e = hipSuccess;
  int rc = 0;
  for (int q = 0; q < 7 && e == hipSuccess; ++q) {
    e = hipMalloc(&din[q], in_bytes[q] + 8);
    if (e == hipSuccess && in_bytes[q]) e = hipMemcpy(din[q], in_host[q], in_bytes[q], hipMemcpyHostToDevice);
  }
  for (int q = 0; q < 3 && e == hipSuccess; ++q) e = hipMalloc(&dout[q], out_bytes[q] + 8);
  if (e == hipSuccess) e = hipMalloc(&prep, pb + 8);
  if (e == hipSuccess) e = hipMalloc(&ws, wb + 8);
  if (e == hipSuccess) {
    m.nstates = static_cast<const int *>(din[0]);
    m.prior = static_cast<const double *>(din[1]);
    m.trans = static_cast<const double *>(din[2]);
    m.mean = static_cast<const double *>(din[3]);
    m.cov = static_cast<const double *>(din[4]);
    s.offsets = static_cast<const int *>(din[5]);
    s.x = static_cast<const double *>(din[6]);
    rc = vbhmm_score_prepare(&m, prep, pb, nullptr);
    if (rc == 0) rc = vbhmm_score_ll(&m, prep, &s, static_cast<double *>(dout[0]), nullptr);
    if (rc == 0)
      rc = vbhmm_score_viterbi(&m, prep, &s, total, static_cast<int *>(dout[2]),
                               static_cast<double *>(dout[1]), ws, wb, nullptr);
    if (rc == 0) e = hipDeviceSynchronize();
  }
  for (int q = 0; q < 3 && e == hipSuccess && rc == 0; ++q)
    if (out_bytes[q]) e = hipMemcpy(out_host[q], dout[q], out_bytes[q], hipMemcpyDeviceToHost);
  for (void *p : din) (void)hipFree(p);
  for (void *p : dout) (void)hipFree(p);
  (void)hipFree(prep);
  (void)hipFree(ws);
  return rc != 0 ? rc : (int)e;
}

}  // extern "C"
