// vbhmm_score.hip -- scoring sequences under point HMMs (include/vbhmm_score.h):
// the log-likelihood of src/hmm/vbhmm_ll.m:40-116 and the Viterbi path of
// src/hmm/vbhmm_map_state.m:28-103 for every (HMM, sequence) pair of a set of H
// HMMs and a ragged batch of N sequences.
//
// The scheme of vbhmm_fb_kernel (vbhmm_fb.hip): one lane per pair, the recursion's
// state vector in registers (state-count buckets 4 / 8 / 16, dimension buckets
// 2 / 4 / 8 as template parameters, so every loop unrolls and nothing is indexed
// dynamically), the HMM's prepared block staged once per workgroup in LDS and read
// as broadcasts.  A workgroup covers kScoreThreads consecutive sequences of one
// HMM; the grid is (sequence tiles x H), linearised (H may exceed the y limit).
// loglik[h][n] is stored by consecutive lanes at consecutive addresses.  The
// per-pair arithmetic is vbhmm_score_pair.h, shared with the host check build.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_hmmset.h"
#include "vbhmm_score.h"
#include "vbhmm_score_pair.h"

namespace vbhem {
namespace {

using namespace score;

constexpr int kScoreThreads = 128;
constexpr int kPrepThreads = 256;
enum ScoreMode : int { kScoreLL = 0, kScoreViterbi = 1 };

struct PrepArgs {
  hmmset::Dims n;
  Layout L;
  hmmset::Arrays a;
};

__global__ __launch_bounds__(kPrepThreads) void hmm_score_prep_kernel(const PrepArgs p) {
  hmmset::prep_lane(p.n, p.L.stride, p.a, kPrepThreads, [&](const hmmset::State &s) {
    return prepare_state(p.L, s.blk, s.k, s.K, p.n.d, p.n.diag != 0, s.prior, s.trans, s.mean, s.cov);
  });
}

struct ScoreArgs {
  int H, N, d, diag, tiles;
  Layout L;
  const double *blocks;
  const int *offsets;
  const double *x;
  double *loglik;
  long long total;
  int *path;
  unsigned char *bp;
};

template <int KB, int DB, int MODE>
__global__ __launch_bounds__(kScoreThreads) void hmm_score_kernel(const ScoreArgs p) {
  __shared__ double sh[BlockLen<KB, DB>::value];
  const int h = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
  const double *blk = p.blocks + (size_t)h * p.L.stride;
  hmmset::stage_block(sh, blk, p.L.stride, kScoreThreads);
  __syncthreads();
  const int n = tile * kScoreThreads + threadIdx.x;
  if (n >= p.N) return;
  const Hmm m = view(p.L, sh, p.diag != 0);
  const int off = p.offsets[n], T = p.offsets[n + 1] - off;
  const double *xn = p.x + (size_t)off * p.d;
  double ll;
  if (MODE == kScoreLL) {
    ll = pair_loglik<KB, DB>(m, xn, T, p.d);
  } else {
    const size_t at = (size_t)h * p.total + off;
    ll = pair_viterbi<KB, DB>(m, xn, T, p.d, p.bp + at * KB, p.path + at);
  }
  p.loglik[(size_t)h * p.N + n] = ll;
}

template <int MODE>
struct Launch {
  const ScoreArgs &a;
  hipStream_t st;
  template <int KB, int DB>
  hipError_t operator()() const {
    static_assert(BlockLen<KB, DB>::value >= 2 * KB + KB * KB + KB * DB + KB * packed_len(DB) + 1, "LDS block");
    const unsigned grid = (unsigned)((long long)a.tiles * a.H);
    hipLaunchKernelGGL((hmm_score_kernel<KB, DB, MODE>), dim3(grid), dim3(kScoreThreads), 0, st, a);
    return hipGetLastError();
  }
};

// the set, the sequences and the (HMM, sequence tile) grid of a scoring call
int check_call(const vbhmm_score_hmms_t *m, const vbhmm_seqs_t *s, long long &tiles) {
  int rc = hmmset::check_set(m, "vbhmm_score");
  if (rc == VBHEM_OK) rc = hmmset::check_seqs(m, s);
  if (rc != VBHEM_OK) return rc;
  tiles = ((long long)s->N + kScoreThreads - 1) / kScoreThreads;
  if (tiles * m->H > INT_MAX)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_score: too many (HMM, sequence tile) workgroups; split the HMM set");
  return VBHEM_OK;
}

ScoreArgs score_args(const vbhmm_score_hmms_t *m, const void *prepared, const vbhmm_seqs_t *s,
                     long long tiles, double *loglik) {
  ScoreArgs a{};
  a.H = m->H; a.N = s->N; a.d = m->dim; a.diag = m->covmode == VBHEM_COV_DIAG; a.tiles = (int)tiles;
  a.L = make_layout(m->KM, m->dim);
  a.blocks = hmmset::blocks(prepared);
  a.offsets = s->offsets; a.x = s->x; a.loglik = loglik;
  return a;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_score_prepared_bytes(const vbhmm_score_hmms_t *m) {
  using namespace vbhem;
  return hmmset::prepared_bytes(m, [](int KM, int d) { return make_layout(KM, d).stride; });
}

int vbhmm_score_prepare(const vbhmm_score_hmms_t *m, void *prepared_dev, size_t prepared_bytes,
                        void *stream) {
  using namespace vbhem;
  const int rc = hmmset::check_set(m, "vbhmm_score");
  if (rc != VBHEM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return hmmset::prepare(m, prepared_dev, prepared_bytes, vbhmm_score_prepared_bytes(m), st,
                         "hmm_score_prep_kernel", "covariance",
                         [&](const hmmset::Dims &n, const hmmset::Arrays &arrays) {
                           const PrepArgs a{n, make_layout(n.KM, n.d), arrays};
                           hipLaunchKernelGGL(hmm_score_prep_kernel, dim3(hmmset::prep_grid(n, kPrepThreads)),
                                              dim3(kPrepThreads), 0, st, a);
                         });
}

size_t vbhmm_score_workspace_bytes(const vbhmm_score_hmms_t *m, long long total_steps) {
  using namespace vbhem;
  if (!m || m->H < 0 || m->KM < 1 || m->KM > kMaxStates || total_steps < 0) return 0;
  return (size_t)m->H * (size_t)total_steps * state_bucket(m->KM) + 256;
}

int vbhmm_score_ll(const vbhmm_score_hmms_t *m, const void *prepared_dev, const vbhmm_seqs_t *s,
                   double *loglik_dev, void *stream) {
  using namespace vbhem;
  long long tiles = 0;
  const int rc = check_call(m, s, tiles);
  if (rc != VBHEM_OK) return rc;
  if (m->H == 0 || s->N == 0) return VBHEM_OK;
  if (!prepared_dev || !loglik_dev) return set_error(VBHEM_ERR_ARG, "null prepared buffer or output");
  const ScoreArgs a = score_args(m, prepared_dev, s, tiles, loglik_dev);
  const hipError_t e = dispatch(m->KM, m->dim, Launch<kScoreLL>{a, static_cast<hipStream_t>(stream)});
  if (e != hipSuccess) return hip_fail(e, "hmm_score_kernel(ll)");
  return VBHEM_OK;
}

int vbhmm_score_viterbi(const vbhmm_score_hmms_t *m, const void *prepared_dev, const vbhmm_seqs_t *s,
                        long long total_steps, int *path_dev, double *loglik_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  long long tiles = 0;
  const int rc = check_call(m, s, tiles);
  if (rc != VBHEM_OK) return rc;
  if (total_steps < 0) return set_error(VBHEM_ERR_ARG, "total_steps must be >= 0");
  if (m->H == 0 || s->N == 0) return VBHEM_OK;
  if (!prepared_dev || !loglik_dev || !path_dev) return set_error(VBHEM_ERR_ARG, "null prepared buffer or output");
  const size_t need = vbhmm_score_workspace_bytes(m, total_steps);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace_dev) % 16)
    return set_error(VBHEM_ERR_ARG, "workspace must be 16-byte aligned");
  ScoreArgs a = score_args(m, prepared_dev, s, tiles, loglik_dev);
  a.total = total_steps;
  a.path = path_dev;
  a.bp = static_cast<unsigned char *>(workspace_dev);
  const hipError_t e = dispatch(m->KM, m->dim, Launch<kScoreViterbi>{a, static_cast<hipStream_t>(stream)});
  if (e != hipSuccess) return hip_fail(e, "hmm_score_kernel(viterbi)");
  return VBHEM_OK;
}

}  // extern "C"
