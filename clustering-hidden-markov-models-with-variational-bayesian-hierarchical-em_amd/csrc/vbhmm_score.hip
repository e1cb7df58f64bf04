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
#include "vbhmm_score.h"
#include "vbhmm_score_pair.h"

namespace vbhem {
namespace {

using namespace score;

constexpr int kScoreThreads = 128;
constexpr int kPrepThreads = 256;
constexpr int kPrepHead = 8;  // doubles before the blocks: [0] two unsigned flags
constexpr unsigned kNoFlag = 0xFFFFFFFFu;
enum ScoreMode : int { kScoreLL = 0, kScoreViterbi = 1 };

struct PrepArgs {
  int H, KM, d, diag;
  Layout L;
  const int *nstates;
  const double *prior, *trans, *mean, *cov;
  unsigned *flags;  // [0] first (h KM + k) not positive definite, [1] first h with a bad state count
  double *blocks;
};

__global__ __launch_bounds__(kPrepThreads) void hmm_score_prep_kernel(const PrepArgs p) {
  const long long g = (long long)blockIdx.x * kPrepThreads + threadIdx.x;
  if (g >= (long long)p.H * p.KM) return;
  const int h = (int)(g / p.KM), k = (int)(g % p.KM), KM = p.KM, d = p.d;
  int K = p.nstates[h];
  if (K < 1 || K > KM) {
    atomicMin(&p.flags[1], (unsigned)h);
    K = K < 1 ? 0 : KM;
  }
  const size_t cs = p.diag ? (size_t)d : (size_t)d * d;
  const bool ok = prepare_state(p.L, p.blocks + (size_t)h * p.L.stride, k, K, d, p.diag != 0,
                                p.prior + (size_t)h * KM, p.trans + (size_t)h * KM * KM,
                                p.mean + (size_t)h * KM * d, p.cov + (size_t)h * KM * cs);
  if (!ok) atomicMin(&p.flags[0], (unsigned)g);
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
  for (int q = threadIdx.x; q < p.L.stride; q += kScoreThreads) sh[q] = blk[q];
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

int check_hmms(const vbhmm_score_hmms_t *m) {
  if (!m) return set_error(VBHEM_ERR_ARG, "null HMM set");
  if (m->H < 0 || m->KM < 1 || m->dim < 1 ||
      (m->covmode != VBHEM_COV_DIAG && m->covmode != VBHEM_COV_FULL))
    return set_error(VBHEM_ERR_ARG, "invalid HMM set (need H>=0, KM>=1, dim>=1, covmode diag or full)");
  if (m->KM > kMaxStates || m->dim > kMaxDim)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_score: at most 16 states and 8 dimensions supported");
  return VBHEM_OK;
}

int check_seqs(const vbhmm_score_hmms_t *m, const vbhmm_seqs_t *s, long long &tiles) {
  if (!s) return set_error(VBHEM_ERR_ARG, "null sequences");
  if (s->N < 0 || s->dim != m->dim) return set_error(VBHEM_ERR_ARG, "invalid sequences (need N>=0, the HMMs' dim)");
  if (s->N > 0 && (!s->offsets || !s->x)) return set_error(VBHEM_ERR_ARG, "null sequence array");
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
  a.blocks = static_cast<const double *>(prepared) + kPrepHead;
  a.offsets = s->offsets; a.x = s->x; a.loglik = loglik;
  return a;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_score_prepared_bytes(const vbhmm_score_hmms_t *m) {
  using namespace vbhem;
  if (!m || m->H < 0 || m->KM < 1 || m->KM > kMaxStates || m->dim < 1 || m->dim > kMaxDim) return 0;
  return ((size_t)kPrepHead + (size_t)m->H * make_layout(m->KM, m->dim).stride) * sizeof(double);
}

int vbhmm_score_prepare(const vbhmm_score_hmms_t *m, void *prepared_dev, size_t prepared_bytes,
                        void *stream) {
  using namespace vbhem;
  int rc = check_hmms(m);
  if (rc != VBHEM_OK) return rc;
  const size_t need = vbhmm_score_prepared_bytes(m);
  if (!prepared_dev || prepared_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "prepared buffer too small: need " + std::to_string(need) + " bytes");
  if (m->H == 0) return VBHEM_OK;
  if (!m->nstates || !m->prior || !m->trans || !m->mean || !m->cov)
    return set_error(VBHEM_ERR_ARG, "null HMM array");
  hipStream_t st = static_cast<hipStream_t>(stream);
  PrepArgs a{};
  a.H = m->H; a.KM = m->KM; a.d = m->dim; a.diag = m->covmode == VBHEM_COV_DIAG;
  a.L = make_layout(m->KM, m->dim);
  a.nstates = m->nstates; a.prior = m->prior; a.trans = m->trans; a.mean = m->mean; a.cov = m->cov;
  a.flags = static_cast<unsigned *>(prepared_dev);
  a.blocks = static_cast<double *>(prepared_dev) + kPrepHead;
  hipError_t e = hipMemsetAsync(prepared_dev, 0xFF, kPrepHead * sizeof(double), st);
  if (e != hipSuccess) return set_error(VBHEM_ERR_HIP, std::string("hipMemsetAsync(flags): ") + hipGetErrorString(e));
  const unsigned grid = (unsigned)(((long long)m->H * m->KM + kPrepThreads - 1) / kPrepThreads);
  hipLaunchKernelGGL(hmm_score_prep_kernel, dim3(grid), dim3(kPrepThreads), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return set_error(VBHEM_ERR_HIP, std::string("hmm_score_prep_kernel: ") + hipGetErrorString(e));
  unsigned flags[2] = {kNoFlag, kNoFlag};
  e = hipMemcpyAsync(flags, prepared_dev, sizeof(flags), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error(VBHEM_ERR_HIP, std::string("hmm_score_prep_kernel (flags): ") + hipGetErrorString(e));
  if (flags[1] != kNoFlag)
    return set_error(VBHEM_ERR_ARG, "state count of HMM " + std::to_string(flags[1]) + " is outside [1, KM]");
  if (flags[0] != kNoFlag)
    return set_error(VBHEM_ERR_ARG, "covariance of HMM " + std::to_string(flags[0] / m->KM) + " state " +
                                        std::to_string(flags[0] % m->KM) + " is not positive definite");
  return VBHEM_OK;
}

size_t vbhmm_score_workspace_bytes(const vbhmm_score_hmms_t *m, long long total_steps) {
  using namespace vbhem;
  if (!m || m->H < 0 || m->KM < 1 || m->KM > kMaxStates || total_steps < 0) return 0;
  return (size_t)m->H * (size_t)total_steps * state_bucket(m->KM) + 256;
}

int vbhmm_score_ll(const vbhmm_score_hmms_t *m, const void *prepared_dev, const vbhmm_seqs_t *s,
                   double *loglik_dev, void *stream) {
  using namespace vbhem;
  int rc = check_hmms(m);
  long long tiles = 0;
  if (rc == VBHEM_OK) rc = check_seqs(m, s, tiles);
  if (rc != VBHEM_OK) return rc;
  if (m->H == 0 || s->N == 0) return VBHEM_OK;
  if (!prepared_dev || !loglik_dev) return set_error(VBHEM_ERR_ARG, "null prepared buffer or output");
  const ScoreArgs a = score_args(m, prepared_dev, s, tiles, loglik_dev);
  const hipError_t e = dispatch(m->KM, m->dim, Launch<kScoreLL>{a, static_cast<hipStream_t>(stream)});
  if (e != hipSuccess) return set_error(VBHEM_ERR_HIP, std::string("hmm_score_kernel(ll): ") + hipGetErrorString(e));
  return VBHEM_OK;
}

int vbhmm_score_viterbi(const vbhmm_score_hmms_t *m, const void *prepared_dev, const vbhmm_seqs_t *s,
                        long long total_steps, int *path_dev, double *loglik_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  int rc = check_hmms(m);
  long long tiles = 0;
  if (rc == VBHEM_OK) rc = check_seqs(m, s, tiles);
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
  if (e != hipSuccess) return set_error(VBHEM_ERR_HIP, std::string("hmm_score_kernel(viterbi): ") + hipGetErrorString(e));
  return VBHEM_OK;
}

}  // extern "C"
