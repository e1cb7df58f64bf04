// vbhmm_hmmset.h -- the prepared set of point HMMs (vbhmm_score_hmms_t of
// include/vbhmm_score.h) that the scoring, PPK and CCFD kernels read: everything
// about it that does not depend on a feature's per-state arithmetic.
//
// A prepared buffer is kPrepHead doubles, then H blocks of `stride` doubles; what a
// block holds is the feature's own Layout (score::Layout, ppk::Layout).  The head's
// first two 32-bit words are flags, written by the prep kernel with atomicMin over
// kNoFlag: [0] the lowest (h KM + k) whose state was refused, [1] the lowest h whose
// state count is outside [1, KM].  prepare() sets both to kNoFlag before the launch
// and reads them back after it, so a buffer may be prepared again after a refusal.
//
// A prep kernel stays a __global__ in its feature's file and calls prep_lane with the
// feature's prepare_state; prepare() is the host sequence around its launch.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_score.h"
#include "vbhmm_score_pair.h"

namespace vbhem {
namespace hmmset {

constexpr int kPrepHead = 8;  // doubles before the blocks: [0] two unsigned flags
constexpr unsigned kNoFlag = 0xFFFFFFFFu;

inline unsigned *flags(void *prepared) { return static_cast<unsigned *>(prepared); }
inline double *blocks(void *prepared) { return static_cast<double *>(prepared) + kPrepHead; }
inline const double *blocks(const void *prepared) { return static_cast<const double *>(prepared) + kPrepHead; }

// the two ends of a prep kernel's argument block (the feature's Layout and
// parameters go between them)
struct Dims {
  int H, KM, d, diag;
};
struct Arrays {
  const int *nstates;
  const double *prior, *trans, *mean, *cov;
  unsigned *flags;
  double *blocks;
};

// state k of HMM h as prepare_state takes it: the HMM's block and its own arrays
struct State {
  double *blk;
  int k, K;
  const double *prior, *trans, *mean, *cov;
};

// One lane of a prep kernel of `threads` lanes per workgroup: state (h, k) of the
// global index.  A state count outside [1, KM] is flagged and clamped before
// anything is read with it; prep(State) == false flags the state.
template <class F>
__device__ inline void prep_lane(const Dims &n, int stride, const Arrays &a, int threads, F prep) {
  const long long g = (long long)blockIdx.x * threads + threadIdx.x;
  if (g >= (long long)n.H * n.KM) return;
  const int h = (int)(g / n.KM), k = (int)(g % n.KM), KM = n.KM, d = n.d;
  int K = a.nstates[h];
  if (K < 1 || K > KM) {
    atomicMin(&a.flags[1], (unsigned)h);
    K = K < 1 ? 0 : KM;
  }
  const size_t cs = n.diag ? (size_t)d : (size_t)d * d;
  const State s{a.blocks + (size_t)h * stride, k, K, a.prior + (size_t)h * KM, a.trans + (size_t)h * KM * KM,
                a.mean + (size_t)h * KM * d, a.cov + (size_t)h * KM * cs};
  if (!prep(s)) atomicMin(&a.flags[0], (unsigned)g);
}

// The cooperative copy of one HMM's block into LDS by a workgroup of `threads`
// lanes.  The barrier before the first read of sh is the caller's.
__device__ inline void stage_block(double *sh, const double *blk, int len, int threads) {
  for (int q = threadIdx.x; q < len; q += threads) sh[q] = blk[q];
}

static inline int check_set(const vbhmm_score_hmms_t *m, const char *who) {
  if (!m) return set_error(VBHEM_ERR_ARG, "null HMM set");
  if (m->H < 0 || m->KM < 1 || m->dim < 1 || (m->covmode != VBHEM_COV_DIAG && m->covmode != VBHEM_COV_FULL))
    return set_error(VBHEM_ERR_ARG, "invalid HMM set (need H>=0, KM>=1, dim>=1, covmode diag or full)");
  if (m->KM > score::kMaxStates || m->dim > score::kMaxDim)
    return set_error(VBHEM_ERR_UNSUPPORTED, std::string(who) + ": at most 16 states and 8 dimensions supported");
  return VBHEM_OK;
}

static inline int check_seqs(const vbhmm_score_hmms_t *m, const vbhmm_seqs_t *s) {
  if (!s) return set_error(VBHEM_ERR_ARG, "null sequences");
  if (s->N < 0 || s->dim != m->dim) return set_error(VBHEM_ERR_ARG, "invalid sequences (need N>=0, the HMMs' dim)");
  if (s->N > 0 && (!s->offsets || !s->x)) return set_error(VBHEM_ERR_ARG, "null sequence array");
  return VBHEM_OK;
}

// bytes of the prepared buffer of a set whose blocks are `stride(KM, dim)` doubles;
// 0 for a set no buffer can be sized for
template <class Stride>
inline size_t prepared_bytes(const vbhmm_score_hmms_t *m, Stride stride) {
  if (!m || m->H < 0 || m->KM < 1 || m->KM > score::kMaxStates || m->dim < 1 || m->dim > score::kMaxDim) return 0;
  return ((size_t)kPrepHead + (size_t)m->H * stride(m->KM, m->dim)) * sizeof(double);
}

inline unsigned prep_grid(const Dims &n, int threads) {
  return (unsigned)(((long long)n.H * n.KM + threads - 1) / threads);
}

// The prepare sequence of a set that passed check_set: `need` is its prepared_bytes,
// launch(Dims, Arrays) starts the feature's prep kernel `kernel` on st, `noun` is
// what a refused state's message calls its matrix.  Synchronises st.
template <class Launch>
inline int prepare(const vbhmm_score_hmms_t *m, void *prepared, size_t bytes, size_t need, hipStream_t st,
                   const char *kernel, const char *noun, Launch launch) {
  if (!prepared || bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "prepared buffer too small: need " + std::to_string(need) + " bytes");
  if (m->H == 0) return VBHEM_OK;
  if (!m->nstates || !m->prior || !m->trans || !m->mean || !m->cov)
    return set_error(VBHEM_ERR_ARG, "null HMM array");
  hipError_t e = hipMemsetAsync(prepared, 0xFF, kPrepHead * sizeof(double), st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(flags)");
  launch(Dims{m->H, m->KM, m->dim, m->covmode == VBHEM_COV_DIAG},
         Arrays{m->nstates, m->prior, m->trans, m->mean, m->cov, flags(prepared), blocks(prepared)});
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, kernel);
  unsigned f[2] = {kNoFlag, kNoFlag};
  e = hipMemcpyAsync(f, prepared, sizeof(f), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, (std::string(kernel) + " (flags)").c_str());
  if (f[1] != kNoFlag)
    return set_error(VBHEM_ERR_ARG, "state count of HMM " + std::to_string(f[1]) + " is outside [1, KM]");
  if (f[0] != kNoFlag)
    return set_error(VBHEM_ERR_ARG, std::string(noun) + " of HMM " + std::to_string(f[0] / m->KM) + " state " +
                                        std::to_string(f[0] % m->KM) + " is not positive definite");
  return VBHEM_OK;
}

}  // namespace hmmset
}  // namespace vbhem
