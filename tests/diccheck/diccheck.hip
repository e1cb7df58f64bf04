// tests/diccheck/diccheck.hip -- TEST-ONLY exports of the DIC likelihood: host loops over
// the pair routine the kernel calls (csrc/vbhmm_dic_pair.h), so the arithmetic is checked
// on a machine without a GPU, and the same call through the library's kernels on device 0.
// Arrays are host arrays in the layouts of include/vbhem_estep.h (base set, diag) and
// include/vbhmm_dic.h (models).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "device_pool.h"
#include "vbhmm_dic.h"
#include "vbhmm_dic_pair.h"

namespace {

using namespace vbhem::dic;

using checklib::Pool;

template <int SP>
void host_pairs(int N, int SB, int d, const int *nstates, const double *prior, const double *A,
                const double *centres, const double *covars, int C, int S, const int *nstates_r,
                const double *logA, const double *logPi, const double *m, const double *P, const double *c,
                int T, int exact_only, double *L, int *recomputed) {
  std::vector<double> blk((size_t)block_len(SP, d));
  for (int j = 0; j < C; ++j) {
    const size_t cs = (size_t)j * S;
    prepare_block(blk.data(), SP, d, nstates_r[j], S, logA + cs * S, logPi + cs, c + cs, m + cs * d, P + cs * d);
    const Cluster k = view_block(blk.data(), SP, d, logA + cs * S, S);
    for (int i = 0; i < N; ++i) {
      const size_t b0 = (size_t)i * SB;
      L[(size_t)i * C + j] = pair_serial<SP>(k, nstates[i], SB, prior + b0, A + b0 * SB, centres + b0 * d,
                                             covars + b0 * d, T, exact_only != 0, recomputed);
    }
  }
}

}  // namespace

extern "C" {

// L [N][C] by pair_serial; *recomputed: the pairs redone in reference order.
// -2: outside the routine's limits.
int diccheck_pairs_host(int N, int SB, int d, const int *nstates, const double *prior, const double *A,
                        const double *centres, const double *covars, int C, int S, const int *nstates_r,
                        const double *logA, const double *logPi, const double *m, const double *P,
                        const double *c, int T, int exact_only, double *L, int *recomputed) {
  if (SB > kMaxStates || S > kMaxStates || d > kMaxDim) return -2;
  *recomputed = 0;
  const int SP = state_bucket(S);
  if (SP == 4)
    host_pairs<4>(N, SB, d, nstates, prior, A, centres, covars, C, S, nstates_r, logA, logPi, m, P, c, T,
                  exact_only, L, recomputed);
  else if (SP == 8)
    host_pairs<8>(N, SB, d, nstates, prior, A, centres, covars, C, S, nstates_r, logA, logPi, m, P, c, T,
                  exact_only, L, recomputed);
  else
    host_pairs<16>(N, SB, d, nstates, prior, A, centres, covars, C, S, nstates_r, logA, logPi, m, P, c, T,
                   exact_only, L, recomputed);
  return 0;
}

// LL [G] from L [N][C]: the mixture terms, their LSE and the sum over bases in index order.
void diccheck_mix_host(int N, int C, int G, const int *model_off, const double *logw, const double *scale,
                       const double *L, double *LL) {
  std::vector<double> val;
  for (int g = 0; g < G; ++g) {
    const int c0 = model_off[g], K = model_off[g + 1] - c0;
    val.assign((size_t)K, 0.0);
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
      for (int j = 0; j < K; ++j) val[j] = mixture_term(logw[c0 + j], scale[g], L[(size_t)i * C + c0 + j]);
      sum += mixture_lse(val.data(), K, 1);
    }
    LL[g] = sum;
  }
}

size_t diccheck_workspace_bytes(int N, int SB, int d, int covmode, int G, int C, int S, int maxK, int T) {
  vbhem_base_t b = {N, SB, d, covmode, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  vbhmm_dic_models_t m = {G, C, S, d, maxK, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  return vbhmm_dic_workspace_bytes(&b, &m, T);
}

// vbhmm_dic_loglik on device 0: LL [G], L [N][C] (or NULL).  Returns the library's status,
// or a positive hipError_t of the copies.  covars is [N][SB][d] (diag) or [N][SB][d][d].
int diccheck_loglik_device(int N, int SB, int d, int covmode, const int *nstates, const double *prior,
                           const double *A, const double *centres, const double *covars, int G, int C, int S,
                           int maxK, const int *model_off, const int *nstates_r, const double *logw,
                           const double *scale, const double *logA, const double *logPi, const double *m,
                           const double *P, const double *c, int T, double *LL, double *L) {
  Pool pool;
  const size_t cv = covmode == VBHEM_COV_DIAG ? (size_t)d : (size_t)d * d;
  vbhem_base_t b = {N, SB, d, covmode,
                    static_cast<const int *>(pool.put(nstates, (size_t)N * sizeof(int))),
                    static_cast<const double *>(pool.put(prior, (size_t)N * SB * 8)),
                    static_cast<const double *>(pool.put(A, (size_t)N * SB * SB * 8)),
                    static_cast<const double *>(pool.put(centres, (size_t)N * SB * d * 8)),
                    static_cast<const double *>(pool.put(covars, (size_t)N * SB * cv * 8)), nullptr};
  vbhmm_dic_models_t md = {G, C, S, d, maxK,
                           static_cast<const int *>(pool.put(model_off, (size_t)(G + 1) * sizeof(int))),
                           static_cast<const int *>(pool.put(nstates_r, (size_t)C * sizeof(int))),
                           static_cast<const double *>(pool.put(logw, (size_t)C * 8)),
                           static_cast<const double *>(pool.put(scale, (size_t)G * 8)),
                           static_cast<const double *>(pool.put(logA, (size_t)C * S * S * 8)),
                           static_cast<const double *>(pool.put(logPi, (size_t)C * S * 8)),
                           static_cast<const double *>(pool.put(m, (size_t)C * S * d * 8)),
                           static_cast<const double *>(pool.put(P, (size_t)C * S * d * 8)),
                           static_cast<const double *>(pool.put(c, (size_t)C * S * 8))};
  const size_t wb = vbhmm_dic_workspace_bytes(&b, &md, T);
  void *ws = pool.put(nullptr, wb);
  double *dLL = static_cast<double *>(pool.put(nullptr, (size_t)G * 8));
  double *dL = L ? static_cast<double *>(pool.put(nullptr, (size_t)N * C * 8)) : nullptr;
  if (pool.e != hipSuccess) return (int)pool.e;
  const int rc = vbhmm_dic_loglik(&b, &md, T, dLL, dL, ws, wb, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(LL, dLL, (size_t)G * 8);
  if (L) pool.get(L, dL, (size_t)N * C * 8);
  return (int)pool.e;
}

}  // extern "C"
