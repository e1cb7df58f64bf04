// vbhmm_dic.hip -- the DIC likelihood of a grid of models (include/vbhmm_dic.h):
// LL[g] = sum_i LSE_{c in model g}(logw[c] + scale[g] L(i, c)) with L the VHEM expected
// log-likelihood of src/compare_mtds/dic/myDIC.m:160-170, backward sweep and termination
// only.  The arithmetic of a pair is vbhmm_dic_pair.h, shared with the host check build.
//
// Three launches:
//   dic_prep_kernel    a thread per cluster: the cluster's block [S | A' | amax | logPi |
//                      c | m | P] (A' = exp(logA - amax), rows padded to the state bucket)
//                      into the workspace.
//   dic_kernel<SP,SBP> a workgroup of 256 lanes per (tile of 64 bases, model).  A lane owns
//                      one base-state column of a pair (sigma / rho in registers, SP = the
//                      cluster state bucket); the SBP lanes of a base sit side by side in a
//                      wave and mix their columns with Ab by shuffles.  64 SBP / 256
//                      sub-tiles are taken one after the other.  The workgroup walks the
//                      model's clusters: the current block is read from LDS while every lane
//                      holds its share of the next one in registers and stores it after the
//                      pair is done (two buffers, one barrier per cluster).  Each base's
//                      logw + scale L goes to LDS [cluster][base]; after the last cluster a
//                      lane per base takes the mixture LSE (max first, sum in cluster order)
//                      and lane 0 adds the tile's bases in index order: one partial per
//                      (tile, model).
//                      A wave in which a pair's Z fell below kZMin runs the sweep again in
//                      reference order, and the lanes of that pair take its result.
//   dic_reduce_kernel  a workgroup per model: lane t adds the partials of tiles t, t + 256,
//                      ..., lane 0 the 256 sums in lane order.
// The tiling depends on N alone, so LL[g] does not depend on what else is in the grid.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_dic.h"
#include "vbhmm_dic_pair.h"

namespace vbhem {
namespace {

using namespace dic;

constexpr int kThreads = 256;
constexpr int kTile = 64;  // bases per (tile, model) partial

struct DicArgs {
  int N, SB, d, T, G, C, S, blen;
  const int *nstates;
  const double *prior, *A, *centres, *covars;
  const int *model_off, *nstates_r;
  const double *logw, *scale, *logA, *logPi, *m, *P, *c;
  double *blocks, *partial, *LL, *L_pairs;
  int ntiles;
};

__global__ __launch_bounds__(64) void dic_prep_kernel(const DicArgs p, int SP) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= p.C) return;
  int n = p.nstates_r[c];
  n = n < 1 ? 1 : n > p.S ? p.S : n;
  const size_t cs = (size_t)c * p.S;
  prepare_block(p.blocks + (size_t)c * p.blen, SP, p.d, n, p.S, p.logA + cs * p.S, p.logPi + cs,
                p.c + cs, p.m + cs * p.d, p.P + cs * p.d);
}

// L'[gamma, rho] = sum_beta Ab[gamma, beta] s(rho, beta) for the lane's own gamma: the SBP lanes
// of a base hold its columns side by side, beta ascending; S (uniform) own cluster states, Sb
// own base states.  Every lane of the wave must be here.
template <int SP, int SBP>
__device__ __forceinline__ void mix_columns(int S, int Sb, const double (&Abrow)[SBP], const double (&s)[SP],
                                            double (&L)[SP]) {
#pragma unroll
  for (int r = 0; r < SP; ++r) {
    double acc = 0.0;
    if (r < S) {
#pragma unroll
      for (int b = 0; b < SBP; ++b) {
        const double sv = __shfl(s[r], b, SBP);
        acc = b < Sb ? fma(Abrow[b], sv, acc) : acc;
      }
    }
    L[r] = acc;
  }
}

template <int SP, int SBP>
__global__ __launch_bounds__(kThreads) void dic_kernel(const DicArgs p) {
  constexpr int BL = block_len(SP, kMaxDim);
  constexpr int NPF = (BL + kThreads - 1) / kThreads;
  constexpr int BPS = kThreads / SBP;  // bases per sub-tile
  constexpr int NSUB = kTile / BPS;
  __shared__ double cst[2][BL];
  __shared__ double val[kMaxModelClusters][kTile];
  __shared__ double res[kTile];
  const int tid = threadIdx.x, tile = blockIdx.x, g = blockIdx.y;
  const int c0 = p.model_off[g], K = p.model_off[g + 1] - c0;
  if (K < 1 || K > kMaxModelClusters || c0 < 0 || c0 + K > p.C) {
    if (tid == 0) p.partial[(size_t)tile * p.G + g] = NAN;
    return;
  }
  const double scale = p.scale[g];
  const int blen = p.blen, d = p.d, SB = p.SB;
  const int beta = tid & (SBP - 1);
  const unsigned long long grp = ((SBP == 64 ? 0ull : (1ull << SBP)) - 1ull) << ((tid & 63) & ~(SBP - 1));

  for (int sub = 0; sub < NSUB; ++sub) {
    const int bl = sub * BPS + tid / SBP;
    const int i = tile * kTile + bl;
    const bool inb = i < p.N;
    const int ii = inb ? i : p.N - 1;
    int Sb = inb ? p.nstates[ii] : 0;
    Sb = Sb < 0 ? 0 : Sb > SB ? SB : Sb;
    const bool live = beta < Sb;
    const size_t col = (size_t)ii * SB + (live ? beta : 0);
    double Abrow[SBP];
#pragma unroll
    for (int q = 0; q < SBP; ++q) Abrow[q] = (live && q < Sb) ? p.A[col * SB + q] : 0.0;
    const double pi = live ? p.prior[col] : 0.0;
    const double *mu = p.centres + col * d, *cov = p.covars + col * d;

    for (int q = tid; q < blen; q += kThreads) cst[0][q] = p.blocks[(size_t)c0 * blen + q];
    __syncthreads();

    for (int j = 0; j < K; ++j) {
      double pf[NPF];
      if (j + 1 < K) {
        const double *nxt = p.blocks + (size_t)(c0 + j + 1) * blen;
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
          const int q = tid + u * kThreads;
          pf[u] = q < blen ? nxt[q] : 0.0;
        }
      }
      Cluster k = view_block(cst[j & 1], SP, d, p.logA + (size_t)(c0 + j) * p.S * p.S, p.S);
      k.S = __builtin_amdgcn_readfirstlane(k.S);

      double E[SP], L[SP], s[SP];
      column_emission<SP>(k, mu, cov, E);
#pragma unroll
      for (int q = 0; q < SP; ++q) {
        E[q] = live ? E[q] : 0.0;
        L[q] = 0.0;
      }
      bool low = false;
      for (int t = p.T - 1; t >= 1; --t) {
        double v[SP];
#pragma unroll
        for (int q = 0; q < SP; ++q) v[q] = E[q] + L[q];
        low = column_step<SP>(k, v, s) || low;
        mix_columns<SP, SBP>(k.S, Sb, Abrow, s, L);
      }
      const unsigned long long bal = __ballot(low && live);
      if (bal != 0ull) {  // uniform over the wave: the sweep again, in reference order
        double L2[SP];
#pragma unroll
        for (int q = 0; q < SP; ++q) L2[q] = 0.0;
        for (int t = p.T - 1; t >= 1; --t) {
          column_step_exact<SP>(k, E, L2, s);
          mix_columns<SP, SBP>(k.S, Sb, Abrow, s, L2);
        }
        const bool redo = (bal & grp) != 0ull;
#pragma unroll
        for (int q = 0; q < SP; ++q) L[q] = redo ? L2[q] : L[q];
      }
      const double ls = column_term<SP>(k, E, L);
      const double term = live ? pi * ls : 0.0;
      double tot = 0.0;
#pragma unroll
      for (int b = 0; b < SBP; ++b) {
        const double x = __shfl(term, b, SBP);
        tot = b < Sb ? tot + x : tot;
      }
      if (beta == 0 && inb) {
        val[j][bl] = mixture_term(p.logw[c0 + j], scale, tot);
        if (p.L_pairs) p.L_pairs[(size_t)i * p.C + c0 + j] = tot;
      }
      if (j + 1 < K) {
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
          const int q = tid + u * kThreads;
          if (q < blen) cst[(j + 1) & 1][q] = pf[u];
        }
      }
      __syncthreads();
    }
  }
  if (tid < kTile) {
    const int i = tile * kTile + tid;
    res[tid] = i < p.N ? mixture_lse(&val[0][tid], K, kTile) : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int b = 0; b < kTile && tile * kTile + b < p.N; ++b) sum += res[b];
    p.partial[(size_t)tile * p.G + g] = sum;
  }
}

__global__ __launch_bounds__(kThreads) void dic_reduce_kernel(const DicArgs p) {
  __shared__ double part[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int t = tid; t < p.ntiles; t += kThreads) acc += p.partial[(size_t)t * p.G + g];
  part[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    const int n = p.ntiles < kThreads ? p.ntiles : kThreads;
    for (int t = 0; t < n; ++t) sum += part[t];
    p.LL[g] = sum;
  }
}

template <int SP>
hipError_t launch_sbp(const DicArgs &a, int SBP, dim3 grid, hipStream_t st) {
  if (SBP == 4)
    hipLaunchKernelGGL((dic_kernel<SP, 4>), grid, dim3(kThreads), 0, st, a);
  else if (SBP == 8)
    hipLaunchKernelGGL((dic_kernel<SP, 8>), grid, dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL((dic_kernel<SP, 16>), grid, dim3(kThreads), 0, st, a);
  return hipGetLastError();
}


struct WsLayout {
  size_t blocks, partial, total;
  int blen, ntiles;
};

// 0 on an unsupported or invalid pair of descriptors
int ws_layout(const vbhem_base_t *b, const vbhmm_dic_models_t *m, WsLayout &w) {
  if (!b || !m) return set_error(VBHEM_ERR_ARG, "vbhmm_dic: null descriptor");
  if (b->N < 1 || b->SB < 1 || b->d < 1 || m->G < 1 || m->C < 1 || m->S < 1 || m->d != b->d ||
      m->max_model_clusters < 1)
    return set_error(VBHEM_ERR_ARG,
                     "vbhmm_dic: need N, SB, d, G, C, S, max_model_clusters >= 1 and the base set's d");
  if (b->covmode != VBHEM_COV_DIAG)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_dic: diagonal covariances only");
  if (b->SB > kMaxStates || m->S > kMaxStates || b->d > kMaxDim)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_dic: at most 16 states (base and cluster) and 16 dimensions");
  if (m->max_model_clusters > kMaxModelClusters)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_dic: at most 64 clusters per model");
  if (m->G > 65535) return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_dic: at most 65535 models per call");
  w.blen = block_len(state_bucket(m->S), b->d);
  w.ntiles = (b->N + kTile - 1) / kTile;
  w.blocks = 0;
  w.partial = align_up((size_t)m->C * w.blen * sizeof(double), 16);
  w.total = w.partial + align_up((size_t)w.ntiles * m->G * sizeof(double), 16);
  return VBHEM_OK;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_dic_workspace_bytes(const vbhem_base_t *base, const vbhmm_dic_models_t *models, int T) {
  vbhem::WsLayout w;
  if (T < 1 || vbhem::ws_layout(base, models, w) != VBHEM_OK) return 0;
  return w.total;
}

int vbhmm_dic_loglik(const vbhem_base_t *b, const vbhmm_dic_models_t *m, int T, double *LL_dev,
                     double *L_pairs_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  WsLayout w;
  const int rc = ws_layout(b, m, w);
  if (rc != VBHEM_OK) return rc;
  if (T < 1) return set_error(VBHEM_ERR_ARG, "vbhmm_dic_loglik: need T >= 1");
  if (!b->nstates || !b->prior || !b->A || !b->centres || !b->covars || !m->model_off || !m->nstates_r ||
      !m->logw || !m->scale || !m->logA || !m->logPi || !m->m || !m->P || !m->c || !LL_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_dic_loglik: null array");
  if (!workspace_dev || workspace_bytes < w.total)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(w.total) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace_dev) % 16)
    return set_error(VBHEM_ERR_ARG, "workspace must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *ws = static_cast<char *>(workspace_dev);
  DicArgs a{};
  a.N = b->N; a.SB = b->SB; a.d = b->d; a.T = T; a.G = m->G; a.C = m->C; a.S = m->S; a.blen = w.blen;
  a.nstates = b->nstates; a.prior = b->prior; a.A = b->A; a.centres = b->centres; a.covars = b->covars;
  a.model_off = m->model_off; a.nstates_r = m->nstates_r;
  a.logw = m->logw; a.scale = m->scale; a.logA = m->logA; a.logPi = m->logPi; a.m = m->m; a.P = m->P; a.c = m->c;
  a.blocks = reinterpret_cast<double *>(ws + w.blocks);
  a.partial = reinterpret_cast<double *>(ws + w.partial);
  a.LL = LL_dev; a.L_pairs = L_pairs_dev; a.ntiles = w.ntiles;

  const int SP = state_bucket(m->S), SBP = state_bucket(b->SB);
  hipLaunchKernelGGL(dic_prep_kernel, dim3((unsigned)((m->C + 63) / 64)), dim3(64), 0, st, a, SP);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "dic_prep_kernel");
  const dim3 grid((unsigned)w.ntiles, (unsigned)m->G);
  e = SP == 4 ? launch_sbp<4>(a, SBP, grid, st) : SP == 8 ? launch_sbp<8>(a, SBP, grid, st)
                                                          : launch_sbp<16>(a, SBP, grid, st);
  if (e != hipSuccess) return hip_fail(e, "dic_kernel");
  hipLaunchKernelGGL(dic_reduce_kernel, dim3((unsigned)m->G), dim3(kThreads), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "dic_reduce_kernel");
  return VBHEM_OK;
}

}  // extern "C"
