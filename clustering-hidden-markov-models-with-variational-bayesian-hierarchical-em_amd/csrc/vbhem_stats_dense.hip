// vbhem_stats_dense.hip -- the fused E-step epilogue's dense-schedule statistics and the
// final reduction of either schedule (gfx950).
//
//   nm_kernel          streaming weighted sums over this chunk's bases
//                      (vbhem_compute_Statistics.m:33-55, gate Z > 1e-8):
//                        N1[j][s]    += g Z(i,j) sum_nu_1(i,j,s)
//                        M[j][s][r]  += g Z(i,j) sum_xi(i,j,s,r)
//   stats_kernel<..>   split-K reduction
//                        U[(j,s)][c] += sum_b (g Z(i,j) sum_t_nu(i,j,s,b)) u(i,b,c)
//                      with u = [1, mu, packed Sigma + mu mu'] -- the emission
//                      moments of mex.c:1348-1469 contracted over the base states
//                      and the bases at once: a (K*S) x (N*Sb) x NU GEMM on
//                      v_mfma_f64_16x16x4f64, K-dim streamed in batches of NBB bases.
//   stats_final_kernel fixed-order sum of the per-chunk slabs.
//   stats_final_fold_kernel  the same finish with list4_stats_reduce_kernel's reduction
//                      inside it (one base group, sums accumulated in fb_list4_kernel).
//
// Grid: x = chunk of consecutive bases, y = group of JG clusters (rows j*S+s),
// so no tile is loaded twice; every block keeps its whole (JG*S) x NU output
// block in MFMA accumulators and its N1/M entries in registers.
// All sums run in a fixed order (no atomics): bit-reproducible.
// The geometry and the kernels' buckets: plan_stats_dense (vbhem_stats_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vbhem_internal.h"
#include "vbhem_stats_dev.h"
#include "vbhem_stats_plan.h"

namespace vbhem {

typedef double double4_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// stats_kernel<TPW>: the emission-moment GEMM U (TPW = max MFMA tiles per
// wave).  Software-pipelined over batches of NBB (<= 4) bases: while batch b
// is contracted on the MFMA, the loads of batch b+1 (sum_t_nu, Z, covariances,
// means) are in flight into registers.  N1 / M are summed by nm_kernel.
// ---------------------------------------------------------------------------
template <int TPW, int GM>
__global__ __launch_bounds__(kStatsThreads) void stats_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, S = p.S, SB = p.SB, SBp = p.SBp, d = p.d, NU = p.NU, NBB = p.NBB;
  const int AST = p.AST, UST = p.UST;
  const int j0 = blockIdx.y * p.JG, j1 = min(K, j0 + p.JG), JGc = j1 - j0;
  const int RG = JGc * S, SS = S * S;
  const int MT = (RG + 15) / 16, NTL = (NU + 15) / 16, ntiles = MT * NTL;
  const bool full = p.covmode == kCovFull;
  const int dd = full ? d * d : d;
  const int NA = NBB * RG * SB;          // A elements per batch
  const int NRC = NBB * SB * dd;         // raw covariance values per batch
  const int NR = NRC + NBB * SB * d;     // + means

  double *As = lds;                                   // [RG][AST]   g Z sum_t_nu
  double *Us = As + (size_t)RG * AST;                 // [NBB*SBp][UST] base moments
  double *raw = Us + (size_t)NBB * SBp * UST;         // [NBB*SB][dd] | [NBB*SB][d]
  double *gzs = raw + (size_t)NR;                     // [NBB][JGc]
  int *tab = reinterpret_cast<int *>(gzs + (size_t)NBB * JGc);  // [NU] packed (a,b)

  for (int x = tid; x < RG * AST + NBB * SBp * UST; x += kStatsThreads) As[x] = 0.0;
  for (int c = tid; c < NU; c += kStatsThreads) {
    int a = -1, b = -1;
    if (c >= 1 && c <= d) {
      a = c - 1;
    } else if (c > d) {
      if (full) {
        int k = c - 1 - d;
        a = 0;
        while (k >= d - a) { k -= d - a; ++a; }
        b = a + k;
      } else {
        a = b = c - 1 - d;
      }
    }
    tab[c] = (a + 1) | ((b + 1) << 16);
  }

  const float invNU = 1.0f / (float)NU, invSB = 1.0f / (float)SB, invS = 1.0f / (float)S;
  const float invJG = 1.0f / (float)JGc;
  const float invRSB = 1.0f / (float)(RG * SB);

  double4_t acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};

  int b0, b1;
  chunk_range(p.i_end - p.i_begin, p.i_begin, blockIdx.x, gridDim.x, b0, b1);
  const double *__restrict__ tnu = p.tnu;

  // ---- register prefetch buffers ----
  double pa[kStatsMaxA], pr[kStatsMaxR], pz = 0.0;
  auto prefetch = [&](int ib) {
    const int nq = min(NBB, b1 - ib);
#pragma unroll
    for (int e = 0; e < kStatsMaxA; ++e) {
      const int x = tid + e * kStatsThreads;
      const int q = qdiv(x, invRSB), rem = x - q * RG * SB;
      pa[e] = (x < NA && q < nq) ? tnu[((size_t)(ib + q - p.i_buf0) * K * S + (size_t)j0 * S) * SB + rem]
                                 : 0.0;
    }
    const size_t gs = (size_t)ib * SB;
#pragma unroll
    for (int e = 0; e < kStatsMaxR; ++e) {
      const int x = tid + e * kStatsThreads;
      double v = 0.0;
      if (x < NRC) {
        if (x < nq * SB * dd) v = p.covars[gs * dd + x];
      } else if (x < NR) {
        const int y = x - NRC;
        if (y < nq * SB * d) v = p.centres[gs * d + y];
      }
      pr[e] = v;
    }
    if (tid < NBB * JGc) {
      const int q = qdiv(tid, invJG), jj = tid - q * JGc;
      pz = q < nq ? p.Z[(size_t)(ib + q - p.i_buf0) * K + j0 + jj] : 0.0;
    }
  };
  __syncthreads();
  if (b0 < b1) prefetch(b0);

  for (int ib = b0; ib < b1; ib += NBB) {
    const int nq = min(NBB, b1 - ib);
    // -- commit: gated Z and the raw base data of this batch -> LDS ------------------
    if (tid < NBB * JGc) gzs[tid] = (pz > Gate<GM>::value) ? pz : 0.0;
#pragma unroll
    for (int e = 0; e < kStatsMaxR; ++e) {
      const int x = tid + e * kStatsThreads;
      if (x < NR) raw[x] = pr[e];
    }
    __syncthreads();
    // -- A = g Z sum_t_nu and the base moments U -------------------------------------
#pragma unroll
    for (int e = 0; e < kStatsMaxA; ++e) {
      const int x = tid + e * kStatsThreads;
      if (x < NA) {
        const int q = qdiv(x, invRSB), rem = x - q * RG * SB;
        const int r = qdiv(rem, invSB), be = rem - r * SB;
        As[r * AST + q * SBp + be] = (q < nq) ? gzs[q * JGc + qdiv(r, invS)] * pa[e] : 0.0;
      }
    }
    for (int x = tid; x < NBB * SB * NU; x += kStatsThreads) {
      const int row = qdiv(x, invNU), c = x - row * NU;
      const int q = qdiv(row, invSB), be = row - q * SB;
      double u = 0.0;
      if (q < nq) {
        const int t = tab[c], a = (t & 0xffff) - 1, b = (t >> 16) - 1;
        const double *mu = raw + NRC + (size_t)row * d;
        if (a < 0) {
          u = 1.0;
        } else if (b < 0) {
          u = mu[a];
        } else {
          const double *C = raw + (size_t)row * dd;
          u = (full ? C[a * d + b] : C[a]) + mu[a] * mu[b];
        }
      }
      Us[(q * SBp + be) * UST + c] = u;
    }
    __syncthreads();
    // -- next batch's loads fly while this batch is contracted --------------------------
    if (ib + NBB < b1) prefetch(ib + NBB);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = wave + t * kStatsWaves;
      if (tile < ntiles) {
        const int mt = tile % MT, nt = tile / MT;
        const int row = mt * 16 + (lane & 15);
        const int col = nt * 16 + (lane & 15);
        const double *arow = As + (size_t)(row < RG ? row : 0) * AST;
        const double amask = row < RG ? 1.0 : 0.0;
        for (int ks = 0; ks < NBB * SBp; ks += 4) {
          const int k = ks + (lane >> 4);
          const double av = amask * arow[k];
          const double bv = Us[k * UST + col];
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // -- slab (this chunk) += partials ------------------------------------------
  double *slab = p.slabs + (size_t)blockIdx.x * p.slab_len;
  double *slabU = slab + K + (size_t)K * S + (size_t)K * SS + 2;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wave + t * kStatsWaves;
    if (tile < ntiles) {
      const int mt = tile % MT, nt = tile / MT;
      const int col = nt * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mt * 16 + (lane >> 4) + 4 * r;
        if (row < RG && col < NU) slabU[((size_t)j0 * S + row) * NU + col] += acc[t][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// nm_kernel: N1[j][s] += g Z(i,j) sum_nu_1(i,j,s) and M[j][s][r] += g Z(i,j)
// sum_xi(i,j,s,r) over this chunk's bases -- plain streaming weighted sums
// (each thread owns fixed outputs; 4 bases in flight per step).
// ---------------------------------------------------------------------------

// PER outputs per thread (K*S + K*S*S <= PER * 256), UNR bases per step in flight.
template <int PER, int UNR, int GM>
__global__ __launch_bounds__(kNmThreads) void nm_kernel(const StatsArgs p) {
  const int tid = threadIdx.x;
  const int K = p.K, S = p.S, KS = K * S, KSS = KS * S, NO = KS + KSS;
  int b0, b1;
  chunk_range(p.i_end - p.i_begin, p.i_begin, blockIdx.x, gridDim.x, b0, b1);
  double acc[PER];
  int jo[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    acc[e] = 0.0;
    const int x = tid + e * kNmThreads;
    jo[e] = x < KS ? x / S : (x < NO ? (x - KS) / (S * S) : 0);
  }
  for (int i = b0; i < b1; i += UNR) {
    double v[UNR][PER], z[UNR][PER];
    // branch-free: clamped addresses and unconditional loads (a conditional load
    // becomes a branch with its own vmcnt(0) wait and serialises the stream)
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const bool iv = i + u < b1;
      const size_t ir = (size_t)((iv ? i + u : i) - p.i_buf0);
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int x = tid + e * kNmThreads;
        const int xc = x < NO ? x : 0;
        const double *src = xc < KS ? p.nu1 + ir * KS + xc : p.xi + ir * KSS + (xc - KS);
        v[u][e] = *src;
        z[u][e] = p.Z[ir * K + jo[e]];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const bool iv = i + u < b1;
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int x = tid + e * kNmThreads;
        const double zz = z[u][e];
        z[u][e] = (iv && x < NO && zz > Gate<GM>::value) ? zz : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int e = 0; e < PER; ++e) acc[e] = fma(z[u][e], v[u][e], acc[e]);
  }
  double *slab = p.slabs + (size_t)blockIdx.x * p.slab_len + K;  // [N1 | M]
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int x = tid + e * kNmThreads;
    if (x < NO) slab[x] += acc[e];
  }
}

// 256 threads = 16 columns x 16 slab partitions: partition p sums slabs
// p, p+16, p+32, ... (128-B rows, four loads in flight per thread), then the 16
// partials are added in fixed order -- deterministic; ~slab_len/16 blocks (C4:
// 506) keep every CU's loads in flight (32-column blocks left it latency-bound).
// (The pieces shared with stats_final_fold_kernel: vbhem_stats_dev.h.)
__global__ __launch_bounds__(256) void stats_final_kernel(const double *slabs, int nslab_all,
                                                          int nslab_stats, int slab_len, int KT,
                                                          int S, int SL, double *out, int *fpre,
                                                          unsigned long long tag,
                                                          unsigned long long *done,
                                                          unsigned long long done_val) {
  __shared__ double part[kFinalParts][kFinalCols];
  if (fpre && blockIdx.x == 0 && threadIdx.x == 0) final_close_head(fpre, tag, done != nullptr);
  const int c = threadIdx.x % kFinalCols, pp = threadIdx.x / kFinalCols;
  const int x = blockIdx.x * kFinalCols + c;
  // resp_kernel's columns (Nj, Lt1, Lt7) have a partial in every chunk's slab; the
  // gated statistics' only in their kernel's parts
  const int xs = x % SL, lt = KT * (1 + S + S * S);
  const int nslab = (xs < KT || (xs >= lt && xs < lt + 2)) ? nslab_all : nslab_stats;
  part[pp][c] = x < slab_len ? final_partial(slabs, nslab, slab_len, x, pp) : 0.0;
  __syncthreads();
  if (pp == 0 && x < slab_len) {
    double s = part[0][c];
#pragma unroll
    for (int q = 1; q < kFinalParts; ++q) s += part[q][c];
    final_store(out + x, s, fpre, done != nullptr);
  }
  if (done && fpre) final_publish(fpre, done, done_val);
}

// stats_final_fold_kernel: the finish of a call whose gate-list pass accumulated the gated
// sums (fb_list4_kernel's partials, vbhem_list4_slots.h) over one base group -- what
// list4_stats_reduce_kernel followed by stats_final_kernel compute, in one launch and
// without the round trip through slab 0.  Blocks [0, K S): block (j, s) sums state s's row
// of cluster j over the cluster's slots (list4_reduce_row, the reduction's own order),
// shifts it back by z (su_entry) and stores it in the packed statistics; the value passes
// through the `0.0 +` that stats_final_kernel's sum over the one slab applied, so the bits
// are those of the two launches.  The blocks after them sum the responsibility kernels'
// columns (Nj, Lt1, Lt7 of each trial section) over every chunk's slab as
// stats_final_kernel does, 16 columns per block on the first 256 threads.  Block 0 closes
// the flag head; the completion word counts every block.
__global__ __launch_bounds__(kL4rThreads) void stats_final_fold_kernel(
    const StatsArgs p, const double *parts, int nw, int nslab_all, double *out, int *fpre,
    unsigned long long tag, unsigned long long *done, unsigned long long done_val) {
  extern __shared__ double lds[];
  __shared__ int plan[2];
  __shared__ double part[kL4rParts][kL4rCols];
  const int tid = threadIdx.x, K = p.K, S = p.S, KT = p.KT;
  if (fpre && blockIdx.x == 0 && tid == 0) final_close_head(fpre, tag, done != nullptr);
  if ((int)blockIdx.x < K * S) {
    const int j = blockIdx.x / S, s2 = blockIdx.x - j * S;
    const int NO = S * p.NU + S + S * S, tr = j / KT, jt = j - tr * KT;
    double *red = lds;  // [S][NU] | [S] | [S][S]: row s2 filled; then z [d]
    list4_reduce_row(p, parts, nw, j, s2, tid, red, plan, part);
    for (int o = tid; o < NO; o += kL4rThreads) {
      if (su_row(p, o) != s2) continue;
      size_t at;
      double s = 0.0;  // (stats_final_kernel's sum over slab 0 alone: -0.0 becomes 0.0)
      s += su_entry(p, red, red + NO, o, jt, at);
      final_store(out + (size_t)tr * p.SL + at, s, fpre, done != nullptr);
    }
  } else {
    // column r of the trials' (Nj [KT] | Lt1, Lt7) entries
    double(*fp)[kFinalCols] = reinterpret_cast<double(*)[kFinalCols]>(&part[0][0]);
    const int c = tid % kFinalCols, pp = tid / kFinalCols;
    const int r = ((int)blockIdx.x - K * S) * kFinalCols + c, ncol = (K / KT) * (KT + 2);
    const int tr = r / (KT + 2), q = r - tr * (KT + 2);
    const int x = tr * p.SL + (q < KT ? q : KT * (1 + S + S * S) + (q - KT));
    const bool act = pp < kFinalParts && r < ncol;
    if (pp < kFinalParts) fp[pp][c] = act ? final_partial(p.slabs, nslab_all, p.slab_len, x, pp) : 0.0;
    __syncthreads();
    if (pp == 0 && act) {
      double s = fp[0][c];
#pragma unroll
      for (int k = 1; k < kFinalParts; ++k) s += fp[k][c];
      final_store(out + x, s, fpre, done != nullptr);
    }
  }
  if (done && fpre) final_publish(fpre, done, done_val);
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
template <int GM>
static hipError_t launch_stats_gate(const StatsArgs &a, const DensePlan &dp, int nchunk, hipStream_t st) {
  const StatsKernel fn =
      pick_kernel<4, 8, 16>(dp.TPW, [](auto tpw) { return stats_kernel<decltype(tpw)::value, GM>; });
  const StatsKernel nm = dp.nm_per == 6 ? nm_kernel<6, 4, GM> : nm_kernel<24, 1, GM>;
  if (!dp.ok || !fn) return hipErrorInvalidValue;
  hipError_t e = set_dyn_lds(reinterpret_cast<const void *>(fn), dp.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(nchunk, dp.ngroups), dim3(kStatsThreads), dp.lds, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(nm, dim3(nchunk), dim3(kNmThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_stats(const StatsArgs &a, const DensePlan &dp, int nchunk, hipStream_t st) {
  return a.vhem ? launch_stats_gate<kGateVhem>(a, dp, nchunk, st)
                : launch_stats_gate<kGateVbhem>(a, dp, nchunk, st);
}

hipError_t launch_stats_final(const double *slabs, int nslab, int nslab_stats, int slab_len, int KT,
                              int S, int SL, double *out, hipStream_t st, int *fpre,
                              unsigned long long *done, unsigned long long done_val) {
  if (nslab_stats < 1 || nslab_stats > nslab || SL < 1 || slab_len % SL != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stats_final_kernel, dim3((slab_len + kFinalCols - 1) / kFinalCols), dim3(256),
                     0, st, slabs, nslab, nslab_stats, slab_len, KT, S, SL, out, fpre,
                     fpre ? flag_tag() : 0ull, fpre ? done : nullptr, done_val);
  return hipGetLastError();
}

hipError_t launch_stats_final_fold(const StatsArgs &a, const GatedPlan &gp, const double *parts, int nw,
                                   int nslab, double *out, hipStream_t st, int *fpre,
                                   unsigned long long *done, unsigned long long done_val) {
  if (!gp.ok || gp.kernel != GatedStats::kList4Reduce || gp.cap != a.S || !parts || nw < 1 || !a.uz ||
      !a.list_tot || !a.assign || nslab < 1 || a.KT < 1 || a.K % a.KT != 0 ||
      a.slab_len != (a.K / a.KT) * a.SL)
    return hipErrorInvalidValue;
  const int ncol = (a.K / a.KT) * (a.KT + 2);
  hipLaunchKernelGGL(stats_final_fold_kernel, dim3(a.K * a.S + (ncol + kFinalCols - 1) / kFinalCols),
                     dim3(kL4rThreads), gp.lds, st, a, parts, nw, nslab, out, fpre,
                     fpre ? flag_tag() : 0ull, fpre ? done : nullptr, done_val);
  return hipGetLastError();
}

}  // namespace vbhem
