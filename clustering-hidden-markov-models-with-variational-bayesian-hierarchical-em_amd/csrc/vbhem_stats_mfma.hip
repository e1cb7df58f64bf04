// vbhem_stats_mfma.hip -- the fused E-step epilogue's gated statistic sums from the
// statistics copy Us of a prepared base set (gfx950):
//
//   stats_list_m_kernel        the sums over the gate lists on the MFMA pipe
//   list4_stats_reduce_kernel  the reduction of the partial sums that fb_list4_kernel's
//                              accumulating variant left (vbhem_list4_slots.h)
// All sums run in a fixed order (no atomics).  Buckets and block counts: vbhem_stats_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vbhem_internal.h"
#include "vbhem_stats_dev.h"
#include "vbhem_stats_plan.h"

namespace vbhem {

// ---------------------------------------------------------------------------
// stats_list_m_kernel<NTW, G, KSM, NXR, PD>: the gated sums on the MFMA pipe, from the
// statistics copy Us of the prepared operand.  For cluster j the emission moments are
//   acc[s][f] = sum over the gated pairs (i, j) and base states b of
//               (Z tnu)(s, b) * Us(i, b, f)
// i.e. one (16 x 4) x (4 x 16) v_mfma_f64_16x16x4f64 per k-slice of four base states
// and 16-feature tile: A = Z tnu (lane: state s = lane & 15, base state 4 kk + lane / 16;
// zero past S / SB; KSM = SBP / 4 k-slices), B = 16 consecutive features of four base
// states (one contiguous 512-byte segment of Us's tile-major block per load).  Block
// (c, j) = part c of cluster j's list, as stats_list_u_kernel.  Its 4 waves are G pair
// groups x 4 / G tile groups: wave w takes
// the part's pairs w % G, + G, ... and the feature tiles w / G + (4 / G) t, t < NTW,
// plus the sum_nu_1 | sum_xi entries lane + 64 (w / G + (4 / G) r).  The next PD - 1
// pairs' operands are in flight while a pair's MFMAs run (a register ring; the kernel is
// bound by memory latency, not by the MFMA pipe); no LDS in the loop.  The
// pair groups' sums are added in group order at the end (bit-reproducible).  Output
// as stats_list_u_kernel (shifted back by z).
// ---------------------------------------------------------------------------
typedef double dbl4 __attribute__((ext_vector_type(4)));

template <int NTW, int G, int KSM, int NXR, int PD>
__global__ __launch_bounds__(64 * kSmWaves) void stats_list_m_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  constexpr int TG = kSmWaves / G;  // tile groups; NXR: sum_nu_1 | sum_xi chunks of 64 per wave
  // the wave index in an SGPR: the tile / pair-group tests below are scalar branches and
  // the loads' tile offsets scalar adds to the pair's base
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave % G, tg = wave / G;
  const int K = p.K, S = p.S, SB = p.SB, d = p.d, NU = p.NU;
  const int SBP = us_sbp(SB), NUP = us_nup(NU), ntile = NUP / 16;  // SBP = 4 KSM (launch)
  const int OT = S * SB, NX = S + S * S;
  // block -> (cluster j, part c of its list, parts nch): the gated pairs of all clusters
  // in parts of about P = total / (blocks - K) pairs, at most p.nzero (the slab count)
  // parts per cluster, at least one (an empty cluster's block writes its zeros)
  __shared__ int sm_map[3];
  if (wave == 0) {
    int total = 0;
    for (int x = lane; x < K; x += 64) total += p.list_tot[x];
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    const int nb = (int)gridDim.x, P = max(1, (total + max(1, nb - K) - 1) / max(1, nb - K));
    int pre = 0, jj = -1, cc = 0, np = 1;
    for (int x0 = 0; x0 < K && jj < 0; x0 += 64) {
      const int x = x0 + lane;
      int parts = 0;
      if (x < K) {
        const int t = p.list_tot[x], Pj = max(P, (t + p.nzero - 1) / p.nzero);
        parts = max(1, (t + Pj - 1) / Pj);
      }
      int inc = parts;  // inclusive prefix over the lanes
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      const int b0 = pre + inc - parts;  // this cluster's first block
      const bool hit = x < K && (int)blockIdx.x >= b0 && (int)blockIdx.x < b0 + parts;
      const unsigned long long m = __ballot(hit);
      if (m) {
        const int src = __builtin_ctzll(m);
        jj = __shfl(x, src, 64);
        cc = (int)blockIdx.x - __shfl(b0, src, 64);
        np = __shfl(parts, src, 64);
      }
      pre += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      sm_map[0] = jj;
      sm_map[1] = cc;
      sm_map[2] = np;
    }
  }
  __syncthreads();
  const int j = sm_map[0], c = sm_map[1], nch = sm_map[2];
  if (j < 0) return;  // past the last part (block-uniform)
  double *red = lds;                                  // [S][NU] | [S] | [S][S]
  double *zs = red + (size_t)S * NU + S + S * S;      // [d]
  for (int a = tid; a < d; a += 64 * kSmWaves) zs[a] = p.uz[a];
  const int kl = lane >> 4, cl = lane & 15;
  dbl4 acc[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t) acc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
  double ax[NXR];
#pragma unroll
  for (int r = 0; r < NXR; ++r) ax[r] = 0.0;
  const int tot = p.list_tot[j];
  const int n0 = (int)((long long)tot * c / nch), n1 = (int)((long long)tot * (c + 1) / nch);
  const int *lst = p.list + (size_t)j * p.list_cap;
  // one pair's operands: A values per k-slice, B values per (tile, k-slice), its Z and
  // its sum_nu_1 / sum_xi entries; a ring of PD of them (PD - 1 pairs' loads in flight
  // while a pair's MFMAs run)
  struct Ops {
    double ta[KSM], ub[NTW][KSM], xv[NXR], z;
  };
  bool ta_ok[KSM];  // this lane's A entry (state cl, base state 4 kk + kl) exists
#pragma unroll
  for (int kk = 0; kk < KSM; ++kk) ta_ok[kk] = cl < S && 4 * kk + kl < SB;
  Ops buf[PD];
  auto load = [&](int i, Ops &o) {
    // wave-uniform bases (SGPRs), 32-bit lane offsets: saddr loads, no 64-bit address
    // arithmetic per lane
    const size_t lp = (size_t)(i - p.i_buf0) * K + j;
    // Z by a vector load (an address in VGPRs), in order with the pair's other loads: a
    // scalar load would be waited for (lgkmcnt(0)) at the start of the next pair
    unsigned zo = (unsigned)lp;  // (a 32-bit offset: the laundered pointer would be flat)
    asm("" : "+v"(zo));
    o.z = p.Z[zo];
    const double *us = p.Us + (size_t)i * SBP * NUP;
    const double *tp = p.tnu + lp * OT, *n1p = p.nu1 + lp * S, *xp = p.xi + lp * S * S;
    // lane-varying bounds by clamped (always valid) loads, not branches; the select that
    // zeroes the clamped lanes waits for compute (a select here would wait for the load,
    // and with it for every load issued before it: no prefetch at all)
#pragma unroll
    for (int kk = 0; kk < KSM; ++kk) {
      const int b = 4 * kk + kl;
      o.ta[kk] = tp[ta_ok[kk] ? (unsigned)(cl * SB + b) : 0u];
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        const int ft = min(tg + TG * t, ntile - 1);  // past ntile: a repeat, never used
        o.ub[t][kk] = us[(unsigned)((ft * SBP + b) * 16 + cl)];  // b < SBP: in the block
      }
    }
    // one load from a lane-selected address (lanes past NX read xi[0]: their sums are
    // never stored)
#pragma unroll
    for (int r = 0; r < NXR; ++r) {
      const int x = lane + 64 * (tg + TG * r);
      o.xv[r] = *(x < S ? n1p + x : xp + (x < NX ? x - S : 0));
    }
  };
  auto compute = [&](const Ops &o) {
#pragma unroll
    for (int kk = 0; kk < KSM; ++kk) {
      const double av = o.z * (ta_ok[kk] ? o.ta[kk] : 0.0);
#pragma unroll
      for (int t = 0; t < NTW; ++t)
        if (tg + TG * t < ntile) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, o.ub[t][kk], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < NXR; ++r) ax[r] = fma(o.z, o.xv[r], ax[r]);
  };
  // this wave's pairs: n0 + pg + G k, k < cnt.  The loop body is branch-free around the
  // loads (every slot loaded, the cursor clamped to the last pair; the list entries by
  // scalar loads one pair ahead), so the compiler's wait before a pair's MFMAs counts
  // exactly the PD - 1 later pairs' loads instead of draining them at a join.
  const int nf = n0 + pg;
  const int cnt = nf < n1 ? (n1 - nf + G - 1) / G : 0;
  if (cnt > 0) {  // wave-uniform
    const int kmax = cnt - 1;
    const int *lw = lst + nf;
#pragma unroll
    for (int u = 0; u < PD - 1; ++u) load(lw[G * min(u, kmax)], buf[u]);
    int inext = lw[G * min(PD - 1, kmax)];
    for (int k0 = 0; k0 < cnt; k0 += PD) {
#pragma unroll
      for (int u = 0; u < PD; ++u) {
        const int k = k0 + u;
        const int il = inext;
        inext = lw[G * min(k + PD, kmax)];
        load(il, buf[(u + PD - 1) % PD]);  // pair min(k + PD - 1, cnt - 1)
        if (k < cnt) compute(buf[u]);      // wave-uniform
      }
    }
  }
  // the pair groups' sums into the block's LDS record in group order, then su_output
  for (int g = 0; g < G; ++g) {
    if (pg == g) {
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        const int f = 16 * (tg + TG * t) + cl;
        if (tg + TG * t < ntile && f < NU)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int s2 = kl + 4 * v;
            if (s2 < S) {
              double *r = red + (size_t)s2 * NU + f;
              *r = g == 0 ? acc[t][v] : *r + acc[t][v];
            }
          }
      }
#pragma unroll
      for (int r = 0; r < NXR; ++r) {
        const int x = lane + 64 * (tg + TG * r);
        if (x < NX) {
          double *o = red + (size_t)S * NU + x;
          *o = g == 0 ? ax[r] : *o + ax[r];
        }
      }
    }
    __syncthreads();
  }
  su_output(p, red, zs, c, nch, j, tid);
}

// list4_stats_reduce_kernel: the gated sums that fb_list4_kernel's accumulating variant
// left as partials (vbhem_list4_slots.h).  Block (j, s) sums state s's row of cluster j over
// the cluster's slots (list4_reduce_row, vbhem_stats_dev.h); su_output then shifts the row
// back by z (which needs only the row's own sums) and writes or adds slab 0's sections.
// With one base group the finishing kernel does this itself (stats_final_fold_kernel,
// vbhem_stats_dense.hip) and this kernel is not launched.
__global__ __launch_bounds__(kL4rThreads) void list4_stats_reduce_kernel(const StatsArgs p,
                                                                        const double *parts, int nw) {
  extern __shared__ double lds[];
  __shared__ int plan[2];
  __shared__ double part[kL4rParts][kL4rCols];
  const int tid = threadIdx.x, S = p.S, j = blockIdx.x / S, s2 = blockIdx.x - j * S;
  double *red = lds;  // [S][NU] | [S] | [S][S]: row s2 filled; then z [d]
  list4_reduce_row(p, parts, nw, j, s2, tid, red, plan, part);
  if (tid < 64 * kSuWaves) su_output(p, red, red + S * p.NU + S + S * S, 0, 1, j, tid, s2);
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
// ring depth 3 since the load phase is branch-free (profiles/r05ad_ab_stats_ring_depth.txt:
// statistics per step C4 0.160 -> 0.155 ms, C5 4.7-4.9 -> 4.5-4.7 ms, shard and C3 equal;
// depth 4 in between).  Before that fix depth 3 lost: the ring never filled and its
// registers cost residency (C5 7.7 vs 5.8 ms)
#ifndef VBHEM_SM_PDD
#define VBHEM_SM_PDD 3   // the ring depth (build switch for A/B)
#endif

// stats_list_m_kernel's instance for a plan's bucket (NTW, G) x KSM x NXR (null: none);
// launch_stats_list launches it
StatsKernel stats_mfma_kernel(const GatedPlan &gp) {
  return pick_kernel<41, 42, 43, 44, 23, 24, 13>(10 * gp.G + gp.NTW, [&](auto gn) {
    return pick_kernel<1, 2, 3, 4>(gp.KSM, [&](auto ksm) {
      return pick_kernel<1, 2, 3, 5>(gp.NXR, [](auto nxr) {
        constexpr int NTW = decltype(gn)::value % 10, G = decltype(gn)::value / 10;
        return stats_list_m_kernel<NTW, G, decltype(ksm)::value, decltype(nxr)::value, VBHEM_SM_PDD>;
      });
    });
  });
}

hipError_t launch_list4_stats_reduce(const StatsArgs &a, const GatedPlan &gp, const double *parts, int nw,
                                     hipStream_t st) {
  if (!gp.ok || gp.kernel != GatedStats::kList4Reduce || !parts || nw < 1 || !a.uz || !a.list_tot)
    return hipErrorInvalidValue;
  StatsArgs b = a;
  b.nzero = gp.nzero;
  hipLaunchKernelGGL(list4_stats_reduce_kernel, dim3(a.K * gp.cap), dim3(kL4rThreads), gp.lds, st, b,
                     parts, nw);
  return hipGetLastError();
}

}  // namespace vbhem
