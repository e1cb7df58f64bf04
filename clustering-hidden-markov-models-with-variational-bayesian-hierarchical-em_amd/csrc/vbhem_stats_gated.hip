// vbhem_stats_gated.hip -- the fused E-step epilogue's gated schedule (gfx950): the
// per-cluster lists of pairs with Z > 1e-8 and the Z-weighted statistic sums over them
// only (vbhem_compute_Statistics.m:33-55).
//
//   gate_list_kernel     the lists, from resp_kernel's per-chunk gate counts
//   stats_list_kernel    the sums with the base moments gathered from the covariances
//   stats_list_u_kernel  ... read from the emission GEMM's prepared operand U
//   stats_list_g_kernel  ... the same for small moment vectors, several pairs per wave
// (stats_list_m_kernel and list4_stats_reduce_kernel: vbhem_stats_mfma.hip.)  All sums run
// in a fixed order (no atomics).  Which kernel runs: plan_stats_gated (vbhem_stats_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vbhem_internal.h"
#include "vbhem_stats_dev.h"
#include "vbhem_stats_plan.h"

namespace vbhem {

// ---------------------------------------------------------------------------
// gate_list_kernel: the gated pairs as per-cluster lists of bases, ascending i
// (list[j][n], n < list_tot[j]).  Block = the resp_kernel chunk: its offset in
// cluster j's list is the gate count of the chunks before it; inside the chunk
// the bases are ranked by wave ballots (masks in LDS, one barrier per slice).
// Deterministic (no global atomics): the same list every call.
// MASK (K <= 64): the gate test read from the responsibility kernel's masks
// (StatsArgs::gmask, 8 bytes per base) instead of made again on the K doubles of Z.
// ---------------------------------------------------------------------------

template <int GM, bool MASK>
__global__ __launch_bounds__(kListThreads) void gate_list_kernel(const StatsArgs p) {
  extern __shared__ int ish[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = kListThreads / 64;
  const int K = p.K, nchunk = gridDim.x, me = blockIdx.x;
  int *before = ish;          // [K] this chunk's offset in every cluster's list
  int *total = ish + K;       // [K]
  int *wcnt = ish + 2 * K;    // [NW] (unused slot)
  // this chunk's offset (gate counts of chunks c < me) and cluster totals: thread
  // (r, j) sums chunks c = r, r + R, ...; then the R partials of each j in order
  int *pb = wcnt + NW;        // [R][K]
  int *pt = pb + kListThreads;  // [R][K]
  for (int j0 = 0; j0 < K; j0 += kListThreads) {
    const int KC = min(K - j0, kListThreads), R = kListThreads / KC;
    const int r = tid / KC, j = j0 + (tid - r * KC);
    if (r < R) {
      // 32 chunks' counts in flight per thread (clamped addresses, then masked sums): one
      // memory round trip for up to 32 R chunks instead of one per 8
      int sb = 0, stt = 0;
      for (int c0 = r; c0 < nchunk; c0 += 32 * R) {
        int v[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) {
          const int c = min(c0 + q * R, nchunk - 1);
          v[q] = p.gate_cnt[(size_t)c * K + j];
        }
#pragma unroll
        for (int q = 0; q < 32; ++q) {
          const int c = c0 + q * R;
          stt += c < nchunk ? v[q] : 0;
          sb += c < me ? v[q] : 0;
        }
      }
      pb[tid] = sb;
      pt[tid] = stt;
    }
    __syncthreads();
    if (tid < KC) {
      int sb = 0, stt = 0;
      for (int q = 0; q < R; ++q) {
        sb += pb[q * KC + tid];
        stt += pt[q * KC + tid];
      }
      before[j0 + tid] = sb;
      total[j0 + tid] = stt;
    }
    __syncthreads();
  }
  if (me == 0)
    for (int j = tid; j < K; j += kListThreads) p.list_tot[j] = total[j];
  int b0, b1;
  chunk_range(p.i_end - p.i_begin, p.i_begin, me, nchunk, b0, b1);
  // per 256-base slice: every wave ballots all K clusters into LDS masks (no
  // barrier per cluster), one barrier, then each thread places its base in the
  // lists that gate it in, after the bases of the lower waves and chunks
  unsigned long long *msk = reinterpret_cast<unsigned long long *>(
      ish + ((2 * K + NW + 2 * kListThreads + 1) & ~1));  // [NW][K], 8-byte aligned
  constexpr int kJB = 16;  // clusters whose Z are loaded together (one round trip, not K)
  for (int i0 = b0; i0 < b1; i0 += kListThreads) {
    const int i = i0 + tid;
    const bool iv = i < b1;
    if constexpr (MASK) {
      // K <= 64: the base's gate mask (one coalesced load per slice), the test the
      // responsibility kernel made when it counted gate_cnt
      const unsigned long long gm = iv ? p.gmask[i - p.i_buf0] : 0ull;
      for (int j = 0; j < K; ++j) {
        const unsigned long long m = __ballot((gm >> j) & 1ull);
        if (lane == 0) msk[wave * K + j] = m;
      }
    } else {
      const double *Zi = p.Z + (size_t)((iv ? i : b0) - p.i_buf0) * K;
      for (int j0 = 0; j0 < K; j0 += kJB) {
        double z[kJB];
#pragma unroll
        for (int q = 0; q < kJB; ++q) z[q] = j0 + q < K ? Zi[j0 + q] : 0.0;
#pragma unroll
        for (int q = 0; q < kJB; ++q) {
          const unsigned long long m = __ballot(iv && z[q] > Gate<GM>::value);
          if (lane == 0 && j0 + q < K) msk[wave * K + j0 + q] = m;
        }
      }
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
      const unsigned long long m = msk[wave * K + j];
      if ((m >> lane) & 1ull) {
        int off = before[j];
        for (int w = 0; w < wave; ++w) off += __popcll(msk[w * K + j]);
        p.list[(size_t)j * p.list_cap + off + __popcll(m & ((1ull << lane) - 1ull))] = i;
      }
    }
    __syncthreads();  // every thread has read before[] and the masks
    for (int j = tid; j < K; j += kListThreads) {
      int t = 0;
      for (int w = 0; w < NW; ++w) t += __popcll(msk[w * K + j]);
      before[j] += t;
    }
    __syncthreads();  // before[] updated before the next slice's masks overwrite these
  }
}

// ---------------------------------------------------------------------------
// stats_list_kernel<PER>: the gated sums over the gated-pair lists only.
// Block (c, j) = part c of cluster j's list (fixed split, ascending bases) ->
// slab c's cluster-j entries; PB pairs per batch staged in LDS as
//   [ Z sum_t_nu (S x SB) | Z sum_nu_1 (S) | Z sum_xi (S x S) | u (SB x NU) ],
// each thread owning PER outputs of  N1 (S) | M (S x S) | U (S x NU).
// ---------------------------------------------------------------------------

template <int PER>
__global__ __launch_bounds__(kSlThreads) void stats_list_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int K = p.K, S = p.S, SB = p.SB, d = p.d, NU = p.NU, PB = p.PB;
  const int j = blockIdx.y, c = blockIdx.x, nch = gridDim.x;
  const bool full = p.covmode == kCovFull;
  const int dd = full ? d * d : d;
  const int OT = S * SB, OM = OT + S, OU = OM + S * S;  // record: tnu | nu1 | xi | u
  const int RS = (OU + SB * NU + 1) / 2 * 2;  // record stride (doubles), = sl_record()
  const int NO = S + S * S + S * NU;
  double *rec = lds;                                            // [PB][RS]
  int *tab = reinterpret_cast<int *>(rec + (size_t)PB * RS);    // [NU] packed (a, b)
  double *sz = reinterpret_cast<double *>(tab + (NU + 1) / 2 * 2);  // [PB] Z of the batch
  int *sidx = reinterpret_cast<int *>(sz + PB);                   // [PB] bases of the batch
  for (int cc = tid; cc < NU; cc += kSlThreads) {
    int a = -1, b = -1;
    if (cc >= 1 && cc <= d) {
      a = cc - 1;
    } else if (cc > d) {
      if (full) {
        int k = cc - 1 - d;
        a = 0;
        while (k >= d - a) { k -= d - a; ++a; }
        b = a + k;
      } else {
        a = b = cc - 1 - d;
      }
    }
    tab[cc] = (a + 1) | ((b + 1) << 16);
  }
  const int tot = p.list_tot[j];
  const int n0 = (int)((long long)tot * c / nch), n1 = (int)((long long)tot * (c + 1) / nch);
  const int *lst = p.list + (size_t)j * p.list_cap;
  const float invNU = 1.0f / (float)NU, invOU = 1.0f / (float)OU, invUN = 1.0f / (float)(SB * NU);
  double *slab = p.slabs + (size_t)c * p.slab_len;
  // trial section of cluster j (R = K / KT trials; one section when KT = K)
  const int KT = p.KT, tr = j / KT, jt = j - tr * KT;
  double *tsl = slab + (size_t)tr * p.SL;
  for (int o0 = 0; o0 < NO; o0 += PER * kSlThreads) {
    double acc[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[e] = 0.0;
    for (int n = n0; n < n1; n += PB) {
      const int np = min(PB, n1 - n);
      __syncthreads();  // tab ready / previous batch consumed
      // batch-wide staging: every element of every pair in flight at once
      if (tid < np) {
        const int i = lst[n + tid];
        const size_t lp = (size_t)(i - p.i_buf0) * K + j;
        sidx[tid] = i;
        sz[tid] = p.Z[lp];
      }
      __syncthreads();
      for (int x = tid; x < np * OU; x += kSlThreads) {
        const int pq = qdiv(x, invOU), e = x - pq * OU;
        const size_t lp = (size_t)(sidx[pq] - p.i_buf0) * K + j;
        double v;
        if (e < OT) v = p.tnu[lp * OT + e];
        else if (e < OM) v = p.nu1[lp * S + (e - OT)];
        else v = p.xi[lp * S * S + (e - OM)];
        rec[(size_t)pq * RS + e] = sz[pq] * v;
      }
      for (int x = tid; x < np * SB * NU; x += kSlThreads) {
        const int pq = qdiv(x, invUN), e = x - pq * SB * NU;
        const int bb = qdiv(e, invNU), cc = e - bb * NU;
        const int i = sidx[pq];
        const int t = tab[cc], a = (t & 0xffff) - 1, b2 = (t >> 16) - 1;
        const double *mu = p.centres + ((size_t)i * SB + bb) * d;
        const double *C = p.covars + ((size_t)i * SB + bb) * dd;
        double u;
        if (a < 0) u = 1.0;
        else if (b2 < 0) u = mu[a];
        else u = (full ? C[a * d + b2] : C[a]) + mu[a] * mu[b2];
        rec[(size_t)pq * RS + OU + e] = u;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int o = o0 + tid + e * kSlThreads;
        if (o < S) {
          for (int pq = 0; pq < np; ++pq) acc[e] += rec[(size_t)pq * RS + OT + o];
        } else if (o < S + S * S) {
          for (int pq = 0; pq < np; ++pq) acc[e] += rec[(size_t)pq * RS + OM + (o - S)];
        } else if (o < NO) {
          const int oo = o - S - S * S;
          const int sg = qdiv(oo, invNU), cc = oo - sg * NU;
          for (int pq = 0; pq < np; ++pq) {
            const double *r = rec + (size_t)pq * RS;
            for (int bb = 0; bb < SB; ++bb) acc[e] = fma(r[sg * SB + bb], r[OU + bb * NU + cc], acc[e]);
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int o = o0 + tid + e * kSlThreads;
      double *dst = nullptr;
      if (o < S) {
        dst = tsl + KT + (size_t)jt * S + o;
      } else if (o < S + S * S) {
        dst = tsl + KT + (size_t)KT * S + (size_t)jt * S * S + (o - S);
      } else if (o < NO) {
        const int oo = o - S - S * S;
        dst = tsl + KT + (size_t)KT * S + (size_t)KT * S * S + 2 + (size_t)jt * S * NU + oo;
      }
      if (dst) *dst = p.assign ? acc[e] : *dst + acc[e];
    }
  }
}

// ---------------------------------------------------------------------------
// stats_list_u_kernel<FPL, SM>: stats_list_kernel on the emission GEMM's prepared
// operand U (vbhem_emission.hip: per base-state column the features
// [Sigma_ab + Sigma_ba + 2 mu'_a mu'_b (a < b) | Sigma_aa + mu'_a^2, mu'], mu' = mu - z),
// so the emission moments need no gather of the d x d covariances and no
// per-element rebuild.  Block (c, j) = part c of cluster j's list, as
// stats_list_kernel; wave w takes the part's pairs w, w + 4, ...:
//   lane f (+ 64 q) owns moment column f = 0 (ones) | 1 + a (mu_a) | 1 + d + k (packed
//   (a, b) of Sigma + mu mu') for every state s: acc[q][s] += sum_b Z tnu(s, b) u(b, f),
//   with Z tnu and the pair's U columns staged per pair in a wave-private LDS slab (U
//   read coalesced: lanes over (k-step, k, base state), SB contiguous columns per row);
//   sum_xi / sum_nu_1 accumulate lane-parallel from global memory.
// Waves reduce in fixed order (bit-reproducible), then every output is shifted back:
//   mu_a = m'_a + z_a N,  (Sigma + mu mu')_ab = Q'_ab + z_a m'_b + z_b m'_a + z_a z_b N
// (Q' = half the off-diagonal feature), N = sum Z tnu, m' = sum Z tnu mu'.
// FPL = moment columns per lane.  Only FPL = 1 (NU <= 64) is built: with two or three
// columns per lane the covariance gather of stats_list_kernel measured faster (C5, d = 16
// full: 1.74 against 1.78 ms per 100 k-base step), so the plan sends NU > 64 there.
// ---------------------------------------------------------------------------
template <int FPL, int SM>
__global__ __launch_bounds__(64 * kSuWaves) void stats_list_u_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, S = p.S, SB = p.SB, d = p.d, NU = p.NU, kq = p.ukdp / 4;
  const bool full = p.covmode == kCovFull;
  const int NPF = full ? d * (d + 1) / 2 : d;
  const int j = blockIdx.y, c = blockIdx.x, nch = gridDim.x;
  const int OT = S * SB, TS = (OT + 1) / 2 * 2, KP = p.ukdp + 1;
  const int WS = TS + (SB * KP + 1) / 2 * 2;
  double *tw = lds + (size_t)wave * WS;                 // [SB][S] Z tnu of the wave's pair
  double *uw = tw + TS;                                 // [SB][KP] its U columns
  double *red = lds + (size_t)kSuWaves * WS;           // [S][NU] | [S] | [S][S]
  double *zs = red + (size_t)S * NU + S + S * S;       // [d]
  for (int a = tid; a < d; a += 64 * kSuWaves) zs[a] = p.uz[a];
  // my moment columns: U feature (-1: the ones column), valid
  int ue[FPL];
  bool fv[FPL];
#pragma unroll
  for (int q = 0; q < FPL; ++q) {
    const int f = lane + 64 * q;
    fv[q] = f < NU;
    ue[q] = f == 0 ? -1 : f <= d ? NPF + f - 1 : f - 1 - d;
  }
  double acc[FPL][SM], accx[4], accn = 0.0;
#pragma unroll
  for (int q = 0; q < FPL; ++q)
#pragma unroll
    for (int s2 = 0; s2 < SM; ++s2) acc[q][s2] = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) accx[e] = 0.0;
  const int tot = p.list_tot[j];
  const int n0 = (int)((long long)tot * c / nch), n1 = (int)((long long)tot * (c + 1) / nch);
  const int *lst = p.list + (size_t)j * p.list_cap;
  const double *Ub0 = p.U + kUHead;
  for (int nb = n0 + wave; nb < n1; nb += 64 * kSuWaves) {
    // the bases of the next 64 pairs of this wave, one per lane
    const int nl = nb + lane * kSuWaves;
    const int il = nl < n1 ? lst[nl] : 0;
    const int np = min(64, (n1 - nb + kSuWaves - 1) / kSuWaves);
    for (int k = 0; k < np; ++k) {
      const int i = __builtin_amdgcn_readlane(il, k);
      const size_t lp = (size_t)(i - p.i_buf0) * K + j;
      const double z = p.Z[lp];
      // every load of the pair in flight before the first LDS write (a plain loop
      // waits on each load before its store)
      {
        double v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int x = lane + 64 * e;
          v[e] = x < OT ? p.tnu[lp * OT + x] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int x = lane + 64 * e;
          if (x < OT) {
            const int s2 = x / SB, b = x - s2 * SB;
            tw[b * S + s2] = z * v[e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = lane + 64 * e;
        if (x < S * S) accx[e] = fma(z, p.xi[lp * S * S + x], accx[e]);
      }
      if (lane < S) accn = fma(z, p.nu1[lp * S + lane], accn);
      const long long c0 = (long long)i * SB - p.u_col0;
      for (int x0 = lane; x0 < 4 * kq * SB; x0 += 64 * 8) {
        double v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int x = x0 + 64 * e;
          const int t4 = x / SB, b = x - t4 * SB;  // t4 = 4 t + k: feature e
          const long long col = c0 + b;
          v[e] = x < 4 * kq * SB
                     ? Ub0[(size_t)(col >> 4) * kq * 64 + (t4 >> 2) * 64 + (t4 & 3) * 16 + (col & 15)]
                     : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int x = x0 + 64 * e;
          const int t4 = x / SB, b = x - t4 * SB;
          if (x < 4 * kq * SB) uw[b * KP + t4] = v[e];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
      for (int b = 0; b < SM; ++b) {
        if (b < SB) {
          double uv[FPL];
#pragma unroll
          for (int q = 0; q < FPL; ++q)
            uv[q] = !fv[q] ? 0.0 : ue[q] < 0 ? 1.0 : uw[b * KP + ue[q]];
#pragma unroll
          for (int s2 = 0; s2 < SM; ++s2) {
            if (s2 < S) {
              const double tv = tw[b * S + s2];
#pragma unroll
              for (int q = 0; q < FPL; ++q) acc[q][s2] = fma(tv, uv[q], acc[q][s2]);
            }
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  // fixed-order reduction over the waves
  for (int w = 0; w < kSuWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int q = 0; q < FPL; ++q)
#pragma unroll
        for (int s2 = 0; s2 < SM; ++s2) {
          const int f = lane + 64 * q;
          if (fv[q] && s2 < S) {
            double *r = red + (size_t)s2 * NU + f;
            *r = w == 0 ? acc[q][s2] : *r + acc[q][s2];
          }
        }
      if (lane < S) {
        double *r = red + (size_t)S * NU + lane;
        *r = w == 0 ? accn : *r + accn;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = lane + 64 * e;
        if (x < S * S) {
          double *r = red + (size_t)S * NU + S + x;
          *r = w == 0 ? accx[e] : *r + accx[e];
        }
      }
    }
    __syncthreads();
  }
  su_output(p, red, zs, c, nch, j, tid);
}

// stats_list_g_kernel<LG, SM>: stats_list_u_kernel for small moment vectors
// (NU <= LG <= 32, e.g. d = 2 diag: NU = 5): a wavefront is 64 / LG lane groups, each
// taking its own pair (group g of wave w: pairs w G + g, + 4 G, ...), so a pair
// no longer leaves 59 of 64 lanes idle.  Per group a private LDS slab; the groups
// and waves reduce in fixed order (bit-reproducible), output as stats_list_u_kernel.
template <int LG, int SM>
__global__ __launch_bounds__(64 * kSuWaves) void stats_list_g_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  constexpr int NG = 64 / LG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane / LG, gl = lane - grp * LG;
  const int K = p.K, S = p.S, SB = p.SB, d = p.d, NU = p.NU, kq = p.ukdp / 4;
  const bool full = p.covmode == kCovFull;
  const int NPF = full ? d * (d + 1) / 2 : d;
  const int j = blockIdx.y, c = blockIdx.x, nch = gridDim.x;
  const int OT = S * SB, TS = (OT + 1) / 2 * 2, KP = p.ukdp + 1;
  const int WS = TS + (SB * KP + 1) / 2 * 2;
  double *tw = lds + (size_t)(wave * NG + grp) * WS;   // [SB][S] Z tnu of the group's pair
  double *uw = tw + TS;                                 // [SB][KP] its U columns
  double *red = lds + (size_t)kSuWaves * NG * WS;      // [S][NU] | [S] | [S][S]
  double *zs = red + (size_t)S * NU + S + S * S;       // [d]
  for (int a = tid; a < d; a += 64 * kSuWaves) zs[a] = p.uz[a];
  const bool fv = gl < NU;
  const int ue = gl == 0 ? -1 : gl <= d ? NPF + gl - 1 : gl - 1 - d;
  double acc[SM], accx[4], accn = 0.0;
#pragma unroll
  for (int s2 = 0; s2 < SM; ++s2) acc[s2] = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) accx[e] = 0.0;
  const int tot = p.list_tot[j];
  const int n0 = (int)((long long)tot * c / nch), n1 = (int)((long long)tot * (c + 1) / nch);
  const int *lst = p.list + (size_t)j * p.list_cap;
  const double *Ub0 = p.U + kUHead;
  const int nu4 = 4 * kq * SB;
  // wave-uniform trip count; a group past the part's end stages a zero-weight copy
  for (int nb = n0 + wave * NG; nb < n1; nb += kSuWaves * NG) {
    const int n = nb + grp;
    const bool pv = n < n1;
    const int i = lst[pv ? n : n0];
    const size_t lp = (size_t)(i - p.i_buf0) * K + j;
    const double z = pv ? p.Z[lp] : 0.0;
    double tv[4], xv[4], uv[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = gl + LG * e;
      tv[e] = x < OT ? p.tnu[lp * OT + x] : 0.0;
      xv[e] = x < S * S ? p.xi[lp * S * S + x] : 0.0;
    }
    const double nv = gl < S ? p.nu1[lp * S + gl] : 0.0;
    const long long c0 = (long long)i * SB - p.u_col0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int x = gl + LG * e;
      const int t4 = x / SB, b = x - t4 * SB;
      const long long col = c0 + b;
      uv[e] = x < nu4 ? Ub0[(size_t)(col >> 4) * kq * 64 + (t4 >> 2) * 64 + (t4 & 3) * 16 + (col & 15)]
                      : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = gl + LG * e;
      if (x < OT) {
        const int s2 = x / SB, b = x - s2 * SB;
        tw[b * S + s2] = z * tv[e];
      }
      accx[e] = fma(z, xv[e], accx[e]);
    }
    accn = fma(z, nv, accn);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int x = gl + LG * e;
      const int t4 = x / SB, b = x - t4 * SB;
      if (x < nu4) uw[b * KP + t4] = uv[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (fv) {
#pragma unroll 1
      for (int b = 0; b < SB; ++b) {
        const double u = ue < 0 ? 1.0 : uw[b * KP + ue];
#pragma unroll
        for (int s2 = 0; s2 < SM; ++s2)
          if (s2 < S) acc[s2] = fma(tw[b * S + s2], u, acc[s2]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // fixed-order reduction: waves in order, and within a wave its groups in order
  // (exec-masked stores of one wavefront retire in program order)
  for (int w = 0; w < kSuWaves; ++w) {
    if (wave == w) {
      for (int g = 0; g < NG; ++g) {
        if (grp == g) {
          const bool first = w == 0 && g == 0;
#pragma unroll
          for (int s2 = 0; s2 < SM; ++s2)
            if (fv && s2 < S) {
              double *r = red + (size_t)s2 * NU + gl;
              *r = first ? acc[s2] : *r + acc[s2];
            }
          if (gl < S) {
            double *r = red + (size_t)S * NU + gl;
            *r = first ? accn : *r + accn;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = gl + LG * e;
            if (x < S * S) {
              double *r = red + (size_t)S * NU + S + x;
              *r = first ? accx[e] : *r + accx[e];
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
    __syncthreads();
  }
  su_output(p, red, zs, c, nch, j, tid);
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
hipError_t launch_gate_list(const StatsArgs &a, int nchunk, hipStream_t st) {
  // (above 64 KB the launch needs the attribute)
  const size_t lds = gate_list_lds(a.K);
  if (a.gmask && a.K > 64) return hipErrorInvalidValue;
  // (with masks the gate is in them: one instantiation serves both modes)
  auto *fn = a.gmask ? &gate_list_kernel<kGateVbhem, true>
             : a.vhem ? &gate_list_kernel<kGateVhem, false>
                      : &gate_list_kernel<kGateVbhem, false>;
  hipError_t e = set_dyn_lds(reinterpret_cast<const void *>(fn), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(nchunk), dim3(kListThreads), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_stats_list(const StatsArgs &a, const GatedPlan &gp, hipStream_t st) {
  StatsKernel fn = nullptr;
  // (the state-count bucket SM of the prepared-operand kernels: one ladder for both)
  auto with_sm = [&](auto kernel_of) { return pick_kernel<4, 8, 12, 16>(gp.SM, kernel_of); };
  switch (gp.kernel) {
    case GatedStats::kMfma: fn = stats_mfma_kernel(gp); break;
    case GatedStats::kGrouped:
      fn = pick_kernel<8, 16, 32>(gp.LG, [&](auto lg) {
        return with_sm([](auto sm) { return stats_list_g_kernel<decltype(lg)::value, decltype(sm)::value>; });
      });
      break;
    case GatedStats::kOperand:
      fn = with_sm([](auto sm) { return stats_list_u_kernel<1, decltype(sm)::value>; });
      break;
    case GatedStats::kGather: fn = gp.PER == 4 ? stats_list_kernel<4> : stats_list_kernel<8>; break;
    case GatedStats::kList4Reduce: break;  // (launch_list4_stats_reduce: it takes the partials)
  }
  if (!gp.ok || !fn) return hipErrorInvalidValue;
  if (gp.exact_first) {
    hipError_t e = launch_fb_exact(a.fx, a.xscratch, (size_t)a.xstride, kExactSlots, st, true);
    if (e != hipSuccess) return e;
  }
  StatsArgs b = a;
  b.nzero = gp.nzero;
  hipError_t e = set_dyn_lds(reinterpret_cast<const void *>(fn), gp.lds);
  if (e != hipSuccess) return e;
  dim3 grid(gp.cap, a.K);  // block (c, j): part c of cluster j's list
  const int threads = gp.kernel == GatedStats::kGather ? kSlThreads : 64 * kSuWaves;
  if (gp.kernel == GatedStats::kMfma) {  // one 1-D grid over all clusters' parts
    const int per_cu = resident_per_cu(reinterpret_cast<const void *>(fn), threads, gp.lds);
    grid = dim3(stats_m_blocks((long long)per_cu * device_cus(), a.K, gp.cap, switches()));
  }
  hipLaunchKernelGGL(fn, grid, dim3(threads), gp.lds, st, b);
  return hipGetLastError();
}

}  // namespace vbhem
