// vbhem_fb_list4.hip -- the gated schedule's second pass (both sweeps, K2-K4 of
// mex.c:915-1298, for the pairs of the gate lists) for S = 8 cluster states, SB <= 8
// and T = 10, with every contraction on the fp64 matrix cores
// (v_mfma_f64_4x4x4f64) in the P / Q layouts of vbhem_mfma4.h.
//
// One wavefront takes a quad: 4 consecutive entries of one cluster's gate list (4
// bases, the 4 MFMA blocks).  Per quad:
//   backward  as fb_bwd4_kernel (G = exp(V - M), Z^T = G^T A'^T, sv = M + log Z,
//             V = Ef + sv Ab^T), keeping G_t of every step in registers (the lattice:
//             T - 1 slices of 4 doubles per lane);
//   K3        nu_1 = prior exp(lpi + V - logsumexp_sigma), sum_nu_1 = sum_beta nu_1;
//   forward   with nu and the other per-step matrices kept transposed (beta-first):
//               f^T = Ab^T nu^T             (nu Ab, the base transitions)
//               Z^T = G^T A'^T              (recomputed: the backward's Z)
//               g^T = f^T / Z^T
//               H  += g G^T                 (sum_xi before the A' factor)
//               Qm^T = g^T A'               (g transposed once per step)
//               nu^T = G^T o Qm^T,  sum_t nu^T += nu^T
//             -- 32 MFMAs per quad and step, two per-pair transposes (G -> G^T,
//             g^T -> g) through ds_bpermute, and a reciprocal;
//   outputs   sum_nu_1 [S], sum_t_nu [S][SB], sum_xi = A' o H [S][S] per pair.
// An item's inputs are loaded during the previous item's forward sweep (C4 list pass
// 0.240 -> 0.206 ms, profiles/r05v_ab_c4_list4_prefetch.txt).
// The fallback flags are fb_bwd4_kernel's (underflow of Z, |V| range, non-finite
// inputs); a flagged pair is recomputed by the wave itself after its item loop
// (xinline: queued in LDS; no fb_exact_kernel launch after the pass) or by the exact
// kernel.
// The sums (ACC; SplitArgs::acc, needs xinline): instead of the per-pair outputs the wave
// accumulates the gated statistics of its items in LDS -- Z nu_1, Z (A' o H) and, on the
// matrix cores, (Z sum_t_nu) Us against the base's statistic features (the quad's tnT
// blocks are the A operands as they stand, a 512-byte segment of Us the B operand of all
// four MFMA blocks, one pair's A copied to the four blocks by ds_bpermute) -- over a
// contiguous range of items, and flushes one partial per cluster of the range
// (vbhem_list4_slots.h) for list4_stats_reduce_kernel.  A flagged pair is added from its
// exact values, by the wave that queued it.  C4: list pass 0.208 -> 0.226 ms, statistics
// kernels 0.153 -> 0.049 ms (profiles/r07a_ab_c4_list4_stats.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "vbhem_exact.h"
#include "vbhem_internal.h"
#include "vbhem_math.h"
#include "vbhem_mfma4.h"

// (The backward half keeps the round-3 step on 32 KB of tables -- 2^(j/2048) and the
// 1024-interval log -- two 4-wave blocks per CU: fb_bwd4_kernel's larger-table step
// measured no gain here, 0.242 vs 0.244 ms at C4 (profiles/r04e_ab_l4r4_c4.txt), since
// the forward sweep sets this kernel's time.)

namespace vbhem {

namespace {
using namespace m4;
constexpr int kL4Waves = 2;   // waves per SIMD (the lattice is 72 VGPRs)
constexpr int kL4NWB = 4;    // waves per block
constexpr int kL4T = 10;      // the tau this kernel is built for (C3 - C5)
}  // namespace
constexpr int kL4XQ = 1024;   // flagged pairs queued per wave (xinline; list4_xq_fits)
namespace {
// ACC: a wave's accumulators in LDS, doubles: the (Z sum_t_nu) Us tiles [2 I][3 F'][64
// lanes] and Z (A' o H) [2 I][2 I'][64 lanes] in the lanes that compute them, then Z nu_1
// [2 I][4 r][4 pairs] and the item's own nu_1 sums (kept from K3 to the epilogue here,
// not in registers)
constexpr int kL4AccM = 2 * kL4sMaxTiles * 64, kL4AccN = kL4AccM + 4 * 64, kL4AccS = kL4AccN + 32;
constexpr int kL4AccLen = kL4AccS + 32;
// the forward steps at which the Us operands of pairs 0, 1 and of pairs 2, 3 are
// requested (T1 >= T: after the sweep); build switches for A/B
#ifndef VBHEM_L4_US_T0
#define VBHEM_L4_US_T0 8
#endif
#ifndef VBHEM_L4_US_T1
#define VBHEM_L4_US_T1 10
#endif

// ---- ACC: the sums of fb_list4_kernel<T, FAST, true> (lane = 16 r + 4 b + c) ----
// a wave's own LDS exchange: program order, writes visible to its other lanes
__device__ __forceinline__ void l4_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// base i's statistic features as the B operands of the tile MFMAs: ub[F'][J] = element
// `lane` of the 512-byte segment (feature tile F', base states 4 J .. 4 J + 3) of its Us
// block, i.e. Us(b = 4 J + r, f = 16 F' + 4 q + c) in block q.  Tiles and slices the
// shape does not have repeat an existing one (no branch around a load; their products
// are never flushed, or meet a zero A operand)
__device__ __forceinline__ void l4_load_us(const SplitArgs &p, int i, int sbp, int ntile, int lane,
                                           double (&ub)[kL4sMaxTiles][2]) {
  const double *us = p.accUs + (size_t)i * sbp * p.acc_nup + lane;
#pragma unroll
  for (int f = 0; f < kL4sMaxTiles; ++f)
#pragma unroll
    for (int J = 0; J < 2; ++J) ub[f][J] = us[((f < ntile ? f : ntile - 1) * sbp + (4 * J < sbp ? 4 * J : 0)) * 16];
}
// U tile (I, F') += sum over the NP pair slots and J of (Z tn)^T block (J, I) of the pair,
// copied into all four MFMA blocks, times ub[pair][F'][J]: lane (r, q, c) holds
// (sigma = 4 I + r, f = 16 F' + 4 q + c).  za: this lane's pair's Z tn^T blocks, zero
// where the pair does not count
template <int NP>
__device__ __forceinline__ void l4_acc_u(double *accw, const double (&za)[2][2],
                                         const double (&ub)[NP][kL4sMaxTiles][2], int r, int c, int lane) {
  double acc[2][kL4sMaxTiles];
#pragma unroll
  for (int I = 0; I < 2; ++I)
#pragma unroll
    for (int f = 0; f < kL4sMaxTiles; ++f) acc[I][f] = accw[(I * kL4sMaxTiles + f) * 64 + lane];
#pragma unroll
  for (int pp = 0; pp < NP; ++pp) {
    const int src = (16 * r + 4 * pp + c) << 2;
#pragma unroll
    for (int J = 0; J < 2; ++J)
#pragma unroll
      for (int I = 0; I < 2; ++I) {
        const double xa = bperm_d(src, za[J][I]);
#pragma unroll
        for (int f = 0; f < kL4sMaxTiles; ++f) acc[I][f] = mfma4(xa, ub[pp][f][J], acc[I][f]);
      }
  }
#pragma unroll
  for (int I = 0; I < 2; ++I)
#pragma unroll
    for (int f = 0; f < kL4sMaxTiles; ++f) accw[(I * kL4sMaxTiles + f) * 64 + lane] = acc[I][f];
}
// Z nu_1 (lanes c == 0: sigma = 4 I + r of pair b) and Z (A' o H) (every lane: (4 I + r,
// 4 I' + c) of pair b), kept per pair slot
__device__ __forceinline__ void l4_acc_nm(double *accw, const double (&n1)[2], const double (&xm)[2][2],
                                          int r, int b, int c, int lane) {
#pragma unroll
  for (int I = 0; I < 2; ++I) {
    if (c == 0) accw[kL4AccN + 16 * I + 4 * r + b] += n1[I];
#pragma unroll
    for (int I2 = 0; I2 < 2; ++I2) accw[kL4AccM + (2 * I + I2) * 64 + lane] += xm[I][I2];
  }
}
// the wave's sums to partial `slot` (U [S][NUP] | N1 [S] | M [S][S]; written, or added by
// the lanes that wrote it), the pair slots of N1 and M folded in slot order; zeroed after
__device__ __forceinline__ void l4_flush(const SplitArgs &p, double *accw, int slot, bool add, int ntile,
                                         int lane) {
  constexpr int S = 8;
  const int nup = p.acc_nup, r = lane >> 4, b = (lane >> 2) & 3, c = lane & 3;
  double *part = p.acc_parts + (size_t)slot * l4s_part_len(S, nup);
  auto put = [add](double *dst, double v) { *dst = add ? *dst + v : v; };
#pragma unroll
  for (int I = 0; I < 2; ++I)
#pragma unroll
    for (int f = 0; f < kL4sMaxTiles; ++f) {
      double *a = accw + (I * kL4sMaxTiles + f) * 64 + lane;
      if (f < ntile) put(part + (4 * I + r) * nup + 16 * f + 4 * b + c, *a);
      *a = 0.0;
    }
  l4_wsync();
  {  // M entry (sigma, sigma') = (lane >> 3, lane & 7)
    const double *a = accw + kL4AccM + (2 * (lane >> 5) + ((lane >> 2) & 1)) * 64 + 16 * ((lane >> 3) & 3) + (lane & 3);
    put(part + S * nup + S + lane, ((a[0] + a[4]) + a[8]) + a[12]);
  }
  if (lane < S) {  // N1 entry sigma = lane
    const double *a = accw + kL4AccN + 16 * (lane >> 2) + 4 * (lane & 3);
    put(part + S * nup + lane, ((a[0] + a[1]) + a[2]) + a[3]);
  }
  l4_wsync();
#pragma unroll
  for (int x = 0; x < 4; ++x) accw[kL4AccM + 64 * x + lane] = 0.0;
  if (lane < 32) accw[kL4AccN + lane] = 0.0;
  l4_wsync();
}
}  // namespace

// FAST: SB == 8 (no clamp or zero select in the item's addresses and operands) and
// 32-bit load offsets (A, the prior and E below 4 GB), as fb_bwd4_kernel<O32>
// ACC: the gated statistics accumulated here (SplitArgs::acc; the header's "sums" below)
template <int T, bool FAST, bool ACC>
__global__ __launch_bounds__(64 * kL4NWB) __attribute__((amdgpu_waves_per_eu(kL4Waves)))
void fb_list4_kernel(const SplitArgs p) {
  constexpr int S = 8;
  __shared__ __attribute__((aligned(16))) double etab[2048];
  __shared__ __attribute__((aligned(16))) double ltab[2 * 1024];
  __shared__ int pre[kList4MaxK + 1];  // first quad item of every cluster
  __shared__ int tots[kList4MaxK];     // the gate lists' lengths
  __shared__ int xq[kL4NWB * kL4XQ];   // per wave: its flagged pairs (xinline)
  __shared__ __attribute__((aligned(16))) double accs[ACC ? kL4NWB * kL4AccLen : 1];
  const int tid = threadIdx.x;
  stage_tables(etab, ltab, tid, 64 * kL4NWB);
  if constexpr (ACC)  // every wave's sums
    for (int x = tid; x < kL4NWB * kL4AccLen; x += 64 * kL4NWB) accs[x] = 0.0;
  const int K = p.K, SB = FAST ? 8 : p.SB;
  using off_t_ = typename std::conditional<FAST, unsigned, size_t>::type;
  auto ld = [](const double *base, off_t_ x) {
    if constexpr (FAST)
      return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + x * 8u);
    else
      return base[x];
  };
  if (tid == 0) {
    int s = 0;
    for (int jj = 0; jj < K; ++jj) {
      const int t = p.list_tot[jj];
      pre[jj] = s;
      tots[jj] = t;
      s += (t + 3) / 4;
    }
    pre[K] = s;
  }
  __syncthreads();
  const int nitem = __builtin_amdgcn_readfirstlane(pre[K]);
  const double vlim = kVMax / (double)T - 3.0;
  // (ACC: the wave index in an SGPR -- its item range and slots are scalar then)
  const int gw = ACC ? __builtin_amdgcn_readfirstlane((int)blockIdx.x * kL4NWB + (tid >> 6))
                     : (int)blockIdx.x * kL4NWB + (tid >> 6),
            nw = (int)gridDim.x * kL4NWB;

  // An item's global inputs (A in both layouts, E, the prior) are loaded during the
  // previous item's forward sweep, once its first lattice slices are dead (no extra
  // registers), and the item's gate-list entries at the previous item's start: an
  // item starts with its inputs in registers instead of two dependent memory
  // latencies (list entry, then inputs).  Clamped addresses; the selects on the loaded
  // values only where the item uses them.
  struct ItemIn {
    double ab[2][2], e[2][2], pr[2], af[2][2];
  };
  auto load_in = [&](int i, int jj, int r_, int c_, ItemIn &in) {
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
      for (int j3 = 0; j3 < 2; ++j3) {
        const int be = 4 * j3 + c_, bp = 4 * j2 + r_;
        const int bec = be < SB ? be : SB - 1, bpc = bp < SB ? bp : SB - 1;
        in.ab[j2][j3] = ld(p.A, ((off_t_)i * SB + bec) * SB + bpc);
        in.af[j2][j3] = ld(p.A, ((off_t_)i * SB + bpc) * SB + bec);
      }
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int j3 = 0; j3 < 2; ++j3) {
        const int be = 4 * j3 + c_;
        in.e[i2][j3] = ld(p.E, (off_t_)(jj * S + 4 * i2 + r_) * (off_t_)p.e_ld + (off_t_)(i - p.i_buf0) * SB +
                                   (be < SB ? be : SB - 1));
      }
#pragma unroll
    for (int j3 = 0; j3 < 2; ++j3) {
      const int be = 4 * j3 + c_;
      in.pr[j3] = ld(p.prior, (off_t_)i * SB + (be < SB ? be : SB - 1));
    }
  };
  // the base of pair b of item it (cluster jj; past the list's end: the quad's first)
  auto base_of = [&](int it, int jj, int b_) -> int {
    const int n0 = (it - pre[jj]) * 4;
    const int tot = tots[jj];
    return p.list[(size_t)jj * p.list_cap + (n0 + b_ < tot ? n0 + b_ : n0)];
  };
  int js = 0, jsn = 0, nq = 0;
  ItemIn cur;
  int icur = 0;
  // the wave's items: gw, gw + nw, ...; ACC: the contiguous range [gw per, (gw + 1) per)
  // (vbhem_list4_slots.h), so that its sums change cluster, and are flushed, rarely
  const int per = ACC ? l4s_per_wave(nitem, nw) : 1;
  const int it0 = ACC ? gw * per : gw, itend = ACC ? min(nitem, it0 + per) : nitem;
  const int istep = ACC ? 1 : nw;
  if (it0 < itend) {
    const int lane = tid & 63;
    while (pre[js + 1] <= it0) ++js;
    jsn = js;
    icur = base_of(it0, __builtin_amdgcn_readfirstlane(js), (lane >> 2) & 3);
    load_in(icur, __builtin_amdgcn_readfirstlane(js), lane >> 4, lane & 3, cur);
  }
  for (int it = it0; it < itend; it += istep) {
    // lane geometry recomputed per item from an opaque copy of the thread id, so that
    // no lane-invariant address is hoisted out of the item loop (such live ranges
    // spilled to scratch at 256 VGPRs)
    int tq = tid;
    asm volatile("" : "+v"(tq));
    const int lane = tq & 63;
    const int r = lane >> 4, b = (lane >> 2) & 3, c = lane & 3;
    double *const accw = accs + (ACC ? (tq >> 6) * kL4AccLen : 0);  // ACC: this wave's sums
    const int qsrc0 = (4 * b + r) << 2, qsrc1 = (16 + 4 * b + r) << 2;
    const int taddr = (16 * c + 4 * b + r) << 2;
    const unsigned long long pmask = 0x000F000F000F000Full << (4 * b);
    const int j = __builtin_amdgcn_readfirstlane(js);  // (js: advanced to it)
    // the next item (a repeat of this one past the end): its cluster and list entry now
    const int itn = min(it + istep, itend - 1);
    while (pre[jsn + 1] <= itn) ++jsn;
    const int jn = __builtin_amdgcn_readfirstlane(jsn);
    const int inext = base_of(itn, jn, b);
    // the cluster's constants, loaded per item (cache hits; holding them across items
    // spilled 17 values to scratch): A'^T as the B operand of Z^T (block (K, I'):
    // A'[4I' + c][4K + r]), A' in P (A'[4I + r][4I' + c]), amax (rows 4I + c), lpi
    double AT[2][2], Ap[2][2], amQ[2], lpP[2];
    bool cl_nf;
    {
      const double *At = p.Atg + (size_t)j * S * S;
      bool nf = false;
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
          AT[x][y] = At[(4 * y + c) * S + 4 * x + r];
          Ap[x][y] = At[(4 * x + r) * S + 4 * y + c];
        }
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const double *la = p.logA + ((size_t)j * S + 4 * i2 + r) * S;  // (P rows: the fma below)
        double mx = la[0];
#pragma unroll
        for (int s2 = 1; s2 < S; ++s2) mx = fmax(mx, la[s2]);
        amQ[i2] = mx;
        lpP[i2] = p.logPi[(size_t)j * S + 4 * i2 + r];
        nf |= isnan(mx) || isnan(lpP[i2]);
      }
      cl_nf = __ballot(nf) != 0;
    }
    const int n0 = (it - pre[j]) * 4;
    const int tot = tots[j];
    const bool act = n0 + b < tot;
    const int i = icur;
    const size_t lp = (size_t)(i - p.i_buf0) * K + j;

    // ---- per-pair inputs: Ab^T as the backward's B operand, E, Ef ----
    double AbT[2][2], Ef[2][2], V[2][2];
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int be = 4 * jj + c, bp = 4 * j2 + r;
        AbT[j2][jj] = (be < SB && bp < SB) ? cur.ab[j2][jj] : 0.0;
      }
    bool nfp = false;
    uint64_t bigm = 0;  // the lanes failing the range check (ordered compares into a mask)
    // Ef = E + amax[sigma] rowsum(Ab)[beta]: one fma per element from the row sums
    // (as fb_bwd4_kernel; amQ holds the P rows 4I + r here)
    double rsj[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) rsj[jj] = mfma4(1.0, AbT[1][jj], mfma4(1.0, AbT[0][jj], 0.0));
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const double e = cur.e[i2][jj];
        V[i2][jj] = e;
        Ef[i2][jj] = fma(amQ[i2], rsj[jj], e);
        bigm |= ge_mask(fabs(e), vlim) | ge_mask(fabs(Ef[i2][jj]), vlim);
        nfp |= !isfinite(Ef[i2][jj]);
      }
    bigm |= gt_mask(rsj[0], 1.0 + 1e-6) | gt_mask(rsj[1], 1.0 + 1e-6);
    const bool rbad = lane_in(bigm);
    int zmin = 0x7fffffff;

    // ---- K2: backward recursion (fb_bwd4_kernel's round-3 step), G_t kept for the forward ----
    double lat[T][2][2];
#pragma unroll
    for (int t = T - 1; t >= 1; --t) {
      double s[2][2];
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) s[i2][jj] = red_s(V[i2][jj]);
      const unsigned w = colmax_rows(max(lo_u(s[0][0]), lo_u(s[1][0])), max(lo_u(s[0][1]), lo_u(s[1][1])));
      const int wq = (int)(w + kWq0);
      const int mq[2] = {__builtin_amdgcn_ds_bpermute(qsrc0, wq), __builtin_amdgcn_ds_bpermute(qsrc1, wq)};
      unsigned wp[2];
      split_rows(w - kBias, wp[0], wp[1]);
      {
        const double vf[4] = {V[0][0], V[0][1], V[1][0], V[1][1]};
        const double sf[4] = {s[0][0], s[0][1], s[1][0], s[1][1]};
        const unsigned wpf[4] = {wp[0], wp[1], wp[0], wp[1]};
        double gf[4];
        exp_m_n<4>(gf, vf, sf, wpf, etab);
        lat[t][0][0] = gf[0]; lat[t][0][1] = gf[1]; lat[t][1][0] = gf[2]; lat[t][1][1] = gf[3];
      }
      double z[4];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2)
          z[2 * jj + i2] = mfma4(lat[t][1][jj], AT[1][i2], mfma4(lat[t][0][jj], AT[0][i2], 0.0));
      zmin = min(zmin, min(min(__double2hiint(z[0]), __double2hiint(z[1])),
                           min(__double2hiint(z[2]), __double2hiint(z[3]))));
      double svf[4];
      {
        const int wqf[4] = {mq[0], mq[0], mq[1], mq[1]};
        log_m_n<4>(svf, z, wqf, ltab);
      }
      // sv(I, J') is Z^T's block (J', I) = svf[2 J' + I]
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          V[i2][jj] = mfma4(svf[2 + i2], AbT[1][jj], mfma4(svf[i2], AbT[0][jj], Ef[i2][jj]));
    }

    // ---- K3: nu_1 = prior exp(lpi + V - logsumexp over sigma), sum_nu_1 ----
    double nu[2][2];
    bool bad;
    {
      double W[2][2], s[2][2];
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          W[i2][jj] = fmax(lpP[i2] + V[i2][jj], -7.2e5);
          s[i2][jj] = red_s(W[i2][jj]);
        }
      const unsigned w = colmax_rows(max(lo_u(s[0][0]), lo_u(s[1][0])), max(lo_u(s[0][1]), lo_u(s[1][1])));
      unsigned wp[2];
      split_rows(w - kBias, wp[0], wp[1]);
      double ev[4];
      {
        const double wf[4] = {W[0][0], W[0][1], W[1][0], W[1][1]};
        const double sf[4] = {s[0][0], s[0][1], s[1][0], s[1][1]};
        const unsigned wpf[4] = {wp[0], wp[1], wp[0], wp[1]};
        exp_m_n<4>(ev, wf, sf, wpf, etab);
      }
      // row r: column 4 (r & 1) + c (w's layout), then both column blocks in every row
      const double zs = colsum_rows(ev[0] + ev[2], ev[1] + ev[3]);
      double lser[1];
      {
        const double zsf[1] = {zs};
        const int wqf[1] = {(int)(w + kWq0)};
        log_m_n<1>(lser, zsf, wqf, ltab);
      }
      bad = zmin < kZMinHi || rbad || !isfinite(lser[0]);
      const auto sl = __builtin_amdgcn_permlane16_swap(lo_u(lser[0]), lo_u(lser[0]), false, false);
      const auto sh = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(lser[0]),
                                                       (unsigned)__double2hiint(lser[0]), false, false);
      const double lse[2] = {__hiloint2double((int)sh[0], (int)sl[0]), __hiloint2double((int)sh[1], (int)sl[1])};
      double xf[4], sf[4], ef[4];
      unsigned wpf[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        xf[x] = fmax(W[x / 2][x % 2] - lse[x % 2], -7.0e5);  // (in the integer range)
        sf[x] = red_s(xf[x]);
        wpf[x] = 2147483648u - kBias;  // m = 0
      }
      exp_m_n<4>(ef, xf, sf, wpf, etab);
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int be = 4 * jj + c;
        const double pb = be < SB ? cur.pr[jj] : 0.0;
        nu[0][jj] = pb * ef[jj];
        nu[1][jj] = pb * ef[2 + jj];
      }
      // sum_nu_1[sigma = 4I + r]: over the column blocks, then the 4 lanes c
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        double a = nu[i2][0] + nu[i2][1];
        a += shfl_xor_d(a, 1);
        a += shfl_xor_d(a, 2);
        if constexpr (ACC) {
          if (c == 0) accw[kL4AccS + 16 * i2 + 4 * r + b] = a;  // (read back by this lane)
        } else {
          if (act && c == 0) p.nu1[lp * S + 4 * i2 + r] = a;
        }
      }
    }

    // ---- K4: forward recursion, beta-first ----
    double AbF[2][2];  // Ab in P (Ab[4J' + r][4J + c]): f^T = Ab^T nu^T
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int bp = 4 * j2 + r, be = 4 * jj + c;
        AbF[j2][jj] = (be < SB && bp < SB) ? cur.af[j2][jj] : 0.0;
      }
    ItemIn nxt;
    // ACC: the pair's weight, and the four bases' Us operands: loaded into the registers
    // of dead lattice slices during the last forward steps (two pairs) and after them
    double zc = 0.0, ub[ACC ? 4 : 1][kL4sMaxTiles][2];
    const int sbp = us_sbp(SB), ntile = ACC ? p.acc_nup / 16 : 1;
    if constexpr (ACC) zc = p.accZ[lp];
    double nuT[2][2], tnT[2][2], H[2][2];
    transpose8(nu, nuT, taddr);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        tnT[x][y] = nuT[x][y];
        H[x][y] = 0.0;
      }
#pragma unroll
    for (int t = 1; t < T; ++t) {
      // the next item's inputs, into the registers of the lattice slices 1 .. T/2 - 1
      if (t == T / 2) load_in(inext, jn, r, c, nxt);
      if constexpr (ACC)
        if (t == VBHEM_L4_US_T0) {
          l4_load_us(p, __builtin_amdgcn_readlane(i, 0), sbp, ntile, lane, ub[0]);
          l4_load_us(p, __builtin_amdgcn_readlane(i, 4), sbp, ntile, lane, ub[1]);
        }
      if constexpr (ACC)
        if (t == VBHEM_L4_US_T1) {
          l4_load_us(p, __builtin_amdgcn_readlane(i, 8), sbp, ntile, lane, ub[2]);
          l4_load_us(p, __builtin_amdgcn_readlane(i, 12), sbp, ntile, lane, ub[3]);
        }
      double Gt[2][2];
      transpose8(lat[t], Gt, taddr);
      // f^T block (J, I) = sum_J' Ab(J', J)^T nu^T(J', I); Z^T block (J, I') as the backward's
      double fT[2][2], ZT[2][2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2) {
          fT[jj][i2] = mfma4(AbF[1][jj], nuT[1][i2], mfma4(AbF[0][jj], nuT[0][i2], 0.0));
          ZT[jj][i2] = mfma4(lat[t][1][jj], AT[1][i2], mfma4(lat[t][0][jj], AT[0][i2], 0.0));
        }
      double gT[2][2];
      {
        const double zf[4] = {ZT[0][0], ZT[0][1], ZT[1][0], ZT[1][1]};
        double rz[4];
        rcp_pos_n<4>(rz, zf);
        gT[0][0] = fT[0][0] * rz[0]; gT[0][1] = fT[0][1] * rz[1];
        gT[1][0] = fT[1][0] * rz[2]; gT[1][1] = fT[1][1] * rz[3];
      }
      // H block (I, I') += sum_J gT(J, I)^T G^T(J, I')
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int i3 = 0; i3 < 2; ++i3) H[i2][i3] = mfma4(gT[1][i2], Gt[1][i3], mfma4(gT[0][i2], Gt[0][i3], H[i2][i3]));
      double g[2][2];
      transpose8(gT, g, taddr);
      // Qm^T block (J, I') = sum_I g(I, J)^T A'(I, I'); nu^T = G^T o Qm^T
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int i3 = 0; i3 < 2; ++i3) {
          const double qm = mfma4(g[1][jj], Ap[1][i3], mfma4(g[0][jj], Ap[0][i3], 0.0));
          nuT[jj][i3] = Gt[jj][i3] * qm;
          tnT[jj][i3] += nuT[jj][i3];
        }
    }

    // ---- outputs and fallback flags ----
    const bool pbad = (__ballot(bad) & pmask) != 0;
    const bool pnf = cl_nf || (__ballot(nfp) & pmask) != 0;
    if constexpr (ACC) {
      // the sums: a pair slot past the list's end, or flagged for the exact recursion
      // (counted below from its exact values), has its operands selected to zero -- not
      // multiplied: a flagged pair's fast values may be non-finite
      if (VBHEM_L4_US_T1 >= T) {
        l4_load_us(p, __builtin_amdgcn_readlane(i, 8), sbp, ntile, lane, ub[2]);
        l4_load_us(p, __builtin_amdgcn_readlane(i, 12), sbp, ntile, lane, ub[3]);
      }
      const bool use = act && !(pbad && !pnf);
      double za[2][2], xm[2][2], n1[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        n1[x] = use ? zc * accw[kL4AccS + 16 * x + 4 * r + b] : 0.0;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
          // tnT block (J = x, I = y): beta = 4 x + r; H block (I = x, I' = y)
          za[x][y] = (use && (FAST || 4 * x + r < SB)) ? zc * tnT[x][y] : 0.0;
          xm[x][y] = use ? zc * (Ap[x][y] * H[x][y]) : 0.0;
        }
      }
      l4_acc_nm(accw, n1, xm, r, b, c, lane);
      l4_acc_u<4>(accw, za, ub, r, c, lane);
      if (act && pbad && !pnf && lane == 4 * b) atomicAdd(p.flag_count + 1, 1);
      // the sums leave the wave at a cluster boundary and after its last item
      if (it + 1 >= itend || jn != j) l4_flush(p, accw, l4s_slot(it, j, per), false, ntile, lane);
    } else if (act) {
      // sum_t_nu[sigma][beta]: tnT block (J, I) lane (r, b, c) = tn[4I + c][4J + r]
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2) {
          const int be = 4 * jj + r;
          if (be < SB) p.tnu[(lp * S + 4 * i2 + c) * SB + be] = tnT[jj][i2];
        }
      // sum_xi = A' o H: H block (I, I') lane (r, b, c) = H[4I + r][4I' + c], as Ap
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int i3 = 0; i3 < 2; ++i3) p.xi[(lp * S + 4 * i2 + r) * S + 4 * i3 + c] = Ap[i2][i3] * H[i2][i3];
      if (pbad && !pnf && lane == 4 * b) {
        // underflow or range with finite inputs: the pair is recomputed by the exact
        // recursion -- below, by this wave (xinline), or by the exact kernel
        atomicAdd(p.flag_count + 1, 1);
        if (!p.xinline) {
          const int slot = atomicAdd(p.flag_count, 1);
          p.flag_list[slot] = (int)((size_t)i * K + j);
        }
      }
    }
    if (p.xinline) {
      // the wave's flagged pairs into its LDS queue (recomputed after the item loop)
      const unsigned long long fm = __ballot(act && pbad && !pnf && lane == 4 * b);
      if (fm) {
        const int l = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(fm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)fm, 0u));
        // (ACC: from the opaque copy -- the hoisted queue address was spilled to scratch)
        if (fm >> lane & 1) xq[((ACC ? tq : tid) >> 6) * kL4XQ + nq + l] = (int)((size_t)i * K + j);
        nq += __builtin_popcountll(fm);
      }
    }
    cur = nxt;
    icur = inext;
    js = jsn;
  }
  // the exact recursion of the wave's flagged pairs (SplitArgs::xinline: the host
  // inlines when every wave's queue bound fits and the grid has a scratch slot per
  // wave), after the item loop, where none of the loop's registers are live
  if (p.xinline) {
    const int *q = xq + (tid >> 6) * kL4XQ;
    for (int x = 0; x < nq; ++x) {
      const int pair = __builtin_amdgcn_readfirstlane(q[x]);
      exact_pair_wave<true>(p.xf, pair, p.xscr + (size_t)gw * p.xstride, nullptr);
      if constexpr (ACC) {
        // ACC: the pair's exact nu_1, xi and sum_t_nu read back from the workspace (other
        // lanes' stores: device-scope fence) as pair slot 0 of a quad and added to the
        // partial of its cluster, which the item loop wrote: counted once, in queue order
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        __builtin_amdgcn_wave_barrier();
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int lane = tq & 63, r = lane >> 4, b = (lane >> 2) & 3, c = lane & 3;
        double *const accw = accs + (tq >> 6) * kL4AccLen;
        const int i = pair / K, j = pair - i * K;
        const size_t lp = (size_t)(i - p.i_buf0) * K + j;
        const int sbp = us_sbp(SB), ntile = p.acc_nup / 16;
        const bool on = b == 0;
        const double zc = p.accZ[lp];
        double ub[1][kL4sMaxTiles][2], za[2][2], xm[2][2], n1[2];
        l4_load_us(p, i, sbp, ntile, lane, ub[0]);
#pragma unroll
        for (int x2 = 0; x2 < 2; ++x2) {
          n1[x2] = on ? zc * p.nu1[lp * S + 4 * x2 + r] : 0.0;
#pragma unroll
          for (int y = 0; y < 2; ++y) {
            const bool tv = on && 4 * x2 + r < SB;
            za[x2][y] = tv ? zc * p.tnu[(lp * S + 4 * y + c) * SB + 4 * x2 + r] : 0.0;
            xm[x2][y] = on ? zc * p.xi[(lp * S + 4 * x2 + r) * S + 4 * y + c] : 0.0;
          }
        }
        l4_acc_nm(accw, n1, xm, r, b, c, lane);
        l4_acc_u<1>(accw, za, ub, r, c, lane);
        const int jx = x + 1 < nq ? __builtin_amdgcn_readfirstlane(q[x + 1]) % K : -1;
        if (jx != j) l4_flush(p, accw, gw + j, true, ntile, lane);
      }
    }
  }
}

// ---------------------------------------------------------------------------
bool list4_supported(int S, int SB, int T, int K) {
  return S == 8 && SB >= 1 && SB <= 8 && T == kL4T && K >= 1 && K <= kList4MaxK;
}
bool list4_fast(const SplitArgs &a) {
  const unsigned long long lim = 0xffffffffull / 8;
  return a.SB == 8 && (unsigned long long)a.i_end * a.SB * a.SB < lim &&
         (unsigned long long)a.K * a.S * (unsigned long long)a.e_ld < lim;
}
long long list4_inline_waves(const SplitArgs &a, unsigned grid) {
  const long long nw = (long long)grid * kL4NWB;
  const long long items = (long long)a.K * ((a.i_end - a.i_begin + 3) / 4);  // all lists full
  if (nw < 1 || 4 * ((items + nw - 1) / nw) > kL4XQ) return 1ll << 40;
  return nw;
}
bool list4_acc_supported(int S, int SB, int T, int K, int NU) {
  return list4_supported(S, SB, T, K) && us_nup(NU) <= 16 * kL4sMaxTiles;
}
int list4_resident_blocks(bool acc) {
  auto *fn = acc ? &fb_list4_kernel<kL4T, true, true> : &fb_list4_kernel<kL4T, true, false>;
  return resident_per_cu(reinterpret_cast<const void *>(fn), 64 * kL4NWB, 0);
}
hipError_t launch_list4(const SplitArgs &a, unsigned grid, hipStream_t st) {
  if (!list4_supported(a.S, a.SB, a.T, a.K) || !a.Atg || !a.list || !a.list_tot) return hipErrorInvalidValue;
  auto *fn = list4_fast(a) ? &fb_list4_kernel<kL4T, true, false> : &fb_list4_kernel<kL4T, false, false>;
  if (a.acc) {
    // the sums need the inline fallback (a flagged pair is added from its exact values by
    // the wave that queued it), the operands and a partial per slot of this grid
    if (!a.xinline || !a.accZ || !a.accUs || !a.acc_parts || a.acc_nup < 16 || a.acc_nup % 16 ||
        a.acc_nup > 16 * kL4sMaxTiles)
      return hipErrorInvalidValue;
    fn = list4_fast(a) ? &fb_list4_kernel<kL4T, true, true> : &fb_list4_kernel<kL4T, false, true>;
  }
  hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * kL4NWB), 0, st, a);
  return hipGetLastError();
}

}  // namespace vbhem

extern "C" int vbhem_list4_stats_slot_plan(const int *tot, int K, int nw, int *per, int *first,
                                           int *count) {
  int nitem = 0;
  for (int j = 0; j < K; ++j) nitem += vbhem::l4s_items(tot[j]);
  const int pw = vbhem::l4s_per_wave(nitem, nw);
  if (per) *per = pw;
  int pre = 0;
  for (int j = 0; j < K; ++j) {
    const int n = vbhem::l4s_items(tot[j]);
    if (first) first[j] = n ? vbhem::l4s_slot(pre, j, pw) : 0;
    if (count) count[j] = n ? vbhem::l4s_slot(pre + n - 1, j, pw) - vbhem::l4s_slot(pre, j, pw) + 1 : 0;
    pre += n;
  }
  return nitem;
}
