// vbhem_estep_plan.h -- launch geometry of the E-step's recursion kernels: pairs
// per block, LDS carve-up, lanes per column, the persistent grid.  Arithmetic on
// sizes only, no HIP call: the scheduler (vbhem_estep_sched.hip), fb_split_kernel
// (SplitLayout) and the host check (tests/plancheck) share these definitions.
#pragma once
#include <algorithm>
#include <cstddef>
#include <type_traits>

#include "vbhem_internal.h"
#include "vbhem_exact.h"
#include "vbhem_math.h"

namespace vbhem {

constexpr size_t kLdsLimit = 160 * 1024;  // gfx950 LDS per workgroup
constexpr int kFbMaxThreads = 512;        // fb_pairs_kernel launch bound

// ---- fb_split_kernel (one base-state column per LPC lanes) ---------------------
constexpr bool split_supported(int S, int SB, int d) {
  return S >= 1 && S <= kSplitMaxS && SB >= 1 && SB <= S && d >= 1 && d <= 64;
}
// lanes per column of the dense / list modes
constexpr int split_lpc(int S) {
#ifdef VBHEM_SPLIT_LPC5  // A/B: at S = 5
  if (S == 5) return VBHEM_SPLIT_LPC5;
#endif
  return S <= 4 ? 1 : S <= 8 ? 2 : 4;
}
// the backward-only mode's alternative (no H / sum_t_nu registers: wider columns fit)
constexpr int split_lpc_bwd(int S) { return S <= 8 ? 1 : 2; }
template <int S>
using SplitLPC = std::integral_constant<int, split_lpc(S)>;
template <int S>
using BwdLPC = std::integral_constant<int, split_lpc_bwd(S)>;

// LDS layout (doubles): head | ppb per-pair slabs | Y | flags | region
constexpr int split_rows(int S, int LPC) { return (S + LPC - 1) / LPC; }  // rows per lane
constexpr int split_col_stride(int S, int LPC) {  // slab column stride (even)
  return (LPC * split_rows(S, LPC) + 1) / 2 * 2 + 2;
}
constexpr int split_pair_slab(int S, int LPC) { return S * split_col_stride(S, LPC) + 2; }
constexpr int split_head(int S) { return 2 * S * S + 2 * S; }  // At, AtT, amax, lpi
constexpr int split_off_x(int S) { return (split_head(S) + 1) / 2 * 2; }
template <int S, int LPC>
struct SplitLayout {
  static constexpr int SH = split_rows(S, LPC), XCS = split_col_stride(S, LPC);
  static constexpr int XP = split_pair_slab(S, LPC), HEAD = split_head(S), OFF_X = split_off_x(S);
};
// what depends on the waves per block
// (ppb: pairs per block, 0 when a pair needs more lanes; region: the lattice, or the
// parked H blocks of sum_xi for S > 8)
struct SplitOffsets {
  int ppb, off_Y, off_F, off_R, off_L;
  size_t region;
};
constexpr SplitOffsets split_offsets(int S, int LPC, int T, int nwb) {
  SplitOffsets o{};
  const int NT = nwb * 64, SH = split_rows(S, LPC);
  o.ppb = NT / (S * LPC);
  o.off_Y = split_off_x(S) + o.ppb * split_pair_slab(S, LPC);
  o.off_F = (o.off_Y + o.ppb * S + 1) / 2 * 2;
  o.off_R = (o.off_F + (o.ppb + 1) / 2 + 1) / 2 * 2;
  const size_t lattice = (size_t)std::max(0, T - 2) * SH * NT;
  const size_t xi_park = S > 8 ? (size_t)o.ppb * S * S * LPC * SH : 0;
  o.region = std::max<size_t>(std::max(lattice, xi_park), 2);
  o.off_L = (int)(o.off_R + o.region);
  return o;
}

struct SplitPlan {
  bool ok = false;
  SplitArgs a{};
  size_t lds = 0;       // kFbDense
  size_t lds_bwd = 0;   // kFbBackward (no lattice)
  size_t lds_list = 0;  // kFbList (lattice + work-item prefix)
  int ppb = 0;
  // kFbList: its own geometry (up to 8 waves per block, compact tables in LDS)
  SplitArgs al{};
  size_t lds_l = 0;
};

inline SplitPlan plan_split(int SB, int d, int covmode, int K, int S, int T, int LPC) {
  SplitPlan sp;
  if (!split_supported(S, SB, d)) return sp;
  const int LPP = S * LPC;
  double best = -1.0;
  for (int nwb = 1; nwb <= 4; ++nwb) {
    const SplitOffsets o = split_offsets(S, LPC, T, nwb);
    if (o.ppb < 1) continue;
    const size_t lds_list = ((size_t)o.off_L + ((size_t)K + 2) / 2) * sizeof(double);
    if (lds_list > kLdsLimit) continue;
    const double util = double(o.ppb * LPP) / (nwb * 64);
    if (util > best + 0.02 || (LPC != split_lpc(S) && util >= best)) {
      best = util;
      SplitArgs &x = sp.a;
      x.SB = SB; x.d = d; x.covmode = covmode; x.K = K; x.S = S; x.T = T; x.nwb = nwb;
      x.lpc = LPC;
      x.off_Y = o.off_Y; x.off_F = o.off_F; x.off_R = o.off_R; x.off_L = o.off_L;
      x.mode = kFbDense;
      sp.lds = ((size_t)o.off_R + o.region) * sizeof(double);
      x.off_T = o.off_R + 2;
      sp.lds_bwd = ((size_t)x.off_T + kLogTabDoubles + kExpTabDoubles) * sizeof(double);
      sp.lds_list = lds_list;
      sp.ppb = o.ppb;
      sp.ok = true;
    }
  }
  // list mode: the lattice dominates LDS and the kernel runs 2 waves per SIMD, so the
  // most waves per CU come from one 8-wave block (C4: 156 KB) rather than 4-wave
  // blocks that no longer pair up once the 4 KB of tables are added
  int best_w = 0;
  for (int nwb : {8, 4, 2, 1}) {
    if (!sp.ok) break;
    const SplitOffsets o = split_offsets(S, LPC, T, nwb);
    if (o.ppb < 1) continue;
    const int off_T = (o.off_L + (K + 2) / 2 + 1) / 2 * 2;
    const size_t lds = ((size_t)off_T + kExpTabEntries + 2 * kLogTabEntries) * sizeof(double);
    if (lds > kLdsLimit) continue;
    const int waves = std::min(8, nwb * (int)(kLdsLimit / lds));
    if (waves > best_w) {
      best_w = waves;
      SplitArgs x = sp.a;
      x.nwb = nwb;
      x.off_Y = o.off_Y; x.off_F = o.off_F; x.off_R = o.off_R; x.off_L = o.off_L; x.off_T = off_T;
      x.mode = kFbList;
      sp.al = x;
      sp.lds_l = lds;
    }
  }
  return sp;
}

// ---- fb_pairs_kernel (one lattice element per lane) ----------------------------
struct FbPlan {
  FbArgs a;
  dim3 block;
  size_t lds;
  int PPB;
};

inline int odd_up(int x) { return (x % 2 == 0) ? x + 1 : x; }

inline bool plan_fb(int SB, int d, int covmode, int K, int S, int T, FbPlan &out) {
  const int NE = S * SB;
  if (NE > kFbMaxThreads) return false;
  const int RS = odd_up(SB), AS = odd_up(S), ABS = odd_up(SB);
  const int np = covmode == VBHEM_COV_FULL ? d * (d + 1) / 2 : d;
  const int MS = odd_up(d), PS = odd_up(np);
  double best = -1.0;
  bool found = false;
  for (int ppb = 1; ppb <= 32; ++ppb) {
    const int BJ = std::min(ppb, K);
    const int BI = ppb / BJ;
    const int P = BI * BJ;
    if (P != ppb) continue;
    const int threads = (P * NE + 63) / 64 * 64;
    if (threads > kFbMaxThreads) break;
    size_t off = 0;
    FbArgs a{};
    a.off_At = (int)off; off += (size_t)BJ * S * AS;
    a.off_amax = (int)off; off += (size_t)BJ * S;
    a.off_lpi = (int)off; off += (size_t)BJ * S;
    a.off_Ab = (int)off; off += (size_t)BI * SB * ABS;
    a.off_pib = (int)off; off += (size_t)BI * SB;
    a.off_flag = (int)off; off += (size_t)(P + 1) / 2;
    a.off_reg = (int)off;
    size_t k1 = 0;
    a.off_k1m = (int)k1; k1 += (size_t)BJ * S * MS;
    a.off_k1P = (int)k1; k1 += (size_t)BJ * S * PS;
    a.off_k1c = (int)k1; k1 += (size_t)BJ * S;
    a.off_k1mu = (int)k1; k1 += (size_t)BI * SB * MS;
    a.off_k1C = (int)k1; k1 += (size_t)BI * SB * PS;
    const size_t pstride = (size_t)(T - 1) * S * RS + (size_t)(T - 1) * NE + 3 * (size_t)S * RS +
                           (size_t)S * S + SB;
    const size_t reg = std::max(k1, (size_t)P * pstride);
    const size_t lds = (off + reg) * sizeof(double);
    if (lds > kLdsLimit) continue;
    const double util = double(P * NE) / threads;
    const int blocks_per_cu = std::max<int>(1, (int)(kLdsLimit / lds));
    const int waves = std::min(32, blocks_per_cu * threads / 64);
    const double score = util * std::min(waves, 16) + 1e-3 * std::min(threads, 256);
    if (score > best) {
      best = score;
      found = true;
      a.SB = SB; a.d = d; a.covmode = covmode; a.K = K; a.S = S; a.T = T;
      a.BI = BI; a.BJ = BJ; a.NE = NE; a.RS = RS; a.AS = AS; a.ABS = ABS;
      a.njb = (K + BJ - 1) / BJ;
      a.np = np; a.MS = MS; a.PS = PS;
      a.pair_stride = (int)pstride;
      out.a = a;
      out.block = dim3(threads);
      out.lds = lds;
      out.PPB = P;
    }
  }
  return found;
}

// fb_exact_kernel's scratch slot: Theta [T][S][S][SB], then the small arrays
inline size_t exact_stride(int S, int SB, int T) {
  return (size_t)S * S * SB * T + (size_t)exact_wave_lds(S, SB);
}

// Persistent grid of the backward-only kernels: blocks per cluster, at most the
// tiles of a cluster and the device's resident blocks shared among the K clusters;
// from 8 up a multiple of 8
inline unsigned persistent_blocks(unsigned tiles, unsigned resident, unsigned K) {
  const unsigned nb = std::max(1u, std::min(tiles, resident / K));
  return nb >= 8 ? nb / 8 * 8 : nb;
}

}  // namespace vbhem
