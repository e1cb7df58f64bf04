// vbhem_stats_plan.h -- the fused E-step epilogue's planner: which responsibility,
// dense-statistics and gated-statistics kernel runs, its template bucket, dynamic LDS and
// block counts.  Arithmetic on sizes and switches only, no HIP call; device properties
// come in as arguments.  The scheduler plans once per fused call, the launchers switch
// over the plans, tests/plancheck compares them with a recorded table.
#pragma once
#include <algorithm>
#include <cstddef>

#include "vbhem_internal.h"
#include "vbhem_exact.h"

namespace vbhem {

// ---- the kernels' block shapes ----------------------------------------------------
#ifndef VBHEM_RESP_THREADS
#define VBHEM_RESP_THREADS 512  // 8 waves per chunk block: 2x the bases in flight (C4 -10 us)
#endif
constexpr int kRespThreads = VBHEM_RESP_THREADS;
constexpr int kRespFoldWaves = 4;  // folded fallback: worker wavefronts per chunk block
constexpr int kRespSlots = 4;      // resp_trials_kernel: clusters per lane (K <= 256)
constexpr int kListThreads = 256;  // gate_list_kernel
constexpr int kSlThreads = 256;    // stats_list_kernel
constexpr int kStatsThreads = 512;  // stats_kernel
constexpr int kStatsWaves = kStatsThreads / 64;
constexpr int kStatsMaxNBB = 4;
constexpr int kStatsMaxA = 8;   // sum_t_nu values per thread per batch
constexpr int kStatsMaxR = 8;   // raw covariance / mean values per thread per batch
constexpr int kNmThreads = 256;  // nm_kernel
constexpr int kSuWaves = 4;      // stats_list_u_kernel, stats_list_g_kernel
constexpr int kSmWaves = 4;      // stats_list_m_kernel
static_assert(kSmWaves == kSuWaves, "su_output's thread stride");
constexpr int kL4rParts = 16, kL4rCols = 64, kL4rThreads = kL4rParts * kL4rCols;

// ---- shared geometry ----------------------------------------------------------------
// the list kernels' block reduction area: sums [S][NU] | [S] | [S][S], then the shift z [d]
inline size_t stats_red_doubles(int S, int NU, int d) {
  return (size_t)S * NU + S + (size_t)S * S + d;
}
// a wave's (or lane group's) staging slab of the prepared-operand kernels:
// Z tnu [SB][S] | the pair's U columns [SB][ukdp + 1], each rounded up to even
inline size_t stats_wave_slab(int S, int SB, int ukdp) {
  return ((size_t)S * SB + 1) / 2 * 2 + ((size_t)SB * (ukdp + 1) + 1) / 2 * 2;
}
// the state-count bucket (registers per lane) of the prepared-operand kernels
inline int stats_sm(int S) { return S <= 4 ? 4 : S <= 8 ? 8 : S <= 12 ? 12 : 16; }

// the shape of one fused call, as far as the epilogue's choices depend on it
struct StatsShape {
  int K, KT, S, SB, d, covmode;
  int ukdp;     // k-extent of the emission GEMM's operand U (has_U)
  bool has_U;   // the call has the operand U (prepared, or built per group)
  bool has_Us;  // ... and its statistics copy Us (prepared base sets only)
  bool vhem;
  int NU() const { return us_nu(d, covmode); }
};

// ---- responsibilities ---------------------------------------------------------------
// dynamic LDS of resp_kernel / resp_trials_kernel, and of vhem_resp_kernel
// (at least the folded fallback's queue, which borrows this space first)
inline size_t resp_lds(int K, int KT) {
  int G = 1;
  while (G < K && G < 64) G <<= 1;
  const size_t R = KT >= 1 && K % KT == 0 ? (size_t)(K / KT) : 1;
  return std::max(((size_t)(kRespThreads / 64) * ((64 / G) * (size_t)K + 2 * R)) * sizeof(double) +
                      (size_t)K * sizeof(int),
                  (size_t)(kRespThreads + 1) * sizeof(int));
}
inline size_t vhem_resp_lds(int K, int KT) {
  const size_t R = KT >= 1 && K % KT == 0 ? (size_t)(K / KT) : 1;
  return std::max((size_t)(kRespThreads / 64) * ((size_t)K + R) * sizeof(double) +
                      (size_t)K * sizeof(int),
                  (size_t)(kRespThreads + 1) * sizeof(int));
}
// dynamic LDS of gate_list_kernel: the per-wave ballot masks grow with K (the caller keeps
// the gated schedule only while this fits a CU)
inline size_t gate_list_lds(int K) {
  const size_t ints = (size_t)2 * K + kListThreads / 64 + 2 * kListThreads;
  return (ints + 1) / 2 * 2 * sizeof(int) +
         (size_t)(kListThreads / 64) * K * sizeof(unsigned long long);
}

// the gate masks (StatsArgs::gmask): one 64-bit word per base of a group, bit j = pair
// (i, j) passes the gate -- while a word holds every cluster
inline bool gate_masks_supported(int K) { return K >= 1 && K <= 64; }
inline size_t gate_mask_words(size_t group_bases) { return group_bases; }

enum class RespKernel { kVhem, kTrials, kKP, kGeneric };
struct RespPlan {
  bool ok = false;  // false: K / KT outside the kernel's range
  RespKernel kernel = RespKernel::kGeneric;
  int KP = 0;       // kKP: resp_kernel<KP>, K a power of two in 4 .. 64
  size_t lds = 0;   // per-wave Nj accumulators of all K clusters (past 64 KB at K ~ 960)
};
// fold: resp_kernel runs the backward pass's exact fallback first (StatsArgs::fold)
inline RespPlan plan_resp(const StatsShape &s, bool fold, const Switches &sw) {
  RespPlan p;
  const int K = s.K, KT = s.KT;
  p.lds = s.vhem ? vhem_resp_lds(K, KT) : resp_lds(K, KT);
  // the folded fallback borrows the accumulators' space first (queue + worker regions)
  if (fold) p.lds = std::max(p.lds, fold_lds_bytes(kRespThreads, kRespFoldWaves, s.S, s.SB));
  const bool pow2 = K == 4 || K == 8 || K == 16 || K == 32 || K == 64;
  p.kernel = s.vhem ? RespKernel::kVhem      // one kernel for every K and trial count
             : KT != K ? RespKernel::kTrials  // batched trials
             : pow2 && !sw.RESP_GENERIC ? RespKernel::kKP : RespKernel::kGeneric;  // (A/B: the generic kernel)
  p.KP = p.kernel == RespKernel::kKP ? K : 0;
  p.ok = KT == K || (KT >= 1 && K % KT == 0 && (s.vhem || K <= kRespSlots * 64));
  return p;
}

// ---- dense-schedule statistics (stats_kernel + nm_kernel) ---------------------------
constexpr size_t kStatsLdsTarget = 78 * 1024;  // two 512-thread blocks per CU
constexpr int kMaxTPW = 16;

struct DensePlan {
  bool ok = false;
  int SBp = 0, UST = 0, JG = 0, NBB = 0, AST = 0;  // StatsArgs fields of the same names
  int ngroups = 1;  // grid.y: row groups of JG clusters
  size_t lds = 0;
  int TPW = 0;                 // stats_kernel<TPW>: MFMA tiles per wave, 4 / 8 / 16
  int nm_per = 0, nm_unr = 0;  // nm_kernel<PER, UNR>: <6, 4> or <24, 1>
};
inline DensePlan plan_stats_dense(const StatsShape &s) {
  DensePlan p;
  const int K = s.K, S = s.S, SB = s.SB, d = s.d, NU = s.NU();
  p.SBp = (SB + 3) / 4 * 4;
  const int NTL = (NU + 15) / 16;
  p.UST = NTL * 16;
  // clusters per row group: at most 128 rows, balanced over the groups
  int jg = std::max(1, 128 / S);
  p.ngroups = (K + jg - 1) / jg;
  jg = (K + p.ngroups - 1) / p.ngroups;
  p.JG = jg;
  const int RG = jg * S;
  const int tpw = (((RG + 15) / 16) * NTL + kStatsWaves - 1) / kStatsWaves;
  const int no = K * S + K * S * S;  // nm_kernel's outputs
  if (tpw > kMaxTPW || no > 24 * kNmThreads || RG > kStatsThreads) return p;
  const int dd = s.covmode == kCovFull ? d * d : d;
  for (int nbb = kStatsMaxNBB; nbb >= 1; --nbb) {
    const bool regs_ok = (nbb * RG * SB + kStatsThreads - 1) / kStatsThreads <= kStatsMaxA &&
                         (nbb * SB * (dd + d) + kStatsThreads - 1) / kStatsThreads <= kStatsMaxR;
    p.NBB = nbb;
    p.AST = nbb * p.SBp + 1;
    p.lds = ((size_t)RG * p.AST + (size_t)nbb * p.SBp * p.UST + (size_t)nbb * SB * (dd + d) +
             (size_t)nbb * jg) * sizeof(double) + (size_t)NU * sizeof(int);
    if (regs_ok && p.lds <= kStatsLdsTarget) {
      p.ok = true;
      break;
    }
  }
  p.TPW = tpw <= 4 ? 4 : tpw <= 8 ? 8 : 16;
  p.nm_per = no <= 6 * kNmThreads ? 6 : 24;
  p.nm_unr = no <= 6 * kNmThreads ? 4 : 1;
  return p;
}

// ---- gated-schedule statistics --------------------------------------------------------
//   kList4Reduce  list4_stats_reduce_kernel: fb_list4_kernel accumulated the sums
//   kMfma         stats_list_m_kernel<NTW, G, KSM, NXR> on the statistics copy Us
//   kGrouped      stats_list_g_kernel<LG, SM>: LG lanes per pair, on the operand U
//   kOperand      stats_list_u_kernel<SM>: a wave per pair, on the operand U
//   kGather       stats_list_kernel<PER>: the moments gathered from the covariances
enum class GatedStats { kList4Reduce, kMfma, kGrouped, kOperand, kGather };
struct GatedPlan {
  bool ok = false;  // false: the gated schedule's statistics do not fit this shape
  GatedStats kernel = GatedStats::kGather;
  int NTW = 0, G = 0, KSM = 0, NXR = 0;  // kMfma
  int LG = 0, SM = 0;                    // kGrouped; SM: kOperand too
  int PER = 0;                           // kGather
  int PB = 0;      // stats_list_kernel's pairs per LDS batch (StatsArgs::PB)
  size_t lds = 0;  // the chosen kernel's dynamic LDS
  // one base group (plan_gated_group)
  int cap = 0;          // blocks per cluster (kMfma: of the 1-D grid over all clusters,
                        // before stats_m_blocks)
  int nzero = 0;        // StatsArgs::nzero (0: the kernel's grid covers every slab)
  int stats_slabs = 0;  // the slabs [0, n) that hold the group's N1 / M / U entries
  bool exact_first = false;  // an fb_exact_kernel launch from flag_count[3] precedes it
};

constexpr size_t kSlLdsBudget = 48 * 1024;  // stats_list_kernel's batch records

// lanes per pair group of the grouped kernel (0: shape too large for it)
inline int stats_group_lanes(const StatsShape &s, const Switches &sw) {
  if (sw.NO_STATS_G) return 0;
  const int OT = s.S * s.SB, nu4 = s.ukdp * s.SB;
  for (int LG : {8, 16, 32})
    if (s.NU() <= LG && OT <= 4 * LG && s.S * s.S <= 4 * LG && nu4 <= 8 * LG) return LG;
  return 0;
}

// The kernel and its bucket, once per fused call.  max_group_bases: the bases of the
// call's largest base group.
inline GatedPlan plan_stats_gated(const StatsShape &s, long long max_group_bases, const Switches &sw) {
  GatedPlan p;
  const int K = s.K, S = s.S, SB = s.SB, NU = s.NU();
  // stats_list_kernel's batch: records [tnu | nu1 | xi | u] + tab + Z / base index per pair
  const size_t rs = (size_t)((S * SB + S + S * S + SB * NU + 1) / 2 * 2) * sizeof(double);
  const size_t tab = (size_t)(NU + 1) / 2 * 2 * sizeof(int);
  if (rs + tab + 12 > kSlLdsBudget) return p;
  // small batches: many resident blocks hide the gather latency (6 measured best at C4)
  p.PB = (int)std::min<size_t>(6, (kSlLdsBudget - tab) / (rs + 12));
  p.ok = true;
  const size_t red = stats_red_doubles(S, NU, s.d) * sizeof(double);
  // the MFMA kernel on the statistics copy Us (prepared base sets; S <= 16 rows of one
  // MFMA tile, SB <= 16, at most 12 feature tiles over 4 waves); also for the small
  // moment vectors of the grouped kernel (C3: statistics 0.039 -> 0.032 ms per step)
  // (it reads Z at the 32-bit offset (i - i_buf0) K + j: a base group times K must stay
  // below 2^32 -- always so for a workspace group, checked anyway)
  const bool z32 = (unsigned long long)max_group_bases * (unsigned long long)K < (1ull << 32);
  const int nt = us_nup(NU) / 16;
  if (s.has_Us && !sw.NO_STATS_U && !sw.NO_STATS_M && z32 && S <= 16 && SB <= 16 && nt <= 12) {
    p.kernel = GatedStats::kMfma;
    p.KSM = us_sbp(SB) / 4;  // the k-slices of four base states, exact
    // 4 pair groups (every wave all feature tiles) up to 4 tiles (NU <= 64), 2 groups up
    // to 8 tiles, else one group of 4 tile groups
    // (C4: 1 or 2 pair groups measured 0.41 / 0.25 ms of statistics per step against 0.21)
    p.G = nt <= 4 ? 4 : nt <= 8 ? 2 : 1;
    p.NTW = nt <= 4 ? nt : nt <= 6 ? 3 : nt <= 8 ? 4 : 3;
    // the sum_nu_1 | sum_xi chunks per wave: ceil(ceil((S + S^2) / 64) / tile groups)
    const int TG = kSmWaves / p.G, nxr = ((S + S * S + 63) / 64 + TG - 1) / TG;
    p.NXR = nxr <= 3 ? nxr : 5;
    p.lds = red;
    return p;
  }
  // on the prepared operand's tile layout when the call has one (S <= 16: the split
  // kernel's range).  NU > 64, e.g. d = 16 full at C5: the covariance gather of
  // stats_list_kernel measured 2 % faster (1.74 vs 1.78 ms per 100 k-base step) than
  // stats_list_u_kernel with two or three moment columns per lane, so it takes those
  if (s.has_U && !sw.NO_STATS_U && NU <= 64 && S <= 16 && SB <= S) {
    const size_t ws = stats_wave_slab(S, SB, s.ukdp);
    p.SM = stats_sm(S);
    p.LG = stats_group_lanes(s, sw);
    p.kernel = p.LG ? GatedStats::kGrouped : GatedStats::kOperand;
    p.lds = (size_t)kSuWaves * (p.LG ? 64 / p.LG : 1) * ws * sizeof(double) + red;
    return p;
  }
  p.kernel = GatedStats::kGather;
  p.PER = S + S * S + S * NU <= 4 * kSlThreads ? 4 : 8;
  p.lds = (size_t)p.PB * (rs + 12) + tab;
  return p;
}

// The geometry of one base group of nchunk chunks.  nzero_m: at most that many parts
// (slabs) per cluster for the MFMA kernel (0: nchunk); fold: StatsArgs::fold.
inline GatedPlan plan_gated_group(GatedPlan p, const StatsShape &s, int nchunk, int nzero_m, int fold,
                                  const Switches &sw) {
  const int K1 = std::max(1, s.K);
  // blocks of the list kernels on the prepared operand: the per-block cost (wave
  // reduction, slab writes) grows with the output count NO: at most ~4M block outputs
  // per launch (C4: 512 x 16 blocks of 432, C5: 64 x 32 of 1992 -- measured: 16384
  // blocks of 1992 ran 1.3x slower than 2048), and at most 4096 blocks in all (C4: 256
  // parts per cluster instead of 512, statistics 0.245 -> 0.231 ms; 3072 blocks 0.243,
  // 6144 0.235)
  const long long NO = (long long)s.S + (long long)s.S * s.S + (long long)s.S * s.NU();
  long long cap = std::min<long long>((4ll << 20) / (NO * K1), 4096 / K1);
  if (sw.SU_BLOCKS >= 0) cap = sw.SU_BLOCKS / K1;  // A/B
  const int nb = (int)std::max(1ll, std::min((long long)nchunk, cap));
  p.nzero = nchunk;
  p.stats_slabs = nchunk;
  // the gate-list pass's flagged pairs (resp_kernel folded the backward pass's): an
  // fb_exact_kernel launch from flag_count[3] before any statistics kernel reads them.
  // (Folded into stats_list_m_kernel as well it measured no faster when nothing is
  // flagged -- its inlined fallback cost the kernel ~9 us at C4 -- and 3x slower when
  // every base is flagged: one worker wave per block there)
  p.exact_first = fold == 1;  // (2: the list kernel recomputed its flagged pairs itself)
  switch (p.kernel) {
    case GatedStats::kMfma:
      // one 1-D grid over all clusters' gated pairs (balanced parts; the block maps
      // itself to (cluster, part)); at most nzero_m parts per cluster, so the slabs past
      // them hold none of its N1 / M / U entries (stats_final_kernel reads only those)
      if (nzero_m > 0) p.nzero = std::min(nzero_m, nchunk);
      p.stats_slabs = p.nzero;
      p.cap = (int)std::min<long long>((long long)nchunk * s.K, 1ll << 30);
      break;
    case GatedStats::kGrouped:
      // the grouped kernel runs 64 / LG pairs per wave at once: half the blocks (C3,
      // 80 per cluster: statistics 0.047 -> 0.043 ms; with 156 it was 0.057)
      p.cap = sw.SU_BLOCKS >= 0 ? nb : std::max(1, nb / 2);
      break;
    case GatedStats::kOperand:
      p.cap = nb;
      break;
    case GatedStats::kGather:
      p.cap = nchunk;
      p.nzero = 0;
      break;
    case GatedStats::kList4Reduce:  // (plan_list4_reduce is already a group's plan)
      break;
  }
  return p;
}

// stats_list_m_kernel's blocks: one generation of resident blocks (the kernel is
// latency-bound: a second round of blocks repeats every block's start-up chain; C4: 1024
// blocks 0.177 ms per step of statistics, 2048 0.211, 4096 0.188 at the ring depth 2), at
// least one per cluster, at most the slab count per cluster (cap)
inline unsigned stats_m_blocks(long long resident_blocks, int K, int cap, const Switches &sw) {
  long long nb = resident_blocks;
  if (sw.SU_BLOCKS >= 0) nb = sw.SU_BLOCKS;  // A/B
  return (unsigned)std::min<long long>(std::max<long long>(nb, K + 1), cap);
}

// May fb_list4_kernel accumulate the gated sums itself?  Only where stats_list_m_kernel
// would otherwise sum them: the same operand, weights and switches.
inline bool list4_acc_eligible(const GatedPlan &p, const StatsShape &s, int T, bool has_Z,
                               const Switches &sw) {
  return p.ok && p.kernel == GatedStats::kMfma && s.has_Us && has_Z && !s.vhem &&
         list4_acc_supported(s.S, s.SB, T, s.K, s.NU()) && !sw.NO_LIST4_STATS;
}
// ... and the reduction of its partials: block (j, s) sums state s's row of cluster j
// (at most kL4rCols columns: NU <= 48 at S = 8); slab 0 alone holds the N1 | M | U sections
inline GatedPlan plan_list4_reduce(const StatsShape &s) {
  GatedPlan p;
  p.kernel = GatedStats::kList4Reduce;
  p.ok = s.NU() + 1 + s.S <= kL4rCols;
  p.lds = stats_red_doubles(s.S, s.NU(), s.d) * sizeof(double);
  p.cap = s.S;  // blocks per cluster
  p.nzero = 1;
  p.stats_slabs = 1;
  return p;
}

}  // namespace vbhem
