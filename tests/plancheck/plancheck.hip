// tests/plancheck/plancheck.hip -- TEST-ONLY exports of the E-step's launch planners
// (csrc/vbhem_estep_plan.h, csrc/vbhem_stats_plan.h): every field of plan_split and
// plan_fb, of the epilogue's responsibility / dense / gated plans, and the block-count
// rules as integers, so the geometry and the choice of kernel are checked on a machine
// without a GPU (tests/test_estep_plan.py and tests/test_stats_plan.py compare them with
// recorded tables; tests/test_dimension_cases.py reads the emission GEMM's plan per dimension).
#include <hip/hip_runtime.h>

#include "vbhem_estep_plan.h"
#include "vbhem_stats_plan.h"

namespace {

using namespace vbhem;

// SplitLayout<S, LPC> is the run-time layout, for every S and both lane counts
template <int S, int LPC>
constexpr bool layout_matches() {
  using LY = SplitLayout<S, LPC>;
  return LY::SH == split_rows(S, LPC) && LY::XCS == split_col_stride(S, LPC) &&
         LY::XP == split_pair_slab(S, LPC) && LY::HEAD == split_head(S) &&
         LY::OFF_X == split_off_x(S) && LY::OFF_X == split_offsets(S, LPC, 10, 1).off_Y -
                                                         split_offsets(S, LPC, 10, 1).ppb * LY::XP;
}
template <int S>
constexpr bool state_count_matches() {
  return SplitLPC<S>::value == split_lpc(S) && BwdLPC<S>::value == split_lpc_bwd(S) &&
         layout_matches<S, split_lpc(S)>() && layout_matches<S, split_lpc_bwd(S)>();
}
template <int... S>
constexpr bool all_match() {
  return (state_count_matches<S>() && ...);
}
static_assert(all_match<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(),
              "SplitLayout / SplitLPC / BwdLPC differ from the run-time layout functions");

}  // namespace

extern "C" {

// out [19]: ok nwb lpc ppb off_Y off_F off_R off_L off_T lds lds_bwd lds_list, then the
// list geometry's nwb off_Y off_F off_R off_L off_T lds_l
void plancheck_split(int SB, int d, int covmode, int K, int S, int T, int LPC, long long *out) {
  const SplitPlan sp = plan_split(SB, d, covmode, K, S, T, LPC);
  const SplitArgs &a = sp.a, &l = sp.al;
  const long long v[19] = {sp.ok, a.nwb, a.lpc, sp.ppb, a.off_Y, a.off_F, a.off_R, a.off_L, a.off_T,
                           (long long)sp.lds, (long long)sp.lds_bwd, (long long)sp.lds_list,
                           l.nwb, l.off_Y, l.off_F, l.off_R, l.off_L, l.off_T, (long long)sp.lds_l};
  for (int k = 0; k < 19; ++k) out[k] = v[k];
}

// out [20]: found PPB threads lds BI BJ njb pair_stride off_At off_amax off_lpi off_Ab
// off_pib off_flag off_reg off_k1m off_k1P off_k1c off_k1mu off_k1C (zeros: refused)
void plancheck_fb(int SB, int d, int covmode, int K, int S, int T, long long *out) {
  FbPlan p{};
  const bool found = plan_fb(SB, d, covmode, K, S, T, p);
  if (!found) p = FbPlan{};
  const FbArgs &a = p.a;
  const long long v[20] = {found, p.PPB, found ? (long long)p.block.x : 0, (long long)p.lds,
                           a.BI, a.BJ, a.njb, a.pair_stride, a.off_At, a.off_amax, a.off_lpi,
                           a.off_Ab, a.off_pib, a.off_flag, a.off_reg, a.off_k1m, a.off_k1P,
                           a.off_k1c, a.off_k1mu, a.off_k1C};
  for (int k = 0; k < 20; ++k) out[k] = v[k];
}

long long plancheck_persistent_blocks(long long tiles, long long resident, long long K) {
  return persistent_blocks((unsigned)tiles, (unsigned)resident, (unsigned)K);
}

// ---- the epilogue's planner (csrc/vbhem_stats_plan.h) ----
// out [11]: ok ngroups lds SBp UST JG NBB AST TPW nm_per nm_unr
void plancheck_stats_dense(int K, int S, int SB, int d, int covmode, long long *out) {
  const DensePlan p = plan_stats_dense(StatsShape{K, K, S, SB, d, covmode, 0, false, false, false});
  const long long v[11] = {p.ok, p.ngroups, (long long)p.lds, p.SBp, p.UST, p.JG, p.NBB, p.AST,
                           p.TPW, p.nm_per, p.nm_unr};
  for (int k = 0; k < 11; ++k) out[k] = v[k];
}

// out [5]: ok kernel (RespKernel) KP lds, then gate_list_lds(K)
void plancheck_resp(int K, int KT, int S, int SB, int vhem, int fold, int generic, long long *out) {
  Switches sw;
  sw.RESP_GENERIC = generic;
  const RespPlan p = plan_resp(StatsShape{K, KT, S, SB, 2, kCovFull, 0, false, false, vhem != 0},
                               fold != 0, sw);
  const long long v[5] = {p.ok, (long long)p.kernel, p.KP, (long long)p.lds, (long long)gate_list_lds(K)};
  for (int k = 0; k < 5; ++k) out[k] = v[k];
}

// the LDS a workgroup may ask for (estep_fused_checked refuses a resp_lds above it)
long long plancheck_lds_limit() { return (long long)kLdsLimit; }

namespace {
// out [16]: ok kernel (GatedStats) NTW G KSM NXR LG SM PER PB lds cap nzero stats_slabs
// exact_first, then the blocks along x that the launcher asks for
void gated_out(const GatedPlan &p, int K, long long resident, const Switches &sw, long long *out) {
  const long long blocks = p.kernel == GatedStats::kMfma ? stats_m_blocks(resident, K, p.cap, sw)
                         : p.kernel == GatedStats::kList4Reduce ? (long long)K * p.cap : p.cap;
  const long long v[16] = {p.ok, (long long)p.kernel, p.NTW, p.G, p.KSM, p.NXR, p.LG, p.SM, p.PER, p.PB,
                           (long long)p.lds, p.cap, p.nzero, p.stats_slabs, p.exact_first, blocks};
  for (int k = 0; k < 16; ++k) out[k] = p.ok ? v[k] : 0;  // (zeros: refused)
}
}  // namespace

// opnd: 0 no operand, 1 U only, 2 U and its statistics copy Us; sw [4]: NO_STATS_M
// NO_STATS_U NO_STATS_G SU_BLOCKS
void plancheck_stats_gated(int K, int S, int SB, int d, int covmode, int opnd, int nchunk,
                           long long nbases, long long resident, int fold, int nzero_m,
                           const long long *swv, long long *out) {
  Switches sw;
  sw.NO_STATS_M = swv[0]; sw.NO_STATS_U = swv[1]; sw.NO_STATS_G = swv[2]; sw.SU_BLOCKS = swv[3];
  const StatsShape s{K, K, S, SB, d, covmode, opnd ? emission_kdp(d, covmode) : 0, opnd >= 1, opnd >= 2, false};
  GatedPlan p = plan_stats_gated(s, nbases, sw);
  if (p.ok) p = plan_gated_group(p, s, nchunk, nzero_m, fold, sw);
  gated_out(p, K, resident, sw, out);
}

void plancheck_list4_reduce(int K, int S, int d, int covmode, long long *out) {
  const StatsShape s{K, K, S, S, d, covmode, emission_kdp(d, covmode), true, true, false};
  gated_out(plan_list4_reduce(s), K, 0, Switches{}, out);
}

// ---- the emission GEMM on the prepared operand (plan_emission_u, csrc/vbhem_emission.hip) ----
// out [8]: k-steps emission_kdp / 4, W' rows emission_ksp(K S), then plan_emission_u's ok,
// register bucket ukqb, row tiles per W' chunk urc, chunks (ksp / 16 / urc), waves per
// block, dynamic LDS (zeros from ok on: past kUMaxKq k-steps, the raw / generic kernels)
void plancheck_emission(int K, int S, int d, int covmode, long long *out) {
  EmissionArgs a{};
  a.K = K; a.S = S; a.d = d; a.covmode = covmode;
  a.kdp = emission_kdp(d, covmode);
  a.ksp = emission_ksp(K * S);
  size_t lds = 0;
  const bool ok = plan_emission_u(a, lds);
  const long long v[8] = {a.kdp / 4, a.ksp, ok, a.ukqb, a.urc, ok ? a.ksp / 16 / a.urc : 0, a.nwave,
                          (long long)lds};
  for (int k = 0; k < 8; ++k) out[k] = k < 2 || ok ? v[k] : 0;
}

// may fb_list4_kernel accumulate the gated sums itself (S = 8, T = 10, at most three feature
// tiles), with list4_stats_reduce_kernel behind it?
int plancheck_list4_acc(int K, int S, int SB, int T, int d, int covmode) {
  return list4_acc_supported(S, SB, T, K, us_nu(d, covmode));
}

long long plancheck_stats_m_blocks(long long resident, int K, int cap, long long su_blocks) {
  Switches sw;
  sw.SU_BLOCKS = su_blocks;
  return stats_m_blocks(resident, K, cap, sw);
}

}  // extern "C"
