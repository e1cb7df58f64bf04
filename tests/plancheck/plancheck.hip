// tests/plancheck/plancheck.hip -- TEST-ONLY exports of the E-step's launch planner
// (csrc/vbhem_estep_plan.h): every field of plan_split and plan_fb as integers and the
// persistent-grid rule, so the geometry is checked on a machine without a GPU
// (tests/test_estep_plan.py compares them with a recorded table).
#include <hip/hip_runtime.h>

#include "vbhem_estep_plan.h"

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

}  // extern "C"
