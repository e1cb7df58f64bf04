// vbhem_switches.h -- the run-time switches of the library (A/B runs and tests; none is
// needed in production), one table.
//
// Each row: X(NAME, unset, meaning).  The switch VBHEM_<NAME> starts, for the whole
// process, from the environment variable of that name, read once (vbhem_capi.hip).
// Every host thread has its own current set, a copy of that default when the thread
// first asks, changed by vbhem_switch_set / vbhem_set_fused_mode on that thread only.
//   unset = 0:  a boolean.  On (1) when the variable is set to anything but "0" or "".
//   unset = -1: an integer (strtoll of the variable); negative means "not set".
#pragma once

#define VBHEM_SWITCHES(X)                                                                      \
  X(FUSED_DENSE, 0, "dense schedule instead of the gated one (vbhem_set_fused_mode)")          \
  X(NO_UGEMM, 0, "emission on the raw / generic kernels instead of the prepared operand")      \
  X(GROUP_BASES, -1, "tests: at most n bases per group of the fused call")                     \
  X(NSLAB, -1, "tests: at most n statistics slabs (1 .. 8192)")                                \
  X(NO_BWD2, 0, "backward pass on fb_split_kernel's backward mode, not fb_bwd2_kernel")        \
  X(NO_BWD4, 0, "S = 8: fb_bwd2_kernel<8> instead of fb_bwd4_kernel")                          \
  X(NO_BWD4_TRIM, 0, "S = 8: fb_bwd4_kernel with the tile copy and K3's clamp of every quad")  \
  X(NO_BWD12, 0, "S = 12: fb_bwd2_kernel<12> instead of fb_bwd12_kernel")                      \
  X(NO_LIST4, 0, "S = 8: fb_split_kernel's list mode instead of fb_list4_kernel")              \
  X(NO_LIST12, 0, "S = 12: fb_split_kernel's list mode instead of fb_list12_kernel")           \
  X(NO_K1_IN_KERNEL, 0, "short K1 through the emission GEMM, not inside the recursion")        \
  X(NO_LIST4_STATS, 0, "S = 8: per-pair outputs + stats_list_m_kernel, not sums in fb_list4_kernel") \
  X(NO_LIST_INLINE, 0, "the gate-list pass's flagged pairs through an fb_exact_kernel launch") \
  X(NO_BWD2_PREP, 0, "emission_prep_kernel launched, not its work inside fb_bwd2_kernel")      \
  X(NO_FOLD_EXACT, 0, "the backward pass's fallback as a launch, not folded into resp_kernel") \
  X(EM_NOBST, 0, "the one-chunk emission GEMM without buffer stores")                          \
  X(EM_SPLIT, -1, "the one-chunk emission GEMM in whole (0) or half (1) tiles")                \
  X(EM_NODB, 0, "the chunked emission GEMM on emission_u_kernel, not emission_db_kernel")      \
  X(RESP_GENERIC, 0, "resp_kernel's generic path for every K")                                 \
  X(NO_GATE_MASKS, 0, "K <= 64: gate_list_kernel re-reads Z, not the responsibility kernel's gate masks") \
  X(NO_FINAL_FOLD, 0, "list4_stats_reduce_kernel launched, not folded into the finishing kernel") \
  X(SU_BLOCKS, -1, "gated statistics: the block count")                                        \
  X(NO_STATS_G, 0, "gated statistics: no lane-grouped kernel")                                 \
  X(NO_STATS_U, 0, "gated statistics: the covariance-gather kernel")                           \
  X(NO_STATS_M, 0, "gated statistics: without stats_list_m_kernel")                            \
  X(EM_HOST_MATH, 0, "the EM loop's per-iteration math on the host")

namespace vbhem {

struct Switches {
#define X(name, unset, doc) long long name = unset;
  VBHEM_SWITCHES(X)
#undef X
};

// the calling thread's current set (vbhem_capi.hip)
const Switches &switches();

}  // namespace vbhem
