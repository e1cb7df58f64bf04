// vbhem_estep_sched.hip -- the E-step's scheduler: carves the caller's workspace,
// chooses the recursion kernels from the plan (vbhem_estep_plan.h) and enqueues them,
// the emission GEMM and the statistics kernels on the caller's stream.  No allocation,
// no host synchronisation (graph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_estep_plan.h"
#include "vbhem_estep_sched.h"
#include "vbhem_internal.h"
#include "vbhem_stats_plan.h"

namespace {

using namespace vbhem;

// the fault-injection hook of vbhem_debug_extra_lds (tests only; 0 in production)
std::atomic<size_t> g_debug_extra_lds{0};

// the kernels the last call of this host thread ran for its recursion passes
// (vbhem_last_kernel: what a benchmark line names, taken from the launch itself)
// ([2]: the fused call's gated statistics kernel family, [3]: its finishing kernel)
thread_local std::string g_last_kernel[4];
std::string split_name(const SplitArgs &a) {
  return "vbhem::fb_split_kernel<" + std::to_string(a.S) + ", " + std::to_string(a.lpc) + ", " +
         std::to_string(a.mode) + ">";
}
const char *tf(bool b) { return b ? "true>" : "false>"; }

constexpr int kExactThreads = kExactSlots;        // fallback scratch slots (one per wavefront)
constexpr int kChunkMinBases = 64;                // fused epilogue: bases per chunk, at least
constexpr size_t kGroupBudget = (size_t)8 << 30;  // per-pair buffers per group (fused)
constexpr int kMaxSlabs = 512;                    // statistics chunks (= resp/stats blocks per group)
constexpr int kHeadInts = kFlagPre + kFlagHead;   // the flag head and the counters after it

template <class Args>  // the inputs FbArgs and SplitArgs share
void fill_inputs(Args &a, const vbhem_base_t *b, const vbhem_cluster_t *c) {
  a.prior = b->prior; a.A = b->A; a.logA = c->logA; a.logPi = c->logPi;
}

// a pass's bases [i_begin, i_end) (buffers' row 0 = i_buf0), outputs and fallback flags
struct Pass {
  int i_begin, i_end, i_buf0;
  double *LL, *nu1, *xi, *tnu;
  int *flags;
};
template <class Args>  // FbArgs, SplitArgs
void set_pass(Args &a, const Pass &p) {
  a.i_begin = p.i_begin; a.i_end = p.i_end; a.i_buf0 = p.i_buf0;
  a.LL = p.LL; a.nu1 = p.nu1; a.xi = p.xi; a.tnu = p.tnu;
  a.flag_count = p.flags; a.flag_list = p.flags + kFlagHead;
}

// ---- workspace carving -------------------------------------------------------
struct Carver {
  char *base;
  size_t off = 0;
  explicit Carver(void *p) : base(static_cast<char *>(p)) {}
  template <class T>
  T *take(size_t n) {
    off = align_up(off, 256);
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// emission_u_kernel applies (k-steps <= kUMaxKq): the per-call operand U is needed
// unless the caller prepared one (base->U)
bool u_gemm_ok(const vbhem_base_t *b) {
  return emission_kdp(b->d, b->covmode) / 4 <= kUMaxKq && !switches().NO_UGEMM;
}
bool need_u_ws(const vbhem_base_t *b) { return !b->U && u_gemm_ok(b); }

// the carved workspace of either call (the pairs call: the flag head, tnu, the emission
// GEMM's buffers and scratch only)
struct Ws {
  int group;  // bases per group
  int nslab;
  int slab_len;
  int *fpre, *flags;                // the flag head (kFlagPre), then [0]=count [1]=total [2..] list
  int *gate_cnt, *list, *list_tot;  // gated schedule: [nslab][K], [K][group], [K]
  unsigned long long *gmask;        // gated schedule, K <= 64: [group] gate masks (else null)
  double *Atg;                      // gated schedule: [K][S][S] A' for the backward pass
  double *scratch, *nu1, *xi, *tnu, *Z, *slabs;
  double *E, *W, *bias, *shift;     // emission GEMM (split path)
  double *U;                        // per-call operand of the emission GEMM (null: prepared)
  double *l4parts;                  // fb_list4_kernel's statistics partials (null: not its shape)
};

// the emission GEMM's buffers for nb bases x all K S cluster states
void carve_emission(Carver &cv, const vbhem_base_t *b, int K, int S, size_t nb, Ws &w) {
  w.E = cv.take<double>(nb * K * S * b->SB);
  w.W = cv.take<double>((size_t)emission_kdp(b->d, b->covmode) * emission_ksp(K * S));
  w.bias = cv.take<double>((size_t)emission_ksp(K * S));
  w.shift = cv.take<double>((size_t)b->d);
  w.U = need_u_ws(b) ? cv.take<double>(u_doubles((long long)nb * b->SB + 16, b->d, b->covmode))
                     : nullptr;
}

size_t carve_pairs(void *ws, const vbhem_base_t *b, const vbhem_cluster_t *c, int T, bool need_tnu,
                   Ws &w) {
  Carver cv(ws);
  const size_t np = (size_t)b->N * c->K;
  w.fpre = cv.take<int>(kHeadInts + np);  // first: see kFlagPre
  w.flags = w.fpre + kFlagPre;
  w.tnu = need_tnu ? cv.take<double>(np * c->S * b->SB) : nullptr;
  carve_emission(cv, b, c->K, c->S, (size_t)b->N, w);
  // the exact fallback's scratch last: its size does not move the hot buffers
  w.scratch = cv.take<double>(exact_stride(c->S, b->SB, T) * kExactThreads);
  return cv.off + 256;
}

size_t carve_fused(void *ws, const vbhem_base_t *b, const vbhem_cluster_t *c, int T, Ws &w,
                   int R = 1) {
  Carver cv(ws);
  const int K = c->K, S = c->S, SB = b->SB;
  const size_t per_base = (size_t)K * (S + (size_t)S * S + 2 * (size_t)S * SB) * sizeof(double);
  size_t g = std::max<size_t>(1, kGroupBudget / std::max<size_t>(1, per_base));
  g = std::min<size_t>(g, (size_t)std::max(1, b->N));
  const Switches &sw = switches();
  if (sw.GROUP_BASES >= 0)  // tests: force several groups
    g = std::max<size_t>(1, std::min<size_t>(g, (size_t)sw.GROUP_BASES));
  w.group = (int)g;
  int maxslab = kMaxSlabs;
  if (sw.NSLAB >= 0) maxslab = (int)std::max(1ll, std::min(8192ll, sw.NSLAB));
  w.nslab = std::min<int>(w.group, maxslab);
  w.slab_len = R * (int)vbhem_stats_len(K / R, S, b->d, b->covmode);
  // flagged-pair list: with the fallback folded into the consumers the backward pass's
  // entries stay while the gate-list pass appends its own (at most g K + g K)
  w.fpre = cv.take<int>(kHeadInts + 2 * g * K);  // first: see kFlagPre
  w.flags = w.fpre + kFlagPre;
  w.nu1 = cv.take<double>(g * K * S);
  w.xi = cv.take<double>(g * K * S * S);
  w.tnu = cv.take<double>(g * K * S * SB);
  w.Z = cv.take<double>(g * K);
  w.slabs = cv.take<double>((size_t)w.nslab * w.slab_len);
  carve_emission(cv, b, K, S, g, w);
  w.gate_cnt = cv.take<int>((size_t)w.nslab * K);
  w.list = cv.take<int>(g * K);
  w.list_tot = cv.take<int>((size_t)K);
  // A' [K][S][S] (read-only for every recursion kernel)
  w.Atg = cv.take<double>((size_t)K * S * S);
  // the accumulating gate-list pass's partials: a slot per wave of its grid (at most the
  // inline fallback's kExactThreads) and cluster (vbhem_list4_slots.h)
  const int NU = (int)vbhem_stats_nu(b->d, b->covmode);
  w.l4parts = list4_acc_supported(S, SB, T, K, NU)
                  ? cv.take<double>((size_t)l4s_max_slots(kExactThreads, K) *
                                    l4s_part_len(S, us_nup(NU)))
                  : nullptr;
  // the gate masks, a word per base of the group (whatever the switches say: the size
  // depends on the shape alone)
  w.gmask = gate_masks_supported(K) ? cv.take<unsigned long long>(gate_mask_words(g)) : nullptr;
  // the exact fallback's scratch last: its size does not move the hot buffers
  w.scratch = cv.take<double>(exact_stride(S, SB, T) * kExactThreads);
  return cv.off + 256;
}

// ---- kernel choice and dispatch -----------------------------------------------
// the gated schedule's backward-only pass: fb_split_kernel's backward mode, or
//   kBwd2   fb_bwd2_kernel (S <= kBwd2MaxS)
//   kBwd4   S = 8, SB <= 8: fb_bwd4_kernel (MFMA contractions)
//   kBwd12  S = 12, SB <= 12: fb_bwd12_kernel (MFMA contractions)
enum class BwdKernel { kSplit, kBwd2, kBwd4, kBwd12 };
// its gate-list pass: fb_split_kernel's list mode, or
//   kList4   S = 8, SB <= 8, T = 10: fb_list4_kernel
//   kList12  S = 12, SB <= 12, T = 10: fb_list12_kernel
enum class ListKernel { kSplit, kList4, kList12 };

struct FbCtx {
  FbPlan plan;      // generic element-per-lane kernel
  SplitPlan split;  // column-per-LPC-lanes kernel (preferred when it applies)
  SplitPlan bwd;    // its backward-only mode (gated schedule), possibly another LPC
  BwdKernel bwd_kernel = BwdKernel::kSplit;
  ListKernel list_kernel = ListKernel::kSplit;
  // BwdKernel::kBwd2: LDS bytes, pairs per block, waves per block
  size_t bwd2_lds = 0;
  int bwd2_ppb = 0, bwd2_nwb = 0;
  // gated schedule on fb_bwd2_kernel + fb_split_kernel's list mode with a short K1
  // (kdp <= 8: C2, C3): both evaluate E from the prepared operand (SplitArgs::eU);
  // no emission GEMM launch, no E traffic
  bool k1_in_kernel = false;
  // ... and emission_prep_kernel's work inside fb_bwd2_kernel (SplitArgs::prep): fpre, the
  // workspace's flag head, set by the fused call for a prepared operand
  int *fpre = nullptr;
  EmissionArgs em{};  // K1 GEMM feeding the split kernel
  size_t em_lds = 0;
  // emission_u_kernel: on the prepared operand (base->U) or one built per call in u_ws
  bool use_u = false;
  size_t em_lds_u = 0;
  const vbhem_base_t *base = nullptr;
  double *u_ws = nullptr;
};

// split_first_pass (the VHEM fused call): the gated schedule's backward-only pass runs on
// fb_split_kernel's backward mode, whose L_elbo has the dense schedule's rounding, not on
// fb_bwd2 / fb_bwd4 / fb_bwd12_kernel.  VHEM multiplies L_elbo by N_i / inf_norm (up to
// hundreds) before the softmax, so the few ulp that the reduced-operation exp / log of
// those kernels cost show in Z, Nj and the statistics.
int prepare_fb(FbCtx &c, const vbhem_base_t *b, const vbhem_cluster_t *cl, int T,
               double smooth = 1.0, bool split_first_pass = false) {
  const int S = cl->S, SB = b->SB;
  const Switches &sw = switches();
  c.split = plan_split(SB, b->d, b->covmode, cl->K, S, T, split_lpc(S));
  // backward-only pass: half the lanes per column (no forward-sweep registers to
  // hold), more rows per lane: no DPP for S <= 8, more independent exp/log chains
  c.bwd = plan_split(SB, b->d, b->covmode, cl->K, S, T, split_lpc_bwd(S));
  if (c.split.ok) {
    EmissionArgs &e = c.em;
    e.SB = SB; e.d = b->d; e.covmode = b->covmode; e.K = cl->K; e.S = S;
    e.smooth = smooth;
    e.centres = b->centres; e.covars = b->covars; e.m = cl->m; e.P = cl->P; e.c = cl->c;
    if (!plan_emission(e, c.em_lds)) c.split.ok = false;
    if (c.split.ok && u_gemm_ok(b) && plan_emission_u(e, c.em_lds_u)) {
      c.use_u = true;
      e.zfix = b->U;  // a prepared operand carries its shift in its head
    }
  }
  c.base = b;
  const bool have_elems = plan_fb(SB, b->d, b->covmode, cl->K, S, T, c.plan);
  if (!c.split.ok && !have_elems)
    return set_error(VBHEM_ERR_UNSUPPORTED,
                     "no launch geometry fits (S*SB must be <= 512 and the per-pair lattice "
                     "(2*(T-1)+3)*S*SB doubles must fit in 160 KiB of LDS)");
  if (!have_elems) c.plan = FbPlan{};
  FbArgs &pa = c.plan.a;
  fill_inputs(pa, b, cl);
  pa.centres = b->centres; pa.covars = b->covars; pa.m = cl->m; pa.P = cl->P; pa.c = cl->c;
  // fields the exact fallback kernel needs even when the generic plan is unused
  pa.SB = SB; pa.d = b->d; pa.covmode = b->covmode; pa.K = cl->K; pa.S = S; pa.T = T;
  pa.smooth = smooth;
  if (c.split.ok) {
    fill_inputs(c.split.a, b, cl);
    fill_inputs(c.split.al, b, cl);
    fill_inputs(c.bwd.a, b, cl);
    if (c.bwd.ok && S <= kBwd2MaxS && !sw.NO_BWD2) {
      if (!split_first_pass) {
        c.bwd2_nwb = bwd2_waves(S);
        c.bwd2_lds = bwd2_lds(S, c.bwd2_nwb);
        c.bwd2_ppb = bwd2_ppb(S, c.bwd2_nwb);
        if (bwd4_supported(S, SB) && !sw.NO_BWD4) c.bwd_kernel = BwdKernel::kBwd4;
        else if (bwd12_supported(S, SB) && !sw.NO_BWD12) c.bwd_kernel = BwdKernel::kBwd12;
        else if (c.bwd2_lds) c.bwd_kernel = BwdKernel::kBwd2;
      }
      if (list4_supported(S, SB, T, cl->K) && !sw.NO_LIST4) c.list_kernel = ListKernel::kList4;
      else if (list12_supported(S, SB, T, cl->K) && !sw.NO_LIST12) c.list_kernel = ListKernel::kList12;
    }
    c.k1_in_kernel = c.use_u && c.bwd_kernel == BwdKernel::kBwd2 &&
                     c.list_kernel == ListKernel::kSplit && c.em.kdp <= kK1InKernelMaxKdp &&
                     !sw.NO_K1_IN_KERNEL;
  }
  return VBHEM_OK;
}

// the emission GEMM's base-set operand and the global column of its tile 0: the
// prepared operand, or this call's (run_fb builds it for bases from i_begin: tile 0 at
// column i_begin SB rounded down to 16)
const double *operand(const FbCtx &c, int i_begin, long long *col0) {
  *col0 = c.base->U ? 0 : (long long)i_begin * c.base->SB / 16 * 16;
  return c.base->U ? c.base->U : c.u_ws;
}

// the in-kernel K1's operands (FbCtx::k1_in_kernel)
void set_k1_operands(const FbCtx &c, int i_begin, SplitArgs &ca) {
  ca.eU = operand(c, i_begin, &ca.e_col0);
  ca.eW = c.em.W; ca.ebias = c.em.bias;
  ca.ekdp = c.em.kdp; ca.eksp = c.em.ksp; ca.esmooth = c.em.smooth;
}

// W, bias, shift of the emission GEMM: once per call (depends on the clusters only)
int run_emission_prep(FbCtx &c, double *W, double *bias, double *shift, hipStream_t st,
                      int *zero_ints = nullptr, int n_zero = 0, double *Atg = nullptr,
                      const double *logA = nullptr) {
  if (!c.split.ok) return VBHEM_OK;
  c.em.W = W; c.em.bias = bias; c.em.shift = shift;
  c.em.zero_ints = zero_ints; c.em.n_zero = zero_ints ? n_zero : 0;
  c.em.Atg = Atg; c.em.logA = logA;
  hipError_t e = launch_emission_prep(c.em, st);
  if (e != hipSuccess) return hip_fail(e, "emission_prep_kernel");
  return VBHEM_OK;
}

// every resident block of the device, for a kernel with per_cu of them per CU
unsigned resident_blocks(int per_cu) { return (unsigned)(device_cus() * std::max(1, per_cu)); }

int run_fb_exact(const FbArgs &a, double *scratch, hipStream_t st) {
  hipError_t e = launch_fb_exact(a, scratch, exact_stride(a.S, a.SB, a.T), kExactThreads, st);
  if (e != hipSuccess) return hip_fail(e, "fb_exact_kernel");
  return VBHEM_OK;
}

// Gated schedule, second pass: both sweeps for the pairs of the gate lists (p.LL: the
// backward pass's, rewritten only for the pairs the exact fallback takes).
int run_fb_list(const FbCtx &c, const Pass &p, const double *Ebuf, long long e_ld, const int *list,
                const int *list_tot, int list_cap, double *scratch, hipStream_t st,
                bool fold = false, bool *inlined = nullptr, const StatsArgs *acc_sa = nullptr,
                const GatedPlan *acc_plan = nullptr, const StatsShape *acc_shape = nullptr,
                double *acc_parts = nullptr, int *acc_waves = nullptr) {
  if (p.i_end <= p.i_begin) return VBHEM_OK;
  // flags[0] is zero here: the backward pass's fb_exact_kernel reset it
  if (!c.split.lds_l) return set_error(VBHEM_ERR_UNSUPPORTED, "gate-list pass does not fit LDS");
  SplitArgs ca = c.split.al;
  ca.mode = kFbList;
  ca.E = Ebuf; ca.e_ld = e_ld;
  set_pass(ca, p);
  ca.LL = nullptr;
  ca.list = list; ca.list_tot = list_tot; ca.list_cap = list_cap;
  FbArgs fx = c.plan.a;  // the exact fallback's arguments
  set_pass(fx, p);
  // folded fallback: the list kernel recomputes its own flagged pairs when its
  // persistent grid has a scratch slot per wavefront (then no launch after the pass)
  ca.xinline = 0;
  // fb_list4_kernel's statistics-accumulating variant (acc_sa: this group's statistics
  // arguments; acc_plan, acc_shape: the call's gated-statistics plan): only where
  // stats_list_m_kernel would otherwise sum them (list4_acc_eligible); it needs the
  // inline fallback, which it may take without the fold as well (several base groups)
  // unless the fold was switched off
  const Switches &sw = switches();
  const bool acc = c.list_kernel == ListKernel::kList4 && acc_sa && acc_plan && acc_shape && acc_parts &&
                   list4_acc_eligible(*acc_plan, *acc_shape, ca.T, acc_sa->Z != nullptr, sw);
  if (acc_waves) *acc_waves = 0;
  auto set_inline = [&](long long waves) {
    if (!(fold || (acc && !sw.NO_FOLD_EXACT)) || waves > kExactThreads || sw.NO_LIST_INLINE) return;
    ca.xinline = 1;
    ca.xscr = scratch;
    ca.xstride = (long long)exact_stride(fx.S, fx.SB, fx.T);
    ca.xf = fx;
  };
  if (c.list_kernel != ListKernel::kSplit) ca.Atg = c.bwd.a.Atg;
  hipEvent_t ev0 = timing_start(st);
  hipError_t e;
  switch (c.list_kernel) {
    case ListKernel::kList4: {  // one wave per quad item
      unsigned grid = resident_blocks(list4_resident_blocks(acc));
      set_inline(list4_inline_waves(ca, grid));
      if (acc && ca.xinline) {
        ca.acc = 1;
        ca.acc_nup = us_nup(acc_sa->NU);
        ca.accZ = acc_sa->Z; ca.accUs = acc_sa->Us; ca.acc_parts = acc_parts;
        if (acc_waves) *acc_waves = (int)list4_inline_waves(ca, grid);
      } else if (acc) {  // no inline fallback: the per-pair outputs, on that kernel's grid
        grid = resident_blocks(list4_resident_blocks());
        if (fold) set_inline(list4_inline_waves(ca, grid));  // (that path inlines under the fold only)
      }
      e = launch_list4(ca, grid, st);
      if (e != hipSuccess) return hip_fail(e, "fb_list4_kernel");
      g_last_kernel[1] = "vbhem::fb_list4_kernel<" + std::to_string(ca.T) + ", " + tf(list4_fast(ca));
      break;
    }
    case ListKernel::kList12:  // one wave per quad
      e = launch_list12(ca, resident_blocks(list12_resident_blocks()), st);
      if (e != hipSuccess) return hip_fail(e, "fb_list12_kernel");
      g_last_kernel[1] = "vbhem::fb_list12_kernel<" + std::to_string(ca.T) + ", " + tf(list12_fast(ca));
      break;
    case ListKernel::kSplit: {
      if (c.k1_in_kernel) set_k1_operands(c, p.i_begin, ca);
      const unsigned grid = resident_blocks(split_resident_blocks(ca, c.split.lds_l));
      if (ca.S >= kSplitInlineMinS && ca.S <= kSplitInlineMaxS) set_inline((long long)grid * ca.nwb);
      e = launch_split(ca, grid, c.split.lds_l, st);
      if (e != hipSuccess) return hip_fail(e, "fb_split_kernel(list)");
      g_last_kernel[1] = split_name(ca);
      break;
    }
  }
  timing_stop(kTimeGatedForward, ev0, st);
  if (inlined) *inlined = ca.xinline != 0;
  if (fold) return VBHEM_OK;  // inline, or launch_stats_list runs fb_exact_kernel from flag_count[3]
  return run_fb_exact(fx, scratch, st);
}

// K1 + K2-K4 over the pass's bases x all clusters.  mode kFbBackward (split path
// only) computes K2 + K3 (LL) alone; flagged pairs still get every output from the
// exact kernel.
int run_fb(const FbCtx &c, const Pass &p, double *Ebuf, long long e_ld, double *scratch,
           hipStream_t st, int mode = kFbDense, FbArgs *fold = nullptr) {
  if (p.i_end <= p.i_begin) return VBHEM_OK;
  const int nbases = p.i_end - p.i_begin;
  FbArgs a = c.plan.a;
  set_pass(a, p);
  hipError_t e = hipSuccess;
  const BwdKernel kern = mode == kFbBackward ? c.bwd_kernel : BwdKernel::kSplit;
  // K1 inside fb_bwd2_kernel (and the list pass after it): no emission GEMM
  const bool k1 = c.k1_in_kernel && mode == kFbBackward;
  if (!c.split.ok) {  // split path: zeroed by emission_prep_kernel, reset by fb_exact_kernel
    e = hipMemsetAsync(p.flags, 0, sizeof(int), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(flags)");
  } else {
    EmissionArgs ea = c.em;
    ea.i_begin = p.i_begin; ea.i_end = p.i_end; ea.i_buf0 = p.i_buf0; ea.E = Ebuf; ea.e_ld = e_ld;
    hipEvent_t em0 = !k1 ? timing_start(st) : nullptr;
    if (c.use_u) ea.U = operand(c, p.i_begin, &ea.u_col0);
    if (c.use_u && !c.base->U) {  // this call's operand for bases [i_begin, i_end), shifted like W' / bias'
      if (!c.u_ws) return set_error(VBHEM_ERR_WORKSPACE, "no operand buffer for the emission GEMM");
      const vbhem_base_t *b = c.base;
      UPrepArgs ua{};
      ua.N = b->N; ua.SB = b->SB; ua.d = b->d; ua.covmode = b->covmode;
      ua.kdp = c.em.kdp; ua.i_begin = p.i_begin; ua.i_end = p.i_end; ua.u_col0 = ea.u_col0;
      ua.nstates = b->nstates; ua.centres = b->centres; ua.covars = b->covars;
      ua.U = c.u_ws; ua.z = c.em.shift;
      e = launch_u_prep(ua, st);
      if (e != hipSuccess) return hip_fail(e, "u_prep_kernel");
    }
    if (!k1) {
      e = launch_emission(ea, c.use_u ? c.em_lds_u : c.em_lds, st);
      if (e != hipSuccess) return hip_fail(e, "emission_kernel");
      timing_stop(kTimeEmission, em0, st);
    }
  }
  // the backward-only kernels take their timing events into the dispatch itself
  // (hipExtLaunchKernelGGL: start / end of the kernel, no marker packets around it);
  // the others are bracketed by two event records
  hipEvent_t ev1 = nullptr;
  hipEvent_t ev0 = timing_start(st, true, kern != BwdKernel::kSplit ? &ev1 : nullptr);
  if (c.split.ok) {
    const SplitPlan &sp = mode == kFbBackward ? c.bwd : c.split;
    SplitArgs ca = sp.a;
    ca.mode = mode;
    ca.E = Ebuf; ca.e_ld = e_ld;
    set_pass(ca, p);
    // tiles of ppb pairs per cluster; the backward-only pass: a persistent grid, NB blocks
    // per cluster, of a kernel with per_cu resident blocks per CU
    const unsigned K = (unsigned)ca.K;
    auto tiles = [&](int ppb) { return (unsigned)((nbases + ppb - 1) / ppb); };
    auto grid = [&](int ppb, int per_cu) {
      return K * persistent_blocks(tiles(ppb), resident_blocks(per_cu), K);
    };
    const char *label = "fb_split_kernel";
    std::string targs;  // the kernel's template arguments, for vbhem_last_kernel
    switch (kern) {
      case BwdKernel::kBwd4:
        label = "fb_bwd4_kernel"; targs = tf(bwd4_o32(ca));
        if (switches().NO_BWD4_TRIM > 0) targs = bwd4_o32(ca) ? "true, false>" : "false, false>";
        e = launch_bwd4(ca, grid(bwd4_ppb(), bwd4_resident_blocks()), st, ev0, ev1);
        break;
      case BwdKernel::kBwd12:
        label = "fb_bwd12_kernel"; targs = tf(bwd12_o32(ca));
        e = launch_bwd12(ca, grid(bwd12_ppb(), bwd12_resident_blocks()), st, ev0, ev1);
        break;
      case BwdKernel::kBwd2: {
        ca.nwb = c.bwd2_nwb;
        if (k1) set_k1_operands(c, p.i_begin, ca);
        if (k1 && c.fpre) {
          ca.prep = 1;
          ca.pm = c.em.m; ca.pP = c.em.P; ca.pc = c.em.c; ca.pz = c.em.zfix; ca.pshift = c.em.shift;
          ca.ftag = reinterpret_cast<unsigned long long *>(c.fpre);
          ca.ftag_val = flag_tag();
        }
        label = "fb_bwd2_kernel"; targs = std::to_string(ca.S) + ">";
        // vbhem_debug_extra_lds(n): n more bytes of dynamic LDS -- fault injection for the
        // tests of a refused launch (tests/test_robustness.py), never set in production
        const size_t lds2 = c.bwd2_lds + g_debug_extra_lds.load(std::memory_order_relaxed);
        e = launch_bwd2(ca, grid(c.bwd2_ppb, bwd2_resident_blocks(ca.S, ca.nwb, c.bwd2_lds)), lds2,
                        st, ev0, ev1);
        break;
      }
      case BwdKernel::kSplit:  // dense: a block per tile and cluster
        if (mode == kFbBackward)
          e = launch_split(ca, grid(sp.ppb, split_resident_blocks(ca, sp.lds_bwd)), sp.lds_bwd, st);
        else e = launch_split(ca, K * tiles(sp.ppb), sp.lds, st);
    }
    if (e != hipSuccess) return hip_fail(e, label);
    g_last_kernel[0] = kern == BwdKernel::kSplit ? split_name(ca)
                                                 : std::string("vbhem::") + label + "<" + targs;
  } else {
    const int nib = (nbases + a.BI - 1) / a.BI;
    const dim3 grid((unsigned)nib * (unsigned)a.njb);
    e = launch_fb(a, grid, c.plan.block, c.plan.lds, st);
    if (e != hipSuccess) return hip_fail(e, "fb_pairs_kernel");
    g_last_kernel[0] = "vbhem::fb_pairs_kernel";
  }
  timing_stop(kTimeFb, ev0, st, ev1, (long long)nbases * a.K);
  if (fold) {  // resp_kernel takes the flagged pairs (StatsArgs::fold): no exact launch
    *fold = a;
    return VBHEM_OK;
  }
  return run_fb_exact(a, scratch, st);
}

}  // namespace

namespace vbhem {

const char *last_kernel(int pass) {
  return (pass >= 0 && pass <= 3) ? g_last_kernel[pass].c_str() : "";
}

size_t pairs_workspace_bytes(const vbhem_base_t *b, const vbhem_cluster_t *c, int T, bool need_tnu) {
  Ws w;
  return carve_pairs(nullptr, b, c, T, need_tnu, w);
}

size_t fused_workspace_bytes(const vbhem_base_t *b, const vbhem_cluster_t *c, int T, int R) {
  Ws w;
  return carve_fused(nullptr, b, c, T, w, R);
}

int sched_estep_pairs(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T, double smooth,
                      double *LL_elbo_dev, double *sum_nu_1_dev, double *emit_pr_dev,
                      double *emit_mu_dev, double *emit_Mu_dev, double *sum_xi_dev,
                      double *sum_t_nu_dev, void *workspace_dev, size_t workspace_bytes,
                      void *stream) {
  Ws w;
  const size_t need = carve_pairs(nullptr, base, clus, T, sum_t_nu_dev == nullptr, w);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  carve_pairs(workspace_dev, base, clus, T, sum_t_nu_dev == nullptr, w);
  double *tnu = sum_t_nu_dev ? sum_t_nu_dev : w.tnu;
  hipStream_t st = static_cast<hipStream_t>(stream);
  FbCtx ctx;
  int rc = prepare_fb(ctx, base, clus, T, smooth);
  if (rc != VBHEM_OK) return rc;
  ctx.u_ws = w.U;
  hipError_t e = hipSuccess;
  if (!ctx.split.ok) {
    e = hipMemsetAsync(w.fpre, 0, kHeadInts * sizeof(int), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(flags)");
  }
  rc = run_emission_prep(ctx, w.W, w.bias, w.shift, st, w.fpre, kHeadInts);
  if (rc != VBHEM_OK) return rc;
  rc = run_fb(ctx, Pass{0, base->N, 0, LL_elbo_dev, sum_nu_1_dev, sum_xi_dev, tnu, w.flags}, w.E,
              (long long)base->N * base->SB, w.scratch, st);
  if (rc != VBHEM_OK) return rc;
  EmitArgs ea{};
  ea.SB = base->SB; ea.d = base->d; ea.covmode = base->covmode; ea.K = clus->K; ea.S = clus->S;
  ea.i_begin = 0; ea.i_end = base->N;
  ea.centres = base->centres; ea.covars = base->covars; ea.tnu = tnu;
  ea.emit_pr = emit_pr_dev; ea.emit_mu = emit_mu_dev; ea.emit_Mu = emit_Mu_dev;
  e = launch_emit(ea, st);
  if (e != hipSuccess) return hip_fail(e, "pair_emit_kernel");
  return VBHEM_OK;
}

int sched_estep_fused(const vbhem_base_t *base, const vbhem_cluster_t *clus, int R, int T,
                      const double *tildeN_dev, const double *logOmega_dev, double *stats_dev,
                      double *hatZ_dev, double *LL_elbo_dev, void *workspace_dev,
                      size_t workspace_bytes, void *stream, const VhemIn *vh,
                      unsigned long long *done_word, unsigned long long done_val) {
  Ws w;
  const size_t need = carve_fused(nullptr, base, clus, T, w, R);
  if (!workspace_dev || workspace_bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
  carve_fused(workspace_dev, base, clus, T, w, R);
  hipStream_t st = static_cast<hipStream_t>(stream);

  // statistics kernels' geometry
  const int K = clus->K, S = clus->S, SB = base->SB, d = base->d;
  StatsArgs sa{};
  sa.K = K; sa.S = S; sa.SB = SB; sa.d = d; sa.covmode = base->covmode;
  sa.NU = (int)vbhem_stats_nu(d, base->covmode);
  sa.slab_len = w.slab_len;
  sa.KT = K / R;
  sa.SL = w.slab_len / R;
  sa.centres = base->centres; sa.covars = base->covars; sa.LL = LL_elbo_dev;
  sa.nu1 = w.nu1; sa.xi = w.xi; sa.tnu = w.tnu; sa.tildeN = tildeN_dev; sa.logOmega = logOmega_dev;
  sa.Z = w.Z; sa.hatZ = hatZ_dev; sa.slabs = w.slabs;
  if (vh) {  // Z: the weights w = Z omega_b; hatZ: Z (vhem_resp_kernel)
    sa.vhem = 1;
    sa.omegaB = vh->omegaB;
    sa.inf_norm = vh->inf_norm;
  }

  FbCtx ctx;
  int rc = prepare_fb(ctx, base, clus, T, vh ? vh->smooth : 1.0, vh != nullptr);
  if (rc != VBHEM_OK) return rc;
  ctx.u_ws = w.U;
  const Switches &sw = switches();  // this thread's set, fixed for the call
  // the epilogue's plans (vbhem_stats_plan.h), once per call.  The emission GEMM's operand
  // serves the statistics too: the prepared one with its statistics copy, or the one
  // run_fb builds per group
  const bool opnd = ctx.split.ok && ctx.use_u;
  const StatsShape shape{K, K / R, S, SB, d, base->covmode, opnd ? ctx.em.kdp : 0,
                         opnd && (base->U || ctx.u_ws), opnd && base->U, vh != nullptr};
  const DensePlan dense = plan_stats_dense(shape);
  sa.SBp = dense.SBp; sa.UST = dense.UST; sa.JG = dense.JG; sa.NBB = dense.NBB; sa.AST = dense.AST;
  const GatedPlan gplan = plan_stats_gated(shape, std::min(base->N, w.group), sw);
  sa.PB = gplan.PB;
  // gated schedule: split kernel + list statistics tile must apply
  // (gate lists: per-wave ballot masks of all K clusters in LDS, K up to ~2,400)
  const bool gated = !sw.FUSED_DENSE && ctx.split.ok && ctx.split.lds_l && gplan.ok &&
                     gate_list_lds(K) <= kLdsLimit;
  if (R > 1 && !gated)
    return set_error(VBHEM_ERR_UNSUPPORTED,
                     "trials need the gated schedule (split-kernel shapes: S <= 16, Sb <= S)");
  if (!gated && !dense.ok)
    return set_error(VBHEM_ERR_UNSUPPORTED, "statistics tile does not fit (S or d too large)");
  sa.gate_cnt = gated ? w.gate_cnt : nullptr;
  sa.list = w.list; sa.list_tot = w.list_tot; sa.list_cap = w.group;
  // K <= 64: the responsibility kernel leaves a gate mask per base, gate_list_kernel
  // ranks from those instead of reading Z again
  sa.gmask = gated && !sw.NO_GATE_MASKS ? w.gmask : nullptr;
  // chunks of >= kChunkMinBases bases; the first group has the most, and in the
  // gated schedule its kernels write (not add to) every entry of slabs [0, nslab_used)
  auto chunks = [&w](int nb) { return std::min(w.nslab, (nb + kChunkMinBases - 1) / kChunkMinBases); };
  const int nslab_used = std::max(1, chunks(std::min(base->N, w.group)));
  // the MFMA statistics kernel: at most 128 parts per cluster (stats_final_kernel then
  // sums 128 slabs of the N1 / M / U columns instead of every chunk's: C4 28 -> 7 MB)
  sa.nzero_m = std::min(nslab_used, 128);
  int stats_slabs = nslab_used;
  hipError_t e = hipSuccess;
  if (!gated || base->N == 0) {
    e = hipMemsetAsync(w.slabs, 0, sizeof(double) * (size_t)nslab_used * w.slab_len, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(slabs)");
  }
  // a call that returns early leaves the flag head zeroed (tag included): the next
  // call's in-kernel preparation then zeroes the counters itself
  struct HeadGuard {
    int *fpre;
    hipStream_t st;
    ~HeadGuard() {
      if (fpre) (void)hipMemsetAsync(fpre, 0, kHeadInts * sizeof(int), st);
    }
  } guard{w.fpre, st};
  if (!ctx.split.ok) {
    e = hipMemsetAsync(w.fpre, 0, kHeadInts * sizeof(int), st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(flags)");
  }
  if (gated) ctx.bwd.a.Atg = w.Atg;
  // K1 inside fb_bwd2_kernel on a prepared operand: W' / bias' / A' and the counters'
  // reset inside that kernel too (no emission_prep_kernel launch)
  // (thread 448 of the block runs the flag-head handshake: blocks of >= 8 waves only;
  // smaller ones, e.g. a VBHEM_BWD2_WAVES build, take the emission_prep_kernel path)
  if (gated && ctx.k1_in_kernel && ctx.em.zfix && ctx.bwd2_nwb * 64 >= 512 &&
      !sw.NO_BWD2_PREP) {
    ctx.em.W = w.W; ctx.em.bias = w.bias; ctx.em.shift = w.shift;
    ctx.fpre = w.fpre;
  } else {
    rc = run_emission_prep(ctx, w.W, w.bias, w.shift, st, w.fpre, kHeadInts,
                           gated ? w.Atg : nullptr, clus->logA);
    if (rc != VBHEM_OK) return rc;
  }
  // the backward pass's exact fallback folded into resp_kernel (one base group, one
  // trial: one fb_exact_kernel launch less per E-step; the gate-list pass's flags get
  // their launch in launch_stats_list, from flag_count[3]); resp_kernel needs a
  // scratch slot per chunk block: at most kExactThreads chunks
  const bool fold = gated && R == 1 && base->N <= w.group && ctx.split.ok && K < kExactThreads &&
                    w.nslab <= kExactThreads && !sw.NO_FOLD_EXACT;
  sa.fold = 0;
  const RespPlan resp = plan_resp(shape, fold, sw);
  const GatedPlan l4reduce = plan_list4_reduce(shape);
  // one base group whose gate-list pass accumulated the gated sums: the finishing kernel
  // reduces the partials itself (stats_final_fold_kernel: no list4_stats_reduce_kernel
  // launch, no pass through slab 0); final_l4w: that pass's waves, final_ev0: the
  // statistics span left open for it
  const bool may_fold_final = base->N <= w.group && !sw.NO_FINAL_FOLD;
  int final_l4w = 0;
  hipEvent_t final_ev0 = nullptr;
  for (int g0 = 0; g0 < base->N; g0 += w.group) {
    const int g1 = std::min(base->N, g0 + w.group);
    const long long e_ld = (long long)w.group * SB;
    const Pass pass{g0, g1, g0, LL_elbo_dev, w.nu1, w.xi, w.tnu, w.flags};
    rc = run_fb(ctx, pass, w.E, e_ld, w.scratch, st, gated ? kFbBackward : kFbDense,
                fold ? &sa.fx : nullptr);
    if (rc != VBHEM_OK) return rc;
    if (fold) {
      sa.fold = 1;
      sa.xscratch = w.scratch;
      sa.xstride = (long long)exact_stride(S, SB, T);
      sa.xslots = kExactThreads;
    }
    sa.i_begin = g0; sa.i_end = g1; sa.i_buf0 = g0;
    sa.assign = gated && g0 == 0;
    // the emission GEMM's operand for this group (prepared, or built by run_fb)
    sa.U = sa.Us = nullptr;
    if (ctx.split.ok && ctx.use_u) {
      sa.ukdp = ctx.em.kdp;
      if (base->U || ctx.u_ws) sa.U = operand(ctx, g0, &sa.u_col0);
      if (sa.U) sa.uz = base->U ? base->U : ctx.em.shift;  // a prepared operand's head, or this call's shift
      if (base->U) sa.Us = base->U + u_doubles((long long)base->N * SB, base->d, base->covmode);
    }
    const int nchunk = std::max(1, chunks(g1 - g0));
    hipEvent_t ev0 = timing_start(st);
    e = launch_resp(sa, resp, nchunk, st);
    if (e != hipSuccess) return hip_fail(e, "resp_kernel");
    if (gated) {
      e = launch_gate_list(sa, nchunk, st);
      if (e != hipSuccess) return hip_fail(e, "gate_list_kernel");
      timing_stop(kTimeStats, ev0, st);
      bool inl = false;
      int l4w = 0;  // > 0: fb_list4_kernel accumulated the statistics, on that many waves
      rc = run_fb_list(ctx, pass, w.E, e_ld, w.list, w.list_tot, w.group, w.scratch, st, fold, &inl,
                       &sa, &gplan, &shape, w.l4parts, &l4w);
      if (rc != VBHEM_OK) return rc;
      if (fold) sa.fold = inl ? 2 : 1;  // 2: no fb_exact_kernel launch before the statistics
      ev0 = timing_start(st);
      int ss = 0;
      if (l4w > 0) {
        ss = l4reduce.stats_slabs;
        g_last_kernel[2] = "vbhem::list4_stats_reduce_kernel";
        if (may_fold_final && sa.assign) {
          final_l4w = l4w;
          final_ev0 = ev0;
          break;  // (the only group)
        }
        e = launch_list4_stats_reduce(sa, l4reduce, w.l4parts, l4w, st);
        if (e != hipSuccess) return hip_fail(e, "list4_stats_reduce_kernel");
      } else {
        const GatedPlan gp = plan_gated_group(gplan, shape, nchunk, sa.nzero_m, sa.fold, sw);
        ss = gp.stats_slabs;
        g_last_kernel[2] = "vbhem::stats_list_kernels";
        e = launch_stats_list(sa, gp, st);
      }
      if (e != hipSuccess) return hip_fail(e, "stats_list_kernel");
      if (g0 == 0) stats_slabs = ss;  // later groups add into [0, ss) with ss <= this
    } else {
      e = launch_stats(sa, dense, nchunk, st);
      if (e != hipSuccess) return hip_fail(e, "stats_kernel");
    }
    timing_stop(kTimeStats, ev0, st);
  }
  if (final_l4w > 0) {
    e = launch_stats_final_fold(sa, l4reduce, w.l4parts, final_l4w, nslab_used, stats_dev, st, w.fpre,
                                done_word, done_val);
    if (e != hipSuccess) return hip_fail(e, "stats_final_fold_kernel");
    g_last_kernel[3] = "vbhem::stats_final_fold_kernel";
    timing_stop(kTimeStats, final_ev0, st);
  } else {
    e = launch_stats_final(w.slabs, nslab_used, stats_slabs, w.slab_len, sa.KT, S, sa.SL, stats_dev,
                           st, w.fpre, done_word, done_val);
    if (e != hipSuccess) return hip_fail(e, "stats_final_kernel");
    g_last_kernel[3] = "vbhem::stats_final_kernel";
  }
  guard.fpre = nullptr;
  return VBHEM_OK;
}

}  // namespace vbhem

extern "C" size_t vbhem_debug_extra_lds(size_t bytes) { return g_debug_extra_lds.exchange(bytes); }

extern "C" size_t vbhem_fused_workspace_layout(const vbhem_base_t *base, const vbhem_cluster_t *clus,
                                               int T, int R, long long *out) {
  if (!base || !clus || !out || R < 1) return 0;
  Ws w;
  char *const origin = reinterpret_cast<char *>(256);  // (an address to measure from, never read)
  const size_t bytes = carve_fused(origin, base, clus, T, w, R);
  auto at = [&](const void *q) { return q ? (long long)(static_cast<const char *>(q) - origin) : -1ll; };
  out[0] = w.group;
  out[1] = at(w.list);
  out[2] = at(w.list_tot);
  out[3] = at(w.gmask);
  out[4] = at(w.scratch);
  return bytes;
}

extern "C" int vbhem_bwd4_launch_plan(int K, int nbases, int *out) {
  if (K < 1 || nbases < 1 || !out) return VBHEM_ERR_ARG;
  const unsigned ppb = (unsigned)vbhem::bwd4_ppb();
  const unsigned tiles = ((unsigned)nbases + ppb - 1) / ppb;
  out[0] = vbhem::bwd4_ppb() / vbhem::bwd4_waves();
  out[1] = vbhem::bwd4_waves();
  out[2] = (int)vbhem::persistent_blocks(tiles, resident_blocks(vbhem::bwd4_resident_blocks()),
                                        (unsigned)K);
  return VBHEM_OK;
}
