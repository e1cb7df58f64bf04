// vbhem_capi.hip -- C ABI of libvbhem_estep.so (declared in include/vbhem_estep.h):
// the last error, the switch table, and the device-pointer E-step entries, which
// validate their arguments and hand over to the scheduler (vbhem_estep_sched.hip).
// No allocation, no host synchronisation on those entry points (graph-capturable).
// The timing entries are in vbhem_timing.hip, the host-array ones in
// vbhem_estep_host.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_estep_plan.h"
#include "vbhem_estep_sched.h"
#include "vbhem_internal.h"
#include "vbhem_stats_plan.h"

namespace {

thread_local std::string g_err;

// The switch table (vbhem_switches.h) by index, for the vbhem_switch_* functions
struct SwitchRow {
  const char *name;  // with the VBHEM_ prefix, as in the environment
  long long unset;
  long long vbhem::Switches::*field;
};
constexpr SwitchRow kSwitchRows[] = {
#define X(name, unset, doc) {"VBHEM_" #name, unset, &vbhem::Switches::name},
    VBHEM_SWITCHES(X)
#undef X
};
constexpr int kSwitchCount = (int)(sizeof(kSwitchRows) / sizeof(kSwitchRows[0]));

// a boolean switch holds 0 or 1; an integer one any value (negative: not set)
long long switch_value(const SwitchRow &r, long long v) { return r.unset == 0 ? (v != 0) : v; }

// the process default: the environment, read once (the library's only getenv)
const vbhem::Switches &default_switches() {
  static const vbhem::Switches def = [] {
    vbhem::Switches s;
    for (const SwitchRow &r : kSwitchRows)
      if (const char *ev = std::getenv(r.name)) {
        if (r.unset == 0) s.*r.field = ev[0] != '\0' && std::strcmp(ev, "0") != 0;
        else s.*r.field = std::strtoll(ev, nullptr, 10);
      }
    return s;
  }();
  return def;
}
// the set of this host thread (the fused schedule, vbhem_set_fused_mode, is its
// FUSED_DENSE entry)
thread_local vbhem::Switches g_switches = default_switches();

const SwitchRow *find_switch(const char *name) {
  if (!name) return nullptr;
  if (std::strncmp(name, "VBHEM_", 6) == 0) name += 6;
  for (const SwitchRow &r : kSwitchRows)
    if (std::strcmp(name, r.name + 6) == 0) return &r;
  return nullptr;
}

}  // namespace

namespace vbhem {

const Switches &switches() { return g_switches; }

// shared by every C-ABI translation unit: vbhem_last_error()
int set_error(int code, const std::string &msg) {
  g_err = msg;
  // a refused launch (too much LDS, a bad grid) also leaves HIP's per-thread last
  // error set; left pending it would surface in the caller's next, unrelated HIP
  // call (torch checks hipGetLastError after each of its launches).  The error is
  // reported here, through the status and vbhem_last_error(), so it is consumed.
  if (code == VBHEM_ERR_HIP) (void)hipGetLastError();
  return code;
}

// this process's clean tag of the flag head (kFlagPre): random, never 0 (a zeroed head)
unsigned long long flag_tag() {
  static const unsigned long long t = [] {
    std::random_device rd;
    unsigned long long v = ((unsigned long long)rd() << 32) ^ rd();
    v ^= (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
    return v | 1ull;
  }();
  return t;
}

int check_inputs(const vbhem_base_t *b, const vbhem_cluster_t *c, int T, bool need_ptrs) {
  if (!b || !c) return set_error(VBHEM_ERR_ARG, "null base or cluster descriptor");
  if (b->N < 0 || b->SB < 1 || b->d < 1 || c->K < 1 || c->S < 1 || T < 1)
    return set_error(VBHEM_ERR_ARG, "invalid sizes (need N>=0, SB>=1, d>=1, K>=1, S>=1, T>=1)");
  if (b->covmode != VBHEM_COV_DIAG && b->covmode != VBHEM_COV_FULL)
    return set_error(VBHEM_ERR_ARG, "covmode must be VBHEM_COV_DIAG or VBHEM_COV_FULL");
  if (need_ptrs && b->N > 0 &&
      (!b->prior || !b->A || !b->centres || !b->covars || !c->logA || !c->logPi || !c->m ||
       !c->P || !c->c))
    return set_error(VBHEM_ERR_ARG, "null input array");
  if ((long long)b->N * c->K > 0x7fffffffLL)
    return set_error(VBHEM_ERR_UNSUPPORTED, "N*K exceeds 2^31-1 pairs per call; shard the bases");
  return VBHEM_OK;
}

}  // namespace vbhem

namespace {

using vbhem::check_inputs;
using vbhem::hip_fail;
using vbhem::set_error;

// vbhem_arm_done_word: the completion word of the next fused call (taken by that call)
std::atomic<unsigned long long *> g_done_word{nullptr};
std::atomic<unsigned long long> g_done_val{0};

int estep_fused_checked(const vbhem_base_t *base, const vbhem_cluster_t *clus, int R, int T,
                        const double *tildeN_dev, const double *logOmega_dev, double *stats_dev,
                        double *hatZ_dev, double *LL_elbo_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream, const vbhem::VhemIn *vh) {
  // (taken first: a call that fails leaves nothing armed for the next one)
  unsigned long long *const done_word = g_done_word.exchange(nullptr);
  const unsigned long long done_val = g_done_val.load();
  int rc = check_inputs(base, clus, T);
  if (rc != VBHEM_OK) return rc;
  if (vh) {
    if (!(vh->smooth > 0.0) || !std::isfinite(vh->smooth))
      return set_error(VBHEM_ERR_ARG, "smooth must be a positive finite number");
    if (!(vh->inf_norm > 0.0) || !std::isfinite(vh->inf_norm))
      return set_error(VBHEM_ERR_ARG, "inf_norm must be a positive finite number");
    if (base->N > 0 && !vh->omegaB) return set_error(VBHEM_ERR_ARG, "null fused argument");
  }
  if (R < 1 || clus->K % R != 0)
    return set_error(VBHEM_ERR_ARG, "trials: K must be a positive multiple of R");
  if (!vh && R > 1 && clus->K > 256)  // (resp_trials_kernel; vhem_resp_kernel has no such limit)
    return set_error(VBHEM_ERR_UNSUPPORTED, "trials: at most 256 clusters in total (R * K_trial)");
  if (!logOmega_dev || !stats_dev ||
      (base->N > 0 && (!tildeN_dev || !hatZ_dev || !LL_elbo_dev)))
    return set_error(VBHEM_ERR_ARG, "null fused argument");
  if ((vh ? vbhem::vhem_resp_lds(clus->K, clus->K / R) : vbhem::resp_lds(clus->K, clus->K / R)) >
      vbhem::kLdsLimit)
    return set_error(VBHEM_ERR_UNSUPPORTED, "fused: too many clusters for the responsibilities "
                                            "kernel (K <= ~2,400)");
  return vbhem::sched_estep_fused(base, clus, R, T, tildeN_dev, logOmega_dev, stats_dev, hatZ_dev,
                                  LL_elbo_dev, workspace_dev, workspace_bytes, stream, vh, done_word,
                                  done_val);
}

}  // namespace

extern "C" {

const char *vbhem_last_error(void) { return g_err.c_str(); }

const char *vbhem_last_kernel(int pass) { return vbhem::last_kernel(pass); }

const char *vbhem_version(void) { return "vbhem-mi355x 0.1.0 (gfx950)"; }

size_t vbhem_stats_nu(int d, int covmode) {
  return covmode == VBHEM_COV_FULL ? (size_t)1 + d + (size_t)d * (d + 1) / 2 : (size_t)1 + 2 * d;
}

size_t vbhem_stats_len(int K, int S, int d, int covmode) {
  return (size_t)K + (size_t)K * S + (size_t)K * S * S + 2 + (size_t)K * S * vbhem_stats_nu(d, covmode);
}

size_t vbhem_prepare_base_bytes(const vbhem_base_t *base) {
  if (!base || base->N < 0 || base->SB < 1 || base->d < 1 || base->d > vbhem::kUHead ||
      (base->covmode != VBHEM_COV_DIAG && base->covmode != VBHEM_COV_FULL))
    return 0;
  if (vbhem::emission_kdp(base->d, base->covmode) / 4 > vbhem::kUMaxKq) return 0;
  // the emission GEMM's operand U, then its statistics copy Us (vbhem_internal.h)
  return (vbhem::u_doubles((long long)base->N * base->SB, base->d, base->covmode) +
          vbhem::us_doubles(base->N, base->SB, base->d, base->covmode)) * sizeof(double);
}

int vbhem_prepare_base(const vbhem_base_t *base, double *U_dev, size_t bytes, void *stream) {
  const size_t need = vbhem_prepare_base_bytes(base);
  if (need == 0)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhem_prepare_base: invalid descriptor or d too large");
  if (!U_dev || bytes < need)
    return set_error(VBHEM_ERR_WORKSPACE, "vbhem_prepare_base: need " + std::to_string(need) + " bytes");
  if (base->N > 0 && (!base->centres || !base->covars))
    return set_error(VBHEM_ERR_ARG, "vbhem_prepare_base: null base array");
  vbhem::UPrepArgs ua{};
  ua.N = base->N; ua.SB = base->SB; ua.d = base->d; ua.covmode = base->covmode;
  ua.kdp = vbhem::emission_kdp(base->d, base->covmode);
  ua.i_begin = 0; ua.i_end = base->N; ua.u_col0 = 0;
  ua.nstates = base->nstates; ua.centres = base->centres; ua.covars = base->covars;
  ua.U = U_dev; ua.z = nullptr;  // shift = mean of the valid base means
  hipError_t e = vbhem::launch_u_prep(ua, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "u_prep_kernel");
  e = vbhem::launch_us_build(ua, U_dev + vbhem::u_doubles((long long)base->N * base->SB, base->d,
                                                         base->covmode),
                             static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "us_build_kernel");
  return VBHEM_OK;
}

size_t vbhem_pairs_workspace_bytes(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T) {
  if (check_inputs(base, clus, T, false) != VBHEM_OK) return 0;
  return vbhem::pairs_workspace_bytes(base, clus, T, true);
}

int vbhem_estep_pairs(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T,
                      double *LL_elbo_dev, double *sum_nu_1_dev, double *emit_pr_dev,
                      double *emit_mu_dev, double *emit_Mu_dev, double *sum_xi_dev,
                      double *sum_t_nu_dev, void *workspace_dev, size_t workspace_bytes,
                      void *stream) {
  return vhem_estep_pairs(base, clus, T, 1.0, LL_elbo_dev, sum_nu_1_dev, emit_pr_dev, emit_mu_dev,
                          emit_Mu_dev, sum_xi_dev, sum_t_nu_dev, workspace_dev, workspace_bytes,
                          stream);
}

int vhem_estep_pairs(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T, double smooth,
                     double *LL_elbo_dev, double *sum_nu_1_dev, double *emit_pr_dev,
                     double *emit_mu_dev, double *emit_Mu_dev, double *sum_xi_dev,
                     double *sum_t_nu_dev, void *workspace_dev, size_t workspace_bytes,
                     void *stream) {
  if (!(smooth > 0.0) || !std::isfinite(smooth))
    return set_error(VBHEM_ERR_ARG, "smooth must be a positive finite number");
  int rc = check_inputs(base, clus, T);
  if (rc != VBHEM_OK) return rc;
  if (base->N == 0) return VBHEM_OK;
  if (!LL_elbo_dev || !sum_nu_1_dev || !emit_pr_dev || !emit_mu_dev || !emit_Mu_dev || !sum_xi_dev)
    return set_error(VBHEM_ERR_ARG, "null output array");
  return vbhem::sched_estep_pairs(base, clus, T, smooth, LL_elbo_dev, sum_nu_1_dev, emit_pr_dev,
                                  emit_mu_dev, emit_Mu_dev, sum_xi_dev, sum_t_nu_dev, workspace_dev,
                                  workspace_bytes, stream);
}

size_t vbhem_fused_workspace_bytes(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T) {
  return vbhem_fused_trials_workspace_bytes(base, clus, 1, T);
}

size_t vbhem_fused_trials_workspace_bytes(const vbhem_base_t *base, const vbhem_cluster_t *clus,
                                          int R, int T) {
  if (check_inputs(base, clus, T, false) != VBHEM_OK || R < 1 || clus->K % R != 0) return 0;
  return vbhem::fused_workspace_bytes(base, clus, T, R);
}

int vbhem_estep_fused(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T,
                      const double *tildeN_dev, const double *logOmega_dev, double *stats_dev,
                      double *hatZ_dev, double *LL_elbo_dev, void *workspace_dev,
                      size_t workspace_bytes, void *stream) {
  return vbhem_estep_fused_trials(base, clus, 1, T, tildeN_dev, logOmega_dev, stats_dev, hatZ_dev,
                                  LL_elbo_dev, workspace_dev, workspace_bytes, stream);
}

int vbhem_arm_done_word(void *word, unsigned long long value) {
  if (word && reinterpret_cast<uintptr_t>(word) % 8 != 0) return set_error(VBHEM_ERR_ARG, "done word not 8-byte aligned");
  g_done_val.store(value);
  g_done_word.store(static_cast<unsigned long long *>(word));
  return VBHEM_OK;
}

int vbhem_done_word_alloc(void **host_ptr, void **dev_ptr) {
  if (!host_ptr || !dev_ptr) return set_error(VBHEM_ERR_ARG, "null pointer");
  void *h = nullptr;
  hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(done word)");
  std::memset(h, 0, 64);
  void *d = nullptr;
  e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(h);
    return hip_fail(e, "hipHostGetDevicePointer(done word)");
  }
  *host_ptr = h;
  *dev_ptr = d;
  return VBHEM_OK;
}

int vbhem_done_word_free(void *host_ptr) {
  if (!host_ptr) return VBHEM_OK;
  const hipError_t e = hipHostFree(host_ptr);
  return e == hipSuccess ? VBHEM_OK : hip_fail(e, "hipHostFree(done word)");
}

int vbhem_estep_fused_trials(const vbhem_base_t *base, const vbhem_cluster_t *clus, int R, int T,
                             const double *tildeN_dev, const double *logOmega_dev,
                             double *stats_dev, double *hatZ_dev, double *LL_elbo_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream) {
  return estep_fused_checked(base, clus, R, T, tildeN_dev, logOmega_dev, stats_dev, hatZ_dev,
                             LL_elbo_dev, workspace_dev, workspace_bytes, stream, nullptr);
}

size_t vhem_fused_workspace_bytes(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T) {
  return vbhem_fused_trials_workspace_bytes(base, clus, 1, T);
}

size_t vhem_fused_trials_workspace_bytes(const vbhem_base_t *base, const vbhem_cluster_t *clus,
                                         int R, int T) {
  return vbhem_fused_trials_workspace_bytes(base, clus, R, T);
}

int vhem_estep_fused(const vbhem_base_t *base, const vbhem_cluster_t *clus, int T, double smooth,
                     const double *Ni_dev, const double *omegaB_dev, double inf_norm,
                     const double *logOmega_dev, double *stats_dev, double *Z_dev,
                     double *LL_elbo_dev, void *workspace_dev, size_t workspace_bytes,
                     void *stream) {
  return vhem_estep_fused_trials(base, clus, 1, T, smooth, Ni_dev, omegaB_dev, inf_norm,
                                 logOmega_dev, stats_dev, Z_dev, LL_elbo_dev, workspace_dev,
                                 workspace_bytes, stream);
}

int vhem_estep_fused_trials(const vbhem_base_t *base, const vbhem_cluster_t *clus, int R, int T,
                            double smooth, const double *Ni_dev, const double *omegaB_dev,
                            double inf_norm, const double *logOmega_dev, double *stats_dev,
                            double *Z_dev, double *LL_elbo_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream) {
  const vbhem::VhemIn vh{smooth, inf_norm, omegaB_dev};
  return estep_fused_checked(base, clus, R, T, Ni_dev, logOmega_dev, stats_dev, Z_dev, LL_elbo_dev,
                             workspace_dev, workspace_bytes, stream, &vh);
}

int vbhem_set_fused_mode(int mode) {
  const int prev = g_switches.FUSED_DENSE ? VBHEM_FUSED_DENSE : VBHEM_FUSED_GATED;
  if (mode == VBHEM_FUSED_GATED || mode == VBHEM_FUSED_DENSE)
    g_switches.FUSED_DENSE = mode == VBHEM_FUSED_DENSE;
  return prev;
}

int vbhem_switch_count(void) { return kSwitchCount; }

const char *vbhem_switch_name(int index) {
  return index >= 0 && index < kSwitchCount ? kSwitchRows[index].name : nullptr;
}

int vbhem_switch_get(const char *name, long long *value) {
  const SwitchRow *r = find_switch(name);
  if (!r) return set_error(VBHEM_ERR_ARG, std::string("unknown switch: ") + (name ? name : "(null)"));
  if (value) *value = g_switches.*r->field;
  return VBHEM_OK;
}

int vbhem_switch_set(const char *name, long long value, long long *previous) {
  const SwitchRow *r = find_switch(name);
  if (!r) return set_error(VBHEM_ERR_ARG, std::string("unknown switch: ") + (name ? name : "(null)"));
  if (previous) *previous = g_switches.*r->field;
  g_switches.*r->field = switch_value(*r, value);
  return VBHEM_OK;
}

void vbhem_switch_reset(void) { g_switches = default_switches(); }

int vbhem_last_fallback_count(void *stream, const void *workspace_dev) {
  // the flag head leads the workspace (vbhem_internal.h kFlagPre): a fused call
  // leaves its total in [2] and the counters zeroed; the pairs path zeroes [2] and
  // leaves its count in the counters ([1] the total, [0] the last pass's)
  int v[vbhem::kFlagPre + 2] = {0};
  if (!workspace_dev) return set_error(VBHEM_ERR_ARG, "null workspace");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(v, workspace_dev, sizeof(v), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "vbhem_last_fallback_count");
  if (v[vbhem::kFlagLost] == vbhem::kFlagLostMark)
    return set_error(VBHEM_ERR_WORKSPACE, "fb_bwd2_kernel lost the flag-head handshake: the fused "
                                          "call's statistics are NaN (results untrusted)");
  return std::max(v[2], std::max(v[vbhem::kFlagPre], v[vbhem::kFlagPre + 1]));
}

int vbhem_host_device_pointer(void *host_ptr, void **dev_ptr) {
  if (!host_ptr || !dev_ptr) return set_error(VBHEM_ERR_ARG, "null pointer");
  *dev_ptr = nullptr;
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, host_ptr) != hipSuccess || at.type != hipMemoryTypeHost) {
    (void)hipGetLastError();
    return set_error(VBHEM_ERR_ARG, "not pinned host memory");
  }
  void *d = nullptr;
  hipError_t e = hipHostGetDevicePointer(&d, host_ptr, 0);
  if (e != hipSuccess || !d) {
    (void)hipGetLastError();
    return set_error(VBHEM_ERR_ARG, "pinned host memory is not mapped for the device");
  }
  *dev_ptr = d;
  return VBHEM_OK;
}

}  // extern "C"
