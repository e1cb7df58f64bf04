// vbhem_resp.hip -- the fused E-step epilogue's responsibilities (gfx950).
//
//   resp_kernel        hat_Z / Z = hat_Z * tilde_N per base (vbhem_h3m_c_step_fc.m:271-283)
//                      and the per-chunk partial sums Nj = sum_i Z (:282),
//                      Lt1 = sum Z .* L_elbo, Lt7 = sum hat_Z .* log(hat_Z)
//                      (vbhemh3m_lb.m:90, 107).
//   resp_trials_kernel the same for R independent EM trials batched as one cluster set
//   vhem_resp_kernel   the VHEM mode's responsibilities Z, weights w = Z omega_b and
//                      partial sums Nj, LogL (hem_h3m_c_step.m:293-314, 430, 443); the
//                      statistics kernels then sum under its gate w > 0 (Gate<kGateVhem>)
// For K <= 64 each of them also stores the gate mask of every base (StatsArgs::gmask), from
// the comparison that feeds the per-chunk gate counts; gate_list_kernel ranks from those.
// Grid: x = chunk of consecutive bases.  All sums run in a fixed order (no atomics on
// doubles).  Which kernel runs: plan_resp (vbhem_stats_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vbhem_internal.h"
#include "vbhem_exact.h"
#include "vbhem_stats_dev.h"
#include "vbhem_stats_plan.h"

namespace vbhem {

// ---------------------------------------------------------------------------
// resp_kernel: one wavefront per base (lanes over clusters j).
// ---------------------------------------------------------------------------
#ifndef VBHEM_RESP_UNROLL
#define VBHEM_RESP_UNROLL 1   // base steps of a wave unrolled (build switch for A/B)
#endif

// G = lanes per base (power of two >= K, <= 64): 64/G bases per wavefront step.
// (4 waves per SIMD: two chunk blocks per CU; the folded fallback must not raise it)
#ifndef VBHEM_RESP_WPE
#define VBHEM_RESP_WPE 4
#endif
typedef unsigned int resp_u2 __attribute__((ext_vector_type(2)));

// The gate mask of a base (StatsArgs::gmask, K <= 64) from the ballot of the gate test over
// a wavefront whose lane groups of G lanes hold a base each, a cluster per lane: the G bits
// of group sub, bit j = cluster j.
__device__ __forceinline__ unsigned long long group_bits(unsigned long long ballot, int sub, int G) {
  return G >= 64 ? ballot : (ballot >> (sub * G)) & ((1ull << G) - 1ull);
}

// KP: K when it is a power of two <= 64 (every lane of a base group holds a cluster:
// the group reductions unroll and the stores need no lane mask), else 0
template <int KP>
__global__ __launch_bounds__(kRespThreads) __attribute__((amdgpu_waves_per_eu(VBHEM_RESP_WPE))) void resp_kernel(
    const StatsArgs p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = kRespThreads / 64;
  const int K = KP ? KP : p.K;
  int G = KP ? KP : 1;
  if (!KP)
    while (G < K && G < 64) G <<= 1;
  const int BPW = 64 / G;            // bases per wave step
  const int sub = lane / G, gl = lane - sub * G;
  double *accNj = lds;               // [NW*BPW][K]
  double *accLt = accNj + NW * BPW * K;  // [NW][2]
  int *gcnt = reinterpret_cast<int *>(accLt + 2 * NW);  // [K] gated pairs of this chunk
  int b0, b1;
  chunk_range(p.i_end - p.i_begin, p.i_begin, blockIdx.x, gridDim.x, b0, b1);
  if (p.fold) {
    // the folded fallback (vbhem_internal.h, kFlagHead): the backward pass's flagged
    // pairs of this block's bases get their exact L_elbo (and other outputs) before any
    // of them is read; block 0 records where the gate-list pass's entries will start.
    // The block's scratch slots: xslots / gridDim of them (the host folds only when
    // gridDim <= xslots); the queue borrows the accumulators' LDS before they are set
    int *fc = p.fx.flag_count;
    const int cnt = __atomic_load_n(fc, __ATOMIC_RELAXED);
    if (blockIdx.x == 0 && tid == 0) fc[3] = cnt;
    if (cnt > 0) {  // block-uniform
      const int nw = min(kRespFoldWaves, max(1, p.xslots / (int)gridDim.x));
      int *q = reinterpret_cast<int *>(lds), *qn = q + kRespThreads;
      auto mine = [&](int pair) { const int i = pair / K; return i >= b0 && i < b1; };
      if (exact_wave_in_lds(p.fx.S, p.fx.SB))
        fold_exact<false>(p.fx, 0, cnt, mine, p.xscratch, p.xstride, (int)blockIdx.x * nw, nw, q, qn,
                          lds + fold_lds_bytes(kRespThreads, 0, 1, 1) / sizeof(double));
      else
        fold_exact<true>(p.fx, 0, cnt, mine, p.xscratch, p.xstride, (int)blockIdx.x * nw, nw, q, qn,
                         nullptr);
    }
  }
  for (int x = tid; x < NW * BPW * K + 2 * NW; x += kRespThreads) accNj[x] = 0.0;
  for (int x = tid; x < K; x += kRespThreads) gcnt[x] = 0;
  __syncthreads();
  double l1 = 0.0, l7 = 0.0;
  if constexpr (KP > 0) {
    // K = G: a lane per cluster, 64 / K bases per wave step.  Two bases' loads in
    // flight behind the one being computed (two named buffers, no register copies), and
    // the hat_Z / Z stores are buffer stores whose lanes past the chunk carry an
    // out-of-range offset (dropped by the hardware) instead of a branch: the compiler
    // then waits for a buffer's loads without also waiting for the stores issued after
    // them (a join after branched stores drains every store of the step)
    constexpr int BP = 64 / KP;
    const int stride = NW * BP;
    const double lo = p.logOmega[gl];
    const int nb = b1 - b0;
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
        p.hatZ + (size_t)b0 * KP, (short)0, nb * KP * 8, 0x00020000);
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
        p.Z + (size_t)(b0 - p.i_buf0) * KP, (short)0, nb * KP * 8, 0x00020000);
    // the gate masks: a word per base from lane 0 of its group (no masks: no records,
    // every store dropped)
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
        p.gmask ? p.gmask + (b0 - p.i_buf0) : nullptr, (short)0, p.gmask ? nb * 8 : 0, 0x00020000);
    auto step = [&](int ib, double tnb, double llb) {
#pragma clang fp contract(off)
      const bool iv = ib < b1;
      const double lz = tnb * (lo + llb);  // rounded before the shift (see below)
      double mx = lz;
#pragma unroll
      for (int off = KP >> 1; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
      double sm = exp(lz - mx);
#pragma unroll
      for (int off = KP >> 1; off >= 1; off >>= 1) sm += __shfl_xor(sm, off, 64);
      const double lse = mx + log(sm);
      const double hz = exp(lz - lse) + 1e-50;
      const double Z = hz * tnb;
      const int off = iv ? ((ib - b0) * KP + gl) * 8 : 0x7ffffff0;
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(resp_u2, hz), rh, off, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(resp_u2, Z), rz, off, 0, 0);
      // (no branch in the step: the lanes past the chunk add zeros)
      accNj[(wave * BP + sub) * KP + gl] += iv ? Z : 0.0;
      const bool gt = iv && Z > kGateZ;
      atomicAdd(&gcnt[gl], gt ? 1 : 0);
      const unsigned long long gm = group_bits(__ballot(gt), sub, KP);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(resp_u2, gm), rm,
                                            (iv && gl == 0) ? (ib - b0) * 8 : 0x7ffffff0, 0, 0);
      l1 += iv ? Z * llb : 0.0;
      l7 += iv ? hz * log(hz) : 0.0;
    };
    auto ld = [&](int ib, double &tnb, double &llb) {
      const int ii = ib < b1 ? ib : b0;
      tnb = p.tildeN[ii];
      llb = p.LL[(size_t)ii * KP + gl];
    };
    int i = b0 + wave * BP + sub;
    // (all of a wave's steps loaded up front -- seven at C4 -- measured slower than these
    // two buffers: DESIGN.md 8)
    double tA, lA, tB, lB;
    ld(i, tA, lA);
    for (; i - sub < b1; i += 2 * stride) {
      ld(i + stride, tB, lB);
      step(i, tA, lA);
      ld(i + 2 * stride, tA, lA);
      step(i + stride, tB, lB);  // (past the chunk: every lane adds zeros, stores dropped)
    }
  } else if (K <= G) {
    // one cluster per lane: the next base's tilde_N and L_elbo are loaded while
    // this base's ẑ is computed (a C4 wave walks 6 bases of its chunk in turn)
    const int stride = NW * BPW;
    const double lo = gl < K ? p.logOmega[gl] : 0.0;
    int i = b0 + wave * BPW + sub;
    int ii = i < b1 ? i : b0;
    double tn = p.tildeN[ii];
    double ll = gl < K ? p.LL[(size_t)ii * K + gl] : 0.0;
    // one base step: hat_Z, Z and the sums of base ib (valid when ib < b1)
    auto step = [&](int ib, double tnb, double llb) {
#pragma clang fp contract(off)
      const bool iv = ib < b1;
      const double lz = tnb * (lo + llb);  // rounded before the shift (see below)
      double mx = gl < K ? lz : -INFINITY;
      mx = group_max(mx, G);
      double sm = gl < K ? exp(lz - mx) : 0.0;
      sm = group_sum(sm, G);
      const double lse = mx + log(sm);
      bool gt = false;
      if (iv && gl < K) {
        const double hz = exp(lz - lse) + 1e-50;
        const double Z = hz * tnb;
        p.hatZ[(size_t)ib * K + gl] = hz;
        p.Z[(size_t)(ib - p.i_buf0) * K + gl] = Z;
        accNj[(wave * BPW + sub) * K + gl] += Z;
        gt = Z > kGateZ;
        if (gt) atomicAdd(&gcnt[gl], 1);
        l1 += Z * llb;
        l7 += hz * log(hz);
      }
      if (p.gmask) {  // (uniform; the step runs on every lane of the wave)
        const unsigned long long gm = group_bits(__ballot(gt), sub, G);
        if (iv && gl == 0) p.gmask[ib - p.i_buf0] = gm;
      }
    };
#if VBHEM_RESP_UNROLL == 2
    // two base steps per iteration: their chains (group max, exp, group sum, log)
    // interleave; the sums still take base i before base i + stride
    for (; i - sub < b1; i += 2 * stride) {
      const int i2 = i + stride, i2c = i2 < b1 ? i2 : b0;
      const int in = i + 2 * stride < b1 ? i + 2 * stride : b0;
      const double tn2 = p.tildeN[i2c];
      const double ll2 = gl < K ? p.LL[(size_t)i2c * K + gl] : 0.0;
      const double tn_n = p.tildeN[in];
      const double ll_n = gl < K ? p.LL[(size_t)in * K + gl] : 0.0;
      step(i, tn, ll);
      step(i2, tn2, ll2);
      tn = tn_n;
      ll = ll_n;
    }
#else
    for (; i - sub < b1; i += stride) {
      const int in = i + stride < b1 ? i + stride : b0;
      const double tn_n = p.tildeN[in];
      const double ll_n = gl < K ? p.LL[(size_t)in * K + gl] : 0.0;
      step(i, tn, ll);
      tn = tn_n;
      ll = ll_n;
    }
#endif
  } else
  for (int i = b0 + wave * BPW + sub; i - sub < b1; i += NW * BPW) {
    // log_Z = tilde_N .* (logOmega + L_elbo) is rounded before the shift, as in
    // step_fc.m:275-276 (an fma-contracted shift would let the winning entry
    // exceed 1 by ~ulp(log_Z)).
#pragma clang fp contract(off)
    const bool iv = i < b1;
    const int ii = iv ? i : b0;
    const double tn = p.tildeN[ii];
    const double *LL = p.LL + (size_t)ii * K;
    double mx = -INFINITY;
    for (int j = gl; j < K; j += G) mx = fmax(mx, tn * (p.logOmega[j] + LL[j]));
    mx = group_max(mx, G);
    double sm = 0.0;
    for (int j = gl; j < K; j += G) sm += exp(tn * (p.logOmega[j] + LL[j]) - mx);
    sm = group_sum(sm, G);
    const double lse = mx + log(sm);
    if (iv) {
      for (int j = gl; j < K; j += G) {
        const double ll = LL[j];
        const double hz = exp(tn * (p.logOmega[j] + ll) - lse) + 1e-50;
        const double Z = hz * tn;
        p.hatZ[(size_t)i * K + j] = hz;
        p.Z[(size_t)(i - p.i_buf0) * K + j] = Z;
        accNj[(wave * BPW + sub) * K + j] += Z;
        if (Z > kGateZ) atomicAdd(&gcnt[j], 1);
        l1 += Z * ll;
        l7 += hz * log(hz);
      }
    }
  }
  l1 = wave_sum(l1);
  l7 = wave_sum(l7);
  if (lane == 0) {
    accLt[2 * wave] = l1;
    accLt[2 * wave + 1] = l7;
  }
  __syncthreads();
  double *slab = p.slabs + (size_t)blockIdx.x * p.slab_len;
  for (int j = tid; j < K; j += kRespThreads) {
    double s = 0.0;
    for (int w = 0; w < NW * BPW; ++w) s += accNj[w * K + j];
    slab[j] = p.assign ? s : slab[j] + s;
  }
  if (tid < 2) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += accLt[2 * w + tid];
    double &dst = slab[(size_t)K + (size_t)K * p.S + (size_t)K * p.S * p.S + tid];
    dst = p.assign ? s : dst + s;
  }
  if (p.gate_cnt)
    for (int j = tid; j < K; j += kRespThreads) p.gate_cnt[(size_t)blockIdx.x * K + j] = gcnt[j];
}

// ---------------------------------------------------------------------------
// resp_trials_kernel: resp_kernel for R = K / KT independent EM trials batched
// as one cluster set (trial r = clusters [r KT, (r+1) KT)).  hat_Z(i, .) is
// normalised within each trial (step_fc.m:275-281 per trial); Nj, Lt1, Lt7 go
// to trial r's section [r SL, (r+1) SL) of the slab.  K <= 256: a lane holds
// the clusters gl + s G, s < kRespSlots; per-trial sums are masked lane sums in
// a fixed order (deterministic).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(kRespThreads) void resp_trials_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = kRespThreads / 64;
  const int K = p.K, KT = p.KT, R = K / KT, SL = p.SL, S = p.S;
  int G = 1;
  while (G < K && G < 64) G <<= 1;
  const int BPW = 64 / G;
  const int sub = lane / G, gl = lane - sub * G;
  double *accNj = lds;                        // [NW*BPW][K]
  double *accLt = accNj + NW * BPW * K;       // [NW][R][2]
  int *gcnt = reinterpret_cast<int *>(accLt + 2 * NW * R);  // [K]
  for (int x = tid; x < NW * BPW * K + 2 * NW * R; x += kRespThreads) accNj[x] = 0.0;
  for (int x = tid; x < K; x += kRespThreads) gcnt[x] = 0;
  __syncthreads();
  int tr[kRespSlots];  // trial of this lane's slot s (-1: no cluster)
#pragma unroll
  for (int s = 0; s < kRespSlots; ++s) {
    const int j = gl + s * G;
    tr[s] = j < K ? j / KT : -1;
  }
  int b0, b1;
  chunk_range(p.i_end - p.i_begin, p.i_begin, blockIdx.x, gridDim.x, b0, b1);
  double l1[kRespSlots], l7[kRespSlots];
#pragma unroll
  for (int s = 0; s < kRespSlots; ++s) l1[s] = l7[s] = 0.0;
  for (int i = b0 + wave * BPW + sub; i - sub < b1; i += NW * BPW) {
#pragma clang fp contract(off)
    const bool iv = i < b1;
    const int ii = iv ? i : b0;
    const double tn = p.tildeN[ii];
    const double *LL = p.LL + (size_t)ii * K;
    double lz[kRespSlots], lse[kRespSlots];
#pragma unroll
    for (int s = 0; s < kRespSlots; ++s) {
      const int j = tr[s] >= 0 ? gl + s * G : 0;
      lz[s] = tr[s] >= 0 ? tn * (p.logOmega[j] + LL[j]) : -INFINITY;
      lse[s] = 0.0;
    }
    for (int r = 0; r < R; ++r) {
      double mx = -INFINITY;
#pragma unroll
      for (int s = 0; s < kRespSlots; ++s) mx = tr[s] == r ? fmax(mx, lz[s]) : mx;
      mx = group_max(mx, G);
      double sm = 0.0;
#pragma unroll
      for (int s = 0; s < kRespSlots; ++s) sm += tr[s] == r ? exp(lz[s] - mx) : 0.0;
      sm = group_sum(sm, G);
      const double l = mx + log(sm);
#pragma unroll
      for (int s = 0; s < kRespSlots; ++s) lse[s] = tr[s] == r ? l : lse[s];
    }
    bool gt0 = false;  // slot 0's gate test (K <= 64: the only slot with clusters)
    if (iv) {
#pragma unroll
      for (int s = 0; s < kRespSlots; ++s) {
        if (tr[s] < 0) continue;
        const int j = gl + s * G;
        const double hz = exp(lz[s] - lse[s]) + 1e-50;
        const double Z = hz * tn;
        p.hatZ[(size_t)i * K + j] = hz;
        p.Z[(size_t)(i - p.i_buf0) * K + j] = Z;
        accNj[(wave * BPW + sub) * K + j] += Z;
        const bool gt = Z > kGateZ;
        if (gt) atomicAdd(&gcnt[j], 1);
        if (s == 0) gt0 = gt;
        l1[s] += Z * LL[j];
        l7[s] += hz * log(hz);
      }
    }
    if (p.gmask) {  // (uniform, K <= 64; the loop's trip count is the wave's)
      const unsigned long long gm = group_bits(__ballot(gt0), sub, G);
      if (iv && gl == 0) p.gmask[i - p.i_buf0] = gm;
    }
  }
  for (int r = 0; r < R; ++r) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int s = 0; s < kRespSlots; ++s) {
      a += tr[s] == r ? l1[s] : 0.0;
      b += tr[s] == r ? l7[s] : 0.0;
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
      accLt[(wave * R + r) * 2] = a;
      accLt[(wave * R + r) * 2 + 1] = b;
    }
  }
  __syncthreads();
  double *slab = p.slabs + (size_t)blockIdx.x * p.slab_len;
  for (int j = tid; j < K; j += kRespThreads) {
    double s = 0.0;
    for (int w = 0; w < NW * BPW; ++w) s += accNj[w * K + j];
    const int r = j / KT;
    double &dst = slab[(size_t)r * SL + (j - r * KT)];
    dst = p.assign ? s : dst + s;
  }
  for (int x = tid; x < 2 * R; x += kRespThreads) {
    const int r = x >> 1, q = x & 1;
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += accLt[(w * R + r) * 2 + q];
    double &dst = slab[(size_t)r * SL + KT + (size_t)KT * S + (size_t)KT * S * S + q];
    dst = p.assign ? s : dst + s;
  }
  if (p.gate_cnt)
    for (int j = tid; j < K; j += kRespThreads) p.gate_cnt[(size_t)blockIdx.x * K + j] = gcnt[j];
}

// ---------------------------------------------------------------------------
// vhem_resp_kernel: the VHEM responsibilities (hem_h3m_c_step.m:293-314) of R = K / KT
// independent EM trials (R = 1: one cluster set), per base i and trial r:
//   Ls = L_elbo(i, j) / inf_norm,  lz = log omega_j + N_i Ls   (each rounded as written)
//   mx = max_j lz, sm = sum_j exp(lz - mx), lse = mx + log(sm),
//   Z = exp(lz - mx) / sm = exp(lz - lse)  (no 1e-50; log omega = -inf gives exactly 0.
//   The quotient form keeps every row's sum within a few ulp of 1 whatever |lz| is;
//   exp(lz - lse) carries ulp(lse) -- 1e-13 at |lz| ~ 1e3 -- into every entry.)
//   w = Z omega_b(i)  -> the weight buffer StatsArgs::Z,  Z -> StatsArgs::hatZ
// and the per-chunk partial sums Nj = sum_i Z (:430), LogL = sum_i lse (:308) and the
// counts of pairs with w > 0.  A wavefront owns the bases b0 + wave, b0 + wave + NW, ...
// of its chunk, in ascending order; its 64 / G groups of G lanes (G the power of two
// >= KT, <= 64) take the trials r = sub, sub + 64 / G, ... of that base, a lane the
// clusters gl, gl + G, ... of the trial (KT = G: a cluster per lane; KT < G: the lanes
// past KT masked; KT > 64: the loop).  Every (trial, cluster) sum is therefore the sum
// over a wavefront's bases in ascending order, then over the wavefronts in order: the
// same bits whatever R is (a trial batched with others equals the trial alone), no
// atomics on doubles.  The folded exact fallback as in resp_kernel.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kRespThreads) void vhem_resp_kernel(const StatsArgs p) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = kRespThreads / 64;
  const int K = p.K, KT = p.KT, R = K / KT, SL = p.SL, S = p.S;
  int G = 1;
  while (G < KT && G < 64) G <<= 1;
  const int TPS = 64 / G;  // trials per wave step
  const int sub = lane / G, gl = lane - sub * G;
  double *accNj = lds;                 // [NW][K]
  double *accL = accNj + NW * K;       // [NW][R]
  int *gcnt = reinterpret_cast<int *>(accL + NW * R);  // [K]
  int b0, b1;
  chunk_range(p.i_end - p.i_begin, p.i_begin, blockIdx.x, gridDim.x, b0, b1);
  if (p.fold) {  // (see resp_kernel)
    int *fc = p.fx.flag_count;
    const int cnt = __atomic_load_n(fc, __ATOMIC_RELAXED);
    if (blockIdx.x == 0 && tid == 0) fc[3] = cnt;
    if (cnt > 0) {  // block-uniform
      const int nw = min(kRespFoldWaves, max(1, p.xslots / (int)gridDim.x));
      int *q = reinterpret_cast<int *>(lds), *qn = q + kRespThreads;
      auto mine = [&](int pair) { const int i = pair / K; return i >= b0 && i < b1; };
      if (exact_wave_in_lds(p.fx.S, p.fx.SB))
        fold_exact<false>(p.fx, 0, cnt, mine, p.xscratch, p.xstride, (int)blockIdx.x * nw, nw, q, qn,
                          lds + fold_lds_bytes(kRespThreads, 0, 1, 1) / sizeof(double));
      else
        fold_exact<true>(p.fx, 0, cnt, mine, p.xscratch, p.xstride, (int)blockIdx.x * nw, nw, q, qn,
                         nullptr);
    }
  }
  for (int x = tid; x < NW * K + NW * R; x += kRespThreads) accNj[x] = 0.0;
  for (int x = tid; x < K; x += kRespThreads) gcnt[x] = 0;
  __syncthreads();
  const double inf_norm = p.inf_norm;
  for (int i = b0 + wave; i < b1; i += NW) {  // wave-uniform
#pragma clang fp contract(off)
    const double ni = p.tildeN[i], ob = p.omegaB[i];
    const double *LL = p.LL + (size_t)i * K;
    unsigned long long gm = 0ull;  // this lane's clusters of base i that pass the gate
    for (int r0 = 0; r0 < R; r0 += TPS) {  // wave-uniform
      const int r = r0 + sub;
      const bool rv = r < R;
      const int jb = (rv ? r : 0) * KT;
      double mx = -INFINITY;
      for (int j = gl; j < KT; j += G)
        mx = fmax(mx, p.logOmega[jb + j] + ni * (LL[jb + j] / inf_norm));
      mx = group_max(mx, G);
      double sm = 0.0;
      for (int j = gl; j < KT; j += G)
        sm += exp((p.logOmega[jb + j] + ni * (LL[jb + j] / inf_norm)) - mx);
      sm = group_sum(sm, G);
      const double lse = mx + log(sm);
      if (rv) {
        for (int j = gl; j < KT; j += G) {
          const double lz = p.logOmega[jb + j] + ni * (LL[jb + j] / inf_norm);
          const double Z = exp(lz - mx) / sm;
          const double w = Z * ob;
          p.hatZ[(size_t)i * K + jb + j] = Z;
          p.Z[(size_t)(i - p.i_buf0) * K + jb + j] = w;
          accNj[wave * K + jb + j] += Z;
          const bool gt = w > Gate<kGateVhem>::value;
          if (gt) atomicAdd(&gcnt[jb + j], 1);
          if (gt && p.gmask) gm |= 1ull << (jb + j);  // (masks: K <= 64)
        }
        if (gl == 0) accL[wave * R + r] += lse;
      }
    }
    if (p.gmask) {  // (uniform) the lanes' bits into the base's word
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) gm |= __shfl_xor(gm, off, 64);
      if (lane == 0) p.gmask[i - p.i_buf0] = gm;
    }
  }
  __syncthreads();
  double *slab = p.slabs + (size_t)blockIdx.x * p.slab_len;
  for (int j = tid; j < K; j += kRespThreads) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += accNj[w * K + j];
    const int r = j / KT;
    double &dst = slab[(size_t)r * SL + (j - r * KT)];
    dst = p.assign ? s : dst + s;
  }
  for (int x = tid; x < 2 * R; x += kRespThreads) {
    const int r = x >> 1, q = x & 1;
    double s = 0.0;
    if (q == 0)
      for (int w = 0; w < NW; ++w) s += accL[w * R + r];
    double &dst = slab[(size_t)r * SL + KT + (size_t)KT * S + (size_t)KT * S * S + q];
    dst = p.assign ? s : dst + s;
  }
  if (p.gate_cnt)
    for (int j = tid; j < K; j += kRespThreads) p.gate_cnt[(size_t)blockIdx.x * K + j] = gcnt[j];
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
hipError_t launch_resp(const StatsArgs &a, const RespPlan &rp, int nchunk, hipStream_t st) {
  StatsKernel fn = nullptr;
  switch (rp.kernel) {
    case RespKernel::kVhem: fn = vhem_resp_kernel; break;
    case RespKernel::kTrials: fn = resp_trials_kernel; break;
    case RespKernel::kGeneric:
    case RespKernel::kKP:
      fn = pick_kernel<0, 4, 8, 16, 32, 64>(rp.KP, [](auto kp) { return resp_kernel<decltype(kp)::value>; });
  }
  if (!rp.ok || !fn || (a.vhem && !a.omegaB)) return hipErrorInvalidValue;
  hipError_t e = set_dyn_lds(reinterpret_cast<const void *>(fn), rp.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(nchunk), dim3(kRespThreads), rp.lds, st, a);
  return hipGetLastError();
}

}  // namespace vbhem
