// vbhem_stats_dev.h -- device helpers shared by the fused E-step epilogue's kernel files
// (vbhem_resp.hip, vbhem_stats_dense.hip, vbhem_stats_gated.hip, vbhem_stats_mfma.hip):
// wave and lane-group reductions, the exact small division, a chunk's base range, the
// statistics' gate and the prepared-operand kernels' output phase.
#pragma once
#include <hip/hip_runtime.h>

#include "vbhem_internal.h"
#include "vbhem_stats_plan.h"

namespace vbhem {

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// x / D for 0 <= x < 2^22 and small D, via a float reciprocal (exact: the
// +0.5 offset keeps the quotient 0.5/D away from an integer).
__device__ __forceinline__ int qdiv(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }

__device__ __forceinline__ void chunk_range(int nb, int i_begin, int chunk, int nchunk, int &b0,
                                            int &b1) {
  const int per = (nb + nchunk - 1) / nchunk;
  b0 = i_begin + chunk * per;
  b1 = min(i_begin + nb, b0 + per);
}

__device__ __forceinline__ double group_max(double v, int G) {
  for (int off = G >> 1; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double group_sum(double v, int G) {
  for (int off = G >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

constexpr double kGateZ = 1e-8;  // vbhem_compute_Statistics.m:35  (Z_Ni(i) > 1e-8)
// The gate of the statistic sums is a compile-time parameter of the kernels that apply
// it to the weight buffer StatsArgs::Z (gate_list_kernel, stats_kernel, nm_kernel; the
// stats_list_* kernels read the lists and the weights only):
//   kGateVbhem  weight = Z = hat_Z tilde_N, gate Z > 1e-8
//   kGateVhem   weight = w = Z omega_b,     gate w > 0   (hem_mstep_component.m:88)
constexpr int kGateVbhem = 0, kGateVhem = 1;
template <int GM>
struct Gate {
  static constexpr double value = GM == kGateVhem ? 0.0 : kGateZ;
};

// entry o of a block's reduced sums red ([S][NU] | [S] | [S][S]) of cluster jt of its
// trial: the value shifted back by z, and its place in the trial's section of a slab
// (or of the packed statistics: the same layout)
__device__ __forceinline__ double su_entry(const StatsArgs &p, const double *red, const double *zs,
                                           int o, int jt, size_t &at) {
  const int S = p.S, NU = p.NU, d = p.d, KT = p.KT;
  const bool full = p.covmode == kCovFull;
  double v;
  if (o < S * NU) {
    const int s2 = o / NU, f = o - s2 * NU;
    const double *rs = red + (size_t)s2 * NU;
    const double N = rs[0];
    if (f == 0) {
      v = N;
    } else if (f <= d) {
      v = fma(zs[f - 1], N, rs[f]);
    } else {
      int a = f - 1 - d, b = a;
      if (full) {
        int k = a;
        a = 0;
        while (k >= d - a) { k -= d - a; ++a; }
        b = a + k;
      }
      const double q2 = (full && a != b) ? 0.5 * rs[f] : rs[f];
      v = q2 + (zs[a] * rs[1 + b] + zs[b] * rs[1 + a]) + zs[a] * zs[b] * N;
    }
    at = (size_t)KT + (size_t)KT * S + (size_t)KT * S * S + 2 + (size_t)jt * S * NU + o;
  } else if (o < S * NU + S) {
    v = red[o];
    at = (size_t)KT + (size_t)jt * S + (o - S * NU);
  } else {
    v = red[o];
    at = (size_t)KT + (size_t)KT * S + (size_t)jt * S * S + (o - S * NU - S);
  }
  return v;
}
// the state (row of red) that entry o belongs to: its moments, N1 entry and M row
__device__ __forceinline__ int su_row(const StatsArgs &p, int o) {
  const int S = p.S, NU = p.NU;
  return o < S * NU ? o / NU : o < S * NU + S ? o - S * NU : (o - S * NU - S) / S;
}

// the prepared-operand statistics' output phase: the block's reduced sums in red
// ([S][NU] | [S] | [S][S]) shifted back by z and written (or added) to slab c
// (row >= 0: the entries of that state alone -- its moments, N1 entry and M row)
__device__ __forceinline__ void su_output(const StatsArgs &p, const double *red, const double *zs,
                                          int c, int nch, int j, int tid, int row = -1) {
  const int S = p.S, NU = p.NU;
  const int KT = p.KT, tr = j / KT, jt = j - tr * KT;
  double *tsl = p.slabs + (size_t)c * p.slab_len + (size_t)tr * p.SL;
  const int NO = S * NU + S + S * S;
  for (int o = tid; o < NO; o += 64 * kSuWaves) {
    if (row >= 0 && su_row(p, o) != row) continue;
    size_t at;
    const double v = su_entry(p, red, zs, o, jt, at);
    double *dst = tsl + at;
    *dst = p.assign ? v : *dst + v;
    if (p.assign)  // the slabs past this grid's chunks hold nothing of cluster j
      for (int cz = c + nch; cz < p.nzero; cz += nch) dst[(size_t)(cz - c) * p.slab_len] = 0.0;
  }
}

// The reduction of the accumulating gate-list pass's partials (vbhem_list4_slots.h; U
// [S][NUP] | N1 [S] | M [S][S] per slot) for state s2 of cluster j, by a block of
// kL4rThreads threads: the row's NU moments, its N1 entry and its M row -- at most
// kL4rCols columns -- summed over the cluster's slots.  16 thread groups take a sixteenth
// of the slots each, in slot order, eight loads in flight, and the sixteen sums are added
// in group order (fixed: bit-reproducible).  Leaves the row in red ([S][NU] | [S] | [S][S],
// the other rows untouched) and the shift z in red + NO; a cluster with an empty list gets
// zeros.  Shared by list4_stats_reduce_kernel and the folded finish (stats_final_fold_kernel).
__device__ __forceinline__ void list4_reduce_row(const StatsArgs &p, const double *parts, int nw,
                                                 int j, int s2, int tid, double *red, int *plan,
                                                 double (*part)[kL4rCols]) {
  const int S = p.S, NU = p.NU, NUP = us_nup(NU), d = p.d;
  if (tid == 0) {
    int nitem = 0, pre = 0;
    for (int x = 0; x < p.K; ++x) {
      if (x == j) pre = nitem;
      nitem += l4s_items(p.list_tot[x]);
    }
    const int per = l4s_per_wave(nitem, nw), n = l4s_items(p.list_tot[j]);
    plan[0] = l4s_slot(pre, j, per);
    plan[1] = n ? l4s_slot(pre + n - 1, j, per) - plan[0] + 1 : 0;
  }
  __syncthreads();
  const int s0 = plan[0], ns = plan[1];
  const int NO = S * NU + S + S * S, PL = l4s_part_len(S, NUP);
  double *zs = red + NO;                              // [d]
  for (int a = tid; a < d; a += kL4rThreads) zs[a] = p.uz[a];
  // column col of the row: a moment, the N1 entry, an M entry -- in a partial, in red
  const int q = tid / kL4rCols, col = tid - q * kL4rCols;
  const bool cv = col < NU + 1 + S;
  const int src = col < NU ? s2 * NUP + col : col == NU ? S * NUP + s2 : S * NUP + S + s2 * S + (col - NU - 1);
  const int dst = col < NU ? s2 * NU + col : col == NU ? S * NU + s2 : S * NU + S + s2 * S + (col - NU - 1);
  const int k0 = (int)((long long)ns * q / kL4rParts), k1 = (int)((long long)ns * (q + 1) / kL4rParts);
  double acc = 0.0;
  if (cv) {
    const double *g = parts + (size_t)s0 * PL + src;
    int k = k0;
    for (; k + 7 < k1; k += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = g[(size_t)(k + u) * PL];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; k < k1; ++k) acc += g[(size_t)k * PL];
  }
  part[q][col] = acc;
  __syncthreads();
  if (q == 0 && cv) {
    double t = part[0][col];
#pragma unroll
    for (int x = 1; x < kL4rParts; ++x) t += part[x][col];
    red[dst] = t;
  }
  __syncthreads();
}

// ---- the call's finishing kernels (stats_final_kernel, stats_final_fold_kernel) ----
constexpr int kFinalCols = 16, kFinalParts = 16;

// The call's last kernel closes the flag head (kFlagPre): the total kept, the counters
// zeroed, the tag written -- the next call's in-kernel preparation finds them clean.
// With a completion word, counter [2] (fb_exact_kernel's blocks-done, zero between
// passes) counts this kernel's finished blocks instead: the last one resets it
__device__ __forceinline__ void final_close_head(int *fpre, unsigned long long tag, bool done) {
  int *fc = fpre + kFlagPre;
  fpre[2] = fc[1];
  for (int c = 0; c < kFlagHead; ++c)
    if (!(done && c == 2)) fc[c] = 0;
  *reinterpret_cast<unsigned long long *>(fpre) = tag;
}
// partition pp's sum of column x over the slabs pp, pp + 16, ... below nslab (128-B rows,
// four loads in flight per thread)
__device__ __forceinline__ double final_partial(const double *slabs, int nslab, int slab_len, int x,
                                                int pp) {
  double acc = 0.0;
  int k = pp;
  for (; k + 3 * kFinalParts < nslab; k += 4 * kFinalParts) {
    const double *q = slabs + (size_t)k * slab_len + x;
    const double v0 = q[0], v1 = q[(size_t)kFinalParts * slab_len],
                 v2 = q[(size_t)2 * kFinalParts * slab_len], v3 = q[(size_t)3 * kFinalParts * slab_len];
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; k < nslab; k += kFinalParts) acc += slabs[(size_t)k * slab_len + x];
  return acc;
}
// one entry of the packed statistics
__device__ __forceinline__ void final_store(double *dst, double s, const int *fpre, bool done) {
  // a lost flag-head handshake (kFlagLost, fb_bwd2_kernel): results untrusted
  if (fpre && __hip_atomic_load(fpre + kFlagLost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                  kFlagLostMark)
    s = __builtin_nan("");
  if (done)  // written through to the system (the host polls the word, not an event)
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(dst), __double_as_longlong(s),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else
    *dst = s;
}
// the completion word (every thread of the block, after its stores): every store of this
// block acknowledged (written through at system scope: what a system-scope release would
// wait for, without its L2 write-back), then one count per block; the last block to count
// publishes the word after all of them
__device__ __forceinline__ void final_publish(int *fpre, unsigned long long *done,
                                              unsigned long long done_val) {
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  if (threadIdx.x == 0) {
    int *cnt = fpre + kFlagPre + 2;
    const int prev = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == (int)gridDim.x - 1) {
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, done_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace vbhem
