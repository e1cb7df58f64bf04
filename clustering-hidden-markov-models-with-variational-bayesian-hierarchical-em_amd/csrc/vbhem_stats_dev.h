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

// the prepared-operand statistics' output phase: the block's reduced sums in red
// ([S][NU] | [S] | [S][S]) shifted back by z and written (or added) to slab c
// (row >= 0: the entries of that state alone -- its moments, N1 entry and M row)
__device__ __forceinline__ void su_output(const StatsArgs &p, const double *red, const double *zs,
                                          int c, int nch, int j, int tid, int row = -1) {
  const int S = p.S, NU = p.NU, d = p.d;
  const bool full = p.covmode == kCovFull;
  const int KT = p.KT, tr = j / KT, jt = j - tr * KT;
  double *tsl = p.slabs + (size_t)c * p.slab_len + (size_t)tr * p.SL;
  const int NO = S * NU + S + S * S;
  for (int o = tid; o < NO; o += 64 * kSuWaves) {
    double v;
    double *dst;
    if (row >= 0 && (o < S * NU ? o / NU : o < S * NU + S ? o - S * NU : (o - S * NU - S) / S) != row) continue;
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
      dst = tsl + KT + (size_t)KT * S + (size_t)KT * S * S + 2 + (size_t)jt * S * NU + o;
    } else if (o < S * NU + S) {
      v = red[o];
      dst = tsl + KT + (size_t)jt * S + (o - S * NU);
    } else {
      v = red[o];
      dst = tsl + KT + (size_t)KT * S + (size_t)jt * S * S + (o - S * NU - S);
    }
    *dst = p.assign ? v : *dst + v;
    if (p.assign)  // the slabs past this grid's chunks hold nothing of cluster j
      for (int cz = c + nch; cz < p.nzero; cz += nch) dst[(size_t)(cz - c) * p.slab_len] = 0.0;
  }
}

}  // namespace vbhem
