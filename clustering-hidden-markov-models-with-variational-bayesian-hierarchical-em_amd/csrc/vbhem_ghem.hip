// vbhem_ghem.hip -- the batched hierarchical EM of the 'gmmNew' initialisation
// (include/vbhem_init.h).  The arithmetic is vbhem_ghem_run.h, shared with the host check
// build.  Plain fp64.
//
// Per call: ghem_scan_kernel / ghem_scan_finish (the start covariance and the finiteness of
// the points, the same for every trial).  Per chunk of trials: ghem_seed_kernel<DB>, one
// workgroup per trial (kmeans_pp by wtkrun::block_kmeans_pp, the start values, `prepare`);
// then per round four launches and no host read:
//   ghem_estep_kernel    grid (point tile, group of kGroup trials): a thread per point; the
//                        block loops over its group's trials with the same tile, so a
//                        tile's x and cov come from memory once and from cache after that;
//                        posteriors to the workspace, the tile's sums to partA
//   ghem_finish1_kernel  one workgroup per trial: partA in tile order, the stopping rule,
//                        mxwt and the new centres
//   ghem_cov_kernel      the same grid: a thread per covariance entry of a trial walks the
//                        tile's points in order (kAcc entries per thread and walk)
//   ghem_finish2_kernel  one workgroup per trial: partB in tile order, the division, then
//                        `prepare`: a wave per component (its first lane factorises in LDS)
// A finished trial sets its done flag in its slot; every later launch skips it.  A trial
// works in its workspace slot and writes its outputs when it ends OK, its status otherwise.
// No atomics, no block waits on another; every loop is bounded by n, T, d, the tile count,
// the group size or the iteration limits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_init.h"
#include "vbhem_internal.h"
#include "vbhem_ghem_run.h"

namespace vbhem {
namespace {

using namespace ghemrun;
using wtkrun::wave_sum;

constexpr int kEaMax = ea_len(kMaxT, kMaxDim);
constexpr int kHead = 256 + 8;  // vr0 [cd <= 256], then the call's bad flag

struct Args {
  int n, d, T, cd, nt, P, full, iterations, it, R0, cnt, ustride, EA, EB;
  double vs;
  const double *x, *c, *u, *init;
  const int *j0;
  double *mxwt, *centres, *covars, *logpost, *logp;
  int *status, *iters;
  double *head, *scanp, *trials;
  int *scanbad;
  size_t TS, SL;
};

__device__ inline Slot slot_of(const Args &p, int rl) { return slot_at(p.trials + (size_t)rl * p.TS, p.T, p.d, p.cd); }
__device__ inline double *part_a(const Args &p, int rl) { return p.trials + (size_t)rl * p.TS + p.SL; }
__device__ inline double *part_b(const Args &p, int rl) { return part_a(p, rl) + (size_t)p.nt * p.EA; }
__device__ inline double *post_of(const Args &p, int rl) { return part_b(p, rl) + (size_t)p.nt * p.EB; }

// The end of a trial (after a barrier behind the writes of its flags): the outputs of an OK
// trial, the status of any.
__device__ inline void emit(const Args &p, int rl, const Slot &s) {
  const int tid = threadIdx.x, r = p.R0 + rl, st = s.flag[fStatus];
  if (st == kOk) {
    for (int e = tid; e < p.T; e += kBlock) p.mxwt[(size_t)r * p.T + e] = s.mx[e];
    for (int e = tid; e < p.T * p.d; e += kBlock) p.centres[(size_t)r * p.T * p.d + e] = s.cen[e];
    for (int e = tid; e < p.EB; e += kBlock) p.covars[(size_t)r * p.EB + e] = s.vr[e];
  }
  if (tid == 0) {
    if (st == kOk) {
      p.logp[r] = s.sc[1];
      p.iters[2 * r] = s.flag[fLloyd];
      p.iters[2 * r + 1] = s.flag[fEsteps];
    }
    p.status[r] = st;
  }
}

// `prepare` of every component: wave w takes components w, w + kWaves, ...; its first lane
// factorises in the wave's LDS scratch.  True on a failed pivot.
__device__ inline bool block_prepare(const Args &p, const Slot &s, double (*fac)[2][kMaxDim * kMaxDim], int *sing) {
  const int tid = threadIdx.x, w = tid >> 6;
  if (tid == 0) *sing = 0;
  __syncthreads();
  if ((tid & 63) == 0) {
    int f = 0;
    for (int t = w; t < p.T; t += kWaves) f |= prepare_component(s, t, p.d, p.full != 0, fac[w][0], fac[w][1]);
    if (f) *sing = 1;
  }
  __syncthreads();
  return *sing != 0;
}

__device__ inline void end_trial(const Args &p, int rl, const Slot &s, int status) {
  if (threadIdx.x == 0) {
    s.flag[fStatus] = status;
    s.flag[fDone] = 1;
  }
  __syncthreads();
  emit(p, rl, s);
}

__global__ __launch_bounds__(kBlock) void ghem_scan_kernel(const Args p) {
  const int tid = threadIdx.x, tile = blockIdx.x, n = p.n, d = p.d, cd = p.cd;
  const int p0 = tile * p.P, p1 = p0 + p.P < n ? p0 + p.P : n;
  if (tid < cd) {
    double v = p.full ? 0.0 : -INFINITY;
    for (int pt = p0; pt < p1; ++pt) {
      const double c = p.c[(size_t)pt * cd + tid];
      v = p.full ? v + c : (c > v ? c : v);
    }
    p.scanp[(size_t)tile * cd + tid] = v;
  }
  int bad = 0;
  for (size_t e = (size_t)p0 * d + tid; e < (size_t)p1 * d; e += kBlock) bad |= !finite_d(p.x[e]);
  for (size_t e = (size_t)p0 * cd + tid; e < (size_t)p1 * cd; e += kBlock) bad |= !finite_d(p.c[e]);
  bad = __syncthreads_or(bad);
  if (tid == 0) p.scanbad[tile] = bad;
}

__global__ __launch_bounds__(kBlock) void ghem_scan_finish(const Args p) {
  const int tid = threadIdx.x, cd = p.cd;
  if (tid < cd) {
    double v = p.full ? 0.0 : -INFINITY;
    for (int tile = 0; tile < p.nt; ++tile) {
      const double c = p.scanp[(size_t)tile * cd + tid];
      v = p.full ? v + c : (c > v ? c : v);
    }
    p.head[tid] = p.full ? v / p.n : v;
  }
  int bad = 0;
  for (int tile = tid; tile < p.nt; tile += kBlock) bad |= p.scanbad[tile];
  bad = __syncthreads_or(bad);
  if (tid == 0) *reinterpret_cast<int *>(p.head + 256) = bad;
}

template <int DB>
__global__ __launch_bounds__(kBlock) void ghem_seed_kernel(const Args p) {
  __shared__ wtkrun::Block<DB> b;
  __shared__ double fac[kWaves][2][kMaxDim * kMaxDim];
  __shared__ int sing;
  const int tid = threadIdx.x, rl = blockIdx.x, r = p.R0 + rl, n = p.n, d = p.d, T = p.T;
  const Slot s = slot_of(p, rl);
  const int bad = *reinterpret_cast<const int *>(p.head + 256);
  const int j0 = p.init ? 0 : p.j0[r];
  if (bad || j0 < 0 || j0 >= n) {
    end_trial(p, rl, s, kBad);
    return;
  }
  int lloyd = 0;
  if (p.init) {
    for (int e = tid; e < T * d; e += kBlock) s.cen[e] = p.init[(size_t)r * T * d + e];
  } else {
    double *dmin = post_of(p, rl);  // the posteriors' room: T n doubles, T >= 2
    int *lab = reinterpret_cast<int *>(dmin + n);
    const wtkrun::PPResult pp = wtkrun::block_kmeans_pp(b, p.x, d, nullptr, n, T, j0, p.u + (size_t)r * p.ustride,
                                                        wtkrun::kLloydMax, dmin, lab);
    if (pp.status != wtkrun::kOk) {
      end_trial(p, rl, s, pp.status);
      return;
    }
    for (int e = tid; e < T * d; e += kBlock) s.cen[e] = b.cen[e];
    lloyd = pp.iters;
  }
  for (int e = tid; e < p.EB; e += kBlock) s.vr[e] = p.head[e % p.cd];
  for (int t = tid; t < T; t += kBlock) s.mx[t] = 1.0 / T;
  if (tid == 0) {
    s.sc[0] = -1.7976931348623157e308;
    s.sc[1] = 0.0;
    s.flag[fDone] = 0;
    s.flag[fStatus] = kOk;
    s.flag[fEsteps] = 0;
    s.flag[fLloyd] = lloyd;
  }
  __syncthreads();
  if (p.iterations < 1) {
    end_trial(p, rl, s, kOk);
    return;
  }
  if (block_prepare(p, s, fac, &sing)) end_trial(p, rl, s, kSingular);
}

__global__ __launch_bounds__(kBlock) void ghem_estep_kernel(const Args p) {
  __shared__ double wred[kWaves][kEaMax];
  __shared__ double acc[kEaMax];
  const int tid = threadIdx.x, w = tid >> 6, tile = blockIdx.x, g0 = blockIdx.y * kGroup;
  const int n = p.n, d = p.d, T = p.T, cd = p.cd, EA = p.EA;
  const int p0 = tile * p.P, p1 = p0 + p.P < n ? p0 + p.P : n;
  const double prior = 1.0 / n, dpp = prior * p.vs;
  const bool lead = (tid & 63) == 0;
  for (int g = 0; g < kGroup && g0 + g < p.cnt; ++g) {
    const int rl = g0 + g;
    const Slot s = slot_of(p, rl);
    if (s.flag[fDone]) continue;
    const EParams m = eparams_of(s, T, d, p.full != 0);
    double *post = post_of(p, rl);
    for (int e = tid; e < EA; e += kBlock) acc[e] = 0.0;
    __syncthreads();
    for (int q0 = p0; q0 < p1; q0 += kBlock) {
      const int pt = q0 + tid;
      const bool on = pt < p1;
      const double *x = p.x + (size_t)(on ? pt : p0) * d;
      double lx = 0.0;
      if (on) lx = estep_point(m, x, p.c + (size_t)pt * cd, dpp, post + pt, (size_t)n);
      for (int t = 0; t < T; ++t) {
        double po = 0.0;
        if (on) {
          po = exp(post[(size_t)t * n + pt]);
          post[(size_t)t * n + pt] = po;
        }
        const double wp = po * prior;
        double *q = wred[w] + t * (d + 2);
        for (int a = 0; a < d; ++a) {
          const double v = wave_sum(on ? wp * x[a] : 0.0);
          if (lead) q[a] = v;
        }
        const double vw = wave_sum(wp), vp = wave_sum(po);
        if (lead) {
          q[d] = vw;
          q[d + 1] = vp;
        }
      }
      lx = wave_sum(lx);
      if (lead) wred[w][EA - 1] = lx;
      __syncthreads();
      for (int e = tid; e < EA; e += kBlock) {
        double v = wred[0][e];
        for (int q = 1; q < kWaves; ++q) v += wred[q][e];
        acc[e] += v;
      }
      __syncthreads();
    }
    double *out = part_a(p, rl) + (size_t)tile * EA;
    for (int e = tid; e < EA; e += kBlock) out[e] = acc[e];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void ghem_finish1_kernel(const Args p) {
  __shared__ double tot[kEaMax];
  __shared__ int stop;
  const int tid = threadIdx.x, rl = blockIdx.x, d = p.d, T = p.T, EA = p.EA;
  const Slot s = slot_of(p, rl);
  if (s.flag[fDone]) return;
  const double *pa = part_a(p, rl);
  for (int e = tid; e < EA; e += kBlock) {
    double v = 0.0;
    for (int tile = 0; tile < p.nt; ++tile) v += pa[(size_t)tile * EA + e];
    tot[e] = v;
  }
  __syncthreads();
  if (tid == 0) stop = stop_rule(s, tot[EA - 1], p.n);
  __syncthreads();
  if (stop) {
    emit(p, rl, s);
    return;
  }
  for (int t = tid; t < T; t += kBlock) {
    s.mx[t] = tot[t * (d + 2) + d + 1] / p.n;
    s.sw[t] = tot[t * (d + 2) + d];
  }
  for (int e = tid; e < T * d; e += kBlock) {
    const int t = e / d, a = e % d;
    s.cen[e] = tot[t * (d + 2) + a] / tot[t * (d + 2) + d];
  }
}

__global__ __launch_bounds__(kBlock) void ghem_cov_kernel(const Args p) {
  const int tid = threadIdx.x, tile = blockIdx.x, g0 = blockIdx.y * kGroup;
  const int n = p.n, d = p.d, cd = p.cd, EB = p.EB;
  const int p0 = tile * p.P, p1 = p0 + p.P < n ? p0 + p.P : n;
  const int gn = p.cnt - g0 < kGroup ? p.cnt - g0 : kGroup, total = gn * EB;
  const double prior = 1.0 / n;
  for (int base = 0; base < total; base += kBlock * kAcc) {
    double acc[kAcc], ca[kAcc], cb[kAcc];
    const double *wq[kAcc];
    double *out[kAcc];
    int ia[kAcc], ib[kAcc], iab[kAcc];
    bool on[kAcc];
    WTK_UNROLL
    for (int k = 0; k < kAcc; ++k) {
      const int idx = base + k * kBlock + tid;
      acc[k] = 0.0;
      ca[k] = cb[k] = 0.0;
      wq[k] = nullptr;
      out[k] = nullptr;
      ia[k] = ib[k] = iab[k] = 0;
      on[k] = idx < total;
      if (!on[k]) continue;
      const int rl = g0 + idx / EB, e = idx % EB;
      const Slot s = slot_of(p, rl);
      if (s.flag[fDone]) {
        on[k] = false;
        continue;
      }
      const int t = e / cd, ab = e % cd;
      ia[k] = p.full ? ab / d : ab;
      ib[k] = p.full ? ab % d : ab;
      iab[k] = ab;
      ca[k] = s.cen[(size_t)t * d + ia[k]];
      cb[k] = s.cen[(size_t)t * d + ib[k]];
      wq[k] = post_of(p, rl) + (size_t)t * n;
      out[k] = part_b(p, rl) + (size_t)tile * EB + e;
    }
    for (int pt = p0; pt < p1; ++pt) {
      const double *x = p.x + (size_t)pt * d, *C = p.c + (size_t)pt * cd;
      WTK_UNROLL
      for (int k = 0; k < kAcc; ++k)
        if (on[k]) acc[k] += cov_term(wq[k][pt] * prior, x, C, ca[k], cb[k], ia[k], ib[k], iab[k]);
    }
    WTK_UNROLL
    for (int k = 0; k < kAcc; ++k)
      if (on[k]) *out[k] = acc[k];
  }
}

__global__ __launch_bounds__(kBlock) void ghem_finish2_kernel(const Args p) {
  __shared__ double fac[kWaves][2][kMaxDim * kMaxDim];
  __shared__ int sing;
  const int tid = threadIdx.x, rl = blockIdx.x, cd = p.cd, EB = p.EB;
  const Slot s = slot_of(p, rl);
  if (s.flag[fDone]) return;
  const double *pb = part_b(p, rl);
  for (int e = tid; e < EB; e += kBlock) {
    double v = 0.0;
    for (int tile = 0; tile < p.nt; ++tile) v += pb[(size_t)tile * EB + e];
    s.vr[e] = v / s.sw[e / cd];
  }
  __syncthreads();
  if (p.it == p.iterations - 1) {
    end_trial(p, rl, s, kOk);
    return;
  }
  if (block_prepare(p, s, fac, &sing)) end_trial(p, rl, s, kSingular);
}

__global__ __launch_bounds__(kBlock) void ghem_logpost_kernel(const Args p) {
  const int tid = threadIdx.x, tile = blockIdx.x, g0 = blockIdx.y * kGroup;
  const int n = p.n, d = p.d, T = p.T, cd = p.cd;
  const int p0 = tile * p.P, p1 = p0 + p.P < n ? p0 + p.P : n;
  const double dpp = (1.0 / n) * p.vs;
  for (int g = 0; g < kGroup && g0 + g < p.cnt; ++g) {
    const int rl = g0 + g;
    const Slot s = slot_of(p, rl);
    if (!s.flag[fDone] || s.flag[fStatus] != kOk) continue;
    const EParams m = eparams_of(s, T, d, p.full != 0);
    double *lp = p.logpost + (size_t)(p.R0 + rl) * T * n;
    const bool any = s.flag[fEsteps] > 0;
    for (int pt = p0 + tid; pt < p1; pt += kBlock) {
      if (any)
        estep_point(m, p.x + (size_t)pt * d, p.c + (size_t)pt * cd, dpp, lp + pt, (size_t)n);
      else
        for (int t = 0; t < T; ++t) lp[(size_t)t * n + pt] = 0.0;
    }
  }
}

struct Plan {
  int cd, nt, P, EA, EB, chunk;
  size_t SL, TS, fixed, bytes;
};

Plan plan_of(int n, int d, int full, int T, int R, int chunk_trials) {
  Plan q{};
  q.cd = cov_len(d, full != 0);
  q.P = tile_points(n, d);
  q.nt = tiles_of(n, d);
  q.EA = ea_len(T, d);
  q.EB = T * q.cd;
  q.SL = slot_len(T, d, q.cd);
  q.TS = q.SL + (size_t)q.nt * (q.EA + q.EB) + (size_t)T * n;
  q.fixed = (size_t)kHead + (size_t)q.nt * q.cd + (size_t)q.nt;
  const size_t fit =
      VBHEM_GHEM_DEFAULT_WORKSPACE > q.fixed * 8 ? (VBHEM_GHEM_DEFAULT_WORKSPACE - q.fixed * 8) / (q.TS * 8) : 0;
  const int most = std::max(R, 1);
  q.chunk = chunk_trials > 0 ? std::min(chunk_trials, most) : (int)std::max<size_t>(1, std::min<size_t>(most, fit));
  q.bytes = 8 * (q.fixed + (size_t)q.chunk * q.TS);
  return q;
}

int check_sizes(const char *what, int n, int d, int T, int R, int iterations, int chunk_trials) {
  if (n < 1 || d < 1 || T < 2 || R < 0 || iterations < 0 || chunk_trials < 0)
    return set_error(VBHEM_ERR_ARG, std::string(what) + ": need n, d >= 1, T >= 2 and R, iterations, chunk_trials >= 0");
  if (d > kMaxDim) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": d <= 16 supported");
  if (T > kMaxT) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": T <= 32 supported");
  return VBHEM_OK;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhem_ghem_workspace_bytes(int n, int d, int full, int T, int R, int chunk_trials) {
  using namespace vbhem;
  if (check_sizes("vbhem_ghem_workspace_bytes", n, d, T, R, 0, chunk_trials) != VBHEM_OK) return 0;
  return plan_of(n, d, full, T, R, chunk_trials).bytes;
}

int vbhem_ghem_fit_batch(int n, int d, int full, int T, int R, const double *x_dev, const double *cov_dev,
                         double virtual_samples, int iterations, const int *j0_dev, const double *u_dev,
                         const double *init_centres_dev, int chunk_trials, double *mxwt_dev, double *centres_dev,
                         double *covars_dev, double *logpost_dev, double *logp_dev, int *status_dev, int *iters_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  const int rc = check_sizes("vbhem_ghem_fit_batch", n, d, T, R, iterations, chunk_trials);
  if (rc != VBHEM_OK) return rc;
  if (R == 0) return VBHEM_OK;
  if (!x_dev || !cov_dev || (!init_centres_dev && (!j0_dev || !u_dev)) || !mxwt_dev || !centres_dev || !covars_dev ||
      !logp_dev || !status_dev || !iters_dev)
    return set_error(VBHEM_ERR_ARG, "vbhem_ghem_fit_batch: null array");
  const Plan q = plan_of(n, d, full, T, R, chunk_trials);
  if (!workspace_dev || workspace_bytes < q.bytes)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(q.bytes) + " bytes");
  Args a{};
  a.n = n; a.d = d; a.T = T; a.cd = q.cd; a.nt = q.nt; a.P = q.P; a.full = full != 0; a.iterations = iterations;
  a.ustride = std::max(T - 1, 1); a.EA = q.EA; a.EB = q.EB; a.vs = virtual_samples;
  a.x = x_dev; a.c = cov_dev; a.u = u_dev; a.init = init_centres_dev; a.j0 = j0_dev;
  a.mxwt = mxwt_dev; a.centres = centres_dev; a.covars = covars_dev; a.logpost = logpost_dev; a.logp = logp_dev;
  a.status = status_dev; a.iters = iters_dev;
  a.head = static_cast<double *>(workspace_dev);
  a.scanp = a.head + kHead;
  a.scanbad = reinterpret_cast<int *>(a.scanp + (size_t)q.nt * q.cd);
  a.trials = a.scanp + (size_t)q.nt * q.cd + q.nt;
  a.TS = q.TS; a.SL = q.SL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock);
#define GHEM_LAUNCH(kernel, grid)                               \
  do {                                                          \
    hipLaunchKernelGGL(kernel, grid, block, 0, st, a);          \
    const hipError_t e = hipGetLastError();                     \
    if (e != hipSuccess) return hip_fail(e, #kernel);           \
  } while (0)
  GHEM_LAUNCH(ghem_scan_kernel, dim3((unsigned)q.nt));
  GHEM_LAUNCH(ghem_scan_finish, dim3(1));
  for (int r0 = 0; r0 < R; r0 += q.chunk) {
    a.R0 = r0;
    a.cnt = std::min(q.chunk, R - r0);
    const dim3 per_trial((unsigned)a.cnt), tiles((unsigned)q.nt, (unsigned)((a.cnt + kGroup - 1) / kGroup));
    switch (wtkrun::dim_bucket(d)) {
      case 2: GHEM_LAUNCH(ghem_seed_kernel<2>, per_trial); break;
      case 4: GHEM_LAUNCH(ghem_seed_kernel<4>, per_trial); break;
      case 8: GHEM_LAUNCH(ghem_seed_kernel<8>, per_trial); break;
      default: GHEM_LAUNCH(ghem_seed_kernel<16>, per_trial); break;
    }
    for (int it = 0; it < iterations; ++it) {
      a.it = it;
      GHEM_LAUNCH(ghem_estep_kernel, tiles);
      GHEM_LAUNCH(ghem_finish1_kernel, per_trial);
      GHEM_LAUNCH(ghem_cov_kernel, tiles);
      GHEM_LAUNCH(ghem_finish2_kernel, per_trial);
    }
    if (logpost_dev) GHEM_LAUNCH(ghem_logpost_kernel, tiles);
  }
#undef GHEM_LAUNCH
  return VBHEM_OK;
}

}  // extern "C"
