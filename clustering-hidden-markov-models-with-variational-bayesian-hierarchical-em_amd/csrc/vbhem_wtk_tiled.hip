// vbhem_wtk_tiled.hip -- the TILED schedule of the initialisations' k-means
// (include/vbhem_init.h: vbhem_wtk_cluster_tiled_batch, vbhem_wtk_seed_tiled_batch).  The
// phases, the record and the rules are vbhem_wtk_tiled_run.h, shared with the host check
// build; the per-point arithmetic is vbhem_wtk_run.h's, shared with the block schedule.
//
// Per chunk of trials: one wtk_step_kernel launch that writes the records, then per round
// two launches and no host read:
//   wtk_tile_kernel<DB>  grid (point tile, group of kGroup trials), 256 threads.  A block
//                        loops over its group's trials with the same tile (256 points at a
//                        time, staged in LDS): it reads the trial's record and does the
//                        phase's per-point work, a thread per point; then one thread per
//                        (cluster, entry) walks the staged points in point order.  The
//                        tile's row of partials goes to the workspace.
//   wtk_step_kernel      one workgroup per trial: the rows added in tile order, a thread per
//                        entry; the phase's rule; the record, and the outputs of a trial
//                        that ends.
// A finished trial sets its done flag; every later launch leaves it before any write.  A
// trial that empties a cluster in LLOYD sets its re-seed flag and ends without outputs;
// after the rounds the block schedule's kernel runs over the chunk and computes exactly the
// flagged trials from scratch.  The number of launches is fixed by K and the pass caps.  No
// atomics, no block waits on another; every loop is bounded by n, K, d, the tile count, the
// group size or the pass caps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_init.h"
#include "vbhem_internal.h"
#include "vbhem_wtk_tiled_run.h"

namespace vbhem {
namespace {

using namespace wtktile;

constexpr int kEnt = (kMaxK * (kMaxDim + 1) + kBlock - 1) / kBlock;  // sums a thread walks for

struct Args {
  int n, d, K, P, nt, E, R0, cnt, round, seed_only, ustride;
  const double *x, *w, *u;
  const int *j0;
  int *labels, *counts, *status, *iters;
  double *centres;
  double *wd;  // [chunk][n]: d2
  int *wl;     // [chunk][n]: labels
  double *recs, *parts;
  int *badt;  // [nt]
  size_t RL, PS;
};

__device__ inline Rec rec_of(const Args &p, int rl) { return rec_at(p.recs + (size_t)rl * p.RL, p.K, p.d); }

// Every thread e < K (d + 1) adds the staged points of its (cluster, entry) in point order.
__device__ inline void walk_sums(double (&acc)[kEnt], const double *xs, const double *wsm, const int *labs, int cntp,
                                 int K, int d, bool weighted) {
  WTK_UNROLL
  for (int k = 0; k < kEnt; ++k) {
    const int e = threadIdx.x + k * kBlock;
    if (e >= K * (d + 1)) continue;
    const int c = e / (d + 1), a = e % (d + 1);
    double s = acc[k];
    if (a < d) {
      if (weighted) {
        for (int m = 0; m < cntp; ++m)
          if (labs[m] == c) s += xs[m * d + a] * wsm[m];
      } else {
        for (int m = 0; m < cntp; ++m)
          if (labs[m] == c) s += xs[m * d + a];
      }
    } else {
      for (int m = 0; m < cntp; ++m)
        if (labs[m] == c) s += weighted ? wsm[m] : 1.0;
    }
    acc[k] = s;
  }
}

template <int DB>
__global__ __launch_bounds__(kBlock) void wtk_tile_kernel(const Args p) {
  __shared__ double xs[kBlock * DB], cen[kMaxK * DB], cw[kMaxK], ev[kBlock], wsm[kBlock];
  __shared__ int labs[kBlock];
  const int tid = threadIdx.x, tile = blockIdx.x, g0 = blockIdx.y * kGroup;
  const int n = p.n, d = p.d, K = p.K;
  const int p0 = tile * p.P, p1 = p0 + p.P < n ? p0 + p.P : n;
  if (p.round == 0 && blockIdx.y == 0) {  // the BAD check of the shared points, once per chunk
    int bad = 0;
    for (size_t e = (size_t)p0 * d + tid; e < (size_t)p1 * d; e += kBlock) bad |= !finite_d(p.x[e]);
    if (p.w)
      for (int m = p0 + tid; m < p1; m += kBlock) bad |= !finite_d(p.w[m]);
    bad = __syncthreads_or(bad);
    if (tid == 0) p.badt[tile] = bad;
  }
  for (int g = 0; g < kGroup && g0 + g < p.cnt; ++g) {
    const int rl = g0 + g;
    const Rec r = rec_of(p, rl);
    if (r.flag[fDone]) continue;
    const int phase = r.flag[fPhase], step = r.flag[fStep];
    const bool sweep = phase == kWeighted && step >= 1;
    double *dwork = p.wd + (size_t)rl * n;
    int *lwork = p.wl + (size_t)rl * n;
    int *lout = sweep ? p.labels + (size_t)(p.R0 + rl) * n : nullptr;
    __syncthreads();  // the previous trial's walks are over
    for (int e = tid; e < K * d; e += kBlock) cen[e] = r.cen[e];
    if (tid < K) cw[tid] = phase == kWeighted ? r.cw[tid] : 0.0;
    double acc[kEnt];
    WTK_UNROLL
    for (int k = 0; k < kEnt; ++k) acc[k] = 0.0;
    double aen = 0.0, acn = 0.0, scal = 0.0;
    int changed = 0;
    for (int q0 = p0; q0 < p1; q0 += kBlock) {
      const int cntp = p1 - q0 < kBlock ? p1 - q0 : kBlock, pt = q0 + tid;
      const bool on = tid < cntp;
      __syncthreads();  // the previous part's walks are over
      for (int e = tid; e < cntp * d; e += kBlock) xs[e] = p.x[(size_t)q0 * d + e];
      wsm[tid] = on && p.w ? p.w[pt] : 0.0;
      __syncthreads();
      const double *xp = xs + tid * d;
      if (phase == kSeed) {
        if (on) {
          const double v = dist2(xp, cen + (step - 1) * d, d);
          double dd = step == 1 ? v : dwork[pt];
          if (v < dd) dd = v;
          dwork[pt] = dd;
          ev[tid] = dd;
        }
        __syncthreads();
        if (tid == 0)
          for (int m = 0; m < cntp; ++m) scal += ev[m];
      } else if (!sweep) {  // LLOYD, or the first assignment of WEIGHTED
        int ch = 0;
        if (on) {
          double dm;
          const int l = nearest(xp, cen, K, d, &dm);
          ch = phase == kLloyd && step > 0 && l != lwork[pt];
          lwork[pt] = l;
          labs[tid] = l;
        }
        changed += __syncthreads_count(ch);
        walk_sums(acc, xs, wsm, labs, cntp, K, d, phase == kWeighted);
      } else {
        int l = 0;
        double f = 0.0;
        if (on) {
          l = lwork[pt];
          lout[pt] = l;
          const double fm = dist2(xp, cen + l * d, d);
          ev[tid] = wsm[tid] * fm;
          f = wk_member_f(fm, cw[l], wsm[tid]);
          labs[tid] = l;
        }
        __syncthreads();
        if (tid < K)
          for (int m = 0; m < cntp; ++m)
            if (labs[m] == tid) {
              aen += ev[m];
              acn += 1.0;
            }
        if (step <= kWkMax) {
          __syncthreads();
          if (on) {
            const int ln = wk_assign(xp, wsm[tid], l, f, cen, cw, K, d);
            lwork[pt] = ln;
            labs[tid] = ln;
          }
          __syncthreads();
          walk_sums(acc, xs, wsm, labs, cntp, K, d, true);
        }
      }
    }
    double *row = p.parts + (size_t)rl * p.PS + (size_t)tile * p.E;
    if (phase != kSeed) {
      WTK_UNROLL
      for (int k = 0; k < kEnt; ++k) {
        const int e = tid + k * kBlock;
        if (e < K * (d + 1)) row[o_sum() + e] = acc[k];
      }
    }
    if (sweep && tid < K) {
      row[o_energy(K, d) + tid] = aen;
      row[o_count(K, d) + tid] = acn;
    }
    if (tid == 0) row[o_scalar(K, d)] = phase == kSeed ? scal : (double)changed;
  }
}

// The end of a trial: its status and its done flag.
__device__ inline void end_trial(const Args &p, int rl, const Rec &r, int status) {
  if (threadIdx.x == 0) {
    r.flag[fStatus] = status;
    r.flag[fDone] = 1;
    p.status[p.R0 + rl] = status;
  }
}

__global__ __launch_bounds__(kBlock) void wtk_step_kernel(const Args p) {
  __shared__ double tot[kPartMax];
  __shared__ double sc[1024];
  __shared__ double s_excl;
  __shared__ int s_tile, s_pick, s_flag;
  const int tid = threadIdx.x, rl = blockIdx.x, r_out = p.R0 + rl, n = p.n, d = p.d, K = p.K, E = p.E, nt = p.nt;
  const Rec r = rec_of(p, rl);
  if (p.round < 0) {  // before the first round: the record
    if (tid == 0 && !rec_init(r, p.x, n, d, K, p.j0[r_out])) p.status[r_out] = kBad;
    return;
  }
  if (r.flag[fDone]) return;
  const int phase = r.flag[fPhase], step = r.flag[fStep];
  const double eold = *r.eold;
  if (p.round == 0) {
    int bad = 0;
    for (int t = tid; t < nt; t += kBlock) bad |= p.badt[t];
    if (__syncthreads_or(bad)) {
      end_trial(p, rl, r, kBad);
      return;
    }
  }
  const double *part = p.parts + (size_t)rl * p.PS;
  for (int e = tid; e < E; e += kBlock) {
    double v = 0.0;
#pragma unroll 8
    for (int t = 0; t < nt; ++t) v += part[(size_t)t * E + e];
    tot[e] = v;
  }
  __syncthreads();
  const double *sums = tot + o_sum();
  if (phase == kSeed) {
    const double total = tot[o_scalar(K, d)];
    if (!(total > 0.0) || !finite_d(total)) {
      end_trial(p, rl, r, kDegenerate);
      return;
    }
    const double target = p.u[(size_t)r_out * p.ustride + step - 1] * total;
    // the tile that holds the target: the running sum over the tiles, 1,024 at a time
    if (tid == 0) {
      s_tile = -1;
      s_excl = 0.0;
    }
    double run = 0.0, excl = 0.0;  // thread 0's
    for (int t0 = 0; t0 < nt; t0 += 1024) {
      const int ct = nt - t0 < 1024 ? nt - t0 : 1024;
      __syncthreads();
      if (s_tile >= 0) break;
      for (int i = tid; i < ct; i += kBlock) sc[i] = part[(size_t)(t0 + i) * E + o_scalar(K, d)];
      __syncthreads();
      if (tid == 0)
        for (int i = 0; i < ct; ++i) {
          excl = run;
          run += sc[i];
          if (run > target) {
            s_tile = t0 + i;
            s_excl = excl;
            break;
          }
        }
    }
    __syncthreads();
    if (tid == 0 && s_tile < 0) {  // rounding left none: the last tile, from its own start
      s_tile = nt - 1;
      s_excl = excl;
    }
    __syncthreads();
    const int tile = s_tile, p0 = tile * p.P, cntp = (p0 + p.P < n ? p0 + p.P : n) - p0;
    const double *d2 = p.wd + (size_t)rl * n + p0;
    for (int i = tid; i < cntp; i += kBlock) sc[i] = d2[i];
    __syncthreads();
    if (tid == 0) {
      const int m = seed_search(sc, cntp, s_excl, target);
      s_pick = m == kNone ? seed_fallback(tile, nt, p.P, n) : p0 + m;
    }
    __syncthreads();
    if (tid < d) r.cen[(size_t)step * d + tid] = p.x[(size_t)s_pick * d + tid];
    if (tid == 0) {
      r.flag[fPhase] = step + 1 == K ? kLloyd : kSeed;
      r.flag[fStep] = step + 1 == K ? 0 : step + 1;
    }
    return;
  }
  if (phase == kLloyd) {
    const int passes = step + 1;
    bool ended = step > 0 && tot[o_scalar(K, d)] == 0.0;
    if (!ended) {
      int empty = 0;
      for (int c = tid; c < K; c += kBlock) empty |= !(sums[c * (d + 1) + d] > 0.0);
      if (__syncthreads_or(empty)) {
        if (tid == 0) {
          r.flag[fReseed] = 1;
          r.flag[fDone] = 1;
        }
        return;
      }
      for (int e = tid; e < K * d; e += kBlock) {
        const int c = e / d, a = e % d;
        r.cen[e] = sums[c * (d + 1) + a] / sums[c * (d + 1) + d];
      }
      ended = passes == kLloydMax;
    }
    __syncthreads();  // the centres are written before a seeding trial copies them out
    if (tid == 0) {
      r.flag[fStep] = passes;
      if (ended) {
        r.flag[fIt0] = passes;
        if (!p.seed_only) {
          r.flag[fPhase] = kWeighted;
          r.flag[fStep] = 0;
        }
      }
    }
    if (ended && p.seed_only) {
      for (int e = tid; e < K * d; e += kBlock) p.centres[(size_t)r_out * K * d + e] = r.cen[e];
      if (tid == 0) p.iters[r_out] = passes;
      end_trial(p, rl, r, kOk);
    }
    return;
  }
  if (step >= 1) {
    if (tid == 0) {
      double en = 0.0;
      for (int c = 0; c < K; ++c) en += tot[o_energy(K, d) + c];
      int sweeps = 0;
      s_flag = weighted_stop(step, en, eold, &sweeps);
      if (s_flag) {
        r.flag[fIt1] = sweeps;
        p.iters[2 * r_out] = r.flag[fIt0];
        p.iters[2 * r_out + 1] = sweeps;
      } else {
        *r.eold = en;
      }
    }
    __syncthreads();
    if (s_flag) {
      if (tid < K) p.counts[(size_t)r_out * K + tid] = (int)tot[o_count(K, d) + tid];
      end_trial(p, rl, r, kOk);
      return;
    }
  }
  for (int e = tid; e < K * d; e += kBlock) {
    const int c = e / d, a = e % d;
    const double cwc = sums[c * (d + 1) + d], s = sums[c * (d + 1) + a];
    r.cen[e] = cwc > 0.0 ? s / cwc : s;
  }
  if (tid < K) r.cw[tid] = sums[tid * (d + 1) + d];
  if (tid == 0) r.flag[fStep] = step + 1;
}

// The re-seed hand-over of a seeding call: kmeans_pp by the block routine, from scratch, for
// the trials whose flag is set.
template <int DB>
__global__ __launch_bounds__(kBlock) void wtk_seed_block_kernel(const Args p) {
  __shared__ Block<DB> b;
  const int tid = threadIdx.x, rl = blockIdx.x, r_out = p.R0 + rl, n = p.n, d = p.d, K = p.K;
  const Rec r = rec_of(p, rl);
  if (!r.flag[fReseed]) return;
  const PPResult pp = block_kmeans_pp(b, p.x, d, nullptr, n, K, p.j0[r_out], p.u + (size_t)r_out * p.ustride,
                                      kLloydMax, p.wd + (size_t)rl * n, p.wl + (size_t)rl * n);
  if (pp.status == kOk) {
    for (int e = tid; e < K * d; e += kBlock) p.centres[(size_t)r_out * K * d + e] = b.cen[e];
    if (tid == 0) p.iters[r_out] = pp.iters;
  }
  if (tid == 0) p.status[r_out] = pp.status;
}

struct Plan {
  int P, nt, E, chunk;
  size_t RL, PS, per_trial, fixed, bytes;  // in bytes but RL, PS (doubles)
};

size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

Plan plan_of(int n, int d, int K, int R, int chunk_trials) {
  Plan q{};
  q.P = tile_points(n, d);
  q.nt = tiles_of(n, d);
  q.E = part_len(K, d);
  q.RL = rec_len(K, d);
  q.PS = (size_t)q.nt * q.E;
  q.per_trial = (size_t)n * 8 + pad8((size_t)n * 4) + 8 * (q.RL + q.PS);
  q.fixed = pad8((size_t)q.nt * 4) + 8;  // (8: the int arrays' padding between the regions)
  const size_t fit = (VBHEM_WTK_DEFAULT_WORKSPACE - std::min<size_t>(q.fixed, VBHEM_WTK_DEFAULT_WORKSPACE)) / q.per_trial;
  const int most = std::max(R, 1);
  q.chunk = chunk_trials > 0 ? std::min(chunk_trials, most) : (int)std::max<size_t>(1, std::min<size_t>(most, fit));
  q.bytes = q.fixed + (size_t)q.chunk * q.per_trial;
  return q;
}

int check_sizes(const char *what, int n, int d, int K, int R, int chunk_trials, bool seed) {
  if (n < 1 || d < 1 || K < (seed ? 2 : 1) || R < 0 || chunk_trials < 0)
    return set_error(VBHEM_ERR_ARG, std::string(what) + (seed ? ": need n, d >= 1, K >= 2 and R, chunk_trials >= 0"
                                                               : ": need n, d, K >= 1 and R, chunk_trials >= 0"));
  if (d > kMaxDim) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": d <= 16 supported");
  if (K > kMaxK) return set_error(VBHEM_ERR_UNSUPPORTED, std::string(what) + ": K <= 32 supported");
  return VBHEM_OK;
}

#define WTK_LAUNCH(kernel, grid)                       \
  do {                                                 \
    hipLaunchKernelGGL(kernel, grid, block, 0, st, a); \
    const hipError_t e = hipGetLastError();            \
    if (e != hipSuccess) return hip_fail(e, #kernel);  \
  } while (0)

int run_tiled(int n, int d, int K, int R, const double *x, const double *w, const int *j0,
              const double *u, int chunk_trials, int *labels, int *counts, double *centres, int *status, int *iters,
              void *workspace, size_t workspace_bytes, void *stream) {
  const bool seed = w == nullptr;
  const Plan q = plan_of(n, d, K, R, chunk_trials);
  if (!workspace || workspace_bytes < q.bytes)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(q.bytes) + " bytes");
  Args a{};
  a.n = n; a.d = d; a.K = K; a.P = q.P; a.nt = q.nt; a.E = q.E; a.seed_only = seed; a.ustride = std::max(K - 1, 1);
  a.x = x; a.w = w; a.u = u; a.j0 = j0;
  a.labels = labels; a.counts = counts; a.status = status; a.iters = iters; a.centres = centres;
  a.wd = static_cast<double *>(workspace);
  a.wl = reinterpret_cast<int *>(a.wd + (size_t)q.chunk * n);
  a.recs = reinterpret_cast<double *>(reinterpret_cast<char *>(a.wl) + pad8((size_t)q.chunk * n * 4));
  a.parts = a.recs + (size_t)q.chunk * q.RL;
  a.badt = reinterpret_cast<int *>(a.parts + (size_t)q.chunk * q.PS);
  a.RL = q.RL; a.PS = q.PS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock);
  const int rounds = rounds_of(K, seed);
  for (int r0 = 0; r0 < R; r0 += q.chunk) {
    a.R0 = r0;
    a.cnt = std::min(q.chunk, R - r0);
    const dim3 per_trial((unsigned)a.cnt), tiles((unsigned)q.nt, (unsigned)((a.cnt + kGroup - 1) / kGroup));
    a.round = -1;
    WTK_LAUNCH(wtk_step_kernel, per_trial);
    for (int round = 0; round < rounds; ++round) {
      a.round = round;
      switch (dim_bucket(d)) {
        case 2: WTK_LAUNCH(wtk_tile_kernel<2>, tiles); break;
        case 4: WTK_LAUNCH(wtk_tile_kernel<4>, tiles); break;
        case 8: WTK_LAUNCH(wtk_tile_kernel<8>, tiles); break;
        default: WTK_LAUNCH(wtk_tile_kernel<16>, tiles); break;
      }
      WTK_LAUNCH(wtk_step_kernel, per_trial);
    }
    // the re-seed hand-over: the block schedule computes the flagged trials from scratch
    const int *only = reinterpret_cast<const int *>(a.recs) + fReseed;
    if (seed) {
      switch (dim_bucket(d)) {
        case 2: WTK_LAUNCH(wtk_seed_block_kernel<2>, per_trial); break;
        case 4: WTK_LAUNCH(wtk_seed_block_kernel<4>, per_trial); break;
        case 8: WTK_LAUNCH(wtk_seed_block_kernel<8>, per_trial); break;
        default: WTK_LAUNCH(wtk_seed_block_kernel<16>, per_trial); break;
      }
    } else {
      const int rc = wtk_block_rerun(n, d, K, r0, a.cnt, x, w, j0, u, labels, counts, status, iters, a.wd, a.wl, only,
                                     (int)(2 * q.RL), st);
      if (rc != VBHEM_OK) return rc;
    }
  }
  return VBHEM_OK;
}
#undef WTK_LAUNCH

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhem_wtk_cluster_tiled_workspace_bytes(int n, int d, int K, int R, int chunk_trials) {
  using namespace vbhem;
  if (check_sizes("vbhem_wtk_cluster_tiled_workspace_bytes", n, d, K, R, chunk_trials, false) != VBHEM_OK) return 0;
  return plan_of(n, d, K, R, chunk_trials).bytes;
}

int vbhem_wtk_cluster_tiled_batch(int n, int d, int K, int R, const double *x_dev, const double *weight_dev,
                                  const int *j0_dev, const double *u_dev, int chunk_trials, int *labels_dev,
                                  int *counts_dev, int *status_dev, int *iters_dev, void *workspace_dev,
                                  size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  const int rc = check_sizes("vbhem_wtk_cluster_tiled_batch", n, d, K, R, chunk_trials, false);
  if (rc != VBHEM_OK) return rc;
  if (R == 0) return VBHEM_OK;
  if (!x_dev || !weight_dev || !j0_dev || !u_dev || !labels_dev || !counts_dev || !status_dev || !iters_dev)
    return set_error(VBHEM_ERR_ARG, "vbhem_wtk_cluster_tiled_batch: null array");
  return run_tiled(n, d, K, R, x_dev, weight_dev, j0_dev, u_dev, chunk_trials,
                   labels_dev, counts_dev, nullptr, status_dev, iters_dev, workspace_dev, workspace_bytes, stream);
}

size_t vbhem_wtk_seed_tiled_workspace_bytes(int n, int d, int K, int R, int chunk_trials) {
  using namespace vbhem;
  if (check_sizes("vbhem_wtk_seed_tiled_workspace_bytes", n, d, K, R, chunk_trials, true) != VBHEM_OK) return 0;
  return plan_of(n, d, K, R, chunk_trials).bytes;
}

int vbhem_wtk_seed_tiled_batch(int n, int d, int K, int R, const double *x_dev, const int *j0_dev, const double *u_dev,
                               int chunk_trials, double *centres_dev, int *status_dev, int *iters_dev,
                               void *workspace_dev, size_t workspace_bytes, void *stream) {
  using namespace vbhem;
  const int rc = check_sizes("vbhem_wtk_seed_tiled_batch", n, d, K, R, chunk_trials, true);
  if (rc != VBHEM_OK) return rc;
  if (R == 0) return VBHEM_OK;
  if (!x_dev || !j0_dev || !u_dev || !centres_dev || !status_dev || !iters_dev)
    return set_error(VBHEM_ERR_ARG, "vbhem_wtk_seed_tiled_batch: null array");
  return run_tiled(n, d, K, R, x_dev, nullptr, j0_dev, u_dev, chunk_trials, nullptr,
                   nullptr, centres_dev, status_dev, iters_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
