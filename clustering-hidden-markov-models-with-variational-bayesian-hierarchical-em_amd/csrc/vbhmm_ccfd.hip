// vbhmm_ccfd.hip -- CCFD clustering of point HMMs (include/vbhmm_ccfd.h): the
// symmetrised-KL distance matrix of src/compare_mtds/ccfd/myccfd.m:14-30 without the
// [H][N_total] log-likelihood matrix, and the row sweeps of CCFD.m over it.
//
// Distance, three launches:
//   ccfd_own_kernel    a workgroup per (HMM i, tile of 128 of its own sequences), block
//                      i staged in LDS as hmm_score_kernel does; own[n] = ll_i(n) / T_n.
//   ccfd_cross_kernel  a workgroup per (HMM j, tile of whole segments), block j in LDS,
//                      one lane per sequence.  Every lane leaves its term
//                      own[n] - ll_j(n) / T_n in LDS; after the barrier one lane per
//                      segment adds that segment's terms one after the other, in
//                      sequence order, from 0.  A tile is either consecutive whole
//                      segments of at most 128 sequences in all, or one longer segment
//                      alone, taken in passes of 128 with lane 0 carrying the sum on.
//                      So a segment's sum is the same chain of additions wherever the
//                      segment lies.  KL[i][j] goes to D[i][j].
//   ccfd_sym_kernel    a workgroup per row i; the lane that owns the pair (i, j > i)
//                      reads D[i][j] and D[j][i] and stores 0.5 (a + b) to both; the
//                      row's minimum and maximum over j > i come out of the same read.
// The tile tables are built on the host from seg_offsets once per call.
//
// Passes: a workgroup of 256 lanes per row, the row read by consecutive lanes;
// reductions by shuffles inside a wave, then lane 0 combines the four waves' results
// from LDS in wave order.  Up to three cut-offs share one read of the matrix.  The
// per-entry decisions are vbhmm_ccfd_row.h, shared with the host check build.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_ccfd.h"
#include "vbhmm_ccfd_row.h"
#include "vbhmm_hmmset.h"
#include "vbhmm_score_pair.h"

namespace vbhem {
namespace {

using namespace score;
using namespace ccfd;

constexpr int kDistThreads = 128;  // lanes = sequences per tile
constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / 64;

struct DistArgs {
  int H, d, diag, tiles;
  Layout L;
  const double *blocks;
  const int *offsets, *seg;
  const double *x;
  double *own;
  const int2 *own_tiles;    // (HMM, first sequence)
  const int4 *cross_tiles;  // (first sequence, sequences, first segment, segments)
  double *D;
};

template <int KB, int DB>
__device__ inline double seq_loglik(const DistArgs &p, const Hmm &m, int n, int &T) {
  const int off = p.offsets[n];
  T = p.offsets[n + 1] - off;
  return pair_loglik<KB, DB>(m, p.x + (size_t)off * p.d, T, p.d);
}

template <int KB, int DB>
__global__ __launch_bounds__(kDistThreads) void ccfd_own_kernel(const DistArgs p) {
  __shared__ double sh[BlockLen<KB, DB>::value];
  const int2 t = p.own_tiles[blockIdx.x];
  const double *blk = p.blocks + (size_t)t.x * p.L.stride;
  hmmset::stage_block(sh, blk, p.L.stride, kDistThreads);
  __syncthreads();
  const int n = t.y + threadIdx.x;
  if (n >= p.seg[t.x + 1]) return;
  const Hmm m = view(p.L, sh, p.diag != 0);
  int T;
  const double ll = seq_loglik<KB, DB>(p, m, n, T);
  p.own[n] = ll / (double)T;
}

template <int KB, int DB>
__global__ __launch_bounds__(kDistThreads) void ccfd_cross_kernel(const DistArgs p) {
  __shared__ double sh[BlockLen<KB, DB>::value];
  __shared__ double term[kDistThreads];
  const int j = blockIdx.x / p.tiles, tid = threadIdx.x;
  const int4 t = p.cross_tiles[blockIdx.x % p.tiles];
  const int n0 = t.x, cnt = t.y, s0 = t.z, nseg = t.w;
  const double *blk = p.blocks + (size_t)j * p.L.stride;
  hmmset::stage_block(sh, blk, p.L.stride, kDistThreads);
  __syncthreads();
  const Hmm m = view(p.L, sh, p.diag != 0);
  if (cnt > kDistThreads) {  // one long segment, in passes; uniform over the workgroup
    double sum = 0.0;
    for (int base = 0; base < cnt; base += kDistThreads) {
      const int left = cnt - base < kDistThreads ? cnt - base : kDistThreads;
      if (tid < left) {
        int T;
        const int n = n0 + base + tid;
        const double ll = seq_loglik<KB, DB>(p, m, n, T);
        term[tid] = kl_term(p.own[n], ll, T);
      }
      __syncthreads();
      if (tid == 0)
        for (int q = 0; q < left; ++q) sum += term[q];
      __syncthreads();
    }
    if (tid == 0) p.D[(size_t)s0 * p.H + j] = sum / (double)cnt;
    return;
  }
  if (tid < cnt) {
    int T;
    const int n = n0 + tid;
    const double ll = seq_loglik<KB, DB>(p, m, n, T);
    term[tid] = kl_term(p.own[n], ll, T);
  }
  __syncthreads();
  if (tid < nseg) {
    const int s = s0 + tid, a = p.seg[s] - n0, b = p.seg[s + 1] - n0;
    double sum = 0.0;
    for (int q = a; q < b; ++q) sum += term[q];
    p.D[(size_t)s * p.H + j] = sum / (double)(b - a);
  }
}

struct LaunchOwn {
  const DistArgs &a;
  unsigned grid;
  hipStream_t st;
  template <int KB, int DB>
  hipError_t operator()() const {
    hipLaunchKernelGGL((ccfd_own_kernel<KB, DB>), dim3(grid), dim3(kDistThreads), 0, st, a);
    return hipGetLastError();
  }
};

struct LaunchCross {
  const DistArgs &a;
  unsigned grid;
  hipStream_t st;
  template <int KB, int DB>
  hipError_t operator()() const {
    hipLaunchKernelGGL((ccfd_cross_kernel<KB, DB>), dim3(grid), dim3(kDistThreads), 0, st, a);
    return hipGetLastError();
  }
};

// ---------------------------------------------------------------------------
// reductions over a row: shuffles inside a wave, then lane 0 over the waves in order
// ---------------------------------------------------------------------------
__device__ inline Best shfl_down(const Best &b, int o) {
  Best r;
  r.d = __shfl_down(b.d, o, 64);
  r.rank = __shfl_down(b.rank, o, 64);
  r.j = __shfl_down(b.j, o, 64);
  return r;
}
__device__ inline double shfl_down(double v, int o) { return __shfl_down(v, o, 64); }
__device__ inline int shfl_down(int v, int o) { return __shfl_down(v, o, 64); }

// the workgroup's combined value, valid on lane 0; part: kRowWaves entries of LDS
template <class T, class F>
__device__ inline T row_reduce(T v, F comb, T *part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u = shfl_down(v, o);
    comb(v, u);
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kRowWaves; ++w) comb(v, part[w]);
  return v;
}

struct MinOp {
  __device__ void operator()(double &a, double b) const { a = fmin(a, b); }
};
struct MaxOp {
  __device__ void operator()(double &a, double b) const { a = fmax(a, b); }
};
struct AddOp {
  __device__ void operator()(int &a, int b) const { a += b; }
};
struct BestOp {
  __device__ void operator()(Best &a, const Best &b) const { best_merge(a, b); }
};

template <bool SYM>
__global__ __launch_bounds__(kRowThreads) void ccfd_sym_kernel(double *D, int N, double *rowmin,
                                                               double *rowmax) {
  __shared__ double pmin[kRowWaves], pmax[kRowWaves];
  const int i = blockIdx.x;
  double *row = D + (size_t)i * N;
  double mn = INFINITY, mx = -INFINITY;
  for (int j = i + 1 + (int)threadIdx.x; j < N; j += kRowThreads) {
    double v = row[j];
    if (SYM) {
      double *mirror = D + (size_t)j * N + i;
      v = 0.5 * (v + *mirror);
      row[j] = v;
      *mirror = v;
    }
    mn = fmin(mn, v);
    mx = fmax(mx, v);
  }
  mn = row_reduce(mn, MinOp{}, pmin);
  mx = row_reduce(mx, MaxOp{}, pmax);
  if (threadIdx.x == 0) {
    if (SYM) row[i] = 0.0;
    rowmin[i] = mn;
    rowmax[i] = mx;
  }
}

struct CutArgs {
  double dc[kMaxCut];
};

__global__ __launch_bounds__(kRowThreads) void ccfd_rho_kernel(const double *D, int N, CutArgs cut, int C,
                                                               int *rho) {
  __shared__ int part[kMaxCut][kRowWaves];
  const int i = blockIdx.x;
  const double *row = D + (size_t)i * N;
  int cnt[kMaxCut] = {0, 0, 0};
  for (int j = threadIdx.x; j < N; j += kRowThreads) {
    const double v = row[j];
#pragma unroll
    for (int c = 0; c < kMaxCut; ++c)
      if (c < C && j != i && rho_hit(v, cut.dc[c])) ++cnt[c];
  }
#pragma unroll
  for (int c = 0; c < kMaxCut; ++c) {
    if (c >= C) break;
    const int s = row_reduce(cnt[c], AddOp{}, part[c]);
    if (threadIdx.x == 0) rho[(size_t)c * N + i] = s;
  }
}

__global__ __launch_bounds__(kRowThreads) void ccfd_delta_kernel(const double *D, int N, const int *rank, int C,
                                                                 double maxd, double *delta, int *nneigh) {
  __shared__ Best part[kMaxCut][kRowWaves];
  const int i = blockIdx.x;
  const double *row = D + (size_t)i * N;
  Best b[kMaxCut];
  int ri[kMaxCut];
#pragma unroll
  for (int c = 0; c < kMaxCut; ++c) {
    b[c] = best_none();
    ri[c] = c < C ? rank[(size_t)c * N + i] : 0;
  }
  for (int j = threadIdx.x; j < N; j += kRowThreads) {
    const double v = row[j];
#pragma unroll
    for (int c = 0; c < kMaxCut; ++c)
      if (c < C) best_take(b[c], v, rank[(size_t)c * N + j], ri[c], j);
  }
#pragma unroll
  for (int c = 0; c < kMaxCut; ++c) {
    if (c >= C) break;
    const Best r = row_reduce(b[c], BestOp{}, part[c]);
    if (threadIdx.x == 0) {
      double dl;
      int nn;
      best_finish(r, ri[c], maxd, dl, nn);
      delta[(size_t)c * N + i] = dl;
      nneigh[(size_t)c * N + i] = nn;
    }
  }
}

__global__ __launch_bounds__(kRowThreads) void ccfd_border_kernel(const double *D, int N, double dc,
                                                                  const int *cl, const int *rho, double *out) {
  __shared__ double part[kRowWaves];
  const int i = blockIdx.x;
  const double *row = D + (size_t)i * N;
  const int ci = cl[i], ri = rho[i];
  double mx = 0.0;
  for (int j = threadIdx.x; j < N; j += kRowThreads)
    if (border_hit(row[j], dc, ci, cl[j])) mx = fmax(mx, border_value(ri, rho[j]));
  mx = row_reduce(mx, MaxOp{}, part);
  if (threadIdx.x == 0) out[i] = mx;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct WsLayout {
  size_t own, own_tiles, cross_tiles, total;
  long long max_own_tiles;
};

WsLayout ws_layout(int H, long long n_total) {
  WsLayout w;
  w.max_own_tiles = (long long)H + n_total / kDistThreads + 1;
  w.own = 0;
  w.own_tiles = align_up((size_t)(n_total > 0 ? n_total : 1) * sizeof(double), 16);
  w.cross_tiles = w.own_tiles + align_up((size_t)w.max_own_tiles * sizeof(int2), 16);
  w.total = w.cross_tiles + align_up((size_t)(H > 0 ? H : 1) * sizeof(int4), 16);
  return w;
}

int check_matrix(const double *D, int N, const char *who) {
  if (N < 1) return set_error(VBHEM_ERR_ARG, std::string(who) + ": need N >= 1");
  if (!D) return set_error(VBHEM_ERR_ARG, std::string(who) + ": null matrix");
  return VBHEM_OK;
}

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_ccfd_distance_workspace_bytes(int H, long long n_total) {
  if (H < 0 || n_total < 0 || n_total > INT_MAX) return 0;
  return vbhem::ws_layout(H, n_total).total;
}

int vbhmm_ccfd_distance(const vbhmm_score_hmms_t *m, const void *prepared_dev, const vbhmm_seqs_t *s,
                        const int *seg_offsets_dev, void *workspace_dev, size_t workspace_bytes,
                        double *D_dev, double *rowmin_dev, double *rowmax_dev, void *stream) {
  using namespace vbhem;
  if (!m || !s) return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_distance: null HMM set or sequences");
  int rc = hmmset::check_set(m, "vbhmm_ccfd");
  if (rc == VBHEM_OK) rc = hmmset::check_seqs(m, s);
  if (rc != VBHEM_OK) return rc;
  const int H = m->H, N = s->N;
  if (H == 0) return VBHEM_OK;
  if (!prepared_dev || !seg_offsets_dev || !D_dev || !rowmin_dev || !rowmax_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_distance: null prepared buffer, segment offsets or output");
  const WsLayout w = ws_layout(H, N);
  if (!workspace_dev || workspace_bytes < w.total)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(w.total) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace_dev) % 16)
    return set_error(VBHEM_ERR_ARG, "workspace must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);

  // the tile tables, from the segment offsets
  std::vector<int> seg((size_t)H + 1);
  hipError_t e = hipMemcpyAsync(seg.data(), seg_offsets_dev, seg.size() * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "vbhmm_ccfd_distance (segment offsets)");
  if (seg[0] != 0 || seg[H] != N) return set_error(VBHEM_ERR_ARG, "segment offsets must run from 0 to the sequence count");
  for (int i = 0; i < H; ++i)
    if (seg[i + 1] < seg[i]) return set_error(VBHEM_ERR_ARG, "segment offsets must not decrease");
  std::vector<int2> own_tiles;
  std::vector<int4> cross_tiles;
  for (int i = 0; i < H; ++i)
    for (int n = seg[i]; n < seg[i + 1]; n += kDistThreads) own_tiles.push_back(make_int2(i, n));
  for (int i = 0; i < H;) {
    const int c = seg[i + 1] - seg[i];
    if (c > kDistThreads) {
      cross_tiles.push_back(make_int4(seg[i], c, i, 1));
      ++i;
      continue;
    }
    int last = i + 1;  // consecutive whole segments while the lanes last
    while (last < H && last - i < kDistThreads && seg[last + 1] - seg[i] <= kDistThreads) ++last;
    cross_tiles.push_back(make_int4(seg[i], seg[last] - seg[i], i, last - i));
    i = last;
  }
  if ((long long)own_tiles.size() > w.max_own_tiles || cross_tiles.size() > (size_t)H)
    return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_distance: tile table overflow");
  if ((long long)cross_tiles.size() * H > INT_MAX)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_ccfd: too many (HMM, tile) workgroups; split the HMM set");

  char *ws = static_cast<char *>(workspace_dev);
  DistArgs a{};
  a.H = H; a.d = m->dim; a.diag = m->covmode == VBHEM_COV_DIAG; a.tiles = (int)cross_tiles.size();
  a.L = make_layout(m->KM, m->dim);
  a.blocks = hmmset::blocks(prepared_dev);
  a.offsets = s->offsets; a.seg = seg_offsets_dev; a.x = s->x;
  a.own = reinterpret_cast<double *>(ws + w.own);
  a.own_tiles = reinterpret_cast<const int2 *>(ws + w.own_tiles);
  a.cross_tiles = reinterpret_cast<const int4 *>(ws + w.cross_tiles);
  a.D = D_dev;
  if (!own_tiles.empty())
    e = hipMemcpyAsync(ws + w.own_tiles, own_tiles.data(), own_tiles.size() * sizeof(int2), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(ws + w.cross_tiles, cross_tiles.data(), cross_tiles.size() * sizeof(int4),
                       hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the tables are pageable host memory
  if (e != hipSuccess) return hip_fail(e, "vbhmm_ccfd_distance (tile tables)");

  if (!own_tiles.empty()) {
    e = dispatch(m->KM, m->dim, LaunchOwn{a, (unsigned)own_tiles.size(), st});
    if (e != hipSuccess) return hip_fail(e, "ccfd_own_kernel");
  }
  e = dispatch(m->KM, m->dim, LaunchCross{a, (unsigned)((long long)a.tiles * H), st});
  if (e != hipSuccess) return hip_fail(e, "ccfd_cross_kernel");
  hipLaunchKernelGGL((ccfd_sym_kernel<true>), dim3((unsigned)H), dim3(kRowThreads), 0, st, D_dev, H, rowmin_dev,
                     rowmax_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "ccfd_sym_kernel");
  return VBHEM_OK;
}

int vbhmm_ccfd_rowstats(const double *D_dev, int N, double *rowmin_dev, double *rowmax_dev, void *stream) {
  using namespace vbhem;
  const int rc = check_matrix(D_dev, N, "vbhmm_ccfd_rowstats");
  if (rc != VBHEM_OK) return rc;
  if (!rowmin_dev || !rowmax_dev) return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_rowstats: null output");
  hipLaunchKernelGGL((ccfd_sym_kernel<false>), dim3((unsigned)N), dim3(kRowThreads), 0,
                     static_cast<hipStream_t>(stream), const_cast<double *>(D_dev), N, rowmin_dev, rowmax_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VBHEM_OK : hip_fail(e, "ccfd_sym_kernel(stats)");
}

int vbhmm_ccfd_rho(const double *D_dev, int N, const double *dc, int C, int *rho_out_dev, void *stream) {
  using namespace vbhem;
  const int rc = check_matrix(D_dev, N, "vbhmm_ccfd_rho");
  if (rc != VBHEM_OK) return rc;
  if (!dc || C < 1 || C > kMaxCut || !rho_out_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_rho: need 1 to 3 cut-offs and an output");
  CutArgs cut{};
  for (int c = 0; c < C; ++c) cut.dc[c] = dc[c];
  hipLaunchKernelGGL(ccfd_rho_kernel, dim3((unsigned)N), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream),
                     D_dev, N, cut, C, rho_out_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VBHEM_OK : hip_fail(e, "ccfd_rho_kernel");
}

int vbhmm_ccfd_delta(const double *D_dev, int N, const int *rank_dev, int C, double maxd, double *delta_out_dev,
                     int *nneigh_out_dev, void *stream) {
  using namespace vbhem;
  const int rc = check_matrix(D_dev, N, "vbhmm_ccfd_delta");
  if (rc != VBHEM_OK) return rc;
  if (!rank_dev || C < 1 || C > kMaxCut || !delta_out_dev || !nneigh_out_dev)
    return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_delta: need 1 to 3 rank vectors and the outputs");
  hipLaunchKernelGGL(ccfd_delta_kernel, dim3((unsigned)N), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream),
                     D_dev, N, rank_dev, C, maxd, delta_out_dev, nneigh_out_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VBHEM_OK : hip_fail(e, "ccfd_delta_kernel");
}

int vbhmm_ccfd_border(const double *D_dev, int N, double dc, const int *cl_dev, const int *rho_dev,
                      double *rowmax_out_dev, void *stream) {
  using namespace vbhem;
  const int rc = check_matrix(D_dev, N, "vbhmm_ccfd_border");
  if (rc != VBHEM_OK) return rc;
  if (!cl_dev || !rho_dev || !rowmax_out_dev) return set_error(VBHEM_ERR_ARG, "vbhmm_ccfd_border: null array");
  hipLaunchKernelGGL(ccfd_border_kernel, dim3((unsigned)N), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream),
                     D_dev, N, dc, cl_dev, rho_dev, rowmax_out_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VBHEM_OK : hip_fail(e, "ccfd_border_kernel");
}

}  // extern "C"
