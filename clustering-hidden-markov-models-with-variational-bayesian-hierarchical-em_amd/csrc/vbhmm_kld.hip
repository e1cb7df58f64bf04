// vbhmm_kld.hip -- KL jobs over gathered sequence lists (include/vbhmm_kld.h):
// ccfd_cross_kernel's scheme (vbhmm_ccfd.hip) for arbitrary (a, b, list) jobs.
//
//   kld_own_kernel    a workgroup per (HMM a, piece of at most 128 slots of one of its
//                     own-table runs), block a staged in LDS; own[slot] = ll_a(n) / T_n of
//                     the slot's sequence.  One run per unique (a, list) of the jobs.
//   kld_cross_kernel  a workgroup per tile, block b of the tile in LDS, one lane per
//                     (job, item).  One lane per job first spreads the job's own slots
//                     over its lanes in LDS (lane q of a job reads slot job_run + q, whose
//                     sequence own_seq names).  Every lane leaves its term
//                     own[slot] - ll_b(n) / T_n in LDS; after the barrier one lane per
//                     job adds that job's terms one after the other, in list order, from
//                     0.  A tile is either
//                     consecutive whole jobs of one b with at most 128 lanes in all, or
//                     one longer job alone, taken in passes of 128 with lane 0 carrying
//                     the sum on.  So a job's value is the same chain of additions
//                     wherever the job lies and whatever it is packed with.
// The tables come from the host planner (vbhmm_kld_plan.h), which also checks every
// index before anything is uploaded: the kernels index with nothing else.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_ccfd_row.h"
#include "vbhmm_hmmset.h"
#include "vbhmm_kld.h"
#include "vbhmm_kld_plan.h"
#include "vbhmm_score_pair.h"

namespace vbhem {
namespace {

using namespace score;
using ccfd::kl_term;
using kld::kLanes;

static_assert(sizeof(kld::Tile4) == sizeof(int4), "planner table layouts");

struct KldArgs {
  int d, diag;
  Layout L;
  const double *blocks;
  const int *offsets;
  const double *x;
  double *own;
  const int *own_seq;
  const int4 *own_tiles;    // (HMM a, first slot, slots, 0)
  const int4 *cross_tiles;  // (first lane, lanes, first sorted job, jobs)
  const int *tile_b;
  const int *job_first, *job_out, *job_run;
  double *kl;
};

template <int KB, int DB>
__device__ inline double seq_loglik(const KldArgs &p, const Hmm &m, int n, int &T) {
  const int off = p.offsets[n];
  T = p.offsets[n + 1] - off;
  return pair_loglik<KB, DB>(m, p.x + (size_t)off * p.d, T, p.d);
}

template <int KB, int DB>
__global__ __launch_bounds__(kLanes) void kld_own_kernel(const KldArgs p) {
  __shared__ double sh[BlockLen<KB, DB>::value];
  const int4 t = p.own_tiles[blockIdx.x];
  const double *blk = p.blocks + (size_t)t.x * p.L.stride;
  hmmset::stage_block(sh, blk, p.L.stride, kLanes);
  __syncthreads();
  if ((int)threadIdx.x >= t.z) return;
  const int slot = t.y + threadIdx.x;
  const Hmm m = view(p.L, sh, p.diag != 0);
  int T;
  const double ll = seq_loglik<KB, DB>(p, m, p.own_seq[slot], T);
  p.own[slot] = ll / (double)T;
}

// The <8, 2> bucket sits at a register edge: ccfd_cross_kernel takes 96 VGPRs there (5
// waves per SIMD), and the slot lookup would push this kernel to 97 (4 waves).  Asking
// for 5 keeps it at 96 without scratch; every other bucket has room and asks for nothing.
template <int KB, int DB>
struct CrossWaves {
  static constexpr int value = (KB == 8 && DB == 2) ? 5 : 1;
};

template <int KB, int DB>
__global__ __launch_bounds__(kLanes) __attribute__((amdgpu_waves_per_eu(CrossWaves<KB, DB>::value)))
void kld_cross_kernel(const KldArgs p) {
  __shared__ double sh[BlockLen<KB, DB>::value];
  __shared__ double term[kLanes];
  __shared__ int lslot[kLanes];
  const int tid = threadIdx.x;
  const int4 t = p.cross_tiles[blockIdx.x];
  const int l0 = t.x, cnt = t.y, s0 = t.z, njob = t.w;
  const double *blk = p.blocks + (size_t)p.tile_b[blockIdx.x] * p.L.stride;
  hmmset::stage_block(sh, blk, p.L.stride, kLanes);
  __syncthreads();
  const Hmm m = view(p.L, sh, p.diag != 0);
  if (cnt > kLanes) {  // one long job, in passes; uniform over the workgroup
    const int run = p.job_run[s0];
    double sum = 0.0;
    for (int base = 0; base < cnt; base += kLanes) {
      const int left = cnt - base < kLanes ? cnt - base : kLanes;
      if (tid < left) {
        int T;
        const double ll = seq_loglik<KB, DB>(p, m, p.own_seq[run + base + tid], T);
        term[tid] = kl_term(p.own[run + base + tid], ll, T);
      }
      __syncthreads();
      if (tid == 0)
        for (int q = 0; q < left; ++q) sum += term[q];
      __syncthreads();
    }
    if (tid == 0) p.kl[p.job_out[s0]] = sum / (double)cnt;
    return;
  }
  if (tid < njob) {  // at most kLanes stores in the whole tile
    const int s = s0 + tid, a = p.job_first[s] - l0, b = p.job_first[s + 1] - l0, run = p.job_run[s];
    for (int q = a; q < b; ++q) lslot[q] = run + (q - a);
  }
  __syncthreads();
  if (tid < cnt) {
    int T;
    const double ll = seq_loglik<KB, DB>(p, m, p.own_seq[lslot[tid]], T);
    term[tid] = kl_term(p.own[lslot[tid]], ll, T);  // read again: not kept in a register over the recursion
  }
  __syncthreads();
  if (tid < njob) {
    const int s = s0 + tid, a = p.job_first[s] - l0, b = p.job_first[s + 1] - l0;
    double sum = 0.0;
    for (int q = a; q < b; ++q) sum += term[q];
    p.kl[p.job_out[s]] = sum / (double)(b - a);
  }
}

struct LaunchOwn {
  const KldArgs &a;
  unsigned grid;
  hipStream_t st;
  template <int KB, int DB>
  hipError_t operator()() const {
    hipLaunchKernelGGL((kld_own_kernel<KB, DB>), dim3(grid), dim3(kLanes), 0, st, a);
    return hipGetLastError();
  }
};

struct LaunchCross {
  const KldArgs &a;
  unsigned grid;
  hipStream_t st;
  template <int KB, int DB>
  hipError_t operator()() const {
    hipLaunchKernelGGL((kld_cross_kernel<KB, DB>), dim3(grid), dim3(kLanes), 0, st, a);
    return hipGetLastError();
  }
};

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_kld_jobs_workspace_bytes(int n_lists, const int *list_offsets, int n_jobs, const int *jobs) {
  vbhem::kld::Plan p;
  if (vbhem::kld::make_plan(-1, -1, n_lists, list_offsets, nullptr, n_jobs, jobs, p) != VBHEM_OK) return 0;
  return vbhem::kld::ws_layout(p).total;
}

int vbhmm_kld_jobs(const vbhmm_score_hmms_t *m, const void *prepared_dev, const vbhmm_seqs_t *s, int n_lists,
                   const int *list_offsets, const int *list_items, int n_jobs, const int *jobs, void *workspace_dev,
                   size_t workspace_bytes, double *kl_dev, void *stream) {
  using namespace vbhem;
  if (!m || !s) return set_error(VBHEM_ERR_ARG, "vbhmm_kld_jobs: null HMM set or sequences");
  int rc = hmmset::check_set(m, "vbhmm_kld");
  if (rc == VBHEM_OK) rc = hmmset::check_seqs(m, s);
  if (rc != VBHEM_OK) return rc;
  if (n_jobs > 0 && !list_items) {
    bool any = false;  // a null item array is fine while every list is empty
    if (list_offsets && n_lists > 0) any = list_offsets[n_lists] > list_offsets[0];
    if (any) return set_error(VBHEM_ERR_ARG, "vbhmm_kld_jobs: null list items");
  }
  static const int no_items[1] = {0};
  kld::Plan plan;
  rc = kld::make_plan(m->H, s->N, n_lists, list_offsets, list_items ? list_items : no_items, n_jobs, jobs, plan);
  if (rc != VBHEM_OK) return set_error(rc, plan.error);
  if (n_jobs == 0) return VBHEM_OK;
  if (!prepared_dev || !kl_dev) return set_error(VBHEM_ERR_ARG, "vbhmm_kld_jobs: null prepared buffer or output");
  const kld::WsLayout w = kld::ws_layout(plan);
  if (!workspace_dev || workspace_bytes < w.total)
    return set_error(VBHEM_ERR_WORKSPACE, "workspace too small: need " + std::to_string(w.total) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace_dev) % 16)
    return set_error(VBHEM_ERR_ARG, "workspace must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);

  char *ws = static_cast<char *>(workspace_dev);
  const std::vector<char> tables = kld::pack_tables(plan, w);
  hipError_t e = hipMemcpyAsync(ws + w.tables, tables.data(), tables.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the tables are pageable host memory
  if (e != hipSuccess) return hip_fail(e, "vbhmm_kld_jobs (tables)");

  KldArgs a{};
  a.d = m->dim; a.diag = m->covmode == VBHEM_COV_DIAG;
  a.L = score::make_layout(m->KM, m->dim);
  a.blocks = hmmset::blocks(prepared_dev);
  a.offsets = s->offsets; a.x = s->x;
  a.own = reinterpret_cast<double *>(ws + w.own);
  a.own_seq = reinterpret_cast<const int *>(ws + w.own_seq);
  a.own_tiles = reinterpret_cast<const int4 *>(ws + w.own_tiles);
  a.cross_tiles = reinterpret_cast<const int4 *>(ws + w.cross_tiles);
  a.tile_b = reinterpret_cast<const int *>(ws + w.tile_b);
  a.job_first = reinterpret_cast<const int *>(ws + w.job_first);
  a.job_out = reinterpret_cast<const int *>(ws + w.job_out);
  a.job_run = reinterpret_cast<const int *>(ws + w.job_run);
  a.kl = kl_dev;
  if (!plan.own_tiles.empty()) {
    e = score::dispatch(m->KM, m->dim, LaunchOwn{a, (unsigned)plan.own_tiles.size(), st});
    if (e != hipSuccess) return hip_fail(e, "kld_own_kernel");
  }
  e = score::dispatch(m->KM, m->dim, LaunchCross{a, (unsigned)plan.cross_tiles.size(), st});
  if (e != hipSuccess) return hip_fail(e, "kld_cross_kernel");
  return VBHEM_OK;
}

}  // extern "C"
