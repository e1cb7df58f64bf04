// vbhmm_ppk.hip -- the probability product kernel between point HMMs
// (include/vbhmm_ppk.h): the Gram matrix that src/compare_mtds/ppk/ppk_sc.m:17-22
// fills with a double loop over elkernel.m, for every pair of two HMM sets.
//
// hmm_ppk_gram_kernel: a workgroup of 256 lanes owns a tile of TS row HMMs x TS
// column HMMs, whose prepared blocks it stages in LDS once.  KB x KB lanes own the
// state pairs of one HMM pair (state buckets KB = 4 / 8 / 16, dimension buckets
// DB = 2 / 4 / 8 as template parameters): 16, 4 or 1 HMM pairs are in flight per
// workgroup.  Each lane does the Cholesky of its C1 + C2 in registers (every loop
// unrolled, nothing indexed dynamically) and keeps its pot entry and its columns of
// A^rho and B^rho; the two small products of a recursion step go through two LDS
// panels with a barrier after each.
// The grid is (row tiles x column tiles), linearised; in the symmetric mode the
// workgroups below the diagonal leave at once and the pairs i > j of a diagonal tile
// are skipped, every value being stored to out[i][j] and out[j][i].  The mode is a
// run-time argument, so all three modes run the same instructions per pair.  The
// arithmetic is vbhmm_ppk_pair.h, shared with the host check build.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>

#include "vbhem_estep.h"
#include "vbhem_internal.h"
#include "vbhmm_hmmset.h"
#include "vbhmm_ppk.h"
#include "vbhmm_ppk_pair.h"

namespace vbhem {
namespace {

using namespace ppk;

constexpr int kGramThreads = 256;
constexpr int kPrepThreads = 128;

// HMMs per tile side: 4, or 2 where eight of the largest blocks would not leave LDS
// for more than two workgroups per CU
template <int KB, int DB>
struct Tile {
  static constexpr int side = (KB == 16 && DB == 8) ? 2 : 4;
};

struct PrepArgs {
  hmmset::Dims n;
  double rho, pad;
  Layout L;
  hmmset::Arrays a;
};

template <int DB>
__global__ __launch_bounds__(kPrepThreads) void hmm_ppk_prep_kernel(const PrepArgs p) {
  hmmset::prep_lane(p.n, p.L.stride, p.a, kPrepThreads, [&](const hmmset::State &s) {
    return prepare_state<DB>(p.L, s.blk, s.k, s.K, p.n.d, p.n.diag != 0, p.rho, p.pad, s.prior, s.trans, s.mean,
                             s.cov);
  });
}

struct GramArgs {
  int Ha, Hb, d, T, mode, tiles_a, tiles_b;
  Layout La, Lb;
  const double *blocks_a, *blocks_b;
  double *out;
};

template <int KB, int DB>
__global__ __launch_bounds__(kGramThreads) void hmm_ppk_gram_kernel(const GramArgs p) {
  constexpr int TS = Tile<KB, DB>::side, BL = BlockLen<KB, DB>::value;
  constexpr int LP = KB * KB, PP = kGramThreads / LP;  // lanes per HMM pair, pairs in flight
  __shared__ double shA[TS * BL], shB[TS * BL], shX[kGramThreads], shY[kGramThreads];
  const int ta = blockIdx.x / p.tiles_b, tb = p.mode == VBHMM_PPK_DIAG ? ta : blockIdx.x % p.tiles_b;
  if (p.mode == VBHMM_PPK_SYM && ta > tb) return;
  const int a0 = ta * TS, b0 = tb * TS, tid = threadIdx.x;
  for (int q = tid; q < TS * p.La.stride; q += kGramThreads) {
    const int s = q / p.La.stride, r = q % p.La.stride;
    if (a0 + s < p.Ha) shA[s * BL + r] = p.blocks_a[(size_t)(a0 + s) * p.La.stride + r];
  }
  for (int q = tid; q < TS * p.Lb.stride; q += kGramThreads) {
    const int s = q / p.Lb.stride, r = q % p.Lb.stride;
    if (b0 + s < p.Hb) shB[s * BL + r] = p.blocks_b[(size_t)(b0 + s) * p.Lb.stride + r];
  }
  __syncthreads();
  const int slot = tid / LP, e = tid % LP, i = e / KB, j = e % KB;
  double *X = shX + slot * LP, *Y = shY + slot * LP;
  const int np = p.mode == VBHMM_PPK_DIAG ? TS : TS * TS, T = p.T;
  for (int base = 0; base < np; base += PP) {  // uniform: every lane meets every barrier
    const int q = base + slot;
    const int sa = p.mode == VBHMM_PPK_DIAG ? q : q / TS, sb = p.mode == VBHMM_PPK_DIAG ? q : q % TS;
    const int ga = a0 + sa, gb = b0 + sb;
    const bool valid = q < np && ga < p.Ha && gb < p.Hb && !(p.mode == VBHMM_PPK_SYM && ga > gb);
    Hmm A{}, B{};
    bool act = false;
    double pot = 0.0;
    if (valid) {
      A = view(p.La, shA + sa * BL);
      B = view(p.Lb, shB + sb * BL);
      act = i < A.K && j < B.K;
    }
    double ac[KB], bc[KB];  // column i of A^rho, column j of B^rho: fixed over the T steps
    if (act) pot = state_pot<DB>(A, i, B, j, p.d);
    load_col<KB>(A, i, act && T > 1, ac);
    load_col<KB>(B, j, act && T > 1, bc);
    // lanes past the state counts keep zeros in the panels, so the products need no guard
    X[e] = act ? (T == 1 ? A.prior[i] * B.prior[j] : A.prho[i] * B.prho[j]) * pot : 0.0;
    Y[e] = 0.0;
    __syncthreads();
    for (int t = 0; t < T && T > 1; ++t) {
      if (act) Y[e] = dot_col<KB>(ac, X + j, KB);
      __syncthreads();
      if (act) X[e] = dot_col<KB>(bc, Y + i * KB, 1) * pot;
      __syncthreads();
    }
    if (act && j == 0) Y[i] = row_sum(X, KB, i, B.K);
    __syncthreads();
    if (valid && e == 0) {
      const double v = row_sum(Y, 0, 0, A.K);
      if (p.mode == VBHMM_PPK_DIAG) {
        p.out[ga] = v;
      } else {
        p.out[(size_t)ga * p.Hb + gb] = v;
        if (p.mode == VBHMM_PPK_SYM) p.out[(size_t)gb * p.Hb + ga] = v;
      }
    }
    __syncthreads();
  }
}

struct LaunchGram {
  GramArgs a;
  hipStream_t st;
  template <int KB, int DB>
  hipError_t operator()() {
    constexpr int TS = Tile<KB, DB>::side;
    static_assert(kGramThreads % (KB * KB) == 0, "state-pair lanes");
    static_assert((2 * TS * BlockLen<KB, DB>::value + 2 * kGramThreads) * sizeof(double) <= 65536, "LDS");
    a.tiles_a = (a.Ha + TS - 1) / TS;
    a.tiles_b = a.mode == VBHMM_PPK_DIAG ? 1 : (a.Hb + TS - 1) / TS;
    const long long grid = (long long)a.tiles_a * a.tiles_b;
    if (grid > INT_MAX) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((hmm_ppk_gram_kernel<KB, DB>), dim3((unsigned)grid), dim3(kGramThreads), 0, st, a);
    return hipGetLastError();
  }
};

}  // namespace
}  // namespace vbhem

extern "C" {

size_t vbhmm_ppk_prepared_bytes(const vbhmm_score_hmms_t *m) {
  using namespace vbhem;
  return hmmset::prepared_bytes(m, [](int KM, int d) { return make_layout(KM, d).stride; });
}

int vbhmm_ppk_prepare(const vbhmm_score_hmms_t *m, double rho, double pad, void *prepared_dev,
                      size_t prepared_bytes, void *stream) {
  using namespace vbhem;
  const int rc = hmmset::check_set(m, "vbhmm_ppk");
  if (rc != VBHEM_OK) return rc;
  if (!(rho > 0.0) || !(pad >= 0.0) || std::isinf(rho) || std::isinf(pad))
    return set_error(VBHEM_ERR_ARG, "vbhmm_ppk: need a finite rho > 0 and pad >= 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  return hmmset::prepare(
      m, prepared_dev, prepared_bytes, vbhmm_ppk_prepared_bytes(m), st, "hmm_ppk_prep_kernel",
      "regularised covariance", [&](const hmmset::Dims &n, const hmmset::Arrays &arrays) {
        const PrepArgs a{n, rho, pad, make_layout(n.KM, n.d), arrays};
        const dim3 grid(hmmset::prep_grid(n, kPrepThreads)), block(kPrepThreads);
        switch (a.L.DB) {
          case 2: hipLaunchKernelGGL(hmm_ppk_prep_kernel<2>, grid, block, 0, st, a); break;
          case 4: hipLaunchKernelGGL(hmm_ppk_prep_kernel<4>, grid, block, 0, st, a); break;
          default: hipLaunchKernelGGL(hmm_ppk_prep_kernel<8>, grid, block, 0, st, a); break;
        }
      });
}

int vbhmm_ppk_gram(const vbhmm_score_hmms_t *ma, const void *prepared_a, const vbhmm_score_hmms_t *mb,
                   const void *prepared_b, int T, int mode, double *out_dev, void *stream) {
  using namespace vbhem;
  int rc = hmmset::check_set(ma, "vbhmm_ppk");
  if (rc == VBHEM_OK) rc = hmmset::check_set(mb, "vbhmm_ppk");
  if (rc != VBHEM_OK) return rc;
  if (ma->dim != mb->dim) return set_error(VBHEM_ERR_ARG, "vbhmm_ppk_gram: the two sets differ in dimension");
  if (T < 1) return set_error(VBHEM_ERR_ARG, "vbhmm_ppk_gram: T must be >= 1");
  if (mode != VBHMM_PPK_RECT && mode != VBHMM_PPK_SYM && mode != VBHMM_PPK_DIAG)
    return set_error(VBHEM_ERR_ARG, "vbhmm_ppk_gram: unknown mode");
  if (mode != VBHMM_PPK_RECT && ma->H != mb->H)
    return set_error(VBHEM_ERR_ARG, "vbhmm_ppk_gram: the symmetric and diagonal modes need sets of one size");
  if (mode == VBHMM_PPK_SYM && (prepared_a != prepared_b || ma->KM != mb->KM))
    return set_error(VBHEM_ERR_ARG, "vbhmm_ppk_gram: the symmetric mode needs one set on both sides");
  if (ma->H == 0 || mb->H == 0) return VBHEM_OK;
  if (!prepared_a || !prepared_b || !out_dev) return set_error(VBHEM_ERR_ARG, "null prepared buffer or output");
  GramArgs a{};
  a.Ha = ma->H; a.Hb = mb->H; a.d = ma->dim; a.T = T; a.mode = mode;
  a.La = make_layout(ma->KM, ma->dim);
  a.Lb = make_layout(mb->KM, mb->dim);
  a.blocks_a = hmmset::blocks(prepared_a);
  a.blocks_b = hmmset::blocks(prepared_b);
  a.out = out_dev;
  const int KM = ma->KM > mb->KM ? ma->KM : mb->KM;
  const hipError_t e = dispatch(KM, ma->dim, LaunchGram{a, static_cast<hipStream_t>(stream)});
  if (e == hipErrorInvalidConfiguration)
    return set_error(VBHEM_ERR_UNSUPPORTED, "vbhmm_ppk_gram: too many tiles of HMM pairs; split the sets");
  if (e != hipSuccess) return hip_fail(e, "hmm_ppk_gram_kernel");
  return VBHEM_OK;
}

}  // extern "C"
