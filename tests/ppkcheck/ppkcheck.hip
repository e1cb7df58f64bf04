// tests/ppkcheck/ppkcheck.hip -- TEST-ONLY exports of the probability product kernel
// arithmetic (csrc/vbhmm_ppk_pair.h): a host loop over HMM pairs calling the
// routines the kernels call, so the logic is checked on a machine without a GPU,
// and the same call through the library's kernels on device 0.  Arrays are host
// arrays in the layouts of include/vbhmm_score.h; the sets a and b share the
// dimension and the covariance mode.  out: [Ha][Hb] (modes 0, 1) or [Ha] (mode 2).
#include <hip/hip_runtime.h>

#include <vector>

#include "device_pool.h"
#include "vbhmm_ppk.h"
#include "vbhmm_ppk_pair.h"

namespace {

using namespace vbhem::ppk;

struct Set {
  int H, KM;
  const int *nstates;
  const double *prior, *trans, *mean, *cov;
};

struct HostPrep {
  const Set &s;
  int d;
  bool diag;
  double rho, pad;
  const Layout &L;
  std::vector<double> &blocks;
  template <int KB, int DB>
  long long operator()() const {
    const size_t cs = diag ? (size_t)d : (size_t)d * d;
    long long bad = 0;
    for (int h = 0; h < s.H; ++h)
      for (int k = 0; k < s.KM; ++k)
        if (!prepare_state<DB>(L, blocks.data() + (size_t)h * L.stride, k, s.nstates[h], d, diag, rho, pad,
                               s.prior + (size_t)h * s.KM, s.trans + (size_t)h * s.KM * s.KM,
                               s.mean + (size_t)h * s.KM * d, s.cov + (size_t)h * s.KM * cs) &&
            !bad)
          bad = 1 + (long long)h * s.KM + k;
    return bad;
  }
};

struct HostGram {
  const Layout &La, &Lb;
  const std::vector<double> &ba, &bb;
  int Ha, Hb, d, T, mode;
  double *out;
  template <int KB, int DB>
  long long operator()() const {
    for (int i = 0; i < Ha; ++i)
      for (int j = 0; j < Hb; ++j) {
        if ((mode == VBHMM_PPK_DIAG && i != j) || (mode == VBHMM_PPK_SYM && i > j)) continue;
        const double v = pair_kernel<KB, DB>(view(La, ba.data() + (size_t)i * La.stride),
                                             view(Lb, bb.data() + (size_t)j * Lb.stride), d, T);
        if (mode == VBHMM_PPK_DIAG) {
          out[i] = v;
        } else {
          out[(size_t)i * Hb + j] = v;
          if (mode == VBHMM_PPK_SYM) out[(size_t)j * Hb + i] = v;
        }
      }
    return 0;
  }
};

struct DevSet {
  vbhmm_score_hmms_t m{};
  void *prep = nullptr;
  size_t pb = 0;
};

DevSet upload(const Set &s, int d, int covmode, checklib::Pool &pool) {
  const size_t cs = covmode == VBHEM_COV_DIAG ? (size_t)d : (size_t)d * d;
  DevSet v;
  v.m = {s.H, s.KM, d, covmode,
         static_cast<const int *>(pool.put(s.nstates, (size_t)s.H * sizeof(int))),
         static_cast<const double *>(pool.put(s.prior, (size_t)s.H * s.KM * 8)),
         static_cast<const double *>(pool.put(s.trans, (size_t)s.H * s.KM * s.KM * 8)),
         static_cast<const double *>(pool.put(s.mean, (size_t)s.H * s.KM * d * 8)),
         static_cast<const double *>(pool.put(s.cov, (size_t)s.H * s.KM * cs * 8))};
  v.pb = vbhmm_ppk_prepared_bytes(&v.m);
  v.prep = pool.put(nullptr, v.pb);
  return v;
}

}  // namespace

extern "C" {

// 0, or 1 + (h KM + k) of the first regularised covariance of set a that is not
// positive definite, or -(1 + ...) of set b.
long long ppkcheck_host(int d, int covmode, double rho, double pad, int T, int mode, int Ha, int KMa,
                        const int *nstates_a, const double *prior_a, const double *trans_a,
                        const double *mean_a, const double *cov_a, int Hb, int KMb, const int *nstates_b,
                        const double *prior_b, const double *trans_b, const double *mean_b,
                        const double *cov_b, double *out) {
  const Set sa{Ha, KMa, nstates_a, prior_a, trans_a, mean_a, cov_a};
  const Set sb{Hb, KMb, nstates_b, prior_b, trans_b, mean_b, cov_b};
  const Layout La = make_layout(KMa, d), Lb = make_layout(KMb, d);
  const bool diag = covmode == VBHEM_COV_DIAG;
  std::vector<double> ba((size_t)Ha * La.stride, 0.0), bb((size_t)Hb * Lb.stride, 0.0);
  long long bad = dispatch(KMa, d, HostPrep{sa, d, diag, rho, pad, La, ba});
  if (bad) return bad;
  bad = dispatch(KMb, d, HostPrep{sb, d, diag, rho, pad, Lb, bb});
  if (bad) return -bad;
  return dispatch(KMa > KMb ? KMa : KMb, d, HostGram{La, Lb, ba, bb, Ha, Hb, d, T, mode, out});
}

// The same through vbhmm_ppk_prepare / vbhmm_ppk_gram on device 0 (mode 1: set a on
// both sides).  Returns the library's status, or a positive hipError_t of the copies.
int ppkcheck_device(int d, int covmode, double rho, double pad, int T, int mode, int Ha, int KMa,
                    const int *nstates_a, const double *prior_a, const double *trans_a,
                    const double *mean_a, const double *cov_a, int Hb, int KMb, const int *nstates_b,
                    const double *prior_b, const double *trans_b, const double *mean_b,
                    const double *cov_b, double *out) {
  const Set sa{Ha, KMa, nstates_a, prior_a, trans_a, mean_a, cov_a};
  const Set sb{Hb, KMb, nstates_b, prior_b, trans_b, mean_b, cov_b};
  const bool sym = mode == VBHMM_PPK_SYM;
  const size_t out_bytes = (mode == VBHMM_PPK_DIAG ? (size_t)Ha : (size_t)Ha * Hb) * 8;
  checklib::Pool pool;
  const DevSet da = upload(sa, d, covmode, pool), db = sym ? da : upload(sb, d, covmode, pool);
  double *dout = static_cast<double *>(pool.put(nullptr, out_bytes));
  if (pool.e != hipSuccess) return (int)pool.e;
  int rc = vbhmm_ppk_prepare(&da.m, rho, pad, da.prep, da.pb, nullptr);
  if (rc == 0 && !sym) rc = vbhmm_ppk_prepare(&db.m, rho, pad, db.prep, db.pb, nullptr);
  if (rc == 0) rc = vbhmm_ppk_gram(&da.m, da.prep, &db.m, db.prep, T, mode, dout, nullptr);
  if (rc != 0) return rc;
  pool.e = hipDeviceSynchronize();
  pool.get(out, dout, out_bytes);
  return (int)pool.e;
}

}  // extern "C"
