// tests/gmmcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the serial walker of
// csrc/vbhmm_gmm_run.h on seeded inputs, for a run under the address and undefined-behaviour
// sanitizers on the CPU (`make gmm_sanitize`; plain C++, no device compiler).  It walks
// every shape class the kernel has: KM = 4 and 8 with K = KM, dim = 1, 2, 3 and 8, N at the
// edges of a round of lanes and N = K + 1, start rows 0 and N - 1, the initial posterior
// (also under an unequal W0inv), a fit that
// stops at max_iter, an ill-conditioned fit with its regularised refit, and bad fits.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vbhmm_gmm_run.h"
#include "walker_input.h"

using namespace vbhem::gmmrun;
using walker::Lcg;

namespace {

// mode 0: an ordinary fit; 1: max_iter = 2; 2: one far point among the start rows (ill-
// conditioned), then the same rows with reg = 1e-10; 3: bad fits; 4: whatever status the
// fit ends with (N = K + 1 collapses onto single points).  diag: W0inv is 1000 / (1 + a)
template <int KM>
int one_case(int K, int dim, int N, unsigned long long seed, int mode, bool diag = false) {
  Lcg g{seed};
  std::vector<double> x((size_t)N * dim);
  walker::two_cluster_draw(g, x.data(), N, dim);
  std::vector<int> rows(KM, 0);
  for (int k = 0; k < K; ++k) rows[k] = k == 0 ? N - 1 : k == 1 ? 0 : (int)((long long)k * N / K);
  if (mode == 2)
    for (int a = 0; a < dim; ++a) x[(size_t)(N - 1) * dim + a] = 1e4;
  const Hyper h = walker::test_hyper<Hyper>(dim, diag);
  const int PL = vbhem::emrun::post_len(KM, dim), max_iter = mode == 1 ? 2 : 100;
  std::vector<double> prior(KM, -1.0), mean(KM * dim, -1.0), cov(KM * dim * dim, -1.0), lls(max_iter, 0.0),
      post(PL, -1.0), wp((size_t)N * KM), wl(N);
  const Work w{wp.data(), wl.data()};
  int bad = 0;
  if (mode == 3) {
    const int far[KM] = {0, N};
    FitResult r = run_serial<KM>(1, dim, N, N, x.data(), rows.data(), 0.0, max_iter, 1e-5, prior.data(), mean.data(),
                                 cov.data(), lls.data(), &h, post.data(), w);
    bad += r.status != kBadFit;
    r = run_serial<KM>(2, dim, 2, N, x.data(), rows.data(), 0.0, max_iter, 1e-5, prior.data(), mean.data(),
                       cov.data(), lls.data(), &h, post.data(), w);
    bad += r.status != kBadFit;
    r = run_serial<KM>(2, dim, N, N, x.data(), far, 0.0, max_iter, 1e-5, prior.data(), mean.data(), cov.data(),
                       lls.data(), &h, post.data(), w);
    bad += r.status != kBadFit || prior[0] != -1.0 || post[0] != -1.0;
    std::printf("KM=%d bad fits: %s\n", KM, bad ? "FAILED" : "refused");
    return bad;
  }
  FitResult r = run_serial<KM>(K, dim, N, N, x.data(), rows.data(), 0.0, max_iter, 1e-5, prior.data(), mean.data(),
                               cov.data(), lls.data(), &h, post.data(), w);
  std::printf("KM=%d K=%d dim=%d N=%d mode=%d: ll=%.12g iters=%d status=%d\n", KM, K, dim, N, mode, r.ll, r.iters,
              r.status);
  if (mode == 1) return !(r.status == kMaxIter && r.iters == 2);
  if (mode == 2) {
    bad += !(r.status == kIllConditioned && prior[0] == -1.0 && post[0] == -1.0);
    r = run_serial<KM>(K, dim, N, N, x.data(), rows.data(), 1e-10, max_iter, 1e-5, prior.data(), mean.data(),
                       cov.data(), lls.data(), &h, post.data(), w);
    std::printf("  reg=1e-10: ll=%.12g iters=%d status=%d\n", r.ll, r.iters, r.status);
    return bad + !(r.status == kConverged && std::isfinite(r.ll));
  }
  if (mode == 4) return 0;
  double sp = 0.0;
  for (int k = 0; k < K; ++k) sp += prior[k];
  return !(std::isfinite(r.ll) && r.status != kIllConditioned && std::fabs(sp - 1.0) < 1e-12 && post[0] > 1.0);
}

}  // namespace

int main() {
  int bad = 0;
  bad += one_case<4>(2, 2, 250, 1, 0);
  bad += one_case<4>(3, 2, 63, 2, 0);
  bad += one_case<4>(4, 3, 64, 3, 0);
  bad += one_case<4>(2, 2, 65, 4, 0);
  bad += one_case<4>(2, 2, 129, 5, 0);
  bad += one_case<4>(3, 2, 4, 6, 4);
  bad += one_case<8>(8, 2, 300, 7, 0);
  bad += one_case<8>(5, 8, 400, 8, 0);
  bad += one_case<4>(2, 2, 250, 9, 1);
  bad += one_case<4>(2, 2, 41, 10, 2);
  bad += one_case<4>(2, 2, 40, 11, 3);
  bad += one_case<8>(2, 2, 40, 12, 3);
  bad += one_case<4>(4, 8, 300, 13, 0);
  bad += one_case<8>(8, 1, 300, 14, 0);
  bad += one_case<8>(8, 8, 600, 15, 0, true);
  bad += one_case<4>(3, 2, 130, 16, 0, true);
  std::printf(bad ? "FAILED %d\n" : "walker OK\n", bad);
  return bad != 0;
}
