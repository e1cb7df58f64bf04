// tests/vbhmmemcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the serial walker of
// csrc/vbhmm_em_run.h on seeded inputs, for a run under the address and undefined-behaviour
// sanitizers on the CPU (`make vbhmmem_sanitize`; plain C++, no device compiler).  It
// walks every shape class the kernel has: KM = 4 and 8 with K = KM, dim = 1, 2 and 8, 70
// sequences with lengths 1..49 (T = 1 included), 130 short sequences, a single sequence,
// empty sequences (first, last, two adjacent), an unequal W0inv, and an unstable run.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vbhmm_em_run.h"
#include "walker_input.h"

using namespace vbhem::emrun;
using walker::Lcg;

namespace {

// empties: sequences 0, N / 2, N / 2 + 1 and N - 1 have no observation; diag: W0inv is
// 1000 / (1 + a) instead of 1000
template <int KM>
int one_case(int K, int dim, int N, int maxlen, unsigned long long seed, bool break_W, bool empties = false,
             bool diag = false) {
  Lcg g{seed};
  std::vector<int> off(N + 1, 0);
  for (int n = 0; n < N; ++n) {
    const bool none = empties && (n == 0 || n == N / 2 || n == N / 2 + 1 || n == N - 1);
    off[n + 1] = off[n] + (none ? 0 : n == 0 ? 1 : 1 + (int)(g.uni() * maxlen));
  }
  const int obs = off[N];
  std::vector<double> x((size_t)obs * dim);
  walker::two_cluster_draw(g, x.data(), obs, dim);
  const Hyper h = walker::test_hyper<Hyper>(dim, diag);
  const int PL = post_len(KM, dim), SL = stats_len(KM, dim);
  std::vector<double> post(PL, 1.0), est(PL), st(SL), LLs(30, 0.0);
  double *alpha = post.data(), *eps = alpha + KM, *beta = eps + KM * KM, *v = beta + KM, *m = v + KM,
         *W = m + KM * dim;
  for (int k = 0; k < K; ++k) {
    alpha[k] = 1.0 + (double)N / K;
    beta[k] = 1.0 + (double)obs / K;
    v[k] = h.v0 + (double)obs / K + 1;
    for (int j = 0; j < K; ++j) eps[k * KM + j] = 1.0 + (double)N / K;
    for (int a = 0; a < dim; ++a) {
      m[k * dim + a] = 150.0 + 60.0 * k / (K > 1 ? K - 1 : 1) + 10.0 * a;
      for (int b = 0; b < dim; ++b) W[(k * dim + a) * dim + b] = a == b ? 1.0 / (400.0 * v[k]) : 0.0;
    }
  }
  if (break_W) W[0] = -W[0];
  std::vector<double> gm((size_t)obs * KM), lr((size_t)obs * KM), cs(obs), mx(obs), sq((size_t)N * seq_len(KM));
  const Work<KM> w{gm.data(), lr.data(), cs.data(), mx.data(), sq.data()};
  const Subject s{N, off.data(), x.data()};
  const RunResult r = run_serial<KM>(K, dim, s, h, 30, 1e-5, post.data(), est.data(), st.data(), LLs.data(), w);
  std::printf("KM=%d K=%d dim=%d N=%d obs=%d%s%s: LL=%.12g iters=%d status=%d\n", KM, K, dim, N, obs,
              empties ? " empties" : "", diag ? " diag" : "", r.LL, r.iters, r.status);
  if (break_W) return !(r.status == kUnstable && r.iters == 1 && std::isinf(r.LL));
  return !(std::isfinite(r.LL) && r.status != kUnstable && r.iters >= 1);
}

}  // namespace

int main() {
  int bad = 0;
  bad += one_case<4>(1, 2, 70, 49, 1, false);
  bad += one_case<4>(3, 2, 70, 49, 2, false);
  bad += one_case<4>(4, 3, 65, 5, 3, false);
  bad += one_case<8>(5, 2, 64, 5, 4, false);
  bad += one_case<8>(8, 8, 40, 12, 5, false);
  bad += one_case<4>(2, 2, 1, 9, 6, false);
  bad += one_case<4>(2, 2, 30, 5, 7, true);
  bad += one_case<4>(4, 8, 40, 12, 8, false);
  bad += one_case<8>(8, 1, 40, 12, 9, false);
  bad += one_case<4>(3, 2, 130, 3, 10, false);
  bad += one_case<4>(3, 2, 14, 8, 11, false, true);
  bad += one_case<8>(8, 8, 40, 12, 12, false, true, true);
  bad += one_case<4>(3, 2, 30, 5, 13, false, false, true);
  std::printf(bad ? "FAILED %d\n" : "walker OK\n", bad);
  return bad != 0;
}
