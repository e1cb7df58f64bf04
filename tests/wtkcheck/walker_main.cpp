// tests/wtkcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the serial walkers of
// csrc/vbhem_wtk_run.h on seeded inputs, for a run under the address and undefined-behaviour
// sanitizers on the CPU (`make wtk_sanitize`; plain C++, no device compiler).  It walks the
// two stages at the demo's size, at the limits d = 16, K = 32, S = 16, at n = K (singleton
// clusters: Inf and NaN in the sweep), with zero weights, a degenerate trial (fewer
// distinct points than centres), a non-finite coordinate and an out-of-range draw.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vbhem_wtk_run.h"
#include "walker_input.h"

using namespace vbhem::wtkrun;
using walker::Lcg;

namespace {

// mode 0: ordinary; 1: every point the same (degenerate); 2: a NaN coordinate; 3: j0 = n;
// 4: every second weight zero
int one_case(int n, int d, int K, int S, unsigned long long seed, int mode) {
  Lcg g{seed};
  std::vector<double> X((size_t)n * d), w(n);
  for (int m = 0; m < n; ++m) {
    const int z = (int)(g.uni() * K);
    for (int a = 0; a < d; ++a) X[(size_t)m * d + a] = mode == 1 ? 3.0 : 40.0 * z + 7.0 * a + 5.0 * g.uni();
    w[m] = mode == 4 && (m & 1) ? 0.0 : 0.5 + g.uni();
  }
  if (mode == 2) X[(size_t)(n / 2) * d] = NAN;
  std::vector<double> u(K > 1 ? K - 1 : 1), us(S > 1 ? S - 1 : 1);
  for (double &v : u) v = g.uni();
  for (double &v : us) v = g.uni();
  const int kk = K > S ? K : S;
  std::vector<double> cen((size_t)kk * d), cold((size_t)kk * d), sums((size_t)kk * (d + 1)), cw(kk), dw(n),
      out((size_t)S * d, -1.0);
  std::vector<int> lw(n), labels(n, -7), counts(K, -7), idx(n);
  int iters[2] = {-7, -7};
  const int j0 = mode == 3 ? n : (int)(g.uni() * n);
  const int st = cluster_trial_serial(X.data(), w.data(), n, d, K, j0, u.data(), cen.data(), cold.data(), sums.data(),
                                      cw.data(), dw.data(), lw.data(), labels.data(), counts.data(), iters);
  std::printf("n=%d d=%d K=%d S=%d mode=%d: status=%d iters=%d,%d\n", n, d, K, S, mode, st, iters[0], iters[1]);
  if (mode == 1) return !(st == (K > 1 ? kDegenerate : kOk) && (K == 1 || labels[0] == -7));
  if (mode == 2 || mode == 3) return !(st == kBad && labels[0] == -7 && counts[0] == -7 && iters[0] == -7);
  if (st != kOk) return 1;
  int bad = 0, total = 0;
  for (int c = 0; c < K; ++c) total += counts[c];
  bad += total != n;
  for (int c = 0; c < K; ++c) {
    if (counts[c] <= S) continue;
    int it = -7;
    const int s2 = states_item_serial(X.data(), n, d, labels.data(), c, counts[c], S, (int)(g.uni() * counts[c]),
                                      us.data(), idx.data(), cen.data(), cold.data(), sums.data(), dw.data(), lw.data(),
                                      out.data(), &it);
    bad += !(s2 == kOk || s2 == kDegenerate);
    bad += s2 == kOk && !(it >= 1 && std::isfinite(out[0]));
    // a wrong member count is refused
    bad += states_item_serial(X.data(), n, d, labels.data(), c, counts[c] - 1, S, 0, us.data(), idx.data(), cen.data(),
                              cold.data(), sums.data(), dw.data(), lw.data(), out.data(), &it) != kBad;
  }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  bad += one_case(30, 2, 3, 3, 1, 0);
  bad += one_case(255, 3, 2, 1, 2, 0);
  bad += one_case(513, 8, 16, 3, 3, 0);
  bad += one_case(2000, 16, 32, 16, 4, 0);
  bad += one_case(16, 2, 16, 3, 5, 0);
  bad += one_case(300, 2, 1, 3, 6, 0);
  bad += one_case(300, 2, 4, 3, 7, 4);
  bad += one_case(40, 2, 3, 3, 8, 1);
  bad += one_case(40, 2, 3, 3, 9, 2);
  bad += one_case(40, 2, 3, 3, 10, 3);
  std::printf(bad ? "FAILED %d\n" : "walker OK\n", bad);
  return bad != 0;
}
