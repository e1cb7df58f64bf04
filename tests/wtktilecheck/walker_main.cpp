// tests/wtktilecheck/walker_main.cpp -- TEST-ONLY stand-alone program: the serial tiled
// walker of csrc/vbhem_wtk_tiled_run.h on seeded inputs, for a run under the address and
// undefined-behaviour sanitizers on the CPU (`make wtktile_sanitize`; plain C++, no device
// compiler).  It walks both entries (the first stage of 'wtkmeans', kmeans_pp alone) at the
// demo's size, at the edges of a tile (255, 256, 257, 513 points), at the limits d = 16,
// K = 32, at n = K, past the tile-size switch (1,024-point tiles, a last tile of one
// point), with zero weights, a degenerate trial, a non-finite coordinate and an
// out-of-range draw, and compares the discrete outputs with the block schedule's walker.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vbhem_wtk_tiled_run.h"
#include "walker_input.h"

using namespace vbhem::wtktile;
using walker::Lcg;

namespace {

// mode 0: ordinary; 1: every point the same (degenerate); 2: a NaN coordinate; 3: j0 = n;
// 4: every second weight zero
int one_case(int n, int d, int K, unsigned long long seed, int mode) {
  Lcg g{seed};
  std::vector<double> X((size_t)n * d), w(n);
  for (int m = 0; m < n; ++m) {
    const int z = (int)(g.uni() * K);
    for (int a = 0; a < d; ++a) X[(size_t)m * d + a] = mode == 1 ? 3.0 : 40.0 * z + 7.0 * a + 5.0 * g.uni();
    w[m] = mode == 4 && (m & 1) ? 0.0 : 0.5 + g.uni();
  }
  if (mode == 2) X[(size_t)(n / 2) * d] = NAN;
  std::vector<double> u(K > 1 ? K - 1 : 1);
  for (double &v : u) v = g.uni();
  const int j0 = mode == 3 ? n : (int)(g.uni() * n);
  std::vector<double> rec(rec_len(K, d)), part((size_t)tiles_of(n, d) * part_len(K, d)), tot(part_len(K, d)), dw(n),
      cen((size_t)K * d, -1.0), cold((size_t)K * d), sums((size_t)K * (d + 1)), cw(K);
  std::vector<int> lw(n), labels(n, -7), counts(K, -7), blab(n, -7), bcnt(K, -7);
  int iters[2] = {-7, -7}, bit[2] = {-7, -7};
  const WalkOut o = tiled_trial_serial(X.data(), w.data(), n, d, K, j0, u.data(), false, rec.data(), part.data(),
                                       tot.data(), dw.data(), lw.data(), labels.data(), counts.data(), nullptr, iters);
  std::printf("n=%d d=%d K=%d mode=%d: status=%d reseed=%d rounds=%d iters=%d,%d\n", n, d, K, mode, o.status, o.reseed,
              o.rounds, iters[0], iters[1]);
  if (mode == 1) return !(o.status == (K > 1 ? kDegenerate : kOk) && (K == 1 || labels[0] == -7));
  if (mode == 2 || mode == 3) return !(o.status == kBad && labels[0] == -7 && counts[0] == -7 && iters[0] == -7);
  if (o.status != kOk) return 1;
  if (o.reseed) return 0;  // the block schedule's trial
  int bad = 0, total = 0;
  for (int c = 0; c < K; ++c) total += counts[c];
  bad += total != n || o.rounds > rounds_of(K, false);
  // the block schedule's walker: equal discrete outputs on these well-separated inputs
  const int bs = cluster_trial_serial(X.data(), w.data(), n, d, K, j0, u.data(), cen.data(), cold.data(), sums.data(),
                                      cw.data(), dw.data(), lw.data(), blab.data(), bcnt.data(), bit);
  bad += bs != kOk || bit[0] != iters[0] || bit[1] != iters[1] || blab != labels || bcnt != counts;
  // kmeans_pp alone
  if (K >= 2) {
    int it = -7;
    const WalkOut s = tiled_trial_serial(X.data(), nullptr, n, d, K, j0, u.data(), true, rec.data(), part.data(),
                                         tot.data(), dw.data(), lw.data(), nullptr, nullptr, cen.data(), &it);
    bad += !(s.status == kOk && !s.reseed && it == iters[0] && std::isfinite(cen[0]));
    bad += s.rounds > rounds_of(K, true);
  }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  bad += one_case(30, 2, 3, 1, 0);
  bad += one_case(255, 3, 2, 2, 0);
  bad += one_case(256, 2, 3, 11, 0);
  bad += one_case(257, 2, 3, 12, 0);
  bad += one_case(513, 8, 16, 3, 0);
  bad += one_case(2000, 16, 32, 4, 0);
  bad += one_case(16, 2, 16, 5, 0);
  bad += one_case(300, 2, 1, 6, 0);
  bad += one_case(300, 2, 4, 7, 4);
  bad += one_case(262144 + 1025, 2, 2, 13, 0);
  bad += one_case(40, 2, 3, 8, 1);
  bad += one_case(40, 2, 3, 9, 2);
  bad += one_case(40, 2, 3, 10, 3);
  std::printf(bad ? "FAILED %d\n" : "walker OK\n", bad);
  return bad != 0;
}
