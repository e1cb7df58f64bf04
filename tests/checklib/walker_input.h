// tests/checklib/walker_input.h -- TEST-ONLY: the seeded inputs the stand-alone walker
// programs share (tests/*check/walker_main.cpp; plain C++, no device compiler).
#pragma once
#include <cmath>
#include <cstddef>

namespace walker {

struct Lcg {
  unsigned long long s;
  double uni() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) / 9007199254740992.0;
  }
  double normal() { return std::sqrt(-2.0 * std::log(uni() + 1e-300)) * std::cos(6.283185307179586 * uni()); }
};

// rows observations [rows][dim] from two clusters (150 and 210, + 10 per coordinate,
// sigma 20)
inline void two_cluster_draw(Lcg &g, double *x, int rows, int dim) {
  for (int p = 0; p < rows; ++p) {
    const int z = g.uni() < 0.5;
    for (int a = 0; a < dim; ++a) x[(size_t)p * dim + a] = (z ? 150.0 : 210.0) + 10.0 * a + 20.0 * g.normal();
  }
}

// the hyperparameters of the walker cases (H = emrun::Hyper); diag: W0inv is
// 1000 / (1 + a) instead of 1000
template <class H>
H test_hyper(int dim, bool diag) {
  H h;
  h.alpha0 = h.epsilon0 = h.beta0 = 1.0;
  h.v0 = dim + 8.0;
  for (int a = 0; a < (int)(sizeof(h.m0) / sizeof(h.m0[0])); ++a) {
    h.m0[a] = 180.0;
    h.W0inv[a] = diag ? 1000.0 / (1 + a) : 1000.0;
  }
  return h;
}

}  // namespace walker
