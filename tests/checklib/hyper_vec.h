// tests/checklib/hyper_vec.h -- TEST-ONLY: the flat hyperparameter vector of the check
// libraries, [alpha0, epsilon0, beta0, v0, m0[8], W0inv_diag[8]], as the library's struct.
#pragma once
#include "vbhmm_em.h"

namespace checklib {

inline vbhmm_em_hyper_t hyper_struct(const double *hyper) {
  vbhmm_em_hyper_t hy{};
  hy.alpha0 = hyper[0]; hy.epsilon0 = hyper[1]; hy.beta0 = hyper[2]; hy.v0 = hyper[3];
  for (int q = 0; q < 8; ++q) {
    hy.m0[q] = hyper[4 + q];
    hy.W0inv_diag[q] = hyper[12 + q];
  }
  return hy;
}

}  // namespace checklib
