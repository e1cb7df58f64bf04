// tests/checklib/host_prepare.h -- TEST-ONLY: a set of point HMMs (host arrays in the
// layouts of include/vbhmm_score.h) into prepared blocks by a host loop over
// score::prepare_state, the routine hmm_score_prep_kernel calls per state.
#pragma once
#include <vector>

#include "vbhmm_score.h"
#include "vbhmm_score_pair.h"

namespace checklib {

// blocks: [H][L.stride].  0, or 1 + (h KM + k) of the first covariance that is not
// positive definite (the blocks are then unfinished).
inline long long host_prepare(const vbhem::score::Layout &L, int H, int KM, int d, int covmode, const int *nstates,
                              const double *prior, const double *trans, const double *mean, const double *cov,
                              std::vector<double> &blocks) {
  const bool diag = covmode == VBHEM_COV_DIAG;
  const size_t cs = diag ? (size_t)d : (size_t)d * d;
  blocks.assign((size_t)H * L.stride, 0.0);
  for (int h = 0; h < H; ++h)
    for (int k = 0; k < KM; ++k)
      if (!vbhem::score::prepare_state(L, blocks.data() + (size_t)h * L.stride, k, nstates[h], d, diag,
                                       prior + (size_t)h * KM, trans + (size_t)h * KM * KM,
                                       mean + (size_t)h * KM * d, cov + (size_t)h * KM * cs))
        return 1 + (long long)h * KM + k;
  return 0;
}

}  // namespace checklib
