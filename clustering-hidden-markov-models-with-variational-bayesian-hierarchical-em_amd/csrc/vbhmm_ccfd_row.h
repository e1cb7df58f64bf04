// vbhmm_ccfd_row.h -- the per-entry decisions of the density-peak passes over a
// distance matrix (include/vbhmm_ccfd.h), written once for the device kernels
// (vbhmm_ccfd.hip) and for a host build (tests/ccfdcheck):
//   rho_hit        the cut-off kernel of CCFD.m:36-43: dist < dc, strict
//   Best / take / merge / finish
//                  the scan of CCFD.m:52-60 as a reduction: among the points ranked
//                  above the row's own, the lexicographic minimum of (dist, rank);
//                  the scan is in rank order with a strict <, so among equal
//                  distances the lowest rank wins, and a neighbour is kept only
//                  below maxd
//   border_hit / border_value
//                  CCFD.m:196-197: another cluster, dist <= dc (not strict), the
//                  pair's mean density
// The combine is associative and commutative (ranks are distinct), so any
// reduction tree gives the sequential scan's answer.
#pragma once
#include <climits>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBC_HD __host__ __device__
#else
#define VBC_HD
#endif

namespace vbhem {
namespace ccfd {

constexpr int kMaxCut = 3;  // cut-offs evaluated in one read of the matrix

VBC_HD inline bool rho_hit(double dist, double dc) { return dist < dc; }

struct Best {
  double d;
  int rank, j;
};

VBC_HD inline Best best_none() {
  Best b;
  b.d = INFINITY;
  b.rank = INT_MAX;
  b.j = -1;
  return b;
}

// does (d, rank) come before b
VBC_HD inline bool best_before(double d, int rank, const Best &b) {
  return d < b.d || (d == b.d && rank < b.rank);
}

// entry (row, j) of the matrix offered to the row's running minimum
VBC_HD inline void best_take(Best &b, double dist, int rank_j, int rank_row, int j) {
  if (rank_j < rank_row && best_before(dist, rank_j, b)) {
    b.d = dist;
    b.rank = rank_j;
    b.j = j;
  }
}

VBC_HD inline void best_merge(Best &b, const Best &o) {
  if (best_before(o.d, o.rank, b)) b = o;
}

// (delta, nneigh) of a row: the top-ranked row keeps CCFD.m:49-50's placeholder
VBC_HD inline void best_finish(const Best &b, int rank_row, double maxd, double &delta, int &nneigh) {
  if (rank_row == 0) {
    delta = -1.0;
    nneigh = -1;
  } else if (b.j >= 0 && b.d < maxd) {
    delta = b.d;
    nneigh = b.j;
  } else {
    delta = maxd;
    nneigh = -1;
  }
}

VBC_HD inline bool border_hit(double dist, double dc, int cl_i, int cl_j) {
  return cl_i != cl_j && dist <= dc;
}

VBC_HD inline double border_value(int rho_i, int rho_j) { return ((double)rho_i + (double)rho_j) / 2.0; }

// one term of KL[i][j]: own = ll_i(n) / T_n already divided, ll = ll_j(n) not yet
VBC_HD inline double kl_term(double own, double ll, int T) { return own - ll / (double)T; }

}  // namespace ccfd
}  // namespace vbhem
