// vbhem_wtk_tiled_run.h -- the TILED schedule of the k-means of the initialisations
// (include/vbhem_init.h: vbhem_wtk_cluster_tiled_batch, vbhem_wtk_seed_tiled_batch): the
// trial's record, the layout of a tile's partials, the rules a round applies, and a serial
// walker of the whole schedule (one lane; any C++ compiler).  The per-point arithmetic is
// vbhem_wtk_run.h's, unchanged (dist2, nearest, wk_assign, wk_member_f, finite_d); only the
// order of the n-term sums differs from the block schedule's.
//
// A trial is a state machine whose record lives in the workspace.  One ROUND is a pass over
// the points in tiles of ghemrun::tile_points(n, d) points, which leaves a row of partials
// per tile, and a STEP that adds the rows in tile order and applies the phase's rule:
//   SEED c (c = 1 .. K-1)  pass: d2 = min(d2, dist2 to centre c-1) (c = 1: the distance to
//       centre 0 = point j0); partial: the tile's sum of d2.  Step: total = 0 (or not
//       finite) ends the trial DEGENERATE; else the target u[c-1] * total is looked up in
//       the running sum over the tiles: the first tile whose inclusive sum exceeds it (none:
//       the last tile) is searched from its exclusive sum, and centre c is the first point
//       whose running sum exceeds the target; a tile that rounding leaves without one hands
//       the pick to the first point of the next tile (the last tile: to point n-1), which is
//       what block_pick's chunks do with each other.
//   LLOYD (pass 1 .. 100)  pass: nearest, the changed-label count (from the second pass on),
//       per cluster the member count and coordinate sums.  Step: from the second pass on a
//       count of zero ends the phase before any update; else an empty cluster sets the
//       trial's RE-SEED flag and ends the tiled run without outputs (the caller hands the
//       trial to the block schedule); else the centres become the means.
//   WEIGHTED s = 0         pass: nearest; per cluster sum w and sum w x.  Step: gcentroids.
//   WEIGHTED s = 1 .. 101  pass: with the labels and centres of sweep s-1: the labels to the
//       output, per cluster the count and the energy (genergy), f; then (s <= 100) wk_assign
//       and the new labels' sum w and sum w x.  Step: E(s-1) = the clusters' energies added
//       in cluster order; |E(s-1) - E(s-2)| < 1e-6 (s >= 2) ends the trial with s-2 sweeps
//       counted, s = 101 with 100; else gcentroids.  The output labels are then those of
//       sweep s-1, and the counts are theirs.
// Inside a tile every sum runs over the tile's points in point order, per (cluster, entry);
// the rows are added in tile order.  So a trial's result depends on its own inputs only.
#pragma once
#include "vbhem_ghem_run.h"
#include "vbhem_wtk_run.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vbhem {
namespace wtktile {

using namespace wtkrun;
using ghemrun::tile_points;
using ghemrun::tiles_of;

constexpr int kGroup = 8;  // the trials a pass block loops over with its tile's points
constexpr int kSeed = 0, kLloyd = 1, kWeighted = 2;
// the record's integer head
constexpr int fPhase = 0, fStep = 1, fStatus = 2, fIt0 = 3, fIt1 = 4, fDone = 5, fReseed = 6, kFlags = 8;

// the record: kFlags ints, the previous energy, cen [K][d], cw [K] (in doubles)
WTK_HD constexpr size_t rec_len(int K, int d) { return kFlags / 2 + 1 + (size_t)K * d + K; }
struct Rec {
  int *flag;
  double *eold, *cen, *cw;
};
WTK_HD inline Rec rec_at(double *p, int K, int d) {
  Rec r;
  r.flag = reinterpret_cast<int *>(p);
  r.eold = p + kFlags / 2;
  r.cen = r.eold + 1;
  r.cw = r.cen + (size_t)K * d;
  return r;
}

// a tile's row: sums [K][d+1] (the count or weight sum last), energies [K], counts [K], and
// one scalar (SEED: the sum of d2; LLOYD: the changed labels)
WTK_HD constexpr int o_sum() { return 0; }
WTK_HD constexpr int o_energy(int K, int d) { return K * (d + 1); }
WTK_HD constexpr int o_count(int K, int d) { return K * (d + 2); }
WTK_HD constexpr int o_scalar(int K, int d) { return K * (d + 3); }
WTK_HD constexpr int part_len(int K, int d) { return K * (d + 3) + 1; }
constexpr int kPartMax = kMaxK * (kMaxDim + 3) + 1;

// rounds of a call: fixed by K and the pass caps
WTK_HD constexpr int rounds_of(int K, bool seed_only) {
  return (K - 1) + kLloydMax + (seed_only ? 0 : 1 + kWkMax + 1);
}

// The record before the first round (one lane).  False: the draw is out of range (BAD).
WTK_HD inline bool rec_init(const Rec &r, const double *X, int n, int d, int K, int j0) {
  r.flag[fPhase] = K > 1 ? kSeed : kLloyd;
  r.flag[fStep] = K > 1 ? 1 : 0;
  r.flag[fStatus] = kOk;
  r.flag[fIt0] = r.flag[fIt1] = 0;
  r.flag[fDone] = r.flag[fReseed] = 0;
  *r.eold = 0.0;
  if (j0 < 0 || j0 >= n) {
    r.flag[fStatus] = kBad;
    r.flag[fDone] = 1;
    return false;
  }
  for (int a = 0; a < d; ++a) r.cen[a] = X[(size_t)j0 * d + a];
  return true;
}

// SEED: the point a tile's search picks for `target` from the tile's exclusive sum, or kNone
WTK_HD inline int seed_search(const double *d2, int cnt, double run, double target) {
  for (int m = 0; m < cnt; ++m) {
    run += d2[m];
    if (run > target) return m;
  }
  return kNone;
}
WTK_HD inline int seed_fallback(int tile, int nt, int P, int n) { return tile + 1 < nt ? (tile + 1) * P : n - 1; }

// WEIGHTED s >= 1: what the step decides from E = E(s-1): 0 go on, 1 the trial ends
WTK_HD inline int weighted_stop(int s, double E, double eold, int *sweeps) {
  if (s >= 2 && std::fabs(E - eold) < kWkTol) {
    *sweeps = s - 2;
    return 1;
  }
  if (s == kWkMax + 1) {
    *sweeps = kWkMax;
    return 1;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// the serial walker: the rounds of one trial, one lane, the device kernels' order
// ---------------------------------------------------------------------------------------
struct WalkOut {
  int status, reseed, rounds;
};

// the sums [K][d+1] of a tile's points by label, in point order per (cluster, entry)
WTK_HD inline void tile_sums_serial(const double *X, const double *w, int d, int K, const int *lab, int p0, int p1,
                                    double *row) {
  for (int c = 0; c < K; ++c)
    for (int a = 0; a <= d; ++a) {
      double s = 0.0;
      for (int m = p0; m < p1; ++m) {
        if (lab[m] != c) continue;
        if (a < d)
          s += w ? X[(size_t)m * d + a] * w[m] : X[(size_t)m * d + a];
        else
          s += w ? w[m] : 1.0;
      }
      row[o_sum() + c * (d + 1) + a] = s;
    }
}

// One trial.  w null and seed_only: kmeans_pp alone (centres [K][d], iters[0]); else the
// first stage of 'wtkmeans' (labels [n], counts [K], iters [2]).  rec [rec_len], part
// [tiles][part_len], tot [part_len], dwork [n], lwork [n] are scratch.  A trial that is not
// OK, or that asks for a re-seed, leaves the outputs of an OK trial unwritten -- except the
// labels, which a trial writes while it sweeps (every trial that sweeps ends OK).
WTK_HD inline WalkOut tiled_trial_serial(const double *X, const double *w, int n, int d, int K, int j0, const double *u,
                                         bool seed_only, double *recbuf, double *part, double *tot, double *dwork,
                                         int *lwork, int *labels, int *counts, double *centres, int *iters) {
  const int P = tile_points(n, d), nt = tiles_of(n, d), E = part_len(K, d);
  const Rec r = rec_at(recbuf, K, d);
  WalkOut out{kOk, 0, 0};
  if (!rec_init(r, X, n, d, K, j0)) {
    out.status = kBad;
    return out;
  }
  const int rounds = rounds_of(K, seed_only);
  for (int round = 0; round < rounds && !r.flag[fDone]; ++round) {
    out.rounds = round + 1;
    const int phase = r.flag[fPhase], step = r.flag[fStep];
    bool bad = false;
    // the pass
    for (int t = 0; t < nt; ++t) {
      const int p0 = t * P, p1 = p0 + P < n ? p0 + P : n;
      double *row = part + (size_t)t * E;
      for (int e = 0; e < E; ++e) row[e] = 0.0;
      if (round == 0)
        for (int m = p0; m < p1; ++m) {
          for (int a = 0; a < d; ++a) bad = bad || !finite_d(X[(size_t)m * d + a]);
          if (w) bad = bad || !finite_d(w[m]);
        }
      if (phase == kSeed) {
        double s = 0.0;
        for (int m = p0; m < p1; ++m) {
          const double v = dist2(X + (size_t)m * d, r.cen + (size_t)(step - 1) * d, d);
          if (step == 1 || v < dwork[m]) dwork[m] = v;
          s += dwork[m];
        }
        row[o_scalar(K, d)] = s;
      } else if (phase == kLloyd) {
        int ch = 0;
        for (int m = p0; m < p1; ++m) {
          double dm;
          const int l = nearest(X + (size_t)m * d, r.cen, K, d, &dm);
          ch += step > 0 && l != lwork[m];
          lwork[m] = l;
        }
        row[o_scalar(K, d)] = (double)ch;
        tile_sums_serial(X, nullptr, d, K, lwork, p0, p1, row);
      } else if (step == 0) {
        for (int m = p0; m < p1; ++m) {
          double dm;
          lwork[m] = nearest(X + (size_t)m * d, r.cen, K, d, &dm);
        }
        tile_sums_serial(X, w, d, K, lwork, p0, p1, row);
      } else {
        for (int m = p0; m < p1; ++m) {
          const int l = lwork[m];
          const double *x = X + (size_t)m * d;
          const double fm = dist2(x, r.cen + (size_t)l * d, d);
          labels[m] = l;
          row[o_energy(K, d) + l] += w[m] * fm;
          row[o_count(K, d) + l] += 1.0;
          if (step <= kWkMax) dwork[m] = wk_member_f(fm, r.cw[l], w[m]);
        }
        if (step <= kWkMax) {
          for (int m = p0; m < p1; ++m)
            lwork[m] = wk_assign(X + (size_t)m * d, w[m], lwork[m], dwork[m], r.cen, r.cw, K, d);
          tile_sums_serial(X, w, d, K, lwork, p0, p1, row);
        }
      }
    }
    // the step
    if (round == 0 && bad) {
      r.flag[fStatus] = kBad;
      r.flag[fDone] = 1;
      break;
    }
    for (int e = 0; e < E; ++e) {
      double v = 0.0;
      for (int t = 0; t < nt; ++t) v += part[(size_t)t * E + e];
      tot[e] = v;
    }
    const double *sums = tot + o_sum();
    if (phase == kSeed) {
      const double total = tot[o_scalar(K, d)];
      if (!(total > 0.0) || !finite_d(total)) {
        r.flag[fStatus] = kDegenerate;
        r.flag[fDone] = 1;
        break;
      }
      const double target = u[step - 1] * total;
      int tile = nt - 1;
      double run = 0.0, excl = 0.0;
      for (int t = 0; t < nt; ++t) {
        excl = run;
        run += part[(size_t)t * E + o_scalar(K, d)];
        if (run > target) {
          tile = t;
          break;
        }
      }
      const int p0 = tile * P, p1 = p0 + P < n ? p0 + P : n;
      const int m = seed_search(dwork + p0, p1 - p0, excl, target);
      const int pick = m == kNone ? seed_fallback(tile, nt, P, n) : p0 + m;
      for (int a = 0; a < d; ++a) r.cen[(size_t)step * d + a] = X[(size_t)pick * d + a];
      if (step + 1 == K) {
        r.flag[fPhase] = kLloyd;
        r.flag[fStep] = 0;
      } else {
        r.flag[fStep] = step + 1;
      }
      continue;
    }
    if (phase == kLloyd) {
      const int passes = step + 1;
      bool ended = step > 0 && tot[o_scalar(K, d)] == 0.0;
      if (!ended) {
        bool empty = false;
        for (int c = 0; c < K; ++c) empty = empty || !(sums[c * (d + 1) + d] > 0.0);
        if (empty) {
          r.flag[fReseed] = 1;
          r.flag[fDone] = 1;
          break;
        }
        for (int c = 0; c < K; ++c)
          for (int a = 0; a < d; ++a) r.cen[(size_t)c * d + a] = sums[c * (d + 1) + a] / sums[c * (d + 1) + d];
        r.flag[fStep] = passes;
        ended = passes == kLloydMax;
      }
      if (ended) {
        r.flag[fIt0] = passes;
        if (seed_only) {
          r.flag[fDone] = 1;
        } else {
          r.flag[fPhase] = kWeighted;
          r.flag[fStep] = 0;
        }
      }
      continue;
    }
    if (step >= 1) {
      double en = 0.0;
      for (int c = 0; c < K; ++c) en += tot[o_energy(K, d) + c];
      int sweeps = 0;
      if (weighted_stop(step, en, *r.eold, &sweeps)) {
        r.flag[fIt1] = sweeps;
        r.flag[fDone] = 1;
        for (int c = 0; c < K; ++c) counts[c] = (int)tot[o_count(K, d) + c];
        break;
      }
      *r.eold = en;
    }
    for (int c = 0; c < K; ++c) {
      const double cwc = sums[c * (d + 1) + d];
      r.cw[c] = cwc;
      for (int a = 0; a < d; ++a) r.cen[(size_t)c * d + a] = cwc > 0.0 ? sums[c * (d + 1) + a] / cwc : sums[c * (d + 1) + a];
    }
    r.flag[fStep] = step + 1;
  }
  out.status = r.flag[fStatus];
  out.reseed = r.flag[fReseed];
  if (out.status == kOk && !out.reseed) {
    iters[0] = r.flag[fIt0];
    if (seed_only)
      for (int e = 0; e < K * d; ++e) centres[e] = r.cen[e];
    else
      iters[1] = r.flag[fIt1];
  }
  return out;
}

}  // namespace wtktile

#if defined(__HIPCC__)
// vbhem_wtk.hip: wtk_cluster_kernel<DB> over the trials R0 .. R0 + trials - 1, a workgroup
// whose flag only[block * only_stride] is clear leaving at once (the re-seed hand-over)
int wtk_block_rerun(int n, int d, int K, int R0, int trials, const double *x, const double *w, const int *j0,
                    const double *u, int *labels, int *counts, int *status, int *iters, double *wd, int *wl,
                    const int *only, int only_stride, hipStream_t st);
#endif

}  // namespace vbhem
