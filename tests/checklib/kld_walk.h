// tests/checklib/kld_walk.h -- TEST-ONLY: a host walk of the tables that the planner of
// vbhmm_kld_jobs makes (csrc/vbhmm_kld_plan.h), tile by tile and lane by lane as
// kld_own_kernel and kld_cross_kernel take them, with the routines the kernels call
// (pair_loglik, ccfd::kl_term), so a job's value is the kernel's chain of additions.
// It also counts how often every own slot is written and every (job, item) is taken.
// Plain C++: shared by tests/kldcheck/kldcheck.hip and tests/kldcheck/walker_main.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "vbhmm_ccfd_row.h"
#include "vbhmm_kld_plan.h"
#include "vbhmm_score_pair.h"

namespace kldwalk {

using namespace vbhem::score;
using vbhem::kld::kLanes;
using vbhem::kld::Plan;
using vbhem::kld::Tile4;

struct Walk {
  const Layout &L;
  const std::vector<double> &blocks;
  int d;
  bool diag;
  const int *offsets;
  const double *x;
  const Plan &p;
  const int *pair_first;  // [n_jobs]: the first (job, item) counter of every job, in the caller's order
  double *kl;             // [n_jobs]
  int *own_hits;          // [own_len]
  int *pair_hits;         // [n_lanes]

  template <int KB, int DB>
  double loglik(const Hmm &m, int n, int &T) const {
    const int off = offsets[n];
    T = offsets[n + 1] - off;
    return pair_loglik<KB, DB>(m, x + (size_t)off * d, T, d);
  }

  void hit(int s, int lane) const { ++pair_hits[pair_first[p.job_out[s]] + (lane - p.job_first[s])]; }

  template <int KB, int DB>
  int operator()() const {
    std::vector<double> own((size_t)p.own_len, NAN);
    for (const Tile4 &t : p.own_tiles) {
      const Hmm m = view(L, blocks.data() + (size_t)t.x * L.stride, diag);
      for (int tid = 0; tid < t.z; ++tid) {
        const int slot = t.y + tid;
        int T;
        const double ll = loglik<KB, DB>(m, p.own_seq[slot], T);
        own[slot] = ll / (double)T;
        ++own_hits[slot];
      }
    }
    double term[kLanes];
    for (size_t w = 0; w < p.cross_tiles.size(); ++w) {
      const Tile4 &t = p.cross_tiles[w];
      const int l0 = t.x, cnt = t.y, s0 = t.z, njob = t.w;
      const Hmm m = view(L, blocks.data() + (size_t)p.tile_b[w] * L.stride, diag);
      if (cnt > kLanes) {
        double sum = 0.0;
        for (int base = 0; base < cnt; base += kLanes) {
          const int left = cnt - base < kLanes ? cnt - base : kLanes;
          for (int tid = 0; tid < left; ++tid) {
            int T;
            const int slot = p.job_run[s0] + base + tid;
            const double ll = loglik<KB, DB>(m, p.own_seq[slot], T);
            term[tid] = vbhem::ccfd::kl_term(own[slot], ll, T);
            hit(s0, l0 + base + tid);
          }
          for (int q = 0; q < left; ++q) sum += term[q];
        }
        kl[p.job_out[s0]] = sum / (double)cnt;
        continue;
      }
      int lslot[kLanes], stored = 0;
      for (int tid = 0; tid < njob; ++tid) {
        const int s = s0 + tid, a = p.job_first[s] - l0, b = p.job_first[s + 1] - l0;
        for (int q = a; q < b; ++q, ++stored) {
          lslot[q] = p.job_run[s] + (q - a);
          hit(s, l0 + q);
        }
      }
      if (stored != cnt) return 2;  // a tile whose jobs do not cover its lanes
      for (int tid = 0; tid < cnt; ++tid) {
        int T;
        const int slot = lslot[tid];
        const double ll = loglik<KB, DB>(m, p.own_seq[slot], T);
        term[tid] = vbhem::ccfd::kl_term(own[slot], ll, T);
      }
      for (int tid = 0; tid < njob; ++tid) {
        const int s = s0 + tid, a = p.job_first[s] - l0, b = p.job_first[s + 1] - l0;
        double sum = 0.0;
        for (int q = a; q < b; ++q) sum += term[q];
        kl[p.job_out[s]] = sum / (double)(b - a);
      }
    }
    return 0;
  }
};

// the first (job, item) counter of every job in the caller's order, and their total
inline long long pair_firsts(int n_jobs, const int *jobs, const int *list_offsets, std::vector<int> &first) {
  first.assign((size_t)n_jobs, 0);
  long long at = 0;
  for (int j = 0; j < n_jobs; ++j) {
    first[j] = (int)at;
    const int l = jobs[3 * j + 2];
    at += list_offsets[l + 1] - list_offsets[l];
  }
  return at;
}

}  // namespace kldwalk
