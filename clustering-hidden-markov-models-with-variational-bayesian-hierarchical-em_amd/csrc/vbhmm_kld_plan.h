// vbhmm_kld_plan.h -- the host planner of vbhmm_kld_jobs (include/vbhmm_kld.h): it
// checks every index of (lists, jobs) and turns them into the tables the two kernels of
// vbhmm_kld.hip read.  Plain C++, no HIP types: the library, the host check build
// (tests/kldcheck) and the sanitizer program (tests/kldcheck/walker_main.cpp) share it.
//
//   own table    one run of |list| slots per unique (a, list) of the jobs, in ascending
//                (a, list) order; slot q of a run holds ll_a(n_q) / T of the list's item q.
//                own_seq [own_len] is the sequence of every slot, own_tiles cuts the runs
//                into pieces of at most kLanes slots: (HMM a, first slot, slots, 0).
//   cross tiles  the jobs in a stable order by b.  job_first [P + 1] is the first lane of
//                every sorted job, job_out [P] its place in the caller's kl, job_run [P]
//                the first slot of its (a, list) run: lane q of the job reads slot
//                job_run + q, whose sequence is own_seq of that slot.
//                A tile (first lane, lanes, first sorted job, jobs) is either consecutive
//                whole jobs of one b with at most kLanes lanes in all (and at most kLanes
//                jobs, empty ones included), or one longer job alone; tile_b is its b.
// Nothing the kernels index with leaves this file unchecked: a and b against H, the list
// against n_lists, every item of a list some job uses against N.  Lists no job uses are
// neither checked nor uploaded.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "vbhem_estep.h"

namespace vbhem {
namespace kld {

constexpr int kLanes = 128;  // lanes of a workgroup = (job, item) pairs of a tile

struct Tile4 {  // the 16 bytes of an int4
  int x, y, z, w;
};
struct Plan {
  std::vector<Tile4> own_tiles, cross_tiles;
  std::vector<int> own_seq, tile_b, job_first, job_out, job_run;
  long long own_len = 0, n_lanes = 0;
  int n_jobs = 0;
  std::string error;
};

// byte offsets of the workspace: the own table, then the planner's tables in one
// contiguous piece [tables, total) that is uploaded with one copy
struct WsLayout {
  size_t own, tables, own_seq, own_tiles, job_first, job_out, job_run, cross_tiles, tile_b, total;
};

inline size_t up16(size_t x) { return (x + 15) / 16 * 16; }

inline WsLayout ws_layout(long long own_len, size_t n_own_tiles, int n_jobs, size_t n_cross_tiles) {
  WsLayout w;
  w.own = 0;
  w.tables = up16((size_t)(own_len > 0 ? own_len : 1) * sizeof(double));
  w.own_tiles = w.tables;
  w.cross_tiles = w.own_tiles + up16((n_own_tiles > 0 ? n_own_tiles : 1) * sizeof(Tile4));
  w.own_seq = w.cross_tiles + up16((n_cross_tiles > 0 ? n_cross_tiles : 1) * sizeof(Tile4));
  w.job_first = w.own_seq + up16((size_t)(own_len > 0 ? own_len : 1) * sizeof(int));
  w.job_out = w.job_first + up16(((size_t)n_jobs + 1) * sizeof(int));
  w.job_run = w.job_out + up16((size_t)(n_jobs > 0 ? n_jobs : 1) * sizeof(int));
  w.tile_b = w.job_run + up16((size_t)(n_jobs > 0 ? n_jobs : 1) * sizeof(int));
  w.total = w.tile_b + up16((n_cross_tiles > 0 ? n_cross_tiles : 1) * sizeof(int));
  return w;
}

inline WsLayout ws_layout(const Plan &p) {
  return ws_layout(p.own_len, p.own_tiles.size(), p.n_jobs, p.cross_tiles.size());
}

// the planner's tables as the bytes of [w.tables, w.total)
inline std::vector<char> pack_tables(const Plan &p, const WsLayout &w) {
  std::vector<char> buf(w.total - w.tables, 0);
  auto put = [&](size_t at, const void *src, size_t bytes) {
    if (bytes) std::memcpy(buf.data() + (at - w.tables), src, bytes);
  };
  put(w.own_tiles, p.own_tiles.data(), p.own_tiles.size() * sizeof(Tile4));
  put(w.cross_tiles, p.cross_tiles.data(), p.cross_tiles.size() * sizeof(Tile4));
  put(w.own_seq, p.own_seq.data(), p.own_seq.size() * sizeof(int));
  put(w.job_first, p.job_first.data(), p.job_first.size() * sizeof(int));
  put(w.job_out, p.job_out.data(), p.job_out.size() * sizeof(int));
  put(w.job_run, p.job_run.data(), p.job_run.size() * sizeof(int));
  put(w.tile_b, p.tile_b.data(), p.tile_b.size() * sizeof(int));
  return buf;
}

inline int plan_fail(Plan &p, int code, const std::string &msg) {
  p.error = "vbhmm_kld_jobs: " + msg;
  return code;
}

inline std::string outside(const char *what, long long v, long long bound) {
  return std::string(what) + " " + std::to_string(v) + " is outside [0, " + std::to_string(bound) + ")";
}

// (lists, jobs) of H HMMs and N sequences into `p`.  list_items == nullptr: sizes only
// (the tile tables and counts, no item is read and a, b are held to >= 0 alone) -- what
// vbhmm_kld_jobs_workspace_bytes needs.  VBHEM_OK, or the status with p.error naming the
// first offender: the offsets first, then the jobs in order (a, b, list), then the items
// of the lists in use in job order.
inline int make_plan(int H, int N, int n_lists, const int *list_offsets, const int *list_items, int n_jobs,
                     const int *jobs, Plan &p) {
  p = Plan();
  const bool sizing = list_items == nullptr;
  if (n_lists < 0 || n_jobs < 0) return plan_fail(p, VBHEM_ERR_ARG, "negative list or job count");
  if (n_jobs == 0) {
    p.job_first.assign(1, 0);
    return VBHEM_OK;
  }
  if (!list_offsets || !jobs) return plan_fail(p, VBHEM_ERR_ARG, "null list offsets or jobs");
  if (list_offsets[0] < 0) return plan_fail(p, VBHEM_ERR_ARG, "list offsets start below 0");
  for (int l = 0; l < n_lists; ++l)
    if (list_offsets[l + 1] < list_offsets[l])
      return plan_fail(p, VBHEM_ERR_ARG, "list offsets decrease at list " + std::to_string(l));
  for (int j = 0; j < n_jobs; ++j) {
    const int a = jobs[3 * j], b = jobs[3 * j + 1], l = jobs[3 * j + 2];
    const std::string who = "job " + std::to_string(j) + ": ";
    if (a < 0 || (!sizing && a >= H)) return plan_fail(p, VBHEM_ERR_ARG, who + outside("HMM a =", a, H));
    if (b < 0 || (!sizing && b >= H)) return plan_fail(p, VBHEM_ERR_ARG, who + outside("HMM b =", b, H));
    if (l < 0 || l >= n_lists) return plan_fail(p, VBHEM_ERR_ARG, who + outside("list", l, n_lists));
  }
  auto len = [&](int l) { return list_offsets[l + 1] - list_offsets[l]; };
  if (!sizing) {
    std::vector<char> seen((size_t)n_lists, 0);
    for (int j = 0; j < n_jobs; ++j) {
      const int l = jobs[3 * j + 2];
      if (seen[l]) continue;
      seen[l] = 1;
      for (int q = 0; q < len(l); ++q) {
        const int n = list_items[list_offsets[l] + q];
        if (n < 0 || n >= N)
          return plan_fail(p, VBHEM_ERR_ARG,
                           "list " + std::to_string(l) + " item " + std::to_string(q) + ": " + outside("sequence", n, N));
      }
    }
  }

  // the own table: one run per unique (a, list)
  std::vector<long long> keys((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j) keys[j] = (long long)jobs[3 * j] * n_lists + jobs[3 * j + 2];
  std::vector<long long> uniq(keys);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  std::vector<long long> run_first(uniq.size() + 1, 0);
  for (size_t u = 0; u < uniq.size(); ++u) run_first[u + 1] = run_first[u] + len((int)(uniq[u] % n_lists));
  p.own_len = run_first.back();
  if (p.own_len > INT_MAX) return plan_fail(p, VBHEM_ERR_UNSUPPORTED, "more than 2^31 - 1 own-table slots; split the jobs");
  if (!sizing) p.own_seq.resize((size_t)p.own_len);
  for (size_t u = 0; u < uniq.size(); ++u) {
    const int a = (int)(uniq[u] / n_lists), l = (int)(uniq[u] % n_lists), c = len(l);
    if (!sizing)
      for (int q = 0; q < c; ++q) p.own_seq[(size_t)run_first[u] + q] = list_items[list_offsets[l] + q];
    for (int q = 0; q < c; q += kLanes)
      p.own_tiles.push_back(Tile4{a, (int)run_first[u] + q, c - q < kLanes ? c - q : kLanes, 0});
  }

  // the jobs in a stable order by b, their lanes, the tiles
  std::vector<int> order((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j) order[j] = j;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return jobs[3 * x + 1] < jobs[3 * y + 1]; });
  p.n_jobs = n_jobs;
  p.job_first.assign((size_t)n_jobs + 1, 0);
  p.job_out.assign(order.begin(), order.end());
  long long at = 0;
  for (int s = 0; s < n_jobs; ++s) {
    at += len(jobs[3 * order[s] + 2]);
    if (at > INT_MAX) return plan_fail(p, VBHEM_ERR_UNSUPPORTED, "more than 2^31 - 1 (job, item) pairs; split the jobs");
    p.job_first[s + 1] = (int)at;
  }
  p.n_lanes = at;
  p.job_run.resize((size_t)n_jobs);
  for (int s = 0; s < n_jobs; ++s)
    p.job_run[s] = (int)run_first[std::lower_bound(uniq.begin(), uniq.end(), keys[order[s]]) - uniq.begin()];
  const std::vector<int> &jf = p.job_first;
  for (int s = 0; s < n_jobs;) {
    const int b = jobs[3 * order[s] + 1], c = jf[s + 1] - jf[s];
    if (c > kLanes) {
      p.cross_tiles.push_back(Tile4{jf[s], c, s, 1});
      p.tile_b.push_back(b);
      ++s;
      continue;
    }
    int last = s + 1;  // consecutive whole jobs of this b while the lanes last
    while (last < n_jobs && jobs[3 * order[last] + 1] == b && last - s < kLanes && jf[last + 1] - jf[s] <= kLanes) ++last;
    p.cross_tiles.push_back(Tile4{jf[s], jf[last] - jf[s], s, last - s});
    p.tile_b.push_back(b);
    s = last;
  }
  return VBHEM_OK;
}

}  // namespace kld
}  // namespace vbhem
