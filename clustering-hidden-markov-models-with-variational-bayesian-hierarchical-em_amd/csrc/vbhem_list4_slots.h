// vbhem_list4_slots.h -- where the statistics-accumulating gate-list pass
// (fb_list4_kernel<T, FAST, true>) puts its partial sums, shared by that kernel, its
// reduction (list4_stats_reduce_kernel) and the host.  Internal.
//
// The pass's work items are the quads of the gate lists, numbered cluster by cluster:
// cluster j owns the items [pre_j, pre_j + ceil(tot_j / 4)), pre_j the running sum.
// Wave g of a grid of nw waves takes the contiguous range [g per, (g + 1) per) of them,
// per = ceil(items / nw), and writes one partial per cluster its range touches, into
// slot g + j.  Along the item order (g, j) never decreases and one of the two grows from
// one partial to the next, so the slots are distinct and ordered by item, a cluster's
// slots are consecutive (the busy waves are a prefix of the grid), and the largest is
// (nw - 1) + (K - 1): at most nw + K slots, a function of the list lengths and the grid
// alone.
#pragma once
#include <hip/hip_runtime.h>

namespace vbhem {

// the feature tiles (of 16) an accumulating wave holds: NUP <= 48 (d <= 8 full)
constexpr int kL4sMaxTiles = 3;

__host__ __device__ inline int l4s_items(int tot) { return (tot + 3) / 4; }
// items per wave
__host__ __device__ inline int l4s_per_wave(int nitem, int nw) {
  return nitem > 0 && nw > 0 ? (nitem + nw - 1) / nw : 1;
}
__host__ __device__ inline int l4s_wave(int item, int per) { return item / per; }
__host__ __device__ inline int l4s_slot(int item, int cluster, int per) { return item / per + cluster; }
__host__ __device__ inline int l4s_max_slots(int nw, int K) { return nw + K; }
// one partial: U [S][NUP] | N1 [S] | M [S][S]
__host__ __device__ inline int l4s_part_len(int S, int NUP) { return S * NUP + S + S * S; }

}  // namespace vbhem

// (exported for the tests, not part of the public interface) the plan for the list
// lengths tot[K] on a grid of nw waves: *per, and per cluster its first slot and slot
// count (0 for an empty list); returns the item count
extern "C" int vbhem_list4_stats_slot_plan(const int *tot, int K, int nw, int *per, int *first,
                                           int *count);
