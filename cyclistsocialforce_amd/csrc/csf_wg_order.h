// csf_wg_order.h — the order in which the receiver groups of one source chunk are handed to the workgroups of pair_cull_kernel
// (csf_bin.hip: wg_order_kernel; csf_pair.hip: Dev::wg_order, Dev::wg_cost).
//
// The launch is dispatched chunk by chunk, and when its last chunk is under way nothing is left to fill the slots that free
// first: the SIMDs end up to 17 us apart.  A chunk whose heavy groups start first ends with light ones, which pack the tail
// (list scheduling, longest job first).  What a group costs is known from the launch two ticks before: every workgroup leaves
// 28 x tests + 58 x evaluations, the vector instructions of its sift and field passes, in Dev::wg_cost.
//
// The rank of a group is the number of groups of its chunk that are heavier, or as heavy with a lower index.  Counted like that
// the ranks are a permutation of 0 .. n - 1 WHATEVER the costs are - stale, zero or garbage - and that is all the pair kernel
// needs of them: a workgroup's sums go to the slots of its receivers, whichever workgroup serves them.
#pragma once
#include <stdint.h>

namespace csf {

// how many of keys[0 .. n) - the costs of groups first .. first + n - 1 - come before the group `index` with cost `mine`
__host__ __device__ inline int wg_rank_count(const uint32_t *keys, int n, int first, uint32_t mine, int index) {
    int c = 0;
#pragma unroll 16
    for (int j = 0; j < n; j++) c += (keys[j] > mine) | ((keys[j] == mine) & (first + j < index));
    return c;
}

// Host copy of wg_order_kernel for one chunk: order[rank] = group.
inline void wg_order_host(const uint32_t *cost, int n, int32_t *order) {
    for (int i = 0; i < n; i++) order[wg_rank_count(cost, n, 0, cost[i], i)] = i;
}

}  // namespace csf
