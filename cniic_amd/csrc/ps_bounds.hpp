// ps_bounds.hpp -- where the chunks of the persistent colour K-means' cell list begin, in plain functions for host and device.
// The compacted list of M non-empty cells carries a cost prefix, ne_cost[0 .. M] (k_cell_scan: ne_cost[0] = 0, strictly increasing,
// ne_cost[M] = total), and is cut into NC chunks of equal cost: boundary g, 0 <= g <= NC, is
//     cb[g] = the first m in [0, M] with ne_cost[m] >= target(g),   target(g) = total * min(g, NC) / NC,   cb[NC] = M.
// k_ps_ranges finds every cb[g] by bisection.  No search is needed: the prefix is increasing, so the boundaries with
// ne_cost[m] < target(g) <= ne_cost[m + 1] are exactly those with cb[g] = m + 1 -- a run of consecutive g that the owner of cell m can
// name from the two prefixes alone (ps_bounds_between), and the g with target(g) <= ne_cost[0] have cb[g] = 0.  Every g in [0, NC] falls
// into exactly one of these M + 1 runs, so when every cell writes its run (the cell-scan role of k_cc_front_b does) every boundary is
// written once.  tests/ps_bounds_check.cpp compiles this file alone, so it includes nothing of the library.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_PSB_HD __host__ __device__ __forceinline__
#else
#define CNIIC_PSB_HD inline
#endif

namespace cniic {

// total < 2^32 (a u32 prefix), g <= NC < 2^15 (1024 blocks x kPsChunks): the product is below 2^47
CNIIC_PSB_HD uint64_t ps_bound_target(uint64_t total, uint32_t g, uint32_t NC) { return total * (g < NC ? g : NC) / NC; }

struct PsBoundRun { uint32_t first, count; };   // boundaries first, first + 1, ..., count of them (0: none)

// the g in [0, NC] with lo < target(g) <= hi; lo < hi <= total, total > 0.
// target(g) > lo  <=>  total g >= (lo + 1) NC  <=>  g >= ceil((lo + 1) NC / total);   target(g) <= hi  <=>  total g < (hi + 1) NC
CNIIC_PSB_HD PsBoundRun ps_bounds_between(uint64_t lo, uint64_t hi, uint64_t total, uint32_t NC) {
    const uint64_t first = ((lo + 1) * NC + total - 1) / total;
    uint64_t end = ((hi + 1) * NC + total - 1) / total;      // the first g whose target is above hi
    if (end > (uint64_t)NC + 1) end = (uint64_t)NC + 1;
    PsBoundRun r;
    r.first = (uint32_t)first;
    r.count = end > first ? (uint32_t)(end - first) : 0u;
    return r;
}
// the g in [0, NC] with target(g) <= hi (cell 0's: hi = ne_cost[0])
CNIIC_PSB_HD PsBoundRun ps_bounds_upto(uint64_t hi, uint64_t total, uint32_t NC) {
    uint64_t end = ((hi + 1) * NC + total - 1) / total;
    if (end > (uint64_t)NC + 1) end = (uint64_t)NC + 1;
    PsBoundRun r;
    r.first = 0u;
    r.count = (uint32_t)end;
    return r;
}

}  // namespace cniic
