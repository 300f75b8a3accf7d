// cc_small.hpp -- the per-point arithmetic of k_cc_small (k_cc_small.hip: cluster-colors(K <= 256) of a small frame on one workgroup), in
// plain functions for host and device.  tests/cc_small_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The statement to match is kmeans::cluster (src/kmeans.rs) with exact nearest-centroid search: points are a frame's distinct colours in
// ascending key order (0xRRGGBB), weighted by their pixel counts; everything is integer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_CCS_HD __host__ __device__ __forceinline__
#else
#define CNIIC_CCS_HD inline
#endif

namespace cniic {

constexpr uint32_t kCcSmallMaxPx = 16384;   // pixels (so distinct colours at most) of a frame that takes the route
constexpr uint32_t kCcSmallMaxK = 256;
constexpr uint64_t kCcSmallDefaultSeed = 0x636E696963ULL;   // (= kDefaultSeed, common.hpp)
// a cluster's channel sum is at most 255 * (all pixels of the frame): the sums are u32
constexpr uint64_t kCcSmallSumBound = 255ull * kCcSmallMaxPx;
static_assert(kCcSmallSumBound < (1ull << 32), "channel sums of a routed frame fit u32");

// kmeans.rs:61-78 init_assignment per point index (U / K >= 1)
CNIIC_CCS_HD uint32_t ccs_init_label(uint32_t i, uint32_t U, uint32_t K) {
    const uint32_t ppc = U / K, c = (U - 1 - i) / ppc;
    return c > K - 1 ? K - 1 : c;
}
// kmeans.rs:101-108 init_centroids: the first point of cluster c's chunk
CNIIC_CCS_HD uint32_t ccs_init_centroid_point(uint32_t c, uint32_t U, uint32_t K) { return c < K - 1 ? U - (c + 1) * (U / K) : 0; }

// the point whose colour an empty cluster c takes at iteration iter (splitmix64 of seed, iteration and cluster; kmeans.rs:123-133)
CNIIC_CCS_HD uint32_t ccs_reseed_index(uint64_t seed, uint64_t iter, uint32_t c, uint32_t U) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ULL * (iter * 65536ULL + (uint64_t)c + 1ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (uint32_t)(z % U);
}

// r*r' + g*g' + b*b' of two 0xRRGGBB words
CNIIC_CCS_HD uint32_t ccs_dot(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a & 0xffffffu, b & 0xffffffu, 0u, false);
#else
    return ((a >> 16) & 255) * ((b >> 16) & 255) + ((a >> 8) & 255) * ((b >> 8) & 255) + (a & 255) * (b & 255);
#endif
}
// The score of point p against centroid k: ((|c|^2 - 2 p.c) << 8) | k as a signed word.  |p - c|^2 = |p|^2 + (|c|^2 - 2 p.c), so for one
// point the signed minimum over k is the nearest centroid, the LOWEST index among equal distances (the index sits below the value).
// |c|^2 - 2 p.c lies in [-195075, 195075]: the word cannot overflow.  ccs_cconst is the centroid's half, computed once per iteration.
CNIIC_CCS_HD int32_t ccs_cconst(uint32_t cent, uint32_t k) { return (int32_t)(ccs_dot(cent, cent) << 8) + (int32_t)k; }
CNIIC_CCS_HD int32_t ccs_score(uint32_t p, uint32_t cent, int32_t cconst) { return cconst - (int32_t)(ccs_dot(p, cent) << 9); }
// kmeans.rs:375: a point leaves its cluster only for a centroid that is STRICTLY nearer.  best: the minimum score over all k; cur_score:
// the score against the centroid of the point's own cluster
CNIIC_CCS_HD uint32_t ccs_new_label(int32_t best, int32_t cur_score, uint32_t cur) {
    return (best >> 8) < (cur_score >> 8) ? (uint32_t)(best & 255) : cur;
}
// Point::mean for ColorCount (clusterc.rs:83-113): truncating per channel
CNIIC_CCS_HD uint32_t ccs_mean(uint32_t sr, uint32_t sg, uint32_t sb, uint32_t wsum) {
    return ((sr / wsum) & 255) << 16 | ((sg / wsum) & 255) << 8 | ((sb / wsum) & 255);
}

}  // namespace cniic
