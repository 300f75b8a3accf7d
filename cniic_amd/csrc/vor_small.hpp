// vor_small.hpp -- the per-point arithmetic and the stream layout of k_vor_small (k_vor_small.hip: voronoi(K <= 256) of a small frame on one
// workgroup) and the pixel rule of k_vor_small_dec, in plain functions for host and device.  tests/vor_small_check.cpp compiles this file
// alone, so it includes nothing of the library.
//
// The statement to match is kmeans::cluster (src/kmeans.rs) over ColorPos points (clusterc.rs:200-248) with exact nearest-centroid search:
// the points are the frame's pixels in row-major order, x = i % w, y = i / w; everything is integer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_VS_HD __host__ __device__ __forceinline__
#else
#define CNIIC_VS_HD inline
#endif

namespace cniic {

constexpr uint32_t kVorSmallMaxPx = 16384;   // pixels of a frame that takes the route
constexpr uint32_t kVorSmallMaxK = 256;
constexpr uint64_t kVorSmallDefaultSeed = 0x636E696963ULL;   // (= kDefaultSeed, common.hpp)
// w h <= kVorSmallMaxPx: |dx| <= w - 1 and |dy| <= h - 1 with (w - 1) + (h - 1) <= w h - 1, so dx^2 + dy^2 <= (w h - 1)^2
constexpr uint64_t kVorSmallPosBound = (uint64_t)(kVorSmallMaxPx - 1) * (kVorSmallMaxPx - 1);
constexpr uint64_t kVorSmallDistBound = kVorSmallPosBound + 3ull * 255 * 255;   // any squared distance between two points of a routed frame
static_assert(kVorSmallDistBound < (1ull << 29), "a squared distance of a routed frame is below 2^29");
static_assert(4 * kVorSmallDistBound < (1ull << 32), "four times a squared distance fits u32 (the stay test)");
// a cluster's coordinate sum is at most (largest coordinate) * (all pixels of the frame); a colour sum is smaller
constexpr uint64_t kVorSmallSumBound = (uint64_t)(kVorSmallMaxPx - 1) * kVorSmallMaxPx;
static_assert(kVorSmallSumBound < (1ull << 28), "coordinate sums of a routed frame fit u32");
static_assert(255ull * kVorSmallMaxPx < kVorSmallSumBound, "... and so do the colour sums");
// (distance << 8) | index, the packed word of ccs_score, does NOT fit 32 bits here: distances are compared and k walks upwards
static_assert((kVorSmallDistBound << 8) >= (1ull << 32), "no packed score: the distance alone takes 29 bits");

// kmeans.rs:61-78 init_assignment per point index (n / K >= 1)
CNIIC_VS_HD uint32_t vs_init_label(uint32_t i, uint32_t n, uint32_t K) {
    const uint32_t ppc = n / K, c = (n - 1 - i) / ppc;
    return c > K - 1 ? K - 1 : c;
}
// kmeans.rs:101-108 init_centroids: the first point of cluster c's chunk
CNIIC_VS_HD uint32_t vs_init_centroid_point(uint32_t c, uint32_t n, uint32_t K) { return c < K - 1 ? n - (c + 1) * (n / K) : 0; }

// the point an empty cluster c takes at iteration iter (splitmix64 of seed, iteration and cluster; kmeans.rs:123-133)
CNIIC_VS_HD uint32_t vs_reseed_index(uint64_t seed, uint64_t iter, uint32_t c, uint32_t n) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ULL * (iter * 65536ULL + (uint64_t)c + 1ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (uint32_t)(z % n);
}

// A point or a centroid: x | y << 16 (both below 2^14) and 0xRRGGBB (higher bits are ignored).
// The squared distance over the five coordinates (below 2^29, kVorSmallDistBound)
CNIIC_VS_HD uint32_t vs_dist2(uint32_t axy, uint32_t argb, uint32_t bxy, uint32_t brgb) {
    const int32_t dx = (int32_t)(axy & 0xffffu) - (int32_t)(bxy & 0xffffu), dy = (int32_t)(axy >> 16) - (int32_t)(bxy >> 16);
    const int32_t dr = (int32_t)((argb >> 16) & 255u) - (int32_t)((brgb >> 16) & 255u), dg = (int32_t)((argb >> 8) & 255u) - (int32_t)((brgb >> 8) & 255u),
                  db = (int32_t)(argb & 255u) - (int32_t)(brgb & 255u);
    return (uint32_t)(dx * dx + dy * dy + dr * dr + dg * dg + db * db);
}
// The stay test.  dcur: the squared distance of a point to the centroid of its own cluster; sep: the smallest squared distance from that
// centroid to another one (0xffffffff where there is no other).  4 dcur <= sep is 2 d(p, cur) <= d(cur, k) for every other k, so by the
// triangle inequality d(p, k) >= d(cur, k) - d(p, cur) >= d(p, cur): no centroid is STRICTLY nearer and the point stays.  With a duplicate
// of its centroid about (sep = 0) it passes at distance 0 alone.
CNIIC_VS_HD bool vs_stays(uint32_t dcur, uint32_t sep) { return 4u * dcur <= sep; }
// kmeans.rs:375: a point leaves its cluster only for a centroid that is STRICTLY nearer.  best, best_k: the smallest distance over all k and the
// LOWEST index that has it (the search walks k upwards and takes a new minimum on `<` alone)
CNIIC_VS_HD uint32_t vs_new_label(uint32_t best, uint32_t best_k, uint32_t dcur, uint32_t cur) { return best < dcur ? best_k : cur; }
// Point::mean for ColorPos (clusterc.rs:216-247): truncating per coordinate; x and y stay u32, the colours are cut to u8
CNIIC_VS_HD uint32_t vs_mean_xy(uint32_t sx, uint32_t sy, uint32_t members) { return (sx / members) | (sy / members) << 16; }
CNIIC_VS_HD uint32_t vs_mean_rgb(uint32_t sr, uint32_t sg, uint32_t sb, uint32_t members) {
    return ((sr / members) & 255u) << 16 | ((sg / members) & 255u) << 8 | ((sb / members) & 255u);
}

// VoronoiCluster's stream (clusterc.rs:156-164, 250-257): w, h as u32, K as u64, then per centroid x, y as u32, the u64 3, r g b
CNIIC_VS_HD uint32_t vs_stream_len(uint32_t K) { return 16u + 19u * K; }
CNIIC_VS_HD uint32_t vs_centroid_at(uint32_t k) { return 16u + 19u * k; }
// byte j (0 .. 18) of a centroid's record
CNIIC_VS_HD uint8_t vs_centroid_byte(uint32_t x, uint32_t y, uint32_t rgb, uint32_t j) {
    if (j < 4) return (uint8_t)(x >> (8 * j));
    if (j < 8) return (uint8_t)(y >> (8 * (j - 4)));
    if (j < 16) return j == 8 ? 3 : 0;
    return (uint8_t)(rgb >> (8 * (18 - j)));
}

// The decoder's pixel rule (clusterc.rs:183): (c.x - x)^2 + (c.y - y)^2 in u32 arithmetic that wraps, so a hostile centroid coordinate
// gives what the reference's arithmetic gives; the first centroid with the smallest value colours the pixel
CNIIC_VS_HD uint32_t vs_paint_dist(uint32_t cx, uint32_t cy, uint32_t x, uint32_t y) {
    const uint32_t dx = cx - x, dy = cy - y;
    return dx * dx + dy * dy;
}

}  // namespace cniic
