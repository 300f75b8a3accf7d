// vor_paint.hpp -- the arithmetic of the voronoi repaint (k_misc.hip: k_voronoi_paint_tiles, voronoi_paint) and the gate in front of it
// (codec.cpp, the voronoi case of the single decode), in plain functions for host and device.  tests/vor_paint_check.cpp compiles this
// file alone, so it includes nothing of the library.
//
// The statement to match is VoronoiCluster::decode (clusterc.rs:180-186): pixel (x, y) takes the colour of the FIRST centroid with the
// smallest (c.x - x)^2 + (c.y - y)^2 in u32 arithmetic that wraps (vs_paint_dist, vor_small.hpp).  The tiled kernel prunes the centroids
// per tile in true signed 32-bit arithmetic, which equals the wrapping one while every coordinate and both sides stay inside the bound.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_VP_HD __host__ __device__ __forceinline__ constexpr
#else
#define CNIIC_VP_HD inline constexpr
#endif

namespace cniic {

constexpr int32_t kVorPaintTileW = 64, kVorPaintTileH = 32;   // pixels of a tile: one 256-thread block, 8 rows a thread
constexpr uint32_t kVorPaintCap = 256;                        // centroids a tile keeps in LDS; a longer list sends the tile to brute force
constexpr uint32_t kVorPaintMaxK = 4096;                      // largest K of the tiled kernel: 16 consecutive ids a thread, 12 id bits in the pivot word
constexpr uint32_t kVorPaintIdBits = 12;
constexpr uint32_t kVorPaintCoordBound = 1u << 14;            // sides <= this, coordinates < this: the tiled kernel's arithmetic is exact
static_assert(kVorPaintMaxK == 1u << kVorPaintIdBits, "an id of the tiled kernel fits the pivot word's low bits");
static_assert(kVorPaintMaxK == 16 * 256, "16 ids a thread: a bit each in the kernel's 32-bit keep mask");
static_assert(kVorPaintTileW * kVorPaintTileH == 256 * 8, "a tile is 256 threads of 8 pixels");

// The gate (the host checks it; any other stream takes the brute-force kernel k_voronoi_paint, whose arithmetic wraps as the reference's does)
CNIIC_VP_HD bool vp_sides_small(uint32_t w, uint32_t h) { return w <= kVorPaintCoordBound && h <= kVorPaintCoordBound; }
CNIIC_VP_HD bool vp_coord_small(uint32_t x, uint32_t y) { return x < kVorPaintCoordBound && y < kVorPaintCoordBound; }
CNIIC_VP_HD bool vp_tiled_k(uint64_t K) { return K >= 1 && K <= kVorPaintMaxK; }

// A tile's pixels, clipped to the image: x0 <= x <= x1, y0 <= y <= y1.  Behind the gate 0 <= x0 <= x1 <= 16383, and so for y.
struct VpRect { int32_t x0, x1, y0, y1; };
CNIIC_VP_HD uint32_t vp_tiles_x(uint32_t w) { return (w + (uint32_t)kVorPaintTileW - 1) / (uint32_t)kVorPaintTileW; }
CNIIC_VP_HD uint32_t vp_tiles_y(uint32_t h) { return (h + (uint32_t)kVorPaintTileH - 1) / (uint32_t)kVorPaintTileH; }
CNIIC_VP_HD VpRect vp_tile_rect(uint32_t tile, uint32_t tiles_x, uint32_t w, uint32_t h) {
    const uint32_t tx0 = (tile % tiles_x) * (uint32_t)kVorPaintTileW, ty0 = (tile / tiles_x) * (uint32_t)kVorPaintTileH;
    const uint32_t tx1 = tx0 + (uint32_t)kVorPaintTileW, ty1 = ty0 + (uint32_t)kVorPaintTileH;
    return VpRect{(int32_t)tx0, (int32_t)(w < tx1 ? w : tx1) - 1, (int32_t)ty0, (int32_t)(h < ty1 ? h : ty1) - 1};
}

// The pivot of a tile is the centroid nearest the tile's centre, the lowest id among equals: four times the squared distance to the
// centre ((x0 + x1) / 2, (y0 + y1) / 2), in whole numbers.  |2 cx - (x0 + x1)| <= 2 * 16383, so the key is at most 2 * 32766^2.
CNIIC_VP_HD uint32_t vp_pivot_key(int32_t cx, int32_t cy, const VpRect &r) {
    const int32_t dx = 2 * cx - (r.x0 + r.x1), dy = 2 * cy - (r.y0 + r.y1);
    return (uint32_t)(dx * dx + dy * dy);
}
constexpr int64_t kVorPaintKeyBound = 2 * (int64_t)(2 * (kVorPaintCoordBound - 1)) * (2 * (kVorPaintCoordBound - 1));
static_assert(kVorPaintKeyBound == 2147221512ll && kVorPaintKeyBound < (1ll << 31), "the pivot key stays below 2^31");
static_assert(vp_pivot_key(16383, 16383, VpRect{0, 0, 0, 0}) == kVorPaintKeyBound && vp_pivot_key(0, 0, VpRect{16383, 16383, 16383, 16383}) == kVorPaintKeyBound,
              "... and reaches the bound at the far corners (a constant expression: an overflow would not compile)");
// key and id in one word whose minimum over the centroids is the pivot
CNIIC_VP_HD uint64_t vp_pivot_word(uint32_t key, uint32_t k) { return ((uint64_t)key << kVorPaintIdBits) | k; }
CNIIC_VP_HD uint32_t vp_pivot_id(uint64_t word) { return (uint32_t)(word & (uint64_t)(kVorPaintMaxK - 1)); }

// Centroid (kx, ky) is kept beside the pivot (px, py) iff some pixel p of the rectangle has d(p, c) <= d(p, pivot), i.e. unless the pivot
// is STRICTLY nearer everywhere -- so every minimum and every tie survives.  d(p, pivot) - d(p, c) =
// (px - kx)(px + kx - 2 x) + (py - ky)(py + ky - 2 y) is linear in x and in y apart, so its maximum over the rectangle is the sum of the two
// maxima over the ends, and the test is exact, not only safe.  |px - kx| <= 16383 and |px + kx - 2 x| <= 2 * 16383: a product stays below 2^30.
CNIIC_VP_HD int32_t vp_max32(int32_t a, int32_t b) { return a > b ? a : b; }
CNIIC_VP_HD int32_t vp_keep_f(int32_t px, int32_t py, int32_t kx, int32_t ky, const VpRect &r) {
    const int32_t dx = px - kx, dy = py - ky;
    return vp_max32(dx * (kx + px - 2 * r.x0), dx * (kx + px - 2 * r.x1)) + vp_max32(dy * (ky + py - 2 * r.y0), dy * (ky + py - 2 * r.y1));
}
CNIIC_VP_HD bool vp_keep(int32_t px, int32_t py, int32_t kx, int32_t ky, const VpRect &r) { return vp_keep_f(px, py, kx, ky, r) >= 0; }
constexpr int64_t kVorPaintProductBound = (int64_t)(kVorPaintCoordBound - 1) * (2 * (kVorPaintCoordBound - 1));
static_assert(kVorPaintProductBound == 536805378ll && kVorPaintProductBound < (1ll << 30), "each product of the keep predicate stays below 2^30 (and their sum below 2^31)");
static_assert(vp_keep_f(16383, 16383, 0, 0, VpRect{0, 0, 0, 0}) == 2 * (16383 * 16383) && vp_keep_f(0, 0, 16383, 16383, VpRect{0, 16383, 0, 16383}) == 2 * (16383 * 16383),
              "... at the far corners too");
// the tile paints from its list while the kept centroids fit the LDS list
CNIIC_VP_HD bool vp_list_fits(uint32_t kept) { return kept <= kVorPaintCap; }

}  // namespace cniic
