// pal_bounds.hpp -- the box-distance arithmetic of the frozen-palette table (k_palette.hip), in plain functions for host and device.
// tests/palette_bounds_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The colour cube is cut into cells of kPalCellSide^3 colours.  For one cell's box and one palette entry:
//   dmin  the squared distance from the entry to the NEAREST point of the box   (0 when the entry lies inside)
//   dmax  the squared distance from the entry to the FARTHEST point of the box  (always a corner)
// both sums of per-axis integers.  With B = the smallest dmax over all entries, every colour p of the box has an entry within B
// (the one whose dmax is B), so an entry with dmin > B is farther from p than that one and can be nobody's nearest -- not even in a
// tie.  An entry with dmin == B can tie, and under the lowest-index rule a tie can win: the candidate test is <=, never <.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_PAL_HD __host__ __device__ inline
#else
#define CNIIC_PAL_HD inline
#endif

namespace cniic {

constexpr uint32_t kPalCellBits = 4;                          // a cell is 16 x 16 x 16 colours ...
constexpr uint32_t kPalCellSide = 1u << kPalCellBits;
constexpr uint32_t kPalCellsPerAxis = 256u >> kPalCellBits;
constexpr uint32_t kPalCells = kPalCellsPerAxis * kPalCellsPerAxis * kPalCellsPerAxis;   // ... of which the cube has 4096
constexpr uint32_t kPalListMax = 4096;                        // candidates of one cell kept in LDS; a longer list sends the cell down the plain route

// cell number -> the low corner of its box, one channel per byte like a colour key (r << 16 | g << 8 | b)
CNIIC_PAL_HD uint32_t pal_cell_corner(uint32_t cell) {
    const uint32_t m = kPalCellsPerAxis - 1;
    return (((cell / (kPalCellsPerAxis * kPalCellsPerAxis)) & m) << (16 + kPalCellBits)) | (((cell / kPalCellsPerAxis) & m) << (8 + kPalCellBits)) |
           ((cell & m) << kPalCellBits);
}
CNIIC_PAL_HD uint32_t pal_cell_of(uint32_t key) {
    const uint32_t s = kPalCellBits, m = kPalCellsPerAxis - 1;
    return ((((key >> 16) & 255u) >> s) * kPalCellsPerAxis + ((((key >> 8) & 255u) >> s) & m)) * kPalCellsPerAxis + (((key & 255u) >> s) & m);
}

// one axis: the interval [lo, lo + kPalCellSide - 1] against the coordinate c
CNIIC_PAL_HD uint32_t pal_axis_min(int32_t c, int32_t lo) {
    const int32_t hi = lo + (int32_t)kPalCellSide - 1;
    const int32_t d = c < lo ? lo - c : c > hi ? c - hi : 0;
    return (uint32_t)(d * d);
}
CNIIC_PAL_HD uint32_t pal_axis_max(int32_t c, int32_t lo) {
    const int32_t hi = lo + (int32_t)kPalCellSide - 1;
    const int32_t a = c - lo, b = hi - c;          // (one of them may be negative: the other is then the larger in magnitude as well)
    const int32_t d = (a < 0 ? -a : a) > (b < 0 ? -b : b) ? a : b;
    return (uint32_t)(d * d);
}
// entry, corner: 0xRRGGBB words
CNIIC_PAL_HD uint32_t pal_box_dmin(uint32_t entry, uint32_t corner) {
    return pal_axis_min((int32_t)((entry >> 16) & 255u), (int32_t)((corner >> 16) & 255u)) + pal_axis_min((int32_t)((entry >> 8) & 255u), (int32_t)((corner >> 8) & 255u)) +
           pal_axis_min((int32_t)(entry & 255u), (int32_t)(corner & 255u));
}
CNIIC_PAL_HD uint32_t pal_box_dmax(uint32_t entry, uint32_t corner) {
    return pal_axis_max((int32_t)((entry >> 16) & 255u), (int32_t)((corner >> 16) & 255u)) + pal_axis_max((int32_t)((entry >> 8) & 255u), (int32_t)((corner >> 8) & 255u)) +
           pal_axis_max((int32_t)(entry & 255u), (int32_t)(corner & 255u));
}
// bound: the smallest dmax of the cell over all entries
CNIIC_PAL_HD bool pal_is_candidate(uint32_t dmin, uint32_t bound) { return dmin <= bound; }

// the rule itself: squared distance of two 0xRRGGBB words (Rgb<u8>::dist of geom.rs:8-24 before the root)
CNIIC_PAL_HD uint32_t pal_dist2(uint32_t a, uint32_t b) {
    const int32_t dr = (int32_t)((a >> 16) & 255u) - (int32_t)((b >> 16) & 255u), dg = (int32_t)((a >> 8) & 255u) - (int32_t)((b >> 8) & 255u),
                  db = (int32_t)(a & 255u) - (int32_t)(b & 255u);
    return (uint32_t)(dr * dr + dg * dg + db * db);
}

}  // namespace cniic
