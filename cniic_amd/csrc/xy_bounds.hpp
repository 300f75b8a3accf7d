// xy_bounds.hpp -- the integer arithmetic the tiled 5-D K-means (k_kmeans_xyrgb.hip) rests on, in plain functions for host and device:
// the floor division of a centroid's coordinate sums, the distance from a box centre, and the box-dominance bound.
// tests/xy_bounds_check.cpp compiles this file alone, so it includes nothing of the library.
//
// Every product goes through xy_mul24: on the device the 24-bit multiplier (v_mul_i32_i24), on the host the low 32 bits of the product
// of the operands' sign-extended low 24 bits -- what that instruction computes, so a host build shows what the kernel would get, an
// operand that does not fit 24 bits included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_XY_HD __host__ __device__ __forceinline__
typedef int4 xy_int4;
#else
#define CNIIC_XY_HD inline
struct xy_int4 { int32_t x, y, z, w; };   // a centroid: (cx, cy, r << 16 | g << 8 | b, -|c|^2 or its id)
#endif

namespace cniic {

CNIIC_XY_HD int32_t xy_mul24(int32_t a, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    const int64_t a24 = (int64_t)(a & 0xffffff) - ((a & 0x800000) ? 0x1000000 : 0), b24 = (int64_t)(b & 0xffffff) - ((b & 0x800000) ? 0x1000000 : 0);
    return (int32_t)(uint32_t)(uint64_t)(a24 * b24);
#endif
}
CNIIC_XY_HD int32_t xy_max(int32_t a, int32_t b) { return a > b ? a : b; }

// floor(sum / m) for a centroid's coordinate: sum < 2^42 (a coordinate below 2^14 times at most 2^28 members), m < 2^32, quotient < 2^14.
// A SINGLE-precision estimate is within one of it (relative error 3 * 2^-24 on a value below 2^14) and is put right with one 32 x 32 -> 64
// product; two steps either way are allowed for.  (Until round 4: a double quotient and 64 x 64 products, five per changed centroid and
// 2048 centroids per block and launch -- the folded-in update's 2.5 us.)
CNIIC_XY_HD uint32_t xy_div_floor(unsigned long long sum, uint32_t m, float rm) {
    uint32_t e = (uint32_t)((float)sum * rm);
    unsigned long long em = (unsigned long long)e * m;
    if (em > sum) { e--; em -= m; if (em > sum) e--; }
    else if (em + m <= sum) { e++; em += m; if (em + m <= sum) e++; }
    return e;
}

struct Box5 { int32_t lo[5], hi[5]; };  // x, y, r, g, b extents

// squared distance from the box centre to a centroid
CNIIC_XY_HD uint32_t centre_dist(const Box5 &b, xy_int4 c) {
    int32_t d = 0;
    const int32_t v[5] = {c.x, c.y, (c.z >> 16) & 255, (c.z >> 8) & 255, c.z & 255};
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const int32_t e = v[i] - ((b.lo[i] + b.hi[i]) >> 1);
        d = xy_mul24(e, e) + d;
    }
    return (uint32_t)d;
}

// the pivot against one box: a[2 i] = c*_i - 2 lo_i, a[2 i + 1] = c*_i - 2 hi_i
struct Dominance {
    int32_t p[5], a[10];
    CNIIC_XY_HD void set(const Box5 &b, xy_int4 pv) {
        p[0] = pv.x; p[1] = pv.y; p[2] = (pv.z >> 16) & 255; p[3] = (pv.z >> 8) & 255; p[4] = pv.z & 255;
#pragma unroll
        for (int i = 0; i < 5; i++) { a[2 * i] = p[i] - 2 * b.lo[i]; a[2 * i + 1] = p[i] - 2 * b.hi[i]; }
    }
    // max over the box of d(p, pivot) - d(p, c): c can be nearest (or tie) somewhere in the box only if >= 0.
    // |c* - k| < 2^14 and |c* + k - 2p| < 2^15: 24-bit products, and the five terms sum below 2^31.
    CNIIC_XY_HD int32_t worst(xy_int4 c) const {
        const int32_t v[5] = {c.x, c.y, (c.z >> 16) & 255, (c.z >> 8) & 255, c.z & 255};
        int32_t f = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int32_t d = p[i] - v[i];
            f += xy_max(xy_mul24(d, v[i] + a[2 * i]), xy_mul24(d, v[i] + a[2 * i + 1]));
        }
        return f;
    }
};

}  // namespace cniic
