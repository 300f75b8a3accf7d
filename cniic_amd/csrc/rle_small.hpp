// rle_small.hpp -- what k_rle_small (k_rle_small.hip: `hilbert(rle)` / `hilbert(rle(d))` of a small frame on one workgroup) computes per
// frame, in plain functions for host and device, and the accept test it shares with the large encoder (k_rle_approx.hip, whose head
// comment argues the exactness of every step).  tests/rle_small_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The statement to match is Hilbert { compress: RLE(d) }::encode (hilbertc.rs:26-45): u32 w, u32 h, then per run count:u8 and the colour
// as u64 LE 3 + r, g, b.  A pixel joins the open run while the run has fewer than 255 elements and, d == 0: it equals the run's first
// colour (rle_exact); d != 0: its distance to the run's running average is <= d (rle_approx + Approx + RunningAvg, :200-299), and the
// colour is then round(sum / count) per channel.
//
// Names: a frame has n <= kRleSmallMaxPx pixels along the scan, a pixel's key is r << 16 | g << 8 | b.  L(i) is the length of the run
// that WOULD start at position i; it depends on the keys i .. i + 254 alone.  The true run starts are the chain 0, L(0), L(0) + L(L(0)), ...
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_RS_HD __host__ __device__ __forceinline__
#else
#define CNIIC_RS_HD inline
#endif
// the squares and the adds of the accept test must not fuse (hipcc's default is -ffp-contract=fast-honor-pragmas: the pragma inside the
// function; GCC takes the setting as a function attribute)
#if defined(__GNUC__) && !defined(__clang__)
#define CNIIC_RS_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define CNIIC_RS_NO_CONTRACT
#endif

namespace cniic {

constexpr uint32_t kRleSmallMaxPx = 16384;   // pixels of a frame that takes the route
constexpr uint32_t kRleSmallMaxRun = 255;    // RepCount::MAX (hilbertc.rs:23,130)
constexpr uint32_t kRleSmallPiece = 256;     // positions whose chain one lane marks (k_rle_small phase c); a run crosses at most one border

CNIIC_RS_HD uint32_t rs_key(uint8_t r, uint8_t g, uint8_t b) { return ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b; }

// ---- the accept test: Approx::accept for a run of `count` pixels with channel sums s0 s1 s2 and the next pixel's key x, in IEEE f64 as
// the reference computes it, against T(d) in place of the square root
CNIIC_RS_NO_CONTRACT CNIIC_RS_HD bool rla_accept(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t count, uint32_t x, double T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double c = (double)count;
    const double d0 = (double)s0 / c - (double)((x >> 16) & 255u);
    const double d1 = (double)s1 / c - (double)((x >> 8) & 255u);
    const double d2 = (double)s2 / c - (double)(x & 255u);
    const double s = (d0 * d0 + d1 * d1) + d2 * d2;
    return s <= T;
}

// ---- the threshold: sqrt_rn is monotone, so sqrt_rn(s) <= d  <=>  s <= T(d), T(d) the largest double whose correctly rounded square
// root is <= d (binary search over the bit patterns of the non-negative doubles, which sort as the values do; the host's sqrt is IEEE).
// -1 for d < 0 or NaN: no distance is accepted.  +inf for +inf.  Host only.
inline double rla_threshold_of(double d) {
    if (!(d >= 0.0)) return -1.0;
    if (isinf(d)) return d;
    uint64_t lo = 0, hi = 0x7ff0000000000000ull;   // sqrt(lo) = 0 <= d; sqrt(+inf) > d
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        double v;
        memcpy(&v, &mid, 8);
        if (sqrt(v) <= d) lo = mid;
        else hi = mid;
    }
    double t;
    memcpy(&t, &lo, 8);
    return t;
}

// ---- the modes: 0 = the test (T >= 0), 1 = nothing is accepted (T < 0: d < 0 or NaN), 2 = everything is (T >= 3 * 255^2: no distance
// reaches it -- avg_c and x_c lie in [0, 255], so each rounded square is <= 65025 and their rounded sum <= 195075).  The small route
// adds 3 = the exact codec (d == 0, either sign): equality with the run's first colour, no arithmetic.
constexpr int kRlaModeTest = 0, kRlaModeNone = 1, kRlaModeAll = 2, kRsModeExact = 3;
CNIIC_RS_HD int rla_mode(double T) { return T < 0.0 ? kRlaModeNone : T >= 3.0 * 255.0 * 255.0 ? kRlaModeAll : kRlaModeTest; }
CNIIC_RS_HD int rs_mode(double d, double T) { return d == 0.0 ? kRsModeExact : rla_mode(T); }

// ---- the cap: a run that starts at i has at most 255 elements and ends with the frame
CNIIC_RS_HD uint32_t rs_cap(uint32_t i, uint32_t n) { return n - i < kRleSmallMaxRun ? n - i : kRleSmallMaxRun; }

// ---- L(i): k_rla_len_maps' rule.  The pixels equal to key[i] that follow it keep the average at key[i]: distance 0, accepted without
// arithmetic (d >= 0).  From the first that differs on, the test.
CNIIC_RS_HD uint32_t rs_run_len(const uint32_t *key, uint32_t i, uint32_t n, double T, int mode) {
    const uint32_t lim = rs_cap(i, n);
    if (mode == kRlaModeNone) return 1;
    if (mode == kRlaModeAll) return lim;
    const uint32_t k0 = key[i];
    uint32_t len = 1;
    while (len < lim && key[i + len] == k0) len++;
    if (mode == kRsModeExact || len == lim) return len;
    uint32_t s0 = ((k0 >> 16) & 255u) * len, s1 = ((k0 >> 8) & 255u) * len, s2 = (k0 & 255u) * len;
    while (len < lim) {
        const uint32_t x = key[i + len];
        if (!rla_accept(s0, s1, s2, len, x, T)) break;
        s0 += (x >> 16) & 255u; s1 += (x >> 8) & 255u; s2 += x & 255u;
        len++;
    }
    return len;
}

// ---- the rounding: f64::round(sum / count), halves away from zero, in integers (k_rle_approx.hip: the f64 quotient cannot round onto or
// across a half)
CNIIC_RS_HD uint32_t rs_round(uint32_t sum, uint32_t count) { return (2 * sum + count) / (2 * count); }

// ---- the record: count:u8, the u64 little-endian 3, r, g, b = 12 bytes = three little-endian words
CNIIC_RS_HD void rs_record_words(uint32_t count, uint32_t r, uint32_t g, uint32_t b, uint32_t *w) {
    w[0] = count | (3u << 8);
    w[1] = 0u;
    w[2] = (r << 8) | (g << 16) | (b << 24);
}

// ---- the stream: u32 w, u32 h, the records; a slot holds a run per pixel, rounded up to 16 (196 624 at 16 384)
CNIIC_RS_HD uint64_t rs_stream_bytes(uint64_t runs) { return 8 + 12 * runs; }
CNIIC_RS_HD uint64_t rs_stride(uint64_t n) { return (8 + 12 * n + 15) & ~15ull; }

}  // namespace cniic
