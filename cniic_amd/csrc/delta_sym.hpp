// delta_sym.hpp -- the symbol arithmetic of the `delta` encoder's 16-bit stream (k_delta.hip), in plain functions for host and device.
// tests/delta_sym_check.cpp compiles this file alone, so it includes nothing of the library.
//
// A symbol is the difference of two neighbouring pixels of the scan, three channels in [-255, 255].  It has three forms:
//   key     the packed SignedColor (dr + 255) << 18 | (dg + 255) << 9 | (db + 255): what the Huffman stage counts and codes (27 bits)
//   index   inside the cube [-16, 15]^3 ("hot"): (dr + 16) << 10 | (dg + 16) << 5 | (db + 16), the 16-bit stream's word
//   fields  the tile gather's word: three 10-bit fields  db + 528 | (dg + 528) << 10 | (dr + 528) << 20, the ONE subtraction of two
//           pixels' field words plus kC (no borrow between the fields: each is in [273, 783])
// and the kernels go from one to the other four ways (fields -> index / key in k_delta_gather_p2, pixels -> key + index in
// k_delta_gather_any, index -> key in k_delta_hist16, key -> index in k_delta_fill_codes): all of them are here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_DSYM_HD __host__ __device__ __forceinline__
#else
#define CNIIC_DSYM_HD inline
#endif

namespace cniic {

constexpr uint32_t kHot = 32 * 32 * 32;
constexpr uint32_t kCold16 = 0x8000u, kPad16 = 0x8040u;  // kCold16 + r, r < 64

// DiffStream::next (hilbertc.rs:458-476) on two r | g << 8 | b << 16 pixels: the packed SignedColor key and the cube index
CNIIC_DSYM_HD uint32_t delta_key(uint32_t px, uint32_t prev, uint32_t &hot) {
    const int32_t dr = (int32_t)(px & 255) - (int32_t)(prev & 255), dg = (int32_t)((px >> 8) & 255) - (int32_t)((prev >> 8) & 255),
                  db = (int32_t)((px >> 16) & 255) - (int32_t)((prev >> 16) & 255);
    const uint32_t hr = (uint32_t)(dr + 16), hg = (uint32_t)(dg + 16), hb = (uint32_t)(db + 16);
    hot = (hr | hg | hb) < 32u ? (hr << 10) | (hg << 5) | hb : kCold16;
    return ((uint32_t)(dr + 255) << 18) | ((uint32_t)(dg + 255) << 9) | (uint32_t)(db + 255);
}
CNIIC_DSYM_HD uint32_t hot_to_key(uint32_t i) {
    return (((i >> 10) + 255 - 16) << 18) | ((((i >> 5) & 31) + 255 - 16) << 9) | ((i & 31) + 255 - 16);
}
// the other way: true and the cube index when the key lies inside the cube
CNIIC_DSYM_HD bool key_to_hot(uint32_t k, uint32_t &hx) {
    const uint32_t hr = (k >> 18) - (255 - 16), hg = ((k >> 9) & 511) - (255 - 16), hb = (k & 511) - (255 - 16);
    hx = (hr << 10) | (hg << 5) | hb;
    return (hr | hg | hb) < 32u;
}

// three 10-bit fields per pixel, so that ONE subtraction gives the three differences
constexpr uint32_t kField = 528;                                      // c - p + 528 in [273, 783]: ten bits, never negative
constexpr uint32_t kFields = 1u | (1u << 10) | (1u << 20);
constexpr uint32_t kC = kField * kFields, kMask = 0x3e0u * kFields, kHotBits = 0x200u * kFields;
CNIIC_DSYM_HD uint32_t px_fields(uint32_t px) {                      // r | g << 8 | b << 16 (bits 24..31: anything)
    return ((px >> 16) & 255u) + (((px >> 8) & 255u) << 10) + ((px & 255u) << 20) + kField * kFields;
}
CNIIC_DSYM_HD uint32_t fields_diff(uint32_t t, uint32_t prev) { return t - prev + kC; }  // of two px_fields words: fields c - p + 528
CNIIC_DSYM_HD bool fields_cold(uint32_t d) { return (d & kMask) != kHotBits; }            // some field outside [512, 543]
CNIIC_DSYM_HD uint32_t fields_hot(uint32_t d) { return ((d >> 10) & 0x7c00u) | ((d >> 5) & 0x3e0u) | (d & 31u); }
CNIIC_DSYM_HD uint32_t fields_key(uint32_t dd) {
    return ((((dd >> 20) & 1023u) - (kField - 255)) << 18) | ((((dd >> 10) & 1023u) - (kField - 255)) << 9) | ((dd & 1023u) - (kField - 255));
}

}  // namespace cniic
