// huf_small.hpp -- what k_huf_small (k_delta_small.hip: `hufman` of a small frame on one workgroup) computes per frame where it differs from
// the `delta` instantiation of the same body, in plain functions for host and device.  tests/huf_small_check.cpp compiles this file (and
// delta_small.hpp, for the leaf order, the links, the merge and the longest code, none of which knows what a symbol is) alone, so it
// includes nothing else of the library.
//
// The statement to match is Hufman::encode (hufc.rs:12-17) -> huf::encode_all with the tree rule of DESIGN 2, D1 (huff_host.cpp): the
// symbols are the pixels in row-major order, a symbol's key is r << 16 | g << 8 | b, leaves ordered by (count, key).  The stream is
// u32 w, u32 h, the pre-order trie (a leaf: tag 0, u64 LE 3, r, g, b; a branch: tag 1), the payload MSB first, padded to a byte.
#pragma once
#include "delta_small.hpp"

namespace cniic {

constexpr uint32_t kHufSmallMaxPx = 16384;   // pixels (so symbols, and leaves at most) of a frame that takes the route
static_assert(kHufSmallMaxPx <= kDeltaSmallMaxPx, "delta_small.hpp's 14-bit fields and its longest code (an argument about counts alone) hold here");

// ---- the symbol: a pixel's three bytes as one ascending key
CNIIC_DS_HD uint32_t hs_key(uint8_t r, uint8_t g, uint8_t b) { return ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b; }

// the three bytes of the pixel a decoded key stands for (k_huf_small_dec: position d of the symbols is pixel d)
CNIIC_DS_HD void hs_pixel_bytes(uint32_t key, uint8_t *o) { o[0] = (uint8_t)(key >> 16); o[1] = (uint8_t)(key >> 8); o[2] = (uint8_t)key; }

// the eleven symbol bytes of a leaf: the length of the symbol as a little-endian u64 (3), then r, g, b (huff_host.cpp)
constexpr uint32_t kHufSmallLeafSym = 11;
CNIIC_DS_HD void hs_leaf_bytes(uint32_t key, uint8_t *o) {
    o[0] = 3;
    for (int i = 1; i < 8; i++) o[i] = 0;
    o[8] = (uint8_t)(key >> 16);
    o[9] = (uint8_t)(key >> 8);
    o[10] = (uint8_t)key;
}

// ---- sizes and offsets of the serialised trie (pre-order; a leaf is 1 + 11 bytes, a branch is 1)
CNIIC_DS_HD uint32_t hs_subtree_bytes(uint32_t leaves) { return 13 * leaves - 1; }   // leaves * 12 + (leaves - 1)
// ds_walk_step (delta_small.hpp) with this trie's subtree size
CNIIC_DS_HD void hs_walk_step(DsWalk &wk, uint32_t link, uint32_t leaves, uint32_t parent_leaves) {
    const uint32_t side = ds_link_side(link);
    wk.code |= side << wk.depth;
    wk.depth++;
    wk.off += 1 + (side ? hs_subtree_bytes(parent_leaves - leaves) : 0u);
}

// ---- the stream: u32 w, u32 h, the trie, the payload padded to a byte
CNIIC_DS_HD uint64_t hs_header_bytes(uint64_t U) { return 8 + hs_subtree_bytes((uint32_t)U); }
CNIIC_DS_HD uint64_t hs_stream_bytes(uint64_t U, uint64_t payload_bits) { return hs_header_bytes(U) + (payload_bits + 7) / 8; }
// what no stream of a frame of n pixels exceeds, rounded up to 16: n leaves and every symbol under the longest code (251 920 at 16 384)
CNIIC_DS_HD uint64_t hs_stride(uint64_t n) { return (hs_stream_bytes(n, (uint64_t)kDeltaSmallMaxCodeLen * n) + 15) & ~15ull; }

}  // namespace cniic
