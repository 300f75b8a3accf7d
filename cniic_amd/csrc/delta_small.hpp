// delta_small.hpp -- what k_delta_small (k_delta_small.hip: `delta` of a small frame on one workgroup) computes per frame beyond the
// symbols of delta_sym.hpp, in plain functions for host and device.  tests/delta_small_check.cpp compiles this file (and delta_sym.hpp)
// alone, so it includes nothing of the library.
//
// The statement to match is Delta::encode (hilbertc.rs:405-415) with the tree rule of DESIGN 2, D1 (huff_host.cpp): leaves ordered by
// (count, key), two-queue merge, the rarest first, a leaf before a branch among equals; Zero = left, One = right, MSB first.
//
// Names: a frame has n <= kDeltaSmallMaxPx symbols and U <= n distinct ones ("leaves").  Leaf q is the q-th in (count, key) order, branch
// j the j-th made (U - 1 of them, the last is the root).  A node's LINK is its parent branch and which child it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_DS_HD __host__ __device__ __forceinline__
#else
#define CNIIC_DS_HD inline
#endif

namespace cniic {

constexpr uint32_t kDeltaSmallMaxPx = 16384;   // pixels (so symbols, and leaves at most) of a frame that takes the route
constexpr uint32_t kDeltaSmallMinBound = 4096; // the bound is never lowered below this

// The longest code.  A Huffman tree (whatever its ties) whose deepest leaf has depth d carries a total count of at least F(d + 2), with
// F(1) = F(2) = 1 the Fibonacci numbers: on the path from that leaf to the root the sibling subtree at height i was not merged before
// the path's subtree of height i - 1 existed, so it weighs at least as much as the path's subtree of height i - 2, and the weights along
// the path grow at least like F.  F(21) = 10 946 <= 16 384 < 17 711 = F(22): d <= 19.  The bound is met under this tree rule: a chain
// needs every branch STRICTLY lighter than the leaf after next (a leaf goes first among equals), so counts 1, 1, 1, 3, 4, 7, 11, 18, ...
// (leaf k + 2 = branch k - 1 + 1, branch k = branch k - 1 + branch k - 2 + 1: 2, 3, 6, 10, 17, 28, ..., 15 126 at 20 leaves) give depth 19
// with 15 126 symbols, and depth 20 would take 24 475.  tests/delta_small_check.cpp builds that list and asserts both.
constexpr uint32_t kDeltaSmallMaxCodeLen = 19;
static_assert(kDeltaSmallMaxPx <= (1u << 14), "ranks, leaf and branch numbers are 14-bit fields below");
static_assert(kDeltaSmallMaxCodeLen <= 24, "a code and its length share a 32-bit word");

// ---- the leaf order: ascending (count, key).  rank = the key's position among the frame's ascending distinct keys, so sorting this word
// sorts by (count, key); count <= 16 384 takes 15 bits, rank 14
CNIIC_DS_HD uint32_t ds_leaf_order(uint32_t count, uint32_t rank) { return (count << 14) | rank; }
CNIIC_DS_HD uint32_t ds_order_count(uint32_t o) { return o >> 14; }
CNIIC_DS_HD uint32_t ds_order_rank(uint32_t o) { return o & 0x3fffu; }

// ---- links: parent branch (14 bits) | which child << 15.  A weight (<= 16 384, at most bit 14) and a link share a 16-bit slot: the slot
// of a node holds its weight until the merge takes it off its queue and its link from then on
CNIIC_DS_HD uint32_t ds_link(uint32_t parent, uint32_t side) { return parent | (side << 15); }
CNIIC_DS_HD uint32_t ds_link_parent(uint32_t l) { return l & 0x3fffu; }
CNIIC_DS_HD uint32_t ds_link_side(uint32_t l) { return l >> 15; }

// ---- the two-queue merge.  The leaf queue's head weighs lw (have_leaf: it is not empty), the branch queue's bw.
// One pick of the general step: the rarer head, the leaf among equals
CNIIC_DS_HD bool ds_pick_leaf(bool have_leaf, uint32_t lw, bool have_branch, uint32_t bw) { return have_leaf && (!have_branch || lw <= bw); }
// Runs.  While the SECOND leaf of the queue is no heavier than the branch queue's head, the two rarest are the first two leaves; the
// branches this makes are appended behind that head and are no lighter, so the head stays what it is and the test for the k-th next
// pair reads nothing the pairs before it write: a wave tests 64 pairs at once and takes the leading ones that pass.  (An EMPTY branch
// queue gets its head from the first pair: one pair, then look again.)  Likewise while the second branch is STRICTLY lighter than the
// leaf queue's head, the two rarest are the first two branches.
CNIIC_DS_HD bool ds_leaf_pair(uint32_t second_leaf_w, bool have_branch, uint32_t bw) { return !have_branch || second_leaf_w <= bw; }
CNIIC_DS_HD bool ds_branch_pair(uint32_t second_branch_w, bool have_leaf, uint32_t lw) { return !have_leaf || second_branch_w < lw; }

// ---- sizes and offsets of the serialised trie (pre-order; a leaf is 0 + three little-endian i16 = 7 bytes, a branch is 1)
CNIIC_DS_HD uint32_t ds_subtree_bytes(uint32_t leaves) { return 8 * leaves - 1; }   // leaves * 7 + (leaves - 1)
// One step of a node's walk to the root, from a node with `leaves` leaves below it (1 for a leaf) through `link` to its parent, below which
// parent_leaves lie: the node's code gets its next bit (the walk meets the LAST bit first), its pre-order offset the parent's tag and, for
// a right child, the left sibling's subtree
struct DsWalk { uint32_t depth = 0, code = 0, off = 0; };
CNIIC_DS_HD void ds_walk_step(DsWalk &wk, uint32_t link, uint32_t leaves, uint32_t parent_leaves) {
    const uint32_t side = ds_link_side(link);
    wk.code |= side << wk.depth;
    wk.depth++;
    wk.off += 1 + (side ? ds_subtree_bytes(parent_leaves - leaves) : 0u);
}
// a symbol's code and length as the payload phase keeps them
CNIIC_DS_HD uint32_t ds_codeword(uint32_t code, uint32_t len) { return code | (len << 24); }
CNIIC_DS_HD uint32_t ds_codeword_len(uint32_t cw) { return cw >> 24; }
CNIIC_DS_HD uint32_t ds_codeword_code(uint32_t cw) { return cw & 0xffffffu; }

// the six symbol bytes of a leaf: the key's three 9-bit fields minus 255 as little-endian i16 (hilbertc.rs:561-565)
CNIIC_DS_HD void ds_leaf_bytes(uint32_t key, uint8_t *o) {
    for (int i = 0; i < 3; i++) {
        const uint16_t u = (uint16_t)(int16_t)((int32_t)((key >> (18 - 9 * i)) & 511u) - 255);
        o[2 * i] = (uint8_t)u;
        o[2 * i + 1] = (uint8_t)(u >> 8);
    }
}

// ---- the stream: u32 w, u32 h, the trie, the payload padded to a byte
CNIIC_DS_HD uint64_t ds_header_bytes(uint64_t U) { return 8 + ds_subtree_bytes((uint32_t)U); }
CNIIC_DS_HD uint64_t ds_stream_bytes(uint64_t U, uint64_t payload_bits) { return ds_header_bytes(U) + (payload_bits + 7) / 8; }
// what no stream of a frame of n pixels exceeds, rounded up to 16: n leaves and every symbol under the longest code
CNIIC_DS_HD uint64_t ds_stride(uint64_t n) { return (ds_stream_bytes(n, (uint64_t)kDeltaSmallMaxCodeLen * n) + 15) & ~15ull; }

}  // namespace cniic
