// small_trie.hpp -- what k_small_trieparse (k_small_trie.hip: the parse of a small frame's serialised decoder on one workgroup) computes per
// frame that can be stated without the GPU, in plain functions for host and device.  tests/small_trie_check.cpp compiles this file (and
// delta_small_dec.hpp, for the table's words) alone, so it includes nothing else of the library.
//
// The statement to match is huff_parse_leaves (huff_host.cpp; Dec::deserialize, huf.rs:323-348): the trie in pre-order, a record per
// node -- tag 1: a branch, 1 byte; tag 0: a leaf, 1 + S bytes.  S = 6 is a SignedColor (three little-endian i16 in -255..255, get_symbol):
// the leaf of a `delta` stream.  S = 11 is an Rgb<u8> (a little-endian u64 that must be 3, then r, g, b): the leaf of a `hufman` stream and of
// a `cluster-colors` stream.  S is a template parameter throughout, and what follows from it -- the map's word, a lane's chunks, the symbol
// check -- is stated per S below (StMap<S>, st_max_k<S>, StLeafKey<S>); tests/small_trie_rgb_check.cpp is small_trie_check.cpp's S = 11 twin.
//
// Names.  The trie's bytes (the stream behind its 8-byte header) are looked at as far as the WINDOW reaches: M = min(stream bytes,
// st_max_bytes) -- a decoder of at most kSmallTrieMaxLeaves leaves has that many bytes at the most, and a record is read only when it
// lies in the window whole.  The window is cut into CHUNKS of kStChunk = 32 bytes, so that a chunk's tags are two 32-bit masks (which
// bytes are a 1, which are a 0) and a walk through it runs in registers; a LANE owns K = 1 .. 4 consecutive chunks (1 .. 7 for S = 11; K the
// least that gives 1024 lanes the window).  A walk that enters a chunk at offset o in 0 .. S (the first record starts o bytes in) leaves it at an offset of
// the next one, or STOPS at a byte that starts no record (a tag other than 0 / 1, the window's end): the R = S + 1 exits are a MAP in one
// word, R fields of 3 bits (S = 11: 12 fields of 4 bits in a 64-bit word), the value R meaning stopped.  Composing maps is associative, so a scan gives every lane its true entry.
// P of a node = the subtrees still open in front of it = branches - leaves among the earlier nodes; the trie ends behind the first leaf
// met with P = 0 (node E).  Node k + 1 is the left child of branch k; the node behind a leaf is the right child of the last earlier node
// with its own P.  A RUN is a leaf and the branches straight in front of it (a left spine: every node the left child of the one before),
// so run i ends in leaf i and starts behind leaf i - 1; depth(node k of run i) = A[i] + k with A[i] = A[r] + (b + 1 - head_i), b the
// parent of the run's head and r b's run: a chain over at most 16 384 runs that pointer jumping resolves, in at most 5 rounds when no
// leaf lies deeper than 19 (a chain link is a right turn, and 2^5 > 19).
#pragma once
#include <stdint.h>
#include "delta_small_dec.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_ST_HD __host__ __device__ __forceinline__
#else
#define CNIIC_ST_HD inline
#endif

namespace cniic {

constexpr uint32_t kSmallTrieMaxLeaves = 16384;   // leaves of a decoder the kernel finishes: no encoder makes more leaves than pixels
constexpr uint32_t kStLanes = 1024;               // lanes of the workgroup
constexpr uint32_t kStChunk = 32;                 // bytes of a chunk: its tags are two 32-bit masks
constexpr uint32_t kStMaxK = 4;                   // chunks of a lane at the bound (S = 6)
constexpr uint32_t kStMaxKRgb = 7;                // and for S = 11: 7 * 1024 * 32 = 229 376 >= 212 991
template <uint32_t S> constexpr uint32_t st_max_k() { return S == 6 ? kStMaxK : kStMaxKRgb; }
constexpr uint32_t kStMaxP = kDeltaSmallMaxCodeLen;   // P of a node is at most its depth: rows 0 .. kStMaxP of the table of last nodes
constexpr uint32_t kStJumpRounds = 5;             // 2^5 > kDeltaSmallMaxCodeLen links of a chain of runs
static_assert(kSmallTrieMaxLeaves == kDeltaSmallDecMaxPx, "a decoder of a routed frame has no more leaves than the frame has pixels");
static_assert((1u << kStJumpRounds) > kDeltaSmallMaxCodeLen, "the jump rounds reach the root from every leaf the route takes");

// verdicts of a frame (3: the header alone said that the frame is not the route's -- its size, an injected scan, too short a stream)
constexpr uint32_t kStParsed = 0, kStNotDecoder = 1, kStNotOurs = 2, kStSkipped = 3;

template <uint32_t S> constexpr uint32_t st_max_bytes() { return (S + 2) * kSmallTrieMaxLeaves - 1; }   // L leaves, L - 1 branches
static_assert((st_max_bytes<6>() + kStChunk - 1) / kStChunk <= kStMaxK * kStLanes, "1024 lanes of 4 chunks hold the largest window");
static_assert(st_max_bytes<11>() == 212991 && (st_max_bytes<11>() + kStChunk - 1) / kStChunk <= kStMaxKRgb * kStLanes, "1024 lanes of 7 chunks hold the largest window of Rgb leaves");
CNIIC_ST_HD uint32_t st_window(uint64_t trie_bytes, uint32_t max_bytes) { return (uint32_t)(trie_bytes < max_bytes ? trie_bytes : max_bytes); }
CNIIC_ST_HD uint32_t st_chunks(uint32_t window) { return (window + kStChunk - 1) / kStChunk; }
CNIIC_ST_HD uint32_t st_lane_chunks(uint32_t window) { const uint32_t k = (st_chunks(window) + kStLanes - 1) / kStLanes; return k ? k : 1; }
CNIIC_ST_HD uint32_t st_lanes_used(uint32_t window) { return (st_chunks(window) + st_lane_chunks(window) - 1) / st_lane_chunks(window); }
// leaves a stream of `bytes` bytes (header included) has room for: 8 + (S + 2) L - 1 <= bytes
template <uint32_t S> CNIIC_ST_HD uint32_t st_leaves_room(uint64_t bytes) {
    const uint64_t l = bytes >= 8 + S + 1 ? (bytes - 7) / (S + 2) : 0;
    return (uint32_t)(l < kSmallTrieMaxLeaves ? l : kSmallTrieMaxLeaves);
}

// ---- a chunk's masks from its bytes as 8 little-endian words (byte j of the chunk is bits 8 (j & 3) .. of word j / 4): bit j of br = byte
// j is a 1 and lies in the window, bit j of lf = byte j is a 0 and a leaf that starts there ends in the window.  `at`: the chunk's first byte
CNIIC_ST_HD uint32_t st_byte_is_zero(uint32_t x) {   // bit j: byte j of x is 0
    const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu), y = t >> 7;
    return (y | (y >> 7) | (y >> 14) | (y >> 21)) & 15u;
}
CNIIC_ST_HD uint32_t st_low_bits(uint32_t n) { return n >= 32 ? 0xffffffffu : (1u << n) - 1u; }
template <uint32_t S> CNIIC_ST_HD void st_masks(const uint32_t w[8], uint32_t at, uint32_t window, uint32_t &br, uint32_t &lf) {
    br = 0; lf = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        br |= st_byte_is_zero(w[i] ^ 0x01010101u) << (4 * i);
        lf |= st_byte_is_zero(w[i]) << (4 * i);
    }
    br &= st_low_bits(window > at ? window - at : 0);
    lf &= st_low_bits(window >= at + S + 1 ? window - S - at : 0);
}

// ---- maps: field o = the exit of a walk that enters at o; the value R = S + 1 is "stopped", and stopped stays stopped.  The fields' width and
// the word follow from S: 7 fields of 3 bits in 32 bits for S = 6, 12 fields of 4 bits (48 bits) in 64 for S = 11
constexpr uint32_t kStMapBits = 3;   // S = 6
template <uint32_t S> struct StMap;
template <> struct StMap<6> { typedef uint32_t word; static constexpr uint32_t bits = kStMapBits; };
template <> struct StMap<11> { typedef uint64_t word; static constexpr uint32_t bits = 4; };
template <uint32_t S> CNIIC_ST_HD uint32_t st_map_get(typename StMap<S>::word m, uint32_t o) {
    return o > S ? S + 1 : (uint32_t)(m >> (StMap<S>::bits * o)) & ((1u << StMap<S>::bits) - 1u);
}
template <uint32_t S> CNIIC_ST_HD typename StMap<S>::word st_map_identity() {
    typedef typename StMap<S>::word W;
    static_assert(S + 1 < (1u << StMap<S>::bits) && (S + 1) * StMap<S>::bits <= 8 * sizeof(W), "R exits and the stopped value fit the fields, the fields one word");
    W m = 0;
    for (uint32_t o = 0; o <= S; o++) m |= (W)o << (StMap<S>::bits * o);
    return m;
}
// first a, then b
template <uint32_t S> CNIIC_ST_HD typename StMap<S>::word st_map_compose(typename StMap<S>::word a, typename StMap<S>::word b) {
    typedef typename StMap<S>::word W;
    W m = 0;
#pragma unroll
    for (uint32_t o = 0; o <= S; o++) m |= (W)st_map_get<S>(b, st_map_get<S>(a, o)) << (StMap<S>::bits * o);
    return m;
}

// ---- a lane: its chunks' masks, its first byte, and (after the scans) where the true walk enters it, the nodes and leaves in front of it
template <uint32_t MAXK> struct StLaneK {
    static constexpr uint32_t kMaxK = MAXK;
    uint32_t br[MAXK], lf[MAXK];
    uint32_t K, at, entry, nodes_before, leaves_before;
};
typedef StLaneK<kStMaxK> StLane;         // S = 6
typedef StLaneK<kStMaxKRgb> StLaneRgb;   // S = 11
constexpr uint32_t kStNoStop = 0xffffffffu;
// The walk through a lane's chunks from its entry: visit(byte offset of the record, is it a leaf) for every node, until visit says false,
// the chunks end or the walk stops.  -> the byte at which it stopped (kStNoStop: it did not); *exit = the offset into the next lane's
// first chunk (S + 1: stopped, or visit ended it).  Every step advances by a record of at least one byte.
template <uint32_t S, class LN, class F> CNIIC_ST_HD uint32_t st_lane_walk(const LN &ln, uint32_t entry, uint32_t *exit, F &&visit) {
    uint32_t o = entry, stopped = kStNoStop;
#pragma unroll
    for (uint32_t k = 0; k < LN::kMaxK; k++) {
        if (k < ln.K && o <= S) {
            const uint32_t br = ln.br[k], lf = ln.lf[k];
            uint32_t pos = o;
            o = S + 1;
            while (pos < kStChunk) {
                const bool leaf = (lf >> pos) & 1u;
                if (!leaf && !((br >> pos) & 1u)) { stopped = ln.at + kStChunk * k + pos; break; }
                if (!visit(ln.at + kStChunk * k + pos, leaf)) break;
                pos += leaf ? S + 1 : 1;
            }
            if (pos >= kStChunk) o = pos - kStChunk;
        }
    }
    if (exit) *exit = o;
    return stopped;
}
// phase 1: the lane's map
template <uint32_t S, class LN> CNIIC_ST_HD typename StMap<S>::word st_lane_map(const LN &ln) {
    typename StMap<S>::word m = 0;
#pragma unroll
    for (uint32_t o = 0; o <= S; o++) {
        uint32_t e;
        (void)st_lane_walk<S>(ln, o, &e, [](uint32_t, bool) { return true; });
        m |= (typename StMap<S>::word)e << (StMap<S>::bits * o);
    }
    return m;
}
// phase 2: the true walk's nodes and leaves in the lane, whether its last node is a leaf, and where it stopped
template <uint32_t S, class LN> CNIIC_ST_HD uint32_t st_lane_count(const LN &ln, uint32_t &nodes, uint32_t &leaves, uint32_t &last_leaf) {
    uint32_t n = 0, l = 0, last = 0;
    const uint32_t stop = st_lane_walk<S>(ln, ln.entry, nullptr, [&](uint32_t, bool leaf) { n++; l += leaf; last = leaf; return true; });
    nodes = n; leaves = l; last_leaf = last;
    return stop;
}

// ---- the table of last nodes: word = (node + 1) << 15 | the node's run (= leaves in front of it); 0 = none.  Later nodes have larger words,
// so "the last earlier node with this P" over lanes is a prefix maximum per row.  tab[p * pitch + lane]
// The word has 17 bits for node + 1, which a window of S = 6 never exceeds (the first assert below).  A window of S = 11 can hold 212 991 nodes
// -- branches only, or payload bytes behind the trie's end that read as tags --, so st_lane_open writes NO word for a node above
// kStLastNodeMax = 2 kSmallTrieMaxLeaves - 2, for either S.  Nothing that is read misses such a word: a frame that goes on past phase 3 has
// L = E / 2 + 1 <= room <= kSmallTrieMaxLeaves leaves, so E <= kStLastNodeMax; phase 4 reads a slot only for the parent of a head <= E, which
// is a node < E, and the exclusive prefix maximum carries a word only to lanes behind its own, so the words of nodes above E reach lanes that
// hold nothing but nodes above E, where st_lane_runs reads nothing.  The words that are written have node + 1 < 2^15 and run <= node < 2^15
CNIIC_ST_HD uint32_t st_last_word(uint32_t node, uint32_t run) { return ((node + 1) << 15) | run; }
CNIIC_ST_HD uint32_t st_last_node1(uint32_t w) { return w >> 15; }   // node + 1
CNIIC_ST_HD uint32_t st_last_run(uint32_t w) { return w & 0x7fffu; }
static_assert(st_max_bytes<6>() + 1 <= (1u << 17) && st_max_bytes<6>() / 7 < (1u << 15), "a window's nodes and leaves fit the word");
constexpr uint32_t kStLastNodeMax = 2 * kSmallTrieMaxLeaves - 2;   // the last node (leaf E) of the largest trie the kernel finishes
static_assert(kStLastNodeMax + 1 < (1u << 15) && ((uint64_t)(kStLastNodeMax + 1) << 15 | kStLastNodeMax) < (1ull << 32), "the words st_lane_open writes fit 32 bits for every S");
constexpr uint32_t kStNone = 0xffffffffu;
// phase 3: P of the lane's nodes; the last node of every P <= kStMaxP into the lane's column; -> *end = the lane's first leaf with P = 0 (a
// node index, kStNone: none), *deep = its first node with P above kStMaxP.  Nothing behind the lane's first such leaf is the trie's.
template <uint32_t S, class LN> CNIIC_ST_HD void st_lane_open(const LN &ln, uint32_t *tab, uint32_t pitch, uint32_t lane, uint32_t *end, uint32_t *deep) {
    uint32_t node = ln.nodes_before, run = ln.leaves_before, e = kStNone, d = kStNone;
    int32_t P = (int32_t)ln.nodes_before - 2 * (int32_t)ln.leaves_before;
    (void)st_lane_walk<S>(ln, ln.entry, nullptr, [&](uint32_t, bool leaf) {
        if (P < 0) return false;
        if (P > (int32_t)kStMaxP) { if (d == kStNone) d = node; }
        else if (node <= kStLastNodeMax) tab[(uint32_t)P * pitch + lane] = st_last_word(node, run);
        if (leaf && P == 0) { e = node; return false; }
        if (leaf) { run++; P--; } else P++;
        node++;
        return true;
    });
    *end = e; *deep = d;
}

// ---- runs: word = the run jumped to (14 bits) | a signed sum << 14 (18 bits).  Every word states a fact -- "A[i] = A[jump] + sum" -- so a
// jump that reads a target another lane has already moved on is still right.  Only runs of nodes <= E <= kStLastNodeMax get a word: the
// fields depend on node counts alone, not on S
CNIIC_ST_HD uint32_t st_run_word(uint32_t jump, int32_t sum) { return jump | ((uint32_t)sum << 14); }
CNIIC_ST_HD uint32_t st_run_jump(uint32_t w) { return w & 0x3fffu; }
CNIIC_ST_HD int32_t st_run_sum(uint32_t w) { return (int32_t)w >> 14; }
CNIIC_ST_HD uint32_t st_run_hop(uint32_t mine, uint32_t target) { return st_run_word(st_run_jump(target), st_run_sum(mine) + st_run_sum(target)); }
static_assert(kSmallTrieMaxLeaves <= (1u << 14) && 4 * kSmallTrieMaxLeaves < (1u << 17), "a run's index and every sum of node distances fit the word");
// phase 4 (the table now holds, per lane, the last node of every P in front of the lane): the lane's runs that start at nodes <= E.
// head: is the lane's first node behind a leaf (or the root).  -> *pay = the byte behind leaf E when the lane holds it; false: a head without
// a parent (cannot be in a trie that ended at E with P <= kStMaxP throughout; the caller gives the frame up)
template <uint32_t S, class LN> CNIIC_ST_HD bool st_lane_runs(const LN &ln, bool head, uint32_t E, uint32_t *tab, uint32_t pitch, uint32_t lane, uint32_t *runs, uint32_t *pay) {
    uint32_t node = ln.nodes_before, run = ln.leaves_before;
    int32_t P = (int32_t)ln.nodes_before - 2 * (int32_t)ln.leaves_before;
    bool ok = true;
    (void)st_lane_walk<S>(ln, ln.entry, nullptr, [&](uint32_t pos, bool leaf) {
        if (node > E) return false;
        if (P < 0 || P > (int32_t)kStMaxP) { ok = false; return false; }   // (not for a node up to E: the caller has seen to it)
        uint32_t *slot = tab + (uint32_t)P * pitch + lane;
        if (head) {
            if (node == 0) runs[0] = st_run_word(0, 0);
            else {
                const uint32_t w = *slot;
                if (!w) ok = false;
                else runs[run] = st_run_word(st_last_run(w), (int32_t)st_last_node1(w) - (int32_t)node);
            }
        }
        *slot = st_last_word(node, run);
        head = leaf;
        if (leaf && node == E) *pay = pos + S + 1;
        if (leaf) { run++; P--; } else P++;
        node++;
        return true;
    });
    return ok;
}

// ---- codes: leaves in pre-order have ascending left-aligned codes, code[0] = 0 and code[i + 1] = code[i] + 2^(32 - len[i]) (modulo 2^32: the
// sum over all leaves is exactly 2^32, and a single leaf of length 0 adds 2^32 as well)
CNIIC_ST_HD uint32_t st_code_step(uint32_t len) { return len ? 1u << (32 - len) : 0u; }
// phase 5: the lengths of the lane's leaves up to E (A[i] + node) -> their steps' sum and the longest; false: one lies deeper than kDeltaSmallMaxCodeLen
template <uint32_t S, class LN> CNIIC_ST_HD bool st_lane_lens(const LN &ln, uint32_t E, const uint32_t *runs, uint32_t *sum, uint32_t *longest) {
    uint32_t node = ln.nodes_before, run = ln.leaves_before, s = 0, m = 0;
    bool ok = true;
    (void)st_lane_walk<S>(ln, ln.entry, nullptr, [&](uint32_t, bool leaf) {
        if (node > E) return false;
        if (leaf) {
            const int32_t len = st_run_sum(runs[run]) + (int32_t)node;
            if (len < 0 || len > (int32_t)kDeltaSmallMaxCodeLen) { ok = false; return false; }
            s += st_code_step((uint32_t)len);
            m = (uint32_t)len > m ? (uint32_t)len : m;
            run++;
        }
        node++;
        return true;
    });
    *sum = s; *longest = m;
    return ok;
}
// get_symbol for S = 6 from the six bytes as a little-endian number: three i16 in -255 .. 255 -> the key, (v + 255) in 9-bit fields, red on top
CNIIC_ST_HD bool st_symbol6(uint64_t six, uint32_t *key) {
    uint32_t k = 0;
    bool ok = true;
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) {
        const int32_t v = (int16_t)(uint16_t)(six >> (16 * i));
        ok = ok && v >= -255 && v <= 255;
        k = (k << 9) | ((uint32_t)(v + 255) & 511u);
    }
    *key = k;
    return ok;
}
// get_symbol for S = 11 (CNIIC_SYM_RGB): the u64 in front must be 3; rgb = the three bytes behind it as a little-endian number -> hs_key
CNIIC_ST_HD bool st_symbol11(uint64_t len, uint32_t rgb, uint32_t *key) {
    *key = ((rgb & 0xffu) << 16) | (rgb & 0xff00u) | ((rgb >> 16) & 0xffu);
    return len == 3;
}
struct StRgbLeaf { uint64_t len; uint32_t rgb; };   // what a reader of S = 11 returns: bytes 0 .. 7 and 8 .. 10 of the symbol, little-endian
template <uint32_t S> struct StLeafKey;
template <> struct StLeafKey<6> { template <class R> static CNIIC_ST_HD bool get(R &&rd, uint32_t pos, uint32_t *key) { return st_symbol6(rd(pos), key); } };
template <> struct StLeafKey<11> {
    template <class R> static CNIIC_ST_HD bool get(R &&rd, uint32_t pos, uint32_t *key) { const StRgbLeaf l = rd(pos); return st_symbol11(l.len, l.rgb, key); }
};
// phase 6: the table's words of the lane's leaves up to E -- code[i] at table[i], dsd_keylen(key, len) at table[L + i] -- from the code of the
// lane's first leaf.  rd(pos): the symbol's bytes at trie offset pos -- S = 6: the six bytes as a little-endian number; S = 11: an StRgbLeaf.
// false: a symbol that get_symbol refuses (outside -255 .. 255; a length other than 3)
template <uint32_t S, class LN, class R> CNIIC_ST_HD bool st_lane_table(const LN &ln, uint32_t E, const uint32_t *runs, uint32_t code, uint32_t L, uint32_t *table, R &&rd) {
    uint32_t node = ln.nodes_before, run = ln.leaves_before;
    bool ok = true;
    (void)st_lane_walk<S>(ln, ln.entry, nullptr, [&](uint32_t pos, bool leaf) {
        if (node > E) return false;
        if (leaf) {
            const uint32_t len = (uint32_t)(st_run_sum(runs[run]) + (int32_t)node);
            uint32_t key;
            ok = StLeafKey<S>::get(rd, pos + 1, &key) && ok;
            table[run] = code;
            table[L + run] = dsd_keylen(key, len);
            code += st_code_step(len);
            run++;
        }
        node++;
        return true;
    });
    return ok;
}

// ---- the verdict.  Structure first: the walk from byte 0 ends at leaf E (then the symbols up to E, the depth and the leaves decide), stops
// at a tag other than 0 / 1 (not a decoder), or at the window's end -- which is the stream's end (not a decoder: it ends inside the trie) or
// the cap on the decoder's bytes (not ours: more than kSmallTrieMaxLeaves leaves, or that many nodes without an end)
CNIIC_ST_HD uint32_t st_verdict_open(bool bad_tag, uint32_t window, uint64_t trie_bytes) {
    return bad_tag || window == trie_bytes ? kStNotDecoder : kStNotOurs;
}

}  // namespace cniic
