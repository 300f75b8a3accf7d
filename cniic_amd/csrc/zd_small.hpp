// zd_small.hpp -- what k_zd_small (k_zd_small.hip: `zip(dict)` of a small frame on one workgroup) computes per frame, in plain functions for
// host and device.  tests/zd_small_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The statement to match is Zip::Dict::encode (zipc.rs:14-19) over DictEncoder::next_pair (dict.rs:66-94): the text is the two dimensions
// as u32 LE and per pixel the u64 LE 3 and r, g, b; the coder reads the longest text that has a symbol, twice, writes the two u16 symbols
// and gives the next free symbol (0x100 ..) to the two texts joined, while the counter is below `limit` (0xFFFF in the codec; a parameter
// here so that the host check crosses the freeze early).  A text that ends behind the first symbol gets 0xFFFF for the second.
//
// Names.  N = 8 + 11 n bytes of text for n pixels.  The dictionary is a trie whose edges (node, byte) lie in an open-addressed table of
// 8-byte slots.  The root's 256 edges are not stored: byte b has the symbol b and leads to node 1 + b.  Every other edge lives in a slot,
// and the node it leads to is kZsFirstSlotNode + the slot's index -- so a node needs no number of its own, no counter hands numbers out,
// and two lanes that race for one edge cannot make two nodes.  A slot: symbol + 1 (16 bits, 0 = none), has-child (1 bit), key = node << 8 |
// byte (28 bits), used (1 bit).  An entry of L bytes adds at most L - 1 edges, so a frame has at most N of them; the table has at least
// 2 (N + 256) slots.
//
// The kernel's three phases per window of kZsWindow text positions, all here:
//   speculate  zs_walk from every position of the window against the table as it stands, at most kZsSpecCap bytes deep
//   commit     zs_commit: next_pair from the first needed position on; a match is the speculated one (finished first where the cap cut it)
//              unless an entry made earlier in the SAME window -- the list, not yet in the table -- is longer and spells the text there
//   flush      zs_insert of every entry on the list, in any order and concurrently
// A frame one of whose matches is longer than `giveup` bytes is handed back (verdict 1): such walks are one lane's dependent loads.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_ZS_HD __host__ __device__ __forceinline__
#else
#define CNIIC_ZS_HD inline
#endif

namespace cniic {

constexpr uint32_t kZdSmallMaxPx = 16384;   // pixels of a frame that takes the route
constexpr uint32_t kZsWindow = 256;         // text positions speculated together
constexpr uint32_t kZsSpecCap = 32;         // bytes a speculating walk reads at most (NOTES AO)
constexpr uint32_t kZsGiveUp = 1024;        // a match longer than this hands the frame back (NOTES AO)
constexpr uint32_t kZsListCap = kZsWindow / 2 + 1;   // entries a window can make: their second matches start 2 bytes apart at least
constexpr uint32_t kZsEof = 0xFFFF, kZsFirstNew = 0x100, kZsLimit = 0xFFFF;   // ZIP_SPECIAL_EOF, Abbrev::start_after_trivial, where Abbrev::next ends
constexpr uint32_t kZsFirstSlotNode = 257;  // node 0 is the root, 1 + b the node behind the root's edge b
constexpr uint32_t kZsNone = 0xFFFFFFFFu;
constexpr uint32_t kZsOk = 0, kZsHandedBack = 1;

// ---- the text
CNIIC_ZS_HD uint32_t zs_text_len(uint32_t n) { return 8u + 11u * n; }
CNIIC_ZS_HD uint8_t zs_text_byte(uint32_t i, uint32_t w, uint32_t h, const uint8_t *pixels) {
    if (i < 8) return (uint8_t)((i < 4 ? w : h) >> (8 * (i & 3)));
    const uint32_t j = i - 8, p = j / 11, r = j - 11 * p;
    return r == 0 ? 3 : r < 8 ? 0 : pixels[3 * p + (r - 8)];
}
// A text kind is a type with N, the text's length, and operator[](i), its byte i: the walks, the commit and the inserts below take any
// (ZsText here; HzText of hz_small.hpp, the text of Hilbert { compress: Zip }).
struct ZsText {
    const uint8_t *px;
    uint32_t w, h, N;
    CNIIC_ZS_HD uint8_t operator[](uint32_t i) const { return zs_text_byte(i, w, h, px); }
};

// ---- sizes: 4 bytes a pair, a pair per 2 bytes of text at least and one for a last byte alone; the slot stride as rs_stride's
CNIIC_ZS_HD uint64_t zs_stream_max(uint64_t N) { return 2 * N + 2; }
CNIIC_ZS_HD uint64_t zs_stride(uint64_t N) { return (zs_stream_max(N) + 15) & ~15ull; }
CNIIC_ZS_HD uint32_t zs_table_bits(uint64_t N) {
    uint32_t b = 10;
    while ((1ull << b) < 2 * (N + 256)) b++;
    return b;
}

// ---- a slot
constexpr uint64_t kZsSymMask = 0xFFFF, kZsChildBit = 1ull << 16, kZsUsedBit = 1ull << 45;
CNIIC_ZS_HD uint32_t zs_key(uint32_t node, uint8_t b) { return (node << 8) | b; }
CNIIC_ZS_HD uint64_t zs_slot_of(uint32_t key) { return kZsUsedBit | ((uint64_t)key << 17); }
CNIIC_ZS_HD uint32_t zs_slot_key(uint64_t v) { return (uint32_t)(v >> 17) & 0x0FFFFFFFu; }
CNIIC_ZS_HD uint32_t zs_hash(uint32_t key, uint32_t bits) { return (key * 0x9E3779B1u) >> (32 - bits); }

// A table's memory as the host program sees it.  The kernel's policy (k_zd_small.hip) has the same three members as device-scope atomics.
struct ZsPlainMem {
    static uint64_t load(const uint64_t *p) { return *p; }
    static uint64_t cas(uint64_t *p, uint64_t expect, uint64_t want) { const uint64_t old = *p; if (old == expect) *p = want; return old; }
    static uint64_t fetch_or(uint64_t *p, uint64_t bits) { const uint64_t old = *p; *p = old | bits; return old; }
};

// the slot of edge `key` and its word, or kZsNone
template <class Mem>
CNIIC_ZS_HD uint32_t zs_find(const uint64_t *tab, uint32_t bits, uint32_t key, uint64_t *word) {
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t h = zs_hash(key, bits);; h = (h + 1) & mask) {
        const uint64_t v = Mem::load(tab + h);
        if (!v) return kZsNone;
        if (zs_slot_key(v) == key) { *word = v; return h; }
    }
}
// the same, made if it is not there: an empty slot is claimed by compare-and-swap, a loser looks at what the winner wrote
template <class Mem>
CNIIC_ZS_HD uint32_t zs_claim(uint64_t *tab, uint32_t bits, uint32_t key, uint64_t *word) {
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t h = zs_hash(key, bits);; h = (h + 1) & mask) {
        uint64_t v = Mem::load(tab + h);
        if (!v) {
            v = Mem::cas(tab + h, 0, zs_slot_of(key));
            if (!v) { *word = zs_slot_of(key); return h; }
        }
        if (zs_slot_key(v) == key) { *word = v; return h; }
    }
}

// ---- a walk (DictEncoder::find_symbol, dict.rs:96-136) from text position q: `depth` bytes read so far, standing on `node`; (sym, len) the
// deepest symbol on the way.  open: the walk has not ended yet (it ends where the node has no child for the next byte, or with the text).
struct ZsWalk { uint32_t sym, len, node, depth, open; };
template <class Text>
CNIIC_ZS_HD ZsWalk zs_walk_begin(const Text &t, uint32_t q) {
    const uint32_t b = t[q];
    return ZsWalk{b, 1u, 1u + b, 1u, 1u};
}
// goes on until the walk ends or has read `stop` bytes
template <class Mem, class Text>
CNIIC_ZS_HD void zs_walk(const uint64_t *tab, uint32_t bits, const Text &t, uint32_t q, uint32_t stop, ZsWalk &s) {
    while (s.open) {
        if (q + s.depth >= t.N) { s.open = 0; break; }
        if (s.depth >= stop) break;
        uint64_t v = 0;
        const uint32_t slot = zs_find<Mem>(tab, bits, zs_key(s.node, t[q + s.depth]), &v);
        if (slot == kZsNone) { s.open = 0; break; }
        s.depth++;
        if (v & kZsSymMask) { s.sym = (uint32_t)(v & kZsSymMask) - 1u; s.len = s.depth; }
        if (!(v & kZsChildBit)) { s.open = 0; break; }
        s.node = kZsFirstSlotNode + slot;
    }
}

// ---- TrieMap::insert (dict.rs:308-323) of text[start, start + len), len >= 2, with symbol sym; any number of them at once
template <class Mem, class Text>
CNIIC_ZS_HD void zs_insert(uint64_t *tab, uint32_t bits, const Text &t, uint32_t start, uint32_t len, uint32_t sym) {
    uint32_t node = 1u + t[start];
    for (uint32_t j = 1; j < len; j++) {
        uint64_t v = 0;
        const uint32_t slot = zs_claim<Mem>(tab, bits, zs_key(node, t[start + j]), &v);
        if (j + 1 < len) {
            if (!(v & kZsChildBit)) Mem::fetch_or(tab + slot, kZsChildBit);
            node = kZsFirstSlotNode + slot;
        } else {
            Mem::fetch_or(tab + slot, (uint64_t)(sym + 1u));   // (no entry is made twice: the field is written once)
        }
    }
}

// ---- what a window speculated, and the entries it made.  W positions from `base` on; position base + i: sym[i], len[i], and
// node[i] = the node the walk stands on | open << 31, depth[i] the bytes it has read.
struct ZsWindow {
    uint16_t *sym, *len, *depth;
    uint32_t *node;
    uint32_t *e_start, *e_len;   // the list: kZsListCap entries
    uint16_t *e_sym;
};
CNIIC_ZS_HD void zs_window_put(const ZsWindow &win, uint32_t i, const ZsWalk &s) {
    win.sym[i] = (uint16_t)s.sym; win.len[i] = (uint16_t)s.len; win.depth[i] = (uint16_t)s.depth; win.node[i] = s.node | (s.open << 31);
}

// ---- the coder's state between windows
struct ZsState {
    uint32_t pos;       // where the open pair starts
    uint32_t mid;       // have1: where its second match starts
    uint32_t s1, have1;
    uint32_t counter;   // the next symbol
    uint32_t pairs;     // written so far
    uint32_t nlist;     // entries on the window's list
    uint32_t finished;  // walks the commit finished behind the speculation's cap
    uint32_t verdict, done;
};
CNIIC_ZS_HD ZsState zs_state_begin() { return ZsState{0, 0, 0, 0, kZsFirstNew, 0, 0, 0, kZsOk, 0}; }
CNIIC_ZS_HD uint32_t zs_need(const ZsState &st) { return st.have1 ? st.mid : st.pos; }

// The longest entry of the list among those that lane `lane` of `lanes` looks at (entries lane, lane + lanes, ...) that is longer than
// `len` and spells the text at q: its length << 16 | its symbol, or 0.
template <class Text>
CNIIC_ZS_HD uint64_t zs_repair_lane(const Text &t, const ZsWindow &win, uint32_t nlist, uint32_t q, uint32_t len, uint32_t lane, uint32_t lanes) {
    uint64_t best = 0;
    for (uint32_t e = lane; e < nlist; e += lanes) {
        const uint32_t el = win.e_len[e], es = win.e_start[e];
        if (el <= len || el > t.N - q) continue;
        uint32_t i = 0;
        while (i < el && t[q + i] == t[es + i]) i++;
        if (i == el) { len = el; best = ((uint64_t)el << 16) | win.e_sym[e]; }
    }
    return best;
}

// The commit of one window: DictEncoder::next_pair from zs_need(st) on, while the needed position lies in [base, base + W) and the list
// has room.  Every lane of the committing wave calls it with the same arguments (the host: one call); Lanes::best(f) is the maximum of
// f(lane) over the lanes, Lanes::first() is true on the one lane that writes the pairs.  out: the frame's stream, 4-byte aligned.
template <class Mem, class Lanes, class Text>
CNIIC_ZS_HD void zs_commit(const uint64_t *tab, uint32_t bits, const Text &t, const ZsWindow &win, uint32_t base, uint32_t W, uint32_t limit, uint32_t giveup,
                           uint32_t *out, ZsState &st) {
    st.nlist = 0;
    for (;;) {
        const uint32_t q = zs_need(st);
        if (q < base || q - base >= W || st.nlist == kZsListCap) return;
        const uint32_t i = q - base;
        ZsWalk s{win.sym[i], win.len[i], win.node[i] & 0x7FFFFFFFu, win.depth[i], win.node[i] >> 31};
        if (s.open) {   // the cap cut it: finished here, every lane the same loads
            zs_walk<Mem>(tab, bits, t, q, 2 * giveup + 2, s);   // (no entry is longer than two matches)
            st.finished++;
        }
        uint32_t sym = s.sym, len = s.len;
        if (st.nlist) {
            const uint32_t nlist = st.nlist;
            const uint64_t r = Lanes::best([&](uint32_t lane, uint32_t lanes) { return zs_repair_lane(t, win, nlist, q, len, lane, lanes); });
            if (r) { len = (uint32_t)(r >> 16); sym = (uint32_t)(r & 0xFFFF); }
        }
        if (len > giveup || s.open) { st.verdict = kZsHandedBack; st.done = 1; return; }
        if (!st.have1) {
            st.s1 = sym; st.mid = q + len; st.have1 = 1;
            if (st.mid < t.N) continue;
            if (Lanes::first()) out[st.pairs] = st.s1 | (kZsEof << 16);   // (symbol1, ZIP_SPECIAL_EOF), dict.rs:81-86
            st.pairs++; st.pos = t.N; st.have1 = 0; st.done = 1;
            return;
        }
        const uint32_t end = q + len;
        if (Lanes::first()) out[st.pairs] = st.s1 | (sym << 16);
        st.pairs++;
        if (st.counter < limit) {   // create_symbol(seq1 ++ seq2), dict.rs:90-92
            // (every lane stores the same three values, and reads back only what it stored itself)
            win.e_start[st.nlist] = st.pos; win.e_len[st.nlist] = end - st.pos; win.e_sym[st.nlist] = (uint16_t)st.counter;
            st.nlist++; st.counter++;
        }
        st.pos = end; st.have1 = 0;
        if (end >= t.N) { st.done = 1; return; }
    }
}

}  // namespace cniic
