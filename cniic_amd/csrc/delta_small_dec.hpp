// delta_small_dec.hpp -- what k_delta_small_dec (k_delta_small_dec.hip: the decode of a small `delta` frame on one workgroup) computes per
// frame that can be stated without the GPU, in plain functions for host and device.  tests/delta_small_dec_check.cpp compiles this file
// (and delta_small.hpp, for the longest code) alone, so it includes nothing else of the library.
//
// The statement to match is Delta::decode (hilbertc.rs:417-431): DecStream over the payload, MSB first (huf.rs:187-206, bit.rs:256-259;
// huff_decode_host in huff_host.cpp), then FromDiff (hilbertc.rs:482-509) from START = 0.
//
// Names: the payload has b bits, the frame wants n symbols.  The decoder is the table of its L leaves in pre-order (huff_parse_leaves),
// which is ascending order of their codes left-aligned in 32 bits: leaf i covers the windows code[i] .. code[i + 1] - 1, the trie being
// full (every branch has two children), so the symbol at a bit position is the LAST leaf whose code is <= the next 32 bits.
#pragma once
#include <stdint.h>
#include "delta_small.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_DSD_HD __host__ __device__ __forceinline__
#else
#define CNIIC_DSD_HD inline
#endif

namespace cniic {

constexpr uint32_t kDeltaSmallDecMaxPx = 16384;   // pixels of a frame that takes the route: the encode route's kDeltaSmallMaxPx
constexpr uint32_t kDsdLanes = 1024;              // subsequences of a payload: one per lane of the workgroup
constexpr uint32_t kDsdMinSubBits = 32;           // a subsequence is never shorter (a short payload keeps few lanes busy)
constexpr uint32_t kDsdT1Bits = 11;               // the first-level table is indexed by a window's top bits
// Settle rounds before a frame is handed back to the single decode.  Lane 0 is right from the first pass and lane i after i more, so
// kDsdLanes rounds settle any payload; codes of nearly one length (uniform noise: 16 383 leaves, all but one of 14 bits) do need that
// many -- one lane moves per round behind the one shorter code -- and 256 CUs that finish such frames get through a batch of them sooner
// than eight worker contexts that are handed them (NOTES AA).  Tests lower the cap to see the hand-back.
constexpr uint32_t kDsdMaxRounds = kDsdLanes;
static_assert(kDeltaSmallDecMaxPx >= kDeltaSmallMinBound && kDeltaSmallDecMaxPx <= kDeltaSmallMaxPx, "the encode route's bounds hold here");
static_assert(kDeltaSmallMaxCodeLen <= 31, "a code fits the 32-bit window, its length five bits");

// ---- what is staged: no n symbols take more than the longest code each; bytes behind the last symbol are never looked at
CNIIC_DSD_HD uint32_t dsd_stage_bytes(uint32_t n, uint64_t payload_bytes) {
    const uint64_t most = ((uint64_t)kDeltaSmallMaxCodeLen * n + 7) / 8;
    return (uint32_t)(payload_bytes < most ? payload_bytes : most);
}
// the staged payload as big-endian words: word i holds bytes 4 i .. 4 i + 3, the first in its top bits
CNIIC_DSD_HD uint32_t dsd_be_word(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
// the 32 bits from bit position bp on (words[bp / 32 + 1] is read: the staging area has two spare words of zeros)
CNIIC_DSD_HD uint32_t dsd_window(const uint32_t *words, uint32_t bp) {
    const uint32_t i = bp >> 5, s = bp & 31;
    return s ? (words[i] << s) | (words[i + 1] >> (32 - s)) : words[i];
}

// ---- subsequences: lane i starts at bit min(i sub, b) and decodes until it has crossed min((i + 1) sub, b)
CNIIC_DSD_HD uint32_t dsd_sub_bits(uint32_t b) {
    const uint32_t s = (b + kDsdLanes - 1) / kDsdLanes;
    return s < kDsdMinSubBits ? kDsdMinSubBits : s;
}
CNIIC_DSD_HD uint32_t dsd_bound(uint32_t lane, uint32_t sub, uint32_t b) {
    const uint64_t at = (uint64_t)lane * sub;
    return at < b ? (uint32_t)at : b;
}

// ---- a leaf's symbol and length in one word: key (27 bits) | length << 27
CNIIC_DSD_HD uint32_t dsd_keylen(uint32_t key, uint32_t len) { return key | (len << 27); }
CNIIC_DSD_HD uint32_t dsd_keylen_key(uint32_t kl) { return kl & 0x7ffffffu; }
CNIIC_DSD_HD uint32_t dsd_keylen_len(uint32_t kl) { return kl >> 27; }

// ---- the lookup.  The last leaf of [lo, hi] whose code is <= win (code[lo] <= win)
CNIIC_DSD_HD uint32_t dsd_find(const uint32_t *code, uint32_t lo, uint32_t hi, uint32_t win) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (code[mid] <= win) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// The first-level table: t1[p] = the leaf of the window p << (32 - kDsdT1Bits), p = 0 .. 2^kDsdT1Bits - 1, and t1[2^kDsdT1Bits] = L - 1;
// t1k[p] = that leaf's keylen word when its code is no longer than kDsdT1Bits bits -- then every window with these top bits is its --
// and 0 otherwise (no leaf of a decoder with two leaves or more has length 0)
CNIIC_DSD_HD void dsd_t1_entry(const uint32_t *code, const uint32_t *keylen, uint32_t L, uint32_t p, uint32_t *t1, uint32_t *t1k) {
    if (p == (1u << kDsdT1Bits)) { t1[p] = L - 1; return; }
    const uint32_t i = dsd_find(code, 0, L - 1, p << (32 - kDsdT1Bits));
    const uint32_t kl = keylen[i];
    t1[p] = i;
    t1k[p] = dsd_keylen_len(kl) <= kDsdT1Bits ? kl : 0u;
}
// window -> the keylen word of its leaf
CNIIC_DSD_HD uint32_t dsd_lookup(const uint32_t *code, const uint32_t *keylen, const uint32_t *t1, const uint32_t *t1k, uint32_t win) {
    const uint32_t p = win >> (32 - kDsdT1Bits);
    const uint32_t kl = t1k[p];
    if (kl) return kl;
    return keylen[dsd_find(code, t1[p], t1[p + 1], win)];
}

// The settle rounds of a frame whose codes are longer than kDsdT1Bits (noise: thousands of leaves of nearly one length, which settle one
// lane per round) look up in a second, larger table that lies where the symbols go afterwards: big[p] = the keylen word of the leaf of
// the window p << (32 - bits) when its code is no longer than `bits` bits, else 0.  One entry of it, from the first-level table:
CNIIC_DSD_HD uint32_t dsd_big_entry(const uint32_t *code, const uint32_t *keylen, const uint32_t *t1, const uint32_t *t1k, uint32_t bits, uint32_t p) {
    const uint32_t win = p << (32 - bits), ps = win >> (32 - kDsdT1Bits);
    const uint32_t kl = t1k[ps] ? t1k[ps] : keylen[dsd_find(code, t1[ps], t1[ps + 1], win)];
    return dsd_keylen_len(kl) <= bits ? kl : 0u;
}
// window -> keylen word through the larger table (big == nullptr: there is none)
CNIIC_DSD_HD uint32_t dsd_lookup_big(const uint32_t *code, const uint32_t *keylen, const uint32_t *t1, const uint32_t *t1k, const uint32_t *big, uint32_t bits,
                                     uint32_t win) {
    if (big) {
        const uint32_t kl = big[win >> (32 - bits)];
        if (kl) return kl;
    }
    return dsd_lookup(code, keylen, t1, t1k, win);
}

// ---- the end of the stream (huff_decode_host, hd_pass_block): a symbol is there when all its bits are; exactly n symbols are wanted and
// running out of bits before the n-th is the failure.  (The window behind the last bit is whatever the staging area holds: a walk that
// reaches a leaf inside the b bits reads only those, and one that does not ends below a node all of whose leaves lie deeper.)
CNIIC_DSD_HD bool dsd_symbol_fits(uint32_t bp, uint32_t len, uint32_t b) { return bp + len <= b; }

// One lane's pass over its subsequence: from bit `start` until `next` (the following lane's bound) is crossed or the bits run out.
// Returns the symbols met; *end = where the following lane has to start (b when the bits ran out: nothing follows).  With out != nullptr the
// symbols' keys go to out[first], out[first + 1], ... as far as they lie below n (then without the larger table, which lies where they go).
CNIIC_DSD_HD uint32_t dsd_pass(const uint32_t *words, uint32_t b, const uint32_t *code, const uint32_t *keylen, const uint32_t *t1, const uint32_t *t1k,
                               const uint32_t *big, uint32_t big_bits, uint32_t start, uint32_t next, uint32_t *end, uint32_t *out, uint32_t first, uint32_t n) {
    uint32_t bp = start, count = 0;
    while (bp < next) {
        const uint32_t kl = dsd_lookup_big(code, keylen, t1, t1k, big, big_bits, dsd_window(words, bp));
        const uint32_t len = dsd_keylen_len(kl);
        if (!dsd_symbol_fits(bp, len, b)) { bp = b; break; }
        if (out && first + count < n) out[first + count] = dsd_keylen_key(kl);
        bp += len;
        count++;
    }
    *end = bp;
    return count;
}

// ---- FromDiff: a key's three differences (delta_sym.hpp: (v + 255) in 9-bit fields, red in the top one), and the range a running sum must keep
CNIIC_DSD_HD int32_t dsd_diff(uint32_t key, uint32_t ch) { return (int32_t)((key >> (18 - 9 * ch)) & 511u) - 255; }
CNIIC_DSD_HD bool dsd_in_range(int32_t v) { return (uint32_t)v <= 255u; }   // hilbertc.rs:505

// ---- status of a frame
constexpr uint32_t kDsdOk = 0, kDsdShort = 1 /* the payload ends before n symbols */, kDsdUnsettled = 2 /* the single decode's */, kDsdRange = 3 /* a colour left 0..255 */;

}  // namespace cniic
