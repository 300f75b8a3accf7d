// zd_small_dec.hpp -- what k_zd_small_dec (k_zd_small_dec.hip: the decode of a small `zip(dict)` frame on one workgroup) computes per pair and
// per byte, in plain functions for host and device.  tests/zd_small_dec_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The statement to match is Zip::Dict::decode (zipc.rs:28-36) over DictDecoder::next (dict.rs:174-260), as decode_zip_dict (zipdict.cpp)
// restates it: the stream is pairs of u16 symbols; 0 .. 255 are the bytes, 0xFFFF the empty text, and pair k (from 0) hands out symbol
// 0x100 + k, whose text is the pair's own.  The reader is lazy: it reads whole pairs only while it has fewer than need = 8 + 11 w h bytes.
//
// So a symbol s >= 0x100 is "the text of pair s - 0x100", which lies in the output before the pair that uses it.  The lengths L[k] are a
// DAG over earlier pairs, the offsets O[k] their prefix sums, and every output byte reaches a literal by hopping from pair to pair; a hop
// needs the pair's two symbols and the length of the first.  No text is ever written out.
//
// The five phases of the kernel, all of whose arithmetic is here:
//   1 validity  kb = the lowest pair with a symbol that has not been handed out (zsd_pair_bad), P if none; only pairs below kb count
//   2 lengths   in rounds: a pair whose two symbols' lengths are known gets min(l1 + l2, C), C = need + 1 (zsd_pair_len).  What a round
//               writes carries kZsdNewBit and reads as unknown until the round is over (zsd_settle), so a round resolves exactly the pairs
//               whose parts were known before it: round r (from 0) resolves the pairs of GENERATION r -- a pair of literals or empty
//               texts has generation 0, any other one more than the deeper of its parts -- whatever the order of the lanes.  A frame whose
//               pairs below kb reach generation `rounds` or more is handed back.
//   3 offsets   the exclusive sum of L into O[0 .. kb], saturating at C (zsd_sat_add; associative on operands <= C, and 2 C < 2^19)
//   4 verdict   zsd_verdict, in the order the single decode meets its errors
//   5 bytes     zsd_find_pair (one binary search of O), then zsd_byte's hops.  A byte that visits more than `hops` pairs hands the frame
//               back: a byte of a pair of generation g visits g + 1 at most.
// Differences O[j + 1] - O[j] stand for L[j] in phase 5.  That is exact wherever it is used: a byte t < need lies in a pair p with
// O[p] <= t, and every part of p is a pair j < p with O[j + 1] <= O[p] < need -- below the saturation.
//
// kZsdMaxPairs stays below 65 279, the pair that hands out 0xFFFE: the freeze rule (no symbol after 0xFFFE, dict.rs:280-290) cannot be
// reached by a frame of the route, and nothing here restates it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_ZSD_HD __host__ __device__ __forceinline__
#else
#define CNIIC_ZSD_HD inline
#endif

namespace cniic {

constexpr uint32_t kZdSmallDecMaxPx = 16384;   // pixels of a frame that takes the route
constexpr uint32_t kZsdMaxPairs = 24576;       // pairs the kernel looks at (u32 offsets for them and the largest image share a CU's LDS); NOTES AR
constexpr uint32_t kZsdHops = 64;              // pairs a byte may visit (the deepest natural frame measured: generation 16)
constexpr uint32_t kZsdRounds = 64;            // rounds of phase 2
constexpr uint32_t kZsdEof = 0xFFFF, kZsdFirstNew = 0x100;
constexpr uint32_t kZsdUnknown = 0xFFFFFFFFu, kZsdNewBit = 0x80000000u;
static_assert(kZsdMaxPairs < kZsdEof - kZsdFirstNew, "the freeze rule stays out of reach");
// a frame's verdict
constexpr uint32_t kZsdOk = 0, kZsdHandedBack = 1, kZsdBadSymbol = 2, kZsdDangling = 3, kZsdShort = 4, kZsdBadRecord = 5;

CNIIC_ZSD_HD uint32_t zsd_need(uint32_t n) { return 8u + 11u * n; }

// ---- a pair's word: the first symbol in the low half.  A stream starts at any byte, so a pair lies at any residue of 4: the kernel reads
// the aligned words around it (both hold a byte of the pair, so neither lies outside the stream's own words) and shifts.
CNIIC_ZSD_HD uint32_t zsd_word_from_aligned(uint32_t lo, uint32_t hi, uint32_t residue) {
    return residue ? (lo >> (8u * residue)) | (hi << (32u - 8u * residue)) : lo;
}
CNIIC_ZSD_HD uint32_t zsd_word_from_bytes(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---- phase 1
CNIIC_ZSD_HD bool zsd_sym_bad(uint32_t s, uint32_t k) { return s != kZsdEof && s >= kZsdFirstNew + k; }
CNIIC_ZSD_HD bool zsd_pair_bad(uint32_t word, uint32_t k) { return zsd_sym_bad(word & 0xFFFFu, k) || zsd_sym_bad(word >> 16, k); }

// ---- phase 2.  L: a word per pair, kZsdUnknown at the start.
CNIIC_ZSD_HD uint32_t zsd_sym_len(uint32_t s, const volatile uint32_t *L) {   // kZsdUnknown: not known before this round
    if (s < kZsdFirstNew) return 1u;
    if (s == kZsdEof) return 0u;
    const uint32_t l = L[s - kZsdFirstNew];
    return (l & kZsdNewBit) ? kZsdUnknown : l;
}
CNIIC_ZSD_HD uint32_t zsd_pair_len(uint32_t word, const volatile uint32_t *L, uint32_t C) {
    const uint32_t l1 = zsd_sym_len(word & 0xFFFFu, L), l2 = zsd_sym_len(word >> 16, L);
    if (l1 == kZsdUnknown || l2 == kZsdUnknown) return kZsdUnknown;
    return l1 + l2 < C ? l1 + l2 : C;
}
// one pair's share of a round: true when it is resolved now
CNIIC_ZSD_HD bool zsd_resolve(uint32_t word, uint32_t k, volatile uint32_t *L, uint32_t C) {
    if (L[k] != kZsdUnknown) return false;
    const uint32_t l = zsd_pair_len(word, L, C);
    if (l == kZsdUnknown) return false;
    L[k] = l | kZsdNewBit;
    return true;
}
// behind the round's barrier: what the round wrote becomes readable.  Returns whether pair k is still unknown.
CNIIC_ZSD_HD bool zsd_settle(uint32_t k, volatile uint32_t *L) {
    const uint32_t l = L[k];
    if (l == kZsdUnknown) return true;
    if (l & kZsdNewBit) L[k] = l & ~kZsdNewBit;
    return false;
}

// ---- phase 3
CNIIC_ZSD_HD uint32_t zsd_sat_add(uint32_t a, uint32_t b, uint32_t C) { return a + b < C ? a + b : C; }   // a, b <= C < 2^31

// ---- phase 4: total = O[kb], P = the pairs looked at, len = the stream's bytes.  *a, *b: the numbers of the message.
CNIIC_ZSD_HD uint32_t zsd_verdict(uint32_t total, uint32_t need, uint32_t kb, uint32_t P, uint64_t len, uint32_t *a, uint32_t *b) {
    *a = 0; *b = 0;
    if (total >= need) return kZsdOk;   // nothing behind the pair that completes byte need - 1 matters
    if (kb < P) { *a = kb; return kZsdBadSymbol; }
    if (P < len / 4) return kZsdHandedBack;   // the stream goes on behind the cap
    if ((len & 3) >= 2) return kZsdDangling;
    *a = total; *b = need;
    return kZsdShort;
}

// ---- phase 5
// the pair p < kb with O[p] <= t < O[p + 1] (t < O[kb]; pairs of empty texts share their offset with the pair behind them)
CNIIC_ZSD_HD uint32_t zsd_find_pair(const uint32_t *O, uint32_t kb, uint32_t t) {
    uint32_t lo = 0, hi = kb;   // O[lo] <= t < O[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (O[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// Byte t of the text (t < O[kb]).  Pairs: k -> the word of pair k.  false: the byte visits more than `hops` pairs.
template <class Pairs>
CNIIC_ZSD_HD bool zsd_byte(const Pairs &pairs, const uint32_t *O, uint32_t kb, uint32_t t, uint32_t hops, uint8_t *out) {
    uint32_t p = zsd_find_pair(O, kb, t), o = t - O[p];
    for (uint32_t visits = 1;; visits++) {
        if (visits > hops) return false;
        const uint32_t word = pairs(p), s1 = word & 0xFFFFu;
        const uint32_t l1 = s1 < kZsdFirstNew ? 1u : s1 == kZsdEof ? 0u : O[s1 - kZsdFirstNew + 1] - O[s1 - kZsdFirstNew];
        uint32_t s = s1;
        if (o >= l1) { o -= l1; s = word >> 16; }
        if (s < kZsdFirstNew) { *out = (uint8_t)s; return true; }
        p = s - kZsdFirstNew;   // (never 0xFFFF: o lies inside the symbol's text.  p falls with every hop: the pair is valid)
    }
}
// a record is the u64 LE 3 and three bytes (ser.rs:216-221): what byte r < 8 of a record must be
CNIIC_ZSD_HD bool zsd_record_byte_ok(uint32_t r, uint8_t v) { return v == (r == 0 ? 3 : 0); }

// ---- the head, on the host: the first 8 bytes of the text from at most kZsdHeadPairs pairs, as zip_dict_dims (zipdict.cpp) finds them on the
// same bytes -- whole pairs while fewer than 8 bytes are there, nothing behind them looked at -- but with the 17 offsets on the stack (that
// function builds the single decode's table of 65 536 entries for every call: a megabyte per frame, 20 ms for 4096 frames).  false: a
// symbol not handed out, or fewer than 8 bytes.
constexpr uint32_t kZsdHeadPairs = 16;
struct ZsdBytePairs {
    const uint8_t *p;
    CNIIC_ZSD_HD uint32_t operator()(uint32_t k) const { return zsd_word_from_bytes(p + 4ull * k); }
};
CNIIC_ZSD_HD bool zsd_head_dims(const uint8_t *head, uint64_t n, uint32_t *w, uint32_t *h) {
    const uint32_t P = n / 4 < kZsdHeadPairs ? (uint32_t)(n / 4) : kZsdHeadPairs, C = 9;
    uint32_t O[kZsdHeadPairs + 1], k = 0, produced = 0;
    const ZsdBytePairs pairs{head};
    for (; k < P && produced < 8; k++) {
        const uint32_t word = pairs(k);
        if (zsd_pair_bad(word, k)) return false;
        uint32_t len = 0;
        for (uint32_t half = 0; half < 2; half++) {
            const uint32_t s = half ? word >> 16 : word & 0xFFFFu;
            len = zsd_sat_add(len, s < kZsdFirstNew ? 1u : s == kZsdEof ? 0u : O[s - kZsdFirstNew + 1] - O[s - kZsdFirstNew], C);
        }
        O[k] = produced;
        O[k + 1] = produced = zsd_sat_add(produced, len, C);
    }
    if (produced < 8) return false;
    uint8_t t[8];
    for (uint32_t i = 0; i < 8; i++)
        if (!zsd_byte(pairs, O, k, i, kZsdHeadPairs + 1, &t[i])) return false;   // (never: a byte visits at most the k <= 16 pairs)
    *w = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
    *h = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    return true;
}

// ---- the kernel's LDS for a frame: the offsets of P pairs and one more, the image at its destination's phase
constexpr CNIIC_ZSD_HD uint32_t zsd_lds_bytes(uint32_t pairs, uint32_t npx) { return 4u * (pairs + 1u) + ((3u * npx + 16u + 15u) & ~15u); }

}  // namespace cniic
