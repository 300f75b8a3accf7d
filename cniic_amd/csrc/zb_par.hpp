// zb_par.hpp -- the arithmetic of zip(back)'s whole-GPU decode (k_zipback_par.hip), in plain functions for host and device.
// tests/zb_par_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The contract is the serial loop of k_zb_decode (sp: stream position, o: text position, both from 0):
//   1  o >= need or sp + 2 > n: Done                     2  head = u16 at sp, len = head & 0x7FFF
//   3  look-back (bit 15): sp + 4 > n: Done; back > o: BadLookback at sp; k = min(len, back) from o - back; sp += 4
//   4  explicit: sp + 2 + len > n: BadExplicit at sp; k = len; sp += 2 + len
//   5  o += k; k == 0: Done
// Every stage of it is a function of the stream alone, or of the stream and a prefix sum:
//   next     where the symbol behind the one at p starts, were p a symbol start; n (the END node) where the loop could not go on    (zbp_next)
//   chain    the symbol starts are 0, next(0), next(next(0)), ...: jump[p] = next^(2^r)(p) doubles every round, and a round marks
//            jump[p] of every marked p -- after round r the first 2^r starts are marked                          (zbp_chain_rounds)
//   k        the bytes a start brings, 0 where the loop ends at it for a reason the stream alone shows                        (zbp_k)
//   o        the exclusive 64-bit sum of k over the marked positions in stream order
//   event    what the loop does at (p, o): go on, or end -- the FIRST position with an event, in stream order, is where the serial
//            loop ends; position n always has one (no header)                                                             (zbp_event)
//   pointer  text byte o + t of a symbol: a literal (its byte lies in the stream) or a copy of the strictly earlier byte o - back + t,
//            because k = min(len, back) never lets a copy reach itself                                                  (zbp_pointer)
//   jump     P[j] = kZbpNil where byte j is final.  A round: q = P[j]; if P[q] is nil, out[j] = out[q] and P[j] = nil, else
//            P[j] = P[q].  A byte d copies away from a literal is final after ceil(log2(d + 1)) rounds            (zbp_jump_rounds)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_ZBP_HD __host__ __device__ __forceinline__
#else
#define CNIIC_ZBP_HD inline
#endif

namespace cniic {

constexpr uint32_t kZbpNil = 0xFFFFFFFFu;     // a text byte that is final (tables are indexed below 2^32 - 1)
constexpr uint32_t kZbpMaxRounds = 32;        // a depth is below 2^32
constexpr uint32_t kZbpGo = 0, kZbpDone = 1, kZbpBadExplicit = 2, kZbpBadLookback = 3;   // (kZbRunning .. kZbBadLookback of common.hpp)

struct ZbpHead { uint32_t lookback, len, back; };   // back: 0 unless a look-back header with its `back` inside the stream

// the header at p; the caller has seen p + 2 <= n.  No byte outside [in, in + n) is read.
CNIIC_ZBP_HD ZbpHead zbp_head(const uint8_t *in, uint64_t n, uint64_t p) {
    const uint32_t head = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8);
    ZbpHead h{head >> 15, head & 0x7FFFu, 0};
    if (h.lookback && p + 4 <= n) h.back = (uint32_t)in[p + 2] | ((uint32_t)in[p + 3] << 8);
    return h;
}

// next(p) for p in [0, n]: > p, <= n; n where no whole symbol stands at p
CNIIC_ZBP_HD uint64_t zbp_next(const uint8_t *in, uint64_t n, uint64_t p) {
    if (p + 2 > n) return n;
    const ZbpHead h = zbp_head(in, n, p);
    const uint64_t to = h.lookback ? p + 4 : p + 2 + h.len;
    return to > n ? n : to;
}

// the rounds after which every start of a stream of n bytes is marked: a chain has at most n / 2 + 1 nodes besides 0
CNIIC_ZBP_HD uint32_t zbp_chain_rounds(uint64_t n) {
    uint32_t r = 0;
    while (r < 2 * kZbpMaxRounds && (1ull << r) <= n / 2 + 1) r++;
    return r;
}

// the bytes the symbol at p brings (p <= n)
CNIIC_ZBP_HD uint32_t zbp_k(const uint8_t *in, uint64_t n, uint64_t p) {
    if (p + 2 > n) return 0;
    const ZbpHead h = zbp_head(in, n, p);
    if (h.lookback) return p + 4 > n ? 0 : (h.len < h.back ? h.len : h.back);
    return p + 2 + h.len > n ? 0 : h.len;
}

// what the serial loop does when it stands at (p, o), in the order of its tests
CNIIC_ZBP_HD uint32_t zbp_event(const uint8_t *in, uint64_t n, uint64_t need, uint64_t p, uint64_t o) {
    if (o >= need || p + 2 > n) return kZbpDone;
    const ZbpHead h = zbp_head(in, n, p);
    if (h.lookback) {
        if (p + 4 > n) return kZbpDone;
        if (h.back > o) return kZbpBadLookback;
        return (h.len < h.back ? h.len : h.back) ? kZbpGo : kZbpDone;
    }
    if (p + 2 + h.len > n) return kZbpBadExplicit;
    return h.len ? kZbpGo : kZbpDone;
}

// byte t (< k) of the symbol at (p, o), a symbol without an event: where its value comes from.  literal: stream byte `at`; else text byte `at` < o + t
struct ZbpSource { bool literal; uint64_t at; };
CNIIC_ZBP_HD ZbpSource zbp_source(const ZbpHead &h, uint64_t p, uint64_t o, uint32_t t) {
    return h.lookback ? ZbpSource{false, o - h.back + t} : ZbpSource{true, p + 2 + t};
}
CNIIC_ZBP_HD uint32_t zbp_pointer(const ZbpSource &s) { return s.literal ? kZbpNil : (uint32_t)s.at; }

// one jump round of byte j over the tables of the round before: the new pointer; *copy_from = the byte whose value j takes now, or nil
template <class Tab> CNIIC_ZBP_HD uint32_t zbp_jump(const Tab &P, uint32_t j, uint32_t *copy_from) {
    const uint32_t q = P[j];
    *copy_from = kZbpNil;
    if (q == kZbpNil) return kZbpNil;
    const uint32_t pq = P[q];
    if (pq == kZbpNil) { *copy_from = q; return kZbpNil; }
    return pq;
}
// the rounds a byte d copies away from a literal takes: ceil(log2(d + 1))
CNIIC_ZBP_HD uint32_t zbp_jump_rounds(uint64_t d) {
    uint32_t r = 0;
    while (r < 2 * kZbpMaxRounds && (1ull << r) < d + 1) r++;
    return r;
}

}  // namespace cniic
