// zd_chain.hpp -- the arithmetic of the hybrid chain of zip(dict)'s frozen parse (k_zipdict.hip), in plain functions for host and device.
// tests/zd_chain_check.cpp compiles this file alone, so it includes nothing of the library.
//
// The parse starts of M positions are 0, L(0), L(0) + L(L(0)), ... with 1 <= L <= kZcMaxEntry.  Piece j covers positions [256 j, 256 j + 256);
// positions behind M count as steps of 1.  A piece's EXIT from entry offset e is where the chain that starts at 256 j + e first stands at or
// behind 256 j + 256, relative to 256 j: 256 <= exit <= 255 + kZcMaxEntry.  While every L is at most 255 an exit is below 511, the piece is
// a map u8 -> u8 (exit - 256) and the maps compose in groups of 64 (k_rle_approx.hip's scan).  A BREAK piece holds a position with L > 255:
// its exits are kept wide (u16), it gets a dummy map, and the chain is carried across it by a table walk:
//
//   landing   an exit x of piece j lands in piece j + x / 256 at entry offset x % 256                                      (zc_landing)
//   range     the entry offset after the non-break pieces [a, b), through the kept levels of the scan: a level-l map is used only where
//             its 64^l pieces lie inside [a, b)                                                                            (zc_range)
//   table     T[b][e] for break b entered at e: the next break piece the chain stands in and its entry there, or the end  (zc_table_entry)
//   walk      one lane follows T from the first break; the break index rises with every step, and the step counter -- not the table --
//             ends the loop                                                                                                (zc_walk_next)
//   patch     an entered break's map becomes the constant of its landing's entry, the pieces the jump flies over become the identity and
//             are skipped by the marks; then the maps are scanned again                                                    (zc_patch_map)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_ZC_HD __host__ __device__ __forceinline__
#else
#define CNIIC_ZC_HD inline
#endif

namespace cniic {

constexpr uint32_t kZcPiece = 256;          // positions per map (kZdPiece, kRlaPiece)
constexpr uint32_t kZcGroup = 64;           // maps composed into one of the next level (kRlaGroup)
constexpr uint32_t kZcMaxEntry = 32768;     // the longest step (kZdMaxEntry)
constexpr uint32_t kZcMaxLevels = 6;        // 64^6 > 2^31 pieces
constexpr uint32_t kZcEnd = 0xFFFFFFFFu;    // a table entry, a walk state: the chain leaves the text (or meets no further break)
constexpr uint32_t kZcBreakBytes = 512 + 1024 + 4 + 2;   // side tables per break piece: u16 exits, u32 table, its piece, the entered entry + flag
constexpr uint64_t kZcScratchMax = 256ull << 20;         // ... kept below this
constexpr uint32_t kZcMaxBreaks = (uint32_t)(kZcScratchMax / kZcBreakBytes);   // 174 082 (< 2^24: the packing of T)

// ---- a position's step and the break test
CNIIC_ZC_HD uint32_t zc_step(bool inside, uint32_t len) { return inside ? len : 1u; }    // inside: the position lies below M
CNIIC_ZC_HD bool zc_is_break(uint32_t len) { return len >= kZcPiece; }

// ---- a piece's exits by pointer doubling: nx[t] = t + step(t); 8 rounds of nx[t] = nx[nx[t]] while nx[t] < 256 (every step moves on by
// >= 1, so 256 steps leave the piece).  t + step <= 255 + 32768 fits 16 bits.
CNIIC_ZC_HD uint32_t zc_exit_first(uint32_t t, bool inside, uint32_t len) { return t + zc_step(inside, len); }
template <class Tab> CNIIC_ZC_HD uint32_t zc_exit_round(uint32_t nx, const Tab &tab) { return nx < kZcPiece ? (uint32_t)tab[nx] : nx; }
constexpr int kZcRounds = 8;

// ---- where an exit lands
struct ZcLanding { uint32_t piece, entry; };
CNIIC_ZC_HD ZcLanding zc_landing(uint32_t j, uint32_t x) { return ZcLanding{j + (x >> 8), x & 255u}; }

// ---- the levels of the scan: level 0 = the pieces' maps, level l + 1 [g] = level l [64 g + 63] o ... o level l [64 g]
struct ZcLevels { const uint8_t *maps[kZcMaxLevels]; uint32_t n; };
inline uint32_t zc_level_counts(uint32_t npieces, uint32_t *cnt) {   // rla_chain_entries' counts; returns the number of levels
    uint32_t n = 0;
    cnt[n++] = npieces;
    while (cnt[n - 1] > kZcGroup) { cnt[n] = (cnt[n - 1] + kZcGroup - 1) / kZcGroup; n++; }
    return n;
}
// v through the maps of pieces [a, b) (a <= b <= the pieces): climb while the next level's node starts here and ends inside, take a node
// while it ends inside, descend otherwise.  At most 63 nodes per level on the way up and 63 on the way down, and a move between two
// levels for each: the counter ends the loop, whatever a and b are.
CNIIC_ZC_HD uint32_t zc_range_steps(uint32_t nlevels) { return nlevels * (2 * (kZcGroup - 1) + 2) + 2; }
CNIIC_ZC_HD uint32_t zc_range(const ZcLevels &lv, uint32_t a, uint32_t b, uint32_t v) {
    uint64_t cur = a;
    uint32_t l = 0;
    for (uint32_t step = zc_range_steps(lv.n); step && cur < b; step--) {
        const uint64_t span = 1ull << (6 * l), up = span << 6;
        if (l + 1 < lv.n && (cur & (up - 1)) == 0 && cur + up <= b) { l++; continue; }
        if (cur + span <= b) { v = lv.maps[l][((cur >> (6 * l)) << 8) + v]; cur += span; continue; }
        l--;     // (span > 1 here: at level 0 a piece below b always fits)
    }
    return v;
}

// ---- the break table.  nb(q) = the first break piece at or behind q: before[q] = the breaks before piece q, brk_piece[i] = break i's piece
CNIIC_ZC_HD uint32_t zc_pack(uint32_t brk, uint32_t entry) { return (brk << 8) | entry; }
CNIIC_ZC_HD uint32_t zc_brk(uint32_t packed) { return packed >> 8; }
CNIIC_ZC_HD uint32_t zc_entry(uint32_t packed) { return packed & 255u; }
// the state in which the chain that stands at (piece, entry) meets its next break piece; a chain that stands at or behind M has ended
CNIIC_ZC_HD bool zc_behind(uint32_t piece, uint32_t entry, uint64_t M) { return (uint64_t)piece * kZcPiece + entry >= M; }
template <class Before> CNIIC_ZC_HD uint32_t zc_next_break(const ZcLevels &lv, uint32_t piece, uint32_t entry, uint32_t npieces, uint64_t M, const Before *before,
                                                           const uint32_t *brk_piece, uint32_t B) {
    if (piece >= npieces || zc_behind(piece, entry, M)) return kZcEnd;
    const uint64_t i = before[piece];
    if (i >= B) return kZcEnd;
    const uint32_t to = brk_piece[i], e = zc_range(lv, piece, to, entry);
    return zc_behind(to, e, M) ? kZcEnd : zc_pack((uint32_t)i, e);
}
template <class Before> CNIIC_ZC_HD uint32_t zc_table_entry(const ZcLevels &lv, uint32_t j, uint32_t x, uint32_t npieces, uint64_t M, const Before *before,
                                                            const uint32_t *brk_piece, uint32_t B) {
    const ZcLanding to = zc_landing(j, x);
    return zc_next_break(lv, to.piece, to.entry, npieces, M, before, brk_piece, B);
}
// the walk: the state behind break `brk`, from its table entry; anything but a later break below B ends the walk
CNIIC_ZC_HD uint32_t zc_walk_next(uint32_t t, uint32_t brk, uint32_t B) { return t != kZcEnd && zc_brk(t) > brk && zc_brk(t) < B ? t : kZcEnd; }

// ---- the patch.  Break piece j entered with exit x: its map is the constant of the landing's entry; the pieces strictly between j and
// zc_flown_end are flown over: identity, and no parse start
CNIIC_ZC_HD uint32_t zc_flown_end(uint32_t j, uint32_t x, uint32_t npieces) { const uint32_t to = zc_landing(j, x).piece; return to < npieces ? to : npieces; }
CNIIC_ZC_HD uint8_t zc_patch_map(bool origin, uint32_t x, uint32_t t) { return (uint8_t)(origin ? (x & 255u) : t); }

}  // namespace cniic
