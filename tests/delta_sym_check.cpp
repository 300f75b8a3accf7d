// delta_sym_check.cpp -- a stand-alone check of cniic_amd/csrc/delta_sym.hpp, the symbol arithmetic of the `delta` encoder's 16-bit stream
// (tests/test_delta_limits_cpu.py compiles and runs it, once more under -fsanitize=address,undefined).  Nothing here comes from the
// library but the header under test.  A difference (dr, dg, db) of two pixels has, in plain signed integers,
//     cold   some channel < -16 or > 15
//     index  ((dr + 16) * 32 + (dg + 16)) * 32 + (db + 16)      (not cold)
//     key    ((dr + 255) * 512 + (dg + 255)) * 512 + (db + 255)
// and every way the kernels compute them must give exactly these.
//
//   all_diffs  all 511^3 differences, each from a pair of pixels that realises it (anchored at 0 and at 255 in turn): the field word
//              t - prev + kC of the tile gather gives the verdict, the cube index and the key; delta_key gives the same; for hot ones
//              hot_to_key(index) is the key and key_to_hot(key) the index, for cold ones key_to_hot says no.  Exactly 32^3 are hot.
//   borrows    per channel every one of the 256 x 256 (c, p) pairs with the other two channels at each of -255, 0, +255, with bits 24..31
//              of the pixel words clear and set to garbage: every field of the word is in [273, 783] and equals c - p + 528 (no borrow
//              went from one field to the next), nothing lies above bit 29, and garbage changes nothing.
//   faces      each channel at -17, -16, 15, 16 with the others at -16, 0, 15: cold iff the channel is at -17 or 16.
//   keys       (-255, -255, -255) is key 0 and (+255, +255, +255) the largest key; their pages of the 2^27-bin table are the first one
//              and the last one a key can reach, and that one is inside the table.
// Exit status 0 and a line "ok ..." per part; the first violation is printed after "FAIL" and the status is 1.
#include <stdint.h>
#include <stdio.h>

#include "../cniic_amd/csrc/delta_sym.hpp"

using namespace cniic;

static const uint32_t kPageShiftHere = 12;   // kPageShift of common.hpp (the Python test checks that it still is)
static const uint32_t kTableBits = 27;

struct Want { bool cold; uint32_t index, key; };
static Want want_of(int dr, int dg, int db) {
    Want w;
    w.cold = dr < -16 || dr > 15 || dg < -16 || dg > 15 || db < -16 || db > 15;
    w.index = w.cold ? 0u : (uint32_t)(((dr + 16) * 32 + (dg + 16)) * 32 + (db + 16));
    w.key = (uint32_t)(((dr + 255) * 512 + (dg + 255)) * 512 + (db + 255));
    return w;
}
// a channel pair (c, p) with c - p == d: anchored at the bottom (one of them 0) or at the top (one of them 255)
static void pair_of(int d, bool top, uint32_t &c, uint32_t &p) {
    if (!top) { c = d >= 0 ? (uint32_t)d : 0u; p = d >= 0 ? 0u : (uint32_t)-d; }
    else { c = d >= 0 ? 255u : (uint32_t)(255 + d); p = d >= 0 ? (uint32_t)(255 - d) : 255u; }
}
static uint32_t px_of(uint32_t r, uint32_t g, uint32_t b, uint32_t junk) { return r | (g << 8) | (b << 16) | (junk << 24); }

// one difference through every route of the header; 0 when all agree with the plain integers
static int check_one(const char *part, uint32_t cur, uint32_t prev, int dr, int dg, int db) {
    const Want w = want_of(dr, dg, db);
    const uint32_t d = fields_diff(px_fields(cur), px_fields(prev));
    const int fr = (int)((d >> 20) & 1023u), fg = (int)((d >> 10) & 1023u), fb = (int)(d & 1023u);
    if ((d >> 30) || fr != dr + 528 || fg != dg + 528 || fb != db + 528) {
        printf("FAIL %s: (%d %d %d) from pixels %08x %08x: field word %08x = (%d %d %d) - 528 above bit 29: %u\n", part, dr, dg, db, cur, prev, d, fr, fg, fb, d >> 30);
        return 1;
    }
    if (fr < 273 || fr > 783 || fg < 273 || fg > 783 || fb < 273 || fb > 783) { printf("FAIL %s: (%d %d %d): a field outside [273, 783]\n", part, dr, dg, db); return 1; }
    if (fields_cold(d) != w.cold) { printf("FAIL %s: (%d %d %d): the field word says %s\n", part, dr, dg, db, w.cold ? "hot" : "cold"); return 1; }
    if (!w.cold && fields_hot(d) != w.index) { printf("FAIL %s: (%d %d %d): cube index %u from the fields, %u expected\n", part, dr, dg, db, fields_hot(d), w.index); return 1; }
    if (fields_key(d) != w.key) { printf("FAIL %s: (%d %d %d): key %u from the fields, %u expected\n", part, dr, dg, db, fields_key(d), w.key); return 1; }
    uint32_t hot = 0xffffffffu;
    const uint32_t key = delta_key(cur, prev, hot);
    if (key != w.key || hot != (w.cold ? kCold16 : w.index)) {
        printf("FAIL %s: (%d %d %d): delta_key gives key %u symbol %u, expected %u and %u\n", part, dr, dg, db, key, hot, w.key, w.cold ? kCold16 : w.index);
        return 1;
    }
    uint32_t hx = 0xffffffffu;
    const bool inside = key_to_hot(w.key, hx);
    if (inside == w.cold || (!w.cold && hx != w.index)) { printf("FAIL %s: (%d %d %d): key_to_hot(%u) says %d, index %u\n", part, dr, dg, db, w.key, (int)inside, hx); return 1; }
    if (!w.cold && hot_to_key(w.index) != w.key) { printf("FAIL %s: (%d %d %d): hot_to_key(%u) = %u, key %u\n", part, dr, dg, db, w.index, hot_to_key(w.index), w.key); return 1; }
    return 0;
}

static int check_all_diffs() {
    uint64_t cases = 0, hot = 0;
    uint32_t flip = 0;
    for (int dr = -255; dr <= 255; dr++)
        for (int dg = -255; dg <= 255; dg++)
            for (int db = -255; db <= 255; db++) {
                uint32_t c[3], p[3];
                flip = flip * 5u + 1u;   // which anchor each channel takes: all eight combinations come round
                pair_of(dr, (flip >> 3) & 1u, c[0], p[0]);
                pair_of(dg, (flip >> 4) & 1u, c[1], p[1]);
                pair_of(db, (flip >> 5) & 1u, c[2], p[2]);
                if (check_one("all_diffs", px_of(c[0], c[1], c[2], 0), px_of(p[0], p[1], p[2], 0), dr, dg, db)) return 1;
                hot += !want_of(dr, dg, db).cold;
                cases++;
            }
    if (cases != 511ull * 511 * 511 || hot != kHot) { printf("FAIL all_diffs: %llu cases, %llu hot\n", (unsigned long long)cases, (unsigned long long)hot); return 1; }
    if (kCold16 < kHot || kPad16 != kCold16 + 64) { printf("FAIL all_diffs: the stream's words overlap\n"); return 1; }
    printf("ok all_diffs: %llu differences, %llu inside the cube\n", (unsigned long long)cases, (unsigned long long)hot);
    return 0;
}

static int check_borrows() {
    const int others[3] = {-255, 0, 255};
    const uint32_t junk[3][2] = {{0u, 0u}, {0xffu, 0xffu}, {0xa5u, 0x5au}};
    uint64_t cases = 0;
    for (int ch = 0; ch < 3; ch++)
        for (int oa : others)
            for (int ob : others)
                for (uint32_t c = 0; c < 256; c++)
                    for (uint32_t p = 0; p < 256; p++) {
                        int dd[3];
                        uint32_t cc[3], pp[3];
                        const int o[2] = {oa, ob};
                        for (int k = 0, n = 0; k < 3; k++) {
                            if (k == ch) { cc[k] = c; pp[k] = p; dd[k] = (int)c - (int)p; }
                            else { dd[k] = o[n++]; pair_of(dd[k], false, cc[k], pp[k]); }
                        }
                        uint32_t first = 0;
                        for (int j = 0; j < 3; j++) {
                            const uint32_t cur = px_of(cc[0], cc[1], cc[2], junk[j][0]), prev = px_of(pp[0], pp[1], pp[2], junk[j][1]);
                            if (check_one("borrows", cur, prev, dd[0], dd[1], dd[2])) return 1;
                            const uint32_t d = fields_diff(px_fields(cur), px_fields(prev));
                            if (j == 0) first = d;
                            else if (d != first) { printf("FAIL borrows: bits 24..31 of the pixels changed the field word: %08x, %08x without\n", d, first); return 1; }
                            cases++;
                        }
                    }
    printf("ok borrows: %llu pixel pairs\n", (unsigned long long)cases);
    return 0;
}

static int check_faces() {
    const int at[4] = {-17, -16, 15, 16}, others[3] = {-16, 0, 15};
    uint32_t cases = 0, cold = 0;
    for (int ch = 0; ch < 3; ch++)
        for (int a : at)
            for (int oa : others)
                for (int ob : others)
                    for (int top = 0; top < 2; top++) {
                        int dd[3];
                        uint32_t cc[3], pp[3];
                        const int o[2] = {oa, ob};
                        for (int k = 0, n = 0; k < 3; k++) { dd[k] = k == ch ? a : o[n++]; pair_of(dd[k], top != 0, cc[k], pp[k]); }
                        const uint32_t cur = px_of(cc[0], cc[1], cc[2], 0), prev = px_of(pp[0], pp[1], pp[2], 0);
                        if (check_one("faces", cur, prev, dd[0], dd[1], dd[2])) return 1;
                        const bool want_cold = a == -17 || a == 16;   // written out once more: the face itself
                        uint32_t hot, hx;
                        const uint32_t key = delta_key(cur, prev, hot);
                        if (fields_cold(fields_diff(px_fields(cur), px_fields(prev))) != want_cold || (hot == kCold16) != want_cold || key_to_hot(key, hx) == want_cold) {
                            printf("FAIL faces: (%d %d %d) must be %s\n", dd[0], dd[1], dd[2], want_cold ? "cold" : "hot");
                            return 1;
                        }
                        cold += want_cold;
                        cases++;
                    }
    if (cases != 216 || cold != 108) { printf("FAIL faces: %u cases, %u cold\n", cases, cold); return 1; }
    printf("ok faces: %u differences on and next to the cube's faces, %u cold\n", cases, cold);
    return 0;
}

static int check_keys() {
    const uint32_t lo_px = px_of(0, 0, 0, 0), hi_px = px_of(255, 255, 255, 0);
    uint32_t hot;
    const uint32_t kmin = delta_key(lo_px, hi_px, hot), kmax = delta_key(hi_px, lo_px, hot);
    const uint32_t want_max = (510u << 18) | (510u << 9) | 510u;
    if (kmin != 0 || fields_key(fields_diff(px_fields(lo_px), px_fields(hi_px))) != 0) { printf("FAIL keys: (-255, -255, -255) is key %u\n", kmin); return 1; }
    if (kmax != want_max || fields_key(fields_diff(px_fields(hi_px), px_fields(lo_px))) != want_max) { printf("FAIL keys: (255, 255, 255) is key %u, %u expected\n", kmax, want_max); return 1; }
    const uint32_t npages = (1u << kTableBits) >> kPageShiftHere;
    // no key is larger: every field of a key is at most 510
    if (kmax >= (1u << kTableBits) || (kmin >> kPageShiftHere) != 0 || (kmax >> kPageShiftHere) != 32703u || (kmax >> kPageShiftHere) >= npages) {
        printf("FAIL keys: pages %u and %u of %u\n", kmin >> kPageShiftHere, kmax >> kPageShiftHere, npages);
        return 1;
    }
    if (hot_to_key(0) != want_of(-16, -16, -16).key || hot_to_key(kHot - 1) != want_of(15, 15, 15).key) { printf("FAIL keys: the cube's corners\n"); return 1; }
    printf("ok keys: 0 .. %u, pages 0 .. %u of %u\n", kmax, kmax >> kPageShiftHere, npages);
    return 0;
}

int main() {
    if (check_all_diffs()) return 1;
    if (check_borrows()) return 1;
    if (check_faces()) return 1;
    if (check_keys()) return 1;
    return 0;
}
