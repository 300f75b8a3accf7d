// zd_chain_check.cpp -- the hybrid chain of zip(dict)'s frozen parse (cniic_amd/csrc/zd_chain.hpp, the kernels of k_zipdict.hip) as a scalar
// emulation from the header's own functions, held against a plain serial walk on synthetic length arrays: the marks must be equal.
// Every "kernel" runs its lanes in a shuffled order (a round of the pointer doubling reads the table of the round before).
//
//   zd_chain_check                 the sweep of M, the placed cases, the bounds, the corrupted table
//   zd_chain_check len FILE        FILE: u64 M, then M u32 lengths; prints "B entered" and the marks' FNV, or fails
//
// Build: c++ -std=c++17 -O2 -I cniic_amd/csrc tests/zd_chain_check.cpp   (and again with -fsanitize=address,undefined)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <numeric>
#include <set>
#include <string>
#include <vector>

#include "zd_chain.hpp"

using namespace cniic;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
static std::vector<uint32_t> shuffled(uint32_t n) {
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    for (uint32_t i = n; i > 1; i--) std::swap(p[i - 1], p[rnd() % i]);
    return p;
}
static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

// ---- the statement: the parse starts, one after the other
static std::vector<uint8_t> serial_marks(const std::vector<uint32_t> &len) {
    std::vector<uint8_t> mark(len.size(), 0);
    for (uint64_t p = 0; p < len.size(); p += len[p]) mark[p] = 1;
    return mark;
}

// ---- k_rle_approx.hip's scan of the maps (k_rla_compose, k_rla_down), restated
struct Scan { std::vector<std::vector<uint8_t>> maps; std::vector<uint8_t> ent; uint32_t cnt[kZcMaxLevels]; uint32_t n; };
static void scan_maps(const std::vector<uint8_t> &maps0, uint32_t npieces, Scan *s) {
    s->n = zc_level_counts(npieces, s->cnt);
    s->maps.assign(s->n, {});
    s->maps[0] = maps0;
    for (uint32_t l = 0; l + 1 < s->n; l++) {
        s->maps[l + 1].assign((size_t)s->cnt[l + 1] * 256, 0);
        for (uint32_t g : shuffled(s->cnt[l + 1]))
            for (uint32_t v0 = 0; v0 < 256; v0++) {
                uint32_t v = v0;
                for (uint32_t k = 64 * g; k < std::min(64 * g + 64, s->cnt[l]); k++) v = s->maps[l][(size_t)k * 256 + v];
                s->maps[l + 1][(size_t)g * 256 + v0] = (uint8_t)v;
            }
    }
    std::vector<uint8_t> parent;
    for (uint32_t l = s->n; l-- > 0;) {
        std::vector<uint8_t> ent(s->cnt[l]);
        for (uint32_t g = 0; g < (s->cnt[l] + 63) / 64; g++) {
            uint32_t v = parent.empty() ? 0u : parent[g];
            for (uint32_t k = 64 * g; k < std::min(64 * g + 64, s->cnt[l]); k++) { ent[k] = (uint8_t)v; v = s->maps[l][(size_t)k * 256 + v]; }
        }
        parent.swap(ent);
    }
    s->ent = parent;
}
static ZcLevels levels_of(const Scan &s) {
    ZcLevels lv{};
    lv.n = s.n;
    for (uint32_t l = 0; l < s.n; l++) lv.maps[l] = s.maps[l].data();
    return lv;
}

// ---- k_zd_break_walk: B steps at most.  guard = false: the table's word is the next state as it stands (the corrupted-table case)
static uint32_t walk(uint32_t start, const std::vector<uint32_t> &T, uint32_t B, bool guard, std::vector<uint8_t> *entered, std::vector<uint8_t> *entry,
                     uint32_t *steps) {
    uint32_t st = start, n = 0, step = 0;
    for (; step < B && st != kZcEnd; step++) {
        const uint32_t b = zc_brk(st), e = zc_entry(st);
        if (b >= B) break;
        (*entered)[b] = 1;
        (*entry)[b] = (uint8_t)e;
        n++;
        st = guard ? zc_walk_next(T[(size_t)b * 256 + e], b, B) : T[(size_t)b * 256 + e];
    }
    *steps = step;
    return n;
}

struct Result { bool ran = false; uint32_t B = 0, entered = 0, levels = 0; std::vector<uint8_t> mark; std::vector<uint32_t> brk_piece; std::vector<uint8_t> on, entry; };

// ---- steps 1 - 5 of the route
static Result emulate(const std::vector<uint32_t> &len, uint32_t max_breaks) {
    Result R;
    const uint64_t M = len.size();
    const uint32_t npieces = (uint32_t)((M + 255) / 256);
    R.mark.assign(M, 0);
    // k_zd_break_flags, rle_offsets
    std::vector<uint32_t> flags(npieces, 0);
    for (uint32_t j : shuffled(npieces))
        for (uint32_t t = 0; t < 256; t++)
            if ((uint64_t)j * 256 + t < M && zc_is_break(len[(uint64_t)j * 256 + t])) flags[j] = 1;
    std::vector<uint64_t> before(npieces);
    uint64_t B64 = 0;
    for (uint32_t j = 0; j < npieces; j++) { before[j] = B64; B64 += flags[j]; }
    R.B = (uint32_t)B64;
    if (B64 > std::min(max_breaks, kZcMaxBreaks)) return R;
    const uint32_t B = R.B;
    // k_zd_maps_wide
    std::vector<uint8_t> maps0((size_t)npieces * 256, 0xEE);
    std::vector<uint16_t> exits((size_t)B * 256, 0);
    R.brk_piece.assign(B, 0xFFFFFFFFu);
    for (uint32_t j : shuffled(npieces)) {
        uint16_t tab[256], next[256];
        for (uint32_t t : shuffled(256)) {
            const uint64_t r = (uint64_t)j * 256 + t;
            const uint32_t nx = zc_exit_first(t, r < M, r < M ? len[r] : 1u);
            CHECK(nx <= 0xFFFF, "an exit of %u", nx);
            tab[t] = (uint16_t)nx;
        }
        for (int k = 0; k < kZcRounds; k++) {
            for (uint32_t t : shuffled(256)) next[t] = (uint16_t)zc_exit_round(tab[t], tab);
            memcpy(tab, next, sizeof tab);
        }
        for (uint32_t t = 0; t < 256; t++) {
            CHECK(tab[t] >= 256, "piece %u entry %u has not left after %d rounds", j, t, kZcRounds);
            if (flags[j]) { maps0[(size_t)j * 256 + t] = 0; exits[before[j] * 256 + t] = tab[t]; }
            else { CHECK(tab[t] < 511, "a short piece with exit %u", tab[t]); maps0[(size_t)j * 256 + t] = (uint8_t)(tab[t] - 256); }
        }
        if (flags[j]) R.brk_piece[before[j]] = j;
    }
    Scan s1, s2;
    std::vector<uint8_t> skip(npieces, 0);
    scan_maps(maps0, npieces, &s1);
    R.levels = s1.n;
    const Scan *fin = &s1;
    if (B) {
        const ZcLevels lv = levels_of(s1);
        // k_zd_break_table
        std::vector<uint32_t> T((size_t)B * 256, 0x12345678u);
        for (uint32_t at : shuffled(B * 256))
            T[at] = zc_table_entry(lv, R.brk_piece[at >> 8], exits[at], npieces, M, before.data(), R.brk_piece.data(), B);
        // k_zd_break_walk
        R.on.assign(B, 0);
        R.entry.assign(B, 0);
        uint32_t steps = 0;
        R.entered = walk(zc_next_break(lv, 0, 0, npieces, M, before.data(), R.brk_piece.data(), B), T, B, true, &R.on, &R.entry, &steps);
        CHECK(steps <= B, "the walk took %u steps with %u breaks", steps, B);
        // k_zd_break_patch
        for (uint32_t b : shuffled(B)) {
            if (!R.on[b]) continue;
            const uint32_t j = R.brk_piece[b], x = exits[(size_t)b * 256 + R.entry[b]];
            for (uint32_t t : shuffled(256)) {
                maps0[(size_t)j * 256 + t] = zc_patch_map(true, x, t);
                for (uint32_t p = j + 1, end = zc_flown_end(j, x, npieces); p < end; p++) {
                    CHECK(!skip[p] || t, "piece %u is flown over twice", p);
                    maps0[(size_t)p * 256 + t] = zc_patch_map(false, x, t);
                    if (t == 0) skip[p] = 1;
                }
            }
        }
        scan_maps(maps0, npieces, &s2);
        fin = &s2;
        for (uint32_t b = 0; b < B; b++)    // (only such a break keeps its dummy map, and only the last piece can be one)
            CHECK(R.on[b] || skip[R.brk_piece[b]] || zc_behind(R.brk_piece[b], fin->ent[R.brk_piece[b]], M), "break %u is neither entered nor flown over nor reached behind M", b);
        for (uint32_t b = 0; b < B; b++)
            if (R.on[b]) CHECK(fin->ent[R.brk_piece[b]] == R.entry[b], "break %u: the rescan enters at %u, the walk at %u", b, fin->ent[R.brk_piece[b]], R.entry[b]);
    }
    // k_zd_marks
    for (uint32_t j : shuffled(npieces)) {
        if (skip[j]) continue;
        const uint64_t base = (uint64_t)j * 256;
        for (uint32_t p = fin->ent[j]; p < 256 && base + p < M;) { R.mark[base + p] = 1; p += len[base + p]; }
    }
    R.ran = true;
    return R;
}

static uint64_t fnv(const std::vector<uint8_t> &v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : v) h = (h ^ b) * 0x100000001b3ull;
    return h;
}

// the route against the walk at one bound; returns the result
static Result hold(const char *name, const std::vector<uint32_t> &len, uint32_t bound = kZcMaxBreaks) {
    const Result R = emulate(len, bound);
    CHECK(R.ran == (R.B <= bound), "%s: %u breaks, bound %u, ran %d", name, R.B, bound, (int)R.ran);
    if (R.ran) {
        const std::vector<uint8_t> want = serial_marks(len);
        size_t first = 0;
        while (first < want.size() && want[first] == R.mark[first]) first++;
        CHECK(first == want.size(), "%s: M %zu, the marks differ at %zu", name, len.size(), first);
        // the walk's record against the statement: a break piece is entered when it holds a parse start
        uint32_t entered = 0;
        for (uint32_t b = 0; b < R.B; b++) {
            bool any = false;
            uint32_t firstp = 0;
            for (uint32_t t = 0; t < 256 && !any; t++) { const uint64_t r = (uint64_t)R.brk_piece[b] * 256 + t; if (r < want.size() && want[r]) { any = true; firstp = t; } }
            CHECK(any == (R.on[b] != 0) && (!any || firstp == R.entry[b]), "%s: break %u entered %d at %u, the walk says %d at %u", name, b, (int)any, firstp, (int)R.on[b], R.entry[b]);
            entered += any;
        }
        CHECK(entered == R.entered, "%s: %u breaks entered, the walk counted %u", name, entered, R.entered);
    }
    return R;
}

// ---- synthetic lengths
static std::vector<uint32_t> shorts(uint64_t M, uint32_t top) {
    std::vector<uint32_t> len(M);
    for (auto &l : len) l = 1 + rnd() % top;
    return len;
}
// a long step that the parse takes: the 300 positions in front of p step by 1, so every chain that comes by stands on p
static void plant(std::vector<uint32_t> &len, uint64_t p, uint32_t L, std::vector<uint64_t> *planted = nullptr) {
    for (uint64_t q = p > 300 ? p - 300 : 0; q < p; q++)
        if (len[q] < 256) len[q] = 1;
    len[p] = L;
    if (planted) planted->push_back(p);
}
// a long step the parse steps over: the position before it steps by 2
static void plant_dead(std::vector<uint32_t> &len, uint64_t p, uint32_t L) {
    for (uint64_t q = p > 300 ? p - 300 : 0; q + 1 < p; q++)
        if (len[q] < 256) len[q] = 1;
    len[p - 1] = 2;
    len[p] = L;
}
static bool is_start(const std::vector<uint8_t> &mark, uint64_t p) { return p < mark.size() && mark[p]; }

static void part_sweep() {
    const uint64_t Ms[] = {1, 2, 255, 256, 257, 16383, 16384, 16385, 1048575, 1048576, 1048577, 4097ull * 256 + 5, 5000ull * 256 + 77};
    uint32_t three = 0, cases = 0;
    for (uint64_t M : Ms)
        for (int kind = 0; kind < 3; kind++) {
            std::vector<uint32_t> len = shorts(M, kind == 0 ? 255 : kind == 1 ? 3 : 40);
            const uint32_t every = kind == 2 ? 97 : 3001;       // long steps: one position in `every`, up to the cap, also behind M
            for (uint64_t r = 0; r < M; r++)
                if (rnd() % every == 0) len[r] = 256 + rnd() % (kZcMaxEntry - 255);
            if (kind == 1 && M > 1) len[M - 1] = kZcMaxEntry;
            const Result R = hold("sweep", len);
            three += R.levels >= 3;
            cases++;
        }
    CHECK(three >= 6, "three levels in %u cases", three);
    printf("ok sweep: %u texts, %u of them with three levels, M up to %llu\n", cases, three, (unsigned long long)Ms[12]);
}

static void part_placed() {
    uint32_t cases = 0;
    // landings at 0, 1, 254, 255 from origins at 0, 100 and 255, flying over k whole pieces
    std::set<uint32_t> landed, flown, origins;
    for (uint32_t k : {0u, 1u, 2u, 62u, 63u, 64u, 65u, 127u})
        for (uint32_t o : {0u, 100u, 255u})
            for (uint32_t e : {0u, 1u, 254u, 255u}) {
                const int64_t L = (int64_t)(k + 1) * 256 + (int64_t)e - (int64_t)o;
                if (L < 256 || L > (int64_t)kZcMaxEntry) continue;
                for (uint32_t j : {0u, 5u, 63u, 64u}) {
                    if (j == 0 && o < 1 && k) continue;
                    std::vector<uint32_t> len = shorts((uint64_t)(j + k + 4) * 256 + 17, 9);
                    const uint64_t p = (uint64_t)j * 256 + o;
                    plant(len, p, (uint32_t)L);
                    const Result R = hold("placed", len);
                    const std::vector<uint8_t> want = serial_marks(len);
                    CHECK(is_start(want, p) && is_start(want, p + L), "placed: the step at %llu is not taken", (unsigned long long)p);
                    CHECK(R.B == 1 && R.entered == 1, "placed: %u breaks, %u entered", R.B, R.entered);
                    landed.insert(e); flown.insert(k); origins.insert(o);
                    cases++;
                }
            }
    CHECK(landed == std::set<uint32_t>({0, 1, 254, 255}) && flown == std::set<uint32_t>({0, 1, 2, 62, 63, 64, 65, 127}) && origins.count(0) && origins.count(255), "placed: not every case stands");
    // a break at position 0, in the last piece; exits at M - 1, M and behind it
    for (int64_t over : {-1, 0, 1, 1000, 40000}) {
        for (uint64_t M : {3000ull, 256ull * 70, 256ull * 70 + 1}) {
            std::vector<uint32_t> len = shorts(M, 5);
            plant(len, 0, 700);
            const uint64_t p = M - 600;
            if (over <= 32768 - 600) plant(len, p, (uint32_t)(600 + over));
            len[M - 1] = over == 40000 ? kZcMaxEntry : len[M - 1];
            const Result R = hold("ends", len);
            CHECK(R.B >= 2 && R.on[0] && R.entry[0] == 0, "ends: the break at 0");
            cases++;
        }
    }
    // two adjacent breaks, long into long, a landing on a short position of a break piece, a break flown over and never entered, a break
    // entered and left by a short step
    {
        std::vector<uint32_t> len = shorts(256 * 400, 7);
        plant(len, 256 * 10 + 3, 300);                 // lands at piece 11 offset 47 ...
        len[256 * 11 + 47] = 5000;                     // ... on a long step: long into long; pieces 10 and 11 are adjacent breaks
        plant_dead(len, 256 * 40 + 100, 9000);         // entered and left by short steps
        plant(len, 256 * 60 + 200, 256 * 6);           // lands in piece 66 ...
        plant_dead(len, 256 * 66 + 250, 400);          // ... a break piece, on a short position (200), and leaves it by short steps
        plant(len, 256 * 100 + 9, 256 * 20);           // flies over piece 110 ...
        plant_dead(len, 256 * 110 + 50, 3000);         // ... a break that is never entered
        plant(len, 256 * 110 + 60, 2000);
        const Result R = hold("mixed", len);
        const std::vector<uint8_t> want = serial_marks(len);
        CHECK(is_start(want, 256 * 11 + 47) && is_start(want, 256 * 11 + 47 + 5000) && !is_start(want, 256 * 40 + 100) && is_start(want, 256 * 66 + 200) &&
                  !is_start(want, 256 * 110 + 60), "mixed: not every case stands");
        CHECK(R.B == 7 && R.entered == 6 && !R.on[6], "mixed: %u breaks, %u entered", R.B, R.entered);
        cases++;
    }
    // short runs of N pieces between two breaks, at several alignments
    for (uint32_t N : {1u, 63u, 64u, 65u, 4095u, 4096u, 4097u})
        for (uint32_t j : {0u, 1u, 62u, 63u, 4095u}) {
            if (N < 4000 && j == 4095) continue;
            std::vector<uint32_t> len = shorts((uint64_t)(j + N + 5) * 256, 200);
            plant(len, (uint64_t)j * 256 + 7, 300);                    // lands in piece j + 1
            plant(len, (uint64_t)(j + 1 + N) * 256 + 128, 777);        // the next break: N pieces on
            const Result R = hold("runs", len);
            CHECK(R.B == 2 && R.entered == 2, "runs %u at %u: %u breaks, %u entered", N, j, R.B, R.entered);
            cases++;
        }
    // every piece a break; no break at all; the bound at B - 1, B, B + 1
    {
        std::vector<uint32_t> all(256 * 300 + 9, 300), none = shorts(256 * 300 + 9, 255);
        std::vector<uint32_t> dense = shorts(256 * 300 + 9, 3);
        for (uint64_t r = 0; r < dense.size(); r++) if (rnd() % 50 == 0) dense[r] = 256 + rnd() % 3000;
        const Result Ra = hold("all", all), Rn = hold("none", none), Rd = hold("dense", dense);
        CHECK(Ra.B == 301 && Rn.B == 0 && Rd.B > 290, "all %u, none %u, dense %u", Ra.B, Rn.B, Rd.B);
        for (const auto *t : {&all, &dense, &none}) {
            const uint32_t B = t == &all ? Ra.B : t == &dense ? Rd.B : 0;
            for (uint32_t bound : {B ? B - 1 : 0u, B, B + 1}) {
                const Result R = hold("bound", *t, bound);
                CHECK(R.ran == (B <= bound), "bound %u of %u", bound, B);
                cases++;
            }
        }
    }
    printf("ok placed: %u texts\n", cases);
}

static void part_corrupt() {
    // tables whose every entry points back at its own break, at break 0, or beyond B: the counter ends the unguarded walk after B steps, the
    // guarded one ends at the first such entry; neither writes outside its arrays
    uint32_t tables = 0;
    for (uint32_t B : {1u, 2u, 64u, 1000u})
        for (int kind = 0; kind < 4; kind++) {
            std::vector<uint32_t> T((size_t)B * 256);
            for (size_t at = 0; at < T.size(); at++) {
                const uint32_t b = (uint32_t)(at >> 8);
                T[at] = kind == 0 ? zc_pack(b, rnd() & 255) : kind == 1 ? zc_pack(0, 0) : kind == 2 ? zc_pack(rnd() % B, rnd() & 255) : zc_pack(B + rnd() % 5, 3);
            }
            std::vector<uint8_t> on(B, 0), entry(B, 0);
            uint32_t steps = 0;
            walk(zc_pack(0, 0), T, B, false, &on, &entry, &steps);
            CHECK(steps <= B && (kind == 3 || steps == B), "the unguarded walk: %u steps of %u (kind %d)", steps, B, kind);
            walk(zc_pack(0, 0), T, B, true, &on, &entry, &steps);
            CHECK(steps >= 1 && steps <= B && (kind == 2 || steps == 1), "the guarded walk: %u steps (kind %d)", steps, kind);
            tables++;
        }
    // the range climb ends by its counter whatever its arguments are
    std::vector<uint8_t> ident(256 * 64);
    for (size_t i = 0; i < ident.size(); i++) ident[i] = (uint8_t)i;
    ZcLevels lv{};
    lv.n = 1;
    lv.maps[0] = ident.data();
    CHECK(zc_range(lv, 5, 3, 77) == 77 && zc_range(lv, 0, 64, 9) == 9 && zc_range_steps(6) == 770, "the range climb");
    printf("ok corrupt: %u tables\n", tables);
}

int main(int argc, char **argv) {
    if (argc == 3 && strcmp(argv[1], "len") == 0) {
        FILE *fp = fopen(argv[2], "rb");
        uint64_t M = 0;
        if (!fp || fread(&M, 8, 1, fp) != 1) { printf("FAIL: cannot read %s\n", argv[2]); return 2; }
        std::vector<uint32_t> len(M);
        if (M && fread(len.data(), 4, M, fp) != M) { printf("FAIL: %s is short\n", argv[2]); return 2; }
        fclose(fp);
        const Result R = hold(argv[2], len);
        printf("%u %u %016llx\n", R.B, R.entered, (unsigned long long)fnv(R.mark));
        printf("ok total: %d mismatches\n", g_fail);
        return g_fail ? 1 : 0;
    }
    part_sweep();
    part_placed();
    part_corrupt();
    printf("ok total: piece %u, group %u, %u bytes a break, bound %u, %d mismatches\n", kZcPiece, kZcGroup, kZcBreakBytes, kZcMaxBreaks, g_fail);
    return g_fail ? 1 : 0;
}
