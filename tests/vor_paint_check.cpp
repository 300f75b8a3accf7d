// vor_paint_check.cpp -- the arithmetic of the voronoi repaint (cniic_amd/csrc/vor_paint.hpp), checked on the host.
//   equivalence  rectangles 1 x 1, 8 x 4, 8 x 1, 1 x 4 at offsets 0 and 8, every pivot and every centroid from 0 to 23 on both axes: vp_keep is
//                true exactly when some pixel of the rectangle has d(p, c) <= d(p, pivot) (the bound is linear, so exact at the corners)
//   tiles        the kernel's steps on whole images -- pivot by vp_pivot_word, prune by vp_keep, first minimum over the kept list in
//                ascending id, brute force where the list outgrows the cap -- against the wrapping-u32 first minimum over all K, on seeded
//                random sets and on hand-built ones: the corner ties of tests/vor_paint_ref.py, tiles with 255 .. 257 sites, mirrored pairs
//   extremes     centroids at (16383, 16383), (0, 16383), (16383, 0), (0, 0) against rectangles at both ends of a 16384-wide row and of a
//                16384-tall column and 1 x 1 at the origin: pivot key and keep predicate for every pair, against 64-bit arithmetic
//   gate         vp_sides_small, vp_coord_small, vp_tiled_k at their switches; vp_tile_rect of clipped tiles
// Build: c++ -O2 -std=c++17 -I cniic_amd/csrc tests/vor_paint_check.cpp (and once more with -fsanitize=address,undefined).  Prints
// "ok <part>: ..." per part; exit status 1 on a mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "vor_paint.hpp"

using namespace cniic;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Pt { uint32_t x, y; };

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t n) {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (uint32_t)(z % n);
}

// clusterc.rs:183 in u32 arithmetic that wraps; the first minimum wins
static uint32_t wrap_dist(Pt c, uint32_t x, uint32_t y) {
    const uint32_t dx = c.x - x, dy = c.y - y;
    return dx * dx + dy * dy;
}
static uint32_t brute_pixel(const std::vector<Pt> &c, uint32_t x, uint32_t y) {
    uint32_t best = 0, bk = 0;
    for (uint32_t k = 0; k < c.size(); k++) {
        const uint32_t d = wrap_dist(c[k], x, y);
        if (k == 0 || d < best) { best = d; bk = k; }
    }
    return bk;
}

// ---- part 1
static void equivalence() {
    const int fail0 = g_fail;
    const int sizes[4][2] = {{1, 1}, {8, 4}, {8, 1}, {1, 4}};
    uint64_t n = 0, kept = 0, zero = 0;
    for (const auto &s : sizes)
        for (int ox = 0; ox <= 8; ox += 8)
            for (int oy = 0; oy <= 8; oy += 8) {
                const VpRect r{ox, ox + s[0] - 1, oy, oy + s[1] - 1};
                for (int px = 0; px < 24; px++) for (int py = 0; py < 24; py++)
                    for (int kx = 0; kx < 24; kx++) for (int ky = 0; ky < 24; ky++) {
                        bool some = false;
                        int64_t fmax = INT64_MIN;
                        for (int y = r.y0; y <= r.y1; y++)
                            for (int x = r.x0; x <= r.x1; x++) {
                                const int64_t dp = (int64_t)(px - x) * (px - x) + (int64_t)(py - y) * (py - y), dc = (int64_t)(kx - x) * (kx - x) + (int64_t)(ky - y) * (ky - y);
                                some |= dc <= dp;
                                fmax = std::max(fmax, dp - dc);
                            }
                        const bool keep = vp_keep(px, py, kx, ky, r);
                        CHECK(keep == some, "rect %d..%d x %d..%d pivot (%d, %d) centroid (%d, %d): keep %d, some pixel %d", r.x0, r.x1, r.y0, r.y1, px, py, kx, ky, keep, some);
                        CHECK(vp_keep_f(px, py, kx, ky, r) == fmax, "f is the largest d(p, pivot) - d(p, c) of the rectangle");
                        n++; kept += keep; zero += fmax == 0;
                    }
            }
    if (g_fail == fail0) printf("ok equivalence: %llu combinations, %llu kept, %llu of them on f = 0\n", (unsigned long long)n, (unsigned long long)kept, (unsigned long long)zero);
}

// ---- part 2: the kernel's steps for a whole image -> tiles whose list outgrew the cap; every pixel against brute force
struct TileStats { uint32_t tiles = 0, overflow = 0, max_kept = 0; };
static TileStats emulate(const char *what, uint32_t w, uint32_t h, const std::vector<Pt> &c, std::vector<uint32_t> *pivots = nullptr, std::vector<uint32_t> *counts = nullptr) {
    TileStats st;
    const uint32_t K = (uint32_t)c.size(), tiles_x = vp_tiles_x(w), tiles_y = vp_tiles_y(h);
    bool gate = vp_sides_small(w, h) && vp_tiled_k(K);
    for (const Pt &p : c) gate = gate && vp_coord_small(p.x, p.y);
    CHECK(gate, "%s: not a stream of the tiled kernel", what);
    if (!gate) return st;
    for (uint32_t t = 0; t < tiles_x * tiles_y; t++) {
        const VpRect r = vp_tile_rect(t, tiles_x, w, h);
        uint64_t word = ~0ull;
        for (uint32_t k = 0; k < K; k++) word = std::min(word, vp_pivot_word(vp_pivot_key((int32_t)c[k].x, (int32_t)c[k].y, r), k));
        const uint32_t pk = vp_pivot_id(word);
        std::vector<uint32_t> list;
        for (uint32_t k = 0; k < K; k++)
            if (vp_keep((int32_t)c[pk].x, (int32_t)c[pk].y, (int32_t)c[k].x, (int32_t)c[k].y, r)) list.push_back(k);
        st.tiles++;
        st.max_kept = std::max<uint32_t>(st.max_kept, (uint32_t)list.size());
        const bool listed = vp_list_fits((uint32_t)list.size());
        st.overflow += !listed;
        if (pivots) pivots->push_back(pk);
        if (counts) counts->push_back((uint32_t)list.size());
        for (int32_t y = r.y0; y <= r.y1; y++)
            for (int32_t x = r.x0; x <= r.x1; x++) {
                uint32_t bk = 0;
                if (listed) {
                    uint32_t best = 0xffffffffu, bq = 0;
                    for (uint32_t q = 0; q < list.size(); q++) {
                        const int32_t dx = (int32_t)c[list[q]].x - x, dy = (int32_t)c[list[q]].y - y;
                        const uint32_t d = (uint32_t)(dx * dx + dy * dy);
                        if (d < best) { best = d; bq = q; }
                    }
                    CHECK(!list.empty(), "%s: tile %u keeps nothing", what, t);
                    bk = list.empty() ? 0 : list[bq];
                } else {
                    bk = brute_pixel(c, (uint32_t)x, (uint32_t)y);
                }
                const uint32_t want = brute_pixel(c, (uint32_t)x, (uint32_t)y);
                CHECK(bk == want, "%s: pixel (%d, %d) of tile %u takes centroid %u, brute force %u", what, x, y, t, bk, want);
            }
    }
    return st;
}

static std::vector<Pt> distinct_sites(uint32_t n, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh) {   // n distinct pixels of a region, shuffled
    std::vector<uint32_t> at(rw * rh);
    for (uint32_t i = 0; i < at.size(); i++) at[i] = i;
    for (uint32_t i = (uint32_t)at.size() - 1; i > 0; i--) std::swap(at[i], at[rnd(i + 1)]);
    std::vector<Pt> res;
    for (uint32_t i = 0; i < n; i++) res.push_back(Pt{x0 + at[i] % rw, y0 + at[i] / rw});
    return res;
}

static void tiles() {
    const int fail0 = g_fail;
    uint32_t images = 0, overflowed = 0, listed = 0;
    // seeded random sets: inside, up to three sizes outside, on a lattice, about the bound
    for (uint32_t i = 0; i < 120; i++) {
        const uint32_t w = 1 + rnd(200), h = 1 + rnd(120), K = 1 + rnd(i % 4 == 3 ? 1500 : 300), kind = i % 5;
        std::vector<Pt> c(K);
        for (Pt &p : c) {
            const uint32_t how = kind < 4 ? kind : rnd(4);
            if (how == 0) p = Pt{rnd(w), rnd(h)};
            else if (how == 1) p = Pt{rnd(3 * w + 1), rnd(3 * h + 1)};
            else if (how == 2) p = Pt{2 * rnd(w / 2 + 1), 2 * rnd(h / 2 + 1)};
            else p = Pt{kVorPaintCoordBound - 1 - rnd(3), rnd(2) ? rnd(h) : kVorPaintCoordBound - 1 - rnd(3)};
        }
        char what[64];
        snprintf(what, sizeof what, "random %u (%u x %u, K = %u)", i, w, h, K);
        const TileStats st = emulate(what, w, h, c);
        images++; overflowed += st.overflow > 0; listed += st.overflow < st.tiles;
    }
    CHECK(overflowed >= 5 && listed >= 100, "the random sets reach both paths (%u with an overflow, %u with a listed tile)", overflowed, listed);
    // the corner ties (tests/vor_paint_ref.py CORNER_ROWS), their transposes, either id order
    const uint32_t rows[5][8] = {{128, 32, 63, 0, 68, 0, 60, 4}, {128, 32, 64, 0, 59, 0, 67, 4}, {128, 32, 63, 31, 68, 31, 60, 27}, {128, 32, 64, 31, 59, 31, 67, 27},
                                 {100, 32, 99, 0, 104, 0, 96, 4}};
    uint32_t ties = 0;
    for (const auto &r : rows)
        for (int tr = 0; tr < 2; tr++)
            for (int swap = 0; swap < 2; swap++) {
                const uint32_t w = r[tr], h = r[1 - tr], tx = r[2 + tr], ty = r[3 - tr];
                const Pt C{r[4 + tr], r[5 - tr]}, P{r[6 + tr], r[7 - tr]};
                const std::vector<Pt> c = swap ? std::vector<Pt>{P, C} : std::vector<Pt>{C, P};
                char what[64];
                snprintf(what, sizeof what, "corner tie %u x %u at (%u, %u)%s", w, h, tx, ty, swap ? ", P first" : "");
                std::vector<uint32_t> pivots;
                emulate(what, w, h, c, &pivots);
                const uint32_t tile = (ty / kVorPaintTileH) * vp_tiles_x(w) + tx / kVorPaintTileW;
                const VpRect rect = vp_tile_rect(tile, vp_tiles_x(w), w, h);
                CHECK(pivots.size() > tile && pivots[tile] == (swap ? 0u : 1u), "%s: P is the pivot of the tie pixel's tile", what);
                CHECK(vp_keep_f((int32_t)P.x, (int32_t)P.y, (int32_t)C.x, (int32_t)C.y, rect) == 0, "%s: f of C is 0", what);
                CHECK(wrap_dist(C, tx, ty) == 25 && wrap_dist(P, tx, ty) == 25 && brute_pixel(c, tx, ty) == 0, "%s: the tie pixel takes id 0", what);
                ties++;
            }
    // one tile with 255, 256, 257 sites at distinct pixels: each is nearest at its own pixel, so all are kept
    for (uint32_t n = 255; n <= 257; n++)
        for (int far = 0; far < 2; far++) {
            std::vector<Pt> c = distinct_sites(n, 0, 0, 64, 32);
            for (uint32_t j = 0; far && j < 44; j++) c.insert(c.begin() + rnd((uint32_t)c.size() + 1), Pt{5000 + j, 6000});
            std::vector<uint32_t> counts;
            const TileStats st = emulate("one tile", 64, 32, c, nullptr, &counts);
            CHECK(counts.size() == 1 && counts[0] == n && st.overflow == (n > kVorPaintCap ? 1u : 0u), "one tile with %u sites keeps %u, overflow %u", n, counts.empty() ? 0 : counts[0], st.overflow);
        }
    {   // four tiles, one of them overflows
        std::vector<Pt> c = distinct_sites(257, 0, 0, 19, 14);
        for (Pt p : {Pt{80, 16}, Pt{16, 40}, Pt{80, 40}}) c.insert(c.begin() + rnd((uint32_t)c.size() + 1), p);
        const TileStats st = emulate("four tiles", 128, 64, c);
        CHECK(st.tiles == 4 && st.overflow == 1, "four tiles: %u overflow", st.overflow);
    }
    // a pair mirrored about a tile's centre: equal pivot keys, the lower id is the pivot; duplicates of it
    const uint32_t sizes[8][2] = {{1, 1}, {1, 300}, {300, 1}, {63, 31}, {64, 32}, {65, 33}, {5, 200}, {200, 5}};
    for (const auto &s : sizes) {
        const uint32_t w = s[0], h = s[1], tiles_x = vp_tiles_x(w), last = tiles_x * vp_tiles_y(h) - 1;
        const VpRect r = vp_tile_rect(last, tiles_x, w, h);
        CHECK(r.x1 == (int32_t)w - 1 && r.y1 == (int32_t)h - 1 && r.x0 <= r.x1 && r.y0 <= r.y1, "the last tile of %u x %u ends with the image", w, h);
        const uint32_t a = rnd((uint32_t)(r.x1 - r.x0) + 1), b = rnd((uint32_t)(r.y1 - r.y0) + 1);
        std::vector<Pt> c = {Pt{r.x0 + a, r.y0 + b}, Pt{r.x1 - a, r.y1 - b}, Pt{3 * w, h / 2}, Pt{w / 2, 3 * h}, Pt{r.x0 + a, r.y0 + b}};
        CHECK(vp_pivot_key((int32_t)c[0].x, (int32_t)c[0].y, r) == vp_pivot_key((int32_t)c[1].x, (int32_t)c[1].y, r), "mirrored centroids have one key");
        std::vector<uint32_t> pivots;
        emulate("mirrored", w, h, c, &pivots);
        CHECK(pivots.size() == last + 1 && pivots[last] == 0, "the lower id of a mirrored pair is the pivot (%u x %u)", w, h);
        images++;
    }
    if (g_fail == fail0) printf("ok tiles: %u images, %u corner ties, %u random sets with an overflowing tile\n", images + ties + 7, ties, overflowed);
}

// ---- part 3
static void extremes() {
    const int fail0 = g_fail;
    const int32_t B = (int32_t)kVorPaintCoordBound;
    const Pt cents[4] = {{16383, 16383}, {0, 16383}, {16383, 0}, {0, 0}};
    std::vector<VpRect> rects;
    for (uint32_t t : {0u, vp_tiles_x(B) - 1}) rects.push_back(vp_tile_rect(t, vp_tiles_x(B), B, 1));      // both ends of a 16384-wide row
    for (uint32_t t : {0u, vp_tiles_y(B) - 1}) rects.push_back(vp_tile_rect(t, 1, 1, B));                  // ... of a 16384-tall column
    for (uint32_t t : {0u, vp_tiles_x(B) - 1, vp_tiles_x(B) * (vp_tiles_y(B) - 1), vp_tiles_x(B) * vp_tiles_y(B) - 1}) rects.push_back(vp_tile_rect(t, vp_tiles_x(B), B, B));
    rects.push_back(VpRect{0, 0, 0, 0});
    rects.push_back(VpRect{B - 1, B - 1, B - 1, B - 1});
    CHECK(rects[1].x0 == B - 64 && rects[1].x1 == B - 1 && rects[1].y1 == 0 && rects[3].y0 == B - 32 && rects[3].y1 == B - 1 && rects[3].x1 == 0, "the end tiles of the row and the column");
    uint64_t max_key = 0, max_prod = 0, pairs = 0;
    for (const VpRect &r : rects)
        for (const Pt &p : cents) {
            const int64_t dx = 2 * (int64_t)p.x - (r.x0 + r.x1), dy = 2 * (int64_t)p.y - (r.y0 + r.y1), key = dx * dx + dy * dy;
            CHECK((int64_t)vp_pivot_key((int32_t)p.x, (int32_t)p.y, r) == key && key < (1ll << 31), "pivot key of (%u, %u)", p.x, p.y);
            max_key = std::max<uint64_t>(max_key, (uint64_t)key);
            for (const Pt &c : cents) {
                const int64_t ex = (int64_t)p.x - c.x, ey = (int64_t)p.y - c.y;
                const int64_t t[4] = {ex * ((int64_t)c.x + p.x - 2 * r.x0), ex * ((int64_t)c.x + p.x - 2 * r.x1), ey * ((int64_t)c.y + p.y - 2 * r.y0), ey * ((int64_t)c.y + p.y - 2 * r.y1)};
                for (int64_t v : t) { CHECK(std::llabs(v) < (1ll << 30), "a product of the keep predicate"); max_prod = std::max<uint64_t>(max_prod, (uint64_t)std::llabs(v)); }
                const int64_t f = std::max(t[0], t[1]) + std::max(t[2], t[3]);
                CHECK((int64_t)vp_keep_f((int32_t)p.x, (int32_t)p.y, (int32_t)c.x, (int32_t)c.y, r) == f && vp_keep((int32_t)p.x, (int32_t)p.y, (int32_t)c.x, (int32_t)c.y, r) == (f >= 0),
                      "keep predicate of pivot (%u, %u) and centroid (%u, %u)", p.x, p.y, c.x, c.y);
                bool some = false;   // ... and what it claims, over the rectangle's pixels
                for (int32_t y = r.y0; y <= r.y1; y++)
                    for (int32_t x = r.x0; x <= r.x1; x++) {
                        const int64_t dp = ((int64_t)p.x - x) * ((int64_t)p.x - x) + ((int64_t)p.y - y) * ((int64_t)p.y - y), dc = ((int64_t)c.x - x) * ((int64_t)c.x - x) + ((int64_t)c.y - y) * ((int64_t)c.y - y);
                        CHECK(dp < (1ll << 32) && (uint32_t)dp == wrap_dist(p, (uint32_t)x, (uint32_t)y), "true and wrapping distances agree behind the gate");
                        some |= dc <= dp;
                    }
                CHECK(some == (f >= 0), "exact at the extremes");
                pairs++;
            }
        }
    CHECK(max_key == (uint64_t)kVorPaintKeyBound, "the largest key met is the header's bound");
    CHECK(max_prod <= (uint64_t)kVorPaintProductBound, "the largest product met is inside the header's bound");
    if (g_fail == fail0) printf("ok extremes: %llu pairs on %zu rectangles, largest key %llu <= %lld, largest product %llu <= %lld\n", (unsigned long long)pairs, rects.size(), (unsigned long long)max_key,
           (long long)kVorPaintKeyBound, (unsigned long long)max_prod, (long long)kVorPaintProductBound);
}

// ---- part 4
static void gate() {
    const int fail0 = g_fail;
    CHECK(vp_sides_small(16384, 16384) && !vp_sides_small(16385, 1) && !vp_sides_small(1, 16385) && vp_sides_small(1, 1), "sides up to 2^14");
    CHECK(vp_coord_small(16383, 16383) && !vp_coord_small(16384, 0) && !vp_coord_small(0, 16384) && !vp_coord_small(0xffffffffu, 0) && !vp_coord_small(0, 0x80000000u), "coordinates below 2^14");
    CHECK(!vp_tiled_k(0) && vp_tiled_k(1) && vp_tiled_k(4096) && !vp_tiled_k(4097) && !vp_tiled_k(1ull << 32), "1 <= K <= 4096");
    CHECK(vp_list_fits(256) && !vp_list_fits(257) && vp_list_fits(0), "the list holds 256");
    CHECK(vp_tiles_x(1) == 1 && vp_tiles_x(64) == 1 && vp_tiles_x(65) == 2 && vp_tiles_x(16384) == 256 && vp_tiles_y(32) == 1 && vp_tiles_y(33) == 2 && vp_tiles_y(16384) == 512, "tile counts");
    const VpRect r = vp_tile_rect(5, 2, 100, 70);   // tile column 1, tile row 2
    CHECK(r.x0 == 64 && r.x1 == 99 && r.y0 == 64 && r.y1 == 69, "a tile clipped on both sides");
    CHECK(vp_pivot_id(vp_pivot_word(0x7fffffffu, 4095)) == 4095 && vp_pivot_word(1, 0) > vp_pivot_word(0, 4095) && vp_pivot_word(7, 3) < vp_pivot_word(7, 4), "key first, then the lower id");
    if (g_fail == fail0) printf("ok gate: sides <= %u, coordinates < %u, K <= %u, list <= %u\n", kVorPaintCoordBound, kVorPaintCoordBound, kVorPaintMaxK, kVorPaintCap);
}

int main() {
    equivalence();
    tiles();
    extremes();
    gate();
    if (g_fail) { printf("FAIL: %d checks\n", g_fail); return 1; }
    printf("ok total: every check held\n");
    return 0;
}
