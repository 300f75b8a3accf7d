// vor_small_check.cpp -- the per-point arithmetic of the small-frame voronoi kernel (cniic_amd/csrc/vor_small.hpp), checked on the host.
// A scalar K-means built from the header's functions alone -- initial label, first point of each chunk, u32 squared distance, the stay test,
// the "strictly nearer, lowest index" move rule, u32 sums that follow the moves, truncating means, reseed index -- runs with the stay test
// on and with it off beside a plain 64-bit restatement of kmeans::cluster over ColorPos points written out below (int64 differences, the
// minimum searched in index order, u64 sums summed afresh every iteration).  Centroids, labels, iterations, moved_last, reseed counts and
// active clusters must be equal; the largest distance and the largest sum met are held against the header's bounds.  Then the stay test
// alone on random points and centroids, the stream's layout and the decoder's wrapping squares.
// Build: c++ -O2 -std=c++17 -I cniic_amd/csrc tests/vor_small_check.cpp.  Prints "ok <part>: ..." per part; exit status 1 on a mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "vor_small.hpp"

using namespace cniic;

struct Result {
    int refused = 0;
    std::vector<uint32_t> cxy, crgb, lab;
    uint64_t iterations = 0, moved_last = 0, reseeds = 0, active = 0, evals = 0;
    bool operator==(const Result &o) const {
        return refused == o.refused && cxy == o.cxy && crgb == o.crgb && lab == o.lab && iterations == o.iterations && moved_last == o.moved_last &&
               reseeds == o.reseeds && active == o.active;
    }
};

static uint64_t g_max_dist = 0, g_max_sum = 0;

// ---- what the kernel does, one point at a time.  rgb: 0xRRGGBB of the w x h pixels, row-major
static Result run_header(const std::vector<uint32_t> &rgb, uint32_t w, uint32_t K, uint64_t seed, uint64_t max_iters, bool stay) {
    Result r;
    const uint32_t n = (uint32_t)rgb.size();
    if (n / K == 0) { r.refused = 1; return r; }
    auto xy = [&](uint32_t i) { return (i % w) | (i / w) << 16; };
    r.lab.resize(n); r.cxy.resize(K); r.crgb.resize(K);
    std::vector<uint32_t> sum(5 * (size_t)K, 0), mem(K, 0), sep(K);
    auto account = [&](uint32_t i, int from, uint32_t to) {
        const uint32_t v[5] = {xy(i) & 0xffffu, xy(i) >> 16, (rgb[i] >> 16) & 255u, (rgb[i] >> 8) & 255u, rgb[i] & 255u};
        for (int d = 0; d < 5; d++) {
            if (from >= 0) sum[5 * (size_t)from + d] -= v[d];
            g_max_sum = std::max<uint64_t>(g_max_sum, (uint64_t)sum[5 * (size_t)to + d] + v[d]);
            sum[5 * (size_t)to + d] += v[d];
        }
        if (from >= 0) mem[from]--;
        mem[to]++;
    };
    for (uint32_t i = 0; i < n; i++) { r.lab[i] = vs_init_label(i, n, K); account(i, -1, r.lab[i]); }
    for (uint32_t k = 0; k < K; k++) { const uint32_t i = vs_init_centroid_point(k, n, K); r.cxy[k] = xy(i); r.crgb[k] = rgb[i]; }
    for (;;) {
        for (uint32_t c = 0; c < K; c++) {
            uint32_t m = 0xffffffffu;
            for (uint32_t k = 0; k < K; k++) if (k != c) m = std::min(m, vs_dist2(r.cxy[c], r.crgb[c], r.cxy[k], r.crgb[k]));
            sep[c] = m;
        }
        uint64_t moved = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t cur = r.lab[i], dcur = vs_dist2(xy(i), rgb[i], r.cxy[cur], r.crgb[cur]);
            g_max_dist = std::max<uint64_t>(g_max_dist, dcur);
            r.evals++;
            if (stay && vs_stays(dcur, sep[cur])) continue;
            uint32_t best = 0xffffffffu, best_k = 0;
            for (uint32_t k = 0; k < K; k++) {
                const uint32_t d = vs_dist2(xy(i), rgb[i], r.cxy[k], r.crgb[k]);
                g_max_dist = std::max<uint64_t>(g_max_dist, d);
                if (d < best) { best = d; best_k = k; }
            }
            r.evals += K;
            const uint32_t nl = vs_new_label(best, best_k, dcur, cur);
            if (nl != cur) { moved++; r.lab[i] = nl; account(i, (int)cur, nl); }
        }
        r.active = 0;
        for (uint32_t k = 0; k < K; k++) {
            if (mem[k] == 0) { const uint32_t i = vs_reseed_index(seed, r.iterations, k, n); r.cxy[k] = xy(i); r.crgb[k] = rgb[i]; r.reseeds++; }
            else {
                const uint32_t *s = &sum[5 * (size_t)k];
                r.cxy[k] = vs_mean_xy(s[0], s[1], mem[k]); r.crgb[k] = vs_mean_rgb(s[2], s[3], s[4], mem[k]); r.active++;
            }
        }
        r.moved_last = moved;
        r.iterations++;
        if (moved == 0 || (max_iters && r.iterations >= max_iters)) break;
    }
    return r;
}

// ---- kmeans::cluster restated in 64-bit integers: init_assignment and init_centroids (kmeans.rs:61-108), the exact Lloyd step with
// "lowest index among minima" and "ties stay" (kmeans.rs:330-416), Point::mean for ColorPos (clusterc.rs:216-247), the reseed of an
// empty cluster (kmeans.rs:110-137, with splitmix64 standing in for thread_rng)
struct P5 { int64_t v[5]; };
static int64_t dist2(const P5 &a, const P5 &b) {
    int64_t s = 0;
    for (int d = 0; d < 5; d++) { const int64_t t = a.v[d] - b.v[d]; s += t * t; }
    return s;
}
static uint64_t splitmix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static Result run_plain(const std::vector<uint32_t> &rgb, uint32_t w, uint32_t K, uint64_t seed, uint64_t max_iters) {
    Result r;
    const uint64_t n = rgb.size();
    if (n / K == 0) { r.refused = 1; return r; }
    std::vector<P5> pt(n), cent(K);
    for (uint64_t i = 0; i < n; i++) pt[i] = P5{{(int64_t)(i % w), (int64_t)(i / w), (rgb[i] >> 16) & 255, (rgb[i] >> 8) & 255, rgb[i] & 255}};
    const uint64_t ppc = n / K;
    r.lab.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t c = (n - 1 - i) / ppc;
        if (c > (uint64_t)K - 1) c = K - 1;
        r.lab[i] = (uint32_t)c;
    }
    for (uint32_t c = 0; c < K; c++) cent[c] = pt[c < K - 1 ? n - ((uint64_t)c + 1) * ppc : 0];
    uint64_t changed = 1;
    while (changed) {
        std::vector<uint64_t> sums(5 * (size_t)K, 0), members(K, 0);
        changed = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t cur = r.lab[i];
            const int64_t dcur = dist2(cent[cur], pt[i]);
            uint32_t bk = cur;
            if (dcur != 0) {
                int64_t m = INT64_MAX;
                uint32_t mk = 0;
                for (uint32_t k = 0; k < K; k++) {
                    const int64_t dk = dist2(cent[k], pt[i]);
                    if (dk < m) { m = dk; mk = k; }
                }
                if (m < dcur) bk = mk;
            }
            if (bk != cur) changed++;
            r.lab[i] = bk;
            for (int d = 0; d < 5; d++) sums[5 * (size_t)bk + d] += (uint64_t)pt[i].v[d];
            members[bk]++;
        }
        r.active = 0;
        for (uint32_t c = 0; c < K; c++) {
            if (members[c] == 0) {
                cent[c] = pt[splitmix(seed + 0x9E3779B97F4A7C15ULL * (r.iterations * 65536ULL + (uint64_t)c + 1ULL)) % n];
                r.reseeds++;
                continue;
            }
            r.active++;
            for (int d = 0; d < 5; d++) {
                const uint64_t v = sums[5 * (size_t)c + d] / members[c];
                cent[c].v[d] = d < 2 ? (int64_t)(uint32_t)v : (int64_t)(uint8_t)v;
            }
        }
        r.moved_last = changed;
        r.iterations++;
        if (max_iters && r.iterations >= max_iters) break;
    }
    r.cxy.resize(K); r.crgb.resize(K);
    for (uint32_t c = 0; c < K; c++) {
        r.cxy[c] = (uint32_t)cent[c].v[0] | (uint32_t)cent[c].v[1] << 16;
        r.crgb[c] = (uint32_t)cent[c].v[2] << 16 | (uint32_t)cent[c].v[3] << 8 | (uint32_t)cent[c].v[4];
    }
    return r;
}

static uint64_t g_rng = 0x1234567887654321ULL;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(g_rng >> 33); }

static int g_fail = 0;
static uint64_t g_cases = 0, g_stay_saved = 0, g_reseeds = 0, g_refused = 0;
static void check(const char *what, const std::vector<uint32_t> &rgb, uint32_t w, uint32_t K, uint64_t seed, uint64_t max_iters) {
    const Result a = run_header(rgb, w, K, seed, max_iters, true), b = run_header(rgb, w, K, seed, max_iters, false), p = run_plain(rgb, w, K, seed, max_iters);
    g_cases++;
    g_reseeds += p.reseeds;
    g_refused += p.refused;
    if (!(a == p) || !(b == p)) {
        printf("FAIL %s: %u x %u, K = %u, max_iters = %llu: stay on %s, stay off %s (iterations %llu / %llu / %llu)\n", what, w, (unsigned)(rgb.size() / w), K,
               (unsigned long long)max_iters, a == p ? "equal" : "DIFFERS", b == p ? "equal" : "DIFFERS", (unsigned long long)a.iterations,
               (unsigned long long)b.iterations, (unsigned long long)p.iterations);
        g_fail = 1;
    }
    if (a.evals > b.evals) { printf("FAIL %s: the stay test evaluated more than brute force\n", what); g_fail = 1; }
    g_stay_saved += b.evals - a.evals;
}

// colours: 0 = uniform noise, 1 = a few colours (many ties), 2 = smooth (photo-like), 3 = flat
static std::vector<uint32_t> frame(uint32_t w, uint32_t h, int kind) {
    std::vector<uint32_t> v((size_t)w * h);
    const uint32_t flat = rnd() & 0xffffffu;
    for (uint32_t i = 0; i < v.size(); i++) {
        const uint32_t x = i % w, y = i / w;
        if (kind == 0) v[i] = rnd() & 0xffffffu;
        else if (kind == 1) v[i] = (rnd() % 3) * 0x404040u;
        else if (kind == 2) v[i] = ((x * 255 / w) & 255) << 16 | ((y * 255 / h) & 255) << 8 | (((x + y) * 3 + (rnd() & 7)) & 255);
        else v[i] = flat;
    }
    return v;
}

int main() {
    // random frames
    for (int t = 0; t < 60; t++) {
        const uint32_t w = 1 + rnd() % 40, h = 1 + rnd() % 40, K = 1 + rnd() % std::min<uint32_t>(w * h, 64);
        check("random", frame(w, h, t % 3), w, K, kVorSmallDefaultSeed, t % 5 == 4 ? 1 + rnd() % 3 : 0);
    }
    printf("ok random: %llu cases\n", (unsigned long long)g_cases);
    // flat frames: every colour distance a tie; the coordinates alone decide
    for (int t = 0; t < 12; t++) {
        const uint32_t w = 1 + rnd() % 30, h = 1 + rnd() % 30, K = 1 + rnd() % std::min<uint32_t>(w * h, 40);
        check("flat", frame(w, h, 3), w, K, 77 + t, 0);
    }
    check("flat", std::vector<uint32_t>(23 * 12, 0x808080u), 23, 128, kVorSmallDefaultSeed, 0);
    printf("ok flat: %llu cases\n", (unsigned long long)g_cases);
    // duplicate centroids: reseeds onto points that other clusters sit on, and a two-colour board whose means coincide
    {
        const uint64_t before = g_reseeds;
        std::vector<uint32_t> board(23 * 12);
        for (uint32_t i = 0; i < board.size(); i++) board[i] = ((i % 23 + i / 23) & 1) ? 0xC81E28u : 0x0ADC5Au;
        check("duplicates", board, 23, 128, kVorSmallDefaultSeed, 0);
        check("duplicates", board, 23, 128, kVorSmallDefaultSeed, 2);
        check("duplicates", board, 23, 128, 99, 0);
        for (int t = 0; t < 10; t++) {
            const uint32_t w = 2 + rnd() % 20, h = 2 + rnd() % 20;
            check("duplicates", frame(w, h, 1), w, std::max<uint32_t>(1, w * h / 2), 1000 + t, 0);
            check("duplicates", frame(w, h, 0), w, std::max<uint32_t>(1, w * h * 2 / 3), 2000 + t, 0);
        }
        if (g_reseeds == before) { printf("FAIL duplicates: no case reseeded\n"); g_fail = 1; }
        printf("ok duplicates: %llu reseeds\n", (unsigned long long)(g_reseeds - before));
    }
    // K = 1, 2, 255, 256 with n = K - 1, K, K + 1, 2K - 1
    {
        const uint64_t before = g_refused;
        const uint32_t Ks[4] = {1, 2, 255, 256};
        for (uint32_t K : Ks)
            for (uint32_t n : {K - 1, K, K + 1, 2 * K - 1}) {
                if (!n) continue;
                const uint32_t w = n % 7 == 0 ? 7 : n % 3 == 0 ? 3 : n;
                check("limits", frame(w, n / w, 0), w, K, kVorSmallDefaultSeed, 0);
                check("limits", frame(n, 1, 2), n, K, kVorSmallDefaultSeed, 0);
            }
        if (g_refused - before != 6) { printf("FAIL limits: %llu refused, not 6\n", (unsigned long long)(g_refused - before)); g_fail = 1; }
        printf("ok limits: %llu refused\n", (unsigned long long)(g_refused - before));
    }
    // the longest frames: 16384 x 1 and 1 x 16384, where distances and sums come nearest their bounds
    {
        std::vector<uint32_t> ends(kVorSmallMaxPx, 0);
        for (uint32_t i = kVorSmallMaxPx / 2; i < kVorSmallMaxPx; i++) ends[i] = 0xffffffu;
        check("long", ends, kVorSmallMaxPx, 1, kVorSmallDefaultSeed, 0);
        check("long", ends, 1, 1, kVorSmallDefaultSeed, 0);
        check("long", ends, kVorSmallMaxPx, 2, kVorSmallDefaultSeed, 0);
        check("long", frame(kVorSmallMaxPx, 1, 0), kVorSmallMaxPx, 16, kVorSmallDefaultSeed, 0);
        check("long", frame(1, kVorSmallMaxPx, 2), 1, 16, kVorSmallDefaultSeed, 0);
        // (a single cluster of the whole frame: its sum is the frame's)
        std::vector<uint32_t> white(kVorSmallMaxPx, 0xffffffu);
        check("long", white, kVorSmallMaxPx, 1, kVorSmallDefaultSeed, 0);
        printf("ok long: largest distance %llu <= %llu, largest sum %llu <= %llu\n", (unsigned long long)g_max_dist, (unsigned long long)kVorSmallDistBound,
               (unsigned long long)g_max_sum, (unsigned long long)kVorSmallSumBound);
        if (g_max_dist > kVorSmallDistBound || g_max_sum > kVorSmallSumBound) { printf("FAIL long: a bound of the header does not hold\n"); g_fail = 1; }
        if (g_max_sum != (uint64_t)(kVorSmallMaxPx - 1) * kVorSmallMaxPx / 2) { printf("FAIL long: the largest sum is not the whole row's\n"); g_fail = 1; }
    }
    // ---- the stay test alone: it never fires where brute force finds a strictly nearer centroid
    {
        uint64_t fired = 0, tried = 0;
        for (int t = 0; t < 4000; t++) {
            const uint32_t K = 1 + rnd() % 12, span = t % 2 ? 16384 : 24;
            std::vector<uint32_t> cxy(K), crgb(K);
            for (uint32_t k = 0; k < K; k++) {
                cxy[k] = (rnd() % span) | (t % 4 < 2 ? 0u : (rnd() % 2)) << 16;
                crgb[k] = t % 3 ? (rnd() & 0x0f0f0fu) : (rnd() & 0xffffffu);
                if (k && rnd() % 5 == 0) { cxy[k] = cxy[k - 1]; crgb[k] = crgb[k - 1]; }   // duplicates
            }
            for (int q = 0; q < 40; q++) {
                const uint32_t cur = rnd() % K;
                uint32_t pxy = (rnd() % span) | (t % 4 < 2 ? 0u : (rnd() % 2)) << 16, prgb = t % 3 ? (rnd() & 0x0f0f0fu) : (rnd() & 0xffffffu);
                if (q % 4 == 0) { pxy = cxy[cur]; prgb = crgb[cur]; }   // at its centroid
                uint32_t sep = 0xffffffffu;
                for (uint32_t k = 0; k < K; k++) if (k != cur) sep = std::min(sep, vs_dist2(cxy[cur], crgb[cur], cxy[k], crgb[k]));
                const uint32_t dcur = vs_dist2(pxy, prgb, cxy[cur], crgb[cur]);
                tried++;
                if (!vs_stays(dcur, sep)) continue;
                fired++;
                for (uint32_t k = 0; k < K; k++)
                    if (vs_dist2(pxy, prgb, cxy[k], crgb[k]) < dcur) { printf("FAIL stay: fired with a strictly nearer centroid\n"); g_fail = 1; }
            }
        }
        if (fired < tried / 20) { printf("FAIL stay: the test fired %llu times of %llu\n", (unsigned long long)fired, (unsigned long long)tried); g_fail = 1; }
        printf("ok stay: fired %llu of %llu, saved %llu evaluations in the runs above\n", (unsigned long long)fired, (unsigned long long)tried, (unsigned long long)g_stay_saved);
    }
    // ---- the stream's layout and the decoder's wrapping squares
    {
        if (vs_stream_len(256) != 4880 || vs_stream_len(1) != 35 || vs_centroid_at(0) != 16 || vs_centroid_at(255) + 19 != vs_stream_len(256)) { printf("FAIL layout: lengths\n"); g_fail = 1; }
        const uint8_t want[19] = {0x04, 0x03, 0x02, 0x01, 0x08, 0x07, 0x06, 0x05, 3, 0, 0, 0, 0, 0, 0, 0, 0xAA, 0xBB, 0xCC};
        for (uint32_t j = 0; j < 19; j++)
            if (vs_centroid_byte(0x01020304u, 0x05060708u, 0xAABBCCu, j) != want[j]) { printf("FAIL layout: byte %u\n", j); g_fail = 1; }
        const uint32_t xs[6] = {0, 16384, 65536 + 3, 1u << 31, 0xffffffffu, 5};
        for (uint32_t cx : xs)
            for (uint32_t cy : xs)
                for (uint32_t x : {0u, 7u, 16383u})
                    for (uint32_t y : {0u, 9u}) {
                        const uint64_t dx = (uint32_t)(cx - x), dy = (uint32_t)(cy - y);
                        const uint32_t plain = (uint32_t)((uint32_t)(dx * dx) + (uint32_t)(dy * dy));   // (clusterc.rs:183: wrapping u32 sub, pow(2), add)
                        if (vs_paint_dist(cx, cy, x, y) != plain) { printf("FAIL layout: paint distance\n"); g_fail = 1; }
                    }
        printf("ok layout: %u bytes at K = 256\n", vs_stream_len(256));
    }
    printf("ok total: %llu K-means cases\n", (unsigned long long)g_cases);
    return g_fail;
}
