// cc_small_check.cpp -- the per-point arithmetic of the small-frame cluster-colors kernel (cniic_amd/csrc/cc_small.hpp), checked on the host.
// A scalar K-means built from the header's functions alone -- initial label, first point of each chunk, packed score with its tie order,
// "strictly nearer" move rule, u32 weighted sums, truncating mean, reseed index -- runs beside a plain 64-bit restatement of kmeans::cluster
// written out below (per-channel squared differences in int64, the minimum searched in index order, u64 sums).  Centroids, labels,
// iterations, reseed counts and active clusters must be equal, and no sum may reach 2^32.
// Build: c++ -O2 -std=c++17 -I cniic_amd/csrc tests/cc_small_check.cpp.  Prints "ok <part>: ..." per part; exit status 1 on a mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "cc_small.hpp"

using namespace cniic;

struct Result {
    int refused = 0;
    std::vector<uint32_t> cent, lab;
    uint64_t iterations = 0, moved_last = 0, reseeds = 0, active = 0, max_sum = 0;
    bool operator==(const Result &o) const {
        return refused == o.refused && cent == o.cent && lab == o.lab && iterations == o.iterations && moved_last == o.moved_last && reseeds == o.reseeds &&
               active == o.active;
    }
};

// ---- what the kernel does, one point at a time
static Result run_header(const std::vector<uint32_t> &key, const std::vector<uint32_t> &wt, uint32_t K, uint64_t seed, uint64_t max_iters) {
    Result r;
    const uint32_t U = (uint32_t)key.size();
    if (U / K == 0) { r.refused = 1; return r; }
    r.lab.resize(U);
    r.cent.resize(K);
    std::vector<int32_t> cc(K);
    for (uint32_t i = 0; i < U; i++) r.lab[i] = ccs_init_label(i, U, K);
    for (uint32_t k = 0; k < K; k++) { r.cent[k] = key[ccs_init_centroid_point(k, U, K)]; cc[k] = ccs_cconst(r.cent[k], k); }
    for (;;) {
        std::vector<uint32_t> sum(4 * (size_t)K, 0), mem(K, 0);
        uint64_t moved = 0;
        for (uint32_t i = 0; i < U; i++) {
            int32_t best = 0x7fffffff;
            for (uint32_t k = 0; k < K; k++) best = std::min(best, ccs_score(key[i], r.cent[k], cc[k]));
            const uint32_t cur = r.lab[i], nl = ccs_new_label(best, ccs_score(key[i], r.cent[cur], cc[cur]), cur);
            if (nl != cur) moved++;
            r.lab[i] = nl;
            const uint64_t ch[3] = {(key[i] >> 16) & 255, (key[i] >> 8) & 255, key[i] & 255};
            for (int d = 0; d < 3; d++) {
                r.max_sum = std::max<uint64_t>(r.max_sum, (uint64_t)sum[4 * nl + d] + ch[d] * wt[i]);
                sum[4 * nl + d] += (uint32_t)(ch[d] * wt[i]);
            }
            r.max_sum = std::max<uint64_t>(r.max_sum, (uint64_t)sum[4 * nl + 3] + wt[i]);
            sum[4 * nl + 3] += wt[i];
            mem[nl]++;
        }
        r.active = 0;
        for (uint32_t k = 0; k < K; k++) {
            if (mem[k] == 0) { r.cent[k] = key[ccs_reseed_index(seed, r.iterations, k, U)]; r.reseeds++; }
            else { r.cent[k] = ccs_mean(sum[4 * k], sum[4 * k + 1], sum[4 * k + 2], sum[4 * k + 3]); r.active++; }
            cc[k] = ccs_cconst(r.cent[k], k);
        }
        r.moved_last = moved;
        r.iterations++;
        if (moved == 0 || (max_iters && r.iterations >= max_iters)) break;
    }
    return r;
}

// ---- kmeans::cluster restated in 64-bit integers: init_assignment and init_centroids (kmeans.rs:61-108), the exact Lloyd step with
// "lowest index among minima" and "ties stay" (kmeans.rs:330-416), Point::mean for ColorCount (clusterc.rs:83-113), the reseed of an
// empty cluster (kmeans.rs:110-137, with splitmix64 standing in for thread_rng)
static int64_t dist2(uint32_t a, uint32_t b) {
    int64_t s = 0;
    for (int sh = 0; sh <= 16; sh += 8) { const int64_t d = (int64_t)((a >> sh) & 255) - (int64_t)((b >> sh) & 255); s += d * d; }
    return s;
}
static uint64_t splitmix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static Result run_plain(const std::vector<uint32_t> &key, const std::vector<uint32_t> &wt, uint32_t K, uint64_t seed, uint64_t max_iters) {
    Result r;
    const uint64_t n = key.size();
    if (n / K == 0) { r.refused = 1; return r; }
    const uint64_t ppc = n / K;
    r.lab.resize(n);
    r.cent.resize(K);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t c = (n - 1 - i) / ppc;
        if (c > (uint64_t)K - 1) c = K - 1;
        r.lab[i] = (uint32_t)c;
    }
    for (uint32_t c = 0; c < K; c++) r.cent[c] = key[c < K - 1 ? n - ((uint64_t)c + 1) * ppc : 0];
    uint64_t changed = 1;
    while (changed) {
        std::vector<uint64_t> sums(3 * (size_t)K, 0), wsum(K, 0), members(K, 0);
        changed = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t cur = r.lab[i];
            const int64_t dcur = dist2(r.cent[cur], key[i]);
            uint32_t bk = cur;
            if (dcur != 0) {
                int64_t m = INT64_MAX;
                uint32_t mk = 0;
                for (uint32_t k = 0; k < K; k++) {
                    const int64_t dk = dist2(r.cent[k], key[i]);
                    if (dk < m) { m = dk; mk = k; }
                }
                if (m < dcur) bk = mk;
            }
            if (bk != cur) changed++;
            r.lab[i] = bk;
            sums[3 * (size_t)bk] += (uint64_t)((key[i] >> 16) & 255) * wt[i];
            sums[3 * (size_t)bk + 1] += (uint64_t)((key[i] >> 8) & 255) * wt[i];
            sums[3 * (size_t)bk + 2] += (uint64_t)(key[i] & 255) * wt[i];
            wsum[bk] += wt[i];
            members[bk]++;
        }
        r.active = 0;
        for (uint32_t c = 0; c < K; c++) {
            if (members[c] == 0) {
                const uint64_t z = seed + 0x9E3779B97F4A7C15ULL * (r.iterations * 65536ULL + (uint64_t)c + 1ULL);
                r.cent[c] = key[splitmix(z) % n];
                r.reseeds++;
                continue;
            }
            r.active++;
            r.cent[c] = (uint32_t)(uint8_t)(sums[3 * (size_t)c] / wsum[c]) << 16 | (uint32_t)(uint8_t)(sums[3 * (size_t)c + 1] / wsum[c]) << 8 |
                        (uint32_t)(uint8_t)(sums[3 * (size_t)c + 2] / wsum[c]);
            for (int d = 0; d < 3; d++) r.max_sum = std::max(r.max_sum, sums[3 * (size_t)c + d]);
        }
        r.moved_last = changed;
        r.iterations++;
        if (max_iters && r.iterations >= max_iters) break;
    }
    return r;
}

static uint64_t g_rng = 0x1234567ULL;
static uint32_t rnd(uint32_t n) { g_rng += 0x9E3779B97F4A7C15ULL; return (uint32_t)(splitmix(g_rng) % n); }

static int g_fail = 0;
static uint64_t g_runs = 0, g_iters = 0, g_reseeds = 0, g_max_sum = 0;

// keys ascending and distinct unless `raw`; the weights' sum stays within kCcSmallMaxPx, as a routed frame's pixel counts do
static void check(const char *what, std::vector<uint32_t> key, std::vector<uint32_t> wt, uint32_t K, uint64_t seed, uint64_t max_iters, bool raw = false) {
    if (!raw) {
        std::sort(key.begin(), key.end());
        key.erase(std::unique(key.begin(), key.end()), key.end());
        wt.resize(key.size(), 1);
    }
    uint64_t tot = 0;
    for (uint32_t w : wt) tot += w;
    if (tot > kCcSmallMaxPx) { printf("FAIL %s: the case's weights sum to %llu\n", what, (unsigned long long)tot); g_fail = 1; return; }
    const Result a = run_header(key, wt, K, seed, max_iters), b = run_plain(key, wt, K, seed, max_iters);
    g_runs++; g_iters += b.iterations; g_reseeds += b.reseeds;
    g_max_sum = std::max(g_max_sum, std::max(a.max_sum, b.max_sum));
    if (!(a == b) || a.max_sum >= (1ull << 32) || a.max_sum > kCcSmallSumBound) {
        printf("FAIL %s: U %zu K %u: refused %d/%d iterations %llu/%llu reseeds %llu/%llu active %llu/%llu max sum %llu\n", what, key.size(), K, a.refused,
               b.refused, (unsigned long long)a.iterations, (unsigned long long)b.iterations, (unsigned long long)a.reseeds, (unsigned long long)b.reseeds,
               (unsigned long long)a.active, (unsigned long long)b.active, (unsigned long long)a.max_sum);
        g_fail = 1;
    }
}

static std::vector<uint32_t> random_keys(uint32_t n, uint32_t span) {
    std::vector<uint32_t> k(n);
    for (auto &x : k) x = span >= 256 ? rnd(1u << 24) : (rnd(span) << 16 | rnd(span) << 8 | rnd(span));
    return k;
}
static std::vector<uint32_t> random_weights(size_t n, uint32_t total) {   // n weights >= 1 summing to at most `total`
    std::vector<uint32_t> w(n, 1);
    if (total > n) for (uint32_t left = total - (uint32_t)n, i = 0; left && i < 4 * n; i++) { const uint32_t add = rnd(left + 1) / 2; w[rnd((uint32_t)n)] += add; left -= add; }
    return w;
}

int main() {
    const uint32_t Ks[] = {1, 2, 255, 256};
    // ---- random point lists, light and heavy weights, with and without an iteration cap
    for (uint32_t K : {1u, 2u, 3u, 7u, 16u, 64u, 255u, 256u})
        for (int rep = 0; rep < 6; rep++) {
            const uint32_t n = K + rnd(rep < 3 ? 3 * K + 40 : 3000);
            std::vector<uint32_t> key = random_keys(n, rep & 1 ? 256 : 24);
            std::sort(key.begin(), key.end());
            key.erase(std::unique(key.begin(), key.end()), key.end());
            check("random", key, random_weights(key.size(), rep % 3 ? kCcSmallMaxPx : (uint32_t)key.size()), K, rep & 2 ? 77 : kCcSmallDefaultSeed, rep == 5 ? 3 : 0, true);
        }
    // many small crowded lists: points close together and unevenly weighted empty a cluster now and then (the reseed branch)
    for (int rep = 0; rep < 4000; rep++) {
        const uint32_t K = 4 + rnd(40), n = K + rnd(2 * K + 8);
        std::vector<uint32_t> key = random_keys(n, 6 + rnd(20));
        std::sort(key.begin(), key.end());
        key.erase(std::unique(key.begin(), key.end()), key.end());
        if (key.size() < K) continue;
        check("crowded", key, random_weights(key.size(), 40 * (uint32_t)key.size()), K, rep & 1 ? 1 + rnd(1000) : kCcSmallDefaultSeed, 0, true);
    }
    printf("ok random: %llu runs, %llu iterations, %llu reseeds\n", (unsigned long long)g_runs, (unsigned long long)g_iters, (unsigned long long)g_reseeds);
    // ---- points equidistant from two centroids: a grey ramp at K = 2 and 3 (a point halfway stays where it is, and a point that must move
    // takes the lowest index among equal minima), and a lattice whose every point has mirror images
    {
        const uint64_t r0 = g_runs;
        for (uint32_t K : {2u, 3u, 4u, 16u})
            for (uint32_t step : {1u, 2u, 3u, 5u})
                for (uint32_t n : {K, K + 1, 2 * K - 1, 2 * K, 33u, 64u, 255u / step}) {
                    if (n < K) continue;
                    std::vector<uint32_t> key;
                    for (uint32_t i = 0; i < n && i * step < 256; i++) key.push_back(0x010101u * (i * step));
                    check("ramp", key, {}, K, kCcSmallDefaultSeed, 0);
                }
        for (uint32_t K : {2u, 4u, 8u, 27u}) {
            std::vector<uint32_t> key;
            for (uint32_t r = 0; r < 256; r += 51) for (uint32_t g = 0; g < 256; g += 51) for (uint32_t b = 0; b < 256; b += 51) key.push_back(r << 16 | g << 8 | b);
            check("lattice", key, {}, K, kCcSmallDefaultSeed, 0);
        }
        // two centroids at equal distance from a third point that belongs to neither: the lower index wins
        check("equidistant", {0x000000u, 0x0a0000u, 0x140000u, 0x140001u}, {}, 3, kCcSmallDefaultSeed, 0);
        check("equidistant", {0x000000u, 0x000a00u, 0x001400u, 0x001401u, 0x001402u}, {}, 4, kCcSmallDefaultSeed, 0);
        printf("ok ties: %llu runs\n", (unsigned long long)(g_runs - r0));
    }
    // ---- all points equal (one distinct colour; the list itself may repeat a colour only when handed over raw)
    {
        const uint64_t r0 = g_runs;
        check("flat", {0x808080u}, {kCcSmallMaxPx}, 1, kCcSmallDefaultSeed, 0, true);
        check("flat", {0x808080u}, {1}, 2, kCcSmallDefaultSeed, 0, true);      // refused
        for (uint32_t K : Ks) {
            std::vector<uint32_t> key(K + 5, 0x123456u), wt(K + 5, 3);
            check("flat-raw", key, wt, K, kCcSmallDefaultSeed, 0, true);      // equal points: every cluster but one empties and is reseeded
        }
        printf("ok all_equal: %llu runs\n", (unsigned long long)(g_runs - r0));
    }
    // ---- weights up to 16 384: one colour carries nearly every pixel; white at full weight is the largest sum there is
    {
        const uint64_t r0 = g_runs;
        check("heavy", {0xffffffu & 0xffffffu}, {kCcSmallMaxPx}, 1, kCcSmallDefaultSeed, 0, true);
        for (uint32_t K : Ks) {
            std::vector<uint32_t> key = random_keys(K + 9, 256);
            std::sort(key.begin(), key.end());
            key.erase(std::unique(key.begin(), key.end()), key.end());
            std::vector<uint32_t> wt(key.size(), 1);
            wt[key.size() - 1] = kCcSmallMaxPx - (uint32_t)key.size() + 1;
            key[key.size() - 1] = 0xffffffu;
            check("heavy", key, wt, K, kCcSmallDefaultSeed, 0, true);
            wt[key.size() - 1] = 1; wt[0] = kCcSmallMaxPx - (uint32_t)key.size() + 1;
            check("heavy", key, wt, K, kCcSmallDefaultSeed, 0, true);
        }
        if (g_max_sum != kCcSmallSumBound) { printf("FAIL heavy: the largest sum seen is %llu, the bound %llu\n", (unsigned long long)g_max_sum, (unsigned long long)kCcSmallSumBound); g_fail = 1; }
        printf("ok weights: %llu runs, largest sum %llu < 2^32\n", (unsigned long long)(g_runs - r0), (unsigned long long)g_max_sum);
    }
    // ---- K = 1, 2, 255, 256 with U = K, K + 1, 2K - 1, and K - 1 (refused)
    {
        const uint64_t r0 = g_runs;
        for (uint32_t K : Ks)
            for (uint32_t U : {K, K + 1, 2 * K - 1, K - 1}) {
                std::vector<uint32_t> key;
                while (key.size() < U) {
                    key = random_keys(U + 8, 256);
                    std::sort(key.begin(), key.end());
                    key.erase(std::unique(key.begin(), key.end()), key.end());
                }
                key.resize(U);
                const Result a = run_header(key, std::vector<uint32_t>(U, 1), K, 5, 0);
                if (a.refused != (U < K || U == 0)) { printf("FAIL limits: U %u K %u refused %d\n", U, K, a.refused); g_fail = 1; }
                check("limits", key, random_weights(U, 4 * U + 1), K, 5, 0, true);
                check("limits", key, random_weights(U, U), K, 5, 2, true);
            }
        printf("ok limits: %llu runs\n", (unsigned long long)(g_runs - r0));
    }
    if (g_reseeds == 0) { printf("FAIL total: no run reseeded an empty cluster\n"); g_fail = 1; }
    printf("ok total: %llu runs, %llu iterations, %llu reseeds\n", (unsigned long long)g_runs, (unsigned long long)g_iters, (unsigned long long)g_reseeds);
    if (g_fail) { printf("FAIL\n"); return 1; }
    return 0;
}
