// ps_bounds_check.cpp -- a stand-alone check of cniic_amd/csrc/ps_bounds.hpp: the chunk boundaries of the persistent colour K-means
// named by every cell from its two cost prefixes (what the cell-scan role of k_cc_front_b does) against the bisection k_ps_ranges runs
// (ps_ranges_body, kmeans_rgbw.hpp, restated here loop for loop).  For every input: the two cb[] are equal word for word, and the
// direct rule writes every boundary 0 .. NC exactly once.  Built plain with -Wall -Werror and under -fsanitize=address,undefined
// (tests/test_ps_bounds_cpu.py); prints "ok <part>" per part and returns non-zero on the first difference.
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../cniic_amd/csrc/ps_bounds.hpp"

using namespace cniic;

static const uint32_t kChunks = 24;   // kPsChunks

// ps_ranges_body: cb[g] = first m in [0, M) whose prefix is >= target(g), M if none; cb[NC] = M
static std::vector<uint32_t> bisect(const std::vector<uint32_t> &cost, uint32_t NC) {
    const uint32_t M = (uint32_t)cost.size() - 1;
    const uint64_t total = cost[M];
    std::vector<uint32_t> cb(NC + 1);
    for (uint32_t g = 0; g <= NC; g++) {
        const uint64_t c_lo = total * (g < NC ? g : NC) / NC;
        uint32_t a = 0, b = M;
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if (cost[mid] < c_lo) a = mid + 1; else b = mid;
        }
        cb[g] = g == NC ? M : a;
    }
    return cb;
}

// every cell m writes the boundaries between its prefix and the next; cell 0 also those at or below its own
static bool direct(const std::vector<uint32_t> &cost, uint32_t NC, std::vector<uint32_t> &cb, std::vector<uint32_t> &writes) {
    const uint32_t M = (uint32_t)cost.size() - 1;
    const uint64_t total = cost[M];
    cb.assign(NC + 1, 0xffffffffu);
    writes.assign(NC + 1, 0u);
    auto put = [&](PsBoundRun r, uint32_t v) {
        for (uint32_t i = 0; i < r.count; i++) {
            if (r.first + i > NC) return false;
            cb[r.first + i] = v;
            writes[r.first + i]++;
        }
        return true;
    };
    for (uint32_t m = 0; m < M; m++) {
        if (m == 0 && !put(ps_bounds_upto(cost[0], total, NC), 0u)) return false;
        if (!put(ps_bounds_between(cost[m], cost[m + 1], total, NC), m + 1)) return false;
    }
    return true;
}

static int check(const char *what, const std::vector<uint32_t> &cost, uint32_t G) {
    const uint32_t NC = G * kChunks;
    const std::vector<uint32_t> want = bisect(cost, NC);
    std::vector<uint32_t> got, writes;
    if (!direct(cost, NC, got, writes)) { printf("FAIL %s G=%u: a boundary beyond NC\n", what, G); return 1; }
    for (uint32_t g = 0; g <= NC; g++) {
        if (writes[g] != 1) { printf("FAIL %s G=%u: boundary %u written %u times\n", what, G, g, writes[g]); return 1; }
        if (got[g] != want[g]) { printf("FAIL %s G=%u: cb[%u] = %u, the bisection has %u\n", what, G, g, got[g], want[g]); return 1; }
        if (ps_bound_target(cost.back(), g, NC) != (uint64_t)cost.back() * g / NC) { printf("FAIL %s: target(%u)\n", what, g); return 1; }
    }
    return 0;
}

// the prefix k_cell_scan writes: cell m costs 512 + 256 x sweeps
static std::vector<uint32_t> prefix_of(const std::vector<uint32_t> &sweeps) {
    std::vector<uint32_t> cost(sweeps.size() + 1);
    uint64_t run = 0;
    for (size_t m = 0; m < sweeps.size(); m++) { cost[m] = (uint32_t)run; run += 512u + 256ull * sweeps[m]; }
    if (run >= (1ull << 32)) { printf("FAIL: a prefix beyond 32 bits\n"); return {}; }
    cost[sweeps.size()] = (uint32_t)run;
    return cost;
}

int main() {
    static const uint32_t Gs[] = {1, 3, 256};
    int bad = 0;
    // hand-built
    for (uint32_t G : Gs) {
        bad += check("M=1", prefix_of({1}), G);
        bad += check("M=1 heavy", prefix_of({2048}), G);
        bad += check("M<NC", prefix_of({1, 3, 1, 1, 200}), G);
        bad += check("M=23", prefix_of(std::vector<uint32_t>(23, 1)), G);
        bad += check("M=24", prefix_of(std::vector<uint32_t>(24, 2)), G);
        bad += check("M=32768", prefix_of(std::vector<uint32_t>(32768, 1)), G);
        {
            std::vector<uint32_t> s(32768, 1);
            for (size_t i = 0; i < s.size(); i += 3) s[i] = 2;
            bad += check("M=32768 mixed", prefix_of(s), G);
        }
        for (size_t at : {size_t(0), size_t(500), size_t(999)}) {   // one cell carrying nearly all the cost: first, in the middle, last
            std::vector<uint32_t> s(1000, 1);
            s[at] = 60000;
            bad += check("one heavy cell", prefix_of(s), G);
        }
        {   // totals near 2^32: 32768 cells of 509 sweeps are 2^32 - 2^25 + ..., then the last cell takes what is left below 2^32
            std::vector<uint32_t> s(32768, 509);
            std::vector<uint32_t> c = prefix_of(s);
            if (c.empty()) return 1;
            bad += check("total near 2^32", c, G);
            c.back() = 0xffffffffu;                            // (any strictly increasing prefix is an input: the last step longer)
            bad += check("total = 2^32 - 1", c, G);
            s.assign(16384, 1021);
            c = prefix_of(s);
            if (c.empty()) return 1;
            c.back() = 0xfffffff0u;
            bad += check("total near 2^32, M=16384", c, G);
        }
    }
    if (bad) return 1;
    printf("ok hand-built\n");
    // random cost arrays
    std::mt19937 rng(12345);
    for (int it = 0; it < 3000; it++) {
        const uint32_t M = 1 + rng() % (it % 50 == 0 ? 32768u : it % 7 == 0 ? 3000u : 100u);
        std::vector<uint32_t> s(M);
        const uint32_t shape = rng() % 4;
        for (auto &v : s) v = shape == 0 ? 1 : shape == 1 ? 1 + rng() % 4 : shape == 2 ? (rng() % 50 == 0 ? 1 + rng() % 4000 : 1) : 1 + rng() % 64;
        const std::vector<uint32_t> c = prefix_of(s);
        if (c.empty()) return 1;
        const uint32_t G = it % 3 == 0 ? Gs[rng() % 3] : 1 + rng() % 1024;
        if (check("random", c, G)) return 1;
    }
    printf("ok random\n");
    return 0;
}
