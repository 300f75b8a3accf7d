// palette_bounds_check.cpp -- a stand-alone check of cniic_amd/csrc/pal_bounds.hpp (tests/test_palette_cpu.py compiles and runs it, once
// more under -fsanitize=address,undefined).  For every palette below and every one of the 2^24 colours:
//   (a) the true lowest-index nearest entry -- a plain scan of all K entries with a strict < -- is in the candidate set of the colour's cell
//       (the entries with dmin <= B, B = the cell's smallest dmax);
//   (b) the candidate set's own lowest-index nearest (ascending walk, strict <: what the table kernel does) is that same entry.
// Nothing here comes from the library but the header under test.  Exit status 0 and a line "ok ..." per palette; the first violation is
// printed and the status is 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../cniic_amd/csrc/pal_bounds.hpp"

using namespace cniic;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return (r << 16) | (g << 8) | b; }

static std::vector<uint32_t> make_palette(const std::string &kind, uint32_t K) {
    std::vector<uint32_t> p(K);
    const uint32_t S = kPalCellSide;
    if (kind == "random") {
        for (auto &e : p) e = rnd() & 0xffffffu;
    } else if (kind == "equal") {
        const uint32_t e = rnd() & 0xffffffu;
        for (auto &x : p) x = e;
    } else if (kind == "mirrored") {   // pairs mirrored about a cell face: S - 1 and S on one axis, the other two coordinates shared
        for (uint32_t k = 0; k < K; k += 2) {
            const uint32_t face = S * (1 + rnd() % (kPalCellsPerAxis - 1)), axis = rnd() % 3, a = rnd() & 255u, b = rnd() & 255u;
            uint32_t lo[3] = {a, b, a ^ b}, hi[3];
            lo[axis] = face - 1;
            memcpy(hi, lo, sizeof hi);
            hi[axis] = face;
            const bool flip = rnd() & 1u;   // (the higher side may have the lower index)
            p[k] = flip ? rgb(hi[0], hi[1], hi[2]) : rgb(lo[0], lo[1], lo[2]);
            if (k + 1 < K) p[k + 1] = flip ? rgb(lo[0], lo[1], lo[2]) : rgb(hi[0], hi[1], hi[2]);
        }
    } else if (kind == "corners") {    // entries on cell corners: every coordinate is the first or the last of a cell
        for (auto &e : p) {
            uint32_t c[3];
            for (auto &x : c) x = S * (rnd() % kPalCellsPerAxis) + ((rnd() & 1u) ? S - 1 : 0);
            e = rgb(c[0], c[1], c[2]);
        }
    } else if (kind == "cluster") {    // one tight cluster far from most cells
        for (auto &e : p) e = rgb(250 + rnd() % 6, 3 + rnd() % 4, 128 + rnd() % 5);
    } else {
        fprintf(stderr, "unknown palette kind %s\n", kind.c_str());
        exit(2);
    }
    return p;
}

struct Failure { uint32_t cell, key, want, got; int what; };

static bool check_cell(const std::vector<uint32_t> &pal, uint32_t cell, Failure *fail, uint64_t *ncand) {
    const uint32_t K = (uint32_t)pal.size(), corner = pal_cell_corner(cell), S = kPalCellSide, N = S * S * S;
    uint32_t bound = 0xffffffffu;
    for (uint32_t k = 0; k < K; k++) { const uint32_t d = pal_box_dmax(pal[k], corner); if (d < bound) bound = d; }
    std::vector<uint32_t> cand;
    std::vector<uint8_t> is_cand(K, 0);
    for (uint32_t k = 0; k < K; k++)
        if (pal_is_candidate(pal_box_dmin(pal[k], corner), bound)) { cand.push_back(k); is_cand[k] = 1; }
    *ncand += cand.size();
    // the cell's colours, and both scans entry by entry over all of them (loops a compiler vectorises)
    std::vector<uint32_t> key(N), best(N, 0xffffffffu), bidx(N, 0), cbest(N, 0xffffffffu), cidx(N, 0);
    for (uint32_t i = 0; i < N; i++) {
        key[i] = corner + rgb(i / (S * S), (i / S) % S, i % S);
        if (pal_cell_of(key[i]) != cell) { *fail = Failure{cell, key[i], cell, pal_cell_of(key[i]), 2}; return false; }
    }
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t e = pal[k];
        for (uint32_t i = 0; i < N; i++) { const uint32_t d = pal_dist2(key[i], e); if (d < best[i]) { best[i] = d; bidx[i] = k; } }
    }
    if (cand.size() == K) {   // every entry is a candidate: the walk over the candidates IS the scan above
        cidx = bidx;
    } else {
        for (uint32_t k : cand) {
            const uint32_t e = pal[k];
            for (uint32_t i = 0; i < N; i++) { const uint32_t d = pal_dist2(key[i], e); if (d < cbest[i]) { cbest[i] = d; cidx[i] = k; } }
        }
    }
    for (uint32_t i = 0; i < N; i++) {
        if (!is_cand[bidx[i]]) { *fail = Failure{cell, key[i], bidx[i], cidx[i], 0}; return false; }
        if (cidx[i] != bidx[i]) { *fail = Failure{cell, key[i], bidx[i], cidx[i], 1}; return false; }
    }
    return true;
}

static bool check_palette(const std::string &kind, uint32_t K, unsigned threads) {
    const std::vector<uint32_t> pal = make_palette(kind, K);
    std::atomic<uint32_t> next{0};
    std::atomic<int> bad{0};
    std::atomic<uint64_t> ncand{0};
    Failure first{};
    auto work = [&]() {
        uint64_t mine = 0;
        for (uint32_t cell; !bad && (cell = next.fetch_add(1)) < kPalCells;) {
            Failure f{};
            if (!check_cell(pal, cell, &f, &mine) && !bad.exchange(1)) first = f;
        }
        ncand += mine;
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (bad) {
        const char *what[] = {"the nearest entry is not a candidate", "the candidates' nearest is another entry", "pal_cell_of disagrees with pal_cell_corner"};
        printf("FAIL %s K=%u cell %u colour %06x: %s (scan of all entries: %u, candidates: %u)\n", kind.c_str(), K, first.cell, first.key, what[first.what], first.want, first.got);
        return false;
    }
    printf("ok %s K=%u: 16777216 colours, %.1f candidates per cell\n", kind.c_str(), K, (double)ncand / kPalCells);
    return true;
}

int main(int argc, char **argv) {
    unsigned threads = argc > 1 ? (unsigned)atoi(argv[1]) : 0;
    if (!threads) threads = std::thread::hardware_concurrency();
    if (!threads) threads = 1;
    if (threads > 16) threads = 16;
    static_assert(kPalCells == 4096 && kPalCellSide * kPalCellsPerAxis == 256, "the cube is cut into whole cells");
    const char *kinds[] = {"random", "equal", "mirrored", "corners", "cluster"};
    const uint32_t Ks[] = {1, 2, 16, 256};
    bool ok = true;
    for (const char *kind : kinds)
        for (uint32_t K : Ks) ok = check_palette(kind, K, threads) && ok;
    return ok ? 0 : 1;
}
