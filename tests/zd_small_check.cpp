// zd_small_check.cpp -- cniic_amd/csrc/zd_small.hpp without a GPU: a stand-alone host program (tests/test_zd_small_cpu.py builds it plain and
// with -fsanitize=address,undefined).  The header's functions run as a scalar emulation of k_zd_small's three phases -- W lanes in a loop
// that speculate, the commit with 64 lanes over the window's list, the flush with the entries inserted in a shuffled order, which stands
// for the race -- beside a one-pass coder written here without the header: a text built byte by byte, a trie in hash maps, next_pair as
// dict.rs states it.  Usage: zd_small_check [frames.bin [streams.bin]]; frames.bin: u32 count, then per frame u32 w, u32 h and the pixels;
// streams.bin receives per frame the FNV-1a hash of the restated text (u64), the restated stream's length (u32) and its bytes, for the
// Python side to hold against tests/zip_dict_ref.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "zd_small.hpp"

using namespace cniic;

struct Frame { uint32_t w, h; std::vector<uint8_t> px; std::string name; };

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---------------------------------------------------------------- the restatement: nothing of the header
static std::vector<uint8_t> plain_text(const Frame &f) {
    std::vector<uint8_t> t;
    for (int i = 0; i < 4; i++) t.push_back((uint8_t)(f.w >> (8 * i)));
    for (int i = 0; i < 4; i++) t.push_back((uint8_t)(f.h >> (8 * i)));
    for (size_t p = 0; p < (size_t)f.w * f.h; p++) {
        t.push_back(3);
        for (int i = 0; i < 7; i++) t.push_back(0);
        for (int c = 0; c < 3; c++) t.push_back(f.px[3 * p + c]);
    }
    return t;
}
struct Plain { std::vector<uint32_t> pairs; uint32_t longest_match = 0, longest_entry = 1, entries = 0; };
static Plain plain_encode(const std::vector<uint8_t> &t, uint32_t limit) {
    std::unordered_map<uint64_t, uint32_t> child, value;
    for (uint32_t b = 0; b < 256; b++) value[b] = b;
    uint32_t nodes = 1, counter = 0x100;
    const size_t n = t.size();
    Plain out;
    auto longest = [&](size_t pos, uint32_t *sym) {
        uint64_t node = 0;
        size_t best = pos;
        for (size_t j = pos; j < n;) {
            const uint64_t k = (node << 8) | t[j];
            j++;
            auto v = value.find(k);
            if (v != value.end()) { *sym = v->second; best = j; }
            auto c = child.find(k);
            if (c == child.end()) break;
            node = c->second;
        }
        out.longest_match = std::max<uint32_t>(out.longest_match, (uint32_t)(best - pos));
        return best;
    };
    for (size_t pos = 0; pos < n;) {
        uint32_t s1 = 0, s2 = 0xFFFF;
        const size_t mid = longest(pos, &s1);
        if (mid == n) { out.pairs.push_back(s1 | (0xFFFFu << 16)); break; }
        const size_t end = longest(mid, &s2);
        out.pairs.push_back(s1 | (s2 << 16));
        if (counter < limit) {
            uint64_t node = 0;
            for (size_t j = pos; j + 1 < end; j++) {
                const uint64_t k = (node << 8) | t[j];
                auto c = child.find(k);
                if (c == child.end()) c = child.emplace(k, nodes++).first;
                node = c->second;
            }
            value[(node << 8) | t[end - 1]] = counter++;
            out.longest_entry = std::max<uint32_t>(out.longest_entry, (uint32_t)(end - pos));
            out.entries++;
        }
        pos = end;
    }
    return out;
}

// ---------------------------------------------------------------- the emulation: the header's functions in the kernel's phases
struct HostLanes {
    template <class F> static uint64_t best(F f) { uint64_t b = 0; for (uint32_t l = 0; l < 64; l++) b = std::max<uint64_t>(b, f(l, 64u)); return b; }
    static bool first() { return true; }
};
struct Emu { std::vector<uint32_t> pairs; uint32_t verdict, finished, windows; uint64_t edges, inner; };
static Emu emulate(const Frame &f, uint32_t W, uint32_t spec, uint32_t giveup, uint32_t limit, uint32_t seed) {
    const uint32_t n = f.w * f.h, N = zs_text_len(n), bits = zs_table_bits(N);
    const ZsText t{f.px.data(), f.w, f.h, N};
    std::vector<uint64_t> tab(1ull << bits, 0);
    std::vector<uint16_t> sym(W), len(W), depth(W), e_sym(kZsListCap);
    std::vector<uint32_t> node(W), e_start(kZsListCap), e_len(kZsListCap), out(zs_stride(N) / 4);
    const ZsWindow win{sym.data(), len.data(), depth.data(), node.data(), e_start.data(), e_len.data(), e_sym.data()};
    std::mt19937 rng(seed);
    ZsState st = zs_state_begin();
    uint32_t windows = 0;
    while (!st.done) {
        const uint32_t base = zs_need(st);
        for (uint32_t i = 0; i < W && base + i < N; i++) {
            ZsWalk s = zs_walk_begin(t, base + i);
            zs_walk<ZsPlainMem>(tab.data(), bits, t, base + i, spec, s);
            zs_window_put(win, i, s);
        }
        zs_commit<ZsPlainMem, HostLanes>(tab.data(), bits, t, win, base, W, limit, giveup, out.data(), st);
        CHECK(st.done || zs_need(st) > base, "%s: a window that commits nothing", f.name.c_str());
        std::vector<uint32_t> order(st.nlist);
        for (uint32_t e = 0; e < st.nlist; e++) order[e] = e;
        std::shuffle(order.begin(), order.end(), rng);
        for (uint32_t e : order) zs_insert<ZsPlainMem>(tab.data(), bits, t, e_start[e], e_len[e], e_sym[e]);
        windows++;
    }
    Emu r{{}, st.verdict, st.finished, windows, 0, 0};
    r.pairs.assign(out.begin(), out.begin() + st.pairs);
    for (uint64_t v : tab) { r.edges += v != 0; r.inner += (v & kZsChildBit) != 0; }
    // the bounds the table's size and the key's width rest on
    CHECK(r.edges + 256 <= (uint64_t)N + 256 && 2 * (r.edges + 256) <= tab.size(), "%s: %llu edges for %u bytes of text", f.name.c_str(), (unsigned long long)r.edges, N);
    CHECK(257 + r.inner < (1u << 18) && kZsFirstSlotNode + tab.size() <= (1u << 20), "%s: node numbers", f.name.c_str());
    CHECK(4ull * st.pairs <= zs_stream_max(N), "%s: %u pairs", f.name.c_str(), st.pairs);
    return r;
}

// one frame under one setting against the restatement; returns 1 when it was handed back
static int compare(const Frame &f, const Plain &want, uint32_t W, uint32_t spec, uint32_t giveup, uint32_t limit, uint32_t seed, uint32_t *finished = nullptr) {
    const Emu got = emulate(f, W, spec, giveup, limit, seed);
    if (finished) *finished += got.finished;
    const bool back = want.longest_match > giveup;
    CHECK((got.verdict == kZsHandedBack) == back, "%s W %u caps %u %u limit %#x: verdict %u, longest match %u", f.name.c_str(), W, spec, giveup, limit, got.verdict, want.longest_match);
    if (!back) CHECK(got.pairs == want.pairs, "%s W %u caps %u %u limit %#x: %zu pairs against %zu", f.name.c_str(), W, spec, giveup, limit, got.pairs.size(), want.pairs.size());
    if (!back && want.longest_entry <= spec) CHECK(got.finished == 0, "%s: a walk finished behind a cap that no entry reaches", f.name.c_str());   // (a walk is as deep as an entry at most)
    return back;
}

static uint64_t fnv(const std::vector<uint8_t> &v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : v) { h ^= b; h *= 0x100000001b3ull; }
    return h;
}

static std::vector<Frame> random_frames() {
    std::vector<Frame> v;
    std::mt19937 rng(7);
    const uint32_t colours[] = {1, 2, 3, 16, 256};
    for (int k = 0; k < 120; k++) {
        Frame f;
        f.w = 1 + rng() % 64; f.h = 1 + rng() % (2048 / f.w);
        const uint32_t c = colours[k % 5];
        std::vector<uint8_t> pal(3 * c);
        for (auto &b : pal) b = (uint8_t)rng();
        f.px.resize(3ull * f.w * f.h);
        for (size_t p = 0; p < (size_t)f.w * f.h; p++) { const uint32_t i = rng() % c; memcpy(&f.px[3 * p], &pal[3 * i], 3); }
        f.name = "random " + std::to_string(f.w) + "x" + std::to_string(f.h) + " of " + std::to_string(c);
        v.push_back(std::move(f));
    }
    return v;
}

int main(int argc, char **argv) {
    std::vector<Frame> given;
    if (argc > 1) {
        FILE *fp = fopen(argv[1], "rb");
        if (!fp) { printf("FAIL cannot read %s\n", argv[1]); return 2; }
        uint32_t cnt = 0;
        if (fread(&cnt, 4, 1, fp) != 1) cnt = 0;
        for (uint32_t i = 0; i < cnt; i++) {
            Frame f;
            if (fread(&f.w, 4, 1, fp) != 1 || fread(&f.h, 4, 1, fp) != 1) { printf("FAIL short file\n"); return 2; }
            f.px.resize(3ull * f.w * f.h);
            if (fread(f.px.data(), 1, f.px.size(), fp) != f.px.size()) { printf("FAIL short file\n"); return 2; }
            f.name = "frame " + std::to_string(i) + " " + std::to_string(f.w) + "x" + std::to_string(f.h);
            given.push_back(std::move(f));
        }
        fclose(fp);
    }
    const std::vector<Frame> rnd = random_frames();
    std::vector<const Frame *> all;
    for (const Frame &f : given) all.push_back(&f);
    for (const Frame &f : rnd) all.push_back(&f);
    const uint32_t Ws[] = {1, 2, 64, kZsWindow};

    // ---- text: zs_text_byte against the text built byte by byte; the restated streams for the Python side
    FILE *sp = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    std::vector<Plain> plain;
    uint64_t bytes = 0;
    for (size_t k = 0; k < all.size(); k++) {
        const Frame *f = all[k];
        const std::vector<uint8_t> t = plain_text(*f);
        CHECK(t.size() == zs_text_len(f->w * f->h), "%s: text length", f->name.c_str());
        for (uint32_t i = 0; i < t.size(); i++)
            if (zs_text_byte(i, f->w, f->h, f->px.data()) != t[i]) { CHECK(false, "%s: text byte %u", f->name.c_str(), i); break; }
        bytes += t.size();
        plain.push_back(plain_encode(t, kZsLimit));
        if (sp && k < given.size()) {
            const uint64_t h = fnv(t);
            const uint32_t ln = 4 * (uint32_t)plain.back().pairs.size();
            fwrite(&h, 8, 1, sp); fwrite(&ln, 4, 1, sp); fwrite(plain.back().pairs.data(), 1, ln, sp);
        }
    }
    if (sp) fclose(sp);
    printf("ok text: %zu frames, %llu bytes\n", all.size(), (unsigned long long)bytes);

    // ---- every frame at every W under the kernel's caps, three insert orders at the kernel's own W
    uint32_t runs = 0, back = 0, finished = 0;
    for (size_t k = 0; k < all.size(); k++)
        for (uint32_t W : Ws)
            for (uint32_t seed = 0; seed < (W == kZsWindow ? 3u : 1u); seed++) { back += compare(*all[k], plain[k], W, kZsSpecCap, kZsGiveUp, kZsLimit, seed, &finished); runs++; }
    printf("ok windows: %u runs, %u handed back, %u walks finished by the commit\n", runs, back, finished);

    // ---- both caps lowered: walks the commit finishes, frames handed back
    uint32_t cruns = 0, cback = 0, cfin = 0;
    const uint32_t caps[][2] = {{1, 2}, {2, 8}, {4, 24}, {8, 300}, {3, 70000}};
    for (size_t k = 0; k < all.size(); k++)
        for (const auto &c : caps)
            for (uint32_t W : {2u, kZsWindow}) { cback += compare(*all[k], plain[k], W, c[0], c[1], kZsLimit, 11, &cfin); cruns++; }
    CHECK(cback > 0 && cback < cruns && cfin > 0, "the lowered caps reach neither side");
    printf("ok caps: %u runs, %u handed back, %u walks finished by the commit\n", cruns, cback, cfin);

    // ---- the freeze rule: the symbol limit crossed early, in the middle and late
    uint32_t fruns = 0, frozen = 0;
    for (uint32_t limit : {0x104u, 0x140u, 0x1000u})
        for (size_t k = 0; k < all.size(); k++) {
            const Plain want = plain_encode(plain_text(*all[k]), limit);
            CHECK(want.entries <= limit - 0x100, "%s: %u entries under limit %#x", all[k]->name.c_str(), want.entries, limit);
            frozen += want.entries == limit - 0x100 && want.pairs.size() > want.entries;
            for (uint32_t W : Ws) { compare(*all[k], want, W, kZsSpecCap, 70000, limit, 5); fruns++; }
        }
    CHECK(frozen > 0, "no frame crosses a lowered limit");
    printf("ok freeze: %u runs, %u (frame, limit) pairs coded on with a full dictionary\n", fruns, frozen);

    // ---- the five known answers of dict.rs cannot be frames (a text starts with 8 bytes of dimensions); the 1 x 1 frame's 7 pairs are
    {
        Frame f{1, 1, {9, 8, 7}, "1x1"};
        const Plain p = plain_encode(plain_text(f), kZsLimit);
        CHECK(p.pairs.size() == 7, "1x1: %zu pairs", p.pairs.size());
        compare(f, p, kZsWindow, kZsSpecCap, kZsGiveUp, kZsLimit, 0);
    }
    printf("ok total: bound %u pixels, window %u, caps %u %u, stride at the bound %llu, table bits at the bound %u, %d mismatches\n", kZdSmallMaxPx, kZsWindow, kZsSpecCap,
           kZsGiveUp, (unsigned long long)zs_stride(zs_text_len(kZdSmallMaxPx)), zs_table_bits(zs_text_len(kZdSmallMaxPx)), g_fail);
    return g_fail ? 1 : 0;
}
