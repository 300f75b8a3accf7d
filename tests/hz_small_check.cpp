// hz_small_check.cpp -- cniic_amd/csrc/hz_small.hpp beside zd_small.hpp and zd_small_dec.hpp without a GPU: a stand-alone host program
// (tests/test_hz_small_cpu.py builds it plain and with -fsanitize=address,undefined).
//   encode  the three phases of k_hz_small as a scalar emulation over the text kind HzText -- W lanes in a loop that speculate, the commit
//           with 64 lanes over the window's list, the flush in a shuffled order, which stands for the race -- beside a one-pass coder
//           written here without the headers: the text built byte by byte, a trie in hash maps, next_pair as dict.rs states it
//   decode  the five phases of k_hz_small_dec with the lenient verdict and the record cut of hz_small.hpp, the lanes in shuffled order,
//           beside a one-pass table decoder written here without the headers, as decode_hilbert_zip restates hilbertc.rs:58-77
// A frame's pixels are given in SCAN order (the scan itself is the GPU tests' and tests/test_hilbert*.py's): this program knows none.
// Usage:  hz_small_check                                     frames, streams and a few thousand mutants made here
//         hz_small_check enc frames.bin streams.bin          frames.bin: u32 count, then per frame u32 w, u32 h and the pixels; streams.bin
//                                                            receives per frame the restated stream's length (u32) and its bytes
//         hz_small_check dec streams.bin [max_pairs hops rounds]   streams.bin: u32 count, then per stream u32 length and the bytes; one line
//                                                            per stream: "<index> <verdict> <a> <w> <h> <cut> <fnv1a of the pixels in scan order>",
//                                                            verdict -1 for a stream that is no candidate
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "hz_small.hpp"
#include "zd_small.hpp"
#include "zd_small_dec.hpp"

using namespace cniic;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Frame { uint32_t w, h; std::vector<uint8_t> px; std::string name; };   // px: scan order

// ================================================================ encode
// ---------------------------------------------------------------- the restatement: nothing of the headers
static std::vector<uint8_t> plain_text(const Frame &f) {
    std::vector<uint8_t> t;
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
static std::vector<uint8_t> plain_stream(const Frame &f, const Plain &p) {
    std::vector<uint8_t> s(8 + 4 * p.pairs.size());
    memcpy(s.data(), &f.w, 4); memcpy(s.data() + 4, &f.h, 4);
    if (!p.pairs.empty()) memcpy(s.data() + 8, p.pairs.data(), 4 * p.pairs.size());
    return s;
}

// ---------------------------------------------------------------- the emulation: the headers' functions in the kernel's phases
struct HostLanes {
    template <class F> static uint64_t best(F f) { uint64_t b = 0; for (uint32_t l = 0; l < 64; l++) b = std::max<uint64_t>(b, f(l, 64u)); return b; }
    static bool first() { return true; }
};
struct Emu { std::vector<uint32_t> pairs; uint32_t verdict, finished; };
static Emu emulate_enc(const Frame &f, uint32_t W, uint32_t spec, uint32_t giveup, uint32_t limit, uint32_t seed) {
    const uint32_t n = f.w * f.h, N = hz_text_len(n), bits = zs_table_bits(N);
    const HzText t{f.px.data(), N};
    std::vector<uint64_t> tab(1ull << bits, 0);
    std::vector<uint16_t> sym(W), len(W), depth(W), e_sym(kZsListCap);
    std::vector<uint32_t> node(W), e_start(kZsListCap), e_len(kZsListCap), slot(hz_stride(N) / 4);
    const ZsWindow win{sym.data(), len.data(), depth.data(), node.data(), e_start.data(), e_len.data(), e_sym.data()};
    uint32_t *out = slot.data() + kHzHead / 4;   // the pairs behind the head, 4-byte aligned in a slot that is a multiple of 16
    std::mt19937 rng(seed);
    ZsState st = zs_state_begin();
    while (!st.done) {
        const uint32_t base = zs_need(st);
        for (uint32_t i = 0; i < W && base + i < N; i++) {
            ZsWalk s = zs_walk_begin(t, base + i);
            zs_walk<ZsPlainMem>(tab.data(), bits, t, base + i, spec, s);
            zs_window_put(win, i, s);
        }
        zs_commit<ZsPlainMem, HostLanes>(tab.data(), bits, t, win, base, W, limit, giveup, out, st);
        CHECK(st.done || zs_need(st) > base, "%s: a window that commits nothing", f.name.c_str());
        std::vector<uint32_t> order(st.nlist);
        for (uint32_t e = 0; e < st.nlist; e++) order[e] = e;
        std::shuffle(order.begin(), order.end(), rng);
        for (uint32_t e : order) zs_insert<ZsPlainMem>(tab.data(), bits, t, e_start[e], e_len[e], e_sym[e]);
    }
    Emu r{{}, st.verdict, st.finished};
    r.pairs.assign(out, out + st.pairs);
    uint64_t edges = 0;
    for (uint64_t v : tab) edges += v != 0;
    CHECK(edges <= (uint64_t)N && 2 * (edges + 256) <= tab.size(), "%s: %llu edges for %u bytes of text", f.name.c_str(), (unsigned long long)edges, N);
    CHECK(kHzHead + 4ull * st.pairs <= hz_stream_max(N) && hz_stride(N) % 16 == 0 && hz_stride(N) >= hz_stream_max(N), "%s: %u pairs", f.name.c_str(), st.pairs);
    return r;
}
// one frame under one setting against the restatement; returns 1 when it was handed back
static int compare_enc(const Frame &f, const Plain &want, uint32_t W, uint32_t spec, uint32_t giveup, uint32_t limit, uint32_t seed, uint32_t *finished = nullptr) {
    const Emu got = emulate_enc(f, W, spec, giveup, limit, seed);
    if (finished) *finished += got.finished;
    const bool back = want.longest_match > giveup;
    CHECK((got.verdict == kZsHandedBack) == back, "%s W %u caps %u %u limit %#x: verdict %u, longest match %u", f.name.c_str(), W, spec, giveup, limit, got.verdict, want.longest_match);
    if (!back) CHECK(got.pairs == want.pairs, "%s W %u caps %u %u limit %#x: %zu pairs against %zu", f.name.c_str(), W, spec, giveup, limit, got.pairs.size(), want.pairs.size());
    if (!back && want.longest_entry <= spec) CHECK(got.finished == 0, "%s: a walk finished behind a cap that no entry reaches", f.name.c_str());
    return back;
}

static std::vector<Frame> random_frames() {
    std::vector<Frame> v;
    std::mt19937 rng(7);
    const uint32_t colours[] = {1, 2, 3, 16, 256};
    for (int k = 0; k < 100; k++) {
        Frame f;
        f.w = 1 + rng() % 64; f.h = 1 + rng() % (2048 / f.w);
        if (k < 4) { f.w = k == 2 ? 2 : 1; f.h = k == 3 ? 2 : 1; }   // 1x1 (a text of 11 bytes), 1x1, 2x1, 1x2
        if (k == 4) { f.w = 23; f.h = 1; }                          // 253 and 264 bytes: either side of one window
        if (k == 5) { f.w = 24; f.h = 1; }
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

static bool read_frames(const char *path, std::vector<Frame> &given) {
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    uint32_t cnt = 0;
    if (fread(&cnt, 4, 1, fp) != 1) cnt = 0;
    for (uint32_t i = 0; i < cnt; i++) {
        Frame f;
        if (fread(&f.w, 4, 1, fp) != 1 || fread(&f.h, 4, 1, fp) != 1) { fclose(fp); return false; }
        f.px.resize(3ull * f.w * f.h);
        if (fread(f.px.data(), 1, f.px.size(), fp) != f.px.size()) { fclose(fp); return false; }
        f.name = "frame " + std::to_string(i) + " " + std::to_string(f.w) + "x" + std::to_string(f.h);
        given.push_back(std::move(f));
    }
    fclose(fp);
    return true;
}

static void check_encode(const std::vector<Frame> &frames, FILE *sp) {
    const uint32_t Ws[] = {1, 2, 64, kZsWindow};
    std::vector<Plain> plain;
    uint64_t bytes = 0;
    for (const Frame &f : frames) {
        const std::vector<uint8_t> t = plain_text(f);
        CHECK(t.size() == hz_text_len(f.w * f.h), "%s: text length", f.name.c_str());
        for (uint32_t i = 0; i < t.size(); i++)
            if (hz_text_byte(i, f.px.data()) != t[i]) { CHECK(false, "%s: text byte %u", f.name.c_str(), i); break; }
        bytes += t.size();
        plain.push_back(plain_encode(t, kZsLimit));
        if (sp) {
            const std::vector<uint8_t> s = plain_stream(f, plain.back());
            const uint32_t ln = (uint32_t)s.size();
            fwrite(&ln, 4, 1, sp); fwrite(s.data(), 1, ln, sp);
        }
    }
    printf("ok text: %zu frames, %llu bytes\n", frames.size(), (unsigned long long)bytes);
    // ---- every frame at every W under the kernel's caps, three insert orders at the kernel's own W
    uint32_t runs = 0, back = 0, finished = 0;
    for (size_t k = 0; k < frames.size(); k++)
        for (uint32_t W : Ws)
            for (uint32_t seed = 0; seed < (W == kZsWindow ? 3u : 1u); seed++) { back += compare_enc(frames[k], plain[k], W, kZsSpecCap, kZsGiveUp, kZsLimit, seed, &finished); runs++; }
    printf("ok windows: %u runs, %u handed back, %u walks finished by the commit\n", runs, back, finished);
    // ---- both caps lowered: walks the commit finishes, frames handed back
    uint32_t cruns = 0, cback = 0, cfin = 0;
    const uint32_t caps[][2] = {{1, 2}, {2, 8}, {4, 24}, {8, 300}, {3, 70000}};
    for (size_t k = 0; k < frames.size(); k++)
        for (const auto &c : caps)
            for (uint32_t W : {2u, kZsWindow}) { cback += compare_enc(frames[k], plain[k], W, c[0], c[1], kZsLimit, 11, &cfin); cruns++; }
    CHECK(cback > 0 && cback < cruns && cfin > 0, "the lowered caps reach neither side");
    printf("ok caps: %u runs, %u handed back, %u walks finished by the commit\n", cruns, cback, cfin);
    // ---- the freeze rule: the symbol limit crossed early and in the middle
    uint32_t fruns = 0, frozen = 0;
    for (uint32_t limit : {0x104u, 0x140u})
        for (size_t k = 0; k < frames.size(); k++) {
            const Plain want = plain_encode(plain_text(frames[k]), limit);
            frozen += want.entries == limit - 0x100 && want.pairs.size() > want.entries;
            for (uint32_t W : {1u, kZsWindow}) { compare_enc(frames[k], want, W, kZsSpecCap, 70000, limit, 5); fruns++; }
        }
    CHECK(frozen > 0, "no frame crosses a lowered limit");
    printf("ok freeze: %u runs, %u (frame, limit) pairs coded on with a full dictionary\n", fruns, frozen);
}

// ================================================================ decode
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

struct Outcome {
    int verdict = -1;   // -1: no candidate
    uint32_t a = 0, w = 0, h = 0, cut = 0;
    std::vector<uint8_t> px;   // scan order
    bool operator==(const Outcome &o) const { return verdict == o.verdict && a == o.a && w == o.w && h == o.h && cut == o.cut && px == o.px; }
};
struct Caps { uint32_t max_pairs, hops, rounds; };

// ---------------------------------------------------------------- the table decoder (no header): DictDecoder::next, lazily
namespace table {
constexpr uint64_t kBig = 1ull << 40;
struct Dec {
    std::vector<uint64_t> off, len;
    std::vector<int> gen;
    uint64_t pairs = 0, produced = 0;
    uint32_t counter = 0x100;
    Dec() : off(65536, 0), len(65536, 0), gen(65536, -1) { for (int b = 0; b < 256; b++) len[b] = 1; }
    bool scan(const uint8_t *p, uint64_t npairs, uint64_t need) {
        while (pairs < npairs && produced < need) {
            const uint8_t *q = p + 4 * pairs;
            const uint32_t s1 = q[0] | (q[1] << 8), s2 = q[2] | (q[3] << 8);
            if ((s1 != 0xFFFF && s1 >= counter) || (s2 != 0xFFFF && s2 >= counter)) return false;
            off[counter] = produced; len[counter] = std::min(len[s1] + len[s2], kBig);
            gen[counter] = std::max(gen[s1], gen[s2]) + 1;
            counter++;
            produced = std::min(produced + len[counter - 1], kBig);
            pairs++;
        }
        return true;
    }
    void write(const uint8_t *p, uint64_t limit, std::vector<uint8_t> &out, std::vector<uint32_t> &visits) const {
        out.assign(limit, 0); visits.assign(limit, 0);
        uint64_t o = 0;
        for (uint64_t k = 0; k < pairs && o < limit; k++)
            for (int i = 0; i < 2 && o < limit; i++) {
                const uint32_t s = p[4 * k + 2 * i] | (p[4 * k + 2 * i + 1] << 8);
                if (s == 0xFFFF) continue;
                if (s < 256) { out[o] = (uint8_t)s; visits[o] = 1; o++; continue; }
                const uint64_t n = std::min(len[s], limit - o);
                for (uint64_t j = 0; j < n; j++) { out[o + j] = out[off[s] + j]; visits[o + j] = visits[off[s] + j] + 1; }
                o += n;
            }
    }
};

// the whole stream: 8 raw bytes of dimensions, then the pairs
static Outcome decode(const uint8_t *s, uint64_t slen, const Caps &caps) {
    Outcome r;
    if (slen < 8) return r;
    memcpy(&r.w, s, 4); memcpy(&r.h, s + 4, 4);
    const uint64_t npx = (uint64_t)r.w * r.h;
    if (!npx || npx > 16384) return r;
    const uint8_t *p = s + 8;
    const uint64_t n = slen - 8, need = 11 * npx, P = std::min<uint64_t>(n / 4, caps.max_pairs);
    {
        Dec all;
        all.scan(p, P, ~0ull);
        int deepest = -1;
        for (uint64_t k = 0; k < all.pairs; k++) deepest = std::max(deepest, all.gen[0x100 + k]);
        if (deepest >= (int)caps.rounds) { r.verdict = 1; return r; }
    }
    Dec d;
    const bool good = d.scan(p, P, need);
    if (d.produced < need) {
        if (!good) { r.verdict = 2; r.a = (uint32_t)d.pairs; return r; }
        if (P < n / 4) { r.verdict = 1; return r; }
        if ((n & 3) >= 2) { r.verdict = 3; return r; }
    }
    // the colours end where the text does, or at the first record whose length is not 3
    const uint64_t records = std::min(d.produced, need) / 11;
    std::vector<uint8_t> text; std::vector<uint32_t> visits;
    d.write(p, 11 * records, text, visits);
    uint64_t cut = records;
    for (uint64_t i = 0; i < records && cut == records; i++) {
        bool ok = text[11 * i] == 3;
        for (int j = 1; j < 8; j++) ok = ok && text[11 * i + j] == 0;
        if (!ok) cut = i;
    }
    // what the kernel reads: the 8 length bytes of every record reached, the colours below the cut
    for (uint64_t i = 0; i < records; i++)
        for (int j = 0; j < (i < cut ? 11 : 8); j++) if (visits[11 * i + j] > caps.hops) { r.verdict = 1; return r; }
    r.verdict = 0;
    r.cut = (uint32_t)cut;
    r.px.assign(3 * npx, 0);
    for (uint64_t i = 0; i < cut; i++) memcpy(r.px.data() + 3 * i, text.data() + 11 * i + 8, 3);
    return r;
}
}  // namespace table

struct BytePairs {
    const uint8_t *p;
    uint32_t operator()(uint32_t k) const { return zsd_word_from_bytes(p + 4ull * k); }
};

static Outcome emulate_dec(const uint8_t *s, uint64_t slen, const Caps &caps, uint32_t lanes) {
    Outcome r;
    memcpy(&r.w, s, 4); memcpy(&r.h, s + 4, 4);
    const uint8_t *p = s + kHzHead;
    const uint64_t n = slen - kHzHead;
    const uint32_t npx = r.w * r.h, need = hzd_need(npx), C = need + 1, P = (uint32_t)std::min<uint64_t>(n / 4, caps.max_pairs);
    const BytePairs pairs{p};
    std::vector<uint32_t> O(P + 1, kZsdUnknown);
    // 1
    uint32_t kb = P;
    for (uint32_t lane = 0; lane < lanes; lane++)
        for (uint32_t k = lane; k < P; k += lanes)
            if (zsd_pair_bad(pairs(k), k)) { kb = std::min(kb, k); break; }
    // 2: the lanes of a round in shuffled order
    std::vector<uint32_t> order(lanes);
    for (uint32_t i = 0; i < lanes; i++) order[i] = i;
    for (uint32_t round = 0;; round++) {
        if (round == caps.rounds) { r.verdict = kHzdHandedBack; return r; }
        for (uint32_t i = lanes; i > 1; i--) std::swap(order[i - 1], order[rnd() % i]);
        for (uint32_t i = 0; i < lanes; i++)
            for (uint32_t k = order[i]; k < kb; k += lanes) zsd_resolve(pairs(k), k, O.data(), C);
        bool unknown = false;
        for (uint32_t k = 0; k < kb; k++) unknown |= zsd_settle(k, O.data());
        if (!unknown) break;
    }
    // 3
    {
        const uint32_t run = (kb + lanes - 1) / lanes;
        std::vector<uint32_t> sum(lanes, 0);
        for (uint32_t lane = 0; lane < lanes; lane++)
            for (uint32_t k = std::min(lane * run, kb); k < std::min(lane * run + run, kb); k++) sum[lane] = zsd_sat_add(sum[lane], O[k], C);
        uint32_t before = 0;
        for (uint32_t lane = 0; lane < lanes; lane++) {
            uint32_t off = before;
            for (uint32_t k = std::min(lane * run, kb); k < std::min(lane * run + run, kb); k++) { const uint32_t l = O[k]; O[k] = off; off = zsd_sat_add(off, l, C); }
            before = zsd_sat_add(before, sum[lane], C);
        }
        O[kb] = before;
    }
    // 4
    const uint32_t v = hzd_verdict(O[kb], need, kb, P, n, &r.a);
    if (v != kHzdOk) { r.verdict = (int)v; return r; }
    // 5: the length bytes, the cut, the colours (the scan is the identity here)
    const uint32_t records = hzd_records(O[kb], need);
    uint32_t bad = npx;
    for (uint32_t j = 0; j < 8 * records; j++) {
        uint8_t byte = 0;
        if (!zsd_byte(pairs, O.data(), kb, 11 * (j >> 3) + (j & 7), caps.hops, &byte)) { r.verdict = kHzdHandedBack; return r; }
        if (!zsd_record_byte_ok(j & 7, byte)) bad = std::min(bad, j >> 3);
    }
    const uint32_t cut = hzd_cut(records, bad);
    std::vector<uint8_t> img(3 * npx, 0);
    for (uint32_t j = 0; j < 3 * cut; j++) {
        uint8_t byte = 0;
        if (!zsd_byte(pairs, O.data(), kb, 11 * (j / 3) + 8 + j % 3, caps.hops, &byte)) { r.verdict = kHzdHandedBack; return r; }
        img[j] = byte;
    }
    r.verdict = kHzdOk;
    r.cut = cut;
    r.px.swap(img);
    return r;
}

static Outcome check_stream(const std::vector<uint8_t> &s, const Caps &caps, const char *what) {
    const Outcome want = table::decode(s.data(), s.size(), caps);
    if (want.verdict < 0) return want;
    static const uint32_t kLanes[] = {1, 7, 64, 1024};
    for (uint32_t lanes : kLanes) {
        const Outcome got = emulate_dec(s.data(), s.size(), caps, lanes);
        CHECK(got == want, "%s: %u lanes, caps %u %u %u: verdict %d (%u) cut %u against %d (%u) cut %u", what, lanes, caps.max_pairs, caps.hops, caps.rounds, got.verdict, got.a,
              got.cut, want.verdict, want.a, want.cut);
    }
    return want;
}

static uint64_t fnv(const std::vector<uint8_t> &v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : v) { h ^= b; h *= 0x100000001b3ull; }
    return h;
}

static void check_decode(const std::vector<Frame> &frames) {
    const Caps full{kZsdMaxPairs, kZsdHops, kZsdRounds};
    uint32_t verdicts[4] = {0, 0, 0, 0}, zero_filled = 0, none = 0, streams = 0, mutants = 0;
    auto tally = [&](const Outcome &o, uint32_t npx) {
        if (o.verdict < 0) { none++; return; }
        verdicts[o.verdict]++;
        zero_filled += o.verdict == 0 && o.cut < npx;
    };
    std::vector<std::vector<uint8_t>> good;
    for (size_t k = 0; k < frames.size(); k += 3) {
        const Frame &f = frames[k];
        const std::vector<uint8_t> s = plain_stream(f, plain_encode(plain_text(f), kZsLimit));
        const Outcome o = check_stream(s, full, f.name.c_str());
        CHECK(o.verdict == 0 && o.cut == f.w * f.h && o.px == f.px, "%s: the round trip", f.name.c_str());
        tally(o, f.w * f.h);
        good.push_back(s);
        streams++;
        // a record whose length byte is 4, 2 or 1, at the first pixel, a middle pixel and the last
        const uint32_t npx = f.w * f.h;
        for (uint32_t at : {0u, npx / 2, npx - 1})
            for (uint8_t lenb : {4, 2, 1}) {
                std::vector<uint8_t> t = plain_text(f);
                t[11 * at] = lenb;
                Frame g = f;
                const Plain pl = plain_encode(t, kZsLimit);
                const std::vector<uint8_t> sb = plain_stream(g, pl);
                const Outcome ob = check_stream(sb, full, "bad record");
                CHECK(ob.verdict == 0 && ob.cut == at, "%s: record %u of length %u cuts at %u", f.name.c_str(), at, lenb, ob.cut);
                streams++;
            }
    }
    // mutants: a byte changed, the stream cut, garbage behind it, other dimensions
    for (size_t k = 0; k < good.size(); k++)
        for (int m = 0; m < 60; m++) {
            std::vector<uint8_t> s = good[k];
            switch (m % 6) {
            case 0: s[8 + rnd() % (s.size() - 8)] = (uint8_t)rnd(); break;
            case 1: s.resize(rnd() % (s.size() + 1)); break;
            case 2: { const uint32_t at = 8 + 4 * (rnd() % ((s.size() - 8) / 4)); const uint32_t sym = 0x100 + (at - 8) / 4 + rnd() % 3; s[at] = (uint8_t)sym; s[at + 1] = (uint8_t)(sym >> 8); break; }
            case 3: for (uint32_t g = 1 + rnd() % 40; g; g--) s.push_back((uint8_t)rnd()); break;
            case 4: { uint32_t w, h; memcpy(&w, s.data(), 4); memcpy(&h, s.data() + 4, 4); w = rnd() % 3 ? w + rnd() % 5 : rnd() % (w + 1); memcpy(s.data(), &w, 4); if (!(rnd() % 7)) { h = 0; memcpy(s.data() + 4, &h, 4); } break; }
            case 5: s.resize(8 + 4 * (rnd() % ((s.size() - 8) / 4 + 1)) + rnd() % 4); break;
            }
            uint32_t w = 0, h = 0;
            if (s.size() >= 8) { memcpy(&w, s.data(), 4); memcpy(&h, s.data() + 4, 4); }
            tally(check_stream(s, full, "mutant"), w * h);
            mutants++;
        }
    CHECK(verdicts[0] && verdicts[2] && verdicts[3] && zero_filled && none, "the mutants miss a verdict: %u %u %u %u, %u zero-filled, %u no candidates", verdicts[0], verdicts[1],
          verdicts[2], verdicts[3], zero_filled, none);
    printf("ok decode: %u streams, %u mutants: %u ok (%u zero-filled), %u bad symbol, %u dangling, %u no candidates\n", streams, mutants, verdicts[0], zero_filled, verdicts[2],
           verdicts[3], none);
    // lowered caps: every frame on both sides of its own pair count, depth and generations
    uint32_t back = 0, kept = 0;
    for (size_t k = 0; k < good.size(); k++) {
        const std::vector<uint8_t> &s = good[k];
        const uint32_t P = (uint32_t)((s.size() - 8) / 4);
        for (const Caps &c : {Caps{P - 1 ? P - 1 : 1, kZsdHops, kZsdRounds}, Caps{P, kZsdHops, kZsdRounds}, Caps{P + 1, kZsdHops, kZsdRounds}, Caps{kZsdMaxPairs, 1, kZsdRounds},
                              Caps{kZsdMaxPairs, 2, kZsdRounds}, Caps{kZsdMaxPairs, 4, kZsdRounds}, Caps{kZsdMaxPairs, kZsdHops, 1}, Caps{kZsdMaxPairs, kZsdHops, 2},
                              Caps{kZsdMaxPairs, kZsdHops, 5}}) {
            const Outcome o = check_stream(s, c, "caps");
            back += o.verdict == 1; kept += o.verdict == 0;
        }
    }
    CHECK(back && kept, "the lowered caps reach neither side: %u handed back, %u kept", back, kept);
    printf("ok decode caps: %u handed back, %u kept\n", back, kept);
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "enc")) {
        std::vector<Frame> given;
        if (!read_frames(argv[2], given)) { printf("FAIL cannot read %s\n", argv[2]); return 2; }
        FILE *sp = fopen(argv[3], "wb");
        if (!sp) { printf("FAIL cannot write %s\n", argv[3]); return 2; }
        check_encode(given, sp);
        fclose(sp);
    } else if (argc >= 3 && !strcmp(argv[1], "dec")) {
        Caps caps{kZsdMaxPairs, kZsdHops, kZsdRounds};
        if (argc >= 6) caps = Caps{(uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[5])};
        FILE *fp = fopen(argv[2], "rb");
        if (!fp) { printf("FAIL cannot read %s\n", argv[2]); return 2; }
        uint32_t cnt = 0;
        if (fread(&cnt, 4, 1, fp) != 1) cnt = 0;
        for (uint32_t i = 0; i < cnt; i++) {
            uint32_t ln = 0;
            if (fread(&ln, 4, 1, fp) != 1) { printf("FAIL short file\n"); return 2; }
            std::vector<uint8_t> s(ln);
            if (ln && fread(s.data(), 1, ln, fp) != ln) { printf("FAIL short file\n"); return 2; }
            const Outcome o = check_stream(s, caps, "given");
            printf("%u %d %u %u %u %u %016llx\n", i, o.verdict, o.a, o.w, o.h, o.cut, (unsigned long long)fnv(o.px));
        }
        fclose(fp);
    } else {
        const std::vector<Frame> rnd_frames = random_frames();
        check_encode(rnd_frames, nullptr);
        check_decode(rnd_frames);
    }
    printf("ok total: bound %u pixels, window %u, caps %u %u, stride at the bound %llu, table bits at the bound %u, pair cap %u, %d mismatches\n", kHzSmallMaxPx, kZsWindow,
           kZsSpecCap, kZsGiveUp, (unsigned long long)hz_stride(hz_text_len(kHzSmallMaxPx)), zs_table_bits(hz_text_len(kHzSmallMaxPx)), kZsdMaxPairs, g_fail);
    return g_fail ? 1 : 0;
}
