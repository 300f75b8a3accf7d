// zd_small_dec_check.cpp -- cniic_amd/csrc/zd_small_dec.hpp without a GPU: a stand-alone host program (tests/test_zd_small_dec_cpu.py builds it
// plain and with -fsanitize=address,undefined).  The header's functions run as a scalar emulation of k_zd_small_dec's five phases -- the
// lanes in a loop, in shuffled order inside every round of phase 2 -- and every frame's outcome is compared with a one-pass table decoder
// written here without the header, as dict.rs states it: the verdict, the numbers of its message, the pixels, and whether the frame is
// handed back (pairs behind the cap, generations, visits -- all three tracked by the table decoder in its own way).
// Usage: zd_small_dec_check [streams.bin [max_pairs hops rounds]]; streams.bin: u32 count, then per stream u32 length and the bytes.  One
// line per stream: "<index> <verdict> <a> <b> <w> <h> <fnv1a of the pixels>", verdict -1 for a stream that is no candidate.  Without a file:
// streams made here, a few thousand mutants of them, lowered caps, and the saturating scan against 128-bit sums.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zd_small_dec.hpp"

using namespace cniic;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

struct Outcome {
    int verdict = -1;   // -1: no candidate
    uint32_t a = 0, b = 0, w = 0, h = 0;
    std::vector<uint8_t> px;
    bool operator==(const Outcome &o) const { return verdict == o.verdict && a == o.a && b == o.b && w == o.w && h == o.h && px == o.px; }
};
struct Caps { uint32_t max_pairs, hops, rounds; };

// ------------------------------------------------------------------ the table decoder (no header): DictDecoder::next, lazily
namespace table {
constexpr uint64_t kBig = 1ull << 40;   // lengths and positions saturate far above any text asked for
struct Dec {
    std::vector<uint64_t> off, len;
    std::vector<int> gen;
    uint64_t pairs = 0, produced = 0;
    uint32_t counter = 0x100;
    Dec() : off(65536, 0), len(65536, 0), gen(65536, -1) { for (int b = 0; b < 256; b++) len[b] = 1; }
    // whole pairs while fewer than `need` bytes are there; false: a symbol not handed out yet
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
    // the text below `limit`, and per byte how many pairs a reader visits from the pair that wrote it down to its literal
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

static Outcome decode(const uint8_t *p, uint64_t n, const Caps &caps) {
    Outcome r;
    {   // the head: 16 pairs at most
        Dec d;
        if (!d.scan(p, std::min<uint64_t>(n / 4, 16), 8) || d.produced < 8) return r;
        std::vector<uint8_t> t; std::vector<uint32_t> v;
        d.write(p, 8, t, v);
        r.w = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
        r.h = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    }
    const uint64_t npx = (uint64_t)r.w * r.h;
    if (!npx || npx > 16384) return r;
    const uint64_t need = 8 + 11 * npx, P = std::min<uint64_t>(n / 4, caps.max_pairs);
    // the generations of every pair the kernel looks at: those before the first bad one among P, whatever the text needs
    {
        Dec all;
        all.scan(p, P, ~0ull);   // (never reached: every pair)
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
        r.verdict = 4; r.a = (uint32_t)d.produced; r.b = (uint32_t)need;
        return r;
    }
    std::vector<uint8_t> text; std::vector<uint32_t> visits;
    d.write(p, need, text, visits);
    for (uint64_t t = 8; t < need; t++) if (visits[t] > caps.hops) { r.verdict = 1; return r; }
    for (uint64_t i = 0; i < npx; i++) {
        const uint8_t *rec = text.data() + 8 + 11 * i;
        bool ok = rec[0] == 3;
        for (int j = 1; j < 8; j++) ok = ok && rec[j] == 0;
        if (!ok) { r.verdict = 5; r.a = (uint32_t)i; return r; }
    }
    r.verdict = 0;
    r.px.resize(3 * npx);
    for (uint64_t i = 0; i < npx; i++) memcpy(r.px.data() + 3 * i, text.data() + 8 + 11 * i + 8, 3);
    return r;
}
}  // namespace table

// ------------------------------------------------------------------ the header's functions, phase by phase, `lanes` lanes
struct BytePairs {
    const uint8_t *p;
    uint32_t operator()(uint32_t k) const { return zsd_word_from_bytes(p + 4ull * k); }
};

static Outcome emulate(const uint8_t *p, uint64_t n, uint32_t w, uint32_t h, const Caps &caps, uint32_t lanes) {
    Outcome r;
    r.w = w; r.h = h;
    const uint32_t npx = w * h, need = zsd_need(npx), C = need + 1, P = (uint32_t)std::min<uint64_t>(n / 4, caps.max_pairs);
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
        if (round == caps.rounds) { r.verdict = kZsdHandedBack; return r; }
        for (uint32_t i = lanes; i > 1; i--) std::swap(order[i - 1], order[rnd() % i]);
        for (uint32_t i = 0; i < lanes; i++)
            for (uint32_t k = order[i]; k < kb; k += lanes) zsd_resolve(pairs(k), k, O.data(), C);
        bool unknown = false;
        for (uint32_t k = 0; k < kb; k++) unknown |= zsd_settle(k, O.data());
        if (!unknown) break;
    }
    // 3: a run per lane, the lanes' sums scanned
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
    const uint32_t v = zsd_verdict(O[kb], need, kb, P, n, &r.a, &r.b);
    if (v != kZsdOk) { r.verdict = (int)v; return r; }
    // 5
    std::vector<uint8_t> img(3 * npx);
    uint32_t bad = npx;
    for (uint32_t t = 8; t < need; t++) {
        uint8_t byte = 0;
        if (!zsd_byte(pairs, O.data(), kb, t, caps.hops, &byte)) { r.verdict = kZsdHandedBack; return r; }
        const uint32_t j = t - 8, px = j / 11, rr = j - 11 * px;
        if (rr >= 8) img[3 * px + rr - 8] = byte;
        else if (!zsd_record_byte_ok(rr, byte)) bad = std::min(bad, px);
    }
    if (bad < npx) { r.verdict = kZsdBadRecord; r.a = bad; return r; }
    r.verdict = kZsdOk;
    r.px.swap(img);
    return r;
}

static Outcome check_stream(const std::vector<uint8_t> &s, const Caps &caps, const char *what) {
    const Outcome want = table::decode(s.data(), s.size(), caps);
    {   // the head as the host reads it
        uint32_t w = 0, h = 0;
        table::Dec d;
        const bool want_dims = d.scan(s.data(), std::min<uint64_t>(s.size() / 4, 16), 8) && d.produced >= 8;
        const bool got_dims = zsd_head_dims(s.data(), std::min<uint64_t>(s.size(), 64), &w, &h);
        CHECK(got_dims == want_dims && (!got_dims || (w == want.w && h == want.h)), "%s: the head: %d %u x %u against %d %u x %u", what, got_dims, w, h, want_dims, want.w, want.h);
    }
    if (want.verdict < 0) return want;
    static const uint32_t kLanes[] = {1, 7, 64, 1024};
    for (uint32_t lanes : kLanes) {
        const Outcome got = emulate(s.data(), s.size(), want.w, want.h, caps, lanes);
        CHECK(got == want, "%s: %u lanes, caps %u %u %u: verdict %d (%u, %u) against %d (%u, %u)", what, lanes, caps.max_pairs, caps.hops, caps.rounds, got.verdict, got.a, got.b,
              want.verdict, want.a, want.b);
    }
    return want;
}

// ------------------------------------------------------------------ streams made here: a plain greedy coder (longest entry by search), enough for a check's inputs
static std::vector<uint8_t> text_of(uint32_t w, uint32_t h, int kind) {
    std::vector<uint8_t> t(8 + 11ull * w * h, 0);
    for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(w >> (8 * i)); t[4 + i] = (uint8_t)(h >> (8 * i)); }
    for (uint32_t i = 0; i < w * h; i++) {
        uint8_t *rec = t.data() + 8 + 11ull * i;
        rec[0] = 3;
        for (int c = 0; c < 3; c++) rec[8 + c] = kind == 0 ? (uint8_t)(93 + 52 * c) : kind == 1 ? (uint8_t)rnd() : (uint8_t)((i / 3 + c * 40) + (rnd() & 3));
    }
    return t;
}
static std::vector<uint8_t> encode(const std::vector<uint8_t> &t) {
    std::vector<std::string> entry;   // entry k has symbol 0x100 + k
    std::vector<uint8_t> out;
    auto longest = [&](size_t pos, uint32_t *sym) {
        size_t best = 1;
        *sym = t[pos];
        for (size_t k = 0; k < entry.size(); k++)
            if (entry[k].size() > best && entry[k].size() <= t.size() - pos && !memcmp(entry[k].data(), t.data() + pos, entry[k].size())) { best = entry[k].size(); *sym = 0x100 + (uint32_t)k; }
        return best;
    };
    for (size_t pos = 0; pos < t.size();) {
        uint32_t s1, s2 = 0xFFFF;
        const size_t l1 = longest(pos, &s1);
        size_t l2 = 0;
        if (pos + l1 < t.size()) l2 = longest(pos + l1, &s2);
        out.push_back((uint8_t)s1); out.push_back((uint8_t)(s1 >> 8)); out.push_back((uint8_t)s2); out.push_back((uint8_t)(s2 >> 8));
        entry.emplace_back(reinterpret_cast<const char *>(t.data()) + pos, l1 + l2);
        pos += l1 + l2;
    }
    return out;
}
static void put_pair(std::vector<uint8_t> &s, uint32_t s1, uint32_t s2) { s.push_back((uint8_t)s1); s.push_back((uint8_t)(s1 >> 8)); s.push_back((uint8_t)s2); s.push_back((uint8_t)(s2 >> 8)); }
// a black frame of n x 1 whose entries chain D deep (tests/test_zd_small_decode.py builds the same)
static std::vector<uint8_t> chain(uint32_t D) {
    uint32_t m = 0;
    for (uint32_t j = 2; j <= D + 1; j++) m += j;
    const uint32_t n = 1 + m;
    std::vector<uint8_t> s;
    put_pair(s, n & 255, (n >> 8) & 255); put_pair(s, (n >> 16) & 255, n >> 24); put_pair(s, 1, 0); put_pair(s, 0, 0);
    put_pair(s, 3, 0); put_pair(s, 0, 0); put_pair(s, 0x105, 0x105); put_pair(s, 0, 0x105); put_pair(s, 0x104, 0x106); put_pair(s, 0x107, 0x105); put_pair(s, 0x108, 0x109);
    for (uint32_t j = 0; j < D; j++) put_pair(s, 0x10A + j, 0x10A);
    return s;
}

static void saturation() {
    // zsd_sat_add is associative on operands <= C: any grouping of a sum gives min(the 128-bit sum, C)
    for (int trial = 0; trial < 2000; trial++) {
        const uint32_t C = 20 + rnd() % 180234, n = 1 + rnd() % 300;
        std::vector<uint32_t> v(n);
        unsigned __int128 exact = 0;
        for (uint32_t &x : v) { x = (rnd() & 3) ? rnd() % 40 : rnd() % (C + 1); exact += x; }
        const uint32_t want = exact < C ? (uint32_t)exact : C;
        uint32_t left = 0;
        for (uint32_t x : v) left = zsd_sat_add(left, x, C);
        std::vector<uint32_t> tree(v);   // pairwise
        while (tree.size() > 1) {
            std::vector<uint32_t> next;
            for (size_t i = 0; i < tree.size(); i += 2) next.push_back(i + 1 < tree.size() ? zsd_sat_add(tree[i], tree[i + 1], C) : tree[i]);
            tree.swap(next);
        }
        const uint32_t cut = rnd() % n;
        uint32_t a = 0, b = 0;
        for (uint32_t i = 0; i < cut; i++) a = zsd_sat_add(a, v[i], C);
        for (uint32_t i = cut; i < n; i++) b = zsd_sat_add(b, v[i], C);
        CHECK(left == want && tree[0] == want && zsd_sat_add(a, b, C) == want, "saturating sums: %u %u %u against %u", left, tree[0], zsd_sat_add(a, b, C), want);
    }
    // 24 576 pairs that each claim C: the unclamped u32 sum would wrap
    const uint32_t C = zsd_need(kZdSmallDecMaxPx) + 1;
    uint32_t s = 0;
    for (uint32_t k = 0; k < kZsdMaxPairs; k++) s = zsd_sat_add(s, C, C);
    CHECK(s == C && (uint64_t)kZsdMaxPairs * C > 0xFFFFFFFFull, "the sum of the largest claims");
    for (uint32_t r = 0; r < 4; r++) {
        const uint8_t bytes[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        uint32_t lo, hi;
        memcpy(&lo, bytes, 4); memcpy(&hi, bytes + 4, 4);
        CHECK(zsd_word_from_aligned(lo, hi, r) == zsd_word_from_bytes(bytes + r), "a pair at residue %u", r);
    }
}

static uint64_t fnv(const std::vector<uint8_t> &v) {
    uint64_t hsh = 0xcbf29ce484222325ull;
    for (uint8_t b : v) { hsh ^= b; hsh *= 0x100000001b3ull; }
    return hsh;
}

int main(int argc, char **argv) {
    Caps caps{kZsdMaxPairs, kZsdHops, kZsdRounds};
    if (argc >= 5) caps = Caps{(uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4])};
    if (argc >= 2) {
        FILE *fp = fopen(argv[1], "rb");
        if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
        uint32_t count = 0;
        if (fread(&count, 4, 1, fp) != 1) return 2;
        for (uint32_t i = 0; i < count; i++) {
            uint32_t len = 0;
            if (fread(&len, 4, 1, fp) != 1) return 2;
            std::vector<uint8_t> s(len);
            if (len && fread(s.data(), 1, len, fp) != len) return 2;
            const Outcome o = check_stream(s, caps, "file");
            printf("%u %d %u %u %u %u %016llx\n", i, o.verdict, o.a, o.b, o.w, o.h, (unsigned long long)fnv(o.px));
        }
        fclose(fp);
    } else {
        saturation();
        std::vector<std::vector<uint8_t>> base;
        const uint32_t sizes[][2] = {{1, 1}, {2, 1}, {5, 1}, {7, 3}, {13, 5}, {32, 8}};
        for (auto &wh : sizes)
            for (int kind = 0; kind < 3; kind++) base.push_back(encode(text_of(wh[0], wh[1], kind)));
        for (uint32_t D : {3u, 20u, 63u, 64u, 65u}) base.push_back(chain(D));
        int verdicts[6] = {0, 0, 0, 0, 0, 0};
        for (const auto &s : base) {
            const Outcome o = check_stream(s, caps, "base");
            CHECK(o.verdict == 0 || o.verdict == 1, "a good stream: verdict %d", o.verdict);
            for (const Caps &low : {Caps{(uint32_t)s.size() / 4 - 1, kZsdHops, kZsdRounds}, Caps{kZsdMaxPairs, 3, kZsdRounds}, Caps{kZsdMaxPairs, kZsdHops, 3}, Caps{40, 5, 5}, Caps{kZsdMaxPairs, 1, 1}})
                check_stream(s, low, "lowered caps");
        }
        for (int m = 0; m < 4000; m++) {
            std::vector<uint8_t> s = base[rnd() % base.size()];
            const int edits = 1 + rnd() % 3;
            for (int e = 0; e < edits; e++) {
                const size_t at = rnd() % s.size();
                s[at] = (rnd() & 1) ? (uint8_t)rnd() : (uint8_t)(s[at] ^ (1u << (rnd() & 7)));
            }
            if (m % 7 == 0) s.resize(rnd() % (s.size() + 1));
            if (m % 11 == 0) for (int e = rnd() % 8; e > 0; e--) s.push_back((uint8_t)rnd());
            const Outcome o = check_stream(s, (m & 3) ? caps : Caps{1 + rnd() % 200, 1 + rnd() % 8, 1 + rnd() % 8}, "mutant");
            if (o.verdict >= 0) verdicts[o.verdict]++;
        }
        printf("mutants by verdict: ok %d, handed back %d, bad symbol %d, dangling %d, short %d, bad record %d\n", verdicts[0], verdicts[1], verdicts[2], verdicts[3], verdicts[4],
               verdicts[5]);
        for (int v = 0; v < 6; v++) CHECK(verdicts[v] > 0, "no mutant with verdict %d", v);
    }
    printf("%s total: bound %u pixels, pairs %u, hops %u, rounds %u, LDS at the bounds %u, %d mismatches\n", g_fail ? "FAILED" : "ok", kZdSmallDecMaxPx, kZsdMaxPairs, kZsdHops,
           kZsdRounds, zsd_lds_bytes(kZsdMaxPairs, kZdSmallDecMaxPx), g_fail);
    return g_fail ? 1 : 0;
}
