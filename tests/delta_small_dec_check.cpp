// delta_small_dec_check.cpp -- cniic_amd/csrc/delta_small_dec.hpp without a GPU (tests/test_delta_small_decode_cpu.py builds this file
// plain and under -fsanitize=address,undefined and runs it as a program).  A scalar decoder is assembled from the header's functions and
// walks a payload as the workgroup of k_delta_small_dec does: 1024 lanes, one subsequence each, rounds in which every lane whose
// predecessor ended elsewhere decodes again, a vote, the prefix sum of the counts, one more pass that writes.  Beside it runs a plain
// restatement: the trie walked bit by bit, MSB first, a symbol there when all its bits are.  The streams are built here with a binary
// heap ordered by (count, leaf before branch, key): random lists, one and two leaves, 16 384 equal leaves, the strict chain that meets
// the 19-bit bound, payloads of exactly 1, 31, 32, 33 and 19 * 16 384 bits, every truncation point of a short stream, and a stream in
// which every subsequence starts inside a code and nothing synchronises by itself, which takes the most rounds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <queue>
#include <random>
#include <vector>

#include "delta_small_dec.hpp"

using namespace cniic;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

struct Node { int l, r; uint32_t key; };   // l < 0: a leaf
struct Tree {
    std::vector<Node> nodes;
    int root = -1;
    std::vector<uint32_t> code, keylen;      // the leaves in pre-order: left-aligned codes, key | length << 27
    std::vector<uint32_t> enc_code, enc_len; // per symbol index (the order of `counts`)
    uint32_t max_len = 0;
};

// symbol i has key keys[i] and count counts[i] (> 0)
static Tree build(const std::vector<uint32_t> &keys, const std::vector<uint64_t> &counts) {
    Tree t;
    const size_t U = keys.size();
    struct Item { uint64_t count; int branch; uint32_t key; int node; };
    auto later = [](const Item &a, const Item &b) {
        if (a.count != b.count) return a.count > b.count;
        if (a.branch != b.branch) return a.branch > b.branch;
        return a.key > b.key;
    };
    std::priority_queue<Item, std::vector<Item>, decltype(later)> heap(later);
    for (size_t i = 0; i < U; i++) { t.nodes.push_back({-1, -1, keys[i]}); heap.push({counts[i], 0, keys[i], (int)i}); }
    uint32_t made = 0;
    while (heap.size() > 1) {
        const Item a = heap.top(); heap.pop();
        const Item b = heap.top(); heap.pop();
        t.nodes.push_back({a.node, b.node, 0});
        heap.push({a.count + b.count, 1, made++, (int)t.nodes.size() - 1});
    }
    t.root = heap.top().node;
    t.enc_code.assign(U, 0); t.enc_len.assign(U, 0);
    std::function<void(int, uint32_t, uint32_t)> walk = [&](int nd, uint32_t code, uint32_t depth) {
        if (t.nodes[nd].l < 0) {
            t.code.push_back(depth ? code << (32 - depth) : 0u);
            t.keylen.push_back(dsd_keylen(t.nodes[nd].key, depth));
            t.enc_code[nd] = code; t.enc_len[nd] = depth;
            t.max_len = std::max(t.max_len, depth);
            return;
        }
        walk(t.nodes[nd].l, code << 1, depth + 1);
        walk(t.nodes[nd].r, (code << 1) | 1u, depth + 1);
    };
    walk(t.root, 0, 0);
    return t;
}

static std::vector<uint8_t> pack(const Tree &t, const std::vector<uint32_t> &syms, uint64_t *bits_out = nullptr) {
    std::vector<uint8_t> out;
    uint64_t bits = 0;
    for (uint32_t s : syms)
        for (uint32_t k = t.enc_len[s]; k-- > 0;) {
            if (!(bits & 7)) out.push_back(0);
            if ((t.enc_code[s] >> k) & 1u) out.back() |= (uint8_t)(0x80u >> (bits & 7));
            bits++;
        }
    if (bits_out) *bits_out = bits;
    return out;
}

// the plain restatement: n symbols by the bit-by-bit walk; false where the bits run out before the n-th
static bool plain_decode(const Tree &t, const std::vector<uint8_t> &pay, uint32_t n, std::vector<uint32_t> &keys) {
    keys.clear();
    const uint64_t nbits = (uint64_t)pay.size() * 8;
    uint64_t bp = 0;
    for (uint32_t i = 0; i < n; i++) {
        int nd = t.root;
        while (t.nodes[nd].l >= 0) {
            if (bp >= nbits) return false;
            const int bit = (pay[bp >> 3] >> (7 - (bp & 7))) & 1;
            bp++;
            nd = bit ? t.nodes[nd].r : t.nodes[nd].l;
        }
        keys.push_back(t.nodes[nd].key);
    }
    return true;
}

// the header's decoder in the kernel's order.  Returns the status; *rounds = votes taken
// cap_px: the pixels the launch has room for (0: the frame's own, rounded up to 256 as the launcher does), which sizes the larger table
static uint32_t lanes_decode(const Tree &t, const std::vector<uint8_t> &pay, uint32_t n, uint32_t max_rounds, std::vector<uint32_t> &keys, uint32_t *rounds,
                             uint32_t cap_px = 0) {
    const uint32_t L = (uint32_t)t.code.size();
    keys.assign(n, 0xffffffffu);
    *rounds = 0;
    if (L == 1) { std::fill(keys.begin(), keys.end(), dsd_keylen_key(t.keylen[0])); return kDsdOk; }
    const uint32_t nst = dsd_stage_bytes(n, pay.size()), b = nst * 8, nw = (nst + 3) / 4;
    std::vector<uint32_t> words(nw + 2, 0u);
    for (uint32_t i = 0; i < nw; i++) {
        uint8_t q[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < 4 && 4 * i + k < nst; k++) q[k] = pay[4 * i + k];
        words[i] = dsd_be_word(q);
    }
    std::vector<uint32_t> t1((1u << kDsdT1Bits) + 1), t1k(1u << kDsdT1Bits);
    for (uint32_t p = 0; p <= (1u << kDsdT1Bits); p++) dsd_t1_entry(t.code.data(), t.keylen.data(), L, p, t1.data(), t1k.data());
    if (!cap_px) cap_px = (n + 255) & ~255u;
    uint32_t big_bits = 0;
    while ((2u << big_bits) <= cap_px) big_bits++;   // 2^big_bits <= cap_px
    std::vector<uint32_t> big;                       // the settle rounds' table, where the symbols go afterwards
    if (big_bits > kDsdT1Bits && t.max_len > kDsdT1Bits) {
        big.resize(cap_px);
        for (uint32_t p = 0; p < (1u << big_bits); p++) big[p] = dsd_big_entry(t.code.data(), t.keylen.data(), t1.data(), t1k.data(), big_bits, p);
    }
    const uint32_t sub = dsd_sub_bits(b);
    std::vector<uint32_t> start(kDsdLanes), end(kDsdLanes), count(kDsdLanes);
    auto pass = [&](uint32_t lane, uint32_t *out, uint32_t first) {
        const uint32_t *tab = out || big.empty() ? nullptr : big.data();
        count[lane] = dsd_pass(words.data(), b, t.code.data(), t.keylen.data(), t1.data(), t1k.data(), tab, big_bits, start[lane], dsd_bound(lane + 1, sub, b),
                               &end[lane], out, first, n);
    };
    for (uint32_t lane = 0; lane < kDsdLanes; lane++) { start[lane] = dsd_bound(lane, sub, b); pass(lane, nullptr, 0); }
    bool settled = false;
    for (uint32_t round = 1;; round++) {
        *rounds = round;
        const std::vector<uint32_t> seen = end;   // (every lane reads its predecessor's end before any lane writes)
        bool any = false;
        for (uint32_t lane = 1; lane < kDsdLanes; lane++) any |= seen[lane - 1] != start[lane];
        if (!any) { settled = true; break; }
        if (round >= max_rounds) break;
        for (uint32_t lane = 1; lane < kDsdLanes; lane++)
            if (seen[lane - 1] != start[lane]) { start[lane] = seen[lane - 1]; pass(lane, nullptr, 0); }
    }
    if (!settled) return kDsdUnsettled;
    uint64_t total = 0;
    std::vector<uint32_t> first(kDsdLanes);
    for (uint32_t lane = 0; lane < kDsdLanes; lane++) { first[lane] = (uint32_t)total; total += count[lane]; }
    if (total < n) return kDsdShort;
    for (uint32_t lane = 0; lane < kDsdLanes; lane++)
        if (first[lane] < n) pass(lane, keys.data(), first[lane]);
    return kDsdOk;
}

// both decoders on one payload; returns the rounds the lanes took
static uint32_t compare(const char *what, const Tree &t, const std::vector<uint8_t> &pay, uint32_t n, int want_ok = -1) {
    std::vector<uint32_t> a, b;
    uint32_t rounds = 0;
    const bool ok = plain_decode(t, pay, n, a);
    const uint32_t st = lanes_decode(t, pay, n, kDsdMaxRounds, b, &rounds);
    CHECK(st == (ok ? kDsdOk : kDsdShort), "%s: status %u, the plain walk %s (n %u, %zu bytes)", what, st, ok ? "decodes" : "fails", n, pay.size());
    if (ok && st == kDsdOk) CHECK(a == b, "%s: symbols differ (n %u, %zu bytes)", what, n, pay.size());
    std::vector<uint32_t> c;   // in company with a frame at the bound: the larger table at its largest
    uint32_t rounds_c = 0;
    const uint32_t st_c = lanes_decode(t, pay, n, kDsdMaxRounds, c, &rounds_c, kDeltaSmallDecMaxPx);
    CHECK(st_c == st && rounds_c == rounds && (st != kDsdOk || c == b), "%s: another answer with the launch's room at the bound", what);
    if (want_ok >= 0) CHECK((int)ok == want_ok, "%s: the plain walk %s", what, ok ? "decodes" : "fails");
    return rounds;
}

static uint32_t key_of(std::mt19937 &rng) { return ((rng() % 511) << 18) | ((rng() % 511) << 9) | (rng() % 511); }

static std::vector<uint32_t> distinct_keys(size_t U, std::mt19937 &rng) {
    std::vector<uint32_t> k;
    while (k.size() < U) {
        while (k.size() < U) k.push_back(key_of(rng));
        std::sort(k.begin(), k.end());
        k.erase(std::unique(k.begin(), k.end()), k.end());
    }
    std::shuffle(k.begin(), k.end(), rng);
    return k;
}

static std::vector<uint32_t> list_of(const std::vector<uint64_t> &counts, std::mt19937 &rng) {
    std::vector<uint32_t> syms;
    for (size_t i = 0; i < counts.size(); i++) syms.insert(syms.end(), counts[i], (uint32_t)i);
    std::shuffle(syms.begin(), syms.end(), rng);
    return syms;
}

int main() {
    std::mt19937 rng(20240611);
    {   // random lists: few to many symbols, flat to steep counts
        uint32_t most_rounds = 0, longest = 0;
        for (int it = 0; it < 60; it++) {
            const size_t U = 2 + rng() % (it % 3 == 0 ? 2000 : 40);
            std::vector<uint64_t> counts(U);
            uint64_t n = 0;
            for (auto &c : counts) { c = 1 + (it % 2 ? rng() % 8 : (rng() % 100 < 80 ? rng() % 3 : rng() % 400)); n += c; }
            while (n > kDeltaSmallDecMaxPx) { auto &c = counts[rng() % U]; if (c > 1) { n -= c - 1; c = 1; } }
            const Tree t = build(distinct_keys(U, rng), counts);
            CHECK(t.max_len <= kDeltaSmallMaxCodeLen, "random: a code of %u bits", t.max_len);
            longest = std::max(longest, t.max_len);
            const std::vector<uint32_t> syms = list_of(counts, rng);
            std::vector<uint8_t> pay = pack(t, syms);
            most_rounds = std::max(most_rounds, compare("random", t, pay, (uint32_t)n, 1));
            pay.push_back((uint8_t)rng());   // a byte behind the last symbol is ignored
            compare("random + 1 byte", t, pay, (uint32_t)n, 1);
            pay.resize(pay.size() - 2);      // and one byte short: the last symbols are missing (or, by chance of the padding, not)
            compare("random - 1 byte", t, pay, (uint32_t)n);
        }
        printf("ok random: 60 lists, longest code %u, most rounds %u\n", longest, most_rounds);
    }
    {   // one leaf: nothing to decode, whatever the payload
        const Tree t = build({0x3fdfeffu}, {777});
        std::vector<uint32_t> keys;
        uint32_t rounds;
        CHECK(lanes_decode(t, {}, 777, kDsdMaxRounds, keys, &rounds) == kDsdOk && keys == std::vector<uint32_t>(777, 0x3fdfeffu), "one leaf");
        printf("ok one: 777 symbols of a zero-length code\n");
    }
    Tree two = build({5u, 9u}, {3, 4});
    {
        CHECK(two.max_len == 1, "two leaves: length %u", two.max_len);
        std::vector<uint32_t> syms;
        for (int i = 0; i < 4097; i++) syms.push_back(rng() & 1);
        compare("two", two, pack(two, syms), 4097, 1);
        printf("ok two: 4097 one-bit codes\n");
    }
    {   // 16 384 equal leaves: every code has 14 bits
        std::vector<uint32_t> keys(16384);
        for (uint32_t i = 0; i < 16384; i++) keys[i] = (i % 128 + 255) << 18 | (i / 128 + 255) << 9 | 255;
        const Tree t = build(keys, std::vector<uint64_t>(16384, 1));
        CHECK(t.max_len == 14 && *std::min_element(t.enc_len.begin(), t.enc_len.end()) == 14, "equal leaves: longest %u", t.max_len);
        std::vector<uint32_t> syms(16384);
        for (uint32_t i = 0; i < 16384; i++) syms[i] = i;
        std::shuffle(syms.begin(), syms.end(), rng);
        const uint32_t rounds = compare("equal16384", t, pack(t, syms), 16384, 1);
        printf("ok equal16384: every code 14 bits, %u rounds\n", rounds);
    }
    std::vector<uint64_t> chain = {1, 1, 1};
    {   // the strict chain 1, 1, 1, 3, 4, 7, 11, ...: the 19-bit bound is met (delta_small.hpp)
        std::vector<uint64_t> br = {2, 3};
        while (chain.size() < 20) { chain.push_back(br[br.size() - 2] + 1); br.push_back(br[br.size() - 1] + br[br.size() - 2] + 1); }
        uint64_t n = 0;
        for (auto c : chain) n += c;
        CHECK(n == 15126 && chain.back() == 5778, "chain: %llu symbols", (unsigned long long)n);
        const Tree t = build(distinct_keys(20, rng), chain);
        CHECK(t.max_len == kDeltaSmallMaxCodeLen, "chain: longest code %u", t.max_len);
        const uint32_t rounds = compare("chain19", t, pack(t, list_of(chain, rng)), (uint32_t)n, 1);
        printf("ok chain19: longest code met %u, bound %u, %u rounds\n", t.max_len, kDeltaSmallMaxCodeLen, rounds);
        // the longest payload there is: 16 384 symbols of 19 bits
        const uint32_t deep = (uint32_t)(std::find(t.enc_len.begin(), t.enc_len.end(), 19u) - t.enc_len.begin());
        uint64_t bits = 0;
        const std::vector<uint8_t> pay = pack(t, std::vector<uint32_t>(16384, deep), &bits);
        CHECK(bits == 19ull * 16384 && pay.size() == dsd_stage_bytes(16384, 1u << 30) && pay.size() == 38912, "the longest payload: %llu bits", (unsigned long long)bits);
        compare("19 x 16384 bits", t, pay, 16384, 1);
        for (uint32_t nb : {1u, 31u, 32u, 33u}) {   // payloads of exactly nb bits: one-bit codes
            std::vector<uint32_t> syms;
            for (uint32_t i = 0; i < nb; i++) syms.push_back(rng() & 1);
            compare("n bits", two, pack(two, syms), nb, 1);
            compare("n bits, one symbol more", two, pack(two, syms), (nb + 7) / 8 * 8 + 1, 0);
        }
        printf("ok bit_lengths: 1, 31, 32, 33 and %llu bits\n", (unsigned long long)bits);
    }
    {   // every truncation point of a short stream
        const size_t U = 37;
        std::vector<uint64_t> counts(U);
        uint64_t n = 0;
        for (auto &c : counts) { c = 1 + rng() % 30; n += c; }
        const Tree t = build(distinct_keys(U, rng), counts);
        const std::vector<uint8_t> pay = pack(t, list_of(counts, rng));
        uint32_t fails = 0;
        for (size_t cut = 0; cut <= pay.size(); cut++) {
            std::vector<uint8_t> p(pay.begin(), pay.begin() + cut);
            std::vector<uint32_t> a;
            fails += !plain_decode(t, p, (uint32_t)n, a);
            compare("truncation", t, p, (uint32_t)n);
        }
        CHECK(fails >= pay.size() - 1 && fails <= pay.size(), "truncation: %u of %zu cuts fail", fails, pay.size() + 1);
        printf("ok truncation: %zu cuts of a stream of %llu symbols, %u fail\n", pay.size() + 1, (unsigned long long)n, fails);
    }
    {   // a one-bit code first, then only the all-ones code of 8 bits: codes start at bits 1 + 8 k, subsequences at multiples of 32, so every
        // lane but the first starts inside a code, and a run of ones reads the same from any bit: nothing synchronises but through the
        // predecessor, one lane per round
        std::vector<uint32_t> keys = {0u};
        std::vector<uint64_t> counts = {128};
        for (uint32_t i = 0; i < 128; i++) { keys.push_back(1000 + i); counts.push_back(1); }
        const Tree t = build(keys, counts);
        CHECK(t.enc_len[0] == 1 && t.max_len == 8, "resync: lengths %u, %u", t.enc_len[0], t.max_len);
        const uint32_t ones = (uint32_t)(std::find(t.enc_code.begin() + 1, t.enc_code.end(), 0xffu) - t.enc_code.begin());
        std::vector<uint32_t> syms(4001, ones);
        syms[0] = t.enc_code[0] == 0 ? 0 : ones;
        CHECK(t.enc_code[0] == 0 && ones < keys.size(), "resync: the tree's shape");
        const std::vector<uint8_t> pay = pack(t, syms);
        const uint32_t b = (uint32_t)pay.size() * 8, sub = dsd_sub_bits(b), active = (b + sub - 1) / sub;
        CHECK(sub == kDsdMinSubBits && active == 1001, "resync: %u bits, subsequences of %u", b, sub);
        const uint32_t rounds = compare("resync", t, pay, 4001, 1);
        CHECK(rounds == active, "resync: %u rounds, %u lanes with bits", rounds, active);
        std::vector<uint32_t> k2;
        uint32_t r2 = 0;
        CHECK(lanes_decode(t, pay, 4001, active - 1, k2, &r2) == kDsdUnsettled && r2 == active - 1, "resync: a cap of %u rounds", active - 1);
        CHECK(lanes_decode(t, pay, 4001, 1, k2, &r2) == kDsdUnsettled && r2 == 1, "resync: a cap of one round");
        printf("ok resync: %u lanes with bits, settled after %u rounds, handed back under a lower cap\n", active, rounds);
    }
    {   // FromDiff's pieces
        for (int32_t r : {-255, -1, 0, 1, 255})
            for (int32_t g : {-255, 0, 7, 255})
                for (int32_t bl : {-255, -3, 0, 255}) {
                    const uint32_t key = (uint32_t)(r + 255) << 18 | (uint32_t)(g + 255) << 9 | (uint32_t)(bl + 255);
                    CHECK(dsd_diff(key, 0) == r && dsd_diff(key, 1) == g && dsd_diff(key, 2) == bl, "diffs of %d %d %d", r, g, bl);
                    CHECK(dsd_keylen_key(dsd_keylen(key, 19)) == key && dsd_keylen_len(dsd_keylen(key, 19)) == 19, "key | length");
                }
        CHECK(dsd_in_range(0) && dsd_in_range(255) && !dsd_in_range(-1) && !dsd_in_range(256) && !dsd_in_range(-255 * 16384) && !dsd_in_range(255 * 16384), "range");
        printf("ok fromdiff: fields, key | length, range\n");
    }
    printf("constants: max px %u, lanes %u, rounds %u, first level %u bits, longest code %u\n", kDeltaSmallDecMaxPx, kDsdLanes, kDsdMaxRounds, kDsdT1Bits,
           kDeltaSmallMaxCodeLen);
    if (g_fail) { printf("FAIL: %d checks\n", g_fail); return 1; }
    printf("ok total\n");
    return 0;
}
