// small_trie_check.cpp -- cniic_amd/csrc/small_trie.hpp without a GPU (tests/test_small_trie_cpu.py compiles and runs this, plain and under
// -fsanitize=address,undefined).  A scalar parser made of the header's functions -- 1024 lanes of chunks, the phases in k_small_trieparse's
// order, arrays where the kernel has LDS -- beside a byte-by-byte stack parse: verdict, leaves, longest code, payload offset and every word
// of the table.  The streams are built here: w = h = 8, the trie, a payload of filler bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>
#include "small_trie.hpp"

using namespace cniic;
constexpr uint32_t S = 6;
static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; if (g_fail > 20) exit(1); } } while (0)

struct Parsed {
    uint32_t verdict = kStSkipped, L = 0, max_len = 0, pay = 0;
    std::vector<uint32_t> table;
    bool operator==(const Parsed &o) const { return verdict == o.verdict && L == o.L && max_len == o.max_len && pay == o.pay && table == o.table; }
};
static uint64_t g_entered[S + 1], g_left[S + 1];   // chunks on the true walk, by the offset they were entered and left at

// ---------------------------------------------------------------- the byte-by-byte stack parse (huff_parse_leaves with the kernel's verdicts:
// structure first -- the end, a bad tag, the window --, then depth and leaves, then the symbols)
static Parsed ref_parse(const std::vector<uint8_t> &s, bool count_offsets = false) {
    Parsed r;
    const uint8_t *trie = s.data() + 8;
    const uint64_t tb = s.size() - 8;
    const uint32_t window = st_window(tb, st_max_bytes<S>());
    struct Pend { uint64_t code; uint32_t depth; };
    std::vector<Pend> stack;
    struct Leaf { uint32_t at; uint64_t code; uint32_t depth; };
    std::vector<Leaf> leaves;
    std::vector<uint32_t> starts;
    uint64_t code = 0;
    uint32_t depth = 0, pos = 0;
    bool ended = false, bad_tag = false;
    for (;;) {
        if (pos >= window) break;
        const uint8_t tag = trie[pos];
        if (tag == 1) {
            starts.push_back(pos);
            pos++;
            stack.push_back({depth < 64 ? code | (1ull << (63 - depth)) : code, depth + 1});
            depth++;
        } else if (tag == 0) {
            if (pos + S + 1 > window) break;
            starts.push_back(pos);
            leaves.push_back({pos + 1, code, depth});
            pos += S + 1;
            if (stack.empty()) { ended = true; break; }
            code = stack.back().code; depth = stack.back().depth;
            stack.pop_back();
        } else { bad_tag = true; break; }
    }
    if (count_offsets) {   // (of the chunks that a record starts in or behind which the walk goes on)
        for (size_t i = 0; i < starts.size(); i++) {
            const uint32_t c = starts[i] / kStChunk;
            if (i == 0 || starts[i - 1] / kStChunk != c) {
                g_entered[starts[i] % kStChunk]++;
                if (i) g_left[starts[i] % kStChunk]++;
            }
        }
    }
    if (!ended) { r.verdict = st_verdict_open(bad_tag, window, tb); return r; }
    uint32_t longest = 0;
    for (const Leaf &l : leaves) longest = std::max(longest, l.depth);
    if (longest > kDeltaSmallMaxCodeLen || leaves.size() > kSmallTrieMaxLeaves) { r.verdict = kStNotOurs; return r; }
    const uint32_t L = (uint32_t)leaves.size();
    r.table.resize(2 * (size_t)L);
    bool ok = true;
    for (uint32_t i = 0; i < L; i++) {
        uint32_t key = 0;
        for (int k = 0; k < 3; k++) {
            const int v = (int16_t)(uint16_t)(trie[leaves[i].at + 2 * k] | (trie[leaves[i].at + 2 * k + 1] << 8));
            if (v < -255 || v > 255) ok = false;
            key = (key << 9) | ((uint32_t)(v + 255) & 511u);
        }
        r.table[i] = (uint32_t)(leaves[i].code >> 32);
        r.table[L + i] = dsd_keylen(key, leaves[i].depth);
    }
    if (!ok) { r.verdict = kStNotDecoder; r.table.clear(); return r; }
    // the two identities of the codes against the paths just walked
    uint64_t sum = 0;
    for (uint32_t i = 0; i < L; i++) {
        CHECK(r.table[i] == (uint32_t)sum, "code[%u] is not the prefix sum of the lengths", i);
        sum += leaves[i].depth ? 1ull << (32 - leaves[i].depth) : 1ull << 32;
    }
    CHECK(sum == 1ull << 32, "the steps of %u leaves do not add up to 2^32", L);
    r.verdict = kStParsed; r.L = L; r.max_len = longest; r.pay = 8 + pos;
    return r;
}

// ---------------------------------------------------------------- the kernel's order, lane by lane (pitch, room: the launch's)
static Parsed lane_parse(const std::vector<uint8_t> &s, uint32_t pitch, uint32_t room) {
    Parsed r;
    const uint8_t *trie = s.data() + 8;
    const uint64_t tb = s.size() - 8;
    const uint32_t window = st_window(tb, st_max_bytes<S>());
    if (!window) { r.verdict = kStNotDecoder; return r; }
    if (st_lanes_used(window) > pitch || st_leaves_room<S>(s.size()) > room) { r.verdict = kStNotOurs; return r; }
    std::vector<StLane> ln(kStLanes);
    // 1. masks and maps (bytes behind the stream read as 0xEE: the masks hide them)
    auto byte_at = [&](uint64_t i) -> uint32_t { return i < tb ? trie[i] : 0xEEu; };
    std::vector<uint32_t> map(kStLanes);
    for (uint32_t t = 0; t < kStLanes; t++) {
        StLane &l = ln[t];
        l.K = st_lane_chunks(window); l.at = t * l.K * kStChunk; l.entry = 0; l.nodes_before = l.leaves_before = 0;
        for (uint32_t k = 0; k < kStMaxK; k++) {
            l.br[k] = l.lf[k] = 0;
            const uint32_t at = l.at + k * kStChunk;
            if (k < l.K && at < window) {
                uint32_t w[8];
                for (uint32_t i = 0; i < 8; i++) { w[i] = 0; for (uint32_t b = 0; b < 4; b++) w[i] |= byte_at((uint64_t)at + 4 * i + b) << (8 * b); }
                st_masks<S>(w, at, window, l.br[k], l.lf[k]);
            }
        }
        map[t] = st_lane_map<S>(l);
    }
    uint32_t run_map = st_map_identity<S>();
    for (uint32_t t = 0; t < kStLanes; t++) { ln[t].entry = st_map_get<S>(run_map, 0); run_map = st_map_compose<S>(run_map, map[t]); }
    // 2. counts
    std::vector<uint8_t> last(kStLanes);
    bool bad_tag = false, give_up = false;
    uint32_t nodes_run = 0, leaves_run = 0;
    for (uint32_t t = 0; t < kStLanes; t++) {
        uint32_t nodes, leaves, lst;
        const uint32_t stop = st_lane_count<S>(ln[t], nodes, leaves, lst);
        last[t] = (uint8_t)lst;
        if (stop != kStNoStop && stop < window && trie[stop] != 0) bad_tag = true;
        if (nodes && t >= pitch) give_up = true;
        ln[t].nodes_before = nodes_run; ln[t].leaves_before = leaves_run;
        nodes_run += nodes; leaves_run += leaves;
    }
    // 3. P, the end, the table of last nodes
    std::vector<uint32_t> tab((size_t)(kStMaxP + 1) * pitch, 0u), runs(room, 0xdeadbeefu);
    uint32_t E = kStNone, deep = kStNone;
    for (uint32_t t = 0; t < pitch && t < kStLanes; t++) {
        uint32_t e, d;
        st_lane_open<S>(ln[t], tab.data(), pitch, t, &e, &d);
        E = std::min(E, e); deep = std::min(deep, d);
    }
    if (E == kStNone) { r.verdict = st_verdict_open(bad_tag, window, tb); return r; }
    const uint32_t L = E / 2 + 1;
    if (deep <= E || L > room || give_up) { r.verdict = kStNotOurs; return r; }
    for (uint32_t p = 0; p <= kStMaxP; p++) {
        uint32_t carry = 0;
        for (uint32_t t = 0; t < pitch; t++) { const uint32_t v = tab[p * pitch + t]; tab[p * pitch + t] = carry; carry = std::max(carry, v); }
    }
    // 4. runs, jumps
    uint32_t pay = 0;
    bool ok = true;
    for (uint32_t t = 0; t < pitch && t < kStLanes; t++) ok = st_lane_runs<S>(ln[t], t ? last[t - 1] != 0 : true, E, tab.data(), pitch, t, runs.data(), &pay) && ok;
    if (!ok) { r.verdict = kStNotOurs; return r; }
    for (uint32_t round = 0; round < kStJumpRounds; round++)
        for (uint32_t i = 0; i < L; i++) runs[i] = st_run_hop(runs[i], runs[st_run_jump(runs[i])]);
    for (uint32_t i = 0; i < L; i++) if (st_run_jump(runs[i]) != 0) ok = false;
    // 5. lengths, codes
    std::vector<uint32_t> first_code(kStLanes);
    uint32_t code = 0, longest = 0;
    for (uint32_t t = 0; t < kStLanes; t++) {
        uint32_t sum = 0, m = 0;
        if (ok) ok = st_lane_lens<S>(ln[t], E, runs.data(), &sum, &m) && ok;
        first_code[t] = code; code += sum; longest = std::max(longest, m);
    }
    if (!ok) { r.verdict = kStNotOurs; return r; }
    CHECK(code == 0, "the steps do not add up to 2^32");
    // 6. the table
    r.table.assign(2 * (size_t)L, 0xdeadbeefu);
    for (uint32_t t = 0; t < kStLanes; t++)
        ok = st_lane_table<S>(ln[t], E, runs.data(), first_code[t], L, r.table.data(), [&](uint32_t pos) { uint64_t v = 0; for (int b = 0; b < 6; b++) v |= (uint64_t)trie[pos + b] << (8 * b); return v; }) && ok;
    if (!ok) { r.verdict = kStNotDecoder; r.table.clear(); return r; }
    r.verdict = kStParsed; r.L = L; r.max_len = longest; r.pay = 8 + pay;
    return r;
}

// ---------------------------------------------------------------- streams
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }
static void put_leaf(std::vector<uint8_t> &t, uint32_t i, int r0 = 1000) {
    const int v[3] = {r0 != 1000 ? r0 : (int)(i % 511) - 255, (int)(i / 511 % 511) - 255, (int)(i * 7 % 511) - 255};
    t.push_back(0);
    for (int k = 0; k < 3; k++) { t.push_back((uint8_t)(v[k] & 255)); t.push_back((uint8_t)((v[k] >> 8) & 255)); }
}
// a trie of L leaves: split(L, depth) -> the leaves of the left subtree
static void build(std::vector<uint8_t> &t, uint32_t L, uint32_t depth, uint32_t &next, const std::function<uint32_t(uint32_t, uint32_t)> &split) {
    if (L == 1) { put_leaf(t, next++); return; }
    const uint32_t l = split(L, depth);
    t.push_back(1);
    build(t, l, depth + 1, next, split);
    build(t, L - l, depth + 1, next, split);
}
static std::vector<uint8_t> stream_of(const std::vector<uint8_t> &trie, uint32_t payload) {
    std::vector<uint8_t> s = {8, 0, 0, 0, 8, 0, 0, 0};
    s.insert(s.end(), trie.begin(), trie.end());
    for (uint32_t i = 0; i < payload; i++) s.push_back((uint8_t)(0x5a + 37 * i));
    return s;
}
static std::vector<uint8_t> trie_of(uint32_t L, const std::function<uint32_t(uint32_t, uint32_t)> &split) {
    std::vector<uint8_t> t;
    uint32_t next = 0;
    build(t, L, 0, next, split);
    return t;
}
static uint32_t balanced(uint32_t L, uint32_t) { return (L + 1) / 2; }
// any split that keeps both halves within what the depths left can hold (a longest code of 19)
static uint32_t bounded(uint32_t L, uint32_t depth) {
    const uint64_t half = 1ull << (kDeltaSmallMaxCodeLen - depth - 1);
    const uint32_t lo = L > half ? (uint32_t)(L - half) : 1, hi = (uint32_t)std::min<uint64_t>(L - 1, half);
    return lo + rnd(hi - lo + 1);
}
static uint32_t left_chain(uint32_t L, uint32_t) { return L - 1; }
static uint32_t right_chain(uint32_t, uint32_t) { return 1; }

static uint64_t g_compared = 0;
static Parsed compare(const std::vector<uint8_t> &s, const char *what, bool count_offsets = false) {
    const Parsed want = ref_parse(s, count_offsets);
    const uint32_t window = st_window(s.size() - 8, st_max_bytes<S>());
    const Parsed own = lane_parse(s, std::max(1u, st_lanes_used(window)), std::max(1u, st_leaves_room<S>(s.size())));
    CHECK(own == want, "%s (%zu bytes): verdict %u / %u, leaves %u / %u, longest %u / %u, payload at %u / %u, tables %s", what, s.size(), own.verdict, want.verdict, own.L,
          want.L, own.max_len, want.max_len, own.pay, want.pay, own.table == want.table ? "equal" : "differ");
    if (g_compared++ % 16 == 0) {   // in company: the launch sized by a longest stream
        const Parsed big = lane_parse(s, kStLanes, kSmallTrieMaxLeaves);
        CHECK(big == want, "%s (%zu bytes) in a launch at the bound: verdict %u / %u", what, s.size(), big.verdict, want.verdict);
    }
    return want;
}

int main() {
    // ---- the words themselves
    {
        for (int i = 0; i < 2000; i++) {
            uint32_t m[3];
            for (uint32_t &x : m) { x = 0; for (uint32_t o = 0; o <= S; o++) x |= rnd(S + 2) << (kStMapBits * o); }
            CHECK(st_map_compose<S>(st_map_compose<S>(m[0], m[1]), m[2]) == st_map_compose<S>(m[0], st_map_compose<S>(m[1], m[2])), "composition is not associative");
            CHECK(st_map_compose<S>(st_map_identity<S>(), m[0]) == m[0] && st_map_compose<S>(m[0], st_map_identity<S>()) == m[0], "the identity");
        }
        for (uint32_t x : {0u, 1u, 0x00010001u, 0x01000000u, 0x80000000u, 0xffffffffu, 0x00ff0100u, 0x7f008000u}) {
            uint32_t want = 0;
            for (int b = 0; b < 4; b++) want |= (uint32_t)(((x >> (8 * b)) & 255u) == 0) << b;
            CHECK(st_byte_is_zero(x) == want, "st_byte_is_zero(%08x)", x);
        }
        for (int sum : {-131071, -32767, -1, 0, 1, 32767, 131071})
            for (uint32_t j : {0u, 1u, 16383u}) CHECK(st_run_sum(st_run_word(j, sum)) == sum && st_run_jump(st_run_word(j, sum)) == j, "a run's word");
        uint32_t key;
        CHECK(st_symbol6(0x00ff00000001ull | (0xff01ull << 16), &key) && key == (((1u + 255u) << 18) | ((uint32_t)(-255 + 255) << 9) | (255u + 255u)), "st_symbol6");
        printf("ok words: maps associate, zero bytes, run words, symbols\n");
    }
    // ---- one and two leaves
    {
        Parsed p = compare(stream_of(trie_of(1, balanced), 0), "one leaf");
        CHECK(p.verdict == kStParsed && p.L == 1 && p.max_len == 0 && p.pay == 15, "one leaf");
        p = compare(stream_of(trie_of(2, balanced), 3), "two leaves");
        CHECK(p.verdict == kStParsed && p.L == 2 && p.max_len == 1 && p.pay == 8 + 15 && p.table[0] == 0 && p.table[1] == 0x80000000u, "two leaves");
        printf("ok small: one leaf (a 7-byte trie) and two\n");
    }
    // ---- chains
    {
        for (auto split : {left_chain, right_chain}) {
            Parsed p = compare(stream_of(trie_of(20, split), 9), "chain of 20");
            CHECK(p.verdict == kStParsed && p.L == 20 && p.max_len == 19, "a chain of 20 leaves has a longest code of 19");
            p = compare(stream_of(trie_of(21, split), 9), "chain of 21");
            CHECK(p.verdict == kStNotOurs, "a chain of 21 leaves is not ours");
            p = compare(stream_of(trie_of(200, split), 9), "chain of 200");
            CHECK(p.verdict == kStNotOurs, "a chain of 200 leaves is not ours");
        }
        printf("ok chains: left- and right-leaning, 20 leaves (depth 19) parsed, 21 and 200 not ours\n");
    }
    // ---- the bound
    {
        Parsed p = compare(stream_of(trie_of(kSmallTrieMaxLeaves, balanced), 5), "16384 leaves");
        CHECK(p.verdict == kStParsed && p.L == kSmallTrieMaxLeaves && p.max_len == 14 && p.pay == 8 + st_max_bytes<S>(), "16 384 leaves of 14 bits");
        p = compare(stream_of(trie_of(kSmallTrieMaxLeaves + 1, balanced), 5), "16385 leaves");
        CHECK(p.verdict == kStNotOurs, "16 385 leaves are not ours");
        p = compare(stream_of(std::vector<uint8_t>(st_max_bytes<S>() + 100, 1), 0), "branches only");
        CHECK(p.verdict == kStNotOurs, "a window of branches is not ours");
        p = compare(stream_of(std::vector<uint8_t>(5000, 1), 0), "branches to the end");
        CHECK(p.verdict == kStNotDecoder, "branches to the stream's end are no decoder");
        printf("ok bound: %u leaves parsed, %u not ours; constants: leaves %u, lanes %u, chunk %u, window %u, rows %u\n", kSmallTrieMaxLeaves, kSmallTrieMaxLeaves + 1,
               kSmallTrieMaxLeaves, kStLanes, kStChunk, st_max_bytes<S>(), kStMaxP + 1);
    }
    // ---- random tries
    {
        uint32_t parsed = 0, most = 0;
        for (int i = 0; i < 60; i++) {
            const uint32_t L = i < 4 ? kSmallTrieMaxLeaves - (uint32_t)i : 1 + rnd(i % 3 ? kSmallTrieMaxLeaves : 600);
            Parsed p = compare(stream_of(trie_of(L, bounded), rnd(40)), "random", true);
            CHECK(p.verdict == kStParsed && p.L == L, "a random trie of %u leaves", L);
            parsed += p.verdict == kStParsed; most = std::max(most, L);
        }
        for (int i = 0; i < 12; i++) {   // any shape: most of them too deep
            const uint32_t L = 2 + rnd(3000);
            (void)compare(stream_of(trie_of(L, [](uint32_t l, uint32_t) { return 1 + rnd(l - 1); }), rnd(40)), "random, any depth", true);
        }
        printf("ok random: %u tries parsed, up to %u leaves\n", parsed, most);
    }
    // ---- every entry and every exit
    {
        memset(g_entered, 0, sizeof g_entered);
        memset(g_left, 0, sizeof g_left);
        for (uint32_t lead = 0; lead < 40; lead++) {   // `lead` branches in front shift every later record by one byte
            const std::vector<uint8_t> t = trie_of(64 + lead, [&](uint32_t L, uint32_t depth) { return depth < lead % 12 ? L - 1 : (L + 1) / 2; });
            (void)compare(stream_of(t, 4), "offsets", true);
        }
        for (uint32_t o = 0; o <= S; o++) CHECK(g_entered[o] && g_left[o], "no chunk entered or left at offset %u", o);
        printf("ok offsets: chunks entered at 0..%u: %llu %llu %llu %llu %llu %llu %llu, left at each as well\n", S, (unsigned long long)g_entered[0], (unsigned long long)g_entered[1],
               (unsigned long long)g_entered[2], (unsigned long long)g_entered[3], (unsigned long long)g_entered[4], (unsigned long long)g_entered[5], (unsigned long long)g_entered[6]);
    }
    // ---- lengths around the chunks (a trie of L leaves has 8 L - 1 bytes: k C - 1 with L = 4 k)
    {
        const uint32_t kmax = st_max_bytes<S>() / kStChunk;
        for (uint32_t k : {1u, 2u, kmax}) {
            const std::vector<uint8_t> t = trie_of(4 * k, bounded), longer = trie_of(4 * k + 3, bounded);
            CHECK(t.size() == k * kStChunk - 1, "a trie of %u leaves", 4 * k);
            for (uint32_t more = 0; more < 3; more++) {
                Parsed p = compare(stream_of(t, more), "whole, k C - 1 + payload");      // windows of k C - 1, k C, k C + 1 bytes
                CHECK(p.verdict == kStParsed && p.pay == 8 + t.size(), "k = %u, %u more", k, more);
                std::vector<uint8_t> cut = stream_of(longer, 0);
                cut.resize(8 + k * kStChunk - 1 + more);
                p = compare(cut, "cut at k C - 1 + more");
                CHECK(p.verdict == kStNotDecoder, "a trie cut at %u bytes is no decoder", k * kStChunk - 1 + more);
            }
        }
        printf("ok lengths: windows of k C - 1, k C, k C + 1 bytes for k = 1, 2, %u, whole and cut\n", kmax);
    }
    // ---- cuts and edits of a 7-leaf stream
    {
        const std::vector<uint8_t> t = trie_of(7, bounded);
        CHECK(t.size() == 55, "seven leaves");
        const std::vector<uint8_t> s = stream_of(t, 6);
        uint32_t by_verdict[4] = {0, 0, 0, 0};
        for (size_t n = 8; n <= s.size(); n++) {
            Parsed p = compare(std::vector<uint8_t>(s.begin(), s.begin() + n), "cut");
            CHECK((p.verdict == kStParsed) == (n >= 8 + 55) && (p.verdict == kStParsed || p.verdict == kStNotDecoder), "cut at %zu", n);
        }
        for (size_t at = 0; at < 55; at++)
            for (uint32_t d = 1; d < 256; d++) {
                std::vector<uint8_t> e = s;
                e[8 + at] = (uint8_t)(e[8 + at] + d);
                by_verdict[compare(e, "edit").verdict]++;
            }
        CHECK(by_verdict[kStParsed] && by_verdict[kStNotDecoder], "edits parse and fail");
        printf("ok mutations: every cut; %u edits: %u parsed, %u no decoder, %u not ours\n", 55 * 255, by_verdict[kStParsed], by_verdict[kStNotDecoder], by_verdict[kStNotOurs]);
    }
    // ---- symbols at the range's ends, a trie that ends with the stream
    {
        for (int v : {255, -255, 256, -256, 32767, -32768}) {
            std::vector<uint8_t> t = {1};
            put_leaf(t, 0, v);
            put_leaf(t, 1);
            Parsed p = compare(stream_of(t, 2), "symbol");
            CHECK((p.verdict == kStParsed) == (v >= -255 && v <= 255) && (p.verdict == kStParsed || p.verdict == kStNotDecoder), "a symbol of %d", v);
        }
        Parsed p = compare(stream_of(trie_of(300, bounded), 0), "no payload");
        CHECK(p.verdict == kStParsed && p.pay == 8 + 8 * 300 - 1, "a trie that ends exactly at the stream's end");
        printf("ok symbols: +-255 parsed, +-256 no decoder; a trie that ends with its stream\n");
    }
    printf("%s: %llu streams compared, the code identities asserted on every parsed one\n", g_fail ? "FAIL" : "ok total", (unsigned long long)g_compared);
    return g_fail ? 1 : 0;
}
