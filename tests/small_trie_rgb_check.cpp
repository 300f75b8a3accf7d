// small_trie_rgb_check.cpp -- cniic_amd/csrc/small_trie.hpp for S = 11 (the Rgb<u8> leaf of `hufman` and `cluster-colors` streams) without
// a GPU; tests/test_small_trie_rgb_cpu.py compiles and runs this, plain and under -fsanitize=address,undefined.  It is the twin of
// small_trie_check.cpp (S = 6): a scalar parser made of the header's functions -- 1024 lanes of up to 7 chunks, 64-bit maps, the phases in
// k_small_trieparse_rgb's order, arrays where the kernel has LDS -- beside a byte-by-byte stack parse with get_symbol's RGB rule (the length
// word must be 3): verdict, leaves, longest code, payload offset and every word of the table.  The streams are built here: w = h = 8, the
// trie, a payload of filler bytes.
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
constexpr uint32_t S = 11;
typedef StMap<S>::word Map;
static_assert(sizeof(Map) == 8 && StMap<S>::bits == 4, "12 fields of 4 bits in a 64-bit word");
static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; if (g_fail > 20) exit(1); } } while (0)

struct Parsed {
    uint32_t verdict = kStSkipped, L = 0, max_len = 0, pay = 0;
    std::vector<uint32_t> table;
    bool operator==(const Parsed &o) const { return verdict == o.verdict && L == o.L && max_len == o.max_len && pay == o.pay && table == o.table; }
};
static uint64_t g_entered[S + 1], g_left[S + 1];   // chunks on the true walk, by the offset they were entered and left at
static uint32_t g_most_chunks = 0;                 // the most chunks a lane had
static uint64_t g_last_words_kept = 0, g_last_words_dropped = 0;   // nodes with P <= kStMaxP on a true walk: up to kStLastNodeMax, above it

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
        const uint8_t *p = trie + leaves[i].at;
        uint64_t len = 0;
        for (int b = 0; b < 8; b++) len |= (uint64_t)p[b] << (8 * b);
        if (len != 3) ok = false;   // get_symbol, CNIIC_SYM_RGB
        r.table[i] = (uint32_t)(leaves[i].code >> 32);
        r.table[L + i] = dsd_keylen(((uint32_t)p[8] << 16) | ((uint32_t)p[9] << 8) | p[10], leaves[i].depth);
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
    std::vector<StLaneRgb> ln(kStLanes);
    // 1. masks and maps (bytes behind the stream read as 0xEE: the masks hide them)
    auto byte_at = [&](uint64_t i) -> uint32_t { return i < tb ? trie[i] : 0xEEu; };
    std::vector<Map> map(kStLanes);
    CHECK(st_lane_chunks(window) <= kStMaxKRgb && (uint64_t)st_lane_chunks(window) * kStLanes * kStChunk >= window, "1024 lanes of %u chunks hold a window of %u bytes", st_lane_chunks(window), window);
    g_most_chunks = std::max(g_most_chunks, st_lane_chunks(window));
    for (uint32_t t = 0; t < kStLanes; t++) {
        StLaneRgb &l = ln[t];
        l.K = st_lane_chunks(window); l.at = t * l.K * kStChunk; l.entry = 0; l.nodes_before = l.leaves_before = 0;
        for (uint32_t k = 0; k < kStMaxKRgb; k++) {
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
    Map run_map = st_map_identity<S>();
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
    for (uint32_t w : tab) CHECK(w == 0 || (st_last_node1(w) - 1 <= kStLastNodeMax && st_last_run(w) < st_last_node1(w)), "a last-node word of node %u, run %u", st_last_node1(w) - 1, st_last_run(w));
    if (E == kStNone) { r.verdict = st_verdict_open(bad_tag, window, tb); return r; }
    const uint32_t L = E / 2 + 1;
    if (deep <= E || L > room || give_up) { r.verdict = kStNotOurs; return r; }
    CHECK(E <= kStLastNodeMax, "a frame past phase 3 ends at node %u", E);
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
        ok = st_lane_table<S>(ln[t], E, runs.data(), first_code[t], L, r.table.data(), [&](uint32_t pos) {
            StRgbLeaf l = {0, 0};
            for (int b = 0; b < 8; b++) l.len |= (uint64_t)trie[pos + b] << (8 * b);
            for (int b = 0; b < 3; b++) l.rgb |= (uint32_t)trie[pos + 8 + b] << (8 * b);
            return l;
        }) && ok;
    if (!ok) { r.verdict = kStNotDecoder; r.table.clear(); return r; }
    r.verdict = kStParsed; r.L = L; r.max_len = longest; r.pay = 8 + pay;
    return r;
}

// the true walk's nodes that have a P the table of last nodes keeps a row for, by their index: what st_lane_open writes a word for and what not
static void count_last_words(const std::vector<uint8_t> &s) {
    const uint8_t *trie = s.data() + 8;
    const uint32_t window = st_window(s.size() - 8, st_max_bytes<S>());
    int64_t P = 0;
    for (uint32_t pos = 0, node = 0; pos < window; node++) {
        const uint8_t tag = trie[pos];
        if (tag > 1 || (tag == 0 && pos + S + 1 > window)) break;
        if (P >= 0 && P <= (int64_t)kStMaxP) (node <= kStLastNodeMax ? g_last_words_kept : g_last_words_dropped)++;
        if (tag == 1) { P++; pos++; } else { P--; pos += S + 1; }
    }
}

// ---------------------------------------------------------------- streams
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }
static void put_leaf(std::vector<uint8_t> &t, uint32_t i, uint64_t len = 3) {
    t.push_back(0);
    for (int b = 0; b < 8; b++) t.push_back((uint8_t)(len >> (8 * b)));
    t.push_back((uint8_t)i); t.push_back((uint8_t)(i >> 8)); t.push_back((uint8_t)(i * 7 + 1));
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
            Map m[3];
            for (Map &x : m) { x = 0; for (uint32_t o = 0; o <= S; o++) x |= (Map)rnd(S + 2) << (StMap<S>::bits * o); }
            CHECK(st_map_compose<S>(st_map_compose<S>(m[0], m[1]), m[2]) == st_map_compose<S>(m[0], st_map_compose<S>(m[1], m[2])), "composition is not associative");
            CHECK(st_map_compose<S>(st_map_identity<S>(), m[0]) == m[0] && st_map_compose<S>(m[0], st_map_identity<S>()) == m[0], "the identity");
            for (uint32_t o = 0; o <= S + 3; o++) CHECK(st_map_get<S>(m[0], o) == (o > S ? S + 1 : (uint32_t)((m[0] >> (4 * o)) & 15)), "st_map_get at %u", o);
        }
        CHECK(st_map_identity<S>() == 0xba9876543210ull, "the identity is 0 .. 11 in nibbles");
        uint32_t key;
        CHECK(st_symbol11(3, 0x00c0b0a0u, &key) && key == 0xa0b0c0u, "st_symbol11: r << 16 | g << 8 | b");
        CHECK(!st_symbol11(2, 0, &key) && !st_symbol11(4, 0, &key) && !st_symbol11(3ull + (1ull << 32), 0, &key), "a length word other than 3");
        CHECK(st_last_node1(st_last_word(kStLastNodeMax, kStLastNodeMax)) == kStLastNodeMax + 1 && st_last_run(st_last_word(kStLastNodeMax, kStLastNodeMax)) == kStLastNodeMax, "the largest last-node word");
        for (int sum : {-131071, -32767, -1, 0, 1, 32767, 131071})
            for (uint32_t j : {0u, 1u, 16383u}) CHECK(st_run_sum(st_run_word(j, sum)) == sum && st_run_jump(st_run_word(j, sum)) == j, "a run's word");
        CHECK(st_max_bytes<S>() == 212991 && st_chunks(st_max_bytes<S>()) == 6656 && st_lane_chunks(st_max_bytes<S>()) == 7, "the window at the bound");
        CHECK(st_leaves_room<S>(8 + 12) == 1 && st_leaves_room<S>(8 + 11) == 0 && st_leaves_room<S>(8 + 24) == 1 && st_leaves_room<S>(8 + 25) == 2 && st_leaves_room<S>(1u << 30) == kSmallTrieMaxLeaves, "st_leaves_room");
        printf("ok words: 64-bit maps associate, the identity, symbols, last-node and run words, the window\n");
    }
    // ---- one and two leaves
    {
        Parsed p = compare(stream_of(trie_of(1, balanced), 0), "one leaf");
        CHECK(p.verdict == kStParsed && p.L == 1 && p.max_len == 0 && p.pay == 20, "one leaf");
        p = compare(stream_of(trie_of(2, balanced), 3), "two leaves");
        CHECK(p.verdict == kStParsed && p.L == 2 && p.max_len == 1 && p.pay == 8 + 25 && p.table[0] == 0 && p.table[1] == 0x80000000u, "two leaves");
        printf("ok small: one leaf (a 12-byte trie, the 20-byte stream) and two\n");
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
        const std::vector<uint8_t> full = stream_of(trie_of(kSmallTrieMaxLeaves, balanced), 5);
        Parsed p = compare(full, "16384 leaves");
        CHECK(p.verdict == kStParsed && p.L == kSmallTrieMaxLeaves && p.max_len == 14 && p.pay == 8 + st_max_bytes<S>(), "16 384 leaves of 14 bits");
        CHECK(g_most_chunks == kStMaxKRgb && st_lanes_used(st_max_bytes<S>()) == 951, "the full window: 951 lanes of 7 chunks");
        p = compare(stream_of(trie_of(kSmallTrieMaxLeaves + 1, balanced), 5), "16385 leaves");
        CHECK(p.verdict == kStNotOurs, "16 385 leaves are not ours");
        p = compare(stream_of(std::vector<uint8_t>(5000, 1), 0), "branches to the end");
        CHECK(p.verdict == kStNotDecoder, "branches to the stream's end are no decoder");
        printf("ok bound: %u leaves parsed, %u not ours; constants: leaves %u, lanes %u, chunk %u, window %u, lane chunks %u, rows %u\n", kSmallTrieMaxLeaves, kSmallTrieMaxLeaves + 1,
               kSmallTrieMaxLeaves, kStLanes, kStChunk, st_max_bytes<S>(), kStMaxKRgb, kStMaxP + 1);
    }
    // ---- the last-node word: windows with 2^17 nodes and more.  (node + 1) << 15 has no room for them; st_lane_open writes no word for a node
    // above kStLastNodeMax, and lane_parse checks every word of the table it leaves
    {
        std::vector<std::vector<uint8_t>> streams;
        streams.push_back(stream_of(std::vector<uint8_t>(st_max_bytes<S>() + 100, 1), 0));          // nothing but branches
        {   // branches, then leaves to the window's end: P comes down behind node 2^17 as far as the bytes allow
            std::vector<uint8_t> t((1u << 17) + 19, 1);
            for (uint32_t i = 0; t.size() + S + 1 <= st_max_bytes<S>() + 100; i++) put_leaf(t, i);
            streams.push_back(stream_of(t, 0));
        }
        {   // a valid trie, then payload bytes that read as more than 2^17 further nodes: branches, with a leaf's worth of zeros now and then
            std::vector<uint8_t> s = stream_of(trie_of(7, bounded), 0);
            for (uint32_t i = 0; i < 150000; i++) s.push_back(i % 4001 < 12 ? 0 : 1);
            streams.push_back(s);
        }
        {   // one leaf fewer than the largest trie, then branches: 13 of them lie in the window, nodes 32 765 .. 32 777 with P = -1 .. 11
            std::vector<uint8_t> s = stream_of(trie_of(kSmallTrieMaxLeaves - 1, balanced), 0);
            for (uint32_t i = 0; i < 40; i++) s.push_back(1);
            streams.push_back(s);
        }
        const uint32_t want[4] = {kStNotOurs, kStNotOurs, kStParsed, kStParsed};
        for (size_t i = 0; i < streams.size(); i++) {
            count_last_words(streams[i]);
            Parsed p = compare(streams[i], "2^17 nodes");
            CHECK(p.verdict == want[i], "stream %zu of the last-node family: verdict %u", i, p.verdict);
            const Parsed big = lane_parse(streams[i], kStLanes, kSmallTrieMaxLeaves);
            CHECK(big == p, "stream %zu of the last-node family in a launch at the bound", i);
        }
        CHECK(g_last_words_kept && g_last_words_dropped, "nodes with a P of 0 .. 19 on both sides of node %u", kStLastNodeMax);
        printf("ok last: windows of up to %u nodes; nodes with P <= %u: %llu up to node %u (a word each), %llu above (none)\n", st_max_bytes<S>(), kStMaxP,
               (unsigned long long)g_last_words_kept, kStLastNodeMax, (unsigned long long)g_last_words_dropped);
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
        printf("ok offsets: chunks entered at 0..%u:", S);
        for (uint32_t o = 0; o <= S; o++) { CHECK(g_entered[o] && g_left[o], "no chunk entered or left at offset %u", o); printf(" %llu", (unsigned long long)g_entered[o]); }
        printf(", left at each as well\n");
    }
    // ---- lengths around the lane-chunk switches: a window of k * 32 768 bytes is the last that 1024 lanes of k chunks hold
    {
        for (uint32_t k = 1; k <= 6; k++) {
            const uint32_t edge = k * kStLanes * kStChunk, L = edge / (S + 2);
            const std::vector<uint8_t> t = trie_of(L, bounded), longer = trie_of(L + 3, bounded);
            CHECK(t.size() == (S + 2) * L - 1 && t.size() <= edge - 1 && longer.size() > edge + 1, "a trie of %u leaves", L);
            for (uint32_t more = 0; more < 3; more++) {
                const uint32_t window = edge - 1 + more;
                CHECK(st_lane_chunks(window) == (more == 2 ? k + 1 : k), "a window of %u bytes has lanes of %u chunks", window, st_lane_chunks(window));
                Parsed p = compare(stream_of(t, window - (uint32_t)t.size()), "whole, k 32768 - 1 + more");
                CHECK(p.verdict == kStParsed && p.pay == 8 + t.size(), "k = %u, %u more", k, more);
                std::vector<uint8_t> cut = stream_of(longer, 0);
                cut.resize(8 + window);
                p = compare(cut, "cut at k 32768 - 1 + more");
                CHECK(p.verdict == kStNotDecoder, "a trie cut at %u bytes is no decoder", window);
            }
        }
        printf("ok lengths: windows of k 32768 - 1, k 32768, k 32768 + 1 bytes for k = 1 .. 6, whole and cut\n");
    }
    // ---- cuts and edits of a 7-leaf stream
    {
        const std::vector<uint8_t> t = trie_of(7, bounded);
        CHECK(t.size() == 90, "seven leaves");
        const std::vector<uint8_t> s = stream_of(t, 6);
        uint32_t by_verdict[4] = {0, 0, 0, 0};
        for (size_t n = 8; n <= s.size(); n++) {
            Parsed p = compare(std::vector<uint8_t>(s.begin(), s.begin() + n), "cut");
            CHECK((p.verdict == kStParsed) == (n >= 8 + 90) && (p.verdict == kStParsed || p.verdict == kStNotDecoder), "cut at %zu", n);
        }
        for (size_t at = 0; at < 90; at++)
            for (uint32_t d = 1; d < 256; d++) {
                std::vector<uint8_t> e = s;
                e[8 + at] = (uint8_t)(e[8 + at] + d);
                by_verdict[compare(e, "edit").verdict]++;
            }
        CHECK(by_verdict[kStParsed] && by_verdict[kStNotDecoder], "edits parse and fail");
        printf("ok mutations: every cut; %u edits: %u parsed, %u no decoder, %u not ours\n", 90 * 255, by_verdict[kStParsed], by_verdict[kStNotDecoder], by_verdict[kStNotOurs]);
    }
    // ---- the length word, a trie that ends with the stream
    {
        for (uint64_t len : {3ull, 2ull, 4ull, 3ull + (1ull << 32), 0ull, 3ull << 56}) {
            for (uint32_t lead = 0; lead < 4; lead++) {   // (the symbol at every byte shift)
                std::vector<uint8_t> t(lead + 1, 1);
                put_leaf(t, 0, len);
                for (uint32_t i = 0; i <= lead; i++) put_leaf(t, i + 1);
                Parsed p = compare(stream_of(t, 2), "length word");
                CHECK((p.verdict == kStParsed) == (len == 3) && (p.verdict == kStParsed || p.verdict == kStNotDecoder), "a length word of %llu", (unsigned long long)len);
            }
        }
        Parsed p = compare(stream_of(trie_of(300, bounded), 0), "no payload");
        CHECK(p.verdict == kStParsed && p.pay == 8 + 13 * 300 - 1, "a trie that ends exactly at the stream's end");
        printf("ok symbols: a length word of 3 parsed; 2, 4, 3 + 2^32 no decoder; a trie that ends with its stream\n");
    }
    printf("%s: %llu streams compared, the code identities asserted on every parsed one\n", g_fail ? "FAIL" : "ok total", (unsigned long long)g_compared);
    return g_fail ? 1 : 0;
}
