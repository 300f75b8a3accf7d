// delta_small_check.cpp -- what the small-frame `delta` kernel computes per frame (cniic_amd/csrc/delta_small.hpp, delta_sym.hpp), checked on the host.
// A scalar encoder built from the headers' functions -- the leaf order word, the merge in runs of 64 "lanes" as one wave takes them, the
// walks to the root, the header and the payload -- runs beside a plain restatement: a binary heap ordered by (count, leaf before branch,
// key / order of making), codes by recursion from the root, the trie written in pre-order by recursion.  Tree shape, code lengths, codes,
// header bytes and total length must agree.
// Build: c++ -O2 -std=c++17 -I cniic_amd/csrc tests/delta_small_check.cpp.  Prints "ok <part>: ..." per part; exit status 1 on a mismatch.
//
// Second mode: delta_small_check --keys FILE W H [OUT] reads W * H little-endian u32 keys by scan position from FILE, runs the scalar
// encoder above on them (not the restatement) and prints the stream's length and CRC-32 (OUT, if given, receives the stream), then what
// the merge did -- per queue the runs of pairs that were full (64), cut by the weight test, or ended by the queue; a leaf run of one pair
// before any branch exists is "single" -- the general steps by the order of their two picks, the longest code, and how many of the
// kernel's 1024 threads write payload bits that end exactly on a 32-bit word.  tests/test_delta_small_edges_cpu.py reads these lines.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <queue>
#include <tuple>
#include <vector>

#include "delta_small.hpp"
#include "delta_sym.hpp"

using namespace cniic;

static int g_fail = 0;
static uint32_t g_longest = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % n);
}

struct Encoded {
    std::vector<uint32_t> left, right;   // per branch, node ids: leaf q (in (count, key) order) or U + branch
    std::vector<uint32_t> len, code;     // per rank (ascending key)
    std::vector<uint8_t> bytes;          // the whole stream
    uint32_t longest = 0;
    bool operator==(const Encoded &o) const { return left == o.left && right == o.right && len == o.len && code == o.code && bytes == o.bytes; }
};

// what the merge and the payload phase did on one frame (the second mode prints it)
struct MergeStats {
    uint32_t leaf_full = 0, leaf_cut = 0, leaf_queue = 0, leaf_single = 0;   // runs of leaf pairs by what ended them
    uint32_t branch_full = 0, branch_cut = 0, branch_queue = 0;
    uint32_t general[2][2] = {{0, 0}, {0, 0}};                               // [first pick][second pick], 0 = leaf, 1 = branch
    uint32_t longest_leaf_run = 0, longest_branch_run = 0;
    uint32_t threads_with_bits = 0, word_ends = 0, most_thread_bits = 0;
};

static void put_bits(std::vector<uint8_t> &o, uint64_t &bitpos, uint32_t code, uint32_t len) {   // MSB first
    for (uint32_t i = 0; i < len; i++, bitpos++) {
        if ((bitpos >> 3) >= o.size()) o.push_back(0);
        if ((code >> (len - 1 - i)) & 1u) o[bitpos >> 3] |= (uint8_t)(0x80u >> (bitpos & 7));
    }
}

// ---- the kernel's way, scalar, from the headers' functions.  syms: the keys by position
static Encoded encode_headers(uint32_t w, uint32_t h, const std::vector<uint32_t> &syms, MergeStats *ms = nullptr) {
    Encoded e;
    const uint32_t n = (uint32_t)syms.size();
    std::vector<uint32_t> keys(syms);
    std::sort(keys.begin(), keys.end());
    std::vector<uint32_t> cnt;
    {
        std::vector<uint32_t> uk;
        for (uint32_t i = 0; i < n; i++) {
            if (i == 0 || keys[i] != keys[i - 1]) { uk.push_back(keys[i]); cnt.push_back(0); }
            cnt.back()++;
        }
        keys.swap(uk);
    }
    const uint32_t U = (uint32_t)keys.size();
    e.len.assign(U, 0); e.code.assign(U, 0);
    e.bytes.resize(ds_header_bytes(U));
    for (int i = 0; i < 4; i++) { e.bytes[i] = (uint8_t)(w >> (8 * i)); e.bytes[4 + i] = (uint8_t)(h >> (8 * i)); }
    if (U == 1) {
        e.bytes[8] = 0;
        ds_leaf_bytes(keys[0], &e.bytes[9]);
        return e;
    }
    std::vector<uint32_t> ord(U);
    for (uint32_t r = 0; r < U; r++) ord[r] = ds_leaf_order(cnt[r], r);
    std::sort(ord.begin(), ord.end());
    std::vector<uint16_t> qrank(U), lq(U), bq(U), nl(U);
    for (uint32_t q = 0; q < U; q++) { qrank[q] = (uint16_t)ds_order_rank(ord[q]); lq[q] = (uint16_t)ds_order_count(ord[q]); }
    const uint32_t nbr = U - 1, root = U - 2;
    e.left.assign(nbr, 0); e.right.assign(nbr, 0);
    uint32_t li = 0, bi = 0, made = 0;
    while (made < nbr) {
        {   // a run of leaf pairs: 64 lanes test, the leading ones that pass are taken
            const bool hb = bi < made;
            const uint32_t bw = hb ? bq[bi] : 0u;
            uint32_t c = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t i1 = li + 2 * lane + 1;
                if (!((hb || lane == 0) && i1 < U && ds_leaf_pair(lq[i1], hb, bw))) break;
                c++;
            }
            if (c && ms) {
                const uint32_t i1 = li + 2 * c + 1;   // the pair that ended the run
                if (c == 64) ms->leaf_full++;
                else if (!hb) ms->leaf_single++;
                else if (i1 >= U) ms->leaf_queue++;
                else ms->leaf_cut++;
                ms->longest_leaf_run = std::max(ms->longest_leaf_run, c);
            }
            if (c) {
                std::vector<uint32_t> a(c), b(c);
                for (uint32_t lane = 0; lane < c; lane++) { a[lane] = lq[li + 2 * lane]; b[lane] = lq[li + 2 * lane + 1]; }
                for (uint32_t lane = 0; lane < c; lane++) {
                    const uint32_t i1 = li + 2 * lane + 1;
                    lq[i1 - 1] = (uint16_t)ds_link(made + lane, 0); lq[i1] = (uint16_t)ds_link(made + lane, 1);
                    bq[made + lane] = (uint16_t)(a[lane] + b[lane]); nl[made + lane] = 2;
                    e.left[made + lane] = i1 - 1; e.right[made + lane] = i1;
                }
                li += 2 * c; made += c;
                continue;
            }
        }
        {   // a run of branch pairs
            const bool hl = li < U;
            const uint32_t lw = hl ? lq[li] : 0u;
            uint32_t c = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t i1 = bi + 2 * lane + 1;
                if (!(i1 < made && ds_branch_pair(bq[i1], hl, lw))) break;
                c++;
            }
            if (c && ms) {
                if (c == 64) ms->branch_full++;
                else if (bi + 2 * c + 1 >= made) ms->branch_queue++;
                else ms->branch_cut++;
                ms->longest_branch_run = std::max(ms->longest_branch_run, c);
            }
            if (c) {
                std::vector<uint32_t> a(c), b(c), na(c), nb(c);
                for (uint32_t lane = 0; lane < c; lane++) { a[lane] = bq[bi + 2 * lane]; b[lane] = bq[bi + 2 * lane + 1]; na[lane] = nl[bi + 2 * lane]; nb[lane] = nl[bi + 2 * lane + 1]; }
                for (uint32_t lane = 0; lane < c; lane++) {
                    const uint32_t i1 = bi + 2 * lane + 1;
                    bq[i1 - 1] = (uint16_t)ds_link(made + lane, 0); bq[i1] = (uint16_t)ds_link(made + lane, 1);
                    bq[made + lane] = (uint16_t)(a[lane] + b[lane]); nl[made + lane] = (uint16_t)(na[lane] + nb[lane]);
                    e.left[made + lane] = U + i1 - 1; e.right[made + lane] = U + i1;
                }
                bi += 2 * c; made += c;
                continue;
            }
        }
        uint32_t wsum = 0, leaves = 0, picks[2];
        for (uint32_t k = 0; k < 2; k++) {
            const bool hl = li < U, hb = bi < made;
            const uint32_t lw = hl ? lq[li] : 0u, bw = hb ? bq[bi] : 0u;
            uint32_t node;
            if (ds_pick_leaf(hl, lw, hb, bw)) { wsum += lw; leaves += 1; lq[li] = (uint16_t)ds_link(made, k); node = li++; picks[k] = 0; }
            else { wsum += bw; leaves += nl[bi]; bq[bi] = (uint16_t)ds_link(made, k); node = U + bi++; picks[k] = 1; }
            (k ? e.right : e.left)[made] = node;
        }
        if (ms) ms->general[picks[0]][picks[1]]++;
        bq[made] = (uint16_t)wsum; nl[made] = (uint16_t)leaves;
        made++;
    }
    if (bq[root] != n || nl[root] != U) { printf("FAIL: the root weighs %u with %u leaves, expected %u and %u\n", bq[root], nl[root], n, U); g_fail = 1; }
    auto walk = [&](uint32_t link, uint32_t leaves) {
        DsWalk wk;
        for (;;) {
            const uint32_t p = ds_link_parent(link), pl = nl[p];
            ds_walk_step(wk, link, leaves, pl);
            if (p == root) break;
            leaves = pl; link = bq[p];
        }
        return wk;
    };
    std::vector<uint32_t> cw(U);
    for (uint32_t q = 0; q < U; q++) {
        const DsWalk wk = walk(lq[q], 1);
        const uint32_t r = qrank[q];
        cw[r] = ds_codeword(wk.code, wk.depth);
        e.len[r] = wk.depth; e.code[r] = wk.code;
        e.longest = std::max(e.longest, wk.depth);
        e.bytes[8 + wk.off] = 0;
        ds_leaf_bytes(keys[r], &e.bytes[9 + wk.off]);
    }
    for (uint32_t j = 0; j < nbr; j++) e.bytes[8 + (j == root ? 0u : walk(bq[j], nl[j]).off)] = 1;
    uint64_t bitpos = (uint64_t)e.bytes.size() * 8, bits = 0;
    const uint32_t per = (n + 1023) / 1024;   // consecutive positions per thread of the kernel's payload phase
    uint32_t mine = 0;                        // bits of the thread that d belongs to
    for (uint32_t d = 0; d < n; d++) {
        const uint32_t r = (uint32_t)(std::upper_bound(keys.begin(), keys.end(), syms[d]) - keys.begin()) - 1;
        put_bits(e.bytes, bitpos, ds_codeword_code(cw[r]), ds_codeword_len(cw[r]));
        bits += ds_codeword_len(cw[r]);
        mine += ds_codeword_len(cw[r]);
        if (ms && ((d + 1) % per == 0 || d + 1 == n)) {
            if (mine) { ms->threads_with_bits++; ms->word_ends += (bitpos & 31) == 0; }
            ms->most_thread_bits = std::max(ms->most_thread_bits, mine);
            mine = 0;
        }
    }
    if (e.bytes.size() != ds_stream_bytes(U, bits) || e.bytes.size() > ds_stride(n)) { printf("FAIL: %zu bytes, ds_stream_bytes %llu, ds_stride %llu\n", e.bytes.size(), (unsigned long long)ds_stream_bytes(U, bits), (unsigned long long)ds_stride(n)); g_fail = 1; }
    return e;
}

// ---- the plain restatement
static Encoded encode_plain(uint32_t w, uint32_t h, const std::vector<uint32_t> &syms) {
    Encoded e;
    std::vector<std::pair<uint32_t, uint32_t>> kc;   // (key, count), ascending key
    {
        std::vector<uint32_t> s(syms);
        std::sort(s.begin(), s.end());
        for (size_t i = 0; i < s.size(); i++) { if (i == 0 || s[i] != s[i - 1]) kc.push_back({s[i], 0}); kc.back().second++; }
    }
    const uint32_t U = (uint32_t)kc.size();
    // leaf q = the q-th by (count, key)
    std::vector<uint32_t> byq(U);
    for (uint32_t r = 0; r < U; r++) byq[r] = r;
    std::stable_sort(byq.begin(), byq.end(), [&](uint32_t a, uint32_t b) { return kc[a].second < kc[b].second; });
    typedef std::tuple<uint64_t, int, uint32_t, uint32_t> Item;   // count, 0 leaf / 1 branch, key or order of making, node id
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (uint32_t q = 0; q < U; q++) heap.push(Item{kc[byq[q]].second, 0, kc[byq[q]].first, q});
    uint32_t made = 0;
    while (heap.size() > 1) {
        const Item a = heap.top(); heap.pop();
        const Item b = heap.top(); heap.pop();
        e.left.push_back(std::get<3>(a)); e.right.push_back(std::get<3>(b));
        heap.push(Item{std::get<0>(a) + std::get<0>(b), 1, made, U + made});
        made++;
    }
    e.len.assign(U, 0); e.code.assign(U, 0);
    for (int i = 0; i < 4; i++) e.bytes.push_back((uint8_t)(w >> (8 * i)));
    for (int i = 0; i < 4; i++) e.bytes.push_back((uint8_t)(h >> (8 * i)));
    std::function<void(uint32_t, uint32_t, uint32_t)> rec = [&](uint32_t node, uint32_t code, uint32_t depth) {
        if (node < U) {
            const uint32_t r = byq[node], key = kc[r].first;
            e.len[r] = depth; e.code[r] = code;
            e.longest = std::max(e.longest, depth);
            e.bytes.push_back(0);
            for (int i = 0; i < 3; i++) {
                const int v = (int)((key >> (18 - 9 * i)) & 511) - 255;
                const uint16_t u = (uint16_t)(int16_t)v;
                e.bytes.push_back((uint8_t)u); e.bytes.push_back((uint8_t)(u >> 8));
            }
            return;
        }
        e.bytes.push_back(1);
        rec(e.left[node - U], code << 1, depth + 1);
        rec(e.right[node - U], (code << 1) | 1u, depth + 1);
    };
    rec(U > 1 ? 2 * U - 2 : 0, 0, 0);
    uint64_t bitpos = (uint64_t)e.bytes.size() * 8;
    std::vector<uint32_t> keys(U);
    for (uint32_t r = 0; r < U; r++) keys[r] = kc[r].first;
    for (uint32_t s : syms) {
        const uint32_t r = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), s) - keys.begin());
        put_bits(e.bytes, bitpos, e.code[r], e.len[r]);
    }
    return e;
}

// the symbols of a frame with the given counts: count[i] copies of key i (spread over the key's three fields), shuffled
static std::vector<uint32_t> symbols_of(const std::vector<uint32_t> &counts, bool shuffle = true) {
    std::vector<uint32_t> s;
    for (size_t i = 0; i < counts.size(); i++) {
        const uint32_t key = (uint32_t)((i * 7919ull) % (511u * 511u * 511u));   // (7919 is coprime to 511: distinct keys)
        const uint32_t k = ((key / (511u * 511u)) << 18) | (((key / 511u) % 511u) << 9) | (key % 511u);
        for (uint32_t c = 0; c < counts[i]; c++) s.push_back(k);
    }
    if (shuffle) for (size_t i = s.size(); i > 1; i--) std::swap(s[i - 1], s[rnd((uint32_t)i)]);
    return s;
}

static uint32_t check(const char *what, const std::vector<uint32_t> &syms, uint32_t w = 0, uint32_t h = 0) {
    if (!w) { w = (uint32_t)syms.size(); h = 1; }
    if (syms.empty() || syms.size() > kDeltaSmallMaxPx) { printf("FAIL %s: the case has %zu symbols\n", what, syms.size()); g_fail = 1; return 0; }
    const Encoded a = encode_headers(w, h, syms), b = encode_plain(w, h, syms);
    if (!(a == b)) {
        printf("FAIL %s: %zu symbols: shape %d lengths %d codes %d bytes %d (%zu / %zu)\n", what, syms.size(), a.left == b.left && a.right == b.right, a.len == b.len,
               a.code == b.code, a.bytes == b.bytes, a.bytes.size(), b.bytes.size());
        g_fail = 1;
    }
    if (a.longest > kDeltaSmallMaxCodeLen) { printf("FAIL %s: a code of %u bits\n", what, a.longest); g_fail = 1; }
    g_longest = std::max(g_longest, a.longest);
    return a.longest;
}

static uint32_t crc32_of(const std::vector<uint8_t> &v) {   // the CRC-32 of zlib
    uint32_t c = 0xffffffffu;
    for (uint8_t b : v) {
        c ^= b;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

// the second mode: one frame's keys from a file
static int keys_mode(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s --keys FILE W H [OUT]\n", argv[0]); return 2; }
    const uint32_t w = (uint32_t)strtoul(argv[3], nullptr, 10), h = (uint32_t)strtoul(argv[4], nullptr, 10);
    const uint64_t n = (uint64_t)w * h;
    if (!n || n > kDeltaSmallMaxPx) { fprintf(stderr, "%u x %u is outside the route\n", w, h); return 2; }
    std::vector<uint8_t> raw(4 * n);
    FILE *f = fopen(argv[2], "rb");
    if (!f || fread(raw.data(), 1, raw.size(), f) != raw.size() || fgetc(f) != EOF) { fprintf(stderr, "%s does not hold %llu keys\n", argv[2], (unsigned long long)n); return 2; }
    fclose(f);
    std::vector<uint32_t> syms(n);
    for (uint64_t i = 0; i < n; i++) {
        syms[i] = (uint32_t)raw[4 * i] | ((uint32_t)raw[4 * i + 1] << 8) | ((uint32_t)raw[4 * i + 2] << 16) | ((uint32_t)raw[4 * i + 3] << 24);
        if (syms[i] >> 27) { fprintf(stderr, "key %llu is no three 9-bit fields\n", (unsigned long long)i); return 2; }
    }
    MergeStats ms;
    const Encoded e = encode_headers(w, h, syms, &ms);
    if (argc > 5) {
        FILE *o = fopen(argv[5], "wb");
        if (!o || fwrite(e.bytes.data(), 1, e.bytes.size(), o) != e.bytes.size() || fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
    }
    printf("stream %zu %08x\n", e.bytes.size(), crc32_of(e.bytes));
    printf("tree leaves %zu longest %u\n", e.len.size(), e.longest);
    printf("leaf_runs full %u cut %u queue %u single %u longest %u\n", ms.leaf_full, ms.leaf_cut, ms.leaf_queue, ms.leaf_single, ms.longest_leaf_run);
    printf("branch_runs full %u cut %u queue %u longest %u\n", ms.branch_full, ms.branch_cut, ms.branch_queue, ms.longest_branch_run);
    printf("general leaf_leaf %u leaf_branch %u branch_leaf %u branch_branch %u\n", ms.general[0][0], ms.general[0][1], ms.general[1][0], ms.general[1][1]);
    printf("payload threads %u word_ends %u most_bits %u\n", ms.threads_with_bits, ms.word_ends, ms.most_thread_bits);
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--keys")) return keys_mode(argc, argv);
    {   // random symbol lists: a few to many distinct symbols, skewed and flat
        for (int rep = 0; rep < 60; rep++) {
            const uint32_t n = rep < 4 ? 1 + rnd(8) : 1 + rnd(kDeltaSmallMaxPx), spread = 1 + rnd(rep % 3 ? 40 : 511);
            std::vector<uint32_t> s(n);
            for (uint32_t i = 0; i < n; i++) {
                uint32_t hot;
                const uint32_t a = rnd(spread) | (rnd(spread) << 8) | (rnd(spread) << 16), b = rnd(spread) | (rnd(spread) << 8) | (rnd(spread) << 16);
                s[i] = delta_key(a & 0xffffffu & (rep & 1 ? 0xffffffu : 0x0f0f0fu), b & (rep & 1 ? 0xffffffu : 0x0f0f0fu), hot);
            }
            check("random", s);
        }
        {   // every key field at both ends
            uint32_t hot;
            std::vector<uint32_t> s = {delta_key(0xffffffu, 0u, hot), delta_key(0u, 0xffffffu, hot), delta_key(0xffffffu, 0u, hot), delta_key(0u, 0u, hot), delta_key(0xff00ffu, 0x00ff00u, hot)};
            check("random", s);
        }
        printf("ok random: 61 lists\n");
    }
    {
        const uint32_t L = check("all_ones", symbols_of(std::vector<uint32_t>(kDeltaSmallMaxPx, 1)));
        check("all_ones", symbols_of(std::vector<uint32_t>(kDeltaSmallMaxPx - 4, 1)));
        check("all_ones", symbols_of(std::vector<uint32_t>(12345, 1)));
        printf("ok all_ones: %u leaves, every code %u bits\n", kDeltaSmallMaxPx, L);
        if (L != 14) { printf("FAIL all_ones: 16384 equal leaves make a complete tree of depth 14\n"); g_fail = 1; }
    }
    {
        std::vector<uint32_t> c = {1};
        for (uint32_t v = 1; v <= 4096; v <<= 1) c.push_back(v);
        const std::vector<uint32_t> s = symbols_of(c);
        const uint32_t L = check("powers", s, 128, 64);
        printf("ok powers: %zu leaves, %zu symbols, longest code %u\n", c.size(), s.size(), L);
        if (c.size() != 14 || s.size() != 8192 || L != 13) { printf("FAIL powers: expected 14 leaves, 8192 symbols, 13 bits\n"); g_fail = 1; }
    }
    {
        std::vector<uint32_t> c = {1, 1};
        uint32_t tot = 2;
        while (tot + c[c.size() - 1] + c[c.size() - 2] <= kDeltaSmallMaxPx) { c.push_back(c[c.size() - 1] + c[c.size() - 2]); tot += c.back(); }
        const uint32_t L = check("fibonacci", symbols_of(c));
        // the chain that meets the bound under "a leaf before a branch": every branch strictly lighter than the leaf after next
        std::vector<uint32_t> ch = {1, 1, 1};
        std::vector<uint32_t> br = {2, 3};   // branch k = branch k - 1 + branch k - 2 + 1
        uint32_t ctot = 3;
        for (;;) {
            const uint32_t leaf = br[br.size() - 2] + 1;
            if (ctot + leaf > kDeltaSmallMaxPx) break;
            ch.push_back(leaf); ctot += leaf;
            br.push_back(br[br.size() - 1] + br[br.size() - 2] + 1);
        }
        const uint32_t Lc = check("fibonacci", symbols_of(ch));
        printf("ok fibonacci: %zu leaves %u symbols longest %u; strict chain %zu leaves %u symbols longest %u (the bound: %u)\n", c.size(), tot, L, ch.size(), ctot, Lc,
               kDeltaSmallMaxCodeLen);
        if (Lc != kDeltaSmallMaxCodeLen || ch.size() != 20 || ctot != 15126) { printf("FAIL fibonacci: the strict chain does not meet the bound\n"); g_fail = 1; }
        // F(22) > 16384: no total count within the route carries a code of 20 bits
        uint64_t f1 = 1, f2 = 1;
        for (int i = 3; i <= 22; i++) { const uint64_t f = f1 + f2; f1 = f2; f2 = f; }
        if (!(f1 <= kDeltaSmallMaxPx && f2 > kDeltaSmallMaxPx)) { printf("FAIL fibonacci: F(21) = %llu, F(22) = %llu against %u\n", (unsigned long long)f1, (unsigned long long)f2, kDeltaSmallMaxPx); g_fail = 1; }
    }
    {
        const Encoded a = encode_headers(20, 30, std::vector<uint32_t>(600, 0x3fdfeffu));
        check("one", std::vector<uint32_t>(600, 0x3fdfeffu), 20, 30);
        check("one", std::vector<uint32_t>(1, 12345u));
        check("one", std::vector<uint32_t>(kDeltaSmallMaxPx, 0u));
        printf("ok one: %zu bytes, no payload\n", a.bytes.size());
        if (a.bytes.size() != 15) { printf("FAIL one: expected 15 bytes\n"); g_fail = 1; }
    }
    {
        check("two", symbols_of({1, 1}));
        check("two", symbols_of({1, 599}));
        check("two", symbols_of({8192, 8192}));
        check("two", symbols_of({3, 2}, false));
        printf("ok two\n");
    }
    {   // runs of 2^k - 1 / 2^k / 2^k + 1 equal counts: where a run of pairs ends inside, at and just behind a wave's 64 lanes and a power of two
        int cases = 0;
        for (uint32_t k = 1; k <= 12; k++)
            for (int d = -1; d <= 1; d++) {
                const uint32_t m = (1u << k) + d;
                if (m < 1) continue;
                for (uint32_t cnt = 1; cnt <= 3; cnt++) {
                    if (m * cnt > kDeltaSmallMaxPx) continue;
                    check("runs", symbols_of(std::vector<uint32_t>(m, cnt)));
                    std::vector<uint32_t> c(m, cnt);   // ... followed by a second run and a heavy leaf
                    const uint32_t m2 = (1u << (k > 1 ? k - 1 : 1)) - d;
                    for (uint32_t i = 0; i < m2; i++) c.push_back(2 * cnt);
                    c.push_back(cnt * m / 2 + 1);
                    uint64_t tot = 0;
                    for (uint32_t v : c) tot += v;
                    if (tot <= kDeltaSmallMaxPx) { check("runs", symbols_of(c)); cases++; }
                    cases++;
                }
            }
        printf("ok runs: %d lists\n", cases);
    }
    printf("ok total: longest code met %u, bound %u, stride at the bound %llu\n", g_longest, kDeltaSmallMaxCodeLen, (unsigned long long)ds_stride(kDeltaSmallMaxPx));
    if (g_longest != kDeltaSmallMaxCodeLen) { printf("FAIL total: the bound was not met\n"); g_fail = 1; }
    return g_fail;
}
