// huf_small_check.cpp -- what the small-frame `hufman` kernel computes per frame (cniic_amd/csrc/huf_small.hpp, delta_small.hpp), checked on the host.
// A scalar encoder built from the headers' functions -- the key, the leaf order word, the merge in runs of 64 "lanes" as one wave takes
// them, the walks to the root, the leaf bytes, the header and the payload -- runs beside a plain restatement that never sees a key: colours
// compared as (r, g, b), a binary heap ordered by (count, leaf before branch, colour / order of making), codes by recursion from the
// root, the trie written byte by byte in pre-order.  Tree shape, code lengths, codes, header bytes and total length must agree.
// The decode side: k_huf_small_dec's lane (delta_small_dec.hpp's lookup, pass and end-of-stream rule over RGB keys, hs_pixel_bytes) on the
// restatement's streams, whole and cut, against a bit-by-bit walk of the serialised trie.
// Build: c++ -O2 -std=c++17 -I cniic_amd/csrc tests/huf_small_check.cpp.  Prints "ok <part>: ..." per part; exit status 1 on a mismatch.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <queue>
#include <tuple>
#include <vector>

#include "huf_small.hpp"
#include "delta_small_dec.hpp"

using namespace cniic;

typedef std::array<uint8_t, 3> Px;

static int g_fail = 0;
static uint32_t g_longest = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % n);
}

struct Encoded {
    std::vector<uint32_t> left, right;   // per branch, node ids: leaf q (in (count, colour) order) or U + branch
    std::vector<uint32_t> len, code;     // per rank (ascending colour)
    std::vector<uint8_t> bytes;          // the whole stream
    uint32_t longest = 0;
    bool operator==(const Encoded &o) const { return left == o.left && right == o.right && len == o.len && code == o.code && bytes == o.bytes; }
};

static void put_bits(std::vector<uint8_t> &o, uint64_t &bitpos, uint32_t code, uint32_t len) {   // MSB first
    for (uint32_t i = 0; i < len; i++, bitpos++) {
        if ((bitpos >> 3) >= o.size()) o.push_back(0);
        if ((code >> (len - 1 - i)) & 1u) o[bitpos >> 3] |= (uint8_t)(0x80u >> (bitpos & 7));
    }
}

// ---- the kernel's way, scalar, from the headers' functions.  px: the pixels in row-major order
static Encoded encode_headers(uint32_t w, uint32_t h, const std::vector<Px> &px) {
    Encoded e;
    const uint32_t n = (uint32_t)px.size();
    std::vector<uint32_t> syms(n);
    for (uint32_t d = 0; d < n; d++) syms[d] = hs_key(px[d][0], px[d][1], px[d][2]);
    std::vector<uint32_t> keys(syms), cnt;
    std::sort(keys.begin(), keys.end());
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
    e.bytes.resize(hs_header_bytes(U));
    for (int i = 0; i < 4; i++) { e.bytes[i] = (uint8_t)(w >> (8 * i)); e.bytes[4 + i] = (uint8_t)(h >> (8 * i)); }
    if (U == 1) {
        e.bytes[8] = 0;
        hs_leaf_bytes(keys[0], &e.bytes[9]);
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
        uint32_t wsum = 0, leaves = 0;
        for (uint32_t k = 0; k < 2; k++) {
            const bool hl = li < U, hb = bi < made;
            const uint32_t lw = hl ? lq[li] : 0u, bw = hb ? bq[bi] : 0u;
            uint32_t node;
            if (ds_pick_leaf(hl, lw, hb, bw)) { wsum += lw; leaves += 1; lq[li] = (uint16_t)ds_link(made, k); node = li++; }
            else { wsum += bw; leaves += nl[bi]; bq[bi] = (uint16_t)ds_link(made, k); node = U + bi++; }
            (k ? e.right : e.left)[made] = node;
        }
        bq[made] = (uint16_t)wsum; nl[made] = (uint16_t)leaves;
        made++;
    }
    if (bq[root] != n || nl[root] != U) { printf("FAIL: the root weighs %u with %u leaves, expected %u and %u\n", bq[root], nl[root], n, U); g_fail = 1; }
    bool deep = false;
    auto walk = [&](uint32_t link, uint32_t leaves) {
        DsWalk wk;
        for (uint32_t s = 0;; s++) {
            if (s == kDeltaSmallMaxCodeLen) { deep = true; break; }   // (the kernel reports such a frame and writes nothing)
            const uint32_t p = ds_link_parent(link), pl = nl[p];
            hs_walk_step(wk, link, leaves, pl);
            if (p == root) break;
            leaves = pl; link = bq[p];
        }
        return wk;
    };
    std::vector<uint32_t> cw(U);
    for (uint32_t q = 0; q < U; q++) {
        const DsWalk wk = walk(lq[q], 1);
        if (deep || wk.off + 1 + kHufSmallLeafSym > e.bytes.size() - 8) { printf("FAIL: leaf %u walks out of the header\n", q); g_fail = 1; return e; }
        const uint32_t r = qrank[q];
        cw[r] = ds_codeword(wk.code, wk.depth);
        e.len[r] = wk.depth; e.code[r] = wk.code;
        e.longest = std::max(e.longest, wk.depth);
        e.bytes[8 + wk.off] = 0;
        hs_leaf_bytes(keys[r], &e.bytes[9 + wk.off]);
    }
    for (uint32_t j = 0; j < nbr; j++) {
        const uint32_t off = j == root ? 0u : walk(bq[j], nl[j]).off;
        if (deep || off + 1 > e.bytes.size() - 8) { printf("FAIL: branch %u walks out of the header\n", j); g_fail = 1; return e; }
        e.bytes[8 + off] = 1;
    }
    uint64_t bitpos = (uint64_t)e.bytes.size() * 8, bits = 0;
    for (uint32_t d = 0; d < n; d++) {
        const uint32_t r = (uint32_t)(std::upper_bound(keys.begin(), keys.end(), syms[d]) - keys.begin()) - 1;
        put_bits(e.bytes, bitpos, ds_codeword_code(cw[r]), ds_codeword_len(cw[r]));
        bits += ds_codeword_len(cw[r]);
    }
    if (e.bytes.size() != hs_stream_bytes(U, bits) || e.bytes.size() > hs_stride(n)) { printf("FAIL: %zu bytes, hs_stream_bytes %llu, hs_stride %llu\n", e.bytes.size(), (unsigned long long)hs_stream_bytes(U, bits), (unsigned long long)hs_stride(n)); g_fail = 1; }
    return e;
}

// ---- the plain restatement: colours as (r, g, b), no key
static Encoded encode_plain(uint32_t w, uint32_t h, const std::vector<Px> &px) {
    Encoded e;
    std::vector<std::pair<Px, uint32_t>> kc;   // (colour, count), ascending colour
    {
        std::vector<Px> s(px);
        std::sort(s.begin(), s.end());
        for (size_t i = 0; i < s.size(); i++) { if (i == 0 || s[i] != s[i - 1]) kc.push_back({s[i], 0}); kc.back().second++; }
    }
    const uint32_t U = (uint32_t)kc.size();
    std::vector<uint32_t> byq(U);   // leaf q = the q-th by (count, colour)
    for (uint32_t r = 0; r < U; r++) byq[r] = r;
    std::stable_sort(byq.begin(), byq.end(), [&](uint32_t a, uint32_t b) { return kc[a].second < kc[b].second; });
    typedef std::tuple<uint64_t, int, uint32_t, uint32_t> Item;   // count, 0 leaf / 1 branch, rank of the colour or order of making, node id
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (uint32_t q = 0; q < U; q++) heap.push(Item{kc[byq[q]].second, 0, byq[q], q});
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
            const uint32_t r = byq[node];
            e.len[r] = depth; e.code[r] = code;
            e.longest = std::max(e.longest, depth);
            e.bytes.push_back(0);
            const uint64_t three = 3;
            for (int i = 0; i < 8; i++) e.bytes.push_back((uint8_t)(three >> (8 * i)));
            for (int i = 0; i < 3; i++) e.bytes.push_back(kc[r].first[i]);
            return;
        }
        e.bytes.push_back(1);
        rec(e.left[node - U], code << 1, depth + 1);
        rec(e.right[node - U], (code << 1) | 1u, depth + 1);
    };
    rec(U > 1 ? 2 * U - 2 : 0, 0, 0);
    uint64_t bitpos = (uint64_t)e.bytes.size() * 8;
    std::vector<Px> cols(U);
    for (uint32_t r = 0; r < U; r++) cols[r] = kc[r].first;
    for (const Px &p : px) {
        const uint32_t r = (uint32_t)(std::lower_bound(cols.begin(), cols.end(), p) - cols.begin());
        put_bits(e.bytes, bitpos, e.code[r], e.len[r]);
    }
    return e;
}

// the pixels of a frame with the given counts: count[i] copies of colour i * 7919 mod 2^24 (7919 is odd: distinct colours), shuffled
static std::vector<Px> pixels_of(const std::vector<uint32_t> &counts, bool shuffle = true) {
    std::vector<Px> s;
    for (size_t i = 0; i < counts.size(); i++) {
        const uint32_t v = (uint32_t)((i * 7919ull) & 0xffffffu);
        for (uint32_t c = 0; c < counts[i]; c++) s.push_back(Px{(uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v});
    }
    if (shuffle) for (size_t i = s.size(); i > 1; i--) std::swap(s[i - 1], s[rnd((uint32_t)i)]);
    return s;
}

static Encoded check(const char *what, const std::vector<Px> &px, uint32_t w = 0, uint32_t h = 0) {
    if (!w) { w = (uint32_t)px.size(); h = 1; }
    if (px.empty() || px.size() > kHufSmallMaxPx) { printf("FAIL %s: the case has %zu pixels\n", what, px.size()); g_fail = 1; return Encoded(); }
    const Encoded a = encode_headers(w, h, px), b = encode_plain(w, h, px);
    if (!(a == b)) {
        printf("FAIL %s: %zu pixels: shape %d lengths %d codes %d bytes %d (%zu / %zu)\n", what, px.size(), a.left == b.left && a.right == b.right, a.len == b.len,
               a.code == b.code, a.bytes == b.bytes, a.bytes.size(), b.bytes.size());
        g_fail = 1;
    }
    if (a.longest > kDeltaSmallMaxCodeLen) { printf("FAIL %s: a code of %u bits\n", what, a.longest); g_fail = 1; }
    g_longest = std::max(g_longest, a.longest);
    return a;
}

// ---- the decode.  The stream's trie, leaf by leaf in pre-order: codes left-aligned in 32 bits, key | length << 27
struct Table { std::vector<uint32_t> code, keylen; uint32_t max_len = 0; size_t pay = 0; };
static Table table_of(const std::vector<uint8_t> &s) {
    Table t;
    size_t pos = 8;
    std::function<void(uint32_t, uint32_t)> rec = [&](uint32_t code, uint32_t depth) {
        if (s[pos++] == 1) { rec(code << 1, depth + 1); rec((code << 1) | 1u, depth + 1); return; }
        t.code.push_back(depth ? code << (32 - depth) : 0u);
        t.keylen.push_back(dsd_keylen(hs_key(s[pos + 8], s[pos + 9], s[pos + 10]), depth));
        t.max_len = std::max(t.max_len, depth);
        pos += kHufSmallLeafSym;
    };
    rec(0, 0);
    t.pay = pos;
    return t;
}
// bit by bit along the serialised trie: n pixels' bytes; false where the bits run out before the n-th
static bool walk_decode(const std::vector<uint8_t> &s, size_t end, uint32_t n, std::vector<uint8_t> &img) {
    const Table t = table_of(s);
    uint64_t bp = (uint64_t)t.pay * 8;
    img.clear();
    for (uint32_t i = 0; i < n; i++) {
        size_t pos = 8;
        while (s[pos] == 1) {
            if (bp >= (uint64_t)end * 8) return false;
            const int bit = (s[bp >> 3] >> (7 - (bp & 7))) & 1;
            bp++;
            pos++;   // the left child follows its parent; the right one lies behind the left subtree
            if (bit) { uint32_t open = 1; while (open) { if (s[pos] == 1) { open++; pos++; } else { open--; pos += 1 + kHufSmallLeafSym; } } }
        }
        img.insert(img.end(), {s[pos + 9], s[pos + 10], s[pos + 11]});
    }
    return true;
}
// the kernel's order: stage, first-level table, the larger table, the lanes' passes until they settle, prefix sum, second pass, pixel bytes
static uint32_t lanes_decode(const std::vector<uint8_t> &s, size_t end, uint32_t n, std::vector<uint8_t> &img) {
    const Table t = table_of(s);
    const uint32_t L = (uint32_t)t.code.size();
    std::vector<uint32_t> keys(n, 0xffffffffu);
    img.assign(3 * (size_t)n, 0);
    if (L == 1) std::fill(keys.begin(), keys.end(), dsd_keylen_key(t.keylen[0]));
    else {
        const uint32_t nst = dsd_stage_bytes(n, end - t.pay), b = nst * 8, nw = (nst + 3) / 4;
        std::vector<uint32_t> words(nw + 2, 0u);
        for (uint32_t i = 0; i < nw; i++) {
            uint8_t q[4] = {0, 0, 0, 0};
            for (uint32_t k = 0; k < 4 && 4 * i + k < nst; k++) q[k] = s[t.pay + 4 * i + k];
            words[i] = dsd_be_word(q);
        }
        std::vector<uint32_t> t1((1u << kDsdT1Bits) + 1), t1k(1u << kDsdT1Bits);
        for (uint32_t p = 0; p <= (1u << kDsdT1Bits); p++) dsd_t1_entry(t.code.data(), t.keylen.data(), L, p, t1.data(), t1k.data());
        const uint32_t cap_px = (n + 255) & ~255u;
        uint32_t big_bits = 0;
        while ((2u << big_bits) <= cap_px) big_bits++;
        std::vector<uint32_t> big;
        if (big_bits > kDsdT1Bits && t.max_len > kDsdT1Bits) {
            big.resize(cap_px);
            for (uint32_t p = 0; p < (1u << big_bits); p++) big[p] = dsd_big_entry(t.code.data(), t.keylen.data(), t1.data(), t1k.data(), big_bits, p);
        }
        const uint32_t sub = dsd_sub_bits(b);
        std::vector<uint32_t> start(kDsdLanes), fin(kDsdLanes), count(kDsdLanes);
        auto pass = [&](uint32_t lane, uint32_t *out, uint32_t first) {
            count[lane] = dsd_pass(words.data(), b, t.code.data(), t.keylen.data(), t1.data(), t1k.data(), out || big.empty() ? nullptr : big.data(), big_bits, start[lane],
                                   dsd_bound(lane + 1, sub, b), &fin[lane], out, first, n);
        };
        for (uint32_t lane = 0; lane < kDsdLanes; lane++) { start[lane] = dsd_bound(lane, sub, b); pass(lane, nullptr, 0); }
        for (uint32_t round = 1;; round++) {
            const std::vector<uint32_t> seen = fin;
            bool any = false;
            for (uint32_t lane = 1; lane < kDsdLanes; lane++) any |= seen[lane - 1] != start[lane];
            if (!any) break;
            if (round >= kDsdMaxRounds) return kDsdUnsettled;
            for (uint32_t lane = 1; lane < kDsdLanes; lane++)
                if (seen[lane - 1] != start[lane]) { start[lane] = seen[lane - 1]; pass(lane, nullptr, 0); }
        }
        uint64_t total = 0;
        std::vector<uint32_t> first(kDsdLanes);
        for (uint32_t lane = 0; lane < kDsdLanes; lane++) { first[lane] = (uint32_t)total; total += count[lane]; }
        if (total < n) return kDsdShort;
        for (uint32_t lane = 0; lane < kDsdLanes; lane++)
            if (first[lane] < n) pass(lane, keys.data(), first[lane]);
    }
    for (uint32_t d = 0; d < n; d++) hs_pixel_bytes(keys[d], &img[3 * (size_t)d]);
    return kDsdOk;
}
static void check_decode(const char *what, const std::vector<Px> &px) {
    const std::vector<uint8_t> s = encode_plain((uint32_t)px.size(), 1, px).bytes;
    const uint32_t n = (uint32_t)px.size();
    const size_t pay = table_of(s).pay;
    std::vector<uint8_t> src;
    for (const Px &p : px) src.insert(src.end(), p.begin(), p.end());
    const size_t ends[4] = {s.size(), s.size() > pay ? s.size() - 1 : s.size(), pay + (s.size() - pay) / 2, pay};
    for (int k = 0; k < 4; k++) {
        std::vector<uint8_t> a, b;
        const bool ok = walk_decode(s, ends[k], n, a);
        const uint32_t st = lanes_decode(s, ends[k], n, b);
        if (st != (ok ? kDsdOk : kDsdShort) || (ok && a != b) || (k == 0 && (!ok || a != src))) {
            printf("FAIL decode %s: %u pixels, stream cut to %zu of %zu: status %u, the walk %s\n", what, n, ends[k], s.size(), st, ok ? "decodes" : "fails");
            g_fail = 1;
        }
    }
}

int main() {
    {   // random pixel lists: a few to many distinct colours, skewed and flat, with the ends of every channel
        for (int rep = 0; rep < 60; rep++) {
            const uint32_t n = rep < 4 ? 1 + rnd(8) : 1 + rnd(kHufSmallMaxPx), spread = 1 + rnd(rep % 3 ? 6 : 256);
            std::vector<Px> s(n);
            for (uint32_t i = 0; i < n; i++) {
                s[i] = Px{(uint8_t)rnd(spread), (uint8_t)rnd(spread), (uint8_t)rnd(spread)};
                if (rep & 1) for (int k = 0; k < 3; k++) s[i][k] = (uint8_t)(255 - s[i][k] * (uint32_t)(k + 1) % 256);
            }
            check("random", s);
        }
        check("random", {Px{0, 0, 0}, Px{255, 255, 255}, Px{255, 0, 0}, Px{0, 0, 255}, Px{0, 255, 0}, Px{255, 255, 255}, Px{0, 0, 255}});
        printf("ok random: 61 lists\n");
    }
    {
        const Encoded e = check("all_ones", pixels_of(std::vector<uint32_t>(kHufSmallMaxPx, 1)), 128, 128);
        check("all_ones", pixels_of(std::vector<uint32_t>(kHufSmallMaxPx - 4, 1)));
        check("all_ones", pixels_of(std::vector<uint32_t>(12345, 1)));
        printf("ok all_ones: %u leaves, every code %u bits, %zu bytes\n", kHufSmallMaxPx, e.longest, e.bytes.size());
        if (e.longest != 14 || e.bytes.size() != 241671) { printf("FAIL all_ones: 16384 equal leaves make a complete tree of depth 14 and 241671 bytes\n"); g_fail = 1; }
    }
    {
        std::vector<uint32_t> c = {1};
        for (uint32_t v = 1; v <= 4096; v <<= 1) c.push_back(v);
        const std::vector<Px> s = pixels_of(c);
        const Encoded e = check("powers", s, 128, 64);
        printf("ok powers: %zu leaves, %zu pixels, longest code %u, %zu bytes\n", c.size(), s.size(), e.longest, e.bytes.size());
        if (c.size() != 14 || s.size() != 8192 || e.longest != 13 || e.bytes.size() != 2237) { printf("FAIL powers: expected 14 leaves, 8192 pixels, 13 bits, 2237 bytes\n"); g_fail = 1; }
    }
    {   // the chain that meets the bound under "a leaf before a branch": every branch strictly lighter than the leaf after next
        std::vector<uint32_t> ch = {1, 1, 1};
        std::vector<uint32_t> br = {2, 3};   // branch k = branch k - 1 + branch k - 2 + 1
        uint32_t ctot = 3, next = 0;
        for (;;) {
            next = br[br.size() - 2] + 1;
            if (ctot + next > kHufSmallMaxPx) break;
            ch.push_back(next); ctot += next;
            br.push_back(br[br.size() - 1] + br[br.size() - 2] + 1);
        }
        const Encoded e = check("chain", pixels_of(ch), 6, 2521);
        printf("ok chain: %zu leaves, %u pixels, longest code %u (the bound: %u), %zu bytes; a 21st count makes %u pixels\n", ch.size(), ctot, e.longest, kDeltaSmallMaxCodeLen,
               e.bytes.size(), ctot + next);
        if (e.longest != kDeltaSmallMaxCodeLen || ch.size() != 20 || ctot != 15126 || e.bytes.size() != 5215 || ctot + next != 24475) { printf("FAIL chain: the strict chain does not meet the bound as claimed\n"); g_fail = 1; }
        // F(22) > 16384: no total count within the route carries a code of 20 bits
        uint64_t f1 = 1, f2 = 1;
        for (int i = 3; i <= 22; i++) { const uint64_t f = f1 + f2; f1 = f2; f2 = f; }
        if (!(f1 <= kHufSmallMaxPx && f2 > kHufSmallMaxPx)) { printf("FAIL chain: F(21) = %llu, F(22) = %llu against %u\n", (unsigned long long)f1, (unsigned long long)f2, kHufSmallMaxPx); g_fail = 1; }
    }
    {
        const Encoded a = check("one", std::vector<Px>(600, Px{77, 78, 79}), 20, 30);
        const Encoded b = check("one", std::vector<Px>(1, Px{255, 0, 1}));
        check("one", std::vector<Px>(kHufSmallMaxPx, Px{0, 0, 0}));
        printf("ok one: %zu bytes, no payload\n", a.bytes.size());
        if (a.bytes.size() != 20 || b.bytes.size() != 20) { printf("FAIL one: expected 20 bytes\n"); g_fail = 1; }
    }
    {
        check("two", pixels_of({1, 1}));
        check("two", pixels_of({1, 599}));
        check("two", pixels_of({8192, 8192}));
        check("two", pixels_of({3, 2}, false));
        printf("ok two\n");
    }
    {   // runs of 2^k - 1 / 2^k / 2^k + 1 equal counts: where a run of pairs ends inside, at and just behind a wave's 64 lanes and a power of two
        int cases = 0;
        for (uint32_t k = 1; k <= 12; k++)
            for (int d = -1; d <= 1; d++) {
                const uint32_t m = (1u << k) + d;
                if (m < 1) continue;
                for (uint32_t cnt = 1; cnt <= 3; cnt++) {
                    if (m * cnt > kHufSmallMaxPx) continue;
                    check("runs", pixels_of(std::vector<uint32_t>(m, cnt)));
                    std::vector<uint32_t> c(m, cnt);   // ... followed by a second run and a heavy leaf
                    const uint32_t m2 = (1u << (k > 1 ? k - 1 : 1)) - d;
                    for (uint32_t i = 0; i < m2; i++) c.push_back(2 * cnt);
                    c.push_back(cnt * m / 2 + 1);
                    uint64_t tot = 0;
                    for (uint32_t v : c) tot += v;
                    if (tot <= kHufSmallMaxPx) { check("runs", pixels_of(c)); cases++; }
                    cases++;
                }
            }
        printf("ok runs: %d lists\n", cases);
    }
    {   // four equally frequent colours whose order differs between r-major and b-major keys: the leaves lie in the trie by (r, g, b)
        const Px cols[4] = {Px{1, 0, 0}, Px{0, 0, 2}, Px{0, 3, 0}, Px{0, 0, 1}};
        std::vector<Px> s;
        for (int rep = 0; rep < 5; rep++) for (const Px &c : cols) s.push_back(c);
        const Encoded e = check("byte_order", s, 5, 4);
        const Px want[4] = {Px{0, 0, 1}, Px{0, 0, 2}, Px{0, 3, 0}, Px{1, 0, 0}};   // pre-order: 1 1 L L 1 L L
        const size_t at[4] = {8 + 2, 8 + 2 + 12, 8 + 3 + 24, 8 + 3 + 36};
        bool ok = e.bytes.size() == 8 + 13 * 4 - 1 + 5;
        for (int i = 0; ok && i < 4; i++) ok = e.bytes[at[i]] == 0 && e.bytes[at[i] + 1] == 3 && !memcmp(&e.bytes[at[i] + 9], want[i].data(), 3);
        if (!ok) { printf("FAIL byte_order: the leaves are not in (r, g, b) order\n"); g_fail = 1; }
        printf("ok byte_order: %zu bytes\n", e.bytes.size());
    }
    {   // the decode lane on whole and cut streams
        for (int rep = 0; rep < 12; rep++) {
            const uint32_t n = rep < 3 ? 1 + rnd(8) : 1 + rnd(kHufSmallMaxPx), spread = 1 + rnd(rep % 3 ? 6 : 256);
            std::vector<Px> s(n);
            for (uint32_t i = 0; i < n; i++) s[i] = Px{(uint8_t)rnd(spread), (uint8_t)(255 - rnd(spread)), (uint8_t)rnd(spread)};
            check_decode("random", s);
        }
        check_decode("all_ones", pixels_of(std::vector<uint32_t>(kHufSmallMaxPx, 1)));
        check_decode("chain", pixels_of({1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207, 3571, 5778}));
        check_decode("one", std::vector<Px>(600, Px{77, 78, 79}));
        check_decode("two", pixels_of({1, 599}));
        check_decode("ends", {Px{0, 0, 0}, Px{255, 255, 255}, Px{255, 0, 0}, Px{0, 0, 255}, Px{1, 0, 0}, Px{0, 0, 1}, Px{0, 0, 0}});
        printf("ok decode: the lanes against the bit-by-bit walk, whole and cut streams\n");
    }
    printf("ok total: longest code met %u, bound %u, stride at the bound %llu\n", g_longest, kDeltaSmallMaxCodeLen, (unsigned long long)hs_stride(kHufSmallMaxPx));
    if (g_longest != kDeltaSmallMaxCodeLen || hs_stride(kHufSmallMaxPx) != 251920) { printf("FAIL total: the bound was not met or the stride is not 251920\n"); g_fail = 1; }
    return g_fail;
}
