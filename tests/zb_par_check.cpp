// zb_par_check.cpp -- the phases of zip(back)'s whole-GPU decode (cniic_amd/csrc/k_zipback_par.hip) as a scalar emulation over the
// functions of cniic_amd/csrc/zb_par.hpp, held against a one-pass decoder that is the contract's loop word for word.  A program of its
// own (tests/test_zip_back_par_cpu.py compiles it plain and with -fsanitize=address,undefined and runs it directly):
//     zb_par_check [STREAMS]      STREAMS: a file of reference streams, each a little-endian u32 length and its bytes
// The emulation visits the positions of every phase `lanes` at a time in a shuffled order (1, 7, 64, 1024 lanes), so that what a phase
// reads while it writes (the marks) is read in any order; tables that a phase reads only from the round before are two tables here too.
// Every buffer has exactly the size the kernels are given: the stream n bytes, the text cap bytes, the tables n + 1 and min(made, cap).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../cniic_amd/csrc/zb_par.hpp"

using namespace cniic;
typedef std::vector<uint8_t> Bytes;

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

struct Verdict { uint32_t status = 0; uint64_t p = 0, made = 0; Bytes out; uint32_t rounds = 0; bool handed = false; uint64_t depth = 0, symbols = 0; };

// the contract: the serial loop of k_zb_decode; out has exactly cap bytes, 0xEE where nothing was written
static Verdict one_pass(const Bytes &in, uint64_t need, uint64_t cap) {
    Verdict v;
    v.out.assign(cap, 0xEE);
    const uint64_t n = in.size();
    std::vector<uint64_t> depth(cap, 0);
    uint64_t sp = 0, o = 0;
    for (;;) {
        if (o >= need || sp + 2 > n) { v.status = kZbpDone; break; }
        const uint32_t head = in[sp] | (in[sp + 1] << 8), len = head & 0x7FFF;
        uint32_t k;
        if (head & 0x8000) {
            if (sp + 4 > n) { v.status = kZbpDone; break; }
            const uint32_t back = in[sp + 2] | (in[sp + 3] << 8);
            if (back > o) { v.status = kZbpBadLookback; break; }
            k = std::min(len, back);
            for (uint32_t t = 0; t < k; t++)
                if (o + t < cap) { v.out[o + t] = v.out[o - back + t]; depth[o + t] = depth[o - back + t] + 1; v.depth = std::max(v.depth, depth[o + t]); }
            sp += 4;
        } else {
            if (sp + 2 + len > n) { v.status = kZbpBadExplicit; break; }
            k = len;
            for (uint32_t t = 0; t < k; t++)
                if (o + t < cap) v.out[o + t] = in[sp + 2 + t];
            sp += 2 + len;
        }
        o += k;
        v.symbols++;
        if (!k) { v.status = kZbpDone; break; }
    }
    v.p = sp;
    v.made = o;
    return v;
}

// positions [0, count) in groups of `lanes`, each group in a shuffled order
template <class F> static void visit(uint64_t count, uint32_t lanes, Rng &rng, F f) {
    std::vector<uint64_t> order(lanes);
    for (uint64_t base = 0; base < count; base += lanes) {
        const uint64_t m = std::min<uint64_t>(lanes, count - base);
        for (uint64_t i = 0; i < m; i++) order[i] = base + i;
        for (uint64_t i = m; i > 1; i--) std::swap(order[i - 1], order[rng.below(i)]);
        for (uint64_t i = 0; i < m; i++) f(order[i]);
    }
}

static Verdict phases(const Bytes &in_v, uint64_t need, uint64_t cap, uint32_t lanes, Rng &rng, uint32_t round_cap) {
    Verdict v;
    v.out.assign(cap, 0xEE);
    const uint64_t n = in_v.size();
    const uint8_t *in = in_v.data();
    // next, chain
    std::vector<uint32_t> jump[2] = {std::vector<uint32_t>(n + 1), std::vector<uint32_t>(n + 1)};
    Bytes mark(n + 1, 0);
    visit(n + 1, lanes, rng, [&](uint64_t p) { jump[0][p] = (uint32_t)zbp_next(in, n, p); mark[p] = p == 0; });
    const uint32_t R = zbp_chain_rounds(n);
    for (uint32_t r = 0; r < R; r++) {
        const std::vector<uint32_t> &from = jump[r & 1];
        std::vector<uint32_t> &to = jump[(r & 1) ^ 1];
        visit(n + 1, lanes, rng, [&](uint64_t p) { const uint32_t j = from[p]; if (mark[p]) mark[j] = 1; to[p] = from[j]; });
    }
    // k, o, the first event
    std::vector<uint64_t> o_at(n + 1, ~0ull);
    uint64_t o = 0, first = n;
    bool found = false;
    for (uint64_t p = 0; p <= n; p++) {
        if (!mark[p]) continue;
        o_at[p] = o;
        if (!found && zbp_event(in, n, need, p, o) != kZbpGo) { first = p; found = true; }
        o += zbp_k(in, n, p);
    }
    if (!found || !mark[n]) { fprintf(stderr, "the chain does not reach the end of the stream\n"); exit(1); }
    v.p = first;
    v.made = o_at[first];
    v.status = zbp_event(in, n, need, first, v.made);
    if (v.status != kZbpDone) return v;
    const uint64_t W = std::min(v.made, cap);
    if (W >= (1ull << 32)) { v.handed = true; return v; }
    // fill
    std::vector<uint32_t> P[2] = {std::vector<uint32_t>(W), std::vector<uint32_t>(W)};
    bool flag = false;
    visit(first, lanes, rng, [&](uint64_t p) {
        if (!mark[p]) return;
        const ZbpHead h = zbp_head(in, n, p);
        const uint64_t at = o_at[p];
        const uint32_t k = at < W ? zbp_k(in, n, p) : 0;
        if (k && h.lookback) flag = true;
        for (uint32_t t = 0; t < k && at + t < W; t++) {
            const ZbpSource s = zbp_source(h, p, at, t);
            if (s.literal) v.out[at + t] = in_v.at(s.at);
            else if (s.at >= at + t) { fprintf(stderr, "a copy that does not point back\n"); exit(1); }
            P[0][at + t] = zbp_pointer(s);
        }
    });
    // jump rounds
    for (uint32_t r = 0;; r++) {
        if (!flag) break;
        if (r >= round_cap || r >= kZbpMaxRounds) { v.handed = true; break; }
        flag = false;
        const std::vector<uint32_t> &from = P[r & 1];
        std::vector<uint32_t> &to = P[(r & 1) ^ 1];
        visit(W, lanes, rng, [&](uint64_t j) {
            uint32_t src;
            const uint32_t q = zbp_jump(from, (uint32_t)j, &src);
            if (src != kZbpNil) v.out[j] = v.out[src];
            to[j] = q;
            if (q != kZbpNil) flag = true;
        });
        v.rounds = r + 1;
    }
    return v;
}

static int failures = 0;
static uint64_t checked = 0;

static void hold(const char *what, const Bytes &in, uint64_t need, uint64_t cap, Rng &rng) {
    const Verdict want = one_pass(in, need, cap);
    static const uint32_t kLanes[4] = {1, 7, 64, 1024};
    for (uint32_t lanes : kLanes) {
        const Verdict got = phases(in, need, cap, lanes, rng, kZbpMaxRounds);
        checked++;
        bool ok = got.status == want.status && got.made == want.made && !got.handed;
        if (want.status != kZbpDone) ok = ok && got.p == want.p;
        else ok = ok && got.out == want.out && got.rounds == zbp_jump_rounds(want.depth);
        if (!ok) {
            failures++;
            fprintf(stderr, "%s (n %zu, need %llu, cap %llu, %u lanes): status %u / %u, p %llu / %llu, made %llu / %llu, rounds %u / %u%s\n", what, in.size(),
                    (unsigned long long)need, (unsigned long long)cap, lanes, got.status, want.status, (unsigned long long)got.p, (unsigned long long)want.p,
                    (unsigned long long)got.made, (unsigned long long)want.made, got.rounds, zbp_jump_rounds(want.depth), got.out == want.out ? "" : ", bytes differ");
            return;
        }
        // the round cap: one below the stream's own rounds hands it back, exactly at them does not
        if (want.status == kZbpDone && got.rounds && lanes == 64) {
            if (!phases(in, need, cap, lanes, rng, got.rounds - 1).handed || phases(in, need, cap, lanes, rng, got.rounds).handed) {
                failures++;
                fprintf(stderr, "%s: the round cap at %u\n", what, got.rounds);
            }
        }
    }
}

static Bytes explicit_sym(const Bytes &data) {
    Bytes s{(uint8_t)(data.size() & 255), (uint8_t)(data.size() >> 8)};
    s.insert(s.end(), data.begin(), data.end());
    return s;
}
static Bytes lookback(uint32_t len, uint32_t back) { return Bytes{(uint8_t)(len & 255), (uint8_t)(0x80 | (len >> 8)), (uint8_t)(back & 255), (uint8_t)(back >> 8)}; }
static Bytes operator+(Bytes a, const Bytes &b) { a.insert(a.end(), b.begin(), b.end()); return a; }
static Bytes counting(size_t n, uint32_t seed) { Bytes b(n); for (size_t i = 0; i < n; i++) b[i] = (uint8_t)(i * 7 + seed + (i >> 8)); return b; }

static void all_caps(const char *what, const Bytes &in, Rng &rng) {
    const Verdict full = one_pass(in, ~0ull, 0);
    const uint64_t T = full.made;
    for (uint64_t cap : {(uint64_t)0, (uint64_t)1, (uint64_t)7, T ? T - 1 : 0, T, T + 5}) hold(what, in, ~0ull, cap, rng);
    for (uint64_t need : {(uint64_t)0, (uint64_t)1, T / 2, T ? T - 1 : 0, T}) hold(what, in, need, T + 1, rng);
}

int main(int argc, char **argv) {
    Rng rng{20261021};
    const Bytes lit = explicit_sym(counting(8, 1));
    // the orders of the contract
    all_caps("empty", Bytes{}, rng);
    all_caps("one byte", Bytes{0x03}, rng);
    all_caps("a literal", lit, rng);
    all_caps("a literal cut short", Bytes(lit.begin(), lit.end() - 1), rng);
    all_caps("an empty literal, then a bad look-back", lit + explicit_sym(Bytes{}) + lookback(4, 60000), rng);
    all_caps("a look-back of no bytes, then a bad look-back", lit + lookback(0, 4) + lookback(4, 60000), rng);
    all_caps("a look-back from nowhere, then a bad look-back", lit + lookback(4, 0) + lookback(4, 60000), rng);
    all_caps("a look-back behind the start", lit + lookback(4, 9) + lit, rng);
    all_caps("back == o", lit + lookback(4, 8), rng);
    all_caps("len > back", lit + lookback(300, 3) + lookback(20, 11), rng);
    all_caps("a header of one byte", lit + Bytes{0x05}, rng);
    for (int cut = 1; cut <= 3; cut++) { Bytes s = lit + lookback(5, 5); s.resize(s.size() - cut); all_caps("a look-back header cut", s, rng); }
    {   // a bad symbol directly behind the one that reaches need is not seen; one symbol earlier it is
        const Bytes s = lit + lookback(8, 8) + lookback(4, 60000);
        hold("need reached before the bad symbol", s, 16, 64, rng);
        hold("need reached before the bad symbol", s, 9, 64, rng);
        hold("need not reached", s, 17, 64, rng);
        const Bytes e = lit + lookback(4, 60000) + lookback(8, 8);
        hold("the bad symbol one earlier", e, 16, 64, rng);
    }
    {   // back == o and back == o + 1 at o = 65535
        Bytes s = explicit_sym(counting(32767, 3)) + explicit_sym(counting(32767, 5)) + explicit_sym(counting(1, 9));
        all_caps("back == o at 65535", s + lookback(100, 65535), rng);
        Bytes t = explicit_sym(counting(32767, 3)) + explicit_sym(counting(32767, 5));   // o = 65534: back 65535 = o + 1
        hold("back == o + 1", t + lookback(100, 65535), ~0ull, 70000, rng);
    }
    // long symbols off the chain (inside a literal) and on it
    {
        Bytes inner = lookback(32767, 65535) + explicit_sym(counting(300, 1));
        inner.resize(200);
        all_caps("symbols inside a literal", explicit_sym(inner) + lookback(50, 100), rng);
        all_caps("an explicit symbol of 32767 bytes", explicit_sym(counting(32767, 2)) + lookback(32767, 32767) + lookback(32767, 1), rng);
    }
    // depth: explicit(8) + N look-backs of (8, 8); look-backs of (11, 65535) across 200 KB
    for (uint32_t N : {1u, 2u, 3u, 4u, 31u, 32u, 33u, 1000u, 70000u}) {
        Bytes s = lit;
        for (uint32_t i = 0; i < N; i++) s = s + lookback(8, 8);
        const Verdict v = one_pass(s, ~0ull, 8 * (N + 1));
        if (v.depth != N || zbp_jump_rounds(N) != (uint32_t)(64 - __builtin_clzll((uint64_t)N))) { failures++; fprintf(stderr, "depth of %u look-backs: %llu\n", N, (unsigned long long)v.depth); }
        hold("a chain of look-backs", s, ~0ull, 8 * (N + 1), rng);
        if (N == 1000) all_caps("a chain of look-backs", s, rng);
    }
    {
        Bytes s = explicit_sym(counting(32767, 3)) + explicit_sym(counting(32767, 5)) + explicit_sym(counting(1, 9));
        for (uint32_t i = 0; i < 12500; i++) s = s + lookback(11, 65535);
        hold("far look-backs across 200 KB", s, ~0ull, 65535 + 11 * 12500, rng);
    }
    // a small stream with a long text, against a small capacity
    {
        Bytes s = explicit_sym(counting(32767, 3));
        for (uint32_t i = 0; i < 40; i++) s = s + lookback(32767, 32767);
        hold("a long text under a small capacity", s, ~0ull, 1000, rng);
    }
    // seeded mutants of the reference's streams
    std::vector<Bytes> refs;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint8_t l[4];
        while (fread(l, 1, 4, f) == 4) {
            Bytes s((size_t)l[0] | ((size_t)l[1] << 8) | ((size_t)l[2] << 16) | ((size_t)l[3] << 24));
            if (!s.empty() && fread(s.data(), 1, s.size(), f) != s.size()) { fprintf(stderr, "%s: cut short\n", argv[1]); return 2; }
            refs.push_back(s);
        }
        fclose(f);
    } else {
        refs.push_back(lit + lookback(8, 8) + explicit_sym(counting(40, 4)) + lookback(30, 20) + lookback(6, 50));
    }
    for (const Bytes &s : refs) all_caps("a reference stream", s, rng);
    for (uint32_t m = 0; m < 4000; m++) {
        Bytes s = refs[m % refs.size()];
        if (s.size() > 6000) s.resize(6000);
        const uint32_t edits = 1 + (uint32_t)rng.below(3);
        for (uint32_t e = 0; e < edits && !s.empty(); e++) {
            const uint64_t at = rng.below(s.size());
            switch (rng.below(4)) {
                case 0: s[at] = (uint8_t)rng.next(); break;
                case 1: s[at] ^= (uint8_t)(1u << rng.below(8)); break;
                case 2: s.resize(at); break;
                default: s.insert(s.begin() + at, (uint8_t)rng.next()); break;
            }
        }
        const Verdict full = one_pass(s, ~0ull, 0);
        const uint64_t cap = rng.below(3) ? full.made + rng.below(4) : rng.below(full.made + 1);
        const uint64_t need = rng.below(2) ? ~0ull : rng.below(full.made + 2);
        hold("a mutant", s, need, cap, rng);
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("zb_par_check ok: %llu emulated decodes\n", (unsigned long long)checked);
    return 0;
}
