// rle_small_check.cpp -- what the small-frame `hilbert(rle)` / `hilbert(rle(d))` kernel computes per frame (cniic_amd/csrc/rle_small.hpp),
// checked on the host.  A scalar encoder built from the header's functions in the kernel's phases -- L(i) of every start first (rs_run_len
// against T(d)), then the chain in pieces of kRleSmallPiece positions (the doubled pointers, the entries carried from piece to piece, the
// marks from every piece's entry), then the records (rs_round, rs_record_words) -- runs beside a plain one-pass restatement of AbstractRle /
// Approx / RunningAvg with a real sqrt and f64 sums, on pixel lists in scan order.
// Build: c++ -O2 -std=c++17 -I cniic_amd/csrc tests/rle_small_check.cpp.  Prints "ok <part>: ..." per part; exit status 1 on a mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rle_small.hpp"

using namespace cniic;

static int g_fail = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % n);
}
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

typedef std::vector<uint32_t> Keys;   // r << 16 | g << 8 | b along the scan

// ---- the kernel's way, scalar, from the header's functions
static std::vector<uint8_t> encode_header(uint32_t w, uint32_t h, const Keys &key, double d, uint32_t *runs_out) {
    const uint32_t n = (uint32_t)key.size();
    const double T = rla_threshold_of(d);
    const int mode = rs_mode(d, T);
    const uint32_t npieces = (n + kRleSmallPiece - 1) / kRleSmallPiece, ncov = npieces * kRleSmallPiece;
    // b. every start's length
    std::vector<uint8_t> len(ncov), mark(ncov, 0);
    std::vector<uint16_t> nx(ncov);
    for (uint32_t i = 0; i < ncov; i++) {
        const uint32_t l = i < n ? rs_run_len(key.data(), i, n, T, mode) : 1u;
        CHECK(l >= 1 && l <= kRleSmallMaxRun && (i >= n || l <= n - i), "L(%u) = %u", i, l);
        len[i] = (uint8_t)l;
        nx[i] = (uint16_t)((i & (kRleSmallPiece - 1)) + l);
    }
    // c. doubling, entries, marks
    for (int r = 0; r < 8; r++) {
        std::vector<uint16_t> next(nx);
        for (uint32_t i = 0; i < ncov; i++)
            if (nx[i] < kRleSmallPiece) next[i] = nx[(i & ~(kRleSmallPiece - 1)) + nx[i]];
        nx.swap(next);
    }
    std::vector<uint8_t> ent(npieces);
    uint32_t e = 0;
    for (uint32_t k = 0; k < npieces; k++) {
        ent[k] = (uint8_t)e;
        const uint32_t out = nx[k * kRleSmallPiece + e];
        CHECK(out >= kRleSmallPiece && out - kRleSmallPiece < kRleSmallMaxRun, "piece %u leaves at %u", k, out);
        e = out - kRleSmallPiece;
    }
    for (uint32_t k = 0; k < npieces; k++) {
        const uint32_t base = k * kRleSmallPiece;
        uint32_t steps = 0;
        for (uint32_t p = ent[k]; p < kRleSmallPiece && base + p < n; p += len[base + p], steps++) mark[base + p] = 1;
        CHECK(steps <= kRleSmallPiece, "piece %u: %u steps", k, steps);
    }
    // d, e. records
    std::vector<uint32_t> words{w, h};
    uint32_t runs = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!mark[i]) continue;
        const uint32_t cnt = len[i];
        uint32_t c0, c1, c2;
        if (mode == kRsModeExact) { c0 = (key[i] >> 16) & 255u; c1 = (key[i] >> 8) & 255u; c2 = key[i] & 255u; }
        else {
            uint32_t s0 = 0, s1 = 0, s2 = 0;
            for (uint32_t j = 0; j < cnt; j++) { s0 += (key[i + j] >> 16) & 255u; s1 += (key[i + j] >> 8) & 255u; s2 += key[i + j] & 255u; }
            c0 = rs_round(s0, cnt); c1 = rs_round(s1, cnt); c2 = rs_round(s2, cnt);
        }
        uint32_t wd[3];
        rs_record_words(cnt, c0, c1, c2, wd);
        words.insert(words.end(), wd, wd + 3);
        runs++;
    }
    CHECK(rs_stream_bytes(runs) == words.size() * 4 && rs_stream_bytes(runs) <= rs_stride(n), "%u runs, %zu words", runs, words.size());
    std::vector<uint8_t> out(words.size() * 4);
    for (size_t i = 0; i < words.size(); i++)
        for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(words[i] >> (8 * b));   // little-endian words
    *runs_out = runs;
    return out;
}

// ---- the plain restatement: one pass, f64 sums, a real square root (hilbertc.rs:118-155, :200-299)
static void put_u32(std::vector<uint8_t> &o, uint32_t v) { for (int b = 0; b < 4; b++) o.push_back((uint8_t)(v >> (8 * b))); }
static std::vector<uint8_t> encode_plain(uint32_t w, uint32_t h, const Keys &key, double d, uint32_t *runs_out) {
    std::vector<uint8_t> o;
    put_u32(o, w); put_u32(o, h);
    const size_t n = key.size();
    const bool exact = d == 0.0;
    uint32_t runs = 0;
    size_t i = 0;
    while (i < n) {
        const double f[3] = {(double)((key[i] >> 16) & 255u), (double)((key[i] >> 8) & 255u), (double)(key[i] & 255u)};
        double sum[3] = {f[0], f[1], f[2]};
        uint32_t count = 1;
        size_t j = i + 1;
        while (j < n) {
            const double x[3] = {(double)((key[j] >> 16) & 255u), (double)((key[j] >> 8) & 255u), (double)(key[j] & 255u)};
            bool accept;
            if (exact) accept = key[j] == key[i];
            else {
                volatile double a0 = sum[0] / count - x[0], a1 = sum[1] / count - x[1], a2 = sum[2] / count - x[2];
                volatile double q0 = a0 * a0, q1 = a1 * a1, q2 = a2 * a2;   // (volatile: every product and sum rounded on its own)
                volatile double s01 = 0.0 + q0;
                volatile double s012 = s01 + q1;
                volatile double s = s012 + q2;
                accept = std::sqrt(s) <= d;
            }
            if (!accept) break;
            sum[0] += x[0]; sum[1] += x[1]; sum[2] += x[2];
            count++; j++;
            if (count == 255) break;
        }
        o.push_back((uint8_t)count);
        o.push_back(3);
        for (int b = 0; b < 7; b++) o.push_back(0);
        for (int c = 0; c < 3; c++) o.push_back((uint8_t)std::round((exact ? f[c] * count : sum[c]) / count));
        runs++;
        i = j;
    }
    *runs_out = runs;
    return o;
}

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static std::vector<double> d_values() {
    return {0.0, -0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 0.5, std::sqrt(2.0), std::sqrt(3.0), 1e-9, 441.7, kInf, -1.0, kNan};
}

static uint32_t both(const char *what, uint32_t w, uint32_t h, const Keys &key, double d) {
    uint32_t r1 = 0, r2 = 0;
    const std::vector<uint8_t> a = encode_header(w, h, key, d, &r1), b = encode_plain(w, h, key, d, &r2);
    CHECK(a == b && r1 == r2, "%s, %u x %u, d = %g: %u runs / %zu bytes against %u / %zu", what, w, h, d, r1, a.size(), r2, b.size());
    return r1;
}

static Keys flat(uint32_t n, uint32_t k) { return Keys(n, k); }
static Keys noise(uint32_t n, uint32_t levels) {
    Keys v(n);
    for (auto &k : v) k = rs_key((uint8_t)(rnd(levels) * (255 / (levels - 1))), (uint8_t)(rnd(levels) * (255 / (levels - 1))), (uint8_t)(rnd(levels) * (255 / (levels - 1))));
    return v;
}
static Keys walk(uint32_t n, uint32_t step) {   // photo-like: a random walk per channel
    Keys v(n);
    int c[3] = {128, 90, 200};
    for (auto &k : v) {
        for (int &x : c) { x += (int)rnd(2 * step + 1) - (int)step; x = x < 0 ? 0 : x > 255 ? 255 : x; }
        k = rs_key((uint8_t)c[0], (uint8_t)c[1], (uint8_t)c[2]);
    }
    return v;
}

int main() {
    const std::vector<double> ds = d_values();
    // ---- random pixel lists of many lengths, every d
    {
        uint32_t cases = 0;
        const uint32_t lens[] = {1, 2, 3, 254, 255, 256, 257, 510, 511, 512, 513, 1023, 1024, 1025, 4095, 16383, 16384};
        for (uint32_t n : lens)
            for (double d : ds) {
                both("noise", n, 1, noise(n, 256), d);
                both("coarse noise", n, 1, noise(n, 2), d);
                both("walk", 1, n, walk(n, 3), d);
                cases += 3;
            }
        printf("ok random: %u lists\n", cases);
    }
    // ---- the content kinds
    {
        const uint32_t n = kRleSmallMaxPx;
        for (double d : ds) {
            const uint32_t runs = both("flat", n, 1, flat(n, 0x5d29c8), d);
            const bool none = !(d >= 0.0);
            CHECK(runs == (none ? n : 65u), "flat 16384 at d = %g: %u runs", d, runs);
        }
        uint32_t r = 0;
        std::vector<uint8_t> s = encode_header(kRleSmallMaxPx, 1, flat(kRleSmallMaxPx, 7), 4.0, &r);
        CHECK(s[8 + 12 * 63] == 255 && s[8 + 12 * 64] == 64, "the cap's phase");
        // one odd pixel at the piece borders and the run offsets
        uint32_t cases = 0;
        for (uint32_t at : {0u, 1u, 253u, 254u, 255u, 256u, 257u, 509u, 510u, 511u, 512u, 513u, 767u, 768u, 769u, 1023u, 1024u, 1025u, 16383u})
            for (double d : ds) {
                Keys v = flat(n, 0x101010);
                v[at] = 0xf0f0f0;
                both("odd pixel", n, 1, v, d);
                v[at] = 0x101011;   // at distance 1: joins the run from d = 1 on
                both("near pixel", n, 1, v, d);
                cases += 2;
            }
        // two colours alternating; the ramp 0, 1, 0, 1: averages on exact halves round away from zero; the ends of the channels
        for (double d : ds) {
            Keys alt(4099), ramp(4099), ends(4099);
            for (uint32_t i = 0; i < 4099; i++) { alt[i] = i & 1 ? 0x0a141e : 0x283c5a; ramp[i] = i & 1 ? 0x010101 : 0; ends[i] = (i / 3) & 1 ? 0xffffff : 0; }
            both("alternating", 4099, 1, alt, d);
            const uint32_t runs = both("ramp", 4099, 1, ramp, d);
            if (d == 1.0) CHECK(runs == 4099, "the ramp at d = 1: %u runs", runs);   // the first step is sqrt 3 away
            if (d == 2.0) CHECK(runs == 17, "the ramp at d = 2: %u runs", runs);     // 16 runs of 255 and one of 19
            both("ends", 4099, 1, ends, d);
            cases += 3;
        }
        {
            Keys ramp(254);
            for (uint32_t i = 0; i < 254; i++) ramp[i] = i & 1 ? 0x010101 : 0;
            uint32_t runs = 0;
            s = encode_header(254, 1, ramp, 2.0, &runs);
            CHECK(runs == 1 && s[8] == 254 && s[17] == 1 && s[18] == 1 && s[19] == 1, "127 / 254 rounds to 1, not to 0");
        }
        printf("ok contents: %u lists, flat 16384 = 64 runs of 255 and one of 64\n", cases);
    }
    // ---- T(d) against sqrt around the exact distances of small integer triples, and a sweep of d over them
    {
        uint32_t dists = 0, sweeps = 0;
        std::vector<double> exact;
        for (int a = 0; a <= 6; a++)
            for (int b = a; b <= 6; b++)
                for (int c = b; c <= 6; c++) {
                    if (!(a | b | c)) continue;
                    const double s = (double)(a * a + b * b + c * c), d0 = std::sqrt(s);
                    exact.push_back(d0);
                    for (double d : {std::nextafter(d0, 0.0), d0, std::nextafter(d0, kInf)}) {
                        const double T = rla_threshold_of(d);
                        CHECK(std::sqrt(T) <= d && std::sqrt(std::nextafter(T, kInf)) > d, "T(%a) = %a", d, T);
                        CHECK((std::sqrt(s) <= d) == (s <= T), "distance^2 %g against d = %a", s, d);
                        dists++;
                    }
                }
        CHECK(rla_threshold_of(-1.0) == -1.0 && rla_threshold_of(kNan) == -1.0 && rla_threshold_of(kInf) == kInf && rla_threshold_of(0.0) == 0.0, "the edges of T");
        CHECK(rla_mode(-1.0) == kRlaModeNone && rla_mode(kInf) == kRlaModeAll && rla_mode(rla_threshold_of(441.7)) == kRlaModeAll && rla_mode(rla_threshold_of(441.6)) == kRlaModeTest
              && rs_mode(-0.0, 0.0) == kRsModeExact && rs_mode(1e-9, rla_threshold_of(1e-9)) == kRlaModeTest, "the modes");
        const Keys small = noise(2049, 7);   // channel steps of 42: not those distances; the walk below hits them
        Keys near(2049);
        { int c[3] = {3, 3, 3}; for (auto &k : near) { for (int &x : c) { x += (int)rnd(5) - 2; x = x < 0 ? 0 : x > 12 ? 12 : x; } k = rs_key((uint8_t)c[0], (uint8_t)c[1], (uint8_t)c[2]); } }
        for (double d0 : exact)
            for (double d : {std::nextafter(d0, 0.0), d0, std::nextafter(d0, kInf)}) { both("sweep", 2049, 1, near, d); both("sweep", 2049, 1, small, d); sweeps += 2; }
        printf("ok threshold: %u distances against sqrt, %u swept lists\n", dists, sweeps);
    }
    // ---- the rounding against f64::round(sum / count)
    {
        uint64_t pairs = 0;
        for (uint32_t count = 1; count <= 255; count++)
            for (uint32_t sum = 0; sum <= 255 * count; sum++, pairs++)
                if (rs_round(sum, count) != (uint32_t)std::round((double)sum / (double)count)) { CHECK(false, "round(%u / %u)", sum, count); break; }
        printf("ok rounding: %llu (sum, count) pairs\n", (unsigned long long)pairs);
    }
    // ---- sizes
    CHECK(rs_stride(kRleSmallMaxPx) == 196624 && rs_stride(1) == 32 && rs_stream_bytes(1) == 20 && rs_cap(0, 1) == 1 && rs_cap(16384 - 255, 16384) == 255 && rs_cap(16384 - 254, 16384) == 254, "sizes");
    printf("ok total: bound %u pixels, stride at the bound %llu, piece %u, %d mismatches\n", kRleSmallMaxPx, (unsigned long long)rs_stride(kRleSmallMaxPx), kRleSmallPiece, g_fail);
    return g_fail ? 1 : 0;
}
