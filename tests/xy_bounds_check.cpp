// xy_bounds_check.cpp -- a stand-alone check of cniic_amd/csrc/xy_bounds.hpp, the integer arithmetic of the tiled 5-D K-means
// (tests/test_xyrgb_arith_cpu.py compiles and runs it, once more under -fsanitize=address,undefined).  Nothing here comes from the
// library but the header under test; on the host its 24-bit multiply returns what v_mul_i32_i24 returns.
//
//   div_floor    xy_div_floor(q m + r, m, 1.0f / m) == q against 64-bit division, for every sum the kernel can form (sum < 2^42, quotient
//                < 2^14, m <= 2^28), with the reciprocal as computed and nudged one ulp either way.  The raw single-precision estimate must
//                be within one of the floor as computed and within two when nudged, and must be off by one in BOTH directions somewhere:
//                the correction steps, not luck, give the floor.
//   worst        Dominance::worst == the 64-bit maximum over the 32 corners of the box of d(corner, pivot) - d(corner, centroid); no
//                operand leaves 24 bits, no product or partial sum leaves int32; and where worst < 0 the pivot is STRICTLY nearer than
//                the centroid at every corner (squared distances computed directly).
//   centre_dist  == the 64-bit squared distance from the box centre, below 2^31.
// Exit status 0 and a line "ok ..." per part; the first violation is printed after "FAIL" and the status is 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../cniic_amd/csrc/xy_bounds.hpp"

using namespace cniic;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static const int32_t kMaxXY = 16383;

// ------------------------------------------------------------------ xy_div_floor
static int check_div_floor() {
    const uint32_t ms[] = {1u, 2u, 3u, 255u, 257u, 65537u, 104729u, 1000003u, 15485863u, (1u << 24) - 1u, 1u << 24, (1u << 24) + 1u,
                           179424673u, (1u << 28) - 1u, 1u << 28};
    std::vector<uint32_t> qs = {0u, 1u, 2u, 8191u, 8192u, 16382u, 16383u};
    for (int i = 0; i < 4000; i++) qs.push_back(rnd() % 16384u);
    uint64_t cases = 0;
    long long off[3][5] = {{0}};   // [nudge][q - estimate + 2]
    for (uint32_t m : ms) {
        const float rm0 = 1.0f / (float)m;
        const float rms[3] = {rm0, nextafterf(rm0, 0.0f), nextafterf(rm0, 2.0f)};
        const uint64_t rs[5] = {0u, 1u, m / 2u, (uint64_t)m >= 2u ? m - 2u : 0u, m - 1u};
        for (uint32_t q : qs)
            for (uint64_t r : rs) {
                if (r >= m) continue;
                const unsigned long long sum = (unsigned long long)q * m + r;
                if (sum >= (1ull << 42) || sum / m != q) { printf("FAIL div_floor: the case itself is out of range (q=%u m=%u)\n", q, m); return 1; }
                for (int n = 0; n < 3; n++) {
                    const uint32_t got = xy_div_floor(sum, m, rms[n]);
                    if (got != q) { printf("FAIL div_floor: sum=%llu m=%u nudge=%d: got %u, floor is %u\n", sum, m, n, got, q); return 1; }
                    const long long est = (long long)(uint32_t)((float)sum * rms[n]), d = (long long)q - est;
                    const long long lim = n == 0 ? 1 : 2;
                    if (d < -lim || d > lim) { printf("FAIL div_floor: sum=%llu m=%u nudge=%d: estimate %lld is %lld from the floor\n", sum, m, n, est, d); return 1; }
                    off[n][d + 2]++;
                    cases++;
                }
            }
    }
    long long up = 0, down = 0;
    for (int n = 0; n < 3; n++) { up += off[n][3] + off[n][4]; down += off[n][0] + off[n][1]; }
    if (!up || !down) { printf("FAIL div_floor: the estimate was never off %s: the correction steps were not exercised\n", up ? "downwards" : "upwards"); return 1; }
    printf("ok div_floor: %llu cases; floor - estimate in -2..2:", (unsigned long long)cases);
    const char *nm[3] = {"as computed", "rm - 1 ulp", "rm + 1 ulp"};
    for (int n = 0; n < 3; n++) printf(" [%s: %lld %lld %lld %lld %lld]", nm[n], off[n][0], off[n][1], off[n][2], off[n][3], off[n][4]);
    printf("\n");
    return 0;
}

// ------------------------------------------------------------------ Dominance::worst, centre_dist
static int32_t draw(bool xy) {
    const uint32_t t = rnd() % 8u;
    const int32_t top = xy ? kMaxXY : 255;
    switch (t) {
    case 0: return 0;
    case 1: return 1;
    case 2: return top - 1;
    case 3: return top;
    default: return (int32_t)(rnd() % (uint32_t)(top + 1));
    }
}
static bool fits24(int64_t v) { return v >= -(1 << 23) && v < (1 << 23); }
static bool fits32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

struct Case { Box5 b; int32_t p[5], v[5]; };

static int check_case(const Case &c, int64_t &max_abs, uint64_t &dominated) {
    const xy_int4 pv = {c.p[0], c.p[1], (c.p[2] << 16) | (c.p[3] << 8) | c.p[4], 0};
    const xy_int4 cv = {c.v[0], c.v[1], (c.v[2] << 16) | (c.v[3] << 8) | c.v[4], 0};
    Dominance dm;
    dm.set(c.b, pv);
    const int32_t got = dm.worst(cv);
    // the operands and products of the header's own evaluation, in 64 bits
    int64_t part = 0;
    for (int i = 0; i < 5; i++) {
        const int64_t d = (int64_t)c.p[i] - c.v[i];
        const int64_t s0 = (int64_t)c.v[i] + c.p[i] - 2 * (int64_t)c.b.lo[i], s1 = (int64_t)c.v[i] + c.p[i] - 2 * (int64_t)c.b.hi[i];
        if (!fits24(d) || !fits24(s0) || !fits24(s1)) { printf("FAIL worst: an operand of dimension %d leaves 24 bits\n", i); return 1; }
        if (!fits32(d * s0) || !fits32(d * s1)) { printf("FAIL worst: a product of dimension %d leaves int32\n", i); return 1; }
        if (xy_mul24((int32_t)d, (int32_t)s0) != d * s0 || xy_mul24((int32_t)d, (int32_t)s1) != d * s1) { printf("FAIL worst: the 24-bit multiply changed a product of dimension %d\n", i); return 1; }
        part += d * s0 > d * s1 ? d * s0 : d * s1;
        if (!fits32(part)) { printf("FAIL worst: the partial sum after dimension %d leaves int32\n", i); return 1; }
    }
    // the definition: the maximum over the corners of d(corner, pivot) - d(corner, centroid), squared distances computed directly
    int64_t mx = INT64_MIN;
    bool strictly = true;
    for (uint32_t corner = 0; corner < 32; corner++) {
        int64_t dp = 0, dc = 0;
        for (int i = 0; i < 5; i++) {
            const int64_t x = ((corner >> i) & 1u) ? c.b.hi[i] : c.b.lo[i];
            dp += (x - c.p[i]) * (x - c.p[i]);
            dc += (x - c.v[i]) * (x - c.v[i]);
        }
        if (dp - dc > mx) mx = dp - dc;
        if (!(dp < dc)) strictly = false;
    }
    if ((int64_t)got != mx) { printf("FAIL worst: got %d, the maximum over the corners is %lld\n", got, (long long)mx); return 1; }
    if (got < 0) {
        dominated++;
        if (!strictly) { printf("FAIL worst: %d < 0 but the pivot is not strictly nearer at every corner\n", got); return 1; }
    }
    if (mx > max_abs) max_abs = mx;
    if (-mx > max_abs) max_abs = -mx;
    // centre_dist of both points
    for (int which = 0; which < 2; which++) {
        const int32_t *pt = which ? c.v : c.p;
        int64_t want = 0;
        for (int i = 0; i < 5; i++) { const int64_t e = (int64_t)pt[i] - ((c.b.lo[i] + c.b.hi[i]) >> 1); want += e * e; }
        const uint32_t g = centre_dist(c.b, which ? cv : pv);
        if (want >= (1ll << 31) || (int64_t)g != want) { printf("FAIL centre_dist: got %u, want %lld\n", g, (long long)want); return 1; }
    }
    return 0;
}

static void print_case(const Case &c) {
    printf("  box lo (%d %d %d %d %d) hi (%d %d %d %d %d) pivot (%d %d %d %d %d) centroid (%d %d %d %d %d)\n", c.b.lo[0], c.b.lo[1], c.b.lo[2], c.b.lo[3],
           c.b.lo[4], c.b.hi[0], c.b.hi[1], c.b.hi[2], c.b.hi[3], c.b.hi[4], c.p[0], c.p[1], c.p[2], c.p[3], c.p[4], c.v[0], c.v[1], c.v[2], c.v[3], c.v[4]);
}

static int check_worst() {
    int64_t max_abs = 0;
    uint64_t cases = 0, dominated = 0;
    // the corners of the domain: box, pivot and centroid each at 0 or at the largest value of every dimension
    for (uint32_t bits = 0; bits < 16; bits++) {
        Case c;
        if ((bits & 1u) && !(bits & 2u)) continue;   // lo <= hi
        for (int i = 0; i < 5; i++) {
            const int32_t top = i < 2 ? kMaxXY : 255;
            c.b.lo[i] = (bits & 1u) ? top : 0; c.b.hi[i] = (bits & 2u) ? top : 0;
            c.p[i] = (bits & 4u) ? top : 0; c.v[i] = (bits & 8u) ? top : 0;
        }
        if (check_case(c, max_abs, dominated)) { print_case(c); return 1; }
        cases++;
    }
    for (uint32_t n = 0; n < 1000000u; n++) {
        Case c;
        for (int i = 0; i < 5; i++) {
            const int32_t a = draw(i < 2), b = draw(i < 2);
            c.b.lo[i] = a < b ? a : b; c.b.hi[i] = a < b ? b : a;
            c.p[i] = draw(i < 2); c.v[i] = draw(i < 2);
        }
        if (n & 1u) {   // half of the cases: a tile-sized box with pivot and centroid near it, where worst changes sign
            for (int i = 0; i < 2; i++) {
                const int32_t side = i == 0 ? 64 : 16;
                c.b.hi[i] = c.b.lo[i] + (int32_t)(rnd() % (uint32_t)side);
                if (c.b.hi[i] > kMaxXY) c.b.hi[i] = kMaxXY;
                for (int32_t *q : {&c.p[i], &c.v[i]}) {
                    int32_t x = c.b.lo[i] + (int32_t)(rnd() % 257u) - 128;
                    *q = x < 0 ? 0 : x > kMaxXY ? kMaxXY : x;
                }
            }
        }
        if (check_case(c, max_abs, dominated)) { print_case(c); return 1; }
        cases++;
    }
    if (dominated < cases / 20 || dominated > cases - cases / 20) { printf("FAIL worst: %llu of %llu cases dominated: one verdict is hardly tried\n", (unsigned long long)dominated, (unsigned long long)cases); return 1; }
    printf("ok worst: %llu cases, %llu dominated, largest |worst| %lld (2^31 = 2147483648)\n", (unsigned long long)cases, (unsigned long long)dominated, (long long)max_abs);
    printf("ok centre_dist: %llu cases\n", (unsigned long long)(2 * cases));
    return 0;
}

// the host's 24-bit multiply is the instruction's: sign-extended low 24 bits, low 32 bits of the product
static int check_mul24() {
    const int32_t a[] = {0, 1, -1, 0x7fffff, -0x800000, 0x800000, 0x1000000, 0x1000001, -0x800001, INT32_MAX, INT32_MIN, 16383, -32766};
    for (int32_t x : a)
        for (int32_t y : a) {
            const int64_t xs = (int64_t)((x & 0xffffff) ^ 0x800000) - 0x800000, ys = (int64_t)((y & 0xffffff) ^ 0x800000) - 0x800000;
            const int32_t want = (int32_t)(uint32_t)((uint64_t)(xs * ys) & 0xffffffffull);
            if (xy_mul24(x, y) != want) { printf("FAIL mul24: %d * %d: got %d, want %d\n", x, y, xy_mul24(x, y), want); return 1; }
        }
    printf("ok mul24: %zu pairs\n", sizeof(a) / sizeof(a[0]) * (sizeof(a) / sizeof(a[0])));
    return 0;
}

int main() {
    if (check_mul24()) return 1;
    if (check_div_floor()) return 1;
    if (check_worst()) return 1;
    return 0;
}
