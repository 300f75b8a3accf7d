/* rle_approx_ref.c -- CPU restatement of Hilbert { compress: RLE(d) }::encode over an image already in Hilbert order
 * (reference: src/codec/hilbertc.rs:26-45, AbstractRle::next :118-155, Approx :200-238, RunningAvg :240-285, dist :292-299),
 * one run after the other, for the tests' large cases.  Build with -ffp-contract=off: the test's squares and adds must not fuse.
 *
 * rla_encode(lin, n, w, h, d, out): writes the whole stream (w, h as u32, then count:u8 + u64 3 + r g b per run) to out, which has
 * room for 8 + 12 n bytes, and returns its length. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static void put_u32(uint8_t *o, uint32_t v) { for (int k = 0; k < 4; k++) o[k] = (uint8_t)(v >> (8 * k)); }

static uint8_t *put_run(uint8_t *o, uint32_t count, const uint8_t c[3]) {
    o[0] = (uint8_t)count;
    o[1] = 3;
    memset(o + 2, 0, 7);
    memcpy(o + 9, c, 3);
    return o + 12;
}

uint64_t rla_encode(const uint8_t *lin, uint64_t n, uint32_t w, uint32_t h, double d, uint8_t *out) {
    put_u32(out, w);
    put_u32(out + 4, h);
    uint8_t *o = out + 8;
    uint64_t i = 0;
    const int exact = d == 0.0;   /* :33-39 */
    while (i < n) {
        const uint8_t *s = lin + 3 * i;
        double sum[3] = {s[0], s[1], s[2]};
        uint32_t count = 1;
        uint64_t j = i + 1;
        for (; j < n; j++) {
            const uint8_t *x = lin + 3 * j;
            int accept;
            if (exact) {
                accept = x[0] == s[0] && x[1] == s[1] && x[2] == s[2];
            } else {
                double dist = 0.0;
                for (int c = 0; c < 3; c++) {
                    const double a = sum[c] / (double)count - (double)x[c];
                    dist += a * a;
                }
                accept = sqrt(dist) <= d;
            }
            if (!accept) break;   /* x starts the next run */
            for (int c = 0; c < 3; c++) sum[c] += (double)x[c];
            if (++count == 255) { j++; break; }
        }
        uint8_t col[3];
        for (int c = 0; c < 3; c++) col[c] = (uint8_t)round(sum[c] / (double)count);   /* f64::round: halves away from zero */
        o = put_run(o, count, col);
        i = j;
    }
    return (uint64_t)(o - out);
}
