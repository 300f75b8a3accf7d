/* zip_back_ref.c -- single-core restatement of the reference's look-back coder (src/zip/back.rs) for the tests and for
 * tools/zip_back_probe.py; tests/zip_back_ref.py says what it computes and compiles it on demand.
 *
 * The six-byte keys of the window hang in hash chains, newest first (head[] per bucket, prev[] per position modulo 65 536): a probe
 * walks its whole chain -- every earlier occurrence, as the reference does -- and keeps the longest run, the farthest among equals. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ZB_MIN 6u
#define ZB_WINDOW 65535u
#define ZB_MAXLEN 32767u
#define ZB_NONE 0xFFFFFFFFFFFFFFFFull
#define ZB_BUCKETS (1u << 18)

static uint32_t bucket_of(const uint8_t *p) {
    uint64_t k = 0;
    memcpy(&k, p, ZB_MIN);
    return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 46);
}

static void put(uint8_t *out, uint64_t cap, uint64_t at, uint8_t b) {
    if (at < cap) out[at] = b;
}

/* 0: *len bytes in out (more than cap: nothing was written behind cap); 1: the reference panics; 2: out of memory.
 * stats: longest look-back, largest back, longest explicit symbol, probes */
int zb_encode(const uint8_t *text, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len, uint64_t *stats) {
    uint64_t *head = malloc(sizeof(uint64_t) * ZB_BUCKETS), *prev = malloc(sizeof(uint64_t) * 65536);
    uint64_t p = 0, e = 0, o = 0, indexed = 0;
    int rc = 0;
    if (!head || !prev) { free(head); free(prev); return 2; }
    memset(head, 0xff, sizeof(uint64_t) * ZB_BUCKETS);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (;;) {
        uint64_t best = 0, best_q = 0;
        if (p + ZB_MIN <= n) {
            for (; indexed + ZB_MIN <= p; indexed++) {   /* a key is known once all six of its bytes are history */
                const uint32_t b = bucket_of(text + indexed);
                prev[indexed & 65535] = head[b];
                head[b] = indexed;
            }
            stats[3]++;
            for (uint64_t q = head[bucket_of(text + p)]; q != ZB_NONE && q + ZB_WINDOW >= p; q = prev[q & 65535]) {
                if (memcmp(text + q, text + p, ZB_MIN)) continue;
                const uint64_t limit = p - q < n - p ? p - q : n - p;
                uint64_t l = ZB_MIN;
                while (l < limit && text[q + l] == text[p + l]) l++;
                if (l >= best) { best = l; best_q = q; }   /* (newest first: the farthest of equals comes last) */
            }
        }
        if (best) {
            if (best > ZB_MAXLEN) { rc = 1; break; }
            if (e) { put(out, cap, o - e - 2, (uint8_t)e); put(out, cap, o - e - 1, (uint8_t)(e >> 8)); if (e > stats[2]) stats[2] = e; }
            put(out, cap, o, (uint8_t)best); put(out, cap, o + 1, (uint8_t)(0x80 | (best >> 8)));
            put(out, cap, o + 2, (uint8_t)(p - best_q)); put(out, cap, o + 3, (uint8_t)((p - best_q) >> 8));
            if (best > stats[0]) stats[0] = best;
            if (p - best_q > stats[1]) stats[1] = p - best_q;
            o += 4; p += best; e = 0;
            continue;
        }
        uint64_t t = e > 2 ? e : 2;
        const int last = n - p < t;
        if (last) t = n - p;
        if (!e && t) o += 2;                              /* the header's place */
        for (uint64_t i = 0; i < t; i++) put(out, cap, o + i, text[p + i]);
        o += t; p += t; e += t;
        if (e > ZB_MAXLEN) { rc = 1; break; }
        if (last) {
            if (e) { put(out, cap, o - e - 2, (uint8_t)e); put(out, cap, o - e - 1, (uint8_t)(e >> 8)); if (e > stats[2]) stats[2] = e; }
            break;
        }
    }
    free(head); free(prev);
    *len = o;
    return rc;
}

/* need: ZB_NONE = the whole text.  0: *len bytes of text; 1: malformed (the reference panics); 2: the text has *len bytes, more than cap */
int zb_decode(const uint8_t *s, uint64_t n, uint64_t need, uint8_t *out, uint64_t cap, uint64_t *len) {
    uint64_t pos = 0, o = 0;
    uint8_t *ring = malloc(65536);   /* the text's last bytes, also behind cap */
    if (!ring) return 1;
    int rc = 0;
    while (o < need && pos + 2 <= n) {
        const uint32_t head = s[pos] | (s[pos + 1] << 8), l = head & ZB_MAXLEN;
        uint64_t k;
        pos += 2;
        if (head & 0x8000u) {
            if (pos + 2 > n) break;
            const uint32_t back = s[pos] | (s[pos + 1] << 8);
            pos += 2;
            if (back > o) { rc = 1; break; }
            k = l < back ? l : back;
            for (uint64_t i = 0; i < k; i++) {           /* (k <= back: the source lies wholly before the copy) */
                const uint8_t b = ring[(o - back + i) & 65535];
                ring[(o + i) & 65535] = b;
                if (o + i < cap) out[o + i] = b;
            }
        } else {
            if (pos + l > n) { rc = 1; break; }
            k = l;
            for (uint64_t i = 0; i < k; i++) {
                ring[(o + i) & 65535] = s[pos + i];
                if (o + i < cap) out[o + i] = s[pos + i];
            }
            pos += l;
        }
        o += k;
        if (!k) break;
    }
    free(ring);
    *len = o;
    if (!rc && o > cap) rc = 2;
    return rc;
}
