/* zip_dict_ref.c -- single-core restatement of the reference's dictionary coder (src/zip/dict.rs) for the tests and for
 * tools/zip_probe.py; tests/zip_dict_ref.py says what it computes and compiles it on demand.
 *
 * The trie is kept as edges (node, byte) -> (child, symbol) in a chained hash over parallel arrays; the decoder keeps every entry as
 * (offset, length) of the place in its own output where that text first stood. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ZD_EOF 0xFFFFu
#define ZD_NONE 0xFFFFFFFFu

typedef struct {
    uint32_t *head;                 /* bucket -> first edge */
    uint32_t *next, *node, *child;  /* per edge */
    uint8_t *byte;
    uint16_t *sym;                  /* ZD_EOF: the edge carries no symbol */
    uint32_t nbuckets, nedges, cap, nnodes;
} Trie;

static uint32_t bucket_of(const Trie *t, uint32_t node, uint8_t b) {
    /* (the byte's share is scattered, the node's is not: a flat text's single path of nodes then walks through neighbouring buckets) */
    return (node + (uint32_t)(b * 0x85EBCA6Bu >> 7)) & (t->nbuckets - 1);
}

static int trie_init(Trie *t, uint64_t n) {   /* n: the text's length -- there are at most that many edges beside the root's */
    memset(t, 0, sizeof *t);
    t->nbuckets = 1u << 20;
    while (t->nbuckets < n && t->nbuckets < (1u << 30)) t->nbuckets <<= 1;
    t->cap = 1u << 16;
    t->head = malloc(sizeof(uint32_t) * t->nbuckets);
    t->next = malloc(sizeof(uint32_t) * t->cap);
    t->node = malloc(sizeof(uint32_t) * t->cap);
    t->child = malloc(sizeof(uint32_t) * t->cap);
    t->byte = malloc(t->cap);
    t->sym = malloc(sizeof(uint16_t) * t->cap);
    if (!t->head || !t->next || !t->node || !t->child || !t->byte || !t->sym) return 0;
    memset(t->head, 0xff, sizeof(uint32_t) * t->nbuckets);
    t->nnodes = 1;
    return 1;
}

static void trie_free(Trie *t) {
    free(t->head); free(t->next); free(t->node); free(t->child); free(t->byte); free(t->sym);
}

static uint32_t edge_find(const Trie *t, uint32_t node, uint8_t b) {
    for (uint32_t e = t->head[bucket_of(t, node, b)]; e != ZD_NONE; e = t->next[e])
        if (t->node[e] == node && t->byte[e] == b) return e;
    return ZD_NONE;
}

static uint32_t edge_get(Trie *t, uint32_t node, uint8_t b) {   /* found or made */
    uint32_t e = edge_find(t, node, b);
    if (e != ZD_NONE) return e;
    if (t->nedges == t->cap) {
        t->cap *= 2;
        t->next = realloc(t->next, sizeof(uint32_t) * t->cap);
        t->node = realloc(t->node, sizeof(uint32_t) * t->cap);
        t->child = realloc(t->child, sizeof(uint32_t) * t->cap);
        t->byte = realloc(t->byte, t->cap);
        t->sym = realloc(t->sym, sizeof(uint16_t) * t->cap);
        if (!t->next || !t->node || !t->child || !t->byte || !t->sym) abort();
    }
    e = t->nedges++;
    const uint32_t h = bucket_of(t, node, b);
    t->node[e] = node; t->byte[e] = b; t->child[e] = ZD_NONE; t->sym[e] = ZD_EOF;
    t->next[e] = t->head[h];
    t->head[h] = e;
    return e;
}

/* the longest text at in[pos..n) that has a symbol: its end, the symbol in *sym */
static uint64_t longest(const Trie *t, const uint8_t *in, uint64_t pos, uint64_t n, uint16_t *sym) {
    uint32_t node = 0;
    uint64_t best = pos;
    for (uint64_t j = pos; j < n;) {
        const uint32_t e = edge_find(t, node, in[j]);
        j++;
        if (e == ZD_NONE) break;
        if (t->sym[e] != ZD_EOF) { *sym = t->sym[e]; best = j; }
        if (t->child[e] == ZD_NONE) break;
        node = t->child[e];
    }
    return best;
}

/* out: room for 2 n + 4 bytes.  info[0]: the input position behind the pair that handed out 0xFFFE (UINT64_MAX: never),
 * info[1]: the longest entry, info[2]: trie nodes.  Returns the stream's length. */
uint64_t zd_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t *info) {
    Trie t;
    if (!trie_init(&t, n)) abort();
    for (uint32_t b = 0; b < 256; b++) {
        const uint32_t e = edge_get(&t, 0, (uint8_t)b);   /* (may move the arrays: the index first, then the store) */
        t.sym[e] = (uint16_t)b;
    }
    uint32_t counter = 0x100;
    uint64_t pos = 0, len = 0, fill_end = UINT64_MAX, longest_entry = 1;
    while (pos < n) {
        uint16_t s1 = 0, s2 = ZD_EOF;
        const uint64_t mid = longest(&t, in, pos, n, &s1);
        uint64_t end = mid;
        if (mid < n) end = longest(&t, in, mid, n, &s2);
        out[len++] = (uint8_t)s1; out[len++] = (uint8_t)(s1 >> 8);
        out[len++] = (uint8_t)s2; out[len++] = (uint8_t)(s2 >> 8);
        if (mid < n && counter != ZD_EOF) {
            uint32_t node = 0;
            for (uint64_t j = pos; j + 1 < end; j++) {
                const uint32_t e = edge_get(&t, node, in[j]);
                if (t.child[e] == ZD_NONE) t.child[e] = t.nnodes++;
                node = t.child[e];
            }
            const uint32_t last = edge_get(&t, node, in[end - 1]);
            t.sym[last] = (uint16_t)counter++;
            if (end - pos > longest_entry) longest_entry = end - pos;
            if (counter == ZD_EOF) fill_end = end;
        }
        pos = end;
    }
    if (info) { info[0] = fill_end; info[1] = longest_entry; info[2] = t.nnodes; }
    trie_free(&t);
    return len;
}

/* need: UINT64_MAX = the whole stream; else whole pairs are read only while fewer than `need` bytes are there.
 * 0: ok, *len bytes in out; 1: the reference panics; 2: the text outgrows cap (*len: what was needed so far) */
int zd_decode(const uint8_t *in, uint64_t n, uint64_t need, uint8_t *out, uint64_t cap, uint64_t *len) {
    uint64_t *off = malloc(sizeof(uint64_t) * 65536), *ln = malloc(sizeof(uint64_t) * 65536);
    if (!off || !ln) abort();
    uint32_t counter = 0x100;
    uint64_t pos = 0, o = 0;
    int rc = 0;
    while (o < need && pos + 2 <= n) {
        if (pos + 4 > n) { rc = 1; break; }
        const uint16_t s[2] = {(uint16_t)(in[pos] | (in[pos + 1] << 8)), (uint16_t)(in[pos + 2] | (in[pos + 3] << 8))};
        pos += 4;
        if ((s[0] != ZD_EOF && s[0] >= counter) || (s[1] != ZD_EOF && s[1] >= counter)) { rc = 1; break; }
        const uint64_t start = o;
        for (int k = 0; k < 2 && rc == 0; k++) {
            if (s[k] == ZD_EOF) continue;
            const uint64_t l = s[k] < 256 ? 1 : ln[s[k]];
            if (l > cap - o) { o += l; rc = 2; break; }
            if (s[k] < 256) out[o] = (uint8_t)s[k];
            else memcpy(out + o, out + off[s[k]], l);   /* the source ends at or before `start` */
            o += l;
        }
        if (rc) break;
        if (counter != ZD_EOF) { off[counter] = start; ln[counter] = o - start; counter++; }
    }
    *len = o;
    free(off); free(ln);
    return rc;
}
