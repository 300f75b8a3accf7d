// surf_index_check.cpp -- walks cniic_amd/csrc/surf_index.hpp's split of every row the way k_surface.hip does, on the host, through buffers of
// exactly the surface's and the frame's size (so that an address sanitizer sees any byte touched outside them), and asserts that
//   every written byte is produced exactly once, every 16-byte store is aligned and inside its row's pixels,
//   every fetched 16-byte word is aligned and holds a byte of the row it is fetched for, and the bytes equal a byte-wise loop.
// Stand-alone: compiled by tests/test_surfaces_cpu.py, plain and under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../cniic_amd/csrc/surf_index.hpp"

using namespace cniic;

static long failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// a buffer whose first used byte sits `residue` bytes behind a 16-byte boundary and whose last used byte is the allocation's last
struct Buf {
    void *block = nullptr; uint8_t *p = nullptr; uint64_t n = 0;
    Buf(uint32_t residue, uint64_t bytes) : n(bytes) {
        if (posix_memalign(&block, 16, residue + bytes)) abort();
        p = (uint8_t *)block + residue;
    }
    ~Buf() { free(block); }
    Buf(const Buf &) = delete;
};

struct Walk {
    const uint8_t *src_lo, *src_hi;     // the surface's allocation
    uint8_t *dst_lo, *dst_hi;           // the written side's allocation
    std::vector<uint8_t> *written;      // per byte of the written side: how often
    const uint8_t *row_lo, *row_hi;     // the source bytes of the row being read
    uint8_t *out_lo, *out_hi;           // the bytes the row piece may write
    long words = 0, stores16 = 0;

    void store1(uint8_t *a, uint8_t v) {
        CHECK(a >= out_lo && a < out_hi, "byte store outside the piece");
        *a = v; (*written)[a - dst_lo]++;
    }
    void store16(uint8_t *a, const uint32_t v[4]) {
        CHECK(((uintptr_t)a & 15) == 0, "misaligned 16-byte store");
        CHECK(a >= out_lo && a + 16 <= out_hi, "16-byte store outside the piece");
        memcpy(a, v, 16);
        for (int i = 0; i < 16; i++) (*written)[a + i - dst_lo]++;
        stores16++;
    }
    // what the kernel's surf_fetch does: the wanted aligned words, shifted down by m bytes, dword moves then v_alignbit_b32
    template <int NDW> void fetch(const uint8_t *base, uint32_t m, uint32_t nbytes, uint32_t (&d)[NDW]) {
        constexpr int NW = (15 + 4 * NDW + 15) / 16;
        static_assert(4 * NW >= NDW + 4, "room for the shift");
        uint32_t w[4 * NW];
        CHECK(((uintptr_t)base & 15) == 0, "misaligned word");
        for (int i = 0; i < NW; i++) {
            uint8_t b[16];
            memset(b, 0, 16);
            if (surf_word_wanted((uint32_t)i, m, nbytes)) {
                const uint8_t *wa = base + 16 * i;
                CHECK(wa < row_hi && wa + 16 > row_lo, "a fetched word holds no byte of its row");
                CHECK((uint32_t)i < surf_words((uint64_t)(uintptr_t)(base + m), nbytes), "surf_words and surf_word_wanted differ");
                for (int k = 0; k < 16; k++)   // (the hardware reads the whole word: whole words are inside the page; the bytes of it outside the allocation are not used)
                    if (wa + k >= src_lo && wa + k < src_hi) b[k] = wa[k]; else b[k] = 0xEE;
                words++;
            } else CHECK((uint32_t)i >= surf_words((uint64_t)(uintptr_t)(base + m), nbytes), "surf_words and surf_word_wanted differ");
            memcpy(&w[4 * i], b, 16);
        }
        const uint32_t q = m >> 2, r = (m & 3) * 8;
        if (q & 1) for (int j = 0; j < 4 * NW - 1; j++) w[j] = w[j + 1];
        if (q & 2) for (int j = 0; j < 4 * NW - 2; j++) w[j] = w[j + 2];
        for (int j = 0; j < NDW; j++) d[j] = (uint32_t)((((uint64_t)w[j + 1] << 32) | w[j]) >> r);
    }
};

static int src_of(int IB, int OB, int kind, int j) {
    const int p = j / OB, ch = j % OB;
    return ch == 3 ? -1 : kind == 2 ? p * IB : p * IB + (kind == 1 ? 2 - ch : ch);
}

template <int IB, int OB> static void piece(Walk &W, const uint8_t *s, uint8_t *o, uint32_t n, int kind, uint32_t alpha) {
    const SurfSplit sp = surf_split((uint64_t)(uintptr_t)o, n, OB);
    CHECK(sp.head + kSurfGroupPx * sp.groups + sp.tail == n && sp.tail < kSurfGroupPx, "split of %u", n);
    CHECK(sp.head == n || (((uintptr_t)o + (uint64_t)sp.head * OB) & 15) == 0, "the head does not reach a boundary");
    CHECK(sp.head < 16 || (OB == 4 && ((uintptr_t)o & 3)), "head of %u pixels", sp.head);
    auto px = [&](uint32_t i) {
        for (int ch = 0; ch < OB; ch++) {
            const int from = src_of(IB, OB, kind, ch);
            W.store1(o + (uint64_t)i * OB + ch, from < 0 ? (uint8_t)alpha : s[(uint64_t)i * IB + from]);
        }
    };
    for (uint32_t i = 0; i < sp.head; i++) px(i);
    for (uint32_t i = 0; i < sp.tail; i++) px(sp.head + kSurfGroupPx * sp.groups + i);
    if (!sp.groups) return;
    s += (uint64_t)sp.head * IB; o += (uint64_t)sp.head * OB;
    const uint32_t m = (uint32_t)((uintptr_t)s & 15);
    for (uint32_t g = 0; g < sp.groups; g++) {
        uint32_t a[4 * IB], v[4 * OB];
        W.fetch<4 * IB>(s - m + (uint64_t)g * 16 * IB, m, 16 * IB, a);
        for (int d = 0; d < 4 * OB; d++) {
            uint32_t x = 0;
            for (int b = 0; b < 4; b++) {
                const int from = src_of(IB, OB, kind, 4 * d + b);
                x |= (from < 0 ? alpha : (a[from >> 2] >> (8 * (from & 3))) & 255u) << (8 * b);
            }
            v[d] = x;
        }
        for (int k = 0; k < OB; k++) W.store16(o + (uint64_t)g * 16 * OB + 16 * k, &v[4 * k]);
    }
}

static void dispatch(Walk &W, int IB, int OB, const uint8_t *s, uint8_t *o, uint32_t n, int kind, uint32_t alpha) {
    if (OB == 4) { piece<3, 4>(W, s, o, n, kind, alpha); return; }
    switch (IB) {
        case 1: piece<1, 3>(W, s, o, n, kind, alpha); break;
        case 2: piece<2, 3>(W, s, o, n, kind, alpha); break;
        case 3: piece<3, 3>(W, s, o, n, kind, alpha); break;
        default: piece<4, 3>(W, s, o, n, kind, alpha); break;
    }
}

// one surface of w x h, pixels of `bpp` bytes on the pitched side; to_surface: the packed side is read and the pitched side written
static void surface(uint32_t w, uint32_t h, int bpp, int kind, bool to_surface, uint32_t res_pitched, uint32_t res_packed, uint32_t pad, long *words,
                    long *stores16) {
    const uint64_t row = (uint64_t)w * bpp, pitch = row + pad, pitched_bytes = (uint64_t)(h - 1) * pitch + row, packed_bytes = 3ull * w * h;
    Buf pitched(res_pitched, pitched_bytes), packed(res_packed, packed_bytes);
    Buf &rd = to_surface ? packed : pitched, &wr = to_surface ? pitched : packed;
    uint32_t x = 12345u + w * 7919u + h * 31u + (uint32_t)bpp;
    for (uint64_t i = 0; i < rd.n; i++) { x = x * 1664525u + 1013904223u; rd.p[i] = (uint8_t)(x >> 24); }
    memset(wr.p, 0xA5, wr.n);
    std::vector<uint8_t> written(wr.n, 0);
    Walk W;
    W.src_lo = rd.p; W.src_hi = rd.p + rd.n; W.dst_lo = wr.p; W.dst_hi = wr.p + wr.n; W.written = &written;
    const int IB = to_surface ? 3 : bpp, OB = to_surface ? bpp : 3;
    const uint32_t alpha = 0x5C, npx = w * h;
    for (uint32_t p = 0; p < npx; p += kSurfChunkPx) {
        uint32_t left = surf_min_u32(kSurfChunkPx, npx - p);
        SurfPiece pc = surf_piece_first(p, p + left, w);
        do {
            const uint8_t *s; uint8_t *o;
            if (to_surface) {
                s = packed.p + ((uint64_t)pc.y * w + pc.x) * 3; o = pitched.p + pc.y * pitch + (uint64_t)pc.x * bpp;
                W.row_lo = packed.p + (uint64_t)pc.y * w * 3; W.row_hi = W.row_lo + 3ull * w;
            } else {
                s = pitched.p + pc.y * pitch + (uint64_t)pc.x * bpp; o = packed.p + ((uint64_t)pc.y * w + pc.x) * 3;
                W.row_lo = pitched.p + pc.y * pitch; W.row_hi = W.row_lo + row;
            }
            W.out_lo = o; W.out_hi = o + (uint64_t)pc.n * OB;
            dispatch(W, IB, OB, s, o, pc.n, kind, alpha);
        } while (surf_piece_next(pc, left, w));
    }
    // the byte-wise loop
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t xx = 0; xx < w; xx++)
            for (int ch = 0; ch < OB; ch++) {
                const int from = src_of(IB, OB, kind, ch);
                const uint64_t at = to_surface ? y * pitch + (uint64_t)xx * bpp + ch : ((uint64_t)y * w + xx) * 3 + ch;
                const uint8_t want = from < 0 ? (uint8_t)alpha : to_surface ? packed.p[((uint64_t)y * w + xx) * 3 + from] : pitched.p[y * pitch + (uint64_t)xx * bpp + from];
                CHECK(wr.p[at] == want && written[at] == 1, "w %u h %u bpp %d kind %d export %d res %u %u pad %u: byte %llu of pixel (%u, %u) is %u (want %u), written %u times",
                      w, h, bpp, kind, (int)to_surface, res_pitched, res_packed, pad, (unsigned long long)at, xx, y, wr.p[at], want, written[at]);
            }
    if (to_surface)   // the pitch's padding
        for (uint32_t y = 0; y + 1 < h; y++)
            for (uint64_t i = row; i < pitch; i++) CHECK(wr.p[y * pitch + i] == 0xA5 && written[y * pitch + i] == 0, "padding written");
    *words += W.words; *stores16 += W.stores16;
}

int main() {
    // ---- the split on its own: every residue, lengths 0 ... 100
    for (uint32_t wbpp = 3; wbpp <= 4; wbpp++)
        for (uint64_t addr = 4096; addr < 4096 + 16; addr++)
            for (uint32_t n = 0; n <= 100; n++) {
                const SurfSplit sp = surf_split(addr, n, wbpp);
                CHECK(sp.head + 16 * sp.groups + sp.tail == n && sp.tail < 16, "split");
                uint32_t k = 0;   // the fewest pixels to a boundary, by trying
                while (k < n && (addr + (uint64_t)k * wbpp) % 16) k++;
                CHECK(sp.head == k, "addr %llu n %u bpp %u: head %u, by trying %u", (unsigned long long)addr, n, wbpp, sp.head, k);
            }
    if (!failures) printf("ok split: the head is the fewest pixels to a 16-byte boundary\n");

    // ---- the import: widths 1 ... 70 x bpp 1 ... 4 x both residues 0 ... 15 x padding 0, 1, 5 (three rows)
    long before = failures, words = 0, stores = 0, surfaces = 0;
    const uint32_t pads[3] = {0, 1, 5};
    for (uint32_t w = 1; w <= 70; w++)
        for (int bpp = 1; bpp <= 4; bpp++)
            for (uint32_t rs = 0; rs < 16; rs++)
                for (uint32_t rd = 0; rd < 16; rd++)
                    for (uint32_t pad : pads) {
                        const int kind = bpp <= 2 ? 2 : (int)((w + rs) & 1);   // grey; the 3- and 4-byte formats in order and swapped in turn
                        surface(w, 3, bpp, kind, false, rs, rd, pad, &words, &stores);
                        surfaces++;
                    }
    if (failures == before) printf("ok import: %ld surfaces, %ld words fetched, %ld 16-byte stores\n", surfaces, words, stores);

    // ---- the export: the same with 3 and 4 written bytes per pixel
    before = failures; words = stores = surfaces = 0;
    for (uint32_t w = 1; w <= 70; w++)
        for (int bpp = 3; bpp <= 4; bpp++)
            for (uint32_t rs = 0; rs < 16; rs++)
                for (uint32_t rd = 0; rd < 16; rd++)
                    for (uint32_t pad : pads) {
                        surface(w, 3, bpp, (int)((w + rd) & 1), true, rd, rs, pad, &words, &stores);
                        surfaces++;
                    }
    if (failures == before) printf("ok export: %ld surfaces, %ld words fetched, %ld 16-byte stores\n", surfaces, words, stores);

    // ---- chunks: frames of several chunks, rows longer than a chunk, rows that straddle chunks
    before = failures; words = stores = surfaces = 0;
    const uint32_t big[][2] = {{70, 200}, {5000, 3}, {40000, 1}, {3, 9000}, {4096, 2}, {4095, 3}, {4097, 3}, {1365, 7}};
    for (auto &wh : big)
        for (int bpp = 1; bpp <= 4; bpp++) {
            surface(wh[0], wh[1], bpp, bpp <= 2 ? 2 : 1, false, 5, 11, 3, &words, &stores);
            if (bpp >= 3) surface(wh[0], wh[1], bpp, 0, true, 4, 7, 8, &words, &stores);
            surfaces++;
        }
    for (uint32_t w = 1; w <= 70; w++) {   // the pieces alone: in order, inside one row, all of the chunk
        const uint32_t h = 3 * kSurfChunkPx / w + 1, npx = w * h;
        CHECK(surf_chunks(npx) == (npx + kSurfChunkPx - 1) / kSurfChunkPx, "chunks");
        uint32_t at = 0;
        for (uint32_t p = 0; p < npx; p += kSurfChunkPx) {
            uint32_t left = surf_min_u32(kSurfChunkPx, npx - p);
            SurfPiece pc = surf_piece_first(p, p + left, w);
            do {
                CHECK(pc.y * w + pc.x == at && pc.n > 0 && pc.x + pc.n <= w && pc.n <= left, "piece (%u, %u, %u) at pixel %u", pc.y, pc.x, pc.n, at);
                at += pc.n;
            } while (surf_piece_next(pc, left, w));
            CHECK(at == p + surf_min_u32(kSurfChunkPx, npx - p), "a chunk's pieces end at pixel %u", at);
        }
        CHECK(at == npx, "pieces cover %u of %u pixels", at, npx);
    }
    if (failures == before) printf("ok pieces: %ld large surfaces, %ld words fetched, %ld 16-byte stores\n", surfaces, words, stores);

    // ---- NV12's chroma run: the pairs above pixels [x, x + n) are bytes [begin, begin + bytes) of the UV row, inside 2 ceil(w / 2)
    before = failures;
    for (uint32_t w = 1; w <= 70; w++)
        for (uint32_t x = 0; x < w; x++)
            for (uint32_t n = 1; x + n <= w; n++) {
                uint32_t lo = ~0u, hi = 0;
                for (uint32_t i = x; i < x + n; i++) { lo = surf_min_u32(lo, 2 * (i >> 1)); hi = 2 * (i >> 1) + 2 > hi ? 2 * (i >> 1) + 2 : hi; }
                CHECK(surf_uv_begin(x) == lo && surf_uv_begin(x) + surf_uv_bytes(x, n) == hi && hi <= 2 * ((w + 1) / 2), "chroma of pixels [%u, %u)", x, x + n);
                CHECK(n != kSurfGroupPx || surf_uv_bytes(x, n) == 16 + 2 * (x & 1), "a group's chroma bytes");
            }
    if (failures == before) printf("ok nv12_chroma: the pairs of every run of pixels of rows up to 70 wide\n");

    if (failures) { printf("FAIL: %ld checks\n", failures); return 1; }
    return 0;
}
