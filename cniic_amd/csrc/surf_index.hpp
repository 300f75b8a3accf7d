// surf_index.hpp -- the index arithmetic of the surface import / export kernels (k_surface.hip), in plain functions for host and device:
// how a frame's pixels are cut into chunks and a chunk into row pieces, how a row piece splits into head / groups / tail, and which
// aligned 16-byte words a run of source bytes is loaded from.  tests/surf_index_check.cpp compiles this file alone, so it includes
// nothing of the library.
//
// The packed side (rows back to back, 3 bytes per pixel) of a frame is cut into chunks of kSurfChunkPx PIXELS, so that a chunk, and
// with it every row piece, starts on a pixel.  A row piece is the part of one row inside one chunk: n pixels that are contiguous on
// both sides.  On the side that is WRITTEN (the packed RGB of an import, the surface of an export) it splits into
//   head:   the fewest pixels after which the written address is a multiple of 16 (written pixel by pixel in byte stores),
//   groups: of kSurfGroupPx = 16 pixels, 16 x 3 = 48 or 16 x 4 = 64 bytes, three or four aligned 16-byte stores,
//   tail:   fewer than 16 pixels, byte stores again.
// With 3 written bytes per pixel such a head always exists and is below 16 pixels (3 and 16 are coprime); with 4 it exists only where
// the address is a multiple of 4 (then it is below 4 pixels), otherwise the whole piece is head.
// The side that is READ has an alignment of its own: a group's bytes are fetched as the aligned 16-byte words that hold them
// (surf_words) and shifted together in registers.  A word is fetched only if it holds a byte of the run asked for.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_SURF_HD __host__ __device__ __forceinline__
#else
#define CNIIC_SURF_HD inline
#endif

namespace cniic {

constexpr uint32_t kSurfChunkPx = 4096;   // pixels of a chunk: 12 KiB of packed RGB, four steps of 64 lanes x 16 pixels
constexpr uint32_t kSurfGroupPx = 16;

// bytes per pixel of a CNIIC_PX_* format (NV12: of its Y plane); 0: no such format
CNIIC_SURF_HD uint32_t surf_bpp(int32_t format) {
    switch (format) {
        case 1: return 1;   // L8
        case 2: return 2;   // LA8
        case 3: return 3;   // RGB8
        case 4: return 4;   // RGBA8
        case 5: return 3;   // BGR8
        case 6: return 4;   // BGRA8
        case 7: return 1;   // NV12 (Y)
    }
    return 0;
}

struct SurfSplit { uint32_t head, groups, tail; };   // pixels, groups of kSurfGroupPx; head + 16 groups + tail == n

// n pixels of wbpp (3 or 4) bytes each are written from address `addr` on
CNIIC_SURF_HD SurfSplit surf_split(uint64_t addr, uint32_t n, uint32_t wbpp) {
    const uint32_t gap = (uint32_t)((0 - addr) & 15);   // bytes to the next boundary
    uint32_t head;
    if (wbpp == 3) head = (gap * 11u) & 15u;            // 3 head == gap (mod 16), and 3 x 11 == 1 (mod 16)
    else head = (gap & 3u) ? n : gap >> 2;
    if (head > n) head = n;
    SurfSplit s;
    s.head = head;
    s.groups = (n - head) / kSurfGroupPx;
    s.tail = (n - head) % kSurfGroupPx;
    return s;
}

// `nbytes` > 0 bytes from address `addr` on lie in surf_words(addr, nbytes) aligned 16-byte words, the first one at addr - (addr & 15);
// word i of them is wanted iff surf_word_wanted: the fetch declares room for the most words an address can need and skips the rest
CNIIC_SURF_HD uint32_t surf_words(uint64_t addr, uint32_t nbytes) { return ((uint32_t)(addr & 15) + nbytes + 15u) >> 4; }
CNIIC_SURF_HD bool surf_word_wanted(uint32_t i, uint32_t m /* addr & 15 */, uint32_t nbytes) { return 16u * i < m + nbytes; }

// NV12: pixels [x, x + n) of a row take their chroma from bytes [surf_uv_begin, surf_uv_begin + surf_uv_bytes) of the UV row
CNIIC_SURF_HD uint32_t surf_uv_begin(uint32_t x) { return x & ~1u; }
CNIIC_SURF_HD uint32_t surf_uv_bytes(uint32_t x, uint32_t n) { return ((x + n - 1) | 1u) + 1u - (x & ~1u); }

// chunks of a frame of npx pixels
CNIIC_SURF_HD uint64_t surf_chunks(uint64_t npx) { return (npx + kSurfChunkPx - 1) / kSurfChunkPx; }

// The row pieces of pixels [p, p_end) of a frame of width w, in order: surf_piece_first, then surf_piece_next until it says false.
struct SurfPiece { uint32_t y, x, n; };   // n pixels of row y from column x on
CNIIC_SURF_HD uint32_t surf_min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
CNIIC_SURF_HD SurfPiece surf_piece_first(uint32_t p, uint32_t p_end, uint32_t w) {
    SurfPiece r;
    r.y = p / w;
    r.x = p - r.y * w;
    r.n = surf_min_u32(w - r.x, p_end - p);
    return r;
}
// (left: pixels of the chunk behind the piece before this call)
CNIIC_SURF_HD bool surf_piece_next(SurfPiece &r, uint32_t &left, uint32_t w) {
    left -= r.n;
    if (!left) return false;
    r.y += 1;        // (a piece that does not end its chunk ends its row)
    r.x = 0;
    r.n = surf_min_u32(w, left);
    return true;
}

}  // namespace cniic
