// decode_batch_plan.hpp -- what the batch decode routes of codec.cpp (cniic_codec_decode_batch) work out without a GPU: the extent of a
// chunk, where the staged images of a chunk lie, which bytes of a host batch go up, and the reads of a stream's header and of a
// `voronoi` centroid list.  No HIP header; tests/decode_batch_plan_check.cpp compiles this file with huff_host.cpp and nothing else.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "huff_host.hpp"

namespace cniic {

// The decode routes' chunks, whose items cost what they cost each: the end i1 of the chunk that starts at item i0 of n and takes items
// while their cost(i) together stay within budget; the first always fits.
template <class Cost>
static size_t take_chunk(size_t i0, size_t n, uint64_t budget, Cost cost) {
    size_t i1 = i0;
    uint64_t need = 0;
    while (i1 < n && (i1 == i0 || need + cost(i1) <= budget)) need += cost(i1++);
    return i1;
}

// Slots of a block, one behind the other, each rounded up to 16 bytes: item i of n gets one when plan(i, bytes, true) says so
struct SlotLayout {
    static constexpr uint64_t kNone = ~0ull;
    std::vector<uint64_t> at;   // where item i's slot starts, kNone: it has none
    uint64_t total = 0;
    explicit SlotLayout(size_t n) : at(n, kNone) {}
    static uint64_t room(uint64_t bytes) { return (bytes + 15) & ~15ull; }
    void plan(size_t i, uint64_t bytes, bool needed) {
        if (needed) { at[i] = total; total += room(bytes); }
    }
    bool has(size_t i) const { return at[i] != kNone; }
};

// The bytes [lo, hi) of a batch (frame f at f * stride, lens[f] bytes of it) from frame `first` to the end of frame `last` >= first
struct ByteSpan { uint64_t lo, hi; };
inline ByteSpan frames_span(uint32_t first, uint32_t last, uint64_t stride, const uint64_t *lens) {
    return ByteSpan{(uint64_t)first * stride, (uint64_t)last * stride + lens[last]};
}

// A stream's header (create_image_buffer_standard codec.rs:22-26): w and h from the n bytes at p; pos is left behind them
inline bool frame_dims(const uint8_t *p, uint64_t n, uint32_t *w, uint32_t *h, uint64_t *pos) {
    *pos = 0;
    return get_u32(p, n, *pos, *w) && get_u32(p, n, *pos, *h);
}
// 1 .. max_px pixels (below 2^62) whose image fits img_stride
inline bool dims_fit(uint64_t npx, uint64_t max_px, uint64_t img_stride) { return npx && npx <= max_px && npx * 3 <= img_stride; }

// A `voronoi` stream behind its dimensions (clusterc.rs:168-189): K as u64, then per centroid x, y as u32, the u64 3 and r g b, in the n
// bytes at p from pos on.  sink(k, x, y, r, g, b) gets every centroid in front of the first one that is not well formed.
enum class VorHead {
    Ok,
    Truncated,       // the K word is not there
    TruncatedList,   // K > (n - pos) / 19
    BadCentroid,     // a field is missing, the length word is not 3, or the 3 colour bytes are not there
};
template <class Sink>
static VorHead vor_parse_head(const uint8_t *p, uint64_t n, uint64_t &pos, uint64_t *K, Sink sink) {
    if (!get_u64(p, n, pos, *K)) return VorHead::Truncated;
    if (*K > (n - pos) / 19) return VorHead::TruncatedList;
    for (uint64_t k = 0; k < *K; k++) {
        uint32_t x, y;
        uint64_t l;
        if (!get_u32(p, n, pos, x) || !get_u32(p, n, pos, y) || !get_u64(p, n, pos, l) || l != 3 || pos + 3 > n) return VorHead::BadCentroid;
        sink(k, x, y, p[pos], p[pos + 1], p[pos + 2]);
        pos += 3;
    }
    return VorHead::Ok;
}

}  // namespace cniic
