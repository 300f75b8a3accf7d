// hz_small.hpp -- what is different about Hilbert { compress: Zip } (hilbertc.rs:27-29,47-49,58-62,73-77) on the small-frame kernels of
// `zip(dict)`: k_hz_small (k_zd_small.hip) and k_hz_small_dec (k_zd_small_dec.hip) are those kernels' bodies under a second text kind.
// Plain functions for host and device.  tests/hz_small_check.cpp compiles this file beside zd_small.hpp and zd_small_dec.hpp, so it
// includes nothing of the library.
//
// The stream: the two dimensions as u32 LE, RAW, then the dictionary coder's pairs over a text WITHOUT dimensions: per pixel, in the order
// of the scan, the u64 LE 3 and r, g, b.  N = 11 n bytes for n pixels.
//
// The decode is lenient where Zip::Dict's is not (decode_hilbert_zip, zipdict.cpp, restates it): the traversal asks for w h colours and
// takes what it gets.  Colours the text does not reach stay zero (ImageBuffer::new), and so do those from the first record on whose
// length is not 3, which ends deser_stream (ser.rs:216-221, :269-271).  What stays an error is what the lazy reader panics on while it
// still wants bytes: a symbol that has not been handed out, and a first symbol without a second at the stream's end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CNIIC_HZ_HD __host__ __device__ __forceinline__
#else
#define CNIIC_HZ_HD inline
#endif

namespace cniic {

constexpr uint32_t kHzSmallMaxPx = 16384;      // pixels of a frame that takes either route
constexpr uint32_t kHzHead = 8;                // the raw dimensions in front of the pairs
constexpr uint32_t kHzScanLds = 2 * 1024 + 16; // the 2^n scan's tables (HilbertLut) in LDS

// ---- the text of the encode: px holds the frame's pixels in SCAN order, 3 bytes each
CNIIC_HZ_HD uint32_t hz_text_len(uint32_t n) { return 11u * n; }
CNIIC_HZ_HD uint8_t hz_text_byte(uint32_t i, const uint8_t *scan_px) {
    const uint32_t p = i / 11, r = i - 11 * p;
    return r == 0 ? 3 : r < 8 ? 0 : scan_px[3 * p + (r - 8)];
}
struct HzText {
    const uint8_t *px;
    uint32_t N;
    CNIIC_HZ_HD uint8_t operator[](uint32_t i) const { return hz_text_byte(i, px); }
};

// ---- sizes: the head, 4 bytes a pair, a pair per 2 bytes of text at least and one for a last byte alone.  The slot is a multiple of 16,
// and the pairs behind the 8-byte head stay 4-byte aligned in it.
CNIIC_HZ_HD uint64_t hz_stream_max(uint64_t N) { return kHzHead + 2 * N + 2; }
CNIIC_HZ_HD uint64_t hz_stride(uint64_t N) { return (hz_stream_max(N) + 15) & ~15ull; }

// ---- the decode.  The verdicts are numbered as zd_small_dec.hpp's (kZsdOk, kZsdHandedBack, kZsdBadSymbol, kZsdDangling).
constexpr uint32_t kHzdOk = 0, kHzdHandedBack = 1, kHzdBadSymbol = 2, kHzdDangling = 3;
CNIIC_HZ_HD uint32_t hzd_need(uint32_t n) { return 11u * n; }
// total = O[kb] (saturated at need + 1), P = the pairs looked at, len = the bytes behind the head.  *a: the number of the message.
// A short text is no error: the order is the one in which the single decode meets its panics.
CNIIC_HZ_HD uint32_t hzd_verdict(uint32_t total, uint32_t need, uint32_t kb, uint32_t P, uint64_t len, uint32_t *a) {
    *a = 0;
    if (total >= need) return kHzdOk;   // nothing behind the pair that completes byte need - 1 matters
    if (kb < P) { *a = kb; return kHzdBadSymbol; }
    if (P < len / 4) return kHzdHandedBack;   // the stream goes on behind the cap
    if ((len & 3) >= 2) return kHzdDangling;
    return kHzdOk;
}
// the whole records the text reaches: the scan positions whose bytes phase 5 looks at
CNIIC_HZ_HD uint32_t hzd_records(uint32_t total, uint32_t need) { return (total < need ? total : need) / 11u; }
// the record cut: scan positions below it get their colours, every other pixel is zero.  bad: the lowest record among those reached whose
// first 8 bytes are not the u64 3, or any number >= records if there is none.
CNIIC_HZ_HD uint32_t hzd_cut(uint32_t records, uint32_t bad) { return bad < records ? bad : records; }

}  // namespace cniic
