// k_zd_small_dec.hip -- the decode of SMALL `zip(dict)` frames (at most kZdSmallDecMaxPx pixels), one workgroup per frame from its pairs to
// its pixels, any number of frames in one launch (cniic_codec_decode_batch / cniic_codec_measure_batch; codec.cpp zip_dict_batch).
// Unlike the encode, this decode is not serial: pair k hands out symbol 0x100 + k whatever it holds, so a symbol is "the text of an earlier
// pair", the lengths are a DAG, the offsets their prefix sums, and every byte of the text finds its literal by hopping from pair to pair
// (zd_small_dec.hpp has the arithmetic, the five phases and why the differences of saturated offsets are exact where they are used).
// No text buffer, no ordering between copies, no block waits for another.
//
// LDS, all dynamic and sized by the launch's neediest frame (the host launches by size class, so that small frames share a CU): the image
// at its destination's 16-byte phase (3 w h + 16, rounded up), then a word per pair and one more -- the lengths of phase 2, the offsets
// from phase 3 on, in place -- and, where the row says so (it fits beside the rest), the pair words themselves, staged by phase 1.  The
// other frames read their pairs where the stream lies, as aligned words (a stream starts at any byte).
//
// k_hz_small_dec is the same body for Hilbert { compress: Zip } (cniic_hilbert_zip_decode_batch; codec.cpp zip_dict_batch under kSmallDecHilbertZip): the pairs
// start behind the 8 raw bytes of the dimensions (the host reads those and hands the kernel the pairs), need = 11 w h, phases 1 - 3 as
// they are.  The verdict is the lenient one of hz_small.hpp -- a short text and a bad record are no errors: they bound the scan positions
// that get colours, every other pixel is zero -- and in phase 5 the colour of scan position p goes to Scan::xy(p) of the LDS image.
#include "common.hpp"
#include "hilbert_scan.hpp"
#include "hz_small.hpp"
#include "zd_small_dec.hpp"

namespace cniic {

constexpr int kZsdThreads = 1024;   // 16 waves: 128 VGPRs a lane at most
constexpr uint32_t kZsdLdsMax = 160 * 1024 - 512;   // a CU's LDS less the few static words below
static_assert(zsd_lds_bytes(kZsdMaxPairs, kZdSmallDecMaxPx) <= kZsdLdsMax, "the largest frame with the most pairs fits one CU's LDS");
constexpr uint32_t kHzdLdsMax = kZsdLdsMax - kHzScanLds;   // ... less the 2^n scan's tables
static_assert(kHzSmallMaxPx == kZdSmallDecMaxPx && zsd_lds_bytes(kZsdMaxPairs, kHzSmallMaxPx) <= kHzdLdsMax && kHzdLdsMax % 16 == 0 && sizeof(HilbertLut) == kHzScanLds,
              "the 2064 bytes of scan tables fit beside the largest frame with the most pairs");

struct ZsdPairs {
    const uint32_t *lds;     // the staged words, or null
    const uint32_t *words;   // the aligned word that holds the stream's first byte
    uint32_t residue;        // where in it
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
        if (lds) return lds[k];
        return zsd_word_from_aligned(words[k], residue ? words[k + 1] : 0u, residue);
    }
};

// kHilbert: the frame is Hilbert { compress: Zip }'s (row.stream = its pairs, row.len = their bytes; sc: the frame's scan)
template <bool kHilbert>
__device__ __forceinline__ void zsd_frame(const ZdSmallDecRow &row, uint32_t f, uint32_t lds_bytes, uint32_t hops, uint32_t rounds, const Scan &sc,
                                          ZdSmallDecResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t zsd_lds[];
    __shared__ uint32_t s_kb, s_bad, s_back, s_verdict, s_a, s_b, s_wsum[kZsdThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = row.w * row.h, need = kHilbert ? hzd_need(n) : zsd_need(n), C = need + 1u, P = row.pairs;   // n: 1 .. kZdSmallDecMaxPx
    const uint32_t img_room = (3u * n + 16u + 15u) & ~15u;
    if (n == 0 || n > kZdSmallDecMaxPx || P > kZsdMaxPairs || img_room + 4u * (P + 1u) + (row.staged ? 4u * P : 0u) > lds_bytes) {   // (never: the host sized the launch)
        if (tid == 0) res[f] = ZdSmallDecResult{kZsdHandedBack, 0u, 0u, 0u};
        return;
    }
    uint8_t *img = zsd_lds;
    uint32_t *O = reinterpret_cast<uint32_t *>(zsd_lds + img_room);
    uint32_t *staged = row.staged ? O + P + 1u : nullptr;
    const uintptr_t at = reinterpret_cast<uintptr_t>(row.stream);
    const ZsdPairs from_stream{nullptr, reinterpret_cast<const uint32_t *>(at & ~(uintptr_t)3), (uint32_t)(at & 3)};
    const ZsdPairs pairs{staged, from_stream.words, from_stream.residue};

    // ---- 1. validity
    if (tid == 0) { s_kb = P; s_bad = n; s_back = 0; }
    __syncthreads();
    {
        uint32_t first_bad = P;
        for (uint32_t k = tid; k < P; k += kZsdThreads) {
            const uint32_t word = from_stream(k);
            if (staged) staged[k] = word;
            O[k] = kZsdUnknown;
            if (first_bad == P && zsd_pair_bad(word, k)) first_bad = k;
        }
        if (first_bad < P) atomicMin(&s_kb, first_bad);
    }
    __syncthreads();
    const uint32_t kb = s_kb;

    // ---- 2. lengths: round r resolves the pairs of generation r
    for (uint32_t r = 0;; r++) {
        if (r == rounds) {
            if (tid == 0) res[f] = ZdSmallDecResult{kZsdHandedBack, 0u, 0u, 0u};
            return;
        }
        for (uint32_t k = tid; k < kb; k += kZsdThreads)
            if (O[k] == kZsdUnknown) zsd_resolve(pairs(k), k, O, C);
        __syncthreads();
        int unknown = 0;
        for (uint32_t k = tid; k < kb; k += kZsdThreads) unknown |= zsd_settle(k, O) ? 1 : 0;
        if (!__syncthreads_or(unknown)) break;
    }

    // ---- 3. offsets: a run of pairs per lane, the lanes' sums scanned across the block, all saturating at C
    {
        const uint32_t run = (kb + kZsdThreads - 1) / kZsdThreads, k0 = min(tid * run, kb), k1 = min(k0 + run, kb);
        uint32_t sum = 0;
        for (uint32_t k = k0; k < k1; k++) sum = zsd_sat_add(sum, O[k], C);
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if ((tid & 63u) >= (uint32_t)d) incl = zsd_sat_add(incl, o, C);
        }
        if ((tid & 63u) == 63u) s_wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t wv = 0; wv < (tid >> 6); wv++) before = zsd_sat_add(before, s_wsum[wv], C);
        uint32_t excl = zsd_sat_add(before, incl, C);   // the lanes up to this one
        if (tid == kZsdThreads - 1) O[kb] = excl;       // (the word of pair kb, or the one more)
        // what lies before this lane's run: the waves before, and the lanes before in this wave
        uint32_t lane_before = __shfl_up(incl, 1);
        if ((tid & 63u) == 0) lane_before = 0;
        uint32_t off = zsd_sat_add(before, lane_before, C);
        for (uint32_t k = k0; k < k1; k++) {
            const uint32_t l = O[k];
            O[k] = off;
            off = zsd_sat_add(off, l, C);
        }
    }
    __syncthreads();

    // ---- 4. verdict
    if (tid == 0) {
        uint32_t a = 0, b = 0;
        s_verdict = kHilbert ? hzd_verdict(O[kb], need, kb, P, row.len, &a) : zsd_verdict(O[kb], need, kb, P, row.len, &a, &b);
        s_a = a; s_b = b;
    }
    __syncthreads();
    if (s_verdict != kZsdOk) {
        if (tid == 0) res[f] = ZdSmallDecResult{s_verdict, s_a, s_b, 0u};
        return;
    }

    // ---- 5. bytes: a lane per byte of the records (the host has read the first 8)
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(row.dst) & 15);
    if constexpr (kHilbert) {
        // the image starts out zero.  First the 8 length bytes of every record the text reaches: the lowest bad record and their number
        // bound the scan positions that get colours (hzd_cut).  Then the colour bytes of those positions, each to its place in the image.
        const uint32_t records = hzd_records(O[kb], need);
        for (uint32_t i = tid; i < img_room / 16u; i += kZsdThreads) reinterpret_cast<uint4 *>(img)[i] = make_uint4(0u, 0u, 0u, 0u);
        bool back = false;
        for (uint32_t j = tid; j < 8u * records; j += kZsdThreads) {
            const uint32_t px = j >> 3, rr = j & 7u;
            uint8_t v = 0;
            if (!zsd_byte(pairs, O, kb, 11u * px + rr, hops, &v)) { back = true; break; }
            if (!zsd_record_byte_ok(rr, v)) atomicMin(&s_bad, px);
        }
        if (back) atomicOr(&s_back, 1u);
        __syncthreads();
        const uint32_t cut = hzd_cut(records, s_bad);
        for (uint32_t j = tid; j < 3u * cut && !s_back; j += kZsdThreads) {
            const uint32_t px = j / 3u, ch = j - 3u * px;
            uint8_t v = 0;
            if (!zsd_byte(pairs, O, kb, 11u * px + 8u + ch, hops, &v)) { back = true; break; }
            uint32_t x, y;
            sc.xy(px, x, y);
            img[phase + 3u * (y * row.w + x) + ch] = v;
        }
        if (back) atomicOr(&s_back, 1u);
        __syncthreads();
        if (s_back) {
            if (tid == 0) res[f] = ZdSmallDecResult{kZsdHandedBack, 0u, 0u, 0u};
            return;
        }
    } else {
        bool back = false;
        for (uint32_t t = 8u + tid; t < need; t += kZsdThreads) {
            uint8_t v = 0;
            if (!zsd_byte(pairs, O, kb, t, hops, &v)) { back = true; break; }
            const uint32_t j = t - 8u, px = j / 11u, rr = j - 11u * px;
            if (rr >= 8u) img[phase + 3u * px + (rr - 8u)] = v;
            else if (!zsd_record_byte_ok(rr, v)) atomicMin(&s_bad, px);
        }
        if (back) atomicOr(&s_back, 1u);
        __syncthreads();
        if (s_back || s_bad < n) {
            if (tid == 0) res[f] = s_back ? ZdSmallDecResult{kZsdHandedBack, 0u, 0u, 0u} : ZdSmallDecResult{kZsdBadRecord, s_bad, 0u, 0u};
            return;
        }
    }

    // ---- 6. the image, whole: 16-byte stores where the address allows, not a byte outside 3 w h
    uint8_t *__restrict__ dst = row.dst;
    const uint32_t len = 3u * n, to16 = (16u - phase) & 15u, head = len < to16 ? len : to16, body = (len - head) / 16u;
    for (uint32_t i = tid; i < head; i += kZsdThreads) dst[i] = img[phase + i];
    for (uint32_t j = tid; j < body; j += kZsdThreads)
        *reinterpret_cast<uint4 *>(dst + head + 16u * j) = *reinterpret_cast<const uint4 *>(img + phase + head + 16u * j);
    for (uint32_t i = head + 16u * body + tid; i < len; i += kZsdThreads) dst[i] = img[phase + i];
    if (tid == 0) res[f] = ZdSmallDecResult{kZsdOk, 0u, 0u, 0u};
}

__global__ __launch_bounds__(kZsdThreads) void k_zd_small_dec(const ZdSmallDecRow *__restrict__ rows, uint32_t lds_bytes, uint32_t hops, uint32_t rounds,
                                                              ZdSmallDecResult *__restrict__ res) {
    const ZdSmallDecRow row = rows[blockIdx.x];
    zsd_frame<false>(row, blockIdx.x, lds_bytes, hops, rounds, Scan{}, res);
}

__global__ __launch_bounds__(kZsdThreads) void k_hz_small_dec(const ZdSmallDecRow *__restrict__ rows, const HilbertLut *__restrict__ lut, uint32_t lds_bytes, uint32_t hops,
                                                              uint32_t rounds, ZdSmallDecResult *__restrict__ res) {
    __shared__ uint16_t s_l4[1024];
    __shared__ uint8_t s_l1[16];
    const ZdSmallDecRow row = rows[blockIdx.x];
    const uint32_t w = row.w, h = row.h;
    const uint32_t order = (w == h && w >= 2 && !(w & (w - 1))) ? (uint32_t)__builtin_ctz(w) : 0u;   // (pow2_order, k_hilbert.hip)
    const Scan sc = load_scan(w, h, order, order ? lut : nullptr, s_l4, s_l1);
    zsd_frame<true>(row, blockIdx.x, lds_bytes, hops, rounds, sc, res);
}

uint32_t zd_small_dec_lds_max() { return kZsdLdsMax; }
uint32_t hz_small_dec_lds_max() { return kHzdLdsMax; }

int zd_small_dec_run(Ctx *c, const ZdSmallDecRow *rows_d, uint32_t frames, uint32_t lds_bytes, uint32_t hops, uint32_t rounds, ZdSmallDecResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (!lds_bytes || lds_bytes > kZsdLdsMax || (lds_bytes & 15) || !hops || !rounds) return c->fail(CNIIC_ERR_BAD_ARG, "zd_small_dec: LDS or caps outside the route");
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_zd_small_dec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZsdLdsMax));
    hipLaunchKernelGGL(k_zd_small_dec, dim3(frames), dim3(kZsdThreads), lds_bytes, c->stream, rows_d, lds_bytes, hops, rounds, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

int hz_small_dec_run(Ctx *c, const ZdSmallDecRow *rows_d, uint32_t frames, uint32_t lds_bytes, uint32_t hops, uint32_t rounds, ZdSmallDecResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (!lds_bytes || lds_bytes > kHzdLdsMax || (lds_bytes & 15) || !hops || !rounds) return c->fail(CNIIC_ERR_BAD_ARG, "hz_small_dec: LDS or caps outside the route");
    const HilbertLut *lut = nullptr;
    CNIIC_TRY(hilbert_lut(c, &lut));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hz_small_dec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHzdLdsMax));
    hipLaunchKernelGGL(k_hz_small_dec, dim3(frames), dim3(kZsdThreads), lds_bytes, c->stream, rows_d, lut, lds_bytes, hops, rounds, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
