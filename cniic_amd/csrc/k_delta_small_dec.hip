// k_delta_small_dec.hip -- the decode of SMALL `delta` frames (at most kDeltaSmallDecMaxPx pixels), one workgroup per frame, any number of
// frames in one launch (cniic_codec_decode_batch / cniic_codec_measure_batch; codec.cpp delta_small_decode).  Every frame's decoder has
// been parsed into its table of leaves, which lies in HBM -- by k_small_trieparse (k_small_trie.hip) for streams in device memory, by the
// host (huff_parse_leaves) otherwise; the block goes from the payload to the pixels in place:
//   a. stage: the first ceil(19 n / 8) bytes of the payload from any byte alignment into LDS, as big-endian words
//   b. symbols, self-synchronising: the payload's bits in one subsequence per lane; every lane decodes from where it assumes a code starts
//      until it crosses into the next subsequence, lanes whose predecessor ended elsewhere decode again from there, until a block-wide
//      vote sees no change (lane 0 is right from the first round); a frame that has not settled after max_rounds is handed back (status 2).
//      Then a prefix sum of the lanes' symbol counts, and every lane decodes its subsequence once more into its symbols' places
//   c. lookup: a first-level table over a window's top 11 bits in LDS (built by the block), a binary search in the leaves' codes in HBM
//      for the codes that are longer
//   d. FromDiff: a block-wide inclusive scan per channel from START = 0; a sum outside 0..255 fails the frame (status 3)
//   e. pixels: position d to Scan::xy(d) of a row-major image in LDS, then to the destination: bytes up to its 16-byte boundary, 16-byte
//      stores, bytes behind.  Nothing is stored before the image is complete: a frame that fails leaves its destination untouched.
// Dynamic LDS, by phase (px = the launch's largest frame rounded up to 256 pixels; at 16 384: 54.0 + 64 KiB):
//   region A   a-c  payload words (ceil(19 px / 32) + 2) | first-level table (2049 + 2048 words)     e  the image (3 px + 32 bytes)
//   region B   b    during the settle rounds a larger lookup table, 2^floor(log2 px) key | length words (codes of nearly one length settle
//                   one lane per round, and a round must not wait for HBM)        b-e  one word per symbol: its key, from d on its colour
// The full table of leaves (a code word and a key | length word per leaf, up to 2^19 leaves of a hostile stream) stays in HBM.  No block
// waits for another, and no loop is without a bound: a pass advances by a code of at least one bit per step.
//
// Small `hufman` and `cluster-colors` frames (k_huf_small_dec; codec.cpp delta_small_decode under the other kind) are the same body with
// RGB symbols: phases a-c as they are -- a key's 27 bits hold a 24-bit colour r << 16 | g << 8 | b --, no FromDiff (d is skipped, so there
// is no range status) and no scan: position d is pixel d.  Nothing is stored before the image is complete there either.
#include "common.hpp"
#include "hilbert_scan.hpp"
#include "delta_small_dec.hpp"
#include "huf_small.hpp"

namespace cniic {

constexpr uint32_t kDsdT1 = 1u << kDsdT1Bits;
constexpr uint32_t kDsdPer = kDeltaSmallDecMaxPx / kDsdLanes;   // positions per lane at the bound
static_assert(kDsdPer == 16, "the loops over a lane's positions below are unrolled 16 times");

static uint32_t dsd_cap_px(uint32_t max_px) { return (max_px + 255) & ~255u; }
static uint32_t dsd_pay_words(uint32_t cap_px) { return (kDeltaSmallMaxCodeLen * cap_px + 31) / 32 + 2; }
static uint32_t dsd_region_a(uint32_t cap_px) {
    const uint32_t dec = 4 * (dsd_pay_words(cap_px) + 2 * kDsdT1 + 1), img = 3 * cap_px + 32;
    return (std::max(dec, img) + 15) & ~15u;
}
static uint32_t dsd_lds_bytes(uint32_t cap_px) { return dsd_region_a(cap_px) + 4 * cap_px; }
static_assert((kDeltaSmallMaxCodeLen * kDeltaSmallDecMaxPx / 32 + 2 + 2 * kDsdT1 + 1) * 4 + 16 + 4 * kDeltaSmallDecMaxPx + 4096 + 3 * 17 * 4 + 2048 + 16 <= 160 * 1024,
              "the largest routed frame, the lanes' ends, the scans' words and the 2^n scan tables fit one CU's LDS");

// exclusive scan of three values over the block's 1024 lanes; s_w[ch][16] = the sums
__device__ __forceinline__ void dsd_block_scan3(int32_t v[3], int32_t s_w[3][kDsdLanes / 64 + 1]) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int32_t inc[3] = {v[0], v[1], v[2]};
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const int32_t t = __shfl_up(inc[ch], d);
            if (lane >= (uint32_t)d) inc[ch] += t;
        }
    if (lane == 63)
        for (int ch = 0; ch < 3; ch++) s_w[ch][wv] = inc[ch];
    __syncthreads();
    if (threadIdx.x < 3) {
        int32_t run = 0;
        for (uint32_t w = 0; w < kDsdLanes / 64; w++) { const int32_t t = s_w[threadIdx.x][w]; s_w[threadIdx.x][w] = run; run += t; }
        s_w[threadIdx.x][kDsdLanes / 64] = run;
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ch++) v[ch] = s_w[ch][wv] + inc[ch] - v[ch];
}

// one frame, from the payload to the pixels in place.  kDiff: the symbols are differences along the scan (`delta`); otherwise they are the
// pixels' colours in row-major order (`hufman`, `cluster-colors`)
template <bool kDiff>
__device__ __forceinline__ void dsd_frame(const DeltaSmallDecRow *__restrict__ rows, uint32_t cap_px, uint32_t max_rounds, const HilbertLut *__restrict__ lut,
                                          uint32_t *__restrict__ status) {
    extern __shared__ __align__(16) uint8_t dsd_lds[];
    __shared__ uint32_t s_end[kDsdLanes];
    __shared__ int32_t s_scan[3][kDsdLanes / 64 + 1];
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const DeltaSmallDecRow row = rows[f];
    const uint32_t w = row.w, h = row.h, n = w * h, L = row.leaves;   // 1 <= n <= cap_px, 1 <= L
    const uint32_t pay_words = (kDeltaSmallMaxCodeLen * cap_px + 31) / 32 + 2;
    uint32_t *s_pay = reinterpret_cast<uint32_t *>(dsd_lds);           // [pay_words]
    uint32_t *s_t1 = s_pay + pay_words;                                // [kDsdT1 + 1]
    uint32_t *s_t1k = s_t1 + kDsdT1 + 1;                               // [kDsdT1]
    const uint32_t dec = 4 * (pay_words + 2 * kDsdT1 + 1), img = 3 * cap_px + 32;
    uint32_t *s_sym = reinterpret_cast<uint32_t *>(dsd_lds + (((dec > img ? dec : img) + 15) & ~15u));   // [cap_px]
    const uint32_t *__restrict__ code = row.code, *__restrict__ keylen = row.keylen;

    Scan sc{};
    if constexpr (kDiff) {
        __shared__ uint16_t s_l4[1024];
        __shared__ uint8_t s_l1[16];
        const uint32_t order = (w == h && w >= 2 && !(w & (w - 1))) ? (uint32_t)__builtin_ctz(w) : 0u;   // (pow2_order, k_hilbert.hip)
        sc = load_scan(w, h, order, order ? lut : nullptr, s_l4, s_l1);
    }

    if (L == 1) {   // one symbol: zero-length codes and no payload (huf.rs:140-142): the frame is filled, not decoded
        const uint32_t key0 = dsd_keylen_key(keylen[0]);
        for (uint32_t d = tid; d < n; d += kDsdLanes) s_sym[d] = key0;
    } else {
        // ---- a. the payload
        const uint32_t nst = dsd_stage_bytes(n, row.payload_bytes), b = nst * 8, nw = (nst + 3) / 4;   // nw <= pay_words - 2
        {
            const uintptr_t pa = reinterpret_cast<uintptr_t>(row.payload);
            const uint32_t sh = (uint32_t)(pa & 3);
            const uint32_t *__restrict__ g = reinterpret_cast<const uint32_t *>(pa - sh);
            const uint32_t glast = nst ? (sh + nst - 1) >> 2 : 0;   // the last aligned word that holds a byte of the payload
            for (uint32_t i = tid; i < nw; i += kDsdLanes) {
                uint32_t v = g[i] >> (8 * sh);
                if (sh && i + 1 <= glast) v |= g[i + 1] << (32 - 8 * sh);
                s_pay[i] = __builtin_bswap32(v);
            }
            if (tid < 2) s_pay[nw + tid] = 0u;
        }
        // ---- c. the first-level table
        for (uint32_t p = tid; p <= kDsdT1; p += kDsdLanes) dsd_t1_entry(code, keylen, L, p, s_t1, s_t1k);
        __syncthreads();
        // the larger table of the settle rounds, where the symbols go afterwards: as many entries as the launch's frames have room for
        const uint32_t big_bits = 31 - (uint32_t)__builtin_clz(cap_px);   // 2^big_bits <= cap_px
        const uint32_t *s_big = big_bits > kDsdT1Bits && row.max_len > kDsdT1Bits ? s_sym : nullptr;
        if (s_big) {
            for (uint32_t p = tid; p < (1u << big_bits); p += kDsdLanes) s_sym[p] = dsd_big_entry(code, keylen, s_t1, s_t1k, big_bits, p);
            __syncthreads();
        }
        // ---- b. every lane's subsequence, until the starts agree with the ends
        const uint32_t sub = dsd_sub_bits(b), next = dsd_bound(tid + 1, sub, b);
        uint32_t start = dsd_bound(tid, sub, b), end = 0;
        uint32_t count = dsd_pass(s_pay, b, code, keylen, s_t1, s_t1k, s_big, big_bits, start, next, &end, nullptr, 0, 0);
        s_end[tid] = end;
        bool settled = false;
        for (uint32_t round = 1;; round++) {
            __syncthreads();
            const uint32_t from = tid ? s_end[tid - 1] : 0u;
            const bool moved = from != start;
            if (!__syncthreads_or(moved)) { settled = true; break; }   // (its barrier: every lane has read its predecessor's end)
            if (round >= max_rounds) break;
            if (moved) {
                start = from;
                count = dsd_pass(s_pay, b, code, keylen, s_t1, s_t1k, s_big, big_bits, start, next, &end, nullptr, 0, 0);
                s_end[tid] = end;
            }
        }
        if (!settled) {
            if (tid == 0) status[f] = kDsdUnsettled;
            return;
        }
        int32_t cnt[3] = {(int32_t)count, 0, 0};
        dsd_block_scan3(cnt, s_scan);
        if ((uint32_t)s_scan[0][kDsdLanes / 64] < n) {   // the bits ran out before the n-th symbol
            if (tid == 0) status[f] = kDsdShort;
            return;
        }
        // (dsd_block_scan3's barriers: no lane reads the larger table any more)
        if ((uint32_t)cnt[0] < n) (void)dsd_pass(s_pay, b, code, keylen, s_t1, s_t1k, nullptr, 0, start, next, &end, s_sym, (uint32_t)cnt[0], n);
    }
    __syncthreads();

    if constexpr (kDiff) {
    // ---- d. FromDiff: consecutive positions per lane
    const uint32_t per = (n + kDsdLanes - 1) / kDsdLanes, d0 = tid * per;   // per <= 16
    int32_t run[3] = {0, 0, 0};
#pragma unroll
    for (uint32_t q = 0; q < kDsdPer; q++) {
        const uint32_t d = d0 + q;
        if (q < per && d < n) {
            const uint32_t key = s_sym[d];
            run[0] += dsd_diff(key, 0); run[1] += dsd_diff(key, 1); run[2] += dsd_diff(key, 2);
        }
    }
    dsd_block_scan3(run, s_scan);
    bool bad = false;
#pragma unroll
    for (uint32_t q = 0; q < kDsdPer; q++) {
        const uint32_t d = d0 + q;
        if (q < per && d < n) {
            const uint32_t key = s_sym[d];
            run[0] += dsd_diff(key, 0); run[1] += dsd_diff(key, 1); run[2] += dsd_diff(key, 2);
            bad |= !dsd_in_range(run[0]) || !dsd_in_range(run[1]) || !dsd_in_range(run[2]);
            s_sym[d] = (uint32_t)(run[0] & 255) | ((uint32_t)(run[1] & 255) << 8) | ((uint32_t)(run[2] & 255) << 16);
        }
    }
    if (__syncthreads_or(bad)) {   // (its barrier: the colours are all there, and region A is dead)
        if (tid == 0) status[f] = kDsdRange;
        return;
    }
    }   // (RGB symbols: the barrier behind the symbols has made region A dead)

    // ---- e. the image in LDS, at the destination's offset within 16 bytes, then out
    uint8_t *__restrict__ dst = row.dst;
    const uint32_t a16 = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
    uint8_t *s_img = dsd_lds + a16;
    for (uint32_t d = tid; d < n; d += kDsdLanes) {
        const uint32_t v = s_sym[d];
        if constexpr (kDiff) {
            uint32_t x, y;
            sc.xy(d, x, y);
            uint8_t *o = s_img + 3 * (y * w + x);
            o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
        } else {   // position d is pixel d, the key r << 16 | g << 8 | b
            hs_pixel_bytes(v, s_img + 3 * d);
        }
    }
    __syncthreads();
    const uint32_t len = 3 * n, to16 = (16 - a16) & 15, head = len < to16 ? len : to16, body = (len - head) / 16;
    for (uint32_t i = tid; i < head; i += kDsdLanes) dst[i] = s_img[i];
    for (uint32_t j = tid; j < body; j += kDsdLanes)
        *reinterpret_cast<uint4 *>(dst + head + 16 * j) = *reinterpret_cast<const uint4 *>(s_img + head + 16 * j);
    for (uint32_t i = head + 16 * body + tid; i < len; i += kDsdLanes) dst[i] = s_img[i];
    if (tid == 0) status[f] = kDsdOk;
}

__global__ __launch_bounds__(kDsdLanes) void k_delta_small_dec(const DeltaSmallDecRow *__restrict__ rows, uint32_t cap_px, uint32_t max_rounds,
                                                               const HilbertLut *__restrict__ lut, uint32_t *__restrict__ status) {
    dsd_frame<true>(rows, cap_px, max_rounds, lut, status);
}

__global__ __launch_bounds__(kDsdLanes) void k_huf_small_dec(const DeltaSmallDecRow *__restrict__ rows, uint32_t cap_px, uint32_t max_rounds, uint32_t *__restrict__ status) {
    dsd_frame<false>(rows, cap_px, max_rounds, nullptr, status);
}

int delta_small_dec_run(Ctx *c, const DeltaSmallDecRow *rows_d, uint32_t frames, uint32_t max_px, uint32_t max_rounds, uint32_t *status_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kDeltaSmallDecMaxPx || max_rounds == 0) return c->fail(CNIIC_ERR_BAD_ARG, "delta_small_dec: frame size or rounds outside the route");
    const HilbertLut *lut = nullptr;
    CNIIC_TRY(hilbert_lut(c, &lut));
    const uint32_t cap_px = dsd_cap_px(max_px);
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_delta_small_dec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dsd_lds_bytes(kDeltaSmallDecMaxPx)));
    hipLaunchKernelGGL(k_delta_small_dec, dim3(frames), dim3(kDsdLanes), dsd_lds_bytes(cap_px), c->stream, rows_d, cap_px, max_rounds, lut, status_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

int huf_small_dec_run(Ctx *c, const DeltaSmallDecRow *rows_d, uint32_t frames, uint32_t max_px, uint32_t max_rounds, uint32_t *status_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kDeltaSmallDecMaxPx || max_rounds == 0) return c->fail(CNIIC_ERR_BAD_ARG, "huf_small_dec: frame size or rounds outside the route");
    const uint32_t cap_px = dsd_cap_px(max_px);
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_huf_small_dec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dsd_lds_bytes(kDeltaSmallDecMaxPx)));
    hipLaunchKernelGGL(k_huf_small_dec, dim3(frames), dim3(kDsdLanes), dsd_lds_bytes(cap_px), c->stream, rows_d, cap_px, max_rounds, status_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
