// k_rle_small.hip -- `hilbert(rle)` and `hilbert(rle(d))` of SMALL frames (at most kRleSmallMaxPx pixels), one workgroup per frame, any
// number of frames in one launch (cniic_codec_encode_batch_var / cniic_codec_measure_batch; codec.cpp rle_small_encode).  Such a frame
// needs no tree and no K-means: the block goes from the pixels to the finished stream, the 8-byte (w, h) header included, without the host:
//   a. gather: a lane per scan position (Scan::xy as k_delta_small.hip sets it up), the pixel read byte-wise, its key r << 16 | g << 8 | b
//   b. L(i), the length of the run that would start at i, for every i (rs_run_len, rle_small.hpp: k_rla_len_maps' rule bit for bit)
//   c. the chain of true run starts 0, L(0), L(0) + L(L(0)), ... in pieces of kRleSmallPiece positions: p -> p + L(p) doubled 8 times
//      per piece (every step moves on by >= 1, so 256 steps leave the piece) gives, for every entry offset, the offset at which the chain
//      enters the next piece; ONE lane carries the entry through the at most 64 pieces; one lane per piece marks the starts from its
//      entry, at most 256 steps
//   d. a block prefix sum of the marks gives every run its record index; a start's run is L(start) long; its colour is the rounded
//      average of its keys in integers (rs_round)
//   e. the record's three words, stored straight into the frame's 16-byte aligned slot; the result row holds {runs, 8 + 12 runs}
// No block waits for another, every loop is bounded by a constant or by the frame's pixel count.
// LDS: 8 bytes per pixel of the launch's largest frame rounded up to a power of two (at least one piece): 128 KiB at the bound, by phase
//   a-e  keys u32 [cap]
//   b-e  L u8 [cap]
//   c    doubled pointers u16 [cap]
//   c-d  marks u8 [cap]
// beside the 2^n scan's tables (2064 bytes), the pieces' entries (64 bytes) and the scan's words.
#include "common.hpp"
#include "hilbert_scan.hpp"
#include "rle_small.hpp"

namespace cniic {

constexpr int kRsThreads = 1024;
constexpr uint32_t kRsPer = kRleSmallMaxPx / kRsThreads;        // positions per thread at the bound
constexpr uint32_t kRsPieces = kRleSmallMaxPx / kRleSmallPiece;   // 64
constexpr uint32_t kRsMinCap = kRleSmallPiece;
static_assert(kRleSmallMaxPx % kRsThreads == 0 && kRsThreads % kRleSmallPiece == 0, "a thread's positions q * kRsThreads + tid keep its offset in the piece");
static_assert(kRleSmallPiece == 256 && kRleSmallMaxRun < kRleSmallPiece, "8 doublings leave a piece; a run enters at most the next piece");

// bytes of dynamic LDS for frames of at most cap_px pixels (a power of two)
static uint32_t rs_lds_bytes(uint32_t cap_px) { return std::max(cap_px, kRsMinCap) * 8; }
static_assert(kRleSmallMaxPx * 8 + 2048 + 16 + kRsPieces + 256 <= 160 * 1024, "the largest routed frame, the 2^n scan tables, the entries and the scan's words fit one CU's LDS");

// exclusive scan over the block's 1024 threads; s_w[16] = the sum.  s_w: 17 words
__device__ __forceinline__ uint32_t rs_block_scan(uint32_t v, uint32_t *s_w) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int w = 0; w < kRsThreads / 64; w++) { const uint32_t t = s_w[w]; s_w[w] = run; run += t; }
        s_w[kRsThreads / 64] = run;
    }
    __syncthreads();
    return s_w[wv] + inc - v;
}

__global__ __launch_bounds__(kRsThreads) void k_rle_small(const RleSmallRow *__restrict__ rows, uint32_t cap_px, const HilbertLut *__restrict__ lut, double T, int mode,
                                                          uint8_t *__restrict__ scratch, uint64_t sstride, RleSmallResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t rs_lds[];
    __shared__ uint32_t s_scan[kRsThreads / 64 + 1];
    __shared__ uint16_t s_l4[1024];
    __shared__ uint8_t s_l1[16];
    __shared__ uint8_t s_ent[kRsPieces];
    const uint32_t cap = max(cap_px, kRsMinCap);
    uint32_t *s_key = reinterpret_cast<uint32_t *>(rs_lds);      // [cap]
    uint16_t *s_nx = reinterpret_cast<uint16_t *>(s_key + cap);  // [cap]
    uint8_t *s_len = reinterpret_cast<uint8_t *>(s_nx + cap);    // [cap]
    uint8_t *s_mark = s_len + cap;                               // [cap]
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const RleSmallRow row = rows[f];
    const uint32_t w = row.w, h = row.h, n = w * h;              // 1 .. cap_px
    const uint32_t npieces = (n + kRleSmallPiece - 1) / kRleSmallPiece, ncov = npieces * kRleSmallPiece;   // <= cap
    uint32_t *__restrict__ slot = reinterpret_cast<uint32_t *>(scratch + (uint64_t)f * sstride);

    // ---- a. gather
    {
        const uint32_t order = (w == h && w >= 2 && !(w & (w - 1))) ? (uint32_t)__builtin_ctz(w) : 0u;   // (pow2_order, k_hilbert.hip)
        const Scan sc = load_scan(w, h, order, order ? lut : nullptr, s_l4, s_l1);
        for (uint32_t d = tid; d < n; d += kRsThreads) {
            uint32_t x, y;
            sc.xy(d, x, y);
            const uint8_t *p = row.src + 3ull * ((uint64_t)y * w + x);
            s_key[d] = rs_key(p[0], p[1], p[2]);
        }
    }
    __syncthreads();

    // ---- b. the run length of every start; past the frame's end a position steps on by 1
    for (uint32_t i = tid; i < ncov; i += kRsThreads) {
        const uint32_t len = i < n ? rs_run_len(s_key, i, n, T, mode) : 1u;
        s_len[i] = (uint8_t)len;
        s_nx[i] = (uint16_t)((i & (kRleSmallPiece - 1)) + len);   // offset in the piece; >= 256: offset - 256 in the next
        s_mark[i] = 0;
    }
    __syncthreads();

    // ---- c. the pieces' maps by doubling, the entries, the marks
    for (int r = 0; r < 8; r++) {
        uint32_t nx[kRsPer];
#pragma unroll
        for (uint32_t q = 0; q < kRsPer; q++) {
            const uint32_t i = tid + q * kRsThreads;
            if (i < ncov) {
                nx[q] = s_nx[i];
                if (nx[q] < kRleSmallPiece) nx[q] = s_nx[(i & ~(kRleSmallPiece - 1)) + nx[q]];
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < kRsPer; q++) {
            const uint32_t i = tid + q * kRsThreads;
            if (i < ncov) s_nx[i] = (uint16_t)nx[q];
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t e = 0;
        for (uint32_t k = 0; k < npieces; k++) { s_ent[k] = (uint8_t)e; e = s_nx[k * kRleSmallPiece + e] - kRleSmallPiece; }   // <= 254
    }
    __syncthreads();
    if ((tid & 15) == 0 && (tid >> 4) < npieces) {   // a lane per piece, four to a wave
        const uint32_t base = (tid >> 4) * kRleSmallPiece;
        for (uint32_t p = s_ent[tid >> 4]; p < kRleSmallPiece && base + p < n; p += s_len[base + p]) s_mark[base + p] = 1;
    }
    __syncthreads();

    // ---- d. record indices: thread t holds the `per` positions from t * per on
    const uint32_t per = cap / kRsThreads ? cap / kRsThreads : 1u;   // <= 16
    const uint32_t first = tid * per;
    uint32_t starts = 0, nstarts = 0;
#pragma unroll
    for (uint32_t q = 0; q < kRsPer; q++) {
        const uint32_t i = first + q;
        if (q < per && i < n && s_mark[i]) { starts |= 1u << q; nstarts++; }
    }
    uint32_t rec = rs_block_scan(nstarts, s_scan);
    const uint32_t runs = s_scan[kRsThreads / 64];   // 1 .. n

    // ---- e. records: three whole words each behind the two of the header
    for (uint32_t m = starts; m; rec++) {
        const uint32_t q = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        const uint32_t i = first + q, cnt = s_len[i];
        uint32_t c0, c1, c2;
        if (mode == kRsModeExact) {   // the run's own colour
            const uint32_t k = s_key[i];
            c0 = (k >> 16) & 255u; c1 = (k >> 8) & 255u; c2 = k & 255u;
        } else {
            uint32_t s0 = 0, s1 = 0, s2 = 0;
            for (uint32_t j = 0; j < cnt; j++) {
                const uint32_t k = s_key[i + j];
                s0 += (k >> 16) & 255u; s1 += (k >> 8) & 255u; s2 += k & 255u;
            }
            c0 = rs_round(s0, cnt); c1 = rs_round(s1, cnt); c2 = rs_round(s2, cnt);
        }
        uint32_t wd[3];
        rs_record_words(cnt, c0, c1, c2, wd);
        uint32_t *o = slot + 2 + 3 * (size_t)rec;
        o[0] = wd[0]; o[1] = wd[1]; o[2] = wd[2];
    }
    if (tid == 0) {
        slot[0] = w; slot[1] = h;
        res[f] = RleSmallResult{runs, (uint32_t)rs_stream_bytes(runs)};
    }
}

int rle_small_run(Ctx *c, const RleSmallRow *rows_d, uint32_t frames, uint32_t max_px, double T, int mode, uint8_t *scratch_d, uint64_t sstride, RleSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kRleSmallMaxPx || sstride < rs_stride(max_px) || (sstride & 15))
        return c->fail(CNIIC_ERR_BAD_ARG, "rle_small: frame size or scratch outside the route");
    const HilbertLut *lut = nullptr;
    CNIIC_TRY(hilbert_lut(c, &lut));
    uint32_t cap_px = 1;
    while (cap_px < max_px) cap_px <<= 1;
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_rle_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_lds_bytes(kRleSmallMaxPx)));
    hipLaunchKernelGGL(k_rle_small, dim3(frames), dim3(kRsThreads), rs_lds_bytes(cap_px), c->stream, rows_d, cap_px, lut, T, mode, scratch_d, sstride, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
