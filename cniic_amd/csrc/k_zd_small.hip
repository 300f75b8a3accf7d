// k_zd_small.hip -- `zip(dict)` of SMALL frames (at most kZdSmallMaxPx pixels), one workgroup per frame, any number of frames in one
// launch (cniic_codec_encode_batch_var / cniic_codec_measure_batch; codec.cpp zd_small_encode).  Such a frame never fills the dictionary's
// 65 279 symbols, so the single call codes all of it in the host's serial walk.  Here the coder stays serial inside a frame, but most of
// its dependent chain of memory trips is taken away (zd_small.hpp has the arithmetic and argues the repair rule):
//   the text is never written out: the frame's pixels lie in LDS, zs_text_byte gives byte i
//   the trie is a table of 8-byte edge slots in HBM, one table per frame, zeroed before the launch
//   per window of kZsWindow text positions
//     speculate  a lane per position walks the table as it stands, at most `spec` bytes deep: the W walks are independent, the window
//                pays the latency of one
//     commit     wave 0 follows DictEncoder::next_pair in LDS: a match is the speculated one (a walk the cap cut is finished first, every
//                lane issuing the same loads) unless an entry this window made is longer and spells the text there (lanes over the list)
//     flush      a lane per entry inserts the window's entries, edges claimed by 64-bit compare-and-swap
//   a frame with a match longer than `giveup` bytes is handed back (verdict kZsHandedBack): the workers code it
// No block waits for another.  The table is read with device-scope loads and written with device-scope atomics only, so a window sees
// what the windows before it inserted whichever wave did it.  LDS: 3 bytes a pixel of the launch's largest frame, 2560 bytes of window,
// 1290 of list.
//
// k_hz_small is the same body for Hilbert { compress: Zip } (cniic_hilbert_zip_encode_batch_var / cniic_hilbert_zip_measure_batch;
// codec.cpp hz_small_encode): the text kind of hz_small.hpp over the frame's pixels in scan order, and 2064 bytes of scan tables more.
#include "common.hpp"
#include "hilbert_scan.hpp"
#include "hz_small.hpp"
#include "zd_small.hpp"

namespace cniic {

constexpr int kZsThreads = kZsWindow;   // a lane per position of the window
static_assert(kZsThreads % 64 == 0 && kZsListCap <= kZsThreads, "a lane per entry in the flush");

// bytes of dynamic LDS for frames of at most max_px pixels
static uint32_t zs_lds_bytes(uint32_t max_px) { return (3 * max_px + 15) & ~15u; }
static_assert(3 * kZdSmallMaxPx + kZsWindow * 10 + kZsListCap * 10 + 256 <= 160 * 1024, "the largest routed frame, the window and its list fit one CU's LDS");
static_assert(kHzSmallMaxPx == kZdSmallMaxPx && 3 * kHzSmallMaxPx + kZsWindow * 10 + kZsListCap * 10 + 256 + kHzScanLds <= 160 * 1024,
              "... and so they do beside the 2^n scan's tables");
static_assert(sizeof(HilbertLut) == kHzScanLds, "the scan tables' bytes");

struct ZsDevMem {
    static __device__ __forceinline__ uint64_t load(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint64_t cas(uint64_t *p, uint64_t expect, uint64_t want) {
        __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
    static __device__ __forceinline__ uint64_t fetch_or(uint64_t *p, uint64_t bits) { return __hip_atomic_fetch_or(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct ZsWaveLanes {
    template <class F>
    static __device__ __forceinline__ uint64_t best(F f) {
        uint64_t b = f(threadIdx.x & 63u, 64u);
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const uint64_t o = __shfl_xor(b, d);
            b = o > b ? o : b;
        }
        return b;
    }
    static __device__ __forceinline__ bool first() { return (threadIdx.x & 63u) == 0; }
};

// One frame from its text to its pairs: the windows, the commit wave and the flush, whatever the text's kind.  Every thread of the block
// calls it behind the barrier that made the text readable; the coder's last state comes back on every thread.
template <class Text>
__device__ __forceinline__ ZsState zs_code_frame(const Text &t, uint64_t *__restrict__ tab, uint32_t bits, uint32_t spec, uint32_t giveup, uint32_t *__restrict__ out) {
    __shared__ uint16_t s_sym[kZsWindow], s_len[kZsWindow], s_depth[kZsWindow], s_esym[kZsListCap];
    __shared__ uint32_t s_node[kZsWindow], s_estart[kZsListCap], s_elen[kZsListCap];
    __shared__ ZsState s_st;
    const uint32_t tid = threadIdx.x;
    const ZsWindow win{s_sym, s_len, s_depth, s_node, s_estart, s_elen, s_esym};
    if (tid == 0) s_st = zs_state_begin();
    __syncthreads();

    for (;;) {   // a window; at most N of them: each commits its first position at least
        const ZsState st0 = s_st;
        if (st0.done) break;
        const uint32_t base = zs_need(st0);
        // ---- speculate
        if (base + tid < t.N) {
            ZsWalk s = zs_walk_begin(t, base + tid);
            zs_walk<ZsDevMem>(tab, bits, t, base + tid, spec, s);
            zs_window_put(win, tid, s);
        }
        __syncthreads();
        // ---- commit
        if (tid < 64) {
            ZsState st = st0;
            zs_commit<ZsDevMem, ZsWaveLanes>(tab, bits, t, win, base, kZsWindow, kZsLimit, giveup, out, st);
            if (tid == 0) s_st = st;
        }
        __syncthreads();
        // ---- flush
        if (tid < s_st.nlist && !s_st.verdict) zs_insert<ZsDevMem>(tab, bits, t, s_estart[tid], s_elen[tid], s_esym[tid]);
        __threadfence();
        __syncthreads();
    }
    return s_st;
}

__global__ __launch_bounds__(kZsThreads) void k_zd_small(const ZdSmallRow *__restrict__ rows, uint32_t spec, uint32_t giveup, uint64_t *__restrict__ tables, uint32_t bits,
                                                         uint8_t *__restrict__ scratch, uint64_t sstride, ZdSmallResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t zs_px[];
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const ZdSmallRow row = rows[f];
    const uint32_t n = row.w * row.h;   // 1 .. kZdSmallMaxPx
    const ZsText t{zs_px, row.w, row.h, zs_text_len(n)};
    uint64_t *__restrict__ tab = tables + ((uint64_t)f << bits);
    uint32_t *__restrict__ out = reinterpret_cast<uint32_t *>(scratch + (uint64_t)f * sstride);

    for (uint32_t i = tid; i < 3 * n; i += kZsThreads) zs_px[i] = row.src[i];
    __syncthreads();
    const ZsState st = zs_code_frame(t, tab, bits, spec, giveup, out);
    if (tid == 0) res[f] = ZdSmallResult{st.pairs, 4u * st.pairs, st.verdict, st.finished};
}

// Hilbert { compress: Zip } of a small frame: the same coder over the text of hz_small.hpp.  The frame comes into LDS in SCAN order, a
// lane per scan position (load_scan / Scan::xy as k_rle_small.hip sets them up: the tables for a 2^n square, the general walk for every
// other rectangle; a size with an injected scan never comes here), and the 8 raw bytes of the dimensions go in front of the pairs.
__global__ __launch_bounds__(kZsThreads) void k_hz_small(const ZdSmallRow *__restrict__ rows, const HilbertLut *__restrict__ lut, uint32_t spec, uint32_t giveup,
                                                         uint64_t *__restrict__ tables, uint32_t bits, uint8_t *__restrict__ scratch, uint64_t sstride,
                                                         ZdSmallResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t zs_px[];
    __shared__ uint16_t s_l4[1024];
    __shared__ uint8_t s_l1[16];
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const ZdSmallRow row = rows[f];
    const uint32_t w = row.w, h = row.h, n = w * h;   // 1 .. kHzSmallMaxPx
    const HzText t{zs_px, hz_text_len(n)};
    uint64_t *__restrict__ tab = tables + ((uint64_t)f << bits);
    uint32_t *__restrict__ slot = reinterpret_cast<uint32_t *>(scratch + (uint64_t)f * sstride);

    {
        const uint32_t order = (w == h && w >= 2 && !(w & (w - 1))) ? (uint32_t)__builtin_ctz(w) : 0u;   // (pow2_order, k_hilbert.hip)
        const Scan sc = load_scan(w, h, order, order ? lut : nullptr, s_l4, s_l1);
        for (uint32_t d = tid; d < n; d += kZsThreads) {
            uint32_t x, y;
            sc.xy(d, x, y);
            const uint8_t *p = row.src + 3ull * ((uint64_t)y * w + x);
            zs_px[3 * d] = p[0]; zs_px[3 * d + 1] = p[1]; zs_px[3 * d + 2] = p[2];
        }
    }
    __syncthreads();
    const ZsState st = zs_code_frame(t, tab, bits, spec, giveup, slot + kHzHead / 4);
    if (tid == 0) {
        slot[0] = w; slot[1] = h;   // img.dimensions().serialize (hilbertc.rs:27), outside the coder
        res[f] = ZdSmallResult{st.pairs, kHzHead + 4u * st.pairs, st.verdict, st.finished};
    }
}

int zd_small_run(Ctx *c, const ZdSmallRow *rows_d, uint32_t frames, uint32_t max_px, uint32_t spec, uint32_t giveup, uint64_t *tables_d, uint32_t bits, uint8_t *scratch_d,
                 uint64_t sstride, ZdSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kZdSmallMaxPx || bits < zs_table_bits(zs_text_len(max_px)) || bits > 19 || sstride < zs_stride(zs_text_len(max_px)) || (sstride & 15) || !spec || !giveup)
        return c->fail(CNIIC_ERR_BAD_ARG, "zd_small: frame size, table or scratch outside the route");
    CNIIC_HIP_TRY(c, hipMemsetAsync(tables_d, 0, ((uint64_t)frames << bits) * sizeof(uint64_t), c->stream));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_zd_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)zs_lds_bytes(kZdSmallMaxPx)));
    hipLaunchKernelGGL(k_zd_small, dim3(frames), dim3(kZsThreads), zs_lds_bytes(max_px), c->stream, rows_d, spec, giveup, tables_d, bits, scratch_d, sstride, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

int hz_small_run(Ctx *c, const ZdSmallRow *rows_d, uint32_t frames, uint32_t max_px, uint32_t spec, uint32_t giveup, uint64_t *tables_d, uint32_t bits, uint8_t *scratch_d,
                 uint64_t sstride, ZdSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kHzSmallMaxPx || bits < zs_table_bits(hz_text_len(max_px)) || bits > 19 || sstride < hz_stride(hz_text_len(max_px)) || (sstride & 15) || !spec || !giveup)
        return c->fail(CNIIC_ERR_BAD_ARG, "hz_small: frame size, table or scratch outside the route");
    const HilbertLut *lut = nullptr;
    CNIIC_TRY(hilbert_lut(c, &lut));
    CNIIC_HIP_TRY(c, hipMemsetAsync(tables_d, 0, ((uint64_t)frames << bits) * sizeof(uint64_t), c->stream));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hz_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)zs_lds_bytes(kHzSmallMaxPx)));
    hipLaunchKernelGGL(k_hz_small, dim3(frames), dim3(kZsThreads), zs_lds_bytes(max_px), c->stream, rows_d, lut, spec, giveup, tables_d, bits, scratch_d, sstride, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
