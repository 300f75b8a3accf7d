// k_cc_small.hip -- cluster-colors(K <= 256) of SMALL frames (at most kCcSmallMaxPx pixels), one workgroup per frame, any number of
// frames in one launch (cniic_codec_encode_batch_var / cniic_codec_measure_batch; codec.cpp cc_small_encode).  A frame's distinct
// colours, their pixel counts and labels and the K centroids fit in one CU's LDS, so the block goes from the pixels to the palette and
// every pixel's label without leaving it:
//   a. pixels (any byte alignment) -> 24-bit keys in LDS, bitonic sort, unique: the distinct colours in ascending key order with their
//      pixel counts -- the reference's point list and point order (clusterc.rs:21-24)
//   b. kmeans::cluster exactly (kmeans.rs:17-39): labels by position, first point of each chunk as centroid, then brute-force Lloyd with the
//      arithmetic of cc_small.hpp until no point moves (or max_iters)
//   c. every pixel's label by binary search in the sorted colours, u8, at the frame's 16-element-aligned label base
// What follows "every pixel has a label" is frames_tail (codec.cpp).  No block waits for another.
#include "common.hpp"
#include "cc_small.hpp"

namespace cniic {

constexpr int kCcsThreads = 1024;
static_assert(kCcSmallDefaultSeed == kDefaultSeed, "cc_small.hpp restates the library's default seed");
constexpr uint32_t kCcsFixedBytes = (256 + 256 + 4 * 256 + 256) * 4;   // centroids, their constants, four sums per cluster, members

// bytes of dynamic LDS for frames of at most cap_px pixels (cap_px: a power of two): keys u32, weights u16, labels u8, then the fixed part
static uint32_t ccs_lds_bytes(uint32_t cap_px) { return std::max<uint32_t>(cap_px, 4) * 7 + kCcsFixedBytes; }
static_assert(kCcSmallMaxPx * 7 + kCcsFixedBytes + 256 <= 160 * 1024, "the largest routed frame fits one CU's LDS");

__device__ __forceinline__ uint32_t ccs_pixel_key(const uint8_t *__restrict__ src, uint32_t i) {
    const uint8_t *p = src + 3ull * i;
    return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
}

// exclusive scan over the block's 1024 threads; *total (LDS) = the sum.  s_w: 17 words
__device__ __forceinline__ uint32_t ccs_block_scan(uint32_t v, uint32_t *s_w) {
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
        for (int w = 0; w < kCcsThreads / 64; w++) { const uint32_t t = s_w[w]; s_w[w] = run; run += t; }
        s_w[kCcsThreads / 64] = run;
    }
    __syncthreads();
    return s_w[wv] + inc - v;
}

__global__ __launch_bounds__(kCcsThreads) void k_cc_small(const CcSmallRow *__restrict__ rows, uint32_t cap_px, uint32_t K, uint64_t seed, uint64_t max_iters,
                                                          uint8_t *__restrict__ labels_out, uint32_t *__restrict__ cent_out, CcSmallResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t ccs_lds[];
    __shared__ uint32_t s_scan[kCcsThreads / 64 + 1];
    __shared__ uint32_t s_moved, s_reseed, s_active;
    const uint32_t cap = max(cap_px, 4u);
    uint32_t *s_key = reinterpret_cast<uint32_t *>(ccs_lds);                       // [cap]
    uint16_t *s_wt = reinterpret_cast<uint16_t *>(ccs_lds + 4ull * cap);            // [cap]
    uint8_t *s_lab = ccs_lds + 6ull * cap;                                         // [cap]
    uint32_t *s_cent = reinterpret_cast<uint32_t *>(ccs_lds + 7ull * cap);         // [256]
    int32_t *s_cc = reinterpret_cast<int32_t *>(s_cent + 256);                     // [256]
    uint32_t *s_sum = reinterpret_cast<uint32_t *>(s_cc + 256);                    // [256][4]: r, g, b sums weighted, weight
    uint32_t *s_mem = s_sum + 4 * 256;                                             // [256]
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const CcSmallRow row = rows[f];
    const uint32_t npx = row.w * row.h;   // 1 .. cap_px
    const uint8_t *__restrict__ src = row.src;

    // ---- a. load, sort, unique
    uint32_t P = 1;
    while (P < npx) P <<= 1;              // <= cap
    for (uint32_t i = tid; i < P; i += kCcsThreads) s_key[i] = i < npx ? ccs_pixel_key(src, i) : 0xffffffffu;
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (uint32_t t = tid; t < P / 2; t += kCcsThreads) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint32_t u = s_key[lo], v = s_key[hi];
                if ((u > v) == ((lo & k) == 0)) { s_key[lo] = v; s_key[hi] = u; }
            }
        }
    __syncthreads();
    // thread t holds the `per` sorted pixels from t * per on; the heads of runs of one colour are the distinct colours
    const uint32_t per = P > (uint32_t)kCcsThreads ? P / kCcsThreads : 1;   // <= 16
    const uint32_t first = tid * per;
    uint32_t kv[16];
    uint32_t heads = 0, nheads = 0;
    {
        uint32_t prev = first > 0 && first <= npx ? s_key[first - 1] : 0xffffffffu;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t i = first + q;
            const bool live = (uint32_t)q < per && i < npx;
            kv[q] = live ? s_key[i] : 0xffffffffu;
            if (live && (i == 0 || kv[q] != prev)) { heads |= 1u << q; nheads++; }
            prev = kv[q];
        }
    }
    uint32_t rank = ccs_block_scan(nheads, s_scan);   // (its barriers: every thread has read its span)
    const uint32_t U = s_scan[kCcsThreads / 64];
#pragma unroll
    for (int q = 0; q < 16; q++)
        if ((heads >> q) & 1u) { s_key[rank] = kv[q]; s_wt[rank] = (uint16_t)(first + q); rank++; }
    __syncthreads();
    // a colour's pixels: from its head to the next colour's
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const uint32_t r = tid + q * kCcsThreads;
        kv[q] = r < U ? (r + 1 < U ? (uint32_t)s_wt[r + 1] : npx) - (uint32_t)s_wt[r] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const uint32_t r = tid + q * kCcsThreads;
        if (r < U) s_wt[r] = (uint16_t)kv[q];
    }
    if (U / K == 0) {   // kmeans.rs:67-68: fewer points than clusters
        if (tid == 0) res[f] = CcSmallResult{U, 0u, 0u, 0u, 0u, 1u};
        return;
    }

    // ---- b. kmeans::cluster
    for (uint32_t i = tid; i < U; i += kCcsThreads) s_lab[i] = (uint8_t)ccs_init_label(i, U, K);
    __syncthreads();   // (the weights are written; the init centroids read the keys only)
    if (tid < K) {
        const uint32_t ck = s_key[ccs_init_centroid_point(tid, U, K)];
        s_cent[tid] = ck;
        s_cc[tid] = ccs_cconst(ck, tid);
    }
    if (tid == 0) { s_moved = 0; s_reseed = 0; s_active = 0; }
    uint32_t iter = 0, moved_last = 0;
    for (;;) {
        for (uint32_t i = tid; i < 5 * 256; i += kCcsThreads) s_sum[i] = 0;   // (sums and members lie back to back)
        __syncthreads();
        uint32_t moved = 0;
        for (uint32_t i0 = tid * 4; i0 < U; i0 += 4 * kCcsThreads) {
            uint32_t p[4];
            int32_t best[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { p[q] = i0 + q < U ? s_key[i0 + q] : 0u; best[q] = 0x7fffffff; }
            for (uint32_t k = 0; k < K; k++) {
                const uint32_t ck = s_cent[k];
                const int32_t cc = s_cc[k];
#pragma unroll
                for (int q = 0; q < 4; q++) best[q] = min(best[q], ccs_score(p[q], ck, cc));
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t i = i0 + q;
                if (i >= U) break;
                const uint32_t cur = s_lab[i];
                const uint32_t nl = ccs_new_label(best[q], ccs_score(p[q], s_cent[cur], s_cc[cur]), cur);
                if (nl != cur) { moved++; s_lab[i] = (uint8_t)nl; }
                const uint32_t w = s_wt[i];
                atomicAdd(&s_sum[4 * nl], ((p[q] >> 16) & 255) * w);
                atomicAdd(&s_sum[4 * nl + 1], ((p[q] >> 8) & 255) * w);
                atomicAdd(&s_sum[4 * nl + 2], (p[q] & 255) * w);
                atomicAdd(&s_sum[4 * nl + 3], w);
                atomicAdd(&s_mem[nl], 1u);
            }
        }
        if (moved) atomicAdd(&s_moved, moved);
        __syncthreads();
        moved_last = s_moved;
        // Point::mean + the empty-cluster reseed (kmeans.rs:110-137)
        if (tid < K) {
            uint32_t ck;
            if (s_mem[tid] == 0) {
                ck = s_key[ccs_reseed_index(seed, iter, tid, U)];
                atomicAdd(&s_reseed, 1u);
            } else {
                ck = ccs_mean(s_sum[4 * tid], s_sum[4 * tid + 1], s_sum[4 * tid + 2], s_sum[4 * tid + 3]);
                atomicAdd(&s_active, 1u);
            }
            s_cent[tid] = ck;
            s_cc[tid] = ccs_cconst(ck, tid);
        }
        __syncthreads();
        iter++;
        if (moved_last == 0 || (max_iters && iter >= max_iters)) break;
        if (tid == 0) { s_moved = 0; s_active = 0; }
    }
    if (tid < K) cent_out[(size_t)f * K + tid] = s_cent[tid];
    if (tid == 0) res[f] = CcSmallResult{U, iter, moved_last, s_reseed, s_active, 0u};

    // ---- c. every pixel's label
    uint32_t *lab32 = reinterpret_cast<uint32_t *>(labels_out + row.lab_base);   // (16-byte aligned; the frame's run is padded to 16 labels)
    for (uint32_t i0 = tid * 4; i0 < npx; i0 += 4 * kCcsThreads) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = i0 + q;
            if (i >= npx) break;
            const uint32_t key = ccs_pixel_key(src, i);
            uint32_t lo = 0, hi = U;   // keys[lo] <= key < keys[hi]: the key is one of them
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_key[mid] <= key) lo = mid; else hi = mid;
            }
            word |= (uint32_t)s_lab[lo] << (8 * q);
        }
        lab32[i0 >> 2] = word;
    }
}

int cc_small_run(Ctx *c, const CcSmallRow *rows_d, uint32_t frames, uint32_t max_px, uint32_t K, uint64_t seed, uint64_t max_iters, uint8_t *labels_d,
                 uint32_t *cent_d, CcSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (K == 0 || K > kCcSmallMaxK || max_px == 0 || max_px > kCcSmallMaxPx) return c->fail(CNIIC_ERR_BAD_ARG, "cc_small: K or frame size outside the route");
    uint32_t cap_px = 1;
    while (cap_px < max_px) cap_px <<= 1;
    const uint32_t lds = ccs_lds_bytes(cap_px);
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_cc_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ccs_lds_bytes(kCcSmallMaxPx)));
    hipLaunchKernelGGL(k_cc_small, dim3(frames), dim3(kCcsThreads), lds, c->stream, rows_d, cap_px, K, seed, max_iters, labels_d, cent_d, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// ---- every stream from the tail's scratch to its frame's own destination (any alignment): a byte-wise head up to the destination's
// 16-byte boundary, 16-byte stores, a byte-wise tail.  The source behind the head lies at any offset: it is read in aligned words and
// shifted into place (the scratch has 16 spare bytes behind its last stream).
__global__ __launch_bounds__(256) void k_cc_small_place(const CcSmallPlace *__restrict__ pl, const uint8_t *__restrict__ scratch) {
    const CcSmallPlace p = pl[blockIdx.x];
    const uint8_t *__restrict__ src = scratch + p.src_off;
    uint8_t *__restrict__ dst = p.dst;
    const uint64_t len = p.len;
    const uint64_t to16 = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    const uint64_t head = len < to16 ? len : to16;
    const uint64_t body = (len - head) / 16;
    for (uint64_t i = threadIdx.x; i < head; i += 256) dst[i] = src[i];
    for (uint64_t j = threadIdx.x; j < body; j += 256) {
        const uint8_t *s = src + head + 16 * j;
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3) * 8;
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(s - (sh >> 3));
        uint32_t w[5];
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = sw[q];
        w[4] = sh ? sw[4] : 0u;
        uint4 v;
        v.x = sh ? (w[0] >> sh) | (w[1] << (32 - sh)) : w[0];
        v.y = sh ? (w[1] >> sh) | (w[2] << (32 - sh)) : w[1];
        v.z = sh ? (w[2] >> sh) | (w[3] << (32 - sh)) : w[2];
        v.w = sh ? (w[3] >> sh) | (w[4] << (32 - sh)) : w[3];
        *reinterpret_cast<uint4 *>(dst + head + 16 * j) = v;
    }
    for (uint64_t i = head + 16 * body + threadIdx.x; i < len; i += 256) dst[i] = src[i];
}

int cc_small_place(Ctx *c, const CcSmallPlace *pl_d, uint32_t n, const uint8_t *scratch_d) {
    if (!n) return CNIIC_OK;
    hipLaunchKernelGGL(k_cc_small_place, dim3(n), dim3(256), 0, c->stream, pl_d, scratch_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
