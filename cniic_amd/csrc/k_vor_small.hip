// k_vor_small.hip -- voronoi(K <= 256) of SMALL frames (at most kVorSmallMaxPx pixels), one workgroup per frame, any number of frames in one
// launch (cniic_codec_encode_batch_var / cniic_codec_measure_batch; codec.cpp vor_small_encode), and the repaint of such frames' streams
// (cniic_codec_decode_batch; codec.cpp vor_small_decode).
//
// k_vor_small: a frame's pixels with their labels, the K centroids and the clusters' sums fit in one CU's LDS, so the block goes from the
// pixels to the finished stream without leaving it -- kmeans::cluster exactly (kmeans.rs:17-39) over ColorPos points with the arithmetic of
// vor_small.hpp:
//   a. pixels (any byte alignment) -> 0xRRGGBB | label << 24 in LDS, labels by position, the first point of each chunk as centroid, the
//      clusters' sums and members under those labels
//   b. per iteration: every centroid's squared distance to its nearest other centroid (K^2 evaluations, block-wide); every point against
//      its own centroid, and the points that fail the stay test (vs_stays) into a dense list; the list against all K centroids, k walking
//      upwards; a point that moves takes its coordinates from its old cluster's sums to its new one's (the sums are integers: what they
//      hold is what a fresh summation would give); means, empty-cluster reseeds; until no point moves (or max_iters)
//   c. the stream (vs_stream_len) into the frame's slot of scratch and the result row
// k_vor_small_dec: the frame's centroids in LDS, every pixel the colour of the first centroid with the smallest vs_paint_dist, the image
// (in slices of kVorSmallDecSlice pixels, a workgroup each) assembled in LDS at the destination's 16-byte phase and stored with 16-byte
// stores between a byte-wise head and tail.
// No block waits for another.
#include "common.hpp"
#include "vor_small.hpp"

namespace cniic {

constexpr int kVsThreads = 1024;
static_assert(kVorSmallDefaultSeed == kDefaultSeed, "vor_small.hpp restates the library's default seed");
// centroids (x | y << 16, 0xRRGGBB), their separations, five sums per cluster, members
constexpr uint32_t kVsFixedBytes = (2 * 256 + 256 + 5 * 256 + 256) * 4;

// bytes of dynamic LDS for frames of at most cap_px pixels (cap_px: a power of two): a word per point, a u16 per entry of the search list, then the fixed part
static uint32_t vs_lds_bytes(uint32_t cap_px) { return std::max<uint32_t>(cap_px, 8) * 6 + kVsFixedBytes; }
static_assert(kVorSmallMaxPx * 6 + kVsFixedBytes + 256 <= 160 * 1024, "the largest routed frame fits one CU's LDS");

__device__ __forceinline__ uint32_t vs_pixel_key(const uint8_t *__restrict__ src, uint32_t i) {
    const uint8_t *p = src + 3ull * i;
    return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
}

// point `pxy`, `prgb` leaves cluster `from` (if `from` < 256) and joins cluster `to`
__device__ __forceinline__ void vs_account(uint32_t *s_sum, uint32_t *s_mem, uint32_t pxy, uint32_t prgb, uint32_t from, uint32_t to) {
    const uint32_t v[5] = {pxy & 0xffffu, pxy >> 16, (prgb >> 16) & 255u, (prgb >> 8) & 255u, prgb & 255u};
#pragma unroll
    for (int d = 0; d < 5; d++) {
        if (from < 256) atomicSub(&s_sum[5 * from + d], v[d]);
        atomicAdd(&s_sum[5 * to + d], v[d]);
    }
    if (from < 256) atomicSub(&s_mem[from], 1u);
    atomicAdd(&s_mem[to], 1u);
}

__global__ __launch_bounds__(kVsThreads) void k_vor_small(const VorSmallRow *__restrict__ rows, uint32_t cap_px, uint32_t K, uint64_t seed, uint64_t max_iters,
                                                          uint32_t stay_on, uint8_t *__restrict__ scratch, uint64_t sstride, VorSmallResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t vs_lds[];
    __shared__ uint32_t s_moved, s_reseed, s_active, s_evals, s_list_n;
    const uint32_t cap = max(cap_px, 8u);
    uint32_t *s_pt = reinterpret_cast<uint32_t *>(vs_lds);                         // [cap]: 0xRRGGBB | label << 24
    uint16_t *s_list = reinterpret_cast<uint16_t *>(vs_lds + 4ull * cap);           // [cap]: the points to search this iteration
    uint2 *s_cent = reinterpret_cast<uint2 *>(vs_lds + 6ull * cap);                 // [256]: x | y << 16, 0xRRGGBB
    uint32_t *s_sep = reinterpret_cast<uint32_t *>(s_cent + 256);                   // [256]: squared distance to the nearest other centroid
    uint32_t *s_sum = s_sep + 256;                                                 // [256][5]: x, y, r, g, b
    uint32_t *s_mem = s_sum + 5 * 256;                                             // [256]
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const VorSmallRow row = rows[f];
    const uint32_t w = row.w, n = row.w * row.h;   // 1 .. cap_px
    const uint8_t *__restrict__ src = row.src;
    if (n / K == 0) {   // kmeans.rs:67-68: fewer points than clusters
        if (tid == 0) res[f] = VorSmallResult{1u, n, 0u, 0u, 0u, 0u, 0ull};
        return;
    }
    // thread t owns the points t, t + 1024, ...: where the first lies, and the step from one to the next
    const uint32_t x0 = tid % w, y0 = tid / w, step_x = (uint32_t)kVsThreads % w, step_y = (uint32_t)kVsThreads / w;

    // ---- a. load, initial labels, centroids and sums
    for (uint32_t i = tid; i < n; i += kVsThreads) s_pt[i] = vs_pixel_key(src, i) | vs_init_label(i, n, K) << 24;
    for (uint32_t i = tid; i < 6 * 256; i += kVsThreads) s_sum[i] = 0;   // (sums and members lie back to back)
    if (tid == 0) { s_moved = 0; s_reseed = 0; s_active = 0; s_evals = 0; s_list_n = 0; }
    __syncthreads();
    if (tid < K) {
        const uint32_t i = vs_init_centroid_point(tid, n, K);
        s_cent[tid] = make_uint2((i % w) | (i / w) << 16, s_pt[i] & 0xffffffu);
    }
    for (uint32_t i = tid, x = x0, y = y0; i < n; i += kVsThreads) {
        const uint32_t p = s_pt[i];
        vs_account(s_sum, s_mem, x | y << 16, p, 256u, p >> 24);
        x += step_x; y += step_y;
        if (x >= w) { x -= w; y++; }
    }
    __syncthreads();

    // ---- b. kmeans::cluster
    uint32_t iter = 0, moved_last = 0;
    uint64_t evals_total = 0;   // (thread 0's is the frame's)
    for (;;) {
        {   // four lanes per centroid, each over a quarter of the others
            const uint32_t c = tid >> 2, sub = tid & 3;
            uint32_t m = 0xffffffffu;
            if (c < K) {
                const uint2 cc = s_cent[c];
                for (uint32_t k = sub; k < K; k += 4) {
                    const uint2 ck = s_cent[k];
                    if (k != c) m = min(m, vs_dist2(cc.x, cc.y, ck.x, ck.y));
                }
            }
            m = min(m, (uint32_t)__shfl_xor((int)m, 1));
            m = min(m, (uint32_t)__shfl_xor((int)m, 2));
            if (c < K && sub == 0) s_sep[c] = m;
        }
        __syncthreads();
        // every point against its own centroid; the ones that may have a nearer one go on the list
        uint32_t evals = 0;
        for (uint32_t i = tid, x = x0, y = y0; i < n; i += kVsThreads) {
            const uint32_t p = s_pt[i], cur = p >> 24;
            const uint2 cc = s_cent[cur];
            const uint32_t dcur = vs_dist2(x | y << 16, p, cc.x, cc.y);
            evals++;
            if (!(stay_on && vs_stays(dcur, s_sep[cur]))) s_list[atomicAdd(&s_list_n, 1u)] = (uint16_t)i;
            x += step_x; y += step_y;
            if (x >= w) { x -= w; y++; }
        }
        __syncthreads();
        const uint32_t list_n = s_list_n;
        uint32_t moved = 0;
        for (uint32_t j = tid; j < list_n; j += kVsThreads) {
            const uint32_t i = s_list[j], p = s_pt[i], cur = p >> 24, pxy = (i % w) | (i / w) << 16;
            uint32_t best = 0xffffffffu, best_k = 0;
#pragma unroll 4
            for (uint32_t k = 0; k < K; k++) {
                const uint2 ck = s_cent[k];
                const uint32_t d = vs_dist2(pxy, p, ck.x, ck.y);
                if (d < best) { best = d; best_k = k; }
            }
            evals += K;
            const uint2 cc = s_cent[cur];
            const uint32_t nl = vs_new_label(best, best_k, vs_dist2(pxy, p, cc.x, cc.y), cur);
            if (nl != cur) {
                moved++;
                s_pt[i] = (p & 0xffffffu) | nl << 24;
                vs_account(s_sum, s_mem, pxy, p, cur, nl);
            }
        }
        if (moved) atomicAdd(&s_moved, moved);
        if (evals) atomicAdd(&s_evals, evals);
        __syncthreads();
        moved_last = s_moved;
        evals_total += s_evals;
        // Point::mean + the empty-cluster reseed (kmeans.rs:110-137)
        if (tid < K) {
            const uint32_t members = s_mem[tid];
            uint2 ck;
            if (members == 0) {
                const uint32_t i = vs_reseed_index(seed, iter, tid, n);
                ck = make_uint2((i % w) | (i / w) << 16, s_pt[i] & 0xffffffu);
                atomicAdd(&s_reseed, 1u);
            } else {
                const uint32_t *s = s_sum + 5 * tid;
                ck = make_uint2(vs_mean_xy(s[0], s[1], members), vs_mean_rgb(s[2], s[3], s[4], members));
                atomicAdd(&s_active, 1u);
            }
            s_cent[tid] = ck;
        }
        __syncthreads();
        iter++;
        if (moved_last == 0 || (max_iters && iter >= max_iters)) break;
        if (tid == 0) { s_moved = 0; s_active = 0; s_evals = 0; s_list_n = 0; }   // (read again behind the next barrier at the earliest)
    }

    // ---- c. the stream and the result row
    uint8_t *out = scratch + (uint64_t)f * sstride;
    const uint32_t len = vs_stream_len(K);
    for (uint32_t j = tid; j < len; j += kVsThreads) {
        uint8_t b;
        if (j < 4) b = (uint8_t)(row.w >> (8 * j));
        else if (j < 8) b = (uint8_t)(row.h >> (8 * (j - 4)));
        else if (j < 16) b = (uint8_t)(j < 12 ? K >> (8 * (j - 8)) : 0u);
        else {
            const uint32_t k = (j - 16) / 19;
            const uint2 ck = s_cent[k];
            b = vs_centroid_byte(ck.x & 0xffffu, ck.x >> 16, ck.y, j - vs_centroid_at(k));
        }
        out[j] = b;
    }
    if (tid == 0) res[f] = VorSmallResult{0u, n, iter, moved_last, s_reseed, s_active, evals_total};
}

int vor_small_run(Ctx *c, const VorSmallRow *rows_d, uint32_t frames, uint32_t max_px, uint32_t K, uint64_t seed, uint64_t max_iters, bool stay_test,
                  uint8_t *scratch_d, uint64_t sstride, VorSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (K == 0 || K > kVorSmallMaxK || max_px == 0 || max_px > kVorSmallMaxPx || sstride < vs_stream_len(K))
        return c->fail(CNIIC_ERR_BAD_ARG, "vor_small: K, frame size or slot outside the route");
    uint32_t cap_px = 1;
    while (cap_px < max_px) cap_px <<= 1;
    const uint32_t lds = vs_lds_bytes(cap_px);
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_vor_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)vs_lds_bytes(kVorSmallMaxPx)));
    hipLaunchKernelGGL(k_vor_small, dim3(frames), dim3(kVsThreads), lds, c->stream, rows_d, cap_px, K, seed, max_iters, stay_test ? 1u : 0u, scratch_d, sstride, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// ---- the repaint (clusterc.rs:180-186).  A row is a SLICE of a frame: at most kVorSmallDecSlice pixels from pixel px0 on (a multiple of
// the slice, whose 3 x 2048 bytes are a multiple of 16: every slice of a frame starts at the frame's own 16-byte phase), so that a batch of
// few large frames still fills more CUs than it has frames.  Dynamic LDS: 3 * (the largest slice's pixels) + 16 rounded up to 16.
__global__ __launch_bounds__(kVsThreads) void k_vor_small_dec(const VorSmallDecRow *__restrict__ rows, const uint32_t *__restrict__ table) {
    extern __shared__ __align__(16) uint8_t vd_img[];
    __shared__ uint32_t s_cx[256], s_cy[256], s_col[256];
    const uint32_t tid = threadIdx.x;
    const VorSmallDecRow row = rows[blockIdx.x];
    const uint32_t K = row.K, w = row.w, n = min(row.w * row.h - row.px0, kVorSmallDecSlice);
    if (tid < K) {
        const uint32_t *t = table + 3ull * (row.cent0 + tid);
        s_cx[tid] = t[0]; s_cy[tid] = t[1]; s_col[tid] = t[2];
    }
    __syncthreads();
    uint8_t *__restrict__ dst = row.dst + 3ull * row.px0;
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);   // the slice lies in LDS as it lies in memory, modulo 16
    const uint32_t step_x = (uint32_t)kVsThreads % w, step_y = (uint32_t)kVsThreads / w;
    for (uint32_t i = tid, x = (row.px0 + tid) % w, y = (row.px0 + tid) / w; i < n; i += kVsThreads) {
        uint32_t best = vs_paint_dist(s_cx[0], s_cy[0], x, y), bk = 0;
        for (uint32_t k = 1; k < K; k++) {
            const uint32_t d = vs_paint_dist(s_cx[k], s_cy[k], x, y);
            if (d < best) { best = d; bk = k; }
        }
        const uint32_t col = s_col[bk];
        uint8_t *q = vd_img + phase + 3 * i;
        q[0] = (uint8_t)(col >> 16); q[1] = (uint8_t)(col >> 8); q[2] = (uint8_t)col;
        x += step_x; y += step_y;
        if (x >= w) { x -= w; y++; }
    }
    __syncthreads();
    const uint32_t len = 3 * n, to16 = (16 - phase) & 15, head = len < to16 ? len : to16, body = (len - head) / 16;
    for (uint32_t i = tid; i < head; i += kVsThreads) dst[i] = vd_img[phase + i];
    for (uint32_t j = tid; j < body; j += kVsThreads)
        *reinterpret_cast<uint4 *>(dst + head + 16 * j) = *reinterpret_cast<const uint4 *>(vd_img + phase + head + 16 * j);
    for (uint32_t i = head + 16 * body + tid; i < len; i += kVsThreads) dst[i] = vd_img[phase + i];
}

int vor_small_dec_run(Ctx *c, const VorSmallDecRow *rows_d, uint32_t slices, uint32_t max_px, const uint32_t *table_d) {
    if (!slices) return CNIIC_OK;
    if (max_px == 0 || max_px > kVorSmallMaxPx) return c->fail(CNIIC_ERR_BAD_ARG, "vor_small_dec: frame size outside the route");
    static_assert(3 * kVorSmallDecSlice % 16 == 0, "a slice's bytes are a multiple of 16");
    const uint32_t lds = (3 * std::min(max_px, kVorSmallDecSlice) + 16 + 15) & ~15u;
    hipLaunchKernelGGL(k_vor_small_dec, dim3(slices), dim3(kVsThreads), lds, c->stream, rows_d, table_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
