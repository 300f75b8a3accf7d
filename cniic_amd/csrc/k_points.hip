// k_points.hip -- the front and back end of ClusterColors::encode around the K-means, for large images
// (reference: count_freqs of the pixels, src/utils.rs:4-16 called at src/codec/clusterc.rs:21-24, and the
// colour -> centroid-colour remap of every pixel, clusterc.rs:31-47).
//
// What the K-means (k_kmeans_rgbw.hip) wants is the list of DISTINCT colours with their pixel counts in
// cell-major order (cell_of: 32^3 colour cells, the 4^3 cells of a 32^3-colour "super-cell" consecutive), and
// what Huffman wants afterwards is the cluster label of every pixel.  Both are a histogram / a lookup over
// 2^24 colours, far beyond LDS, and scattered 2- or 4-byte accesses to HBM-resident tables are bound by the
// number of L2 requests (one per lane), not by bytes.  So the pixels are partitioned ONCE by super-cell
// (512 buckets), staged through LDS so that every global access is a run of consecutive addresses:
//
//   k_sp_count     per 64 Ki-pixel chunk: pixels per bucket (LDS histogram)                     read 3 B/px
//   k_sp_colscan   where each (chunk, bucket) run starts inside its bucket, and the buckets' totals
//   k_sp_scatter   per chunk: 15-bit colour-in-bucket of every pixel, sorted by bucket in LDS and written as
//                  512 runs; the pixel's place in the chunk's sorted order goes to prank[pixel]  read 3, write 2 + 2 B/px
//                  (every block scans the 512 totals for the buckets' first entries; block 0 leaves them as bstart / sstart)
//   k_sp_hist      per bucket: LDS histogram of its 2^15 colours -> occupied colours per cell, occupancy bitmap,
//                  and the bucket's distinct colours with their counts, staged in cell-major order
//   Then, a single image (cc_prepare_image: sp_front), three launches whose blocks take a role from blockIdx:
//   k_cc_front_a   k_bits_prefix | k_cell_totals | the K-means arenas zeroed
//   k_cc_front_b   k_gidx_finish | k_cell_scan                 (the colour count's 8-byte copy to the host follows)
//   k_cc_front_c   k_ps_ranges | k_rgbw_init_cent | k_sp_emit
//   -- the roles being the bodies of these kernels, which every other caller (sp_build without hist_only, the shared palette's
//   cc_image_create, CNIIC_TEST_CC_FRONT=split) launches one by one.
//   With a persistent K-means launch to come (K <= 256, the context's own CUs, no given centroids; not under CNIIC_TEST_CC_POINTS=arrays)
//   the staged colours are NOT copied into the K-means arrays: the staging is cell-major already, so the launch's set-up reads it where
//   it lies and makes key and initial label itself (k_kmeans_persist.hip, PsDevPtrs::sbin), and k_sp_partlab reads its colours there too.
//   The chain is then
//   k_cc_front_b   k_gidx_finish | k_cell_scan, which also writes the launch's chunk boundaries (ps_bounds.hpp: no bisection)
//   k_cc_front_c   the fit check of those boundaries | k_rgbw_init_cent                      (no emit role, no count copy in between)
//   k_rgbw_persist enqueued without the host having seen the colour count; the count's 8-byte copy follows the launch and is looked at
//                  where the result block is fetched (cc_finish).  k_sp_emit runs only if the arrays are needed after all
//                  (km_rgbw_need_arrays: the loop of launches behind a launch that gave up).
//   The kernels' own stories:
//   k_bits_prefix / k_gidx_finish   bitmap -> popcount prefix = GIdx: rank of a colour in the ascending list of all colours = the
//                  reference's point order, used for init_assignment / init_centroids / the reseed index
//   (km_rgbw_create: arena fill, k_rgbw_init_cent, k_cell_totals, k_cell_scan, arena fill, k_ps_ranges)
//   k_sp_emit      the staged colours, counts and their initial labels to their places in the K-means arrays
//   ... K-means ...
//   k_sp_partlab   per bucket: label of every partitioned pixel from an LDS table of the bucket's colours
//   (the host waits for the K-means result block here, builds the Huffman tree and leaves codes, lengths and header in a pinned block)
//   k_sp_pixpack   narrow labels (K <= 256): per chunk, its 512 label runs into LDS, each pixel picks stage[prank] into a REGISTER,
//                  and the chunk's codes go straight into the stream -- the chunk's first bit from a ticketed look-back over the
//                  chunks' bit counts, the emit the label pack's own (pack_emit, device_utils.hpp)          read 1 + 2 B/px, write the stream
//   k_sp_pixlab    wide labels, the frame batches, the frozen palettes, and when k_sp_pixpack gives its look-back up: the same pick
//                  written out as a label stream for the pack's three passes (k_huff.hip)                   read 1 + 2, write 1 B/px
//
// No atomics on global memory, no table of 2^24 entries, and every pixel's label is found without a random
// read.  Results are identical to the dense-table path (k_hist.hip + k_cells_write_tbl + k_pixel_labels): the
// point set, weights, initial labels and cell order are the same.
#include "common.hpp"
#include "device_utils.hpp"
#include "kmeans_rgbw.hpp"
#include "sp_keys.hpp"

namespace cniic {

constexpr uint32_t kSpBuckets = 512;          // super-cells: r[7:5] g[7:5] b[7:5]
constexpr uint32_t kSpBins = 1u << 15;         // colours of a super-cell
constexpr uint32_t kSpChunk = 1u << 16;        // pixels per chunk: a position inside a run fits 16 bits
constexpr int kSpThreads = 1024;
constexpr uint32_t kSpSliceMin = 1u << 17;     // k_sp_partlab: entries per slice of a bucket, at least
constexpr uint32_t kSpSlices = 8;              // ... and slices per bucket, at most
constexpr uint32_t kSpWaves = kSpThreads / 64;

// (sp_bucket, sp_bin, sp_key: sp_keys.hpp)

// exclusive scan of 512 values held one per thread by threads 0..511 of a 1024-thread block; all threads call
__device__ __forceinline__ uint32_t scan512(uint32_t v, uint32_t *wsum) { return block_exclusive_scan<kSpThreads>(v, wsum); }

// pixels of chunk c: [c * kSpChunk, min(npx, (c + 1) * kSpChunk)); thread t takes the 16-pixel groups t, t + 1024, ...
template <typename F> __device__ __forceinline__ void sp_for_pixels(const uint8_t *__restrict__ rgb, uint64_t npx, F &&f) {
    const uint64_t p0 = (uint64_t)blockIdx.x * kSpChunk, p1 = min(npx, p0 + kSpChunk);
    const uint4 *v = reinterpret_cast<const uint4 *>(rgb);
    for (uint64_t g = p0 / 16 + threadIdx.x; g * 16 < p1; g += kSpThreads) {
        uint32_t key[16];
        if (g * 16 + 16 <= p1) {
            load16px_keys(v + 3 * g, key);
            f(g * 16, key, 16u);
        } else {  // the image's last, partial group
            const uint32_t m = (uint32_t)(p1 - g * 16);
            for (uint32_t i = 0; i < 16; i++) key[i] = i < m ? rgb_key(rgb + 3 * (g * 16 + i)) : 0u;
            f(g * 16, key, m);
        }
    }
}

__global__ __launch_bounds__(kSpThreads) void k_sp_count(const uint8_t *__restrict__ rgb, uint64_t npx, uint32_t *__restrict__ cnt) {
    __shared__ uint32_t h[kSpBuckets];
    if (threadIdx.x < kSpBuckets) h[threadIdx.x] = 0;
    __syncthreads();
    sp_for_pixels(rgb, npx, [&](uint64_t, const uint32_t (&key)[16], uint32_t m) {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (i < m) atomicAdd(&h[sp_bucket(key[i])], 1u);
    });
    __syncthreads();
    if (threadIdx.x < kSpBuckets) cnt[(size_t)blockIdx.x * kSpBuckets + threadIdx.x] = h[threadIdx.x];
}

// one block per bucket: pre[c][b] = pixels of bucket b in the chunks before c; total[b]
__global__ __launch_bounds__(256) void k_sp_colscan(const uint32_t *__restrict__ cnt, uint32_t nchunks, uint32_t *__restrict__ pre,
                                                    uint32_t *__restrict__ total) {
    __shared__ uint32_t wsum[256 / 64];
    const uint32_t b = blockIdx.x, per = (nchunks + 255) / 256;
    const uint32_t c0 = threadIdx.x * per, c1 = min(c0 + per, nchunks);
    uint32_t s = 0;
    for (uint32_t c = c0; c < c1; c++) s += cnt[(size_t)c * kSpBuckets + b];
    uint32_t run = block_exclusive_scan<256>(s, wsum);
    for (uint32_t c = c0; c < c1; c++) {
        pre[(size_t)c * kSpBuckets + b] = run;
        run += cnt[(size_t)c * kSpBuckets + b];
    }
    if (threadIdx.x == 255) total[b] = run;  // (the last thread's range ends the column, or is empty and holds the sum)
}

// The chunk's pixels sorted by bucket occupy positions [0, n) of the LDS stage; off[b] .. off[b + 1] is bucket b's run
// (off[kSpBuckets] = n).  Wave w walks the positions [w per, (w + 1) per) 64 at a time, lane <-> position, each lane
// keeping the bucket of its position (runs are short: the bucket advances about every other step).  STEPS positions
// per lane are handed over together so that their loads can be in flight at once.  A walk by runs instead costs a
// dependent round trip to memory per run, and one by rounds over all runs is quadratic when a run is long.
template <int STEPS, typename F> __device__ __forceinline__ void sp_walk_sorted(const uint32_t *off, uint32_t n, F &&f) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t per = (n + kSpThreads - 1) / kSpThreads * 64;
    const uint32_t j0 = wv * per, j1 = min(n, j0 + per);
    if (j0 >= j1) return;
    const uint32_t jj = min(j0 + lane, j1 - 1);
    uint32_t lo = 0, hi = kSpBuckets;  // off[lo] <= jj < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= jj) lo = mid; else hi = mid;
    }
    uint32_t b = lo, end = off[b + 1];
    for (uint32_t j = j0 + lane; j < j1; j += 64 * STEPS) {
        uint32_t jb[STEPS];
#pragma unroll
        for (int t = 0; t < STEPS; t++) {
            const uint32_t q = j + 64 * t;
            jb[t] = 0xffffffffu;
            if (q < j1) {
                while (q >= end) { b++; end = off[b + 1]; }
                jb[t] = b;
            }
        }
        f(j, jb);
    }
}

// LDS (dynamic): stage u16[kSpChunk] | off u32[kSpBuckets + 1] | cur u32[kSpBuckets]
__global__ __launch_bounds__(kSpThreads) void k_sp_scatter(const uint8_t *__restrict__ rgb, uint64_t npx, const uint32_t *__restrict__ cnt,
                                                           const uint32_t *__restrict__ pre, const uint32_t *__restrict__ total,
                                                           uint32_t *__restrict__ bstart, uint32_t *__restrict__ sstart,
                                                           uint16_t *__restrict__ part, uint16_t *__restrict__ prank) {
    extern __shared__ __align__(16) uint8_t sp_lds[];
    uint16_t *stage = reinterpret_cast<uint16_t *>(sp_lds);
    uint32_t *off = reinterpret_cast<uint32_t *>(sp_lds + (size_t)kSpChunk * 2);  // [kSpBuckets + 1]
    uint32_t *cur = off + kSpBuckets + 1;
    __shared__ uint32_t wsum[kSpWaves];
    __shared__ uint32_t bfirst[kSpBuckets];
    const uint32_t *mycnt = cnt + (size_t)blockIdx.x * kSpBuckets;
    const uint32_t n_b = threadIdx.x < kSpBuckets ? mycnt[threadIdx.x] : 0u;
    // bstart: first entry of every bucket in the partition.  Every block scans the 512 totals itself (a one-block kernel between
    // k_sp_colscan and this one cost a dispatch, 4-5 us, for it); block 0 leaves the result to the kernels behind, with sstart:
    // first slot of a bucket's staged distinct colours (a bucket of n pixels has at most min(n, 2^15) of them)
    const uint32_t tot_b = threadIdx.x < kSpBuckets ? total[threadIdx.x] : 0u;
    const uint32_t first_b = scan512(tot_b, wsum);
    if (threadIdx.x < kSpBuckets) bfirst[threadIdx.x] = first_b;
    if (blockIdx.x == 0) {
        const uint32_t sfirst = scan512(min(tot_b, kSpBins), wsum);
        if (threadIdx.x < kSpBuckets) { bstart[threadIdx.x] = first_b; sstart[threadIdx.x] = sfirst; }
        if (threadIdx.x == kSpBuckets - 1) bstart[kSpBuckets] = first_b + tot_b;
    }
    const uint32_t ex = scan512(n_b, wsum);
    if (threadIdx.x < kSpBuckets) { off[threadIdx.x] = ex; cur[threadIdx.x] = 0; }
    if (threadIdx.x == kSpBuckets - 1) off[kSpBuckets] = ex + n_b;
    __syncthreads();
    sp_for_pixels(rgb, npx, [&](uint64_t first, const uint32_t (&key)[16], uint32_t m) {
        uint32_t rk[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            rk[i] = 0;
            if (i < m) {
                const uint32_t b = sp_bucket(key[i]);
                // its place in the chunk's bucket-sorted order (any order inside a run), remembered per pixel: the way back
                // (k_sp_pixlab) is then one LDS read per pixel -- no colour, no bucket, no offset table
                rk[i] = off[b] + atomicAdd(&cur[b], 1u);
                stage[rk[i]] = (uint16_t)sp_bin(key[i]);
            }
        }
        if (m == 16) {
            uint4 *d = reinterpret_cast<uint4 *>(prank + first);
            d[0] = make_uint4(rk[0] | (rk[1] << 16), rk[2] | (rk[3] << 16), rk[4] | (rk[5] << 16), rk[6] | (rk[7] << 16));
            d[1] = make_uint4(rk[8] | (rk[9] << 16), rk[10] | (rk[11] << 16), rk[12] | (rk[13] << 16), rk[14] | (rk[15] << 16));
        } else {
            for (uint32_t i = 0; i < m; i++) prank[first + i] = (uint16_t)rk[i];
        }
    });
    __syncthreads();
    // the chunk's 512 runs go out, each to consecutive addresses.  Wave w owns buckets w, w + 16, ...: their sizes and
    // places are fetched by 32 lanes at once (fetched per bucket they are 32 dependent round trips to memory)
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t *mypre = pre + (size_t)blockIdx.x * kSpBuckets;
    const uint32_t mb = wv + kSpWaves * (lane & 31);
    const uint32_t m_n = mycnt[mb], m_dst = bfirst[mb] + mypre[mb], m_off = off[mb];
    for (uint32_t k = 0; k < kSpBuckets / kSpWaves; k++) {
        const uint32_t n = __shfl(m_n, k, 64), d0 = __shfl(m_dst, k, 64), o = __shfl(m_off, k, 64);
        for (uint32_t i = lane; i < n; i += 64) part[(size_t)d0 + i] = stage[o + i];
    }
}

// entries [s, e) of a u16 stream, four per load where the address allows (8-byte aligned), else one by one; four
// loads are in flight per thread (a crowded bucket is one block's work: with one load at a time its 220 K entries at
// C2 were 54 dependent round trips to memory and set the kernel's time)
template <typename F> __device__ __forceinline__ void sp_for_entries(const uint16_t *__restrict__ part, uint64_t s, uint64_t e, F &&f) {
    const uint64_t a = min(e, (s + 3) & ~3ull), z = a + ((e - a) & ~3ull);
    for (uint64_t i = s + threadIdx.x; i < a; i += kSpThreads) { const uint32_t v = part[i]; f(i, v, v, v, v, 1u); }
    constexpr uint64_t kStep = 4 * (uint64_t)kSpThreads;
    for (uint64_t i = a + 4 * (uint64_t)threadIdx.x; i < z; i += 4 * kStep) {
        uint2 q[4];
#pragma unroll
        for (int t = 0; t < 4; t++) q[t] = i + t * kStep < z ? *reinterpret_cast<const uint2 *>(part + i + t * kStep) : make_uint2(0u, 0u);
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (i + t * kStep < z) f(i + t * kStep, q[t].x & 0xffffu, q[t].x >> 16, q[t].y & 0xffffu, q[t].y >> 16, 4u);
    }
    for (uint64_t i = z + threadIdx.x; i < e; i += kSpThreads) { const uint32_t v = part[i]; f(i, v, v, v, v, 1u); }
}

// LDS histogram of one bucket's colours.  A flat image puts every pixel of a wave into one bin: equal
// neighbours are added together, and a wave whose 256 entries are all the same colour adds once.
__device__ __forceinline__ void sp_bucket_hist(const uint16_t *__restrict__ part, uint64_t s, uint64_t e, uint32_t *hist) {
    for (uint32_t i = threadIdx.x; i < kSpBins; i += kSpThreads) hist[i] = 0;
    __syncthreads();
    sp_for_entries(part, s, e, [&](uint64_t, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t m) {
        if (m == 1) { atomicAdd(&hist[a], 1u); return; }
        const bool same = a == b && b == c && c == d;
        const uint32_t first = __builtin_amdgcn_readfirstlane(a);
        if (__all(same && a == first) && __popcll(__ballot(1)) == 64) {
            if ((threadIdx.x & 63) == 0) atomicAdd(&hist[a], 256u);
        } else if (same) {
            atomicAdd(&hist[a], 4u);
        } else {
            atomicAdd(&hist[a], 1u); atomicAdd(&hist[b], 1u); atomicAdd(&hist[c], 1u); atomicAdd(&hist[d], 1u);
        }
    });
    __syncthreads();
}


// One block per bucket: LDS histogram of its colours -> occupied colours per cell (cell_count[bucket * 64 + cell]), the
// bucket's words of the occupancy bitmap, and the bucket's distinct colours as (bin, count) pairs in bin order = cell-major
// order, staged at sstart[bucket] (where they go in the K-means arrays is only known when every bucket has counted).
__global__ __launch_bounds__(kSpThreads) void k_sp_hist(const uint16_t *__restrict__ part, const uint32_t *__restrict__ bstart,
                                                        const uint32_t *__restrict__ sstart, uint32_t *__restrict__ cell_count,
                                                        uint32_t *__restrict__ bits32, uint16_t *__restrict__ sbin,
                                                        uint32_t *__restrict__ scnt) {
    extern __shared__ __align__(16) uint8_t sp_lds[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(sp_lds);
    __shared__ uint32_t wsum[kSpWaves];
    const uint32_t bucket = blockIdx.x;
    const uint64_t s = bstart[bucket], e = bstart[bucket + 1];
    const uint32_t r5 = threadIdx.x >> 5, g5 = threadIdx.x & 31;  // thread (r5, g5) owns one colour row of the bitmap
    const uint32_t word_at = ((((bucket >> 6) & 7u) << 5 | r5) << 11) | ((((bucket >> 3) & 7u) << 5 | g5) << 3) | (bucket & 7u);
    if (s == e) {  // no pixel here: no colours (the K-means never looks at an empty cell), but the bitmap words are ours
        if (threadIdx.x < 64) cell_count[bucket * 64 + threadIdx.x] = 0;
        bits32[word_at] = 0;
        return;
    }
    sp_bucket_hist(part, s, e, hist);
    uint32_t word = 0;
#pragma unroll
    for (uint32_t bq = 0; bq < 4; bq++) {
        const uint32_t base = ((r5 >> 3) << 13) | ((g5 >> 3) << 11) | (bq << 9) | ((r5 & 7u) << 6) | ((g5 & 7u) << 3);
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) word |= (hist[base + j] != 0 ? 1u : 0u) << (bq * 8 + j);
    }
    bits32[word_at] = word;
    // wave w owns bins [2048 w, 2048 w + 2048) = 4 cells, 64 at a time with lane <-> bin: the occupied lanes of one
    // step write consecutive positions (one or two lines per store)
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    uint32_t mine = 0;
    for (uint32_t c4 = 0; c4 < 4; c4++) {
        uint32_t in_cell = 0;
        for (uint32_t st = 0; st < 8; st++) in_cell += (uint32_t)__popcll(__ballot(hist[wv * 2048 + c4 * 512 + st * 64 + lane] != 0));
        if (lane == 0) cell_count[bucket * 64 + wv * 4 + c4] = in_cell;
        mine += in_cell;
    }
    if (lane == 0) wsum[wv] = mine;
    __syncthreads();
    uint32_t pos0 = sstart[bucket];
    for (uint32_t i = 0; i < wv; i++) pos0 += wsum[i];
    for (uint32_t st = 0; st < 32; st++) {
        const uint32_t bin = wv * 2048 + st * 64 + lane, v = hist[bin];
        const unsigned long long bm = __ballot(v != 0);
        if (v) {
            const uint32_t pos = pos0 + (uint32_t)__popcll(bm & lt_mask);
            sbin[pos] = (uint16_t)bin;
            scnt[pos] = v;
        }
        pos0 += (uint32_t)__popcll(bm);
    }
}

struct SpEmit {             // where the distinct colours go: the K-means state's cell-major arrays
    const uint32_t *cell_start;
    uint32_t *ckeys, *cweight;
    void *labels;
    uint32_t K, wide;
    GIdx gx;
    const uint64_t *U_dev;      // when set: the length of the point list is here, not yet in gx.U
};

// the staged colours of every bucket -> keys, counts and initial labels at their cell-major positions: a copy, the bucket's
// place being cell_start of its first cell.  kSpEmitSplit blocks per bucket.
// Entry i of the bucket is the work of thread i % 1024 of 1024 (`first`: this thread's number among them), four entries a step --
// whether the 1024 are kSpEmitSplit blocks of 256 (k_sp_emit) or one block (the emit role of k_cc_front_c).
constexpr uint32_t kSpEmitSplit = 4;
__device__ __forceinline__ void sp_emit_body(uint32_t bucket, uint32_t first, const uint32_t *__restrict__ sstart, const uint16_t *__restrict__ sbin,
                                             const uint32_t *__restrict__ scnt, const SpEmit &em) {
    const uint32_t q0 = em.cell_start[bucket * 64], n = em.cell_start[bucket * 64 + 64] - q0, s0 = sstart[bucket];
    const uint32_t U = em.U_dev ? (uint32_t)*em.U_dev : (uint32_t)em.gx.U, ppc = max(U / em.K, 1u);  // (fewer colours than clusters: the host refuses later)
    const float rcp = 1.0f / (float)ppc;
    // four entries per thread and step, each a chain of two loads (the staged colour, then its two index words): the
    // chains travel together
    constexpr uint32_t kStride = 256 * kSpEmitSplit;
    for (uint32_t i0 = first; i0 < n; i0 += 4 * kStride) {
        uint32_t key[4], cnt[4], rank[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t i = i0 + t * kStride;
            key[t] = i < n ? sp_key(bucket, sbin[s0 + i]) : 0u;
            cnt[t] = i < n ? scnt[s0 + i] : 0u;
        }
#pragma unroll
        for (int t = 0; t < 4; t++) rank[t] = i0 + t * kStride < n ? gidx_rank(em.gx, key[t]) : 0u;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t i = i0 + t * kStride;
            if (i >= n) continue;
            em.ckeys[q0 + i] = key[t];
            em.cweight[q0 + i] = cnt[t];
            if (!em.labels) continue;   // (km_rgbw_need_arrays behind a finished run: the labels hold its result)
            const uint32_t lab = init_label24(rank[t], U, em.K, ppc, rcp);  // init_assignment kmeans.rs:61-78
            if (em.wide) static_cast<uint16_t *>(em.labels)[q0 + i] = (uint16_t)lab;
            else static_cast<uint8_t *>(em.labels)[q0 + i] = (uint8_t)lab;
        }
    }
}
__global__ __launch_bounds__(256) void k_sp_emit(const uint32_t *__restrict__ sstart, const uint16_t *__restrict__ sbin,
                                                 const uint32_t *__restrict__ scnt, SpEmit em) {
    sp_emit_body(blockIdx.x / kSpEmitSplit, (blockIdx.x % kSpEmitSplit) * 256 + threadIdx.x, sstart, sbin, scnt, em);
}

// bits (u64[2^18]) -> wprefix inside blocks of 1024 words + blocktot; k_gidx_finish (k_hist.hip) completes it
__global__ __launch_bounds__(256) void k_bits_prefix(const unsigned long long *__restrict__ bits, uint32_t *__restrict__ wprefix,
                                                     uint32_t *__restrict__ blocktot) {
    __shared__ uint32_t wsum[256 / 64];
    bits_prefix_body(blockIdx.x, bits, wprefix, blocktot, wsum);   // (device_utils.hpp)
}

// ---- The set-up between k_sp_hist and the K-means in three launches.  Eleven small dispatches stand there otherwise -- the prefix of the
// bitmap in two steps, the scan of the cells in two, two fills, the initial centroids, the persistent launch's chunk boundaries, the emit,
// and the copy of the colour count -- and all but the emit sit at the few microseconds any dispatch costs; k_ps_ranges is one block's latency.
// Few of them depend on each other, so a block takes its ROLE from blockIdx, and every role is the body of the kernel it replaces:
//   A  k_bits_prefix | k_cell_totals | the zeroing of the K-means arena and of the head of the persistent launch's arena
//   B  k_gidx_finish | k_cell_scan                                   (the colour count is copied to the host behind B)
//   C  k_ps_ranges (block 0: dispatched first, ONE block as ever) | k_rgbw_init_cent | k_sp_emit, a 1024-thread block per bucket
//      (the persistent launch reading the staging itself: B's cell scan has written the boundaries, block 0 only checks that every
//      block's cells fit its LDS, and there is no emit role)
// No role reads what another role of its own launch writes, and no block waits for another: the order is the stream's.
constexpr uint32_t kFrontPrefixBlocks = 256;                    // blocks of 256 threads: k_bits_prefix's / k_gidx_finish's grid
constexpr uint32_t kFrontCellBlocks = kCellGroups / 4;          // ... and four groups of 64 cells to a block, a wave each
constexpr uint32_t kFrontZeroBlocks = 32;
static_assert(kCellGroups % 4 == 0, "four waves of a block each take a group of cells");
struct FrontA {
    const unsigned long long *bits; uint32_t *wprefix, *blocktot;
    const uint32_t *cell_count; uint2 *cell_tot;
    uint4 *zero0, *zero1; uint32_t n0, n1;                      // two ranges of n0 and n1 16-byte words to clear
};
__global__ __launch_bounds__(256) void k_cc_front_a(FrontA a) {
    __shared__ uint32_t wsum[256 / 64];
    const uint32_t b = blockIdx.x;
    if (b < kFrontPrefixBlocks) {
        bits_prefix_body(b, a.bits, a.wprefix, a.blocktot, wsum);
    } else if (b < kFrontPrefixBlocks + kFrontCellBlocks) {
        cell_totals_body((b - kFrontPrefixBlocks) * 4 + (threadIdx.x >> 6), threadIdx.x & 63u, a.cell_count, a.cell_tot);
    } else {
        const uint32_t t = (b - kFrontPrefixBlocks - kFrontCellBlocks) * 256 + threadIdx.x;
        for (uint32_t i = t; i < a.n0; i += kFrontZeroBlocks * 256) a.zero0[i] = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t i = t; i < a.n1; i += kFrontZeroBlocks * 256) a.zero1[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}
struct FrontB {
    uint32_t *wprefix; const uint32_t *blocktot; uint64_t *total;
    const uint32_t *cell_count; const uint2 *cell_tot; CellScanOut scan;
};
__global__ __launch_bounds__(256) void k_cc_front_b(FrontB a) {
    __shared__ uint32_t wsum[256 / 64];
    __shared__ uint32_t boff[256];
    const uint32_t b = blockIdx.x;
    if (b < kFrontPrefixBlocks) gidx_finish_body(b, a.wprefix, a.blocktot, a.total, wsum, boff);
    else cell_scan_body((b - kFrontPrefixBlocks) * 4 + (threadIdx.x >> 6), threadIdx.x & 63u, a.cell_count, a.cell_tot, a.scan, kCellFixedCost, kCellSweepCost);
}
struct FrontC {
    uint32_t ranges, cent_blocks;                               // blocks of the first two roles (ranges: 0 or 1); the buckets' follow (none when
                                                                // the persistent launch takes its points from the staging itself)
    uint32_t fit_only;                                          // the boundaries are there (B's cell scan wrote them): the ranges role checks the fit
    const uint32_t *ne_cost, *ne_count; uint32_t G, budget; uint32_t *cb; PsDev *dev; PsDevPtrs ptrs;
    uint64_t Ulist; uint32_t K, Kpad, idbits; uint2 *cconst; uint32_t *cent, *cent_copy, *moved_list; const uint64_t *U_dev; GIdx cgx;
    const uint32_t *sstart; const uint16_t *sbin; const uint32_t *scnt; SpEmit em;
};
__global__ __launch_bounds__(kSpThreads) void k_cc_front_c(FrontC a) {
    const uint32_t b = blockIdx.x;
    if (b < a.ranges) {
        if (a.fit_only) ps_fit_body(a.G, a.budget, a.cb, a.dev, a.ptrs);
        else ps_ranges_body(a.ne_cost, a.ne_count, a.G, a.budget, a.cb, a.dev, a.ptrs);
    } else if (b < a.ranges + a.cent_blocks) {
        rgbw_init_cent_body((b - a.ranges) * kSpThreads + threadIdx.x, nullptr, a.Ulist, a.K, a.Kpad, a.idbits, a.cconst, a.cent, a.cgx, a.cent_copy,
                            a.moved_list, a.U_dev);
    } else {
        static_assert(kSpThreads == 256 * kSpEmitSplit, "one block is the emit's 1024 threads of a bucket");
        sp_emit_body(b - a.ranges - a.cent_blocks, threadIdx.x, a.sstart, a.sbin, a.scnt, a.em);
    }
}

// ---- back end.  One block per bucket: LDS table bin -> final label from the bucket's points, then the label of
// every partitioned pixel, in partition order.
template <typename LabelT>
__global__ __launch_bounds__(kSpThreads) void k_sp_partlab(const uint16_t *__restrict__ part, const uint32_t *__restrict__ bstart,
                                                           const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ ckeys,
                                                           const LabelT *__restrict__ labels, LabelT *__restrict__ partlab,
                                                           unsigned long long *__restrict__ look, uint32_t look_words,
                                                           const uint32_t *__restrict__ sstart, const uint16_t *__restrict__ sbin) {
    extern __shared__ __align__(16) uint8_t sp_lds[];
    LabelT *lut = reinterpret_cast<LabelT *>(sp_lds);
    // (the ticket, the give-up word and the look-back words of the k_sp_pixpack behind this kernel start at zero: no dispatch of their own)
    if (look && blockIdx.x == 0 && blockIdx.y == 0)
        for (uint32_t i = threadIdx.x; i < look_words; i += kSpThreads) look[i] = 0ull;
    const uint32_t bucket = blockIdx.x;
    uint64_t s = bstart[bucket], e = bstart[bucket + 1];
    if (s == e) return;
    // a crowded bucket is several blocks' work (grid.y slices of at least kSpSliceMin entries; every slice builds the table: up to
    // 2^15 colours against >= 2^17 pixels)
    {
        const uint64_t len = e - s;
        const uint32_t slices = (uint32_t)min<uint64_t>(gridDim.y, max<uint64_t>(1, len / kSpSliceMin));
        if (blockIdx.y >= slices) return;
        const uint64_t per = ((len + slices - 1) / slices + 3) & ~3ull;
        const uint64_t a = s + per * blockIdx.y;
        e = min(e, a + per);
        s = a;
        if (s >= e) return;
    }
    const uint32_t q0 = cell_start[bucket * 64], q1 = cell_start[bucket * 64 + 64];
    if (sbin) {   // the bucket's colours as the histogram staged them (no ckeys: the K-means took its points from the staging too)
        const uint32_t s0 = sstart[bucket];
        for (uint32_t i = q0 + threadIdx.x; i < q1; i += kSpThreads) lut[sbin[s0 + (i - q0)]] = labels[i];
    } else {
        for (uint32_t i = q0 + threadIdx.x; i < q1; i += kSpThreads) lut[sp_bin(ckeys[i])] = labels[i];
    }
    __syncthreads();
    sp_for_entries(part, s, e, [&](uint64_t i, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t m) {
        if (m == 1) { partlab[i] = lut[a]; return; }
        if (sizeof(LabelT) == 1) {  // i is a multiple of 4
            *reinterpret_cast<uint32_t *>(partlab + i) = (uint32_t)lut[a] | ((uint32_t)lut[b] << 8) | ((uint32_t)lut[c] << 16) | ((uint32_t)lut[d] << 24);
        } else {
            *reinterpret_cast<uint2 *>(partlab + i) = make_uint2((uint32_t)lut[a] | ((uint32_t)lut[b] << 16), (uint32_t)lut[c] | ((uint32_t)lut[d] << 16));
        }
    });
}

// A chunk's 512 label runs into LDS: stage[j] = label of the pixel at place j of the chunk's bucket-sorted order.  The whole block calls;
// a barrier stands behind the last store.  off u32[kSpBuckets + 1], gsrc u32[kSpBuckets], wsum u32[kSpWaves]: LDS
template <typename LabelT>
__device__ __forceinline__ void sp_stage_labels(uint32_t chunk, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ pre,
                                                const uint32_t *__restrict__ bstart, const LabelT *__restrict__ partlab, LabelT *stage,
                                                uint32_t *off, uint32_t *gsrc, uint32_t *wsum) {
    const uint32_t *mycnt = cnt + (size_t)chunk * kSpBuckets, *mypre = pre + (size_t)chunk * kSpBuckets;
    const uint32_t n_b = threadIdx.x < kSpBuckets ? mycnt[threadIdx.x] : 0u;
    const uint32_t ex = scan512(n_b, wsum);
    if (threadIdx.x < kSpBuckets) off[threadIdx.x] = ex;
    if (threadIdx.x == kSpBuckets - 1) off[kSpBuckets] = ex + n_b;
    __syncthreads();
    // the chunk's 512 label runs come in: gsrc[b] = where bucket b's run of this chunk starts, minus its place in the stage
    if (threadIdx.x < kSpBuckets) gsrc[threadIdx.x] = bstart[threadIdx.x] + mypre[threadIdx.x] - off[threadIdx.x];
    __syncthreads();
    sp_walk_sorted<8>(off, off[kSpBuckets], [&](uint32_t j, const uint32_t (&jb)[8]) {
        LabelT got[8];
#pragma unroll
        for (int t = 0; t < 8; t++) got[t] = jb[t] != 0xffffffffu ? partlab[(size_t)(gsrc[jb[t]] + (j + 64 * t))] : (LabelT)0;
#pragma unroll
        for (int t = 0; t < 8; t++)
            if (jb[t] != 0xffffffffu) stage[j + 64 * t] = got[t];
    });
    __syncthreads();
}

// One block per chunk: its 512 label runs into LDS (the chunk's pixels in bucket-sorted order), then every pixel picks stage[prank].
// LDS (dynamic): stage LabelT[kSpChunk] | off u32[kSpBuckets + 1] | gsrc u32[kSpBuckets]
template <typename LabelT>
__global__ __launch_bounds__(kSpThreads) void k_sp_pixlab(const uint8_t *__restrict__ rgb, uint64_t npx, const uint32_t *__restrict__ cnt,
                                                          const uint32_t *__restrict__ pre, const uint32_t *__restrict__ bstart,
                                                          const LabelT *__restrict__ partlab, const uint16_t *__restrict__ prank,
                                                          LabelT *__restrict__ pixlab) {
    extern __shared__ __align__(16) uint8_t sp_lds[];
    LabelT *stage = reinterpret_cast<LabelT *>(sp_lds);
    uint32_t *off = reinterpret_cast<uint32_t *>(sp_lds + (size_t)kSpChunk * sizeof(LabelT));  // [kSpBuckets + 1]
    uint32_t *gsrc = off + kSpBuckets + 1;
    __shared__ uint32_t wsum[kSpWaves];
    sp_stage_labels(blockIdx.x, cnt, pre, bstart, partlab, stage, off, gsrc, wsum);
    // every pixel picks stage[its place in the sorted order] (prank, written by k_sp_scatter): 2 + 1 bytes per pixel, the
    // image itself is not read again
    const uint64_t p0 = (uint64_t)blockIdx.x * kSpChunk, p1 = min(npx, p0 + kSpChunk);
    for (uint64_t g = p0 / 16 + threadIdx.x; g * 16 < p1; g += kSpThreads) {
        const uint64_t first = g * 16;
        const uint32_t m = (uint32_t)min<uint64_t>(16, p1 - first);
        uint32_t lab[16];
        if (m == 16) {
            const uint4 *rp = reinterpret_cast<const uint4 *>(prank + first);
            const uint4 r0 = rp[0], r1 = rp[1];
            const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) lab[i] = stage[(rw[i >> 1] >> (16 * (i & 1))) & 0xffffu];
            if (sizeof(LabelT) == 1) {
                uint32_t w[4];
#pragma unroll
                for (int j = 0; j < 4; j++) w[j] = lab[4 * j] | (lab[4 * j + 1] << 8) | (lab[4 * j + 2] << 16) | (lab[4 * j + 3] << 24);
                *reinterpret_cast<uint4 *>(pixlab + first) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                uint4 *d = reinterpret_cast<uint4 *>(pixlab + first);
                d[0] = make_uint4(lab[0] | (lab[1] << 16), lab[2] | (lab[3] << 16), lab[4] | (lab[5] << 16), lab[6] | (lab[7] << 16));
                d[1] = make_uint4(lab[8] | (lab[9] << 16), lab[10] | (lab[11] << 16), lab[12] | (lab[13] << 16), lab[14] | (lab[15] << 16));
            }
        } else {
            for (uint32_t i = 0; i < m; i++) pixlab[first + i] = stage[prank[first + i]];
        }
    }
}

// ---- the pixel labels of a chunk straight into the Huffman stream (narrow labels): k_sp_pixlab's pick and the label pack's count, scan
// and write (k_huff.hip) in one kernel, so the label image -- written once and read twice -- never exists.
// Phase 1: the block stages the chunk's label runs and every thread picks its 64 labels (the 16-pixel groups tid + 1024 r of the chunk,
// r = 0..3, k_sp_pixlab's mapping) into registers, four to a word, and sums their code lengths round by round; ONE block scan of the four
// sums gives every thread its bit offset in every round, the rounds' bits and the chunk's.
// The chunk's first bit, a decoupled look-back: a block takes its chunk from a ticket counter, so the chunks before it belong to blocks
// that have started and wait for nobody before they publish.  Chunk i's word = state << 62 | bits: kLookAgg with the chunk's own bits as
// soon as phase 1 has them, kLookInc with the bits of chunks 0..i once its first bit is known (chunk 0 at once).  The word is the whole
// message, so it is stored and polled with relaxed agent-scope atomics and no fence (Guideline 16's 8-byte granule: nothing else is
// handed over).  Wave 0 looks at 256 words at a time, four a lane, and adds everything down to the nearest inclusive one.  Every spin
// watches the clock and the give-up word (as ps_spin, k_kmeans_persist.hip); who gives up sets that word, every block that sees it
// leaves, and the host packs from partlab with the split kernels, which clear the stream first.
// Phase 2: round by round pack_emit (device_utils.hpp), the pack's own emit.
// look: [0] ticket, [1] give-up, [2] the stream's payload bits (the last chunk's inclusive word without its state), [3 + i] chunk i's
// word -- zeroed by block (0, 0) of the k_sp_partlab in front; the host fetches [1] and [2] with one copy.
constexpr uint32_t kSpPackRounds = kSpChunk / (kSpThreads * 16);
constexpr uint32_t kSpPackImgWords = kSpThreads * 16 / 2 + 2;   // 16 bits per symbol of a round fit (a palette's codes average 8)
constexpr unsigned long long kLookAgg = 1ull << 62, kLookInc = 2ull << 62, kLookMask = (1ull << 62) - 1;
constexpr uint32_t kLookHead = 3, kLookPer = 4;   // words in front of the chunks'; words a lane of wave 0 looks at per window
constexpr size_t kSpPackDyn = (size_t)kSpChunk + kSpBuckets * 8 + 16;
struct SpPackArgs {
    const uint32_t *cnt, *pre, *bstart;
    const uint8_t *partlab;
    const uint16_t *prank;
    uint64_t npx;
    uint32_t nchunks, img_cap;
    const uint8_t *upl;             // the host's pinned block (kCcUp*, common.hpp): codes, lengths, the stream's header -- read where it lies
    uint32_t hdr_bytes;
    uint32_t *out_words;            // pre-zeroed
    uint64_t bit_base;
    unsigned long long *look;
    unsigned long long timeout_ticks;
    uint32_t test_giveup;           // tests: give up at the first poll
};
__device__ __forceinline__ unsigned long long look_ld(unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void look_st(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kSpThreads) void k_sp_pixpack(SpPackArgs a) {
    extern __shared__ __align__(16) uint8_t sp_lds[];
    uint8_t *stage = sp_lds;
    uint32_t *off = reinterpret_cast<uint32_t *>(sp_lds + (size_t)kSpChunk);  // [kSpBuckets + 1]
    uint32_t *gsrc = off + kSpBuckets + 1;
    __shared__ unsigned long long s_tab[256], s_excl;
    __shared__ uint32_t img[kSpPackImgWords];
    __shared__ uint32_t wsum[kSpWaves], s_rsum[kSpPackRounds][kSpWaves], s_chunk, s_ok;
    __shared__ uint8_t s_len[256];
    // stage 64 KiB + offsets 4 KiB + codes 2.3 KiB + bit image 32 KiB: one block per CU
    static_assert(kSpPackDyn + 8 * 257 + 4 * kSpPackImgWords + 4 * ((1 + kSpPackRounds) * kSpWaves + 2) + 256 + 64 <= 160 * 1024, "the LDS of k_sp_pixpack");
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_chunk = atomicAdd(reinterpret_cast<uint32_t *>(a.look), 1u); s_excl = 0ull; s_ok = 1u; }
    // the codes and the header come straight from the host's pinned block (no copy dispatch in front of this kernel): asked for now,
    // used behind the staging, which hides the trip
    unsigned long long tcode = 0;
    uint32_t tlen = 0;
    if (tid < 256) { tcode = reinterpret_cast<const unsigned long long *>(a.upl + kCcUpCode)[tid]; tlen = a.upl[kCcUpLen + tid]; }
    __syncthreads();
    const uint32_t chunk = s_chunk;
    if (chunk >= a.nchunks) return;   // (cannot be: the grid is nchunks blocks and the ticket starts at zero)
    constexpr uint32_t kHdrPer = (kCcUpBytes - kCcUpHdr) / 4 / kSpThreads + 1;
    uint32_t hv[kHdrPer];
    const uint32_t hw = chunk == 0 ? (a.hdr_bytes + 3u) / 4u : 0u;
#pragma unroll
    for (uint32_t q = 0; q < kHdrPer; q++) { const uint32_t i = tid + kSpThreads * q; hv[q] = i < hw ? reinterpret_cast<const uint32_t *>(a.upl + kCcUpHdr)[i] : 0u; }
    // the thread's 64 ranks are asked for now: they need nothing of the stage and arrive while it is filled (a ragged last group reads
    // its 16 ranks all the same: prank has 16 entries of slack, and any rank is a place of the stage)
    const uint64_t p0 = (uint64_t)chunk * kSpChunk, p1 = min(a.npx, p0 + kSpChunk);
    uint4 pr[kSpPackRounds][2];
#pragma unroll
    for (uint32_t r = 0; r < kSpPackRounds; r++) {
        const uint64_t first = p0 + ((uint64_t)tid + kSpThreads * r) * 16;
        const uint4 *rp = reinterpret_cast<const uint4 *>(a.prank + first);
        pr[r][0] = first < p1 ? rp[0] : make_uint4(0, 0, 0, 0);
        pr[r][1] = first < p1 ? rp[1] : make_uint4(0, 0, 0, 0);
    }
    sp_stage_labels<uint8_t>(chunk, a.cnt, a.pre, a.bstart, a.partlab, stage, off, gsrc, wsum);
    if (tid < 256) { s_tab[tid] = tcode; s_len[tid] = (uint8_t)tlen; }
    // the header, as words OR-ed in like everything else: its last word may hold the payload's first bits
#pragma unroll
    for (uint32_t q = 0; q < kHdrPer; q++) { const uint32_t i = tid + kSpThreads * q; if (i < hw && hv[q]) atomicOr(&a.out_words[i], hv[q]); }
    __syncthreads();
    // ---- phase 1
    const uint32_t lane = tid & 63u, wid = tid >> 6;
    uint32_t lw[kSpPackRounds][4], wexcl[kSpPackRounds];   // the packed labels; the bits of the wave's lanes before this one, per round
#pragma unroll
    for (uint32_t r = 0; r < kSpPackRounds; r++) {
        const uint64_t first = p0 + ((uint64_t)tid + kSpThreads * r) * 16;
        const uint32_t m = first < p1 ? (uint32_t)min<uint64_t>(16, p1 - first) : 0u;
        uint32_t lab[16], bits = 0;
        const uint32_t rw[8] = {pr[r][0].x, pr[r][0].y, pr[r][0].z, pr[r][0].w, pr[r][1].x, pr[r][1].y, pr[r][1].z, pr[r][1].w};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) lab[i] = stage[(rw[i >> 1] >> (16 * (i & 1))) & 0xffffu];
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) bits += i < m ? (uint32_t)s_len[lab[i]] : 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) lw[r][j] = lab[4 * j] | (lab[4 * j + 1] << 8) | (lab[4 * j + 2] << 16) | (lab[4 * j + 3] << 24);
        // (a word the compiler cannot see through: it kept the 64 labels it had packed in a register each, for phase 2 to come, and
        // spilled -- tests/test_kernel_resources_cpu.py holds the kernel to a scratch size of zero)
#pragma unroll
        for (int j = 0; j < 4; j++) asm volatile("" : "+v"(lw[r][j]));
        const uint32_t inc = wave_inclusive_scan(bits);
        wexcl[r] = inc - bits;
        if (lane == 63) s_rsum[r][wid] = inc;
    }
    __syncthreads();
    uint32_t total = 0;   // (a chunk has at most 2^16 x 64 bits)
#pragma unroll
    for (uint32_t r = 0; r < kSpPackRounds; r++)
#pragma unroll
        for (uint32_t i = 0; i < kSpWaves; i++) total += s_rsum[r][i];
    // ---- the chunk's first bit
    if (tid < 64) {
        unsigned long long *W = a.look + kLookHead;
        uint32_t *giveup = reinterpret_cast<uint32_t *>(a.look + 1);
        bool ok = true;
        unsigned long long mine = 0;   // what this lane adds to the bits in front of the chunk
        if (chunk == 0) {
            if (tid == 0) look_st(&W[0], kLookInc | total);
        } else {
            if (tid == 0) look_st(&W[chunk], kLookAgg | total);
            const unsigned long long t0 = wall_clock64();
            long long hi = (long long)chunk - 1;
            for (bool found = false; !found; hi -= 64 * kLookPer) {
                unsigned long long v[kLookPer];
                for (uint32_t spins = 0;;) {
                    bool ready = true;
#pragma unroll
                    for (uint32_t k = 0; k < kLookPer; k++) {
                        const long long j = hi - (long long)(tid + 64 * k);
                        v[k] = j >= 0 ? look_ld(&W[j]) : kLookInc;
                        ready = ready && (v[k] >> 62) != 0;
                    }
                    if (a.test_giveup) { ok = false; break; }
                    if (__all(ready)) break;
                    __builtin_amdgcn_s_sleep(1);
                    // (the wave leaves together: one lane's clock past the limit takes all of them)
                    if ((++spins & 63u) == 0 && __any(__hip_atomic_load(giveup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || wall_clock64() - t0 > a.timeout_ticks)) { ok = false; break; }
                }
                if (!ok) break;
#pragma unroll
                for (uint32_t k = 0; k < kLookPer; k++) {   // nearest first: words chunk - 1 - (64 k + lane)
                    const bool there = hi - (long long)(tid + 64 * k) >= 0;
                    const unsigned long long inc = __ballot(there && (v[k] >> 62) == 2);
                    const uint32_t nearest = inc ? (uint32_t)__builtin_ctzll(inc) : 64u;
                    if (!found && there && tid <= nearest) mine += v[k] & kLookMask;
                    found = found || inc != 0;   // (chunk 0's word is inclusive from the start: a window without one has 256 words and more in front of it)
                }
            }
        }
        const unsigned long long sum = wave_inclusive_scan64<false>(mine);   // lane 63: the bits in front of the chunk
        if (tid == 63) {
            if (!ok) {
                __hip_atomic_store(giveup, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_ok = 0u;
            } else {
                s_excl = sum;
                if (chunk) look_st(&W[chunk], kLookInc | (sum + total));
                if (chunk == a.nchunks - 1) look_st(a.look + 2, sum + total);
            }
        }
    }
    __syncthreads();
    if (!s_ok) return;
    const uint64_t g0 = a.bit_base + s_excl;
    // ---- phase 2
    uint32_t run = 0;
#pragma unroll
    for (uint32_t r = 0; r < kSpPackRounds; r++) {
        const uint64_t first = p0 + ((uint64_t)tid + kSpThreads * r) * 16;
        const uint32_t m = first < p1 ? (uint32_t)min<uint64_t>(16, p1 - first) : 0u;
        uint32_t lab[16], l[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            lab[i] = (lw[r][i >> 2] >> (8 * (i & 3))) & 255u;
            l[i] = i < m ? (uint32_t)s_len[lab[i]] : 0u;
        }
        uint32_t before = 0, rtot = 0;   // the waves' sums of the round stay where phase 1 left them
#pragma unroll
        for (uint32_t i = 0; i < kSpWaves; i++) { const uint32_t v = s_rsum[r][i]; rtot += v; if (i < wid) before += v; }
        pack_emit<kSpThreads, 16>(lab, l, before + wexcl[r], rtot, g0 + run, s_tab, img, min(kSpPackImgWords, a.img_cap), a.out_words);
        run += rtot;
        __syncthreads();   // (img is the next round's)
    }
}

// =========================================================================== host
static int sp_set_lds(Ctx *c) {
    static bool done = false;  // (function attributes are per process)
    if (done) return CNIIC_OK;
    const int big = 140 * 1024;
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_scatter), hipFuncAttributeMaxDynamicSharedMemorySize, big));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_hist), hipFuncAttributeMaxDynamicSharedMemorySize, big));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_partlab<uint8_t>), hipFuncAttributeMaxDynamicSharedMemorySize, big));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_partlab<uint16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, big));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_pixlab<uint8_t>), hipFuncAttributeMaxDynamicSharedMemorySize, big));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_pixlab<uint16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, big));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_sp_pixpack), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpPackDyn));   // (beside 35 KiB of static LDS)
    done = true;
    return CNIIC_OK;
}

// pixels -> partition + occupied colours per cell + occupancy bitmap with its prefix.  Nothing waits: the number of
// distinct colours stays on the device (plan->total) for the set-up kernels that follow, and sp_wait_count fetches it
// hist_only: ends behind k_sp_hist -- the prefix of the bitmap and the copy of the count are then the caller's to enqueue, with the K-means'
// set-up (sp_front)
int sp_build(Ctx *c, const uint8_t *rgb_d, uint64_t npx, SpPlan *plan, bool hist_only) {
    if (npx == 0 || (reinterpret_cast<uintptr_t>(rgb_d) & 15)) return c->fail(CNIIC_ERR_BAD_ARG, "sp_build: empty or unaligned image");
    CNIIC_TRY(sp_set_lds(c));
    plan->npx = npx;
    plan->nchunks = (uint32_t)ceil_div(npx, kSpChunk);
    const uint64_t nc = plan->nchunks;
    CNIIC_HIP_TRY(c, plan->cnt.alloc(nc * kSpBuckets * 4));
    CNIIC_HIP_TRY(c, plan->pre.alloc(nc * kSpBuckets * 4));
    CNIIC_HIP_TRY(c, plan->bstart.alloc(((uint64_t)kSpBuckets + 1) * 4));
    CNIIC_HIP_TRY(c, plan->part.alloc(npx * 2 + 16));
    CNIIC_HIP_TRY(c, plan->prank.alloc((npx + 16) * 2));
    CNIIC_HIP_TRY(c, plan->cell_count.alloc((uint64_t)kNumCells * 4));
    const uint64_t smax = std::min<uint64_t>(npx, 1ull << 24);  // distinct colours at most
    CNIIC_HIP_TRY(c, plan->sstart.alloc((uint64_t)kSpBuckets * 4));
    CNIIC_HIP_TRY(c, plan->sbin.alloc(smax * 2));
    CNIIC_HIP_TRY(c, plan->scnt.alloc(smax * 4));
    CNIIC_HIP_TRY(c, plan->bits.alloc((1ull << 18) * 8));
    CNIIC_HIP_TRY(c, plan->wprefix.alloc((1ull << 18) * 4));
    DevBuf total, blocktot;
    CNIIC_HIP_TRY(c, total.alloc((uint64_t)kSpBuckets * 4));
    if (!hist_only) CNIIC_HIP_TRY(c, blocktot.alloc(256 * 4));
    CNIIC_HIP_TRY(c, plan->total.alloc(8));
    CNIIC_HIP_TRY(c, c->pinned_u.reserve(kPinnedUBytes, kPinnedUBytes));
    CNIIC_HIP_TRY(c, c->u_ev.ensure(hipEventDisableTiming));
    hipLaunchKernelGGL(k_sp_count, dim3(plan->nchunks), dim3(kSpThreads), 0, c->stream, rgb_d, npx, plan->cnt.as<uint32_t>());
    hipLaunchKernelGGL(k_sp_colscan, dim3(kSpBuckets), dim3(256), 0, c->stream, plan->cnt.as<uint32_t>(), plan->nchunks,
                       plan->pre.as<uint32_t>(), total.as<uint32_t>());
    hipLaunchKernelGGL(k_sp_scatter, dim3(plan->nchunks), dim3(kSpThreads), (size_t)kSpChunk * 2 + kSpBuckets * 8 + 16, c->stream, rgb_d, npx,
                       plan->cnt.as<uint32_t>(), plan->pre.as<uint32_t>(), (const uint32_t *)total.as<uint32_t>(), plan->bstart.as<uint32_t>(),
                       plan->sstart.as<uint32_t>(), plan->part.as<uint16_t>(), plan->prank.as<uint16_t>());
    hipLaunchKernelGGL(k_sp_hist, dim3(kSpBuckets), dim3(kSpThreads), (size_t)kSpBins * 4, c->stream, plan->part.as<uint16_t>(),
                       plan->bstart.as<uint32_t>(), plan->sstart.as<uint32_t>(), plan->cell_count.as<uint32_t>(), plan->bits.as<uint32_t>(),
                       plan->sbin.as<uint16_t>(), plan->scnt.as<uint32_t>());
    if (hist_only) { CNIIC_HIP_TRY(c, hipGetLastError()); return CNIIC_OK; }
    hipLaunchKernelGGL(k_bits_prefix, dim3(256), dim3(256), 0, c->stream, plan->bits.as<unsigned long long>(), plan->wprefix.as<uint32_t>(),
                       blocktot.as<uint32_t>());
    CNIIC_TRY(gidx_finish(c, plan->wprefix.as<uint32_t>(), blocktot.as<uint32_t>(), plan->total.as<uint64_t>()));
    CNIIC_HIP_TRY(c, hipGetLastError());
    CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuSpCount.at, plan->total.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipEventRecord(c->u_ev, c->stream));
    return CNIIC_OK;
}

// Behind sp_build(hist_only): everything between k_sp_hist and the K-means of state f describes (km_rgbw_create_deferred) -- the prefix of
// the bitmap, the copy of the colour count with its event, the state's set-up dispatches and the emit into its arrays (the point list is
// the image's own: plan's bitmap).  fused: the three launches k_cc_front_a / b / c; else the kernels and fills one by one, as sp_build,
// km_rgbw_create and sp_emit enqueue them.
int sp_front(Ctx *c, SpPlan *plan, const KmFront &f, uint32_t *ckeys_d, uint32_t *cweight_d, void *labels_d, bool wide, bool fused, bool emit, bool count_copy) {
    DevBuf blocktot;   // (lives until everything here is enqueued: the pool hands memory out again in stream order)
    CNIIC_HIP_TRY(c, blocktot.alloc(256 * 4));
    const uint64_t *U_dev = plan->total.as<uint64_t>();
    const GIdx gx{plan->bits.as<unsigned long long>(), plan->wprefix.as<uint32_t>(), 0};
    const SpEmit em{f.scan.cell_start, ckeys_d, cweight_d, labels_d, f.K, wide ? 1u : 0u, gx, U_dev};
    if (!fused) {
        hipLaunchKernelGGL(k_bits_prefix, dim3(256), dim3(256), 0, c->stream, plan->bits.as<unsigned long long>(), plan->wprefix.as<uint32_t>(),
                           blocktot.as<uint32_t>());
        CNIIC_TRY(gidx_finish(c, plan->wprefix.as<uint32_t>(), blocktot.as<uint32_t>(), plan->total.as<uint64_t>()));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuSpCount.at, plan->total.p, 8, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipEventRecord(c->u_ev, c->stream));
        CNIIC_TRY(km_front_enqueue_split(c, f));
        hipLaunchKernelGGL(k_sp_emit, dim3(kSpBuckets * kSpEmitSplit), dim3(256), 0, c->stream, plan->sstart.as<uint32_t>(), plan->sbin.as<uint16_t>(),
                           plan->scnt.as<uint32_t>(), em);
        CNIIC_HIP_TRY(c, hipGetLastError());
        return CNIIC_OK;
    }
    FrontA a{};
    a.bits = plan->bits.as<unsigned long long>(); a.wprefix = plan->wprefix.as<uint32_t>(); a.blocktot = blocktot.as<uint32_t>();
    a.cell_count = f.cell_count; a.cell_tot = f.cell_tot.as<uint2>();
    a.zero0 = static_cast<uint4 *>(f.arena); a.n0 = (uint32_t)(f.arena_bytes / 16);
    a.zero1 = static_cast<uint4 *>(f.ps_arena); a.n1 = f.ranges ? (uint32_t)(f.ps_zero_bytes / 16) : 0u;
    hipLaunchKernelGGL(k_cc_front_a, dim3(kFrontPrefixBlocks + kFrontCellBlocks + kFrontZeroBlocks), dim3(256), 0, c->stream, a);
    FrontB b{};
    b.wprefix = a.wprefix; b.blocktot = a.blocktot; b.total = plan->total.as<uint64_t>();
    b.cell_count = f.cell_count; b.cell_tot = a.cell_tot; b.scan = f.scan;
    const bool direct = !emit && f.ranges;   // (with the staged points: the cell scan writes the chunk boundaries, no bisection in C)
    if (direct) { b.scan.cb = f.cb; b.scan.NC = f.G * kPsChunks; }
    hipLaunchKernelGGL(k_cc_front_b, dim3(kFrontPrefixBlocks + kFrontCellBlocks), dim3(256), 0, c->stream, b);
    CNIIC_HIP_TRY(c, hipGetLastError());
    if (count_copy) CNIIC_TRY(sp_enqueue_count(c, plan));
    FrontC k{};
    k.fit_only = direct ? 1u : 0u;
    k.ranges = f.ranges ? 1u : 0u; k.cent_blocks = (uint32_t)ceil_div(f.Kpad, kSpThreads);
    k.ne_cost = f.scan.ne_cost; k.ne_count = f.scan.ne_count; k.G = f.G; k.budget = f.budget; k.cb = f.cb; k.dev = f.dev; k.ptrs = f.ptrs;
    k.Ulist = f.Ulist; k.K = f.K; k.Kpad = f.Kpad; k.idbits = f.idbits; k.cconst = f.cconst; k.cent = f.cent; k.cent_copy = f.cent_copy;
    k.moved_list = f.moved_list; k.U_dev = f.U_dev; k.cgx = f.gx;
    k.sstart = plan->sstart.as<uint32_t>(); k.sbin = plan->sbin.as<uint16_t>(); k.scnt = plan->scnt.as<uint32_t>(); k.em = em;
    hipLaunchKernelGGL(k_cc_front_c, dim3(k.ranges + k.cent_blocks + (emit ? kSpBuckets : 0u)), dim3(kSpThreads), 0, c->stream, k);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}
// whether sp_front's launches can clear what f asks to be cleared (whole 16-byte words at 16-byte addresses)
bool sp_front_fits(const KmFront &f) {
    auto ok = [](const void *p, uint64_t n) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && n % 16 == 0 && n / 16 < (1ull << 32); };
    return ok(f.arena, f.arena_bytes) && (!f.ranges || ok(f.ps_arena, f.ps_zero_bytes));
}

int sp_enqueue_count(Ctx *c, SpPlan *plan) {
    CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuSpCount.at, plan->total.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipEventRecord(c->u_ev, c->stream));
    return CNIIC_OK;
}
int sp_wait_count(Ctx *c, SpPlan *plan) {
    CNIIC_HIP_TRY(c, hipEventSynchronize(c->u_ev));
    plan->U = c->pinned_u.as<uint64_t>()[kPuSpCount.at];
    return CNIIC_OK;
}

// the distinct colours, counts and initial labels into the K-means state's cell-major arrays (cell_start: its scan of
// plan->cell_count); gx: the index of the reference's point list (this image's own bitmap, or the union's)
int sp_emit(Ctx *c, const SpPlan *plan, const uint32_t *cell_start_d, uint32_t *ckeys_d, uint32_t *cweight_d, void *labels_d, bool wide,
            uint32_t K, const void *gbits_d, const uint32_t *gprefix_d, uint64_t Ug, const uint64_t *Ug_dev) {
    const GIdx gx{static_cast<const unsigned long long *>(gbits_d), gprefix_d, Ug};
    hipLaunchKernelGGL(k_sp_emit, dim3(kSpBuckets * kSpEmitSplit), dim3(256), 0, c->stream, plan->sstart.as<uint32_t>(), plan->sbin.as<uint16_t>(),
                       plan->scnt.as<uint32_t>(), SpEmit{cell_start_d, ckeys_d, cweight_d, labels_d, K, wide ? 1u : 0u, gx, Ug_dev});
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// occupancy of this image's colours as one nibble per colour (u32[2^21]), the form the ranks sum (k_hist.hip: k_occ_pack)
__global__ __launch_bounds__(256) void k_occ_from_bits(const uint32_t *__restrict__ bits32, uint32_t *__restrict__ occ) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;  // occ word i = colours 8 i .. 8 i + 7
    const uint32_t byte = (bits32[i >> 2] >> (8 * (i & 3))) & 255u;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) v |= ((byte >> j) & 1u) << (4 * j);
    occ[i] = v;
}
int sp_occupancy(Ctx *c, const SpPlan *plan, uint32_t *occ_d) {
    hipLaunchKernelGGL(k_occ_from_bits, dim3((1u << 21) / 256), dim3(256), 0, c->stream, plan->bits.as<uint32_t>(), occ_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// labels_d: the K-means' final cell-major labels -> partlab: label of every pixel in partition order.  look (optional, narrow labels): the
// ticket and look-back words of sp_pixpack, allocated here and zeroed by the kernel
int sp_part_labels(Ctx *c, const SpPlan *plan, const uint32_t *cell_start_d, const uint32_t *ckeys_d, const void *labels_d, bool wide, DevBuf &partlab,
                   DevBuf *look, bool staged) {
    const uint32_t *sstart = staged ? plan->sstart.as<uint32_t>() : nullptr;
    const uint16_t *sbin = staged ? plan->sbin.as<uint16_t>() : nullptr;
    const uint64_t lb = wide ? 2 : 1;
    CNIIC_HIP_TRY(c, partlab.alloc(plan->npx * lb + 16));
    const uint32_t look_words = look ? plan->nchunks + kLookHead : 0;
    if (look) CNIIC_HIP_TRY(c, look->alloc((uint64_t)look_words * 8));
    const dim3 grid(kSpBuckets, plan->npx >= 2 * (uint64_t)kSpSliceMin ? kSpSlices : 1);
    if (wide)
        hipLaunchKernelGGL(k_sp_partlab<uint16_t>, grid, dim3(kSpThreads), (size_t)kSpBins * 2, c->stream, plan->part.as<uint16_t>(),
                           plan->bstart.as<uint32_t>(), cell_start_d, ckeys_d, static_cast<const uint16_t *>(labels_d), partlab.as<uint16_t>(),
                           (unsigned long long *)nullptr, 0u, sstart, sbin);
    else
        hipLaunchKernelGGL(k_sp_partlab<uint8_t>, grid, dim3(kSpThreads), (size_t)kSpBins, c->stream, plan->part.as<uint16_t>(),
                           plan->bstart.as<uint32_t>(), cell_start_d, ckeys_d, static_cast<const uint8_t *>(labels_d), partlab.as<uint8_t>(),
                           look ? look->as<unsigned long long>() : nullptr, look_words, sstart, sbin);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// partlab -> pixlab_d: label of every pixel in image order
int sp_pixlab(Ctx *c, const SpPlan *plan, const uint8_t *rgb_d, const void *partlab_d, bool wide, void *pixlab_d) {
    if (wide)
        hipLaunchKernelGGL(k_sp_pixlab<uint16_t>, dim3(plan->nchunks), dim3(kSpThreads), (size_t)kSpChunk * 2 + kSpBuckets * 8 + 16, c->stream, rgb_d,
                           plan->npx, plan->cnt.as<uint32_t>(), plan->pre.as<uint32_t>(), plan->bstart.as<uint32_t>(), static_cast<const uint16_t *>(partlab_d),
                           plan->prank.as<uint16_t>(), static_cast<uint16_t *>(pixlab_d));
    else
        hipLaunchKernelGGL(k_sp_pixlab<uint8_t>, dim3(plan->nchunks), dim3(kSpThreads), (size_t)kSpChunk + kSpBuckets * 8 + 16, c->stream, rgb_d,
                           plan->npx, plan->cnt.as<uint32_t>(), plan->pre.as<uint32_t>(), plan->bstart.as<uint32_t>(), static_cast<const uint8_t *>(partlab_d),
                           plan->prank.as<uint16_t>(), static_cast<uint8_t *>(pixlab_d));
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// labels_d: the K-means' final cell-major labels -> pixlab_d: label of every pixel in image order
int sp_pixel_labels(Ctx *c, const SpPlan *plan, const uint8_t *rgb_d, const uint32_t *cell_start_d, const uint32_t *ckeys_d,
                    const void *labels_d, bool wide, void *pixlab_d) {
    DevBuf partlab;
    CNIIC_TRY(sp_part_labels(c, plan, cell_start_d, ckeys_d, labels_d, wide, partlab, nullptr, false));
    return sp_pixlab(c, plan, rgb_d, partlab.p, wide, pixlab_d);
}

// partlab (narrow labels) -> the Huffman payload behind hdr_bytes of out_d (4-byte aligned, pre-zeroed) and the header in front of it, from the
// host's pinned block upl_h (kCcUp*, common.hpp), which the kernel reads where it lies.  look: from sp_part_labels.  done_h: two pinned
// words that one copy behind the kernel fills -- [0] != 0: a block gave the look-back up and the stream is not complete (the caller packs
// with sp_pixlab + huff_pack_labels), [1] the payload's bits.  Asynchronous: the words are there when the stream has been waited for.
int sp_pixpack(Ctx *c, const SpPlan *plan, const void *partlab_d, DevBuf &look, const uint8_t *upl_h, uint32_t hdr_bytes, uint8_t *out_d, uint64_t *done_h) {
    if (reinterpret_cast<uintptr_t>(out_d) & 3) return c->fail(CNIIC_ERR_BAD_ARG, "sp_pixpack: output must be 4-byte aligned");
    CNIIC_TRY(sp_set_lds(c));
    SpPackArgs a{};
    a.cnt = plan->cnt.as<uint32_t>(); a.pre = plan->pre.as<uint32_t>(); a.bstart = plan->bstart.as<uint32_t>();
    a.partlab = static_cast<const uint8_t *>(partlab_d); a.prank = plan->prank.as<uint16_t>();
    a.npx = plan->npx; a.nchunks = plan->nchunks; a.img_cap = pack_img_cap();
    a.upl = upl_h; a.hdr_bytes = hdr_bytes; a.out_words = reinterpret_cast<uint32_t *>(out_d); a.bit_base = (uint64_t)hdr_bytes * 8;
    a.look = look.as<unsigned long long>();
    a.timeout_ticks = 2000ull * 100000ull;   // 2 s at 100 MHz, as the persistent K-means
    a.test_giveup = test_env("CNIIC_TEST_CC_TAIL_GIVEUP") ? 1u : 0u;
    hipLaunchKernelGGL(k_sp_pixpack, dim3(plan->nchunks), dim3(kSpThreads), kSpPackDyn, c->stream, a);
    CNIIC_HIP_TRY(c, hipGetLastError());
    CNIIC_HIP_TRY(c, hipMemcpyAsync(done_h, look.as<unsigned long long>() + 1, 16, hipMemcpyDeviceToHost, c->stream));
    return CNIIC_OK;
}

}  // namespace cniic
