// k_linearize.hip -- the reference's three linearisations of an image and the per-channel difference histogram of one
// (reference: src/hilbert.rs:10-32 linearize_rect / linearize_small / linearize_large, written out as CSV by src/main.rs:23-55
//  `--special=hilbert`; scripts/experiments/hilbert_distribution.py for the histogram).
//
//   rect   out[d] = img(scan_{w x h}(d))                                   -- hilbert_linearize (k_hilbert.hip), unchanged
//   small  s = min(npot(w) >> 1, npot(h) >> 1): out[d] = img(scan_{s x s}(d)), the top-left s x s crop read in place (row pitch w)
//   large  S = max(npot(w), npot(h)): the scan of S x S, only the positions inside the image kept, in their order
//
// `large` never walks the S^2 positions (a 1 x 2^29 strip has 2^58).  On the classic curve the rank of a kept pixel -- the kept
// positions before it -- is a sum over the levels of the descent to it: at each level the quadrants the sub-curve visits BEFORE the
// pixel's quadrant are axis-aligned squares, each adds the area of its intersection with [0, w) x [0, h):
//   rank(x, y) = sum over levels k = L-1 .. 0 of  sum over q' < q_k of  |Q(k, q') n image|,   L = log2 S
// One block per 64 x 64 tile of the square that meets the image (enumerated in image space): the levels above the tile give the tile's
// entry state and its rank base once per block; the tile is 4096 consecutive curve positions, read from the image row by row into
// LDS, marked in scan order, the marks scanned over the block, the kept pixels compacted in LDS and written as contiguous bytes
// behind the base.  The same kernel serves `small` from 64 x 64 (every position kept: base = 4096 x tile number).
// An injected scan for exactly S x S (cniic_ctx_set_scan) has no such structure: kept flags over its S^2 positions, a scan of the
// per-block counts, a gather -- S^2 is bounded by what was injected.  It doubles as the cross-check of the analytic route.
#include <algorithm>

#include "common.hpp"
#include "device_utils.hpp"
#include "hilbert_scan.hpp"

namespace cniic {

namespace {

// u32::next_power_of_two for v < 2^30 (npot(0) = 1)
inline uint32_t npot(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline uint32_t log2_exact(uint32_t p) {
    uint32_t o = 0;
    while ((1u << o) < p) o++;
    return o;
}
inline bool dims_ok(uint32_t w, uint32_t h) {   // check_dims of k_hilbert.hip
    return w < (1u << 30) && h < (1u << 30) && (uint64_t)w * h < (1ull << 32);
}

// ---------------------------------------------------------------- the descent on the classic curve
// pixels of [0, lim) inside [o, o + side)
__device__ __forceinline__ uint64_t clip_len(uint32_t o, uint32_t side, uint32_t lim) { return o >= lim ? 0u : (lim - o < side ? lim - o : side); }

// One level: the sub-curve in state st over the square of side 2 * half at (ox, oy) continues into its quadrant (qx, qy); the
// quadrants it visits before that one add what they share with the image.  l1: HilbertLut::l1 (x | y << 1 | next state << 2).
__device__ __forceinline__ void large_level(const uint8_t *l1, uint32_t &st, uint32_t &ox, uint32_t &oy, uint64_t &rank, uint32_t half, uint32_t qx,
                                            uint32_t qy, uint32_t w, uint32_t h) {
    const uint32_t want = qx | (qy << 1);
    uint32_t ns = 0;
    bool found = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t e = l1[st * 4 + q];
        if (!found) {
            if ((e & 3u) == want) { found = true; ns = e >> 2; }
            else rank += clip_len(ox + (e & 1u) * half, half, w) * clip_len(oy + ((e >> 1) & 1u) * half, half, h);
        }
    }
    ox += qx * half; oy += qy * half; st = ns;
}

// `large` on squares below 64 x 64 (the image has at most 32 x 32 pixels): one block, a pixel per lane, the whole descent
__global__ __launch_bounds__(256) void k_lin_large_px(const uint8_t *__restrict__ src, uint32_t w, uint32_t h, uint32_t L, const HilbertLut *__restrict__ lut,
                                                      uint8_t *__restrict__ dst) {
    __shared__ uint8_t s_l1[16];
    if (threadIdx.x < 16) s_l1[threadIdx.x] = lut->l1[threadIdx.x];
    __syncthreads();
    const uint64_t n = (uint64_t)w * h;
    for (uint64_t p = threadIdx.x; p < n; p += blockDim.x) {
        const uint32_t x = (uint32_t)(p % w), y = (uint32_t)(p / w);
        uint32_t st = 0, ox = 0, oy = 0;
        uint64_t rank = 0;
        for (uint32_t k = L; k-- > 0;) large_level(s_l1, st, ox, oy, rank, 1u << k, (x >> k) & 1u, (y >> k) & 1u, w, h);
        store_px3(dst + 3 * rank, px_le24(src, p, n));
    }
}

// where pixel (x, y) of a tile lies in LDS: rows of 64 words, the low bits of x XOR-ed with the 4-row group so that the lanes of the
// scan-order pass (each in a 4 x 4 block of its own, 8 x 4 such blocks per half wave) do not pile up on the banks of x alone
__device__ __forceinline__ uint32_t tile_at(uint32_t x, uint32_t y) { return (y << 6) | (x ^ ((y >> 2) & 3u)); }

// The part of the 2^L square (L >= 6) inside the w x h image (row pitch `pitch` pixels, n_img pixels in the buffer), by 64 x 64 tiles.
__global__ __launch_bounds__(256) void k_lin_tiles(const uint8_t *__restrict__ src, uint32_t pitch, uint64_t n_img, uint32_t w, uint32_t h, uint32_t L,
                                                   const HilbertLut *__restrict__ lut, uint8_t *__restrict__ dst) {
    __shared__ uint32_t s_tile[64 * 64];   // the tile's pixels, r | g << 8 | b << 16
    __shared__ uint32_t s_out[64 * 64];    // the kept ones in scan order
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_total;
    __shared__ uint8_t s_l1[16];
    __shared__ uint8_t s_l3[4 * 64];       // three levels from state s for six bits q: x:3 | y:3 << 3 | end state << 6
    if (threadIdx.x < 16) s_l1[threadIdx.x] = lut->l1[threadIdx.x];
    __syncthreads();
    {
        uint32_t st = threadIdx.x >> 6, x = 0, y = 0;
        for (int lv = 2; lv >= 0; lv--) {
            const uint32_t e = s_l1[st * 4 + ((threadIdx.x >> (2 * lv)) & 3)];
            x = (x << 1) | (e & 1); y = (y << 1) | ((e >> 1) & 1); st = e >> 2;
        }
        s_l3[threadIdx.x] = (uint8_t)(x | (y << 3) | (st << 6));
    }
    const uint32_t tw = (w + 63) >> 6, th = (h + 63) >> 6, ntiles = tw * th;   // (w h < 2^32: fewer than 2^25 tiles)
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t tx = tile % tw, ty = tile / tw;
        uint32_t st = 0, ox = 0, oy = 0;
        uint64_t base = 0;   // kept positions before the tile
        for (uint32_t k = L; k-- > 6;) large_level(s_l1, st, ox, oy, base, 1u << k, ((tx << 6) >> k) & 1u, ((ty << 6) >> k) & 1u, w, h);
        __syncthreads();   // s_l3 is written; the tile before has left LDS
        // the image side: rows of the tile, consecutive lanes on consecutive pixels
#pragma unroll 4
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t idx = i * 256 + threadIdx.x, col = idx & 63u, row = idx >> 6;
            if (ox + col < w && oy + row < h) s_tile[tile_at(col, row)] = px_le24(src, (uint64_t)(oy + row) * pitch + ox + col, n_img) & 0xffffffu;
        }
        __syncthreads();
        // the scan side: positions 16 t .. 16 t + 15 of the tile lie in block t / 4 of its 8 x 8 blocks of 64 positions
        const uint32_t eb = s_l3[st * 64 + (threadIdx.x >> 2)];
        const uint32_t bx = (eb & 7u) << 3, by = ((eb >> 3) & 7u) << 3;
        uint32_t px[16], keep = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t e = s_l3[(eb >> 6) * 64 + (threadIdx.x & 3) * 16 + j];
            const uint32_t x = bx | (e & 7u), y = by | ((e >> 3) & 7u);
            px[j] = s_tile[tile_at(x, y)];
            keep |= (uint32_t)(ox + x < w && oy + y < h) << j;
        }
        const uint32_t cnt = (uint32_t)__popc(keep);
        uint32_t at = block_exclusive_scan<256>(cnt, s_wsum);
        if (threadIdx.x == 255) s_total = at + cnt;
#pragma unroll
        for (int j = 0; j < 16; j++)
            if ((keep >> j) & 1u) s_out[at++] = px[j];
        __syncthreads();
        // 3 K contiguous bytes behind the base, by aligned words; the words that hang over either end by bytes
        const uint32_t nbytes = 3 * s_total;
        uint8_t *const out = dst + 3 * base;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 3u);
        const uint32_t nwords = (mis + nbytes + 3) >> 2;
        for (uint32_t j = threadIdx.x; j < nwords; j += 256) {
            const int32_t rel = (int32_t)(4 * j) - (int32_t)mis;   // first byte of the word, from `out`
            if (rel >= 0 && (uint32_t)rel + 4 <= nbytes) {
                const uint32_t p = (uint32_t)rel / 3, r = (uint32_t)rel % 3;
                const uint64_t two = (uint64_t)s_out[p] | ((uint64_t)(p + 1 < s_total ? s_out[p + 1] : 0u) << 24);
                *reinterpret_cast<uint32_t *>(out + rel) = (uint32_t)(two >> (8 * r));
            } else {
                for (int k = 0; k < 4; k++) {
                    const int32_t b = rel + k;
                    if (b >= 0 && (uint32_t)b < nbytes) out[b] = (uint8_t)(s_out[(uint32_t)b / 3] >> (8 * ((uint32_t)b % 3)));
                }
            }
        }
    }
}

// `small` below 64 x 64 or along an injected s x s scan: the scan per position (Scan, hilbert_scan.hpp), four consecutive positions
// per thread, their twelve bytes as three words where the output is 4-byte aligned
__global__ __launch_bounds__(256) void k_lin_small(const uint8_t *__restrict__ src, uint32_t pitch, uint64_t n_img, uint32_t s, uint32_t order,
                                                   const HilbertLut *__restrict__ lut, uint8_t *__restrict__ dst) {
    __shared__ uint16_t s_l4[1024];
    __shared__ uint8_t s_l1[16];
    const Scan sc = load_scan(s, s, order, lut, s_l4, s_l1);
    const uint64_t n = (uint64_t)s * s, nquad = (n + 3) >> 2;
    const bool words = (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += stride) {
        const uint64_t d = q << 2;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[j] = 0;
            if (d + j < n) {
                uint32_t x, y;
                sc.xy(d + j, x, y);
                v[j] = px_le24(src, (uint64_t)y * pitch + x, n_img) & 0xffffffu;
            }
        }
        if (words && d + 4 <= n) {
            uint32_t *o3 = reinterpret_cast<uint32_t *>(dst + 3 * d);
            o3[0] = v[0] | (v[1] << 24); o3[1] = (v[1] >> 8) | (v[2] << 16); o3[2] = (v[2] >> 16) | (v[3] << 8);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (d + j < n) store_px3(dst + 3 * (d + j), v[j]);
        }
    }
}

// ---------------------------------------------------------------- `large` along an injected scan of the S x S square
// a block owns 4096 consecutive positions, a thread 16 of them; kept = inside the image
constexpr uint32_t kInjPerBlock = 4096;
__device__ __forceinline__ uint32_t inj_keep(const uint2 *__restrict__ xy, uint64_t n2, uint64_t d0, uint32_t w, uint32_t h, uint2 (&pos)[16]) {
    uint32_t keep = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        pos[j] = make_uint2(0u, 0u);
        if (d0 + j < n2) {
            pos[j] = xy[d0 + j];
            keep |= (uint32_t)(pos[j].x < w && pos[j].y < h) << j;
        }
    }
    return keep;
}
__global__ __launch_bounds__(256) void k_lin_inj_count(const uint2 *__restrict__ xy, uint64_t n2, uint32_t w, uint32_t h, uint32_t *__restrict__ bcnt) {
    uint2 pos[16];
    const uint32_t keep = inj_keep(xy, n2, (uint64_t)blockIdx.x * kInjPerBlock + threadIdx.x * 16, w, h, pos);
    const uint32_t t = block_reduce_sum<256>((uint32_t)__popc(keep));
    if (threadIdx.x == 0) bcnt[blockIdx.x] = t;
}
// exclusive scan of the nb block counts in place (one block; the total is w h < 2^32)
__global__ __launch_bounds__(256) void k_lin_inj_scan(uint32_t *__restrict__ bcnt, uint32_t nb) {
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < nb; i0 += 256) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < nb ? bcnt[i] : 0u;
        const uint32_t carry = s_carry;
        const uint32_t ex = block_exclusive_scan<256>(v, s_wsum);   // (its barriers stand between the read of s_carry and its update)
        if (i < nb) bcnt[i] = carry + ex;
        if (threadIdx.x == 255) s_carry = carry + ex + v;
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_lin_inj_gather(const uint2 *__restrict__ xy, uint64_t n2, const uint8_t *__restrict__ src, uint32_t w, uint32_t h,
                                                        const uint32_t *__restrict__ boff, uint8_t *__restrict__ dst) {
    __shared__ uint32_t s_wsum[4];
    uint2 pos[16];
    const uint32_t keep = inj_keep(xy, n2, (uint64_t)blockIdx.x * kInjPerBlock + threadIdx.x * 16, w, h, pos);
    uint64_t at = (uint64_t)boff[blockIdx.x] + block_exclusive_scan<256>((uint32_t)__popc(keep), s_wsum);
    const uint64_t n = (uint64_t)w * h;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((keep >> j) & 1u) store_px3(dst + 3 * at++, px_le24(src, (uint64_t)pos[j].y * w + pos[j].x, n));
}

// ---------------------------------------------------------------- the difference histogram
// counts[c][v + 255] = #{ i in 1 .. n-1 : lin[i][c] - lin[i-1][c] == v } (hilbert_distribution.py: pandas.diff drops the first element; no
// START zero, unlike DiffStream).  The stream is cut into a head of < 16 pixels up to the first 16-byte boundary, chunks of 16 pixels
// = three 16-byte loads, a chunk per thread, and a tail of < 16 pixels.  A chunk's first pixel takes its predecessor from the lane
// before (consecutive lanes hold consecutive chunks), lane 0 from memory.  Bins: u32[3][511] in LDS per block (a block meets fewer than
// 2^32 pixels), added to the 64-bit counts once per block.  A flat image would send every lane to bin 255 of each channel: the zero
// difference is counted in a register per lane and channel and summed over the wave at the end; the other bins go through
// atomic_count, which lets the lanes that hold the same bin add together (a two-colour pattern has two such bins per channel).
constexpr uint32_t kDiffBins = 3 * 511;
__device__ __forceinline__ void diff_count(uint32_t *bins, uint32_t (&zero)[3], uint32_t cur, uint32_t prev) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const int32_t v = (int32_t)((cur >> (8 * ch)) & 255u) - (int32_t)((prev >> (8 * ch)) & 255u);
        if (v == 0) zero[ch]++;
        else atomic_count(bins, (uint32_t)(ch * 511 + 255 + v));
    }
}
__device__ __forceinline__ uint32_t px_bytes(const uint8_t *__restrict__ lin, uint64_t i) {
    const uint8_t *p = lin + 3 * i;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
__global__ __launch_bounds__(256) void k_chan_diff_hist(const uint8_t *__restrict__ lin, uint64_t n, uint32_t head, uint64_t nchunks,
                                                        unsigned long long *__restrict__ counts) {
    __shared__ uint32_t s_bins[kDiffBins];
    for (uint32_t i = threadIdx.x; i < kDiffBins; i += 256) s_bins[i] = 0;
    __syncthreads();
    uint32_t zero[3] = {0, 0, 0};
    const uint8_t *const body = lin + 3 * (uint64_t)head;   // 16-byte aligned
    const uint64_t per_round = (uint64_t)gridDim.x * 256;
    const uint64_t rounds = (nchunks + per_round - 1) / per_round;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t r = 0; r < rounds; r++) {   // (the same trip count in every lane: the lane shift below wants the whole wave)
        const uint64_t chunk = r * per_round + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        const bool valid = chunk < nchunks;
        uint32_t px[16];
#pragma unroll
        for (int i = 0; i < 16; i++) px[i] = 0;
        if (valid) {
            const uint4 *p = reinterpret_cast<const uint4 *>(body + 48 * chunk);
            const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
            const uint32_t q[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint32_t a = q[3 * g], b = q[3 * g + 1], c3 = q[3 * g + 2];
                px[4 * g] = a & 0xffffffu; px[4 * g + 1] = ((a >> 24) | (b << 8)) & 0xffffffu; px[4 * g + 2] = ((b >> 16) | (c3 << 16)) & 0xffffffu; px[4 * g + 3] = c3 >> 8;
            }
        }
        uint32_t prev = wave_prev_lane(px[15], 0u);
        const uint64_t first = head + 16 * chunk;   // the chunk's first pixel
        bool has_prev = true;
        if (lane == 0) {
            has_prev = valid && first > 0;
            if (has_prev) prev = px_bytes(lin, first - 1);
        }
        if (valid) {
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (i > 0 || has_prev) diff_count(s_bins, zero, px[i], i > 0 ? px[i - 1] : prev);
        }
    }
    if (blockIdx.x == 0) {   // head and tail, a pixel per lane: pixels 1 .. head-1 and head + 16 nchunks .. n-1 (its first with the body's last)
        const uint64_t tail0 = head + 16 * nchunks;
        uint64_t i = 0;
        if (threadIdx.x < 16) i = threadIdx.x < head ? threadIdx.x : 0;
        else if (threadIdx.x >= 32 && threadIdx.x < 48) i = tail0 + (threadIdx.x - 32) < n ? tail0 + (threadIdx.x - 32) : 0;
        if (i > 0) diff_count(s_bins, zero, px_bytes(lin, i), px_bytes(lin, i - 1));
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t z = wave_reduce_sum(zero[ch]);
        if (lane == 0 && z) atomicAdd(&s_bins[ch * 511 + 255], z);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kDiffBins; i += 256)
        if (s_bins[i]) atomicAdd(&counts[i], (unsigned long long)s_bins[i]);
}

}  // namespace

// ---------------------------------------------------------------- host
int linearize_count(int32_t method, uint32_t w, uint32_t h, uint64_t *npx) {
    if (!npx || !dims_ok(w, h)) return CNIIC_ERR_BAD_ARG;
    if (method == CNIIC_LIN_RECT || method == CNIIC_LIN_LARGE) *npx = (uint64_t)w * h;
    else if (method == CNIIC_LIN_SMALL) {
        const uint64_t s = std::min(npot(w) >> 1, npot(h) >> 1);   // hilbert.rs:18
        *npx = s * s;
    } else return CNIIC_ERR_BAD_ARG;
    return CNIIC_OK;
}

static uint32_t tile_grid(uint32_t w, uint32_t h) {
    return (uint32_t)std::min<uint64_t>((uint64_t)((w + 63) >> 6) * ((h + 63) >> 6), 256 * 8);
}

int linearize_as(Ctx *c, int32_t method, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out_d) {
    uint64_t need = 0;
    if (linearize_count(method, w, h, &need) != CNIIC_OK) return c->fail(CNIIC_ERR_BAD_ARG, "linearize: method %d or image %ux%u refused", method, w, h);
    if (!need) return CNIIC_OK;
    if (method == CNIIC_LIN_RECT) return hilbert_linearize(c, rgb_d, w, h, out_d);
    const uint64_t n_img = (uint64_t)w * h;
    const HilbertLut *lut = nullptr;
    CNIIC_TRY(hilbert_lut(c, &lut));
    if (method == CNIIC_LIN_SMALL) {
        const uint32_t s = std::min(npot(w) >> 1, npot(h) >> 1);
        ScanSel sel;
        CNIIC_TRY(scan_select(c, s, s, &sel));   // the built-in 2^n scan (order >= 1; s == 1: none needed), or one injected for s x s
        ScopedKernelTimer timer(c, "lin_small");
        if (sel.order >= 6)
            hipLaunchKernelGGL(k_lin_tiles, dim3(tile_grid(s, s)), dim3(256), 0, c->stream, rgb_d, w, n_img, s, s, sel.order, lut, out_d);
        else
            hipLaunchKernelGGL(k_lin_small, dim3((uint32_t)std::min<uint64_t>(ceil_div(need, 1024), 256 * 16)), dim3(256), 0, c->stream, rgb_d, w, n_img, s, sel.korder,
                               sel.arg, out_d);
        CNIIC_HIP_TRY(c, hipGetLastError());
        timer.stop(1);
        return CNIIC_OK;
    }
    const uint32_t S = std::max(npot(w), npot(h)), L = log2_exact(S);   // hilbert.rs:27
    ScopedKernelTimer timer(c, "lin_large");
    if (c->scan_xy.p && c->scan_w == S && c->scan_h == S) {
        const uint64_t n2 = (uint64_t)S * S;   // (< 2^32: scan_inject checked the dimensions)
        const uint32_t nb = (uint32_t)ceil_div(n2, kInjPerBlock);
        const uint2 *xy = c->scan_xy.as<uint2>();
        DevBuf bcnt;
        CNIIC_HIP_TRY(c, bcnt.alloc((uint64_t)nb * 4));
        hipLaunchKernelGGL(k_lin_inj_count, dim3(nb), dim3(256), 0, c->stream, xy, n2, w, h, bcnt.as<uint32_t>());
        hipLaunchKernelGGL(k_lin_inj_scan, dim3(1), dim3(256), 0, c->stream, bcnt.as<uint32_t>(), nb);
        hipLaunchKernelGGL(k_lin_inj_gather, dim3(nb), dim3(256), 0, c->stream, xy, n2, rgb_d, w, h, (const uint32_t *)bcnt.as<uint32_t>(), out_d);
        CNIIC_HIP_TRY(c, hipGetLastError());
        timer.stop(3);
        return CNIIC_OK;
    }
    if (L >= 6) hipLaunchKernelGGL(k_lin_tiles, dim3(tile_grid(w, h)), dim3(256), 0, c->stream, rgb_d, w, n_img, w, h, L, lut, out_d);
    else hipLaunchKernelGGL(k_lin_large_px, dim3(1), dim3(256), 0, c->stream, rgb_d, w, h, L, lut, out_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    timer.stop(1);
    return CNIIC_OK;
}

int channel_diff_hist(Ctx *c, const uint8_t *lin_d, uint64_t npx, uint64_t *counts_d) {
    if (npx >= (1ull << 40)) return c->fail(CNIIC_ERR_BAD_ARG, "channel_diff_hist: too many pixels");   // (a block's u32 bins: 2^40 / grid < 2^32)
    CNIIC_HIP_TRY(c, hipMemsetAsync(counts_d, 0, kDiffBins * 8, c->stream));
    if (npx <= 1) return CNIIC_OK;
    // pixels up to the first 16-byte boundary: (addr + 3 k) % 16 == 0 <=> k = 11 (16 - addr % 16) % 16  (3 x 11 = 33 = 1 mod 16)
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(lin_d) & 15);
    const uint32_t head = (uint32_t)std::min<uint64_t>((11u * (16u - mis)) & 15u, npx);
    const uint64_t nchunks = (npx - head) / 16;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ceil_div(nchunks, 256), 1), 256 * 4);
    ScopedKernelTimer timer(c, "chan_diff_hist");
    hipLaunchKernelGGL(k_chan_diff_hist, dim3(grid), dim3(256), 0, c->stream, lin_d, npx, head, nchunks, reinterpret_cast<unsigned long long *>(counts_d));
    CNIIC_HIP_TRY(c, hipGetLastError());
    timer.stop(1);
    return CNIIC_OK;
}

}  // namespace cniic
