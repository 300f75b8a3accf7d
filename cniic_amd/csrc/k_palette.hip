// k_palette.hip -- the colour -> label table of a FROZEN palette (cniic_palette_create): for every one of the 2^24 colours the index k
// that minimises (r-R_k)^2 + (g-G_k)^2 + (b-B_k)^2 in integers, the lowest k among equal minima (Rgb<u8>::dist of geom.rs:8-24 compared
// as squared integers, first minimum).  No K-means state is behind it: the table is a function of the K entries alone.
//
// One workgroup builds the entries of one cell of the colour cube (pal_bounds.hpp: 16^3 colours, 4096 cells), in three steps:
//   bounds      lanes stride over the K entries: dmax of each against the cell's box, block minimum B
//   candidates  the entries with dmin <= B, compacted into LDS in ASCENDING index order (ballot + prefix counts per wave, the waves'
//               totals through LDS): nobody else can be nearest to a colour of the box, not even in a tie
//   fill        a lane owns 16 colours that differ in b only (one 16-byte run of the table for byte labels) and walks the list with a
//               strict <: ascending order and strict < give the lowest index.  Every lane reads the SAME LDS word at each step -- a
//               broadcast read, no bank conflicts -- and (r-R)^2 + (g-G)^2 is computed once for the 16 colours.
// A wave's 64 lanes cover 4 values of r and the 16 of g: its store instruction writes 64 runs of 16 bytes (32 for two-byte labels), 256
// bytes apart.  Runs longer than the cell's side along b do not exist in key order; a cell flatter in r and g and longer in b would write
// longer runs and pay with a wider box, i.e. more candidates (NOTES.md section O).
// A list longer than list_max (kPalListMax entries of LDS; K in the thousands, many equal entries) sends the cell down the plain route: the
// same lanes scan all K entries from memory for their colours.  Correct, and nothing claims it is fast.
// Below it: k_palette_fit, the summed squared error and the pixels per entry of a batch of frames under that table.
#include "common.hpp"
#include "device_utils.hpp"
#include "pal_bounds.hpp"

namespace cniic {

constexpr int kPalThreads = 256;
constexpr int kPalPer = 16;   // colours per lane: one run along b
static_assert(kPalThreads * kPalPer == kPalCellSide * kPalCellSide * kPalCellSide, "one block fills one cell");
static_assert(kPalCellSide == kPalPer && kPalThreads == kPalCellSide * kPalCellSide, "lane = (r, g) of the cell, its colours the cell's side along b");

// one entry against the lane's 16 colours (r, g fixed, b = b0 .. b0 + 15)
__device__ __forceinline__ void pal_step(uint32_t rgb, uint32_t idx, int32_t r, int32_t g, int32_t b0, uint32_t best[kPalPer], uint32_t bidx[kPalPer]) {
    const int32_t dr = r - (int32_t)((rgb >> 16) & 255u), dg = g - (int32_t)((rgb >> 8) & 255u), db0 = b0 - (int32_t)(rgb & 255u);
    const uint32_t base = (uint32_t)(dr * dr + dg * dg);
#pragma unroll
    for (int i = 0; i < kPalPer; i++) {
        const int32_t db = db0 + i;
        const uint32_t d = base + (uint32_t)(db * db);
        const bool nearer = d < best[i];
        best[i] = nearer ? d : best[i];
        bidx[i] = nearer ? idx : bidx[i];
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kPalThreads) void k_palette_lut(const uint32_t *__restrict__ cent /* [K] 0xRRGGBB */, uint32_t K, uint32_t list_max,
                                                             void *__restrict__ table /* u8 or u16 [2^24] */, uint32_t *__restrict__ plain_cells /* or null */) {
    constexpr uint32_t kCap = WIDE ? kPalListMax : 256u;   // (byte labels: K <= 256 entries at most)
    __shared__ uint32_t s_word[kCap];                       // byte labels: index << 24 | rgb; two-byte labels: rgb, the index beside it
    __shared__ uint32_t s_idx[WIDE ? kCap : 1];
    __shared__ uint32_t s_w[kPalThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    const uint32_t corner = pal_cell_corner(blockIdx.x);
    if (list_max > kCap) list_max = kCap;

    // ---- bounds
    uint32_t m = 0xffffffffu;
    for (uint32_t k = t; k < K; k += kPalThreads) m = min(m, pal_box_dmax(cent[k], corner));
    m = wave_reduce_min(m);
    if (lane == 0) s_w[wid] = m;
    __syncthreads();
    uint32_t bound = s_w[0];
#pragma unroll
    for (int i = 1; i < kPalThreads / 64; i++) bound = min(bound, s_w[i]);
    __syncthreads();

    // ---- candidates, ascending
    uint32_t count = 0;
    for (uint32_t k0 = 0; k0 < K && count <= list_max; k0 += kPalThreads) {
        const uint32_t k = k0 + t;
        const uint32_t e = k < K ? cent[k] : 0u;
        const bool in = k < K && pal_is_candidate(pal_box_dmin(e, corner), bound);
        const unsigned long long bal = __ballot(in);
        if (lane == 0) s_w[wid] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t pos = count + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
        for (uint32_t i = 0; i < kPalThreads / 64; i++) {
            const uint32_t n = s_w[i];
            if (i < wid) pos += n;
            all += n;
        }
        if (in && pos < list_max) {
            if (WIDE) { s_word[pos] = e & 0xffffffu; s_idx[pos] = k; }
            else s_word[pos] = (k << 24) | (e & 0xffffffu);
        }
        count += all;
        __syncthreads();
    }

    // ---- fill
    const int32_t r = (int32_t)((corner >> 16) & 255u) + (int32_t)(t >> kPalCellBits), g = (int32_t)((corner >> 8) & 255u) + (int32_t)(t & (kPalCellSide - 1)),
                  b0 = (int32_t)(corner & 255u);
    uint32_t best[kPalPer], bidx[kPalPer];
#pragma unroll
    for (int i = 0; i < kPalPer; i++) { best[i] = 0xffffffffu; bidx[i] = 0; }
    if (count <= list_max) {
        for (uint32_t j = 0; j < count; j++) {
            const uint32_t wd = s_word[j];
            pal_step(wd & 0xffffffu, WIDE ? s_idx[j] : wd >> 24, r, g, b0, best, bidx);
        }
    } else {   // the plain route: every entry, from memory (the address is the same in every lane)
        if (plain_cells && t == 0) atomicAdd(plain_cells, 1u);
        for (uint32_t k = 0; k < K; k++) pal_step(cent[k], k, r, g, b0, best, bidx);
    }
    const uint32_t key0 = ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b0;   // < 2^24, a multiple of 16; key0 + 15 is in the table too
    if (WIDE) {
        uint32_t w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = bidx[2 * j] | (bidx[2 * j + 1] << 16);
        uint4 *dst = reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(table) + key0);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) w[j] = bidx[4 * j] | (bidx[4 * j + 1] << 8) | (bidx[4 * j + 2] << 16) | (bidx[4 * j + 3] << 24);
        *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(table) + key0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// table_d: 2^24 labels of 1 (K <= 256) or 2 bytes, 16-byte aligned; plain_cells_d (optional): a zeroed counter of the cells that took the plain route
int palette_lut(Ctx *c, const uint32_t *cent_d, uint32_t K, bool wide, void *table_d, uint32_t list_max, uint32_t *plain_cells_d) {
    if (!K || K > 65536u || (!wide && K > 256u) || (reinterpret_cast<uintptr_t>(table_d) & 15)) return c->fail(CNIIC_ERR_BAD_ARG, "palette_lut: K = %u", K);
    if (wide)
        hipLaunchKernelGGL(k_palette_lut<true>, dim3(kPalCells), dim3(kPalThreads), 0, c->stream, cent_d, K, list_max, table_d, plain_cells_d);
    else
        hipLaunchKernelGGL(k_palette_lut<false>, dim3(kPalCells), dim3(kPalThreads), 0, c->stream, cent_d, K, list_max, table_d, plain_cells_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

// ---------------------------------------------------------------- how well the palette fits a batch of frames (cniic_palette_fit_frames_var)
// sse[f] = the sum over frame f's pixels of the squared distance to the pixel's entry under the rule, pixels[k] = the pixels of all frames whose
// entry is k.  One launch whatever the number of frames: a 1-D grid over the 4096-pixel chunks of all frames (FrameVar, common.hpp); a block finds
// its frame by the search in chunk0 and never spans two.  Frames of odd sizes start at any byte, so a chunk is cut into a head of < 16 pixels up
// to the first 16-byte boundary, groups of 16 pixels = three 16-byte loads, a group per thread, and a tail of < 16 pixels (a pixel per lane).
// A pixel's label is ONE read of the handle's 2^24 table, its entry's colour comes from LDS (K <= 256) or from memory.  |p - e|^2 as
// p.p + e.e - 2 p.e, three byte dot products; a lane meets at most 17 pixels of at most 195 075 each, a wave's sum stays below 2^28.
// The counts: K <= 256 in u32 bins of the block's LDS, larger K straight onto the u64 counts -- both through a count that lets the lanes
// of a wave that hold the same entry add together, so a flat frame costs a wave one add per round and not 64 on one address.
constexpr int kFitThreads = 256;
static_assert(kFitThreads * 16 == (int)kFrameVarChunk, "a thread's group is 16 pixels, a block's chunk the frame table's");

// counts[key] += 1 for every calling lane; device_utils.hpp's atomic_count for u64 counts in memory
__device__ __forceinline__ void fit_count64(unsigned long long *counts, uint32_t key) {
    bool todo = true;
#pragma unroll 1
    for (int r = 0; r < 8; r++) {
        const unsigned long long act = __ballot(todo);
        if (!act) return;
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(act));
        const bool same = todo && key == k;
        const unsigned long long sm = __ballot(same);
        if (same) {
            if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == (uint32_t)__builtin_ctzll(sm)) atomicAdd(&counts[k], (unsigned long long)__popcll(sm));
            todo = false;
        }
    }
    if (todo) atomicAdd(&counts[key], 1ull);
}

template <typename LabelT>
__global__ __launch_bounds__(kFitThreads) void k_palette_fit(const uint8_t *__restrict__ rgb, const FrameVar *__restrict__ fr, uint32_t frames,
                                                             const LabelT *__restrict__ table, const uint32_t *__restrict__ cent /* [K] 0xRRGGBB */, uint32_t K,
                                                             unsigned long long *__restrict__ sse /* [frames] */, unsigned long long *__restrict__ pixels /* [K] or null */) {
    constexpr bool WIDE = sizeof(LabelT) == 2;
    __shared__ uint32_t s_cent[WIDE ? 1 : 256];
    __shared__ uint32_t s_bins[WIDE ? 1 : 256];
    __shared__ uint32_t s_w[kFitThreads / 64];
    const uint32_t t = threadIdx.x;
    if (!WIDE) {
        s_cent[t] = t < K ? cent[t] : 0u;
        s_bins[t] = 0u;
        __syncthreads();
    }
    const uint32_t f = frame_of_block<&FrameVar::chunk0>(fr, frames, blockIdx.x);
    const uint64_t in_frame = (uint64_t)(blockIdx.x - fr[f].chunk0) * kFrameVarChunk;   // the chunk's first pixel, counted in its frame
    const uint32_t cnt = (uint32_t)min((uint64_t)kFrameVarChunk, fr[f].npx - in_frame);  // 1 .. 4096
    const uint8_t *const base = rgb + 3 * (fr[f].src_base + in_frame);
    // pixels before the first 16-byte boundary: 3 hd = -address (mod 16), and 11 is 3's inverse
    const uint32_t hd = min(cnt, (((16u - (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u) * 11u) & 15u);
    const uint32_t groups = (cnt - hd) / 16u, tail0 = hd + 16u * groups;   // groups <= 256: every thread at most one
    uint32_t sum = 0;
    auto one = [&](uint32_t key) {
        const uint32_t lab = table[key];
        const uint32_t e = WIDE ? cent[lab] : s_cent[lab];
        sum += __builtin_amdgcn_udot4(key, key, __builtin_amdgcn_udot4(e, e, 0u, false), false) - 2u * __builtin_amdgcn_udot4(key, e, 0u, false);
        if (pixels) {
            if (WIDE) fit_count64(pixels, lab);
            else atomic_count(s_bins, lab);
        }
    };
    if (t < groups) {
        uint32_t key[16];
        load16px_keys(reinterpret_cast<const uint4 *>(base + 3 * hd) + 3 * t, key);
#pragma unroll
        for (int i = 0; i < 16; i++) one(key[i]);
    }
    // head and tail, a pixel per lane of the first wave: lanes 0 .. 15 the head, lanes 16 .. 31 the tail
    if (t < 16 ? t < hd : (t < 32 && tail0 + (t - 16) < cnt)) one(rgb_key(base + 3 * (t < 16 ? t : tail0 + (t - 16))));
    sum = wave_reduce_sum(sum);
    if ((t & 63) == 0) s_w[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long all = 0;
#pragma unroll
        for (int i = 0; i < kFitThreads / 64; i++) all += s_w[i];
        if (all) atomicAdd(&sse[f], all);
    }
    if (!WIDE && pixels && t < K && s_bins[t]) atomicAdd(&pixels[t], (unsigned long long)s_bins[t]);
}

// fr_d: the batch's frame table (F rows, `chunks` chunks in all); sse_d: u64[F], pixels_d: u64[K] or null, both zeroed by the caller
int palette_fit(Ctx *c, const uint8_t *rgb_d, const FrameVar *fr_d, uint32_t frames, uint32_t chunks, const void *table_d, bool wide, const uint32_t *cent_d, uint32_t K,
                uint64_t *sse_d, uint64_t *pixels_d) {
    if (!frames || !chunks || !K || (!wide && K > 256u)) return c->fail(CNIIC_ERR_BAD_ARG, "palette_fit: %u frames, K = %u", frames, K);
    auto *sse = reinterpret_cast<unsigned long long *>(sse_d), *px = reinterpret_cast<unsigned long long *>(pixels_d);
    if (wide)
        hipLaunchKernelGGL(k_palette_fit<uint16_t>, dim3(chunks), dim3(kFitThreads), 0, c->stream, rgb_d, fr_d, frames, static_cast<const uint16_t *>(table_d), cent_d, K, sse, px);
    else
        hipLaunchKernelGGL(k_palette_fit<uint8_t>, dim3(chunks), dim3(kFitThreads), 0, c->stream, rgb_d, fr_d, frames, static_cast<const uint8_t *>(table_d), cent_d, K, sse, px);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
