// k_small_trie.hip -- the parse of SMALL frames' serialised decoders (at most kSmallTrieMaxLeaves leaves), one workgroup per frame, any
// number of frames in one launch (cniic_codec_decode_batch / cniic_codec_measure_batch of streams in device memory; codec.cpp
// small_parse_dev).  One body, two kernels: k_small_trieparse for the SignedColor leaves of `delta` streams (S = 6 symbol bytes) and
// k_small_trieparse_rgb for the Rgb<u8> leaves of `hufman` and `cluster-colors` streams (S = 11).  It is the small-decoder counterpart of
// k_trieparse.hip (one decoder of 10^5 .. 10^7 leaves, six kernels): the block reads the frame's header and its pre-order trie where the
// stream lies and leaves the table k_delta_small_dec / k_huf_small_dec read -- the leaves' left-aligned codes, ascending, then their
// key | length << 27 words -- in the frame's slice of HBM scratch, so that no byte of the stream travels to the host.  small_trie.hpp has the
// arithmetic and its names (window, chunk, lane, map, P, run); the phases:
//   0. header: w, h from the stream at any byte alignment (aligned words, funnel-shifted); a frame that is not the route's is skipped
//   1. masks and maps: every lane reads its K chunks of 32 bytes once (K <= 4; <= 7 for S = 11), keeps their tags as two masks per chunk in
//      registers, and walks them from each of the S + 1 entry offsets; a block-wide scan over map composition (32-bit words; 64-bit for
//      S = 11) gives every lane its true entry
//   2. counts: the true walk's nodes and leaves per lane, a block-wide prefix sum -> every lane's first node, first leaf and P
//   3. open subtrees: P of every node; the first leaf with P = 0 ends the trie (node E); the last node of every P per lane into the table
//      of last nodes, then a prefix maximum per row over the lanes: the last earlier node with a given P, for every lane
//   4. runs: the head of every run looks its parent up (the last earlier node with its P) and writes the run's word: the parent's run and
//      the distance; then 5 rounds of pointer jumping over the runs, in place (every word is a fact, whichever round wrote it)
//   5. lengths: a leaf's depth = its run's sum + its node index; a block-wide prefix sum over 2^(32 - len) -> every lane's first code
//   6. table: code and key | length of every leaf to HBM; the symbols' S bytes are read here at any alignment from the aligned words that
//      hold them, and one that get_symbol refuses (outside -255 .. 255; a length word other than 3) fails the frame
// Dynamic LDS (pitch = the lanes a stream of the launch occupies at the most (st_launch), leaves = the leaves its longest stream has room
// for; at the bound 80 + 64 KiB, for either S):
//   table of last nodes   3-4   (kStMaxP + 1) rows x pitch words
//   runs                  4-6   `leaves` words
// The trie's bytes stay in HBM / L2: a lane reads its chunks once (phase 1) and its leaves' symbols once (phase 6); per-node P, parents and
// depths are never stored -- a lane walks its masks again in every phase, which costs a few dozen register steps.  No block waits for
// another, and no loop is without a bound: a walk advances by a record of at least one byte per step and ends with the lane's chunks.
#include "common.hpp"
#include "small_trie.hpp"

namespace cniic {

constexpr uint32_t kStWaves = kStLanes / 64;
// (the same for both kinds: pitch <= 1024 lanes and runs <= 16 384 words whatever S is; the static words are the two scans', the maps' at
// 8 bytes each for S = 11, the lanes' last-leaf bytes and the flags)
static_assert(4 * ((kStMaxP + 1) * kStLanes + kSmallTrieMaxLeaves) + 4 * (2 * (kStWaves + 1)) + 8 * (kStWaves + 1) + kStLanes + 64 <= 160 * 1024, "the largest decoder's table of last nodes and runs fit one CU's LDS");

// four bytes at any alignment as a little-endian word: the aligned words that hold one of them
__device__ __forceinline__ uint32_t st_ld_u32(const uint8_t *p) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t *g = reinterpret_cast<const uint32_t *>(p - a);
    uint32_t v = g[0] >> (8 * a);
    if (a) v |= g[1] << (32 - 8 * a);
    return v;
}
// six bytes at any alignment as a little-endian number
__device__ __forceinline__ uint64_t st_ld_six(const uint8_t *p) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t *g = reinterpret_cast<const uint32_t *>(p - a);
    uint64_t v = ((uint64_t)g[0] | ((uint64_t)g[1] << 32)) >> (8 * a);
    if (a > 2) v |= (uint64_t)g[2] << (64 - 8 * a);
    return v & 0xffffffffffffull;
}
// the eleven bytes of an Rgb leaf's symbol at any alignment: the length word and the three colour bytes (three aligned words, a fourth only
// when the record reaches into it)
__device__ __forceinline__ StRgbLeaf st_ld_rgb_leaf(const uint8_t *p) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t *g = reinterpret_cast<const uint32_t *>(p - a);
    const uint32_t g0 = g[0], g1 = g[1], g2 = g[2], g3 = a > 1 ? g[3] : 0u;
    StRgbLeaf l;
    l.len = ((uint64_t)g0 | ((uint64_t)g1 << 32)) >> (8 * a);
    if (a) l.len |= (uint64_t)g2 << (64 - 8 * a);
    l.rgb = (uint32_t)((((uint64_t)g2 | ((uint64_t)g3 << 32)) >> (8 * a)) & 0xffffffull);
    return l;
}
template <uint32_t S> struct StSymbolLoad;
template <> struct StSymbolLoad<6> { static __device__ __forceinline__ uint64_t ld(const uint8_t *p) { return st_ld_six(p); } };
template <> struct StSymbolLoad<11> { static __device__ __forceinline__ StRgbLeaf ld(const uint8_t *p) { return st_ld_rgb_leaf(p); } };
__device__ __forceinline__ uint32_t st_shfl_up(uint32_t v, int d) { return __shfl_up(v, d); }
__device__ __forceinline__ uint64_t st_shfl_up(uint64_t v, int d) {
    return (uint64_t)__shfl_up((uint32_t)v, d) | ((uint64_t)__shfl_up((uint32_t)(v >> 32), d) << 32);
}
// the 32 bytes of a chunk at q as 8 little-endian words; no aligned word at or behind `end` is read (zeros stand for it)
__device__ __forceinline__ void st_ld_chunk(const uint8_t *q, const uint8_t *end, uint32_t w[8]) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(q) & 3);
    const uint32_t *g = reinterpret_cast<const uint32_t *>(q - a);
    uint32_t x[9];
#pragma unroll
    for (uint32_t i = 0; i < 9; i++) x[i] = reinterpret_cast<const uint8_t *>(g + i) < end && (i < 8 || a) ? g[i] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) w[i] = a ? (x[i] >> (8 * a)) | (x[i + 1] << (32 - 8 * a)) : x[i];
}

// exclusive prefix sums of two values over the block's 1024 lanes
__device__ __forceinline__ void st_block_scan2(uint32_t &a, uint32_t &b, uint32_t s_w[2][kStWaves + 1]) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ta = __shfl_up(ia, d), tb = __shfl_up(ib, d);
        if (lane >= (uint32_t)d) { ia += ta; ib += tb; }
    }
    __syncthreads();   // (whoever still reads the words of an earlier scan has done so)
    if (lane == 63) { s_w[0][wv] = ia; s_w[1][wv] = ib; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t run = 0;
        for (uint32_t w = 0; w < kStWaves; w++) { const uint32_t t = s_w[threadIdx.x][w]; s_w[threadIdx.x][w] = run; run += t; }
        s_w[threadIdx.x][kStWaves] = run;
    }
    __syncthreads();
    a = s_w[0][wv] + ia - a;
    b = s_w[1][wv] + ib - b;
}

template <uint32_t S> __device__ __forceinline__ void st_parse_frame(const SmallTrieRow *__restrict__ rows, uint32_t pitch, uint32_t room, uint32_t max_px, uint64_t img_stride,
                                                                      uint32_t scan_w, uint32_t scan_h, SmallTrieResult *__restrict__ res) {
    typedef typename StMap<S>::word Map;
    extern __shared__ __align__(16) uint32_t st_lds[];
    __shared__ uint32_t s_scan[2][kStWaves + 1];
    __shared__ Map s_map[kStWaves + 1];
    __shared__ uint8_t s_last[kStLanes];
    __shared__ uint32_t s_end, s_deep, s_flags, s_pay, s_longest;
    constexpr uint32_t kBadTag = 1, kGiveUp = 2, kBadSymbol = 4;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.x;
    uint32_t *s_tab = st_lds;                              // [(kStMaxP + 1) * pitch]
    uint32_t *s_runs = st_lds + (kStMaxP + 1) * pitch;     // [room]
    const SmallTrieRow row = rows[f];
    SmallTrieResult r = {0, 0, kStSkipped, 0, 0, 0};

    // ---- 0. the header
    if (row.bytes < 8) { if (tid == 0) res[f] = r; return; }
    r.w = st_ld_u32(row.stream);
    r.h = st_ld_u32(row.stream + 4);
    const uint64_t n = (uint64_t)r.w * r.h;
    if (!n || n > max_px || 3 * n > img_stride || (scan_w && r.w == scan_w && r.h == scan_h)) { if (tid == 0) res[f] = r; return; }
    const uint8_t *__restrict__ trie = row.stream + 8;
    const uint64_t trie_bytes = row.bytes - 8;
    const uint32_t window = st_window(trie_bytes, st_max_bytes<S>());
    if (!window) { r.verdict = kStNotDecoder; if (tid == 0) res[f] = r; return; }
    if (st_lanes_used(window) > pitch || st_leaves_room<S>(row.bytes) > room) { r.verdict = kStNotOurs; if (tid == 0) res[f] = r; return; }   // (not in a launch sized by its longest stream)

    // ---- 1. masks, maps, entries
    StLaneK<st_max_k<S>()> ln;
    ln.K = st_lane_chunks(window);
    ln.at = tid * ln.K * kStChunk;
    ln.entry = 0; ln.nodes_before = 0; ln.leaves_before = 0;
#pragma unroll
    for (uint32_t k = 0; k < st_max_k<S>(); k++) {
        ln.br[k] = 0; ln.lf[k] = 0;
        const uint32_t at = ln.at + k * kStChunk;
        if (k < ln.K && at < window) {
            uint32_t w[8];
            st_ld_chunk(trie + at, trie + window, w);
            st_masks<S>(w, at, window, ln.br[k], ln.lf[k]);
        }
    }
    if (tid == 0) { s_end = kStNone; s_deep = kStNone; s_flags = 0; s_pay = 0; s_longest = 0; }
    {
        Map inc = st_lane_map<S>(ln);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Map t = st_shfl_up(inc, d);
            if (lane >= (uint32_t)d) inc = st_map_compose<S>(t, inc);
        }
        if (lane == 63) s_map[wv] = inc;
        __syncthreads();
        if (tid == 0) {
            Map run = st_map_identity<S>();
            for (uint32_t w = 0; w < kStWaves; w++) { const Map t = s_map[w]; s_map[w] = run; run = st_map_compose<S>(run, t); }
        }
        __syncthreads();
        const uint32_t into_wave = st_map_get<S>(s_map[wv], 0);
        const Map prev = st_shfl_up(inc, 1);
        ln.entry = lane ? st_map_get<S>(prev, into_wave) : into_wave;
    }

    // ---- 2. nodes and leaves in front of every lane
    {
        uint32_t nodes, leaves, last;
        const uint32_t stop = st_lane_count<S>(ln, nodes, leaves, last);
        s_last[tid] = (uint8_t)last;
        if (stop != kStNoStop && stop < window && trie[stop] != 0) atomicOr(&s_flags, kBadTag);   // (a 0 there: a leaf that the window cuts)
        if (nodes && tid >= pitch) atomicOr(&s_flags, kGiveUp);                                    // (not with pitch >= the frame's lanes)
        st_block_scan2(nodes, leaves, s_scan);
        ln.nodes_before = nodes; ln.leaves_before = leaves;
    }

    // ---- 3. P, the trie's end, the last node of every P
    if (tid < pitch) {
        for (uint32_t p = 0; p <= kStMaxP; p++) s_tab[p * pitch + tid] = 0u;
        uint32_t e, d;
        st_lane_open<S>(ln, s_tab, pitch, tid, &e, &d);
        if (e != kStNone) atomicMin(&s_end, e);
        if (d != kStNone) atomicMin(&s_deep, d);
    }
    __syncthreads();
    const uint32_t E = s_end;
    if (E == kStNone) {
        r.verdict = st_verdict_open((s_flags & kBadTag) != 0, window, trie_bytes);
        if (tid == 0) res[f] = r;
        return;
    }
    const uint32_t L = E / 2 + 1;   // E + 1 nodes of a full trie: L leaves, L - 1 branches
    if (s_deep <= E || L > room || (s_flags & kGiveUp)) { r.verdict = kStNotOurs; if (tid == 0) res[f] = r; return; }
    for (uint32_t p = wv; p <= kStMaxP; p += kStWaves) {   // a row per wave: the exclusive prefix maximum over the lanes
        uint32_t carry = 0;
        for (uint32_t m0 = 0; m0 < pitch; m0 += 64) {
            const uint32_t i = m0 + lane;
            uint32_t inc = i < pitch ? s_tab[p * pitch + i] : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(inc, d);
                if (lane >= (uint32_t)d) inc = inc > t ? inc : t;
            }
            uint32_t ex = __shfl_up(inc, 1);
            if (!lane) ex = 0u;
            if (i < pitch) s_tab[p * pitch + i] = carry > ex ? carry : ex;
            const uint32_t top = __shfl(inc, 63);
            carry = carry > top ? carry : top;
        }
    }
    __syncthreads();

    // ---- 4. runs and their chains
    if (tid < pitch) {
        uint32_t pay = 0;
        if (!st_lane_runs<S>(ln, tid ? s_last[tid - 1] != 0 : true, E, s_tab, pitch, tid, s_runs, &pay)) atomicOr(&s_flags, kGiveUp);
        if (pay) s_pay = pay;
    }
    __syncthreads();
    if (s_flags & kGiveUp) { r.verdict = kStNotOurs; if (tid == 0) res[f] = r; return; }
    for (uint32_t round = 0; round < kStJumpRounds; round++) {
        for (uint32_t i = tid; i < L; i += kStLanes) {
            const uint32_t w = s_runs[i];
            s_runs[i] = st_run_hop(w, s_runs[st_run_jump(w)]);
        }
        __syncthreads();
    }
    {
        bool far = false;
        for (uint32_t i = tid; i < L; i += kStLanes) far |= st_run_jump(s_runs[i]) != 0;   // more than 2^5 right turns above it
        if (far) atomicOr(&s_flags, kGiveUp);
    }

    // ---- 5. lengths and codes
    uint32_t code = 0;
    {
        uint32_t longest = 0, unused = 0;
        if (!st_lane_lens<S>(ln, E, s_runs, &code, &longest)) atomicOr(&s_flags, kGiveUp);
        if (longest) atomicMax(&s_longest, longest);
        st_block_scan2(code, unused, s_scan);
    }
    if (s_flags & kGiveUp) { r.verdict = kStNotOurs; if (tid == 0) res[f] = r; return; }   // (st_block_scan2's barriers: every lane has set its flag)

    // ---- 6. the table
    if (!st_lane_table<S>(ln, E, s_runs, code, L, row.table, [&](uint32_t pos) { return StSymbolLoad<S>::ld(trie + pos); })) atomicOr(&s_flags, kBadSymbol);
    __syncthreads();
    if (tid == 0) {
        r.verdict = (s_flags & kBadSymbol) ? kStNotDecoder : kStParsed;
        r.leaves = L; r.max_len = s_longest; r.payload_at = 8 + s_pay;
        res[f] = r;
    }
}

__global__ __launch_bounds__(kStLanes) void k_small_trieparse(const SmallTrieRow *__restrict__ rows, uint32_t pitch, uint32_t room, uint32_t max_px, uint64_t img_stride,
                                                              uint32_t scan_w, uint32_t scan_h, SmallTrieResult *__restrict__ res) {
    st_parse_frame<6>(rows, pitch, room, max_px, img_stride, scan_w, scan_h, res);
}
__global__ __launch_bounds__(kStLanes) void k_small_trieparse_rgb(const SmallTrieRow *__restrict__ rows, uint32_t pitch, uint32_t room, uint32_t max_px, uint64_t img_stride,
                                                                  uint32_t scan_w, uint32_t scan_h, SmallTrieResult *__restrict__ res) {
    st_parse_frame<11>(rows, pitch, room, max_px, img_stride, scan_w, scan_h, res);
}

template <uint32_t S, class K> static int st_launch(Ctx *c, K kernel, const SmallTrieRow *rows_d, uint32_t frames, uint64_t max_bytes, uint32_t max_px, uint64_t img_stride,
                                                    uint32_t scan_w, uint32_t scan_h, SmallTrieResult *res_d) {
    const uint32_t window = st_window(max_bytes > 8 ? max_bytes - 8 : 0, st_max_bytes<S>());
    // The lanes a stream occupies do not grow with its length throughout: a window of 32 768 bytes has 1024 lanes of one chunk, one of 40 000
    // bytes 625 lanes of two.  What no shorter stream exceeds is min(1024, the longest window's chunks), which is the pitch for S = 11.  S = 6
    // keeps the longest stream's own lanes, as it was measured: a shorter stream that needs more is not ours there and parsed on the host
    const uint32_t lanes = S == 6 ? st_lanes_used(window) : std::min(kStLanes, st_chunks(window));
    const uint32_t pitch = std::max(1u, lanes), room = std::max(1u, st_leaves_room<S>(max_bytes));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(4 * ((kStMaxP + 1) * kStLanes + kSmallTrieMaxLeaves))));
    hipLaunchKernelGGL(kernel, dim3(frames), dim3(kStLanes), 4 * ((kStMaxP + 1) * pitch + room), c->stream, rows_d, pitch, room, max_px, img_stride, scan_w, scan_h, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}
// sym_bytes: 6 (SignedColor leaves) or 11 (Rgb leaves, for which there is no scan test: scan_w = 0)
int small_trie_run(Ctx *c, uint32_t sym_bytes, const SmallTrieRow *rows_d, uint32_t frames, uint64_t max_bytes, uint32_t max_px, uint64_t img_stride, uint32_t scan_w,
                   uint32_t scan_h, SmallTrieResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (sym_bytes == 6) return st_launch<6>(c, k_small_trieparse, rows_d, frames, max_bytes, max_px, img_stride, scan_w, scan_h, res_d);
    if (sym_bytes == 11) return st_launch<11>(c, k_small_trieparse_rgb, rows_d, frames, max_bytes, max_px, img_stride, 0u, 0u, res_d);
    return c->fail(CNIIC_ERR_HIP, "small_trie_run: no kernel for leaves of %u symbol bytes", sym_bytes);
}

}  // namespace cniic
