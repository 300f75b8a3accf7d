// k_delta_small.hip -- `delta` of SMALL frames (at most kDeltaSmallMaxPx pixels), one workgroup per frame, any number of frames in one
// launch (cniic_codec_encode_batch_var / cniic_codec_measure_batch; codec.cpp delta_small_encode).  A small `delta` frame is mostly its
// tree -- thousands of leaves, nearly all tied -- and the block goes from the pixels to the finished stream without the host:
//   a. symbols: a lane per scan position, the pixel read byte-wise, the difference to the position before as a CNIIC_SYM_SIGNED key
//   b. alphabet: bitonic sort of the keys, heads of runs, scan, compaction: keys ascending with their counts
//   c. tree: leaves sorted by (count, key), then the two-queue merge of huff_host.cpp on ONE wave, whole runs of leaf pairs / branch pairs
//      per step (delta_small.hpp says why a run's pairs can be tested together); weights and links share 16-bit slots
//   d. every node walks to the root: pre-order offsets for all, codes for the leaves; the header is written
//   e. payload: the symbol's code by binary search in the ascending keys, a block-wide prefix sum of the lengths, bits MSB first
// LDS (8 bytes per pixel of the launch's largest frame, rounded up to a power of two: 128 KiB at the bound) holds, by phase,
//   a-b  keys u32 | head positions u16          c   (keys to HBM) | leaf order words u32
//   c-d  rank of leaf q u16, leaf slots u16 | branch slots u16, leaves under a branch u16
//   e    keys u32 | code words u32 (both back from HBM)
// and a per-frame HBM slice of 12 bytes per pixel holds what LDS cannot beside the tree: the position-ordered symbols (read once more in e),
// the ascending keys (read by d for the header, reloaded by e) and the code words by rank (written by d, loaded by e).  No block waits for
// another.
//
// `hufman` of small frames (k_huf_small; codec.cpp huf_small_encode) is the same body, phases b-e untouched, under another SYMBOL KIND
// (DsKindRgb below): the symbols are the pixels' colours in row-major order, so phase a needs no scan and no tables, a leaf's record is
// 12 bytes against 7 and a subtree 13 * leaves - 1 bytes against 8 * leaves - 1 (huf_small.hpp).  The longest code is a matter of counts
// (delta_small.hpp) and holds for both.
#include "common.hpp"
#include "hilbert_scan.hpp"
#include "delta_sym.hpp"
#include "delta_small.hpp"
#include "huf_small.hpp"

namespace cniic {

constexpr int kDsThreads = 1024;
constexpr uint32_t kDsPer = kDeltaSmallMaxPx / kDsThreads;   // positions / leaves per thread at the bound
static_assert(kDsPer == 16, "the per-thread register arrays below hold 16");
constexpr uint32_t kDsMinCap = 64;
constexpr uint32_t kDsAtRoot = 0xffffffffu;   // a walk's link once it has reached the root

// bytes of dynamic LDS for frames of at most cap_px pixels (a power of two)
static uint32_t ds_lds_bytes(uint32_t cap_px) { return std::max(cap_px, kDsMinCap) * 8; }
static_assert(kDeltaSmallMaxPx * 8 + 2048 + 16 + 256 <= 160 * 1024, "the largest routed frame, the 2^n scan tables and the scan's words fit one CU's LDS");

// exclusive scan over the block's 1024 threads; s_w[16] = the sum.  s_w: 17 words
__device__ __forceinline__ uint32_t ds_block_scan(uint32_t v, uint32_t *s_w) {
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
        for (int w = 0; w < kDsThreads / 64; w++) { const uint32_t t = s_w[w]; s_w[w] = run; run += t; }
        s_w[kDsThreads / 64] = run;
    }
    __syncthreads();
    return s_w[wv] + inc - v;
}

// ascending bitonic sort of s[0 .. P), P a power of two (P = 1: nothing); ends with a barrier
__device__ __forceinline__ void ds_sort(uint32_t *s, uint32_t P) {
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (uint32_t t = threadIdx.x; t < P / 2; t += kDsThreads) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint32_t u = s[lo], v = s[hi];
                if ((u > v) == ((lo & k) == 0)) { s[lo] = v; s[hi] = u; }
            }
        }
    __syncthreads();
}

// ---- a. THE SYMBOL SOURCE: the frame's n symbols by scan position, into s_sym[0 .. n) and syms_g[0 .. n).  (Another codec's small-frame
// route replaces this function alone.)  Ends with a barrier.
__device__ __forceinline__ void ds_symbols(const Scan &sc, const uint8_t *__restrict__ src, uint32_t w, uint32_t n, uint32_t *s_sym, uint32_t *__restrict__ syms_g) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t d = tid; d < n; d += kDsThreads) {
        uint32_t x, y;
        sc.xy(d, x, y);
        const uint8_t *p = src + 3ull * ((uint64_t)y * w + x);
        s_sym[d] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    __syncthreads();
    uint32_t key[kDsPer];
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t d = tid + q * kDsThreads;
        uint32_t hot;
        key[q] = d < n ? delta_key(s_sym[d], d ? s_sym[d - 1] : 0u /* START, hilbertc.rs:445 */, hot) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t d = tid + q * kDsThreads;
        if (d < n) { s_sym[d] = key[q]; syms_g[d] = key[q]; }
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t ds_leading(bool ok) {   // how many lanes from lane 0 on pass, wave-uniform
    const uint64_t m = __ballot(ok);
    return m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
}

// ---- a, for `hufman`: the symbols are the pixels themselves in row-major order, r << 16 | g << 8 | b: no scan, no tables.  Ends with a barrier.
__device__ __forceinline__ void hs_symbols(const uint8_t *__restrict__ src, uint32_t n, uint32_t *s_sym, uint32_t *__restrict__ syms_g) {
    for (uint32_t d = threadIdx.x; d < n; d += kDsThreads) {
        const uint8_t *p = src + 3ull * d;
        const uint32_t key = hs_key(p[0], p[1], p[2]);
        s_sym[d] = key; syms_g[d] = key;
    }
    __syncthreads();
}

// ---- THE SYMBOL KIND: what the phases below ask of a codec -- whether the symbols come along a scan (a), a leaf's record and the
// subtree's size (d), the stream's sizes (b, e).  Everything else (sort, leaf order, merge, walks, search, pack) knows counts and keys only.
struct DsKindDelta {   // `delta`: differences along the Hilbert scan, a leaf is tag + three i16 (delta_small.hpp)
    static constexpr bool kScan = true;
    static constexpr uint32_t kLeaf = 7;
    static __device__ __forceinline__ void leaf_bytes(uint32_t key, uint8_t *o) { ds_leaf_bytes(key, o); }
    static __device__ __forceinline__ void walk_step(DsWalk &wk, uint32_t link, uint32_t leaves, uint32_t pl) { ds_walk_step(wk, link, leaves, pl); }
    static __device__ __forceinline__ uint32_t header_bytes(uint32_t U) { return (uint32_t)ds_header_bytes(U); }
    static __device__ __forceinline__ uint32_t stream_bytes(uint32_t U, uint32_t bits) { return (uint32_t)ds_stream_bytes(U, bits); }
};
struct DsKindRgb {     // `hufman`: the pixels in row-major order, a leaf is tag + u64 3 + r, g, b (huf_small.hpp)
    static constexpr bool kScan = false;
    static constexpr uint32_t kLeaf = 1 + kHufSmallLeafSym;
    static __device__ __forceinline__ void leaf_bytes(uint32_t key, uint8_t *o) { hs_leaf_bytes(key, o); }
    static __device__ __forceinline__ void walk_step(DsWalk &wk, uint32_t link, uint32_t leaves, uint32_t pl) { hs_walk_step(wk, link, leaves, pl); }
    static __device__ __forceinline__ uint32_t header_bytes(uint32_t U) { return (uint32_t)hs_header_bytes(U); }
    static __device__ __forceinline__ uint32_t stream_bytes(uint32_t U, uint32_t bits) { return (uint32_t)hs_stream_bytes(U, bits); }
};

// one frame, from the pixels to the finished stream (k_delta_small and k_huf_small below are this body under the two kinds)
template <class Kind>
__device__ __forceinline__ void ds_frame(const DeltaSmallRow *__restrict__ rows, uint32_t cap_px, const HilbertLut *__restrict__ lut, uint8_t *__restrict__ scratch,
                                         uint64_t sstride, uint32_t *__restrict__ tmp, uint64_t tpx, DeltaSmallResult *__restrict__ res) {
    extern __shared__ __align__(16) uint8_t ds_lds[];
    __shared__ uint32_t s_scan[kDsThreads / 64 + 1];
    __shared__ uint32_t s_bad;   // a walk did not end at the root within the longest code: the frame is reported, not written
    if (threadIdx.x == 0) s_bad = 0;
    const uint32_t cap = max(cap_px, kDsMinCap);
    uint32_t *s_a = reinterpret_cast<uint32_t *>(ds_lds);   // [cap]
    uint32_t *s_b = s_a + cap;                              // [cap]
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const DeltaSmallRow row = rows[f];
    const uint32_t w = row.w, h = row.h, n = w * h;         // 1 .. cap_px
    uint8_t *__restrict__ slot = scratch + (uint64_t)f * sstride;
    uint32_t *__restrict__ syms_g = tmp + (uint64_t)f * 3 * tpx, *__restrict__ keys_g = syms_g + tpx, *__restrict__ cw_g = keys_g + tpx;

    // ---- a. symbols
    if constexpr (Kind::kScan) {
        __shared__ uint16_t s_l4[1024];
        __shared__ uint8_t s_l1[16];
        const uint32_t order = (w == h && w >= 2 && !(w & (w - 1))) ? (uint32_t)__builtin_ctz(w) : 0u;   // (pow2_order, k_hilbert.hip)
        const Scan sc = load_scan(w, h, order, order ? lut : nullptr, s_l4, s_l1);
        ds_symbols(sc, row.src, w, n, s_a, syms_g);
    } else {
        hs_symbols(row.src, n, s_a, syms_g);
    }

    // ---- b. sort, unique
    uint32_t P = 1;
    while (P < n) P <<= 1;   // <= cap
    for (uint32_t i = n + tid; i < P; i += kDsThreads) s_a[i] = 0xffffffffu;
    ds_sort(s_a, P);
    // thread t holds the `per` sorted keys from t * per on; the heads of runs of one key are the distinct symbols
    uint16_t *s_hd = reinterpret_cast<uint16_t *>(s_b);   // [cap]: where each distinct symbol's run begins
    const uint32_t per = P > (uint32_t)kDsThreads ? P / kDsThreads : 1;   // <= 16
    const uint32_t first = tid * per;
    uint32_t kv[kDsPer];
    uint32_t heads = 0, nheads = 0;
    {
        uint32_t prev = first > 0 && first <= n ? s_a[first - 1] : 0xffffffffu;
#pragma unroll
        for (uint32_t q = 0; q < kDsPer; q++) {
            const uint32_t i = first + q;
            const bool live = q < per && i < n;
            kv[q] = live ? s_a[i] : 0xffffffffu;
            if (live && (i == 0 || kv[q] != prev)) { heads |= 1u << q; nheads++; }
            prev = kv[q];
        }
    }
    uint32_t rank = ds_block_scan(nheads, s_scan);   // (its barriers: every thread has read its span)
    const uint32_t U = s_scan[kDsThreads / 64];
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++)
        if ((heads >> q) & 1u) { s_a[rank] = kv[q]; s_hd[rank] = (uint16_t)(first + q); rank++; }
    __syncthreads();
    const uint32_t hdr = Kind::header_bytes(U);
    if (U == 1) {   // one symbol: the zero-length code and no payload (huf.rs:140-142)
        if (tid == 0) {
            for (int i = 0; i < 4; i++) { slot[i] = (uint8_t)(w >> (8 * i)); slot[4 + i] = (uint8_t)(h >> (8 * i)); }
            slot[8] = 0;
            Kind::leaf_bytes(s_a[0], slot + 9);
            res[f] = DeltaSmallResult{1u, hdr};
        }
        return;
    }
    // a symbol's count: from its head to the next symbol's; its leaf order word
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t r = tid + q * kDsThreads;
        kv[q] = r < U ? ds_leaf_order((r + 1 < U ? (uint32_t)s_hd[r + 1] : n) - (uint32_t)s_hd[r], r) : 0xffffffffu;
        if (r < U) keys_g[r] = s_a[r];
    }
    // (meanwhile) the payload's words are ORed together in e: zero from the word the header ends in to the longest payload's last
    {
        uint32_t *words = reinterpret_cast<uint32_t *>(slot);
        const uint32_t w0 = hdr >> 2, w1 = (hdr + (kDeltaSmallMaxCodeLen * n + 7) / 8 + 3) >> 2;   // (<= sstride / 4: ds_stride)
        for (uint32_t i = w0 + tid; i < w1; i += kDsThreads) words[i] = 0u;
    }
    __syncthreads();

    // ---- c. leaves by (count, key), then the merge
    uint32_t P2 = 1;
    while (P2 < U) P2 <<= 1;
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t r = tid + q * kDsThreads;
        if (r < P2) s_b[r] = kv[q];
    }
    ds_sort(s_b, P2);
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t r = tid + q * kDsThreads;
        kv[q] = r < U ? s_b[r] : 0u;
    }
    __syncthreads();
    uint16_t *s_qrank = reinterpret_cast<uint16_t *>(s_a);   // [cap]: leaf q's rank among the ascending keys
    uint16_t *s_lq = s_qrank + cap;                          // [cap]: leaf q's weight, then its link
    uint16_t *s_bq = reinterpret_cast<uint16_t *>(s_b);      // [cap]: branch j's weight, then its link (the root keeps its weight)
    uint16_t *s_nl = s_bq + cap;                             // [cap]: leaves below branch j
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t r = tid + q * kDsThreads;
        if (r < U) { s_qrank[r] = (uint16_t)ds_order_rank(kv[q]); s_lq[r] = (uint16_t)ds_order_count(kv[q]); }
    }
    __syncthreads();
    const uint32_t nbr = U - 1, root = U - 2;
    if (tid < 64) {   // one wave: li / bi = the queues' heads, made = branches so far; every lane keeps the same three
        const uint32_t lane = tid;
        uint32_t li = 0, bi = 0, made = 0;
        while (made < nbr) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            {   // a run of leaf pairs
                const bool hb = bi < made;
                const uint32_t bw = hb ? s_bq[bi] : 0u;
                const uint32_t i1 = li + 2 * lane + 1;
                const uint32_t cnt = ds_leading((hb || lane == 0) && i1 < U && ds_leaf_pair(s_lq[i1 < U ? i1 : 0], hb, bw));
                if (cnt) {
                    if (lane < cnt) {
                        const uint32_t a = s_lq[i1 - 1], b = s_lq[i1];
                        s_lq[i1 - 1] = (uint16_t)ds_link(made + lane, 0);
                        s_lq[i1] = (uint16_t)ds_link(made + lane, 1);
                        s_bq[made + lane] = (uint16_t)(a + b);
                        s_nl[made + lane] = 2;
                    }
                    li += 2 * cnt; made += cnt;
                    continue;
                }
            }
            {   // a run of branch pairs (among the branches that exist now)
                const bool hl = li < U;
                const uint32_t lw = hl ? s_lq[li] : 0u;
                const uint32_t i1 = bi + 2 * lane + 1;
                const uint32_t cnt = ds_leading(i1 < made && ds_branch_pair(s_bq[i1 < made ? i1 : 0], hl, lw));
                if (cnt) {
                    if (lane < cnt) {
                        const uint32_t a = s_bq[i1 - 1], b = s_bq[i1], na = s_nl[i1 - 1], nb = s_nl[i1];
                        s_bq[i1 - 1] = (uint16_t)ds_link(made + lane, 0);
                        s_bq[i1] = (uint16_t)ds_link(made + lane, 1);
                        s_bq[made + lane] = (uint16_t)(a + b);
                        s_nl[made + lane] = (uint16_t)(na + nb);
                    }
                    bi += 2 * cnt; made += cnt;
                    continue;
                }
            }
            // the general step: a leaf and a branch
            uint32_t wsum = 0, leaves = 0;
            for (uint32_t k = 0; k < 2; k++) {
                const bool hl = li < U, hb = bi < made;
                const uint32_t lw = hl ? s_lq[li] : 0u, bw = hb ? s_bq[bi] : 0u;
                if (ds_pick_leaf(hl, lw, hb, bw)) {
                    wsum += lw; leaves += 1;
                    if (lane == 0) s_lq[li] = (uint16_t)ds_link(made, k);
                    li++;
                } else {
                    wsum += bw; leaves += s_nl[bi];
                    if (lane == 0) s_bq[bi] = (uint16_t)ds_link(made, k);
                    bi++;
                }
            }
            if (lane == 0) { s_bq[made] = (uint16_t)wsum; s_nl[made] = (uint16_t)leaves; }
            made++;
        }
    }
    __syncthreads();

    // ---- d. offsets, codes, header
    for (uint32_t q = tid; q < U; q += kDsThreads) {
        DsWalk wk;
        uint32_t link = s_lq[q], leaves = 1;
        for (uint32_t s = 0; s < kDeltaSmallMaxCodeLen; s++) {
            const uint32_t p = ds_link_parent(link), pl = s_nl[p];
            Kind::walk_step(wk, link, leaves, pl);
            if (p == root) { link = kDsAtRoot; break; }
            leaves = pl;
            link = s_bq[p];
        }
        if (link != kDsAtRoot || wk.off + Kind::kLeaf > hdr - 8) { s_bad = 1; continue; }   // (cannot happen: delta_small.hpp's bound; nothing is written out of place)
        const uint32_t r = s_qrank[q];
        cw_g[r] = ds_codeword(wk.code, wk.depth);
        uint8_t *o = slot + 8 + wk.off;
        o[0] = 0;
        Kind::leaf_bytes(keys_g[r], o + 1);
    }
    for (uint32_t j = tid; j < nbr; j += kDsThreads) {
        DsWalk wk;
        if (j != root) {
            uint32_t link = s_bq[j], leaves = s_nl[j];
            for (uint32_t s = 0; s < kDeltaSmallMaxCodeLen; s++) {
                const uint32_t p = ds_link_parent(link), pl = s_nl[p];
                Kind::walk_step(wk, link, leaves, pl);
                if (p == root) { link = kDsAtRoot; break; }
                leaves = pl;
                link = s_bq[p];
            }
            if (link != kDsAtRoot || wk.off + 1 > hdr - 8) { s_bad = 1; continue; }
        }
        slot[8 + wk.off] = 1;
    }
    if (tid < 8) slot[tid] = (uint8_t)((tid < 4 ? w : h) >> (8 * (tid & 3)));
    __syncthreads();

    // ---- e. payload
    for (uint32_t r = tid; r < U; r += kDsThreads) { s_a[r] = keys_g[r]; s_b[r] = cw_g[r]; }
    __syncthreads();
    const uint32_t per2 = (n + kDsThreads - 1) / kDsThreads, d0 = tid * per2;   // consecutive positions per thread
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t q = 0; q < kDsPer; q++) {
        const uint32_t d = d0 + q;
        kv[q] = 0;
        if (q < per2 && d < n) {
            const uint32_t key = syms_g[d];
            uint32_t lo = 0, hi = U;   // keys[lo] <= key < keys[hi]: the key is one of them
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_a[mid] <= key) lo = mid; else hi = mid;
            }
            kv[q] = s_b[lo];
            bits += ds_codeword_len(kv[q]);
        }
    }
    const uint32_t start = ds_block_scan(bits, s_scan);
    const uint32_t total = s_scan[kDsThreads / 64];
    if (bits) {
        // bit p of the stream is bit 7 - (p & 7) of byte p >> 3: 32-bit big-endian words, byte-swapped into place.  The first and the last
        // word of a thread's bits may be shared with its neighbours (ORed); the words between are its own
        uint32_t *words = reinterpret_cast<uint32_t *>(slot);
        const uint32_t p = hdr * 8 + start;
        uint32_t wi = p >> 5, nb = p & 31;
        uint64_t acc = 0;
        bool own = false;
#pragma unroll
        for (uint32_t q = 0; q < kDsPer; q++) {
            const uint32_t len = ds_codeword_len(kv[q]);
            if (!len) continue;
            acc |= (uint64_t)ds_codeword_code(kv[q]) << (64 - nb - len);
            nb += len;
            if (nb >= 32) {
                const uint32_t v = __builtin_bswap32((uint32_t)(acc >> 32));
                if (own) words[wi] = v; else atomicOr(&words[wi], v);
                own = true;
                wi++; acc <<= 32; nb -= 32;
            }
        }
        if (nb) atomicOr(&words[wi], __builtin_bswap32((uint32_t)(acc >> 32)));
    }
    if (tid == 0) res[f] = DeltaSmallResult{U, s_bad ? 0u : Kind::stream_bytes(U, total)};
}

__global__ __launch_bounds__(kDsThreads) void k_delta_small(const DeltaSmallRow *__restrict__ rows, uint32_t cap_px, const HilbertLut *__restrict__ lut,
                                                            uint8_t *__restrict__ scratch, uint64_t sstride, uint32_t *__restrict__ tmp, uint64_t tpx,
                                                            DeltaSmallResult *__restrict__ res) {
    ds_frame<DsKindDelta>(rows, cap_px, lut, scratch, sstride, tmp, tpx, res);
}

// `hufman` of small frames: the same body over the pixels' own colours (no scan: neither load_scan nor its tables in LDS)
__global__ __launch_bounds__(kDsThreads) void k_huf_small(const DeltaSmallRow *__restrict__ rows, uint32_t cap_px, uint8_t *__restrict__ scratch, uint64_t sstride,
                                                          uint32_t *__restrict__ tmp, uint64_t tpx, DeltaSmallResult *__restrict__ res) {
    ds_frame<DsKindRgb>(rows, cap_px, nullptr, scratch, sstride, tmp, tpx, res);
}

int delta_small_run(Ctx *c, const DeltaSmallRow *rows_d, uint32_t frames, uint32_t max_px, uint8_t *scratch_d, uint64_t sstride, uint32_t *tmp_d, uint64_t tmp_px,
                    DeltaSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kDeltaSmallMaxPx || tmp_px < max_px || sstride < ds_stride(max_px) || (sstride & 15))
        return c->fail(CNIIC_ERR_BAD_ARG, "delta_small: frame size or scratch outside the route");
    const HilbertLut *lut = nullptr;
    CNIIC_TRY(hilbert_lut(c, &lut));
    uint32_t cap_px = 1;
    while (cap_px < max_px) cap_px <<= 1;
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_delta_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ds_lds_bytes(kDeltaSmallMaxPx)));
    hipLaunchKernelGGL(k_delta_small, dim3(frames), dim3(kDsThreads), ds_lds_bytes(cap_px), c->stream, rows_d, cap_px, lut, scratch_d, sstride, tmp_d, tmp_px, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

int huf_small_run(Ctx *c, const DeltaSmallRow *rows_d, uint32_t frames, uint32_t max_px, uint8_t *scratch_d, uint64_t sstride, uint32_t *tmp_d, uint64_t tmp_px,
                  DeltaSmallResult *res_d) {
    if (!frames) return CNIIC_OK;
    if (max_px == 0 || max_px > kHufSmallMaxPx || tmp_px < max_px || sstride < hs_stride(max_px) || (sstride & 15))
        return c->fail(CNIIC_ERR_BAD_ARG, "huf_small: frame size or scratch outside the route");
    uint32_t cap_px = 1;
    while (cap_px < max_px) cap_px <<= 1;
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_huf_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ds_lds_bytes(kHufSmallMaxPx)));
    hipLaunchKernelGGL(k_huf_small, dim3(frames), dim3(kDsThreads), ds_lds_bytes(cap_px), c->stream, rows_d, cap_px, scratch_d, sstride, tmp_d, tmp_px, res_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
