// k_zipback_par.hip -- zip(back)'s decode of ONE stream by the whole GPU (the serial walk of one workgroup is k_zb_decode, k_zipback.hip).
// zb_par.hpp has the arithmetic and the reasons; the launches of a stream of n bytes, in stream order:
//
//   k_zbp_next      jump[p] = next(p) for every p in [0, n], position 0 marked
//   k_zbp_chain     zbp_chain_rounds(n) times: marked p marks jump[p]; jump'[p] = jump[jump[p]] (two tables, so that a round reads only
//                   the round before and the marks are exactly the symbol starts)
//   k_zbp_ksum      the bytes the marked positions of a tile of 2048 bring, k_zbp_bscan their exclusive sums (one block),
//   k_zbp_oscan     o of every marked position, and the smallest position with an event: where the serial loop ends
//   k_zbp_result    its (p, o, status) as the ZbState the serial kernel would leave                                 -- the host reads it
//   k_zbp_fill      per symbol before the event: literal bytes to the text, copies' pointers into P (a wave shares a long symbol)
//   k_zbp_round     until no pointer is left (the host reads one flag a round): P'[j] = P[P[j]], or the byte's value once P[P[j]] is final
//
// The tables: two u32 per stream byte (the jumps; later the same bytes hold o as u64), a mark per stream byte, two u32 per text byte
// below min(made, cap).  Nothing is sized by what the stream claims beyond cap.  Every loop is bounded by n, by the text below cap or
// by 32; no kernel waits for another block; no byte outside [in, in + n) is read and none at or behind out + cap written.
#include "common.hpp"
#include "device_utils.hpp"
#include "zb_par.hpp"

namespace cniic {

namespace {

constexpr uint32_t kZbpThreads = 256, kZbpItems = 8, kZbpTile = kZbpThreads * kZbpItems;
constexpr uint32_t kZbpScanThreads = 1024;
constexpr uint32_t kZbpSmallK = 8;          // a lane writes a symbol of up to this many bytes alone; longer ones are shared by its wave
constexpr uint32_t kZbpMaxGrid = 256 * 32;  // grid-stride launches: blocks at the most

struct ZbpHeader { unsigned long long first; uint32_t flag, pad; ZbState state; };

__device__ __forceinline__ uint64_t zbp_block_exclusive_scan64(uint64_t v, uint64_t *wsum, uint64_t *total) {
    const uint64_t inc = wave_inclusive_scan64<false>(v);
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint64_t off = 0, all = 0;
    for (uint32_t i = 0; i < waves; i++) {
        if (i < wid) off += wsum[i];
        all += wsum[i];
    }
    __syncthreads();
    *total = all;
    return off + inc - v;
}

__global__ __launch_bounds__(kZbpThreads) void k_zbp_next(const uint8_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ jump, uint8_t *__restrict__ mark,
                                                          ZbpHeader *__restrict__ hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * kZbpThreads;
    for (uint64_t p = (uint64_t)blockIdx.x * kZbpThreads + threadIdx.x; p <= n; p += stride) {
        jump[p] = (uint32_t)zbp_next(in, n, p);
        mark[p] = p == 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { hdr->first = n; hdr->flag = 0; }
}

// (mark is read and written in one round: a position marked this round marks a later start a round early, never a wrong one)
__global__ __launch_bounds__(kZbpThreads) void k_zbp_chain(const uint32_t *__restrict__ from, uint32_t *__restrict__ to, uint8_t *mark, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * kZbpThreads;
    for (uint64_t p = (uint64_t)blockIdx.x * kZbpThreads + threadIdx.x; p <= n; p += stride) {
        const uint32_t j = from[p];   // <= n
        if (mark[p]) mark[j] = 1;
        to[p] = from[j];
    }
}

__global__ __launch_bounds__(kZbpThreads) void k_zbp_ksum(const uint8_t *__restrict__ in, uint64_t n, const uint8_t *__restrict__ mark, uint64_t *__restrict__ bsum) {
    __shared__ uint64_t s_w[kZbpThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kZbpTile + (uint64_t)threadIdx.x * kZbpItems;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < kZbpItems; i++) {
        const uint64_t p = base + i;
        if (p <= n && mark[p]) v += zbp_k(in, n, p);
    }
    uint64_t total;
    (void)zbp_block_exclusive_scan64(v, s_w, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kZbpScanThreads) void k_zbp_bscan(uint64_t *__restrict__ bsum, uint64_t nb) {
    __shared__ uint64_t s_w[kZbpScanThreads / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nb; base += kZbpScanThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? bsum[i] : 0;
        uint64_t total;
        const uint64_t ex = zbp_block_exclusive_scan64(v, s_w, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kZbpThreads) void k_zbp_oscan(const uint8_t *__restrict__ in, uint64_t n, uint64_t need, const uint8_t *__restrict__ mark,
                                                           const uint64_t *__restrict__ bsum, uint64_t *__restrict__ o_at, ZbpHeader *__restrict__ hdr) {
    __shared__ uint64_t s_w[kZbpThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kZbpTile + (uint64_t)threadIdx.x * kZbpItems;
    uint32_t k[kZbpItems];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < kZbpItems; i++) {
        const uint64_t p = base + i;
        k[i] = p <= n && mark[p] ? zbp_k(in, n, p) : 0;
        v += k[i];
    }
    uint64_t total;
    uint64_t o = bsum[blockIdx.x] + zbp_block_exclusive_scan64(v, s_w, &total);
    uint64_t first = ~0ull;
#pragma unroll
    for (uint32_t i = 0; i < kZbpItems; i++) {
        const uint64_t p = base + i;
        if (p <= n && mark[p]) {
            o_at[p] = o;
            if (first == ~0ull && zbp_event(in, n, need, p, o) != kZbpGo) first = p;
        }
        o += k[i];
    }
    first = wave_reduce_min64(first);
    if ((threadIdx.x & 63) == 0 && first != ~0ull) atomicMin(&hdr->first, (unsigned long long)first);
}

__global__ void k_zbp_result(const uint8_t *__restrict__ in, uint64_t n, uint64_t need, const uint64_t *__restrict__ o_at, ZbpHeader *__restrict__ hdr) {
    const uint64_t p = hdr->first, o = o_at[p];   // (position n is always marked and always an event: first <= n)
    ZbState s;
    s.p = p; s.o = o; s.e = 0; s.status = zbp_event(in, n, need, p, o);
    hdr->state = s;
}

// text byte j = o + t of the symbol at (p, o)
__device__ __forceinline__ void zbp_put(const uint8_t *__restrict__ in, const ZbpHead &h, uint64_t p, uint64_t o, uint32_t t, uint8_t *out, uint32_t *__restrict__ P) {
    const ZbpSource s = zbp_source(h, p, o, t);
    if (s.literal) out[o + t] = in[s.at];
    P[o + t] = zbp_pointer(s);
}

__global__ __launch_bounds__(kZbpThreads) void k_zbp_fill(const uint8_t *__restrict__ in, uint64_t n, const uint8_t *__restrict__ mark, const uint64_t *__restrict__ o_at,
                                                          uint8_t *out, uint32_t *__restrict__ P, uint64_t W, ZbpHeader *__restrict__ hdr) {
    const uint64_t first = hdr->first, stride = (uint64_t)gridDim.x * kZbpThreads;
    const uint32_t lane = threadIdx.x & 63;
    bool copies = false;
    for (uint64_t b = (uint64_t)blockIdx.x * kZbpThreads; b < first; b += stride) {   // (the same trips for every lane of a block)
        const uint64_t p = b + threadIdx.x;
        ZbpHead h{0, 0, 0};
        uint64_t o = 0;
        uint32_t k = 0;
        if (p < first && mark[p]) {   // a symbol before the event: a whole one, p + 2 <= n
            h = zbp_head(in, n, p);
            o = o_at[p];
            k = o < W ? zbp_k(in, n, p) : 0;
        }
        if (k && h.lookback) copies = true;
        if (k <= kZbpSmallK)
            for (uint32_t t = 0; t < k && o + t < W; t++) zbp_put(in, h, p, o, t, out, P);
        uint64_t todo = __ballot(k > kZbpSmallK);
        while (todo) {   // at most 64 symbols, the wave's lanes side by side in each
            const int l = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            ZbpHead hh;
            hh.lookback = (uint32_t)__shfl((int)h.lookback, l);
            hh.len = (uint32_t)__shfl((int)h.len, l);
            hh.back = (uint32_t)__shfl((int)h.back, l);
            const uint32_t kk = (uint32_t)__shfl((int)k, l);
            const uint64_t oo = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(o >> 32), l) << 32) | (uint32_t)__shfl((int)(uint32_t)o, l);
            const uint64_t pp = b + (threadIdx.x & ~63u) + (uint32_t)l;
            for (uint32_t t = lane; t < kk && oo + t < W; t += 64) zbp_put(in, hh, pp, oo, t, out, P);
        }
    }
    if (copies) hdr->flag = 1;
}

__global__ __launch_bounds__(kZbpThreads) void k_zbp_round(const uint32_t *__restrict__ from, uint32_t *__restrict__ to, uint8_t *out, uint64_t W, ZbpHeader *__restrict__ hdr) {
    const uint64_t stride = (uint64_t)gridDim.x * kZbpThreads;
    bool left = false;
    for (uint64_t j = (uint64_t)blockIdx.x * kZbpThreads + threadIdx.x; j < W; j += stride) {
        uint32_t src;
        const uint32_t q = zbp_jump(from, (uint32_t)j, &src);
        if (src != kZbpNil) out[j] = out[src];   // (src was final before this round began: its byte is there)
        to[j] = q;
        left |= q != kZbpNil;
    }
    if (left) hdr->flag = 1;
}

uint32_t zbp_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(kZbpMaxGrid, std::max<uint64_t>(1, (items + kZbpThreads - 1) / kZbpThreads)); }

}  // namespace

uint64_t zb_par_stream_scratch(uint64_t n) { return 9 * (n + 1) + 8 * ((n + 1 + kZbpTile - 1) / kZbpTile) + sizeof(ZbpHeader); }

int zb_par_decode_stream(Ctx *c, const ZbStream &s, uint32_t round_cap, ZbState *st, uint32_t *rounds, bool *handed) {
    const uint64_t n = s.n, nb = (n + 1 + kZbpTile - 1) / kZbpTile;
    *rounds = 0;
    *handed = false;
    DevBuf jbuf, markb, bsumb, hdrb, pbuf;
    CNIIC_HIP_TRY(c, jbuf.alloc(8 * (n + 1)));
    CNIIC_HIP_TRY(c, markb.alloc(n + 1));
    CNIIC_HIP_TRY(c, bsumb.alloc(8 * nb));
    CNIIC_HIP_TRY(c, hdrb.alloc(sizeof(ZbpHeader)));
    uint32_t *jump[2] = {jbuf.as<uint32_t>(), jbuf.as<uint32_t>() + (n + 1)};
    uint64_t *o_at = jbuf.as<uint64_t>();   // (the jumps are over when o is written)
    uint8_t *mark = markb.as<uint8_t>();
    ZbpHeader *hdr = hdrb.as<ZbpHeader>();
    hipLaunchKernelGGL(k_zbp_next, dim3(zbp_grid(n + 1)), dim3(kZbpThreads), 0, c->stream, s.in, n, jump[0], mark, hdr);
    const uint32_t R = zbp_chain_rounds(n);
    for (uint32_t r = 0; r < R; r++)
        hipLaunchKernelGGL(k_zbp_chain, dim3(zbp_grid(n + 1)), dim3(kZbpThreads), 0, c->stream, jump[r & 1], jump[(r & 1) ^ 1], mark, n);
    hipLaunchKernelGGL(k_zbp_ksum, dim3((uint32_t)nb), dim3(kZbpThreads), 0, c->stream, s.in, n, mark, bsumb.as<uint64_t>());
    hipLaunchKernelGGL(k_zbp_bscan, dim3(1), dim3(kZbpScanThreads), 0, c->stream, bsumb.as<uint64_t>(), nb);
    hipLaunchKernelGGL(k_zbp_oscan, dim3((uint32_t)nb), dim3(kZbpThreads), 0, c->stream, s.in, n, s.need, mark, bsumb.as<uint64_t>(), o_at, hdr);
    hipLaunchKernelGGL(k_zbp_result, dim3(1), dim3(1), 0, c->stream, s.in, n, s.need, o_at, hdr);
    CNIIC_HIP_TRY(c, hipGetLastError());
    ZbpHeader h;
    CNIIC_HIP_TRY(c, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *st = h.state;
    if (st->status != kZbDone) return CNIIC_OK;   // a failing stream promises nothing below cap
    const uint64_t W = std::min(st->o, s.cap);
    if (W >= (1ull << 32) || 8 * W > kZbParScratchMax) { *handed = true; return CNIIC_OK; }
    if (!W) return CNIIC_OK;
    CNIIC_HIP_TRY(c, pbuf.alloc(8 * W));
    uint32_t *P[2] = {pbuf.as<uint32_t>(), pbuf.as<uint32_t>() + W};
    hipLaunchKernelGGL(k_zbp_fill, dim3(zbp_grid(h.first)), dim3(kZbpThreads), 0, c->stream, s.in, n, mark, o_at, s.out, P[0], W, hdr);
    for (uint32_t r = 0;; r++) {
        CNIIC_HIP_TRY(c, hipGetLastError());
        CNIIC_HIP_TRY(c, hipMemcpyAsync(&h.flag, &hdr->flag, sizeof h.flag, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!h.flag) break;
        if (r >= round_cap || r >= kZbpMaxRounds) { *handed = true; break; }
        CNIIC_HIP_TRY(c, hipMemsetAsync(&hdr->flag, 0, sizeof h.flag, c->stream));
        hipLaunchKernelGGL(k_zbp_round, dim3(zbp_grid(W)), dim3(kZbpThreads), 0, c->stream, P[r & 1], P[(r & 1) ^ 1], s.out, W, hdr);
        *rounds = r + 1;
    }
    return CNIIC_OK;
}

}  // namespace cniic
