// k_zipback.hip -- the look-back coder of zip(back) (reference: src/zip/back.rs).  zipback.cpp has the host side and the codec.
//
// The parse is serial: where the next probe stands depends on what the last one found.  So ONE workgroup owns one stream and walks it
// probe by probe; what the workgroup shares is the work inside a probe -- the reference visits every earlier occurrence of the six-byte
// key in its 65 535-byte window (back.rs:253-277), here the 1024 lanes scan a slice of the window each.  The window, and the text a
// match may run into, lie in LDS: a ring of 128 KiB indexed by position & 0x1FFFF holds text[p - 65535, p + 65536) at its fullest, and
// the whole block refills it from HBM as p advances.  No index, no sort, no speculation: a probe is a scan, a block reduction of
// (length << 16 | back) -- the longest run, the farthest among equals, which is what the reference's ascending visit with a strict `>`
// leaves (back.rs:264-275) -- and a step every lane takes together.
//
// A launch takes a stream forward by a bounded slice of text (or of stream, in decode) and leaves (position, explicit length, output
// position, status) in a small record in HBM, from which the next launch goes on: no launch runs for long on a large stream, and a
// batch's long streams do not hold a CU while short ones wait.  Streams of a batch are blocks of the same launches.
//
// Every loop is bounded by the text's length; there are no spins and no communication between blocks.
#include "common.hpp"

namespace cniic {

namespace {

constexpr uint32_t kZbThreads = 1024, kZbWaves = kZbThreads / 64;
constexpr uint32_t kZbRing = 1u << 17, kZbMask = kZbRing - 1;
constexpr uint32_t kZbWindow = 65535;      // MAX_RING_BUFFER_SIZE (back.rs:291)
constexpr uint32_t kZbMin = 6;             // MIN_REP (:143)
constexpr uint32_t kZbMaxLen = 32767;      // Len::MAX >> 1 (:45)
constexpr uint32_t kZbAhead = 65536;       // a refill brings the ring up to text[p + kZbAhead)
constexpr uint32_t kZbNeedAhead = 32768 + 8;   // ... and is due when less than this lies ahead: a run of 32 768 bytes must be seen to be refused, and a
                                               // read of four bytes may start at its last one
constexpr uint32_t kZbStage = 16384;       // decode: the stream comes through LDS in pieces of this size
constexpr uint32_t kZbDecLds = kZbRing + kZbStage;
static_assert(kZbWindow + kZbAhead <= kZbRing, "history and look-ahead share the ring");
static_assert(kZbDecLds <= 160 * 1024, "one block per CU");

// four bytes of the ring from any position (what lies behind the filled part is read too and never counted)
__device__ __forceinline__ uint32_t zb_ld4(const uint32_t *ringw, uint64_t pos) {
    const uint32_t i = ((uint32_t)pos & kZbMask) >> 2;
    const uint64_t two = ((uint64_t)ringw[(i + 1) & (kZbMask >> 2)] << 32) | ringw[i];
    return (uint32_t)(two >> (8 * ((uint32_t)pos & 3)));
}

// text[from, to) into the ring, the whole block; to - from <= kZbRing.  Words where the text's address allows it.
__device__ void zb_fill(uint8_t *ring, const uint8_t *__restrict__ text, uint64_t from, uint64_t to) {
    if ((reinterpret_cast<uintptr_t>(text) & 3) == 0 && to - from >= 8) {
        const uint64_t a = (from + 3) & ~3ull, b = to & ~3ull;
        for (uint64_t i = from + threadIdx.x; i < a; i += kZbThreads) ring[i & kZbMask] = text[i];
        const uint32_t *tw = reinterpret_cast<const uint32_t *>(text);
        uint32_t *rw = reinterpret_cast<uint32_t *>(ring);
        for (uint64_t i = (a >> 2) + threadIdx.x; i < (b >> 2); i += kZbThreads) rw[i & (kZbMask >> 2)] = tw[i];
        for (uint64_t i = b + threadIdx.x; i < to; i += kZbThreads) ring[i & kZbMask] = text[i];
    } else {
        for (uint64_t i = from + threadIdx.x; i < to; i += kZbThreads) ring[i & kZbMask] = text[i];
    }
}

__device__ __forceinline__ void zb_put16(uint8_t *out, uint64_t cap, uint64_t at, uint32_t v) {
    if (at < cap) out[at] = (uint8_t)v;
    if (at + 1 < cap) out[at + 1] = (uint8_t)(v >> 8);
}

// ---------------------------------------------------------------- encode
// Encoder::next_symbols (back.rs:148-212) for stream blockIdx.x, from states[blockIdx.x] on, until `slice` more bytes of text are
// accepted, the text is done or the reference would panic.  Bytes behind cap are counted (ZbState::o) and not written.
__global__ __launch_bounds__(kZbThreads) void k_zb_encode(const ZbStream *__restrict__ streams, ZbState *__restrict__ states, uint64_t slice) {
    extern __shared__ uint32_t zb_lds[];
    __shared__ uint32_t s_red[2][kZbWaves];
    uint32_t *ringw = zb_lds;
    uint8_t *ring = reinterpret_cast<uint8_t *>(zb_lds);
    const ZbState s0 = states[blockIdx.x];
    if (s0.status != kZbRunning) return;
    const uint8_t *__restrict__ text = streams[blockIdx.x].in;
    uint8_t *out = streams[blockIdx.x].out;
    const uint64_t n = streams[blockIdx.x].n, cap = streams[blockIdx.x].cap;
    uint64_t p = s0.p, o = s0.o;
    uint32_t e = s0.e, status = kZbRunning, parity = 0;
    const uint64_t stop = p + slice;
    uint64_t hi = min(n, p + kZbAhead);   // the ring holds text[max(0, hi - kZbRing), hi), which includes text[p - kZbWindow, p)
    zb_fill(ring, text, p > kZbWindow ? p - kZbWindow : 0, hi);
    __syncthreads();
    while (p < stop) {
        if (hi < n && hi < p + kZbNeedAhead) {   // (what this overwrites lies before p - kZbWindow)
            const uint64_t nh = min(n, p + kZbAhead);
            __syncthreads();
            zb_fill(ring, text, hi, nh);
            hi = nh;
            __syncthreads();
        }
        uint32_t best = 0;
        if (p >= kZbMin && p + kZbMin <= n) {   // next_repetition (:214-277): candidates q in [p - 65535, p - 6]
            const uint64_t qlo = p > kZbWindow ? p - kZbWindow : 0, qhi = p - kZbMin;
            const uint32_t k4 = zb_ld4(ringw, p), k2 = zb_ld4(ringw, p + 4) & 0xffffu;
            const uint32_t ahead = (uint32_t)min(n - p, (uint64_t)kZbMaxLen + 1);
            for (uint64_t i = (qlo >> 2) + threadIdx.x; i <= (qhi >> 2); i += kZbThreads) {
                const uint32_t wi = (uint32_t)i & (kZbMask >> 2);
                const uint32_t d0 = ringw[wi], d1 = ringw[(wi + 1) & (kZbMask >> 2)], d2 = ringw[(wi + 2) & (kZbMask >> 2)];
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t a = (uint32_t)((((uint64_t)d1 << 32) | d0) >> (8 * j));
                    const uint32_t b = (uint32_t)((((uint64_t)d2 << 32) | d1) >> (8 * j)) & 0xffffu;
                    if (a != k4 || b != k2) continue;
                    const uint64_t q = 4 * i + j;
                    if (q < qlo || q > qhi) continue;
                    // the common run of text[q, p) and text[p, n) (:265-269), as far as a header can say -- and one more, to know that it cannot
                    const uint32_t lim = min((uint32_t)(p - q), ahead);
                    uint32_t l = kZbMin;
                    while (l + 4 <= lim && zb_ld4(ringw, q + l) == zb_ld4(ringw, p + l)) l += 4;
                    while (l < lim && ring[(q + l) & kZbMask] == ring[(p + l) & kZbMask]) l++;
                    best = max(best, (l << 16) | (uint32_t)(p - q));
                }
            }
            for (int off = 32; off; off >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, off));
            if ((threadIdx.x & 63) == 0) s_red[parity][threadIdx.x >> 6] = best;
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kZbWaves; k++) best = max(best, s_red[parity][k]);
            best = __builtin_amdgcn_readfirstlane(best);
            parity ^= 1;   // (the next probe's partial results go to the other row: one barrier a probe)
        }
        if (best) {   // push_explicit, push_lookback (:197-199)
            const uint32_t L = best >> 16, back = best & 0xffffu;
            if (L > kZbMaxLen) { status = kZbBadLookback; break; }
            if (threadIdx.x == 0) {
                if (e) zb_put16(out, cap, o - e - 2, e);
                zb_put16(out, cap, o, 0x8000u | L);
                zb_put16(out, cap, o + 2, back);
            }
            o += 4;
            p += L;
            e = 0;
        } else {      // extend_explicit (:163-186): max(e, 2) more bytes behind a header slot that is filled when the run is written
            uint32_t t = max(e, 2u);
            const bool last = n - p < t;
            if (last) t = (uint32_t)(n - p);
            if (!e && t) o += 2;
            for (uint32_t i = threadIdx.x; i < t; i += kZbThreads)
                if (o + i < cap) out[o + i] = ring[(p + i) & kZbMask];
            o += t;
            p += t;
            e += t;
            if (e > kZbMaxLen) { status = kZbBadExplicit; break; }
            if (last) {
                if (e && threadIdx.x == 0) zb_put16(out, cap, o - e - 2, e);
                status = kZbDone;
                break;
            }
        }
    }
    if (threadIdx.x == 0) {
        ZbState s;
        s.p = p; s.o = o; s.e = e; s.status = status;
        states[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- decode
// Decoder::decode_next (back.rs:677-706) for stream blockIdx.x, whole symbols while fewer than `need` bytes are there, until slice_in
// more bytes of stream are read or slice_out more bytes of text made.  The last 65 536 bytes of text live in the ring (of twice that
// size: a copy's writes then never land on a slot another lane still has to read) and travel between launches through `spill`;
// bytes behind cap are counted and not written.
__global__ __launch_bounds__(kZbThreads) void k_zb_decode(const ZbStream *__restrict__ streams, ZbState *__restrict__ states, uint8_t *__restrict__ spill,
                                                          uint64_t slice_in, uint64_t slice_out) {
    extern __shared__ uint32_t zb_lds[];
    uint8_t *ring = reinterpret_cast<uint8_t *>(zb_lds);
    uint8_t *stg = ring + kZbRing;
    const ZbState s0 = states[blockIdx.x];
    if (s0.status != kZbRunning) return;
    const uint8_t *__restrict__ in = streams[blockIdx.x].in;
    uint8_t *out = streams[blockIdx.x].out;
    const uint64_t n = streams[blockIdx.x].n, cap = streams[blockIdx.x].cap, need = streams[blockIdx.x].need;
    uint8_t *mine = spill + (uint64_t)blockIdx.x * 65536;
    uint64_t sp = s0.p, o = s0.o;
    uint32_t status = kZbRunning;
    for (uint64_t pos = (o > 65536 ? o - 65536 : 0) + threadIdx.x; pos < o; pos += kZbThreads) ring[pos & kZbMask] = mine[pos & 65535];
    uint64_t base = sp, end = min(n, sp + kZbStage);
    for (uint64_t i = base + threadIdx.x; i < end; i += kZbThreads) stg[i - base] = in[i];
    __syncthreads();
    const uint64_t stop_in = sp + slice_in, stop_out = o + slice_out;
    while (sp < stop_in && o < stop_out) {
        if (o >= need || sp + 2 > n) { status = kZbDone; break; }   // enough, or no header (Len::deserialize is None, :92)
        if (sp + 4 > end && end < n) {   // the header and what may follow it, staged
            __syncthreads();
            base = sp;
            end = min(n, sp + kZbStage);
            for (uint64_t i = base + threadIdx.x; i < end; i += kZbThreads) stg[i - base] = in[i];
            __syncthreads();
        }
        const uint32_t head = stg[sp - base] | ((uint32_t)stg[sp - base + 1] << 8), len = head & kZbMaxLen;
        uint32_t k;
        if (head & 0x8000u) {
            if (sp + 4 > n) { status = kZbDone; break; }   // Back::deserialize is None (:101)
            const uint32_t back = stg[sp - base + 2] | ((uint32_t)stg[sp - base + 3] << 8);
            if (back > o) { status = kZbBadLookback; break; }   // lookback_pos underflows (:466)
            k = min(len, back);   // the source ends where the history does (:473-478)
            for (uint32_t i = threadIdx.x; i < k; i += kZbThreads) {
                const uint8_t b = ring[(o - back + i) & kZbMask];
                ring[(o + i) & kZbMask] = b;
                if (o + i < cap) out[o + i] = b;
            }
            sp += 4;
        } else {
            if (sp + 2 + len > n) { status = kZbBadExplicit; break; }   // assert!(data.len() == len) (:97)
            k = len;
            const uint64_t src = sp + 2;
            for (uint32_t done = 0; done < k;) {
                if (src + done >= end) {
                    __syncthreads();
                    base = src + done;
                    end = min(n, base + kZbStage);
                    for (uint64_t i = base + threadIdx.x; i < end; i += kZbThreads) stg[i - base] = in[i];
                    __syncthreads();
                }
                const uint32_t m = (uint32_t)min((uint64_t)(k - done), end - (src + done));
                for (uint32_t i = threadIdx.x; i < m; i += kZbThreads) {
                    const uint8_t b = stg[src + done + i - base];
                    ring[(o + done + i) & kZbMask] = b;
                    if (o + done + i < cap) out[o + done + i] = b;
                }
                done += m;
            }
            sp += 2 + len;
        }
        o += k;
        __syncthreads();   // the next symbol may copy what this one wrote
        if (!k) { status = kZbDone; break; }   // a symbol that brings no byte: Decoder::next answers None (:657-664)
    }
    if (status == kZbRunning)
        for (uint64_t pos = (o > 65536 ? o - 65536 : 0) + threadIdx.x; pos < o; pos += kZbThreads) mine[pos & 65535] = ring[pos & kZbMask];
    if (threadIdx.x == 0) {
        ZbState s;
        s.p = sp; s.o = o; s.e = 0; s.status = status;
        states[blockIdx.x] = s;
    }
}

// the launches of one call: until every stream's record says it is over
template <class Launch> int zb_run(Ctx *c, const char *stage, const ZbStream *streams_h, uint32_t F, ZbState *states_h, uint64_t max_launches, DevBuf *streams_d,
                                   DevBuf *states_d, Launch launch) {
    CNIIC_HIP_TRY(c, streams_d->alloc((uint64_t)F * sizeof(ZbStream)));
    CNIIC_HIP_TRY(c, states_d->alloc((uint64_t)F * sizeof(ZbState)));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(streams_d->p, streams_h, (uint64_t)F * sizeof(ZbStream), hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemsetAsync(states_d->p, 0, (uint64_t)F * sizeof(ZbState), c->stream));
    ScopedKernelTimer timer(c, stage);
    uint64_t launches = 0;
    for (bool running = true; running;) {
        if (launches++ > max_launches) return c->fail(CNIIC_ERR_HIP, "zip-back: %s did not end within %llu launches", stage, (unsigned long long)max_launches);
        launch();
        CNIIC_HIP_TRY(c, hipGetLastError());
        CNIIC_HIP_TRY(c, hipMemcpyAsync(states_h, states_d->p, (uint64_t)F * sizeof(ZbState), hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        running = false;
        for (uint32_t f = 0; f < F; f++) running |= states_h[f].status == kZbRunning;
    }
    timer.stop(launches);
    return CNIIC_OK;
}

// a launch's slice: CNIIC_TEST_ZB_SLICE (testing build) puts the boundaries where the tests want them
uint64_t zb_slice(uint64_t dflt) {
    const char *e = test_env("CNIIC_TEST_ZB_SLICE");
    const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
    return v ? v : dflt;
}

int zb_set_lds(Ctx *c) {
    static bool done = false;   // (function attributes are per process)
    if (done) return CNIIC_OK;
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_zb_encode), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZbRing));
    CNIIC_HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_zb_decode), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kZbDecLds));
    done = true;
    return CNIIC_OK;
}

}  // namespace

int zb_encode_streams(Ctx *c, const ZbStream *streams_h, uint32_t F, ZbState *states_h) {
    if (!F) return CNIIC_OK;
    CNIIC_TRY(zb_set_lds(c));
    const uint64_t slice = zb_slice(kZbEncodeSlice);
    uint64_t longest = 0;
    for (uint32_t f = 0; f < F; f++) longest = std::max(longest, streams_h[f].n);
    DevBuf streams_d, states_d;
    return zb_run(c, "zb_encode", streams_h, F, states_h, longest / slice + 4, &streams_d, &states_d, [&] {
        hipLaunchKernelGGL(k_zb_encode, dim3(F), dim3(kZbThreads), kZbRing, c->stream, streams_d.as<ZbStream>(), states_d.as<ZbState>(), slice);
    });
}

int zb_decode_streams(Ctx *c, const ZbStream *streams_h, uint32_t F, ZbState *states_h) {
    if (!F) return CNIIC_OK;
    CNIIC_TRY(zb_set_lds(c));
    const uint64_t slice = zb_slice(kZbDecodeSlice);
    uint64_t launches = 4;
    for (uint32_t f = 0; f < F; f++) {   // a launch ends a stream or takes it a slice further, on one side or the other
        const uint64_t text = std::min(streams_h[f].need, zb_text_bound(streams_h[f].n));
        launches = std::max(launches, streams_h[f].n / slice + text / slice + 4);
    }
    DevBuf streams_d, states_d, spill;
    CNIIC_HIP_TRY(c, spill.alloc((uint64_t)F * 65536));
    return zb_run(c, "zb_decode", streams_h, F, states_h, launches, &streams_d, &states_d, [&] {
        hipLaunchKernelGGL(k_zb_decode, dim3(F), dim3(kZbThreads), kZbDecLds, c->stream, streams_d.as<ZbStream>(), states_d.as<ZbState>(), spill.as<uint8_t>(),
                           slice, slice);
    });
}

}  // namespace cniic
