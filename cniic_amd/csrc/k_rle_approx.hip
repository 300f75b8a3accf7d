// k_rle_approx.hip -- Hilbert { compress: RLE(d != 0) } on gfx950: run-length coding along the Hilbert scan where a pixel joins
// the open run while its distance to the run's running average is <= d (reference: src/codec/hilbertc.rs:118-155, rle_approx +
// Approx + RunningAvg :200-299).  The records are the exact codec's (count:u8, colour as u64 len = 3 + 3 bytes), with the colour
// round(sum / count) per channel.
//
// The reference walks the image once.  A run has at most RepCount::MAX = 255 elements, so the run that WOULD start at position i
// depends on px[i .. i + 255) alone: its length L(i) is computed for every i at once.  The true run starts are then the chain
// 0, L(0), L(0) + L(L(0)), ...; it is resolved without a walk over the image:
//
//   k_rla_len_maps  a block per 256 positions (a "piece"): L(i) for its 256 starts from a 511-pixel window in LDS (u8 out), then
//                   p -> p + L(p) pointer-doubled 8 times in LDS: for every entry offset e (0..254: a run covers at most 255
//                   positions) the offset in the next piece at which the chain from e enters it.  That is the piece's map, 256 u8.
//   k_rla_compose   maps composed in groups of 64 (upsweep; repeated until at most 64 are left)
//   k_rla_down      the entry offset of every group, then of every element in it (downsweep; the top level starts at offset 0)
//   k_rla_flags     a block per 4096 positions (16 pieces): the starts reachable from each piece's entry, by doubling again --
//                   with the jump tables of 1, 2, ..., 128 steps kept, R <- R u jump_k(R) for k = 7..0 marks every start in 8
//                   rounds -- written in k_rle.hip's layout (a u16 per 16 positions) + runs per 4096 positions
//   rle_offsets     (k_rle.hip) exclusive sum of the runs per chunk
//   k_rla_records   k_rle_records with the run's average for colour
//
// Every step is bounded: L(i) takes at most 254 tests, the doubling 8 rounds, the scan log_64 of the pieces.
//
// Exactness.  The test (Approx::accept, :224-238) is computed as the reference does, in IEEE f64:
//   avg_c = sum_c / count (RunningAvg::avg_f64, :271-274); dist = sqrt((0 + (avg_0 - x_0)^2 + (avg_1 - x_1)^2) + (avg_2 - x_2)^2)
//   (Distance::dist, :292-299); accept iff dist <= d.
//   - the sums are integers < 2^16 and the count < 2^8: their conversions to double are exact, and so is the integer sum kept here
//     in place of the reference's f64 sum (every partial sum of small integers is exact in f64);
//   - the division is IEEE double division (correctly rounded; no fast-math, no reciprocal);
//   - the squares and the adds must not fuse: `#pragma clang fp contract(off)` in rla_accept (hipcc's HIP default is
//     -ffp-contract=fast-honor-pragmas);
//   - "0 + a" is dropped: a square is never -0, so 0.0 + a == a bit for bit;
//   - no square root on the device: sqrt_rn is monotone, so sqrt_rn(s) <= d  <=>  s <= T(d), T(d) the largest double whose
//     correctly rounded root is <= d (found on the host, rla_threshold; -1 for d < 0 or NaN, +inf for +inf).
// The record colour round(sum / count) (RunningAvg::avg, :276-285: f64::round, halves away from zero) is taken in integers:
// floor((2 sum + count) / (2 count)).  The f64 quotient cannot round onto or across a half: a quotient that is not a half lies at
// least 1 / (2 * 255) from one, far above its rounding error.
#include <cmath>

#include "common.hpp"
#include "device_utils.hpp"
#include "rle_small.hpp"   // rla_accept, the threshold and the modes, shared with the small-frame route

namespace cniic {

constexpr int kRlaThreads = 256;
constexpr uint32_t kRlaPiece = 256;                       // positions per map
constexpr uint32_t kRlaMaxRun = 255;                      // RepCount::MAX (hilbertc.rs:23,130)
constexpr uint32_t kRlaWindow = kRlaPiece + kRlaMaxRun;   // 511: the pixels the runs of a piece's starts can cover
constexpr uint32_t kRlaGroup = 64;                        // maps per composition
constexpr uint32_t kRlaChunk = 4096;                      // k_rle.hip's flag chunk: 256 threads x 16 positions
constexpr uint32_t kRlaPieces = kRlaChunk / kRlaPiece;    // 16

// mode: 0 = the test (T >= 0), 1 = nothing is accepted (T < 0: d < 0 or NaN), 2 = everything is (T >= 3 * 255^2: no distance
// reaches it -- avg_c and x_c lie in [0, 255], so each rounded square is <= 65025 and their rounded sum <= 195075)
__global__ __launch_bounds__(kRlaThreads) void k_rla_len_maps(const uint8_t *__restrict__ lin, uint64_t n, double T, int mode,
                                                              uint8_t *__restrict__ L, uint8_t *__restrict__ maps) {
    __shared__ uint32_t s_key[kRlaWindow + 1];
    __shared__ uint32_t s_diff[(kRlaWindow + 1) / 32];   // bit q: key[q] != key[q - 1]
    __shared__ uint16_t s_nx[kRlaPiece];
    const uint64_t p0 = (uint64_t)blockIdx.x * kRlaPiece;
    const uint32_t t = threadIdx.x;
    const uint64_t i = p0 + t;
    uint32_t len = 1;
    if (mode == 0) {
        for (uint32_t q = t; q < kRlaWindow; q += kRlaThreads) s_key[q] = p0 + q < n ? rgb_key(lin + 3 * (p0 + q)) : 0u;
        __syncthreads();
        if (t < (kRlaWindow + 1) / 32) {
            uint32_t m = 0;
            for (uint32_t b = 0; b < 32; b++) {
                const uint32_t q = t * 32 + b;
                if (q > 0 && q < kRlaWindow && s_key[q] != s_key[q - 1]) m |= 1u << b;
            }
            s_diff[t] = m;
        }
        __syncthreads();
        if (i < n) {
            const uint32_t lim = (uint32_t)min<uint64_t>(kRlaMaxRun, n - i);   // the cap, or the end of the stream
            // the pixels equal to px[i] that follow it keep the average at px[i]: distance 0, accepted (d >= 0).  The first that
            // differs is the next set bit of s_diff after t.
            uint32_t e = lim;
            for (uint32_t q = t + 1; q < t + lim;) {
                const uint32_t word = s_diff[q >> 5] >> (q & 31);
                if (word) { e = min(lim, q + (uint32_t)(__ffs((int)word) - 1) - t); break; }
                q = (q | 31) + 1;
            }
            len = e;
            if (e < lim) {
                const uint32_t k0 = s_key[t];
                uint32_t s0 = ((k0 >> 16) & 255u) * e, s1 = ((k0 >> 8) & 255u) * e, s2 = (k0 & 255u) * e;
                while (len < lim) {
                    const uint32_t x = s_key[t + len];
                    if (!rla_accept(s0, s1, s2, len, x, T)) break;
                    s0 += (x >> 16) & 255u; s1 += (x >> 8) & 255u; s2 += x & 255u;
                    len++;
                }
            }
        }
    } else if (mode == 2 && i < n) {
        len = (uint32_t)min<uint64_t>(kRlaMaxRun, n - i);
    }
    if (i < n) L[i] = (uint8_t)len;
    // the piece's map: p -> p + L(p), doubled 8 times (every step moves on by >= 1, so 256 steps leave the piece; positions past
    // the piece stay where they are)
    uint32_t nx = t + len;
    s_nx[t] = (uint16_t)nx;
    __syncthreads();
    for (int r = 0; r < 8; r++) {
        if (nx < kRlaPiece) nx = s_nx[nx];
        __syncthreads();
        s_nx[t] = (uint16_t)nx;
        __syncthreads();
    }
    maps[(size_t)blockIdx.x * kRlaPiece + t] = (uint8_t)(nx - kRlaPiece);   // <= 254
}

// out[g] = in[64 g + 63] o ... o in[64 g]: every entry offset e followed through the group's maps
__global__ __launch_bounds__(kRlaThreads) void k_rla_compose(const uint8_t *__restrict__ in, uint32_t m, uint8_t *__restrict__ out) {
    __shared__ uint8_t s_map[kRlaGroup][kRlaPiece];
    const uint32_t g0 = blockIdx.x * kRlaGroup, cnt = min(kRlaGroup, m - g0);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(in + (size_t)g0 * kRlaPiece);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&s_map[0][0]);
    for (uint32_t k = threadIdx.x; k < cnt * (kRlaPiece / 4); k += kRlaThreads) dst[k] = src[k];
    __syncthreads();
    uint32_t v = threadIdx.x;
    for (uint32_t k = 0; k < cnt; k++) v = s_map[k][v];
    out[(size_t)blockIdx.x * kRlaPiece + threadIdx.x] = (uint8_t)v;
}

// ent[64 g + k] = the entry offset of element 64 g + k: the group's own entry (parent[g], or 0 at the top) through the maps before it
__global__ __launch_bounds__(kRlaThreads) void k_rla_down(const uint8_t *__restrict__ in, uint32_t m, const uint8_t *__restrict__ parent,
                                                          uint8_t *__restrict__ ent) {
    __shared__ uint8_t s_map[kRlaGroup][kRlaPiece];
    __shared__ uint8_t s_ent[kRlaGroup];
    const uint32_t g0 = blockIdx.x * kRlaGroup, cnt = min(kRlaGroup, m - g0);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(in + (size_t)g0 * kRlaPiece);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&s_map[0][0]);
    for (uint32_t k = threadIdx.x; k < cnt * (kRlaPiece / 4); k += kRlaThreads) dst[k] = src[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t v = parent ? parent[blockIdx.x] : 0u;
        for (uint32_t k = 0; k < cnt; k++) { s_ent[k] = (uint8_t)v; v = s_map[k][v]; }
    }
    __syncthreads();
    if (threadIdx.x < cnt) ent[g0 + threadIdx.x] = s_ent[threadIdx.x];
}

// The run starts of 4096 positions (16 pieces; thread t holds position t of every piece) from the pieces' entries.  jump_k(p) =
// the start 2^k runs after p, 0 once it leaves the piece (no position jumps to 0).  With R = {entry}, R <- R u jump_k(R) for
// k = 7 .. 0 gives every start the entry reaches in fewer than 256 runs, i.e. all of the piece's.  A mark set early inside a round
// only marks more starts of the same chain, so the rounds mark in place.
__global__ __launch_bounds__(kRlaThreads) void k_rla_flags(const uint8_t *__restrict__ L, uint64_t n, const uint8_t *__restrict__ ent,
                                                           uint16_t *__restrict__ flags, uint32_t *__restrict__ chunk_runs) {
    __shared__ uint8_t s_jump[8][kRlaChunk];
    __shared__ uint16_t s_nx[kRlaChunk];
    __shared__ uint8_t s_mark[kRlaChunk];
    const uint64_t c0 = (uint64_t)blockIdx.x * kRlaChunk;
    const uint32_t t = threadIdx.x;
    uint32_t nx[kRlaPieces];
#pragma unroll
    for (uint32_t s = 0; s < kRlaPieces; s++) {
        const uint32_t q = s * kRlaPiece + t;
        nx[s] = t + (c0 + q < n ? (uint32_t)L[c0 + q] : 1u);
        s_nx[q] = (uint16_t)nx[s];
        s_mark[q] = 0;
    }
    __syncthreads();
    for (int k = 0; k < 8; k++) {
#pragma unroll
        for (uint32_t s = 0; s < kRlaPieces; s++) {
            s_jump[k][s * kRlaPiece + t] = nx[s] < kRlaPiece ? (uint8_t)nx[s] : (uint8_t)0;
            if (nx[s] < kRlaPiece) nx[s] = s_nx[s * kRlaPiece + nx[s]];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < kRlaPieces; s++) s_nx[s * kRlaPiece + t] = (uint16_t)nx[s];
        __syncthreads();
    }
    if (t < kRlaPieces && c0 + (uint64_t)t * kRlaPiece < n) {
        const uint64_t piece = blockIdx.x * (uint64_t)kRlaPieces + t;
        s_mark[t * kRlaPiece + ent[piece]] = 1;
    }
    __syncthreads();
    for (int k = 7; k >= 0; k--) {
#pragma unroll
        for (uint32_t s = 0; s < kRlaPieces; s++) {
            const uint32_t q = s * kRlaPiece + t;
            const uint32_t j = s_jump[k][q];
            if (s_mark[q] && j) s_mark[s * kRlaPiece + j] = 1;
        }
        __syncthreads();
    }
    // k_rle.hip's layout: thread t's u16 holds positions 16 t .. 16 t + 15 of the chunk
    uint32_t f = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++)
        if (c0 + 16 * t + j < n && s_mark[16 * t + j]) f |= 1u << j;
    flags[(size_t)blockIdx.x * kRlaThreads + t] = (uint16_t)f;
    const uint32_t runs = block_reduce_sum<kRlaThreads>((uint32_t)__popc(f));
    if (t == 0) chunk_runs[blockIdx.x] = runs;
}

// k_rle_records with the run's average for colour: a run ends where the next flag is (a later bit of the thread's own flags, else
// the first bit of one of the next 16 threads' -- a run has at most 255 elements -- else the end of the image)
// record = count:u8 | len:u64 = 3 | r g b  = 12 bytes = words { count | 3 << 8, 0, r << 8 | g << 16 | b << 24 }
__global__ __launch_bounds__(kRlaThreads) void k_rla_records(const uint8_t *__restrict__ lin, uint64_t n, const uint16_t *__restrict__ flags,
                                                             const uint64_t *__restrict__ run_off, uint32_t nchunks, uint32_t *__restrict__ out_words) {
    __shared__ uint32_t wsum[kRlaThreads / 64];
    __shared__ uint16_t s_f[kRlaThreads + 16];
    __shared__ uint32_t s_rec[3 * kRlaChunk];
    __shared__ uint32_t s_total;
    const uint32_t f = flags[(size_t)blockIdx.x * kRlaThreads + threadIdx.x];
    s_f[threadIdx.x] = (uint16_t)f;
    if (threadIdx.x < 16) s_f[kRlaThreads + threadIdx.x] = blockIdx.x + 1 < nchunks ? flags[(size_t)(blockIdx.x + 1) * kRlaThreads + threadIdx.x] : (uint16_t)0;
    const uint32_t mine = (uint32_t)__popc(f);
    uint32_t r = block_exclusive_scan<kRlaThreads>(mine, wsum);  // (its barriers also complete s_f)
    if (threadIdx.x == kRlaThreads - 1) s_total = r + mine;
    if (f) {
        const uint64_t base = (uint64_t)blockIdx.x * kRlaChunk + (uint64_t)threadIdx.x * 16;
        uint64_t after = n;
        for (uint32_t k = 1; k <= 16; k++) {
            const uint32_t g = s_f[threadIdx.x + k];
            if (g) { after = base + (uint64_t)k * 16 + (uint32_t)(__ffs((int)g) - 1); break; }
        }
        if (after > n) after = n;
        for (uint32_t m = f; m; r++) {
            const uint32_t j = (uint32_t)(__ffs((int)m) - 1);
            m &= m - 1;
            const uint64_t s = base + j, e = m ? base + (uint32_t)(__ffs((int)m) - 1) : after;
            const uint32_t cnt = (uint32_t)(e - s);
            uint32_t s0 = 0, s1 = 0, s2 = 0;
            for (const uint8_t *p = lin + 3 * s, *pe = lin + 3 * e; p < pe; p += 3) { s0 += p[0]; s1 += p[1]; s2 += p[2]; }
            const uint32_t r0 = (2 * s0 + cnt) / (2 * cnt), r1 = (2 * s1 + cnt) / (2 * cnt), r2 = (2 * s2 + cnt) / (2 * cnt);
            s_rec[3 * r] = cnt | (3u << 8);
            s_rec[3 * r + 1] = 0u;
            s_rec[3 * r + 2] = (r0 << 8) | (r1 << 16) | (r2 << 24);
        }
    }
    __syncthreads();
    uint32_t *o = out_words + 3 * run_off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < 3 * s_total; i += kRlaThreads) o[i] = s_rec[i];
}

// T(d) (rle_small.hpp): the largest double whose correctly rounded square root is <= d; -1 for d < 0 or NaN
double rla_threshold(double d) { return rla_threshold_of(d); }

// The scan of the maps: level 0 = the pieces' maps, level l + 1 = level l's in groups of 64, up to a level of <= 64; then every
// group's entry offset down the levels again.  (k_zipdict.hip chains its parse through the same maps.)
int rla_chain_entries(Ctx *c, const uint8_t *maps0_d, uint32_t npieces, RlaLevels *keep, const uint8_t **ent0_d) {
    std::vector<uint32_t> cnt{npieces};
    while (cnt.back() > kRlaGroup) cnt.push_back((uint32_t)ceil_div(cnt.back(), kRlaGroup));
    keep->maps.resize(cnt.size());
    keep->ent.resize(cnt.size());
    std::vector<const uint8_t *> maps(cnt.size(), maps0_d);
    for (size_t l = 0; l < cnt.size(); l++) {
        if (l) { CNIIC_HIP_TRY(c, keep->maps[l].alloc((uint64_t)cnt[l] * kRlaPiece)); maps[l] = keep->maps[l].as<uint8_t>(); }
        CNIIC_HIP_TRY(c, keep->ent[l].alloc(cnt[l]));
    }
    for (size_t l = 0; l + 1 < cnt.size(); l++)
        hipLaunchKernelGGL(k_rla_compose, dim3(cnt[l + 1]), dim3(kRlaThreads), 0, c->stream, maps[l], cnt[l], keep->maps[l + 1].as<uint8_t>());
    for (size_t l = cnt.size(); l-- > 0;)
        hipLaunchKernelGGL(k_rla_down, dim3((uint32_t)ceil_div(cnt[l], kRlaGroup)), dim3(kRlaThreads), 0, c->stream, maps[l], cnt[l],
                           l + 1 < cnt.size() ? (const uint8_t *)keep->ent[l + 1].as<uint8_t>() : (const uint8_t *)nullptr, keep->ent[l].as<uint8_t>());
    CNIIC_HIP_TRY(c, hipGetLastError());
    *ent0_d = keep->ent[0].as<uint8_t>();
    return CNIIC_OK;
}

int rle_approx_plan(Ctx *c, const uint8_t *lin_d, uint64_t n, double d, RlePlan *plan) {
    plan->n = n;
    plan->nruns = 0;
    if (n == 0) return CNIIC_OK;
    const uint64_t nchunks64 = ceil_div(n, kRlaChunk);
    if (nchunks64 > 0x7fffffffull) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert-rle-approx: image too large");
    const uint32_t nchunks = (uint32_t)nchunks64;
    const uint32_t npieces = (uint32_t)ceil_div(n, kRlaPiece);
    plan->nchunks = nchunks;
    const double T = rla_threshold(d);
    const int mode = rla_mode(T);
    DevBuf L, maps0, chunk_runs, tot;
    RlaLevels levels;
    CNIIC_HIP_TRY(c, L.alloc(n));
    CNIIC_HIP_TRY(c, maps0.alloc((uint64_t)npieces * kRlaPiece));
    CNIIC_HIP_TRY(c, chunk_runs.alloc((uint64_t)nchunks * 4));
    CNIIC_HIP_TRY(c, tot.alloc(8));
    CNIIC_HIP_TRY(c, plan->flags.alloc((uint64_t)nchunks * kRlaThreads * 2));
    CNIIC_HIP_TRY(c, plan->run_off.alloc((uint64_t)nchunks * 8));
    hipLaunchKernelGGL(k_rla_len_maps, dim3(npieces), dim3(kRlaThreads), 0, c->stream, lin_d, n, T, mode, L.as<uint8_t>(), maps0.as<uint8_t>());
    const uint8_t *ent0 = nullptr;
    CNIIC_TRY(rla_chain_entries(c, maps0.as<uint8_t>(), npieces, &levels, &ent0));
    hipLaunchKernelGGL(k_rla_flags, dim3(nchunks), dim3(kRlaThreads), 0, c->stream, (const uint8_t *)L.as<uint8_t>(), n, ent0,
                       plan->flags.as<uint16_t>(), chunk_runs.as<uint32_t>());
    CNIIC_TRY(rle_offsets(c, chunk_runs.as<uint32_t>(), nchunks, plan->run_off.as<uint64_t>(), tot.as<uint64_t>()));
    CNIIC_HIP_TRY(c, hipGetLastError());
    uint64_t total = 0;
    CNIIC_HIP_TRY(c, hipMemcpyAsync(&total, tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    plan->nruns = total;
    return CNIIC_OK;
}

int rle_approx_emit(Ctx *c, const uint8_t *lin_d, const RlePlan *plan, uint32_t *out_words_d) {
    if (plan->nruns == 0) return CNIIC_OK;
    hipLaunchKernelGGL(k_rla_records, dim3(plan->nchunks), dim3(kRlaThreads), 0, c->stream, lin_d, plan->n, (const uint16_t *)plan->flags.as<uint16_t>(),
                       (const uint64_t *)plan->run_off.as<uint64_t>(), plan->nchunks, out_words_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    return CNIIC_OK;
}

}  // namespace cniic
