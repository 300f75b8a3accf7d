// k_surface.hip -- pitched surfaces <-> packed RGB24 frames (cniic_frames_from_surfaces / cniic_frames_to_surfaces):
//   k_surf_import    L8 / LA8 / RGB8 / RGBA8 / BGR8 / BGRA8 / NV12 surfaces -> rgb + img_off[f]   (the reference's px.to_rgb())
//   k_surf_export    rgb + img_off[f] -> RGB8 / BGR8 / RGBA8 / BGRA8 surfaces, the pitch's padding left alone
// One launch for all frames, after k_sqerr_var (k_misc.hip): the packed side of every frame is cut into chunks (kSurfChunkPx pixels, so
// that a chunk starts on a pixel), the chunks of all frames are numbered through by a host-built table and dealt in contiguous runs --
// here to the WAVES of a bounded grid, not to its blocks: a chunk is worked row piece by row piece, and a row of a video frame is a
// few kilobytes, which is work for 64 lanes and not for 256.  A wave finds its first frame by one binary search and walks on.  There
// is no LDS and no barrier.
// A row piece (surf_index.hpp): head pixels in byte stores until the WRITTEN address is a multiple of 16, then groups of 16 pixels
// whose 48 or 64 written bytes are three or four aligned 16-byte stores, then a tail of fewer than 16 pixels.  The READ side of a
// group sits at an alignment of its own: it is fetched as the aligned 16-byte words that hold its bytes and shifted together with
// v_alignbit_b32.  No load touches a 16-byte word that holds no byte of the run it fetches (the last row of a surface may end its
// allocation), and no store touches a byte outside the row's pixels.
// NV12 goes the same way, row by row: a group fetches its 16 Y bytes and the 16 or 18 bytes of the 8 or 9 chroma pairs above them.
// (Each chroma row is therefore fetched for both of its pixel rows; the second time it comes from the L2.)
#include "common.hpp"
#include "device_utils.hpp"
#include "surf_index.hpp"

namespace cniic {

// shifts the `nbytes` bytes that start m bytes into the aligned words at `base` down to d[0 ...]; NDW dwords are made, of which the
// ones behind nbytes are not meaningful.  m, nbytes: the same for every lane of the wave (the branches are scalar).
template <int NDW>
__device__ __forceinline__ void surf_fetch(const uint4 *__restrict__ base, uint32_t m, uint32_t nbytes, uint32_t (&d)[NDW]) {
    constexpr int NW = (15 + 4 * NDW + 15) / 16;   // the words that 4 NDW bytes can lie in: 4 NW >= NDW + 4
    uint32_t w[4 * NW];
#pragma unroll
    for (int i = 0; i < NW; i++) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (surf_word_wanted((uint32_t)i, m, nbytes)) v = base[i];
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    const uint32_t q = m >> 2, r = (m & 3) * 8;
    if (q & 1) {
#pragma unroll
        for (int j = 0; j < 4 * NW - 1; j++) w[j] = w[j + 1];
    }
    if (q & 2) {
#pragma unroll
        for (int j = 0; j < 4 * NW - 2; j++) w[j] = w[j + 2];
    }
#pragma unroll
    for (int j = 0; j < NDW; j++) d[j] = __builtin_amdgcn_alignbit(w[j + 1], w[j], r);
}

// Which read byte a written byte is: pixels of IB bytes in, OB bytes out.  KIND 0: channels in order, 1: the ends swapped (BGR),
// 2: every channel the first byte (grey).  A fourth written byte is the alpha (-1).
template <int IB, int OB, int KIND>
__device__ __forceinline__ constexpr int surf_src_of(int j) {
    const int p = j / OB, ch = j % OB;
    return ch == 3 ? -1 : KIND == 2 ? p * IB : p * IB + (KIND == 1 ? 2 - ch : ch);
}

template <int IB, int OB, int KIND>
__device__ __forceinline__ void surf_px(const uint8_t *__restrict__ s, uint8_t *__restrict__ o, uint32_t alpha) {
    uint8_t v[OB];
#pragma unroll
    for (int ch = 0; ch < OB; ch++) v[ch] = ch == 3 ? (uint8_t)alpha : s[surf_src_of<IB, OB, KIND>(ch)];
#pragma unroll
    for (int ch = 0; ch < OB; ch++) o[ch] = v[ch];
}

// n pixels, contiguous on both sides: s -> o
template <int IB, int OB, int KIND>
__device__ __forceinline__ void surf_piece(const uint8_t *__restrict__ s, uint8_t *__restrict__ o, uint32_t n, uint32_t alpha, uint32_t lane) {
    const SurfSplit sp = surf_split((uint64_t)reinterpret_cast<uintptr_t>(o), n, OB);
    for (uint32_t i = lane; i < sp.head; i += 64) surf_px<IB, OB, KIND>(s + (uint64_t)i * IB, o + (uint64_t)i * OB, alpha);
    if (lane >= 32 && lane - 32 < sp.tail) {   // (tail < 16: other lanes than a short head's)
        const uint32_t i = sp.head + kSurfGroupPx * sp.groups + (lane - 32);
        surf_px<IB, OB, KIND>(s + (uint64_t)i * IB, o + (uint64_t)i * OB, alpha);
    }
    if (!sp.groups) return;
    s += (uint64_t)sp.head * IB;
    o += (uint64_t)sp.head * OB;
    const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15);   // (a group is 16 IB bytes on: every group has this m)
    const uint8_t *sa = s - m;
    for (uint32_t g = lane; g < sp.groups; g += 64) {
        uint32_t a[4 * IB];
        surf_fetch<4 * IB>(reinterpret_cast<const uint4 *>(sa + (uint64_t)g * (16 * IB)), m, 16 * IB, a);
        uint32_t v[4 * OB];
#pragma unroll
        for (int d = 0; d < 4 * OB; d++) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int from = surf_src_of<IB, OB, KIND>(4 * d + b);
                const uint32_t byte = from < 0 ? alpha : (a[from >> 2] >> (8 * (from & 3))) & 255u;
                x |= byte << (8 * b);
            }
            v[d] = x;
        }
        uint4 *po = reinterpret_cast<uint4 *>(o + (uint64_t)g * (16 * OB));
#pragma unroll
        for (int k = 0; k < OB; k++) po[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
}

// ---------------------------------------------------------------- NV12
// The integer matrices of include/cniic_hip.h: C = Y - ysub, D = U - 128, E = V - 128,
// R = (cy C + rv E + 128) >> 8, G = (cy C + gu D + gv E + 128) >> 8, B = (cy C + bu D + 128) >> 8 (arithmetic shifts: floors), clipped.
struct SurfYuv { int ysub, cy, rv, gu, gv, bu; };
__device__ __forceinline__ SurfYuv surf_yuv(int32_t matrix) {
    switch (matrix) {
        case CNIIC_YUV_601_LIMITED: return {16, 298, 409, -100, -208, 516};
        case CNIIC_YUV_709_LIMITED: return {16, 298, 459, -55, -136, 541};
        case CNIIC_YUV_601_FULL:    return {0, 256, 359, -88, -183, 454};
        default:                    return {0, 256, 403, -48, -120, 475};   // CNIIC_YUV_709_FULL (the host has refused everything else)
    }
}
__device__ __forceinline__ uint32_t surf_clip8(int v) { return (uint32_t)min(max(v, 0), 255); }
// -> r | g << 8 | b << 16
__device__ __forceinline__ uint32_t surf_yuv_px(const SurfYuv &k, int y, int re, int ge, int be) {
    const int yy = k.cy * (y - k.ysub) + 128;
    return surf_clip8((yy + re) >> 8) | surf_clip8((yy + ge) >> 8) << 8 | surf_clip8((yy + be) >> 8) << 16;
}

// n pixels of one row from column x on: sy = their Y bytes, suv = the START of the row's UV row
__device__ __forceinline__ void surf_piece_nv12(const uint8_t *__restrict__ sy, const uint8_t *__restrict__ suv, uint32_t x, uint8_t *__restrict__ o,
                                                uint32_t n, const SurfYuv k, uint32_t lane) {
    const SurfSplit sp = surf_split((uint64_t)reinterpret_cast<uintptr_t>(o), n, 3);
    auto one = [&](uint32_t i) {
        const uint8_t *uv = suv + surf_uv_begin(x + i);
        const int d = (int)uv[0] - 128, e = (int)uv[1] - 128;
        const uint32_t p = surf_yuv_px(k, sy[i], k.rv * e, k.gu * d + k.gv * e, k.bu * d);
        uint8_t *q = o + (uint64_t)i * 3;
        q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8); q[2] = (uint8_t)(p >> 16);
    };
    for (uint32_t i = lane; i < sp.head; i += 64) one(i);
    if (lane >= 32 && lane - 32 < sp.tail) one(sp.head + kSurfGroupPx * sp.groups + (lane - 32));
    if (!sp.groups) return;
    const uint32_t xs = x + sp.head;          // a group starts 16 pixels on: every group has this parity and these alignments
    const bool odd = xs & 1;                  // an odd start: the group's 16 pixels lie under 9 chroma pairs, not 8
    const uint32_t uv_bytes = surf_uv_bytes(xs, kSurfGroupPx);
    sy += sp.head;
    suv += surf_uv_begin(xs);
    o += (uint64_t)sp.head * 3;
    const uint32_t my = (uint32_t)(reinterpret_cast<uintptr_t>(sy) & 15), muv = (uint32_t)(reinterpret_cast<uintptr_t>(suv) & 15);
    const uint8_t *ya = sy - my, *uva = suv - muv;
    for (uint32_t g = lane; g < sp.groups; g += 64) {
        uint32_t yw[4], cw[5];
        surf_fetch<4>(reinterpret_cast<const uint4 *>(ya + (uint64_t)g * 16), my, 16, yw);
        surf_fetch<5>(reinterpret_cast<const uint4 *>(uva + (uint64_t)g * 16), muv, uv_bytes, cw);
        int re[9], ge[9], be[9];
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const uint32_t pr = cw[j >> 1] >> (16 * (j & 1));
            const int d = (int)(pr & 255u) - 128, e = (int)((pr >> 8) & 255u) - 128;
            re[j] = k.rv * e; ge[j] = k.gu * d + k.gv * e; be[j] = k.bu * d;
        }
        uint32_t px[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int y = (int)((yw[i >> 2] >> (8 * (i & 3))) & 255u);
            const int je = i >> 1, jo = (i + 1) >> 1;
            px[i] = surf_yuv_px(k, y, odd ? re[jo] : re[je], odd ? ge[jo] : ge[je], odd ? be[jo] : be[je]);
        }
        uint4 *po = reinterpret_cast<uint4 *>(o + (uint64_t)g * 48);
#pragma unroll
        for (int t = 0; t < 3; t++) {   // pixels 4 t + (0, 1 | 1, 2 | 2, 3 | ...) -> 12 packed bytes per four pixels
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int d = 4 * t + u, a = d / 3 * 4 + d % 3;   // dword d of the 12 holds the end of pixel a and the start of pixel a + 1
                v[u] = d % 3 == 0 ? px[a] | px[a + 1] << 24 : d % 3 == 1 ? px[a] >> 8 | px[a + 1] << 16 : px[a] >> 16 | px[a + 1] << 8;
            }
            po[t] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}

// ---------------------------------------------------------------- the kernels
// The walk both kernels share: this wave's run of chunks, frame by frame, row piece by row piece.  body(F, piece) with everything in
// it the same for all lanes of the wave.
template <class Body>
__device__ __forceinline__ void surf_walk(const SurfFrame *__restrict__ fr, const uint32_t *__restrict__ first /* [frames + 1] */, uint32_t frames,
                                          uint32_t nchunks, Body body) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + wave, nw = (uint64_t)gridDim.x * 4;
    const uint32_t per = (uint32_t)(((uint64_t)nchunks + nw - 1) / nw);
    const uint32_t c0 = (uint32_t)min(gw * per, (uint64_t)nchunks), c1 = (uint32_t)min((uint64_t)c0 + per, (uint64_t)nchunks);
    if (c0 >= c1) return;
    // the frame of chunk c0: the LAST f with first[f] <= c0 (every frame has a pixel, so every frame has a chunk)
    uint32_t f = 0;
    for (uint32_t hi = frames; hi - f > 1;) {   // first[f] <= c0 < first[hi]
        const uint32_t mid = f + (hi - f) / 2;
        if (first[mid] <= c0) f = mid; else hi = mid;
    }
    for (uint32_t c = c0; c < c1; c++) {
        while (c >= first[f + 1]) f++;
        const SurfFrame F = fr[f];
        const uint32_t npx = F.w * F.h, p = (c - first[f]) * kSurfChunkPx;   // (w h < 2^32)
        uint32_t left = surf_min_u32(kSurfChunkPx, npx - p);
        SurfPiece pc = surf_piece_first(p, p + left, F.w);
        do body(F, pc); while (surf_piece_next(pc, left, F.w));
    }
}

__global__ __launch_bounds__(256) void k_surf_import(const uint8_t *__restrict__ src, uint8_t *__restrict__ rgb, const SurfFrame *__restrict__ fr,
                                                     const uint32_t *__restrict__ first, uint32_t frames, uint32_t nchunks) {
    const uint32_t lane = threadIdx.x & 63;
    surf_walk(fr, first, frames, nchunks, [&](const SurfFrame &F, const SurfPiece &pc) {
        uint8_t *o = rgb + F.rgb_off + ((uint64_t)pc.y * F.w + pc.x) * 3;
        const uint8_t *s = src + F.off + (uint64_t)pc.y * F.pitch;
        switch (F.format) {
            case CNIIC_PX_L8:    surf_piece<1, 3, 2>(s + pc.x, o, pc.n, 0, lane); break;
            case CNIIC_PX_LA8:   surf_piece<2, 3, 2>(s + (uint64_t)pc.x * 2, o, pc.n, 0, lane); break;
            case CNIIC_PX_RGB8:  surf_piece<3, 3, 0>(s + (uint64_t)pc.x * 3, o, pc.n, 0, lane); break;
            case CNIIC_PX_RGBA8: surf_piece<4, 3, 0>(s + (uint64_t)pc.x * 4, o, pc.n, 0, lane); break;
            case CNIIC_PX_BGR8:  surf_piece<3, 3, 1>(s + (uint64_t)pc.x * 3, o, pc.n, 0, lane); break;
            case CNIIC_PX_BGRA8: surf_piece<4, 3, 1>(s + (uint64_t)pc.x * 4, o, pc.n, 0, lane); break;
            case CNIIC_PX_NV12:
                surf_piece_nv12(s + pc.x, src + F.off_uv + (uint64_t)(pc.y >> 1) * F.pitch_uv, pc.x, o, pc.n, surf_yuv(F.matrix), lane);
                break;
            default: break;   // (the host has refused it)
        }
    });
}

__global__ __launch_bounds__(256) void k_surf_export(const uint8_t *__restrict__ rgb, uint8_t *__restrict__ dst, const SurfFrame *__restrict__ fr,
                                                     const uint32_t *__restrict__ first, uint32_t frames, uint32_t nchunks, uint32_t alpha) {
    const uint32_t lane = threadIdx.x & 63;
    surf_walk(fr, first, frames, nchunks, [&](const SurfFrame &F, const SurfPiece &pc) {
        const uint8_t *s = rgb + F.rgb_off + ((uint64_t)pc.y * F.w + pc.x) * 3;
        uint8_t *o = dst + F.off + (uint64_t)pc.y * F.pitch;
        switch (F.format) {
            case CNIIC_PX_RGB8:  surf_piece<3, 3, 0>(s, o + (uint64_t)pc.x * 3, pc.n, alpha, lane); break;
            case CNIIC_PX_BGR8:  surf_piece<3, 3, 1>(s, o + (uint64_t)pc.x * 3, pc.n, alpha, lane); break;
            case CNIIC_PX_RGBA8: surf_piece<3, 4, 0>(s, o + (uint64_t)pc.x * 4, pc.n, alpha, lane); break;
            case CNIIC_PX_BGRA8: surf_piece<3, 4, 1>(s, o + (uint64_t)pc.x * 4, pc.n, alpha, lane); break;
            default: break;   // (the host has refused it)
        }
    });
}

// fr_h: `frames` validated frames (every one has a pixel; cniic_surface_span's rules), offsets from in_d / out_d
int surf_convert(Ctx *c, bool to_surfaces, const uint8_t *in_d, uint8_t *out_d, const SurfFrame *fr_h, uint32_t frames, uint32_t alpha) {
    std::vector<uint32_t> first((size_t)frames + 1);
    uint64_t nchunks = 0;
    for (uint32_t f = 0; f < frames; f++) {
        first[f] = (uint32_t)nchunks;
        nchunks += surf_chunks((uint64_t)fr_h[f].w * fr_h[f].h);
        if (nchunks > 0xffffffffull) return c->fail(CNIIC_ERR_BAD_ARG, "surfaces: too many pixels in one call");
    }
    first[frames] = (uint32_t)nchunks;
    // one block of scratch: the frames | the chunk table
    const uint64_t off_first = sizeof(SurfFrame) * (uint64_t)frames;
    DevBuf buf;
    CNIIC_HIP_TRY(c, buf.alloc(off_first + 4ull * (frames + 1)));
    uint8_t *p = buf.as<uint8_t>();
    CNIIC_HIP_TRY(c, hipMemcpyAsync(p, fr_h, off_first, hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(p + off_first, first.data(), 4ull * (frames + 1), hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, c->surf_ev.ensure(hipEventDisableTiming));
    CNIIC_HIP_TRY(c, hipEventRecord(c->surf_ev, c->stream));
    const SurfFrame *fr_d = reinterpret_cast<const SurfFrame *>(p);
    const uint32_t *first_d = reinterpret_cast<const uint32_t *>(p + off_first);
    const dim3 grid((uint32_t)std::min<uint64_t>(ceil_div(nchunks, 4), 256 * 8));
    ScopedKernelTimer t(c, to_surfaces ? "surf_export" : "surf_import");
    if (to_surfaces) hipLaunchKernelGGL(k_surf_export, grid, dim3(256), 0, c->stream, in_d, out_d, fr_d, first_d, frames, (uint32_t)nchunks, alpha);
    else hipLaunchKernelGGL(k_surf_import, grid, dim3(256), 0, c->stream, in_d, out_d, fr_d, first_d, frames, (uint32_t)nchunks);
    CNIIC_HIP_TRY(c, hipGetLastError());
    t.stop(1);
    // the kernel may still run when the call returns (device memory on both sides), but fr_h and first go away with it: the copies above
    // must have read them
    CNIIC_HIP_TRY(c, hipEventSynchronize(c->surf_ev));
    return CNIIC_OK;
}

}  // namespace cniic
