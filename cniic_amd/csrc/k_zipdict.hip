// k_zipdict.hip -- the dictionary coder of zip(dict) (reference: src/zip/dict.rs) on gfx950, from the moment its dictionary is full.
//
// The coder hands out u16 symbols, one per emitted pair; after 0xFFFE the dictionary never changes again (Abbrev::next, dict.rs:280-290).
// Up to there the coder is a serial walk and runs on the host (zipdict.cpp).  From there on:
//
// encode: a greedy longest-match parse of the rest of the text against a read-only trie.
//   k_zd_match   a lane per text position: the longest entry that starts there (length >= 1, its symbol), by DictEncoder::find_symbol's
//                walk (dict.rs:96-136) through the trie's edges, an open-addressed table (node, byte) -> (child, symbol) in HBM
//                (about 3 10^5 edges for a photograph: 8 MB at half load -- L2 / MALL, not LDS)
//   the chain    the parse starts are 0, L(0), L(0) + L(L(0)), ... from the hand-over position.
//     windowed   when the longest entry has at most 255 bytes: k_rle_approx.hip's route -- k_zd_maps turns every 256 positions into a
//                map (entry offset -> entry offset of the next piece, by pointer doubling in LDS), rla_chain_entries scans the maps,
//                k_zd_marks follows every piece from its entry, a lane per piece
//     hybrid     otherwise (a flat stretch of the image made an entry of thousands of bytes), zd_chain.hpp: the pieces that hold a
//                length above 255 -- the BREAK pieces, k_zd_break_flags + rle_offsets number them -- keep their exits wide (k_zd_maps_wide),
//                the other pieces' maps are scanned as above, k_zd_break_table carries every (break, entry) through the kept levels
//                of that scan to the next break piece, k_zd_break_walk follows the table (one lane, one step per break piece the parse
//                enters), k_zd_break_patch turns every entered break into a constant map and the pieces its jump flies over into
//                identities that k_zd_marks skips, and the maps are scanned again.  No break piece in the tail: the windowed kernels alone.
//     plain      more break pieces than kZcMaxBreaks (the side tables: 1.5 KiB each): k_zd_walk, one block that follows the chain
//                through windows of 4096 lengths staged in LDS.  Merely correct: one lane walks.
//   compaction   k_zd_count / rle_offsets / k_zd_emit: the symbols at the marked positions, in order, as u16; 0xFFFF behind an
//                odd number of them (next_pair's (symbol1, ZIP_SPECIAL_EOF), dict.rs:81-86)
//
// decode: every symbol's text is a slice of the text the fill phase decoded (the place where the pair that created it stood), which the
// host writes first.  Behind it: k_zd_dec_sums (lengths per 2048 symbols), k_zd_dec_scan (their exclusive sums), k_zd_dec_copy (a wave
// per 64 symbols, one placed copy each).  Once the dictionary is full every u16 is a symbol that has been handed out (0xFFFF is the
// empty text), so nothing in this phase can be malformed; lengths are summed saturating, and no byte is written at or behind `limit`.
//
// Positions are 64-bit throughout: 8 + 11 w h passes 2^32 from w h = 3.9 10^8 on.
#include "common.hpp"
#include "device_utils.hpp"
#include "zd_chain.hpp"

namespace cniic {

constexpr int kZdThreads = 256;
constexpr uint32_t kZdPiece = 256;                  // positions per map (kRlaPiece)
constexpr uint32_t kZdPer = 16;                     // positions per thread of the compaction
constexpr uint32_t kZdChunk = kZdThreads * kZdPer;  // 4096
constexpr uint32_t kZdDecPer = 8;                   // symbols per thread of the decoder's sums
constexpr uint32_t kZdDecChunk = kZdThreads * kZdDecPer;
static_assert(kZdPiece == kZcPiece && kZdThreads == (int)kZcPiece && kZcMaxEntry == kZdMaxEntry && kZcMaxBreaks < (1u << 24), "zd_chain.hpp restates these");

// ---------------------------------------------------------------- the 11-byte records (ser.rs:164-172,210-214)
// text = [w h as u32 LE when dims] then per pixel: u64 LE 3, r, g, b.  A lane per text byte.
__global__ __launch_bounds__(kZdThreads) void k_zd_serialize(const uint8_t *__restrict__ px, uint64_t nbytes, uint32_t head, uint32_t w, uint32_t h,
                                                             uint8_t *__restrict__ text) {
    const uint64_t i = (uint64_t)blockIdx.x * kZdThreads + threadIdx.x;
    if (i >= nbytes) return;
    if (i < head) { text[i] = (uint8_t)((i < 4 ? w : h) >> (8 * (i & 3))); return; }
    const uint64_t r = i - head, p = r / 11;
    const uint32_t k = (uint32_t)(r - p * 11);
    text[i] = k == 0 ? (uint8_t)3 : k < 8 ? (uint8_t)0 : px[3 * p + (k - 8)];
}

// records -> pixels; *first_bad = the first record whose length is not 3 (atomicMin; the caller starts it at npx)
__global__ __launch_bounds__(kZdThreads) void k_zd_unserialize(const uint8_t *__restrict__ rec, uint64_t npx, uint8_t *__restrict__ px,
                                                               unsigned long long *__restrict__ first_bad) {
    const uint64_t p = (uint64_t)blockIdx.x * kZdThreads + threadIdx.x;
    if (p >= npx) return;
    const uint8_t *q = rec + 11 * p;
    uint32_t rest = 0;
#pragma unroll
    for (int k = 1; k < 8; k++) rest |= q[k];
    if (q[0] != 3 || rest) atomicMin(first_bad, (unsigned long long)p);
    px[3 * p] = q[8]; px[3 * p + 1] = q[9]; px[3 * p + 2] = q[10];
}

// ---------------------------------------------------------------- encode: match
__global__ __launch_bounds__(kZdThreads) void k_zd_match(const uint8_t *__restrict__ text, uint64_t N, uint64_t P0, const uint4 *__restrict__ tab,
                                                         uint32_t bits, uint32_t *__restrict__ len, uint16_t *__restrict__ sym) {
    const uint64_t r = (uint64_t)blockIdx.x * kZdThreads + threadIdx.x, i = P0 + r;
    if (i >= N) return;
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t node = 0, best = 0, best_sym = 0;
    for (uint64_t j = i; j < N; j++) {
        const uint32_t key = (node << 8) | text[j];
        uint32_t h = zd_hash(key, bits);
        uint4 e = tab[h];
        while (e.x != key && e.x != kZdEmpty) { h = (h + 1) & mask; e = tab[h]; }   // (the table is at most half full)
        if (e.x != key) break;
        if (e.z != kZdNoSym) { best = (uint32_t)(j + 1 - i); best_sym = e.z; }
        if (!e.y) break;
        node = e.y;
    }
    len[r] = best;   // >= 1: every single byte has a symbol
    sym[r] = (uint16_t)best_sym;
}

// ---------------------------------------------------------------- encode: the chain, windowed
// a piece's map: p -> p + L(p) doubled 8 times (every step moves on by >= 1); positions behind the text count as steps of 1
__global__ __launch_bounds__(kZdThreads) void k_zd_maps(const uint32_t *__restrict__ len, uint64_t M, uint8_t *__restrict__ maps) {
    __shared__ uint16_t s_nx[kZdPiece];
    const uint32_t t = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * kZdPiece + t;
    uint32_t nx = t + (r < M ? len[r] : 1u);   // len <= 255 on this route
    s_nx[t] = (uint16_t)nx;
    __syncthreads();
    for (int k = 0; k < 8; k++) {
        if (nx < kZdPiece) nx = s_nx[nx];
        __syncthreads();
        s_nx[t] = (uint16_t)nx;
        __syncthreads();
    }
    maps[(size_t)blockIdx.x * kZdPiece + t] = (uint8_t)(nx - kZdPiece);   // <= 254
}

// a lane per piece: the parse starts it holds, from its entry (skip: the pieces a long match flies over, or null)
__global__ __launch_bounds__(kZdThreads) void k_zd_marks(const uint32_t *__restrict__ len, uint64_t M, const uint8_t *__restrict__ ent, uint32_t npieces,
                                                         const uint8_t *__restrict__ skip, uint8_t *__restrict__ mark) {
    const uint32_t piece = blockIdx.x * kZdThreads + threadIdx.x;
    if (piece >= npieces) return;
    if (skip && skip[piece]) return;
    const uint64_t base = (uint64_t)piece * kZdPiece;
    for (uint32_t p = ent[piece]; p < kZdPiece && base + p < M;) {
        mark[base + p] = 1;
        p += len[base + p];
    }
}

// ---------------------------------------------------------------- encode: the chain, hybrid (zd_chain.hpp)
// a wave per piece: does it hold a length above 255?
__global__ __launch_bounds__(kZdThreads) void k_zd_break_flags(const uint32_t *__restrict__ len, uint64_t M, uint32_t npieces, uint32_t *__restrict__ flags) {
    const uint32_t piece = blockIdx.x * (kZdThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (piece >= npieces) return;   // (whole waves)
    const uint64_t base = (uint64_t)piece * kZdPiece;
    bool any = false;
#pragma unroll
    for (uint32_t k = 0; k < kZdPiece / 64; k++) {
        const uint64_t r = base + 64 * k + lane;
        if (r < M) any |= zc_is_break(len[r]);
    }
    const bool brk = __ballot(any) != 0;
    if (lane == 0) flags[piece] = brk ? 1u : 0u;
}

// k_zd_maps with any length: a break piece (number before[piece]) writes its 256 exits as u16 -- one 512-byte row -- and a dummy map
__global__ __launch_bounds__(kZdThreads) void k_zd_maps_wide(const uint32_t *__restrict__ len, uint64_t M, const uint32_t *__restrict__ flags,
                                                             const uint64_t *__restrict__ before, uint8_t *__restrict__ maps,
                                                             uint16_t *__restrict__ exits, uint32_t *__restrict__ brk_piece) {
    __shared__ uint16_t s_nx[kZdPiece];
    const uint32_t t = threadIdx.x;
    const uint64_t r = (uint64_t)blockIdx.x * kZdPiece + t;
    uint32_t nx = zc_exit_first(t, r < M, r < M ? len[r] : 1u);   // <= 255 + 32768
    s_nx[t] = (uint16_t)nx;
    __syncthreads();
    for (int k = 0; k < kZcRounds; k++) {
        nx = zc_exit_round(nx, s_nx);
        __syncthreads();
        s_nx[t] = (uint16_t)nx;
        __syncthreads();
    }
    if (flags[blockIdx.x]) {
        const uint64_t b = before[blockIdx.x];
        maps[(size_t)blockIdx.x * kZdPiece + t] = 0;
        exits[b * kZdPiece + t] = (uint16_t)nx;
        if (t == 0) brk_piece[b] = blockIdx.x;
    } else {
        maps[(size_t)blockIdx.x * kZdPiece + t] = (uint8_t)(nx - kZdPiece);   // <= 254
    }
}

// a lane per (break, entry): the next break piece that chain stands in, and its entry there.  All lanes are independent; each is a
// chain of dependent one-byte loads (zc_range: at most 128 per level), so the grid is what hides them.
__global__ __launch_bounds__(kZdThreads) void k_zd_break_table(ZcLevels lv, const uint16_t *__restrict__ exits, const uint32_t *__restrict__ brk_piece,
                                                               const uint64_t *__restrict__ before, uint32_t npieces, uint64_t M, uint32_t B, uint32_t *__restrict__ table) {
    const size_t at = (size_t)blockIdx.x * kZdPiece + threadIdx.x;
    table[at] = zc_table_entry(lv, brk_piece[blockIdx.x], exits[at], npieces, M, before, brk_piece, B);
}

// one lane: the break pieces the parse enters and its entry offset in each.  Every step moves to a later break, and the loop has B steps.
__global__ __launch_bounds__(64) void k_zd_break_walk(ZcLevels lv, const uint32_t *__restrict__ table, const uint32_t *__restrict__ brk_piece,
                                                      const uint64_t *__restrict__ before, uint32_t npieces, uint64_t M, uint32_t B, uint8_t *__restrict__ entered,
                                                      uint8_t *__restrict__ entry, uint32_t *__restrict__ count) {
    if (threadIdx.x) return;
    uint32_t st = zc_next_break(lv, 0, 0, npieces, M, before, brk_piece, B), n = 0;
    for (uint32_t step = 0; step < B && st != kZcEnd; step++) {
        const uint32_t b = zc_brk(st), e = zc_entry(st);
        if (b >= B) break;
        entered[b] = 1;
        entry[b] = (uint8_t)e;
        n++;
        st = zc_walk_next(table[(size_t)b * kZdPiece + e], b, B);
    }
    *count = n;
}

// a block per break piece that was entered: its map becomes the constant of its landing, the pieces flown over the identity (and `skip`)
__global__ __launch_bounds__(kZdThreads) void k_zd_break_patch(const uint16_t *__restrict__ exits, const uint32_t *__restrict__ brk_piece,
                                                               const uint8_t *__restrict__ entered, const uint8_t *__restrict__ entry, uint32_t npieces,
                                                               uint8_t *__restrict__ maps, uint8_t *__restrict__ skip) {
    if (!entered[blockIdx.x]) return;
    const uint32_t j = brk_piece[blockIdx.x], t = threadIdx.x;
    if (j >= npieces) return;
    const uint32_t x = exits[(size_t)blockIdx.x * kZdPiece + entry[blockIdx.x]];
    maps[(size_t)j * kZdPiece + t] = zc_patch_map(true, x, t);
    for (uint32_t p = j + 1, end = zc_flown_end(j, x, npieces); p < end; p++) {   // (< 129 pieces)
        maps[(size_t)p * kZdPiece + t] = zc_patch_map(false, x, t);
        if (t == 0) skip[p] = 1;
    }
}

// ---------------------------------------------------------------- encode: the chain, plain
// One block follows the chain through windows of 4096 positions: the window's lengths come to LDS in one coalesced read, lane 0 walks
// them there (an LDS read per symbol, not a trip to HBM) and the marks go out in whole lines.  A match that ends behind the window
// starts the next window where it ends.
__global__ __launch_bounds__(kZdThreads) void k_zd_walk(const uint32_t *__restrict__ len, uint64_t M, uint8_t *__restrict__ mark) {
    __shared__ uint32_t s_len[kZdChunk];
    __shared__ uint8_t s_mark[kZdChunk];
    __shared__ uint64_t s_next;
    for (uint64_t base = 0; base < M;) {
        const uint32_t cnt = (uint32_t)min<uint64_t>(kZdChunk, M - base);
        for (uint32_t i = threadIdx.x; i < cnt; i += kZdThreads) { s_len[i] = len[base + i]; s_mark[i] = 0; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t q = 0;
            while (q < cnt) { s_mark[q] = 1; q += s_len[q]; }
            s_next = base + q;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += kZdThreads) mark[base + i] = s_mark[i];
        base = s_next;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- encode: compaction (mark: zero-padded to whole chunks)
__device__ __forceinline__ uint32_t zd_mark_bits(const uint8_t *mark) {   // 16 marks (0 / 1 bytes, 16-byte aligned) -> 16 bits
    const uint4 q = *reinterpret_cast<const uint4 *>(mark);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) f |= (((w[k] & 0x01010101u) * 0x01020408u) >> 24 & 15u) << (4 * k);
    return f;
}

__global__ __launch_bounds__(kZdThreads) void k_zd_count(const uint8_t *__restrict__ mark, uint32_t *__restrict__ chunk_syms) {
    const uint32_t f = zd_mark_bits(mark + (size_t)blockIdx.x * kZdChunk + (size_t)threadIdx.x * kZdPer);
    const uint32_t n = block_reduce_sum<kZdThreads>((uint32_t)__popc(f));
    if (threadIdx.x == 0) chunk_syms[blockIdx.x] = n;
}

__global__ __launch_bounds__(kZdThreads) void k_zd_emit(const uint8_t *__restrict__ mark, const uint16_t *__restrict__ sym, const uint64_t *__restrict__ chunk_off,
                                                        uint64_t total, uint16_t *__restrict__ out) {
    __shared__ uint32_t wsum[kZdThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kZdChunk + (uint64_t)threadIdx.x * kZdPer;
    const uint32_t f = zd_mark_bits(mark + base);
    uint32_t r = block_exclusive_scan<kZdThreads>((uint32_t)__popc(f), wsum);
    uint16_t *o = out + chunk_off[blockIdx.x];
    for (uint32_t m = f; m; m &= m - 1) o[r++] = sym[base + (uint32_t)(__ffs((int)m) - 1)];
    if (blockIdx.x == 0 && threadIdx.x == 0 && (total & 1)) out[total] = (uint16_t)kZdNoSym;
}

// ---------------------------------------------------------------- decode
__device__ __forceinline__ uint32_t zd_sym_at(const uint8_t *syms, uint64_t i) { return (uint32_t)syms[2 * i] | ((uint32_t)syms[2 * i + 1] << 8); }
__device__ __forceinline__ uint64_t zd_sat(uint64_t a) { return a < kZdSat ? a : kZdSat; }

// lengths of 2048 symbols (every table length is <= 2^38, so a chunk's sum stays below 2^49)
__global__ __launch_bounds__(kZdThreads) void k_zd_dec_sums(const uint8_t *__restrict__ syms, uint64_t nsym, const uint64_t *__restrict__ tab_len,
                                                            uint64_t *__restrict__ chunk_sum) {
    __shared__ uint64_t s_w[kZdThreads / 64];
    const uint64_t i0 = ((uint64_t)blockIdx.x * kZdThreads + threadIdx.x) * kZdDecPer;
    uint64_t s = 0;
    for (uint32_t k = 0; k < kZdDecPer; k++)
        if (i0 + k < nsym) s += tab_len[zd_sym_at(syms, i0 + k)];
    s = wave_reduce_sum64(s);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// single block: chunk_off[c] = the saturating sum of the chunks before c; *total = of all
__global__ __launch_bounds__(1024) void k_zd_dec_scan(const uint64_t *__restrict__ chunk_sum, uint32_t nchunks, uint64_t *__restrict__ chunk_off,
                                                      uint64_t *__restrict__ total) {
    __shared__ uint64_t sh[1024];
    const uint32_t per = (nchunks + 1023) / 1024;
    const uint32_t lo = min(threadIdx.x * per, nchunks), hi = min(lo + per, nchunks);
    uint64_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s = zd_sat(s + chunk_sum[i]);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint64_t t = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] = zd_sat(sh[threadIdx.x] + t);
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? sh[threadIdx.x - 1] : 0;
    for (uint32_t i = lo; i < hi; i++) { chunk_off[i] = run; run = zd_sat(run + chunk_sum[i]); }
    if (threadIdx.x == 1023) *total = sh[1023];
}

// a wave per 64 symbols: the text of symbol i goes to out[base + (sum of the lengths before i) ...), as far as it lies below `limit`.
// A symbol below 256 is its byte; any other is out[off, off + len) with off + len <= base (the fill phase's text, written before).
__global__ __launch_bounds__(kZdThreads) void k_zd_dec_copy(const uint8_t *__restrict__ syms, uint64_t nsym, const uint64_t *__restrict__ tab_off,
                                                            const uint64_t *__restrict__ tab_len, const uint64_t *__restrict__ chunk_off, uint64_t base,
                                                            uint8_t *out, uint64_t limit) {
    __shared__ uint64_t s_w[kZdThreads / 64];
    __shared__ uint64_t s_dst[kZdDecChunk], s_src[kZdDecChunk];   // s_src: the offset, or kZdSat | byte for a single byte
    __shared__ uint64_t s_len[kZdDecChunk];                       // (clipped: what is copied)
    const uint64_t i0 = ((uint64_t)blockIdx.x * kZdThreads + threadIdx.x) * kZdDecPer;
    uint64_t l[kZdDecPer], mine = 0;
    uint32_t sv[kZdDecPer];
    for (uint32_t k = 0; k < kZdDecPer; k++) {
        sv[k] = i0 + k < nsym ? zd_sym_at(syms, i0 + k) : kZdNoSym;
        l[k] = i0 + k < nsym ? tab_len[sv[k]] : 0;
        mine += l[k];
    }
    const uint64_t inc = wave_inclusive_scan64<false>(mine);
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint64_t at = zd_sat(zd_sat(base + chunk_off[blockIdx.x]) + (inc - mine));
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) at += s_w[w];
    for (uint32_t k = 0; k < kZdDecPer; k++) {
        const uint32_t q = threadIdx.x * kZdDecPer + k;
        const uint64_t room = at < limit ? limit - at : 0;
        s_dst[q] = at;
        s_len[q] = min(l[k], room);
        s_src[q] = sv[k] < 256 ? (kZdSat | sv[k]) : tab_off[sv[k]];
        at = zd_sat(at + l[k]);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, q0 = (threadIdx.x >> 6) * 64 * kZdDecPer;
    for (uint32_t q = q0; q < q0 + 64 * kZdDecPer; q++) {
        const uint64_t n = s_len[q];
        if (!n) continue;
        const uint64_t src = s_src[q];
        uint8_t *d = out + s_dst[q];
        if (src & kZdSat) { if (lane == 0) d[0] = (uint8_t)src; continue; }
        const uint8_t *s = out + src;
        for (uint64_t b = lane; b < n; b += 64) d[b] = s[b];
    }
}

// ================================================================ host launchers
int zd_serialize(Ctx *c, const uint8_t *px_d, uint64_t npx, bool dims, uint32_t w, uint32_t h, uint8_t *text_d, const char *stage) {
    const uint64_t nbytes = (dims ? 8 : 0) + 11 * npx;
    if (!nbytes) return CNIIC_OK;
    const uint64_t blocks = ceil_div(nbytes, kZdThreads);
    if (blocks > 0x7fffffffull) return c->fail(CNIIC_ERR_BAD_ARG, "zip-dict: image too large");
    ScopedKernelTimer timer(c, stage);
    hipLaunchKernelGGL(k_zd_serialize, dim3((uint32_t)blocks), dim3(kZdThreads), 0, c->stream, px_d, nbytes, dims ? 8u : 0u, w, h, text_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    timer.stop();
    return CNIIC_OK;
}

int zd_unserialize(Ctx *c, const uint8_t *rec_d, uint64_t npx, uint8_t *px_d, uint64_t *first_bad_h, const char *stage) {
    *first_bad_h = npx;
    if (!npx) return CNIIC_OK;
    ScopedKernelTimer timer(c, stage ? stage : "", stage && c->timers);
    DevBuf bad;
    CNIIC_HIP_TRY(c, bad.alloc(8));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(bad.p, first_bad_h, 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_zd_unserialize, dim3((uint32_t)ceil_div(npx, kZdThreads)), dim3(kZdThreads), 0, c->stream, rec_d, npx, px_d,
                       bad.as<unsigned long long>());
    CNIIC_HIP_TRY(c, hipGetLastError());
    CNIIC_HIP_TRY(c, hipMemcpyAsync(first_bad_h, bad.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    timer.stop();
    return CNIIC_OK;
}

// the stages of the hybrid chain as marks of their own (stage timers only): events between the launches, read at the end
struct ZdStageMarks {
    Ctx *c;
    std::vector<std::pair<const char *, hipEvent_t>> ev;
    explicit ZdStageMarks(Ctx *ctx) : c(ctx) { mark(nullptr); }
    ~ZdStageMarks() { for (auto &e : ev) (void)hipEventDestroy(e.second); }
    void mark(const char *ends) {   // `ends`: the stage that ends here
        if (!c->timers) return;
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, c->stream);
        ev.emplace_back(ends, e);
    }
    void finish(const char *whole) {
        if (ev.size() < 2) return;
        (void)hipEventSynchronize(ev.back().second);
        float ms = 0.f;
        for (size_t i = 1; i < ev.size(); i++) {
            if (hipEventElapsedTime(&ms, ev[i - 1].second, ev[i].second) == hipSuccess) c->ktimes[ev[i].first].ms += ms;
            c->ktimes[ev[i].first].launches += 1;
        }
        if (hipEventElapsedTime(&ms, ev.front().second, ev.back().second) == hipSuccess) c->ktimes[whole].ms += ms;
        c->ktimes[whole].launches += 1;
    }
};

static uint32_t zd_max_breaks() {
    uint32_t bound = kZcMaxBreaks;
    if (const char *e = test_env("CNIIC_TEST_ZD_CHAIN_MAX_BREAKS")) bound = (uint32_t)std::min<unsigned long long>(strtoull(e, nullptr, 10), bound);   // (lowers, never raises)
    return bound;
}

// The chain of a text with an entry above 255 bytes, zd_chain.hpp's way.  *ran = false: more break pieces than the bound (or the
// testing library's CNIIC_TEST_ZD_CHAIN=walk), nothing is marked and the caller walks.
static int zd_chain_hybrid(Ctx *c, const uint32_t *len_d, uint64_t M, uint32_t npieces, uint8_t *mark_d, bool *ran) {
    *ran = false;
    if (const char *e = test_env("CNIIC_TEST_ZD_CHAIN")) if (strcmp(e, "walk") == 0) return CNIIC_OK;
    ZdStageMarks stages(c);
    DevBuf flags, before, tot, maps0, exits, brk_piece, table, entered, skip, count;
    RlaLevels levels, levels2;
    CNIIC_HIP_TRY(c, flags.alloc((uint64_t)npieces * 4));
    CNIIC_HIP_TRY(c, before.alloc((uint64_t)npieces * 8));
    CNIIC_HIP_TRY(c, tot.alloc(8));
    hipLaunchKernelGGL(k_zd_break_flags, dim3((uint32_t)ceil_div(npieces, kZdThreads / 64)), dim3(kZdThreads), 0, c->stream, len_d, M, npieces, flags.as<uint32_t>());
    CNIIC_TRY(rle_offsets(c, flags.as<uint32_t>(), npieces, before.as<uint64_t>(), tot.as<uint64_t>()));
    CNIIC_HIP_TRY(c, hipGetLastError());
    uint64_t B64 = 0;
    CNIIC_HIP_TRY(c, hipMemcpyAsync(&B64, tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (B64 > zd_max_breaks()) return CNIIC_OK;
    const uint32_t B = (uint32_t)B64;
    stages.mark("zd_hy_breaks");
    CNIIC_HIP_TRY(c, maps0.alloc((uint64_t)npieces * kZdPiece));
    const uint8_t *ent = nullptr, *skip_d = nullptr;
    uint32_t n_entered = 0;
    if (!B) {   // long entries, none of which matches in the tail: the windowed kernels alone
        hipLaunchKernelGGL(k_zd_maps, dim3(npieces), dim3(kZdThreads), 0, c->stream, len_d, M, maps0.as<uint8_t>());
        stages.mark("zd_hy_maps");
        CNIIC_TRY(rla_chain_entries(c, maps0.as<uint8_t>(), npieces, &levels, &ent));
        stages.mark("zd_hy_scan");
    } else {
        CNIIC_HIP_TRY(c, exits.alloc((uint64_t)B * kZdPiece * 2));
        CNIIC_HIP_TRY(c, table.alloc((uint64_t)B * kZdPiece * 4));
        CNIIC_HIP_TRY(c, brk_piece.alloc((uint64_t)B * 4));
        CNIIC_HIP_TRY(c, entered.alloc((uint64_t)B * 2));   // entered[B], then the entries
        CNIIC_HIP_TRY(c, skip.alloc(npieces));
        CNIIC_HIP_TRY(c, count.alloc(4));
        CNIIC_HIP_TRY(c, hipMemsetAsync(entered.p, 0, (uint64_t)B * 2, c->stream));
        CNIIC_HIP_TRY(c, hipMemsetAsync(skip.p, 0, npieces, c->stream));
        hipLaunchKernelGGL(k_zd_maps_wide, dim3(npieces), dim3(kZdThreads), 0, c->stream, len_d, M, (const uint32_t *)flags.as<uint32_t>(),
                           (const uint64_t *)before.as<uint64_t>(), maps0.as<uint8_t>(), exits.as<uint16_t>(), brk_piece.as<uint32_t>());
        stages.mark("zd_hy_maps");
        CNIIC_TRY(rla_chain_entries(c, maps0.as<uint8_t>(), npieces, &levels, &ent));
        stages.mark("zd_hy_scan");
        ZcLevels lv{};
        lv.n = (uint32_t)levels.maps.size();
        if (lv.n > kZcMaxLevels) return c->fail(CNIIC_ERR_BAD_ARG, "zip-dict: text too long");
        lv.maps[0] = maps0.as<uint8_t>();
        for (uint32_t l = 1; l < lv.n; l++) lv.maps[l] = levels.maps[l].as<uint8_t>();
        hipLaunchKernelGGL(k_zd_break_table, dim3(B), dim3(kZdThreads), 0, c->stream, lv, (const uint16_t *)exits.as<uint16_t>(),
                           (const uint32_t *)brk_piece.as<uint32_t>(), (const uint64_t *)before.as<uint64_t>(), npieces, M, B, table.as<uint32_t>());
        stages.mark("zd_hy_table");
        hipLaunchKernelGGL(k_zd_break_walk, dim3(1), dim3(64), 0, c->stream, lv, (const uint32_t *)table.as<uint32_t>(), (const uint32_t *)brk_piece.as<uint32_t>(),
                           (const uint64_t *)before.as<uint64_t>(), npieces, M, B, entered.as<uint8_t>(), entered.as<uint8_t>() + B, count.as<uint32_t>());
        stages.mark("zd_hy_walk");
        hipLaunchKernelGGL(k_zd_break_patch, dim3(B), dim3(kZdThreads), 0, c->stream, (const uint16_t *)exits.as<uint16_t>(), (const uint32_t *)brk_piece.as<uint32_t>(),
                           (const uint8_t *)entered.as<uint8_t>(), (const uint8_t *)entered.as<uint8_t>() + B, npieces, maps0.as<uint8_t>(), skip.as<uint8_t>());
        CNIIC_TRY(rla_chain_entries(c, maps0.as<uint8_t>(), npieces, &levels2, &ent));
        stages.mark("zd_hy_patch");
        skip_d = skip.as<uint8_t>();
        if (c->timers) CNIIC_HIP_TRY(c, hipMemcpyAsync(&n_entered, count.p, 4, hipMemcpyDeviceToHost, c->stream));
    }
    hipLaunchKernelGGL(k_zd_marks, dim3((uint32_t)ceil_div(npieces, kZdThreads)), dim3(kZdThreads), 0, c->stream, len_d, M, ent, npieces, skip_d, mark_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    stages.mark("zd_hy_marks");
    if (c->timers) {
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        stages.finish("zd_chain_hybrid");
        c->ktimes["zd_chain_breaks"].launches += B;
        c->ktimes["zd_chain_entered"].launches += n_entered;
    }
    *ran = true;
    return CNIIC_OK;
}

int zd_frozen_plan(Ctx *c, const uint8_t *text_d, uint64_t N, uint64_t P0, const ZdEdge *table_h, uint32_t bits, uint64_t max_entry, ZdFrozen *plan) {
    const uint64_t M = N - P0;
    plan->M = M;
    plan->nsyms = 0;
    plan->windowed = max_entry < kZdPiece;
    if (!M) return CNIIC_OK;
    const uint64_t nchunks64 = ceil_div(M, kZdChunk), npieces64 = ceil_div(M, kZdPiece);
    if (npieces64 > 0x7fffffffull) return c->fail(CNIIC_ERR_BAD_ARG, "zip-dict: text too long");
    const uint32_t nchunks = (uint32_t)nchunks64, npieces = (uint32_t)npieces64;
    plan->nchunks = nchunks;
    DevBuf tab, len, chunk_syms, tot, maps0;
    RlaLevels levels;   // (with maps0: held to the end of the call, like rle_approx_plan's)
    CNIIC_HIP_TRY(c, tab.alloc(sizeof(ZdEdge) << bits));
    CNIIC_HIP_TRY(c, len.alloc(M * 4));
    CNIIC_HIP_TRY(c, plan->sym.alloc(M * 2));
    CNIIC_HIP_TRY(c, plan->mark.alloc((uint64_t)nchunks * kZdChunk));
    CNIIC_HIP_TRY(c, chunk_syms.alloc((uint64_t)nchunks * 4));
    CNIIC_HIP_TRY(c, plan->chunk_off.alloc((uint64_t)nchunks * 8));
    CNIIC_HIP_TRY(c, tot.alloc(8));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(tab.p, table_h, sizeof(ZdEdge) << bits, hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemsetAsync(plan->mark.p, 0, (uint64_t)nchunks * kZdChunk, c->stream));
    {
        ScopedKernelTimer timer(c, "zd_match");
        hipLaunchKernelGGL(k_zd_match, dim3(npieces), dim3(kZdThreads), 0, c->stream, text_d, N, P0, (const uint4 *)tab.as<uint4>(), bits, len.as<uint32_t>(),
                           plan->sym.as<uint16_t>());
        CNIIC_HIP_TRY(c, hipGetLastError());
        timer.stop();
    }
    {
        ScopedKernelTimer timer(c, plan->windowed ? "zd_chain" : "zd_chain_plain");
        if (plan->windowed) {
            CNIIC_HIP_TRY(c, maps0.alloc((uint64_t)npieces * kZdPiece));
            hipLaunchKernelGGL(k_zd_maps, dim3(npieces), dim3(kZdThreads), 0, c->stream, (const uint32_t *)len.as<uint32_t>(), M, maps0.as<uint8_t>());
            const uint8_t *ent = nullptr;
            CNIIC_TRY(rla_chain_entries(c, maps0.as<uint8_t>(), npieces, &levels, &ent));
            hipLaunchKernelGGL(k_zd_marks, dim3((uint32_t)ceil_div(npieces, kZdThreads)), dim3(kZdThreads), 0, c->stream, (const uint32_t *)len.as<uint32_t>(), M,
                               ent, npieces, (const uint8_t *)nullptr, plan->mark.as<uint8_t>());
            CNIIC_HIP_TRY(c, hipGetLastError());
        } else {
            bool hybrid = false;
            CNIIC_TRY(zd_chain_hybrid(c, (const uint32_t *)len.as<uint32_t>(), M, npieces, plan->mark.as<uint8_t>(), &hybrid));
            if (!hybrid) {
                hipLaunchKernelGGL(k_zd_walk, dim3(1), dim3(kZdThreads), 0, c->stream, (const uint32_t *)len.as<uint32_t>(), M, plan->mark.as<uint8_t>());
                CNIIC_HIP_TRY(c, hipGetLastError());
            }
        }
        timer.stop();
    }
    ScopedKernelTimer timer(c, "zd_compact");
    hipLaunchKernelGGL(k_zd_count, dim3(nchunks), dim3(kZdThreads), 0, c->stream, (const uint8_t *)plan->mark.as<uint8_t>(), chunk_syms.as<uint32_t>());
    CNIIC_TRY(rle_offsets(c, chunk_syms.as<uint32_t>(), nchunks, plan->chunk_off.as<uint64_t>(), tot.as<uint64_t>()));
    CNIIC_HIP_TRY(c, hipGetLastError());
    CNIIC_HIP_TRY(c, hipMemcpyAsync(&plan->nsyms, tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    timer.stop();
    return CNIIC_OK;
}

int zd_frozen_emit(Ctx *c, const ZdFrozen *plan, uint16_t *out_d) {
    if (!plan->M) return CNIIC_OK;
    ScopedKernelTimer timer(c, "zd_compact");
    hipLaunchKernelGGL(k_zd_emit, dim3(plan->nchunks), dim3(kZdThreads), 0, c->stream, (const uint8_t *)plan->mark.as<uint8_t>(),
                       (const uint16_t *)plan->sym.as<uint16_t>(), (const uint64_t *)plan->chunk_off.as<uint64_t>(), plan->nsyms, out_d);
    CNIIC_HIP_TRY(c, hipGetLastError());
    timer.stop(0);
    return CNIIC_OK;
}

int zd_expand_plan(Ctx *c, const uint8_t *syms_d, uint64_t nsym, const uint64_t *tab_off_h, const uint64_t *tab_len_h, ZdExpand *plan) {
    plan->nsym = nsym;
    plan->total = 0;
    if (!nsym) return CNIIC_OK;
    const uint64_t nchunks64 = ceil_div(nsym, kZdDecChunk);
    if (nchunks64 > 0x7fffffffull) return c->fail(CNIIC_ERR_BAD_ARG, "zip-dict: stream too long");
    plan->nchunks = (uint32_t)nchunks64;
    plan->syms_d = syms_d;
    DevBuf chunk_sum, tot;
    CNIIC_HIP_TRY(c, plan->tab.alloc(2 * 65536 * 8));
    CNIIC_HIP_TRY(c, chunk_sum.alloc((uint64_t)plan->nchunks * 8));
    CNIIC_HIP_TRY(c, plan->chunk_off.alloc((uint64_t)plan->nchunks * 8));
    CNIIC_HIP_TRY(c, tot.alloc(8));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(plan->tab.p, tab_off_h, 65536 * 8, hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(plan->tab.as<uint64_t>() + 65536, tab_len_h, 65536 * 8, hipMemcpyHostToDevice, c->stream));
    ScopedKernelTimer timer(c, "zd_scan");
    hipLaunchKernelGGL(k_zd_dec_sums, dim3(plan->nchunks), dim3(kZdThreads), 0, c->stream, syms_d, nsym, (const uint64_t *)plan->tab.as<uint64_t>() + 65536,
                       chunk_sum.as<uint64_t>());
    hipLaunchKernelGGL(k_zd_dec_scan, dim3(1), dim3(1024), 0, c->stream, (const uint64_t *)chunk_sum.as<uint64_t>(), plan->nchunks, plan->chunk_off.as<uint64_t>(),
                       tot.as<uint64_t>());
    CNIIC_HIP_TRY(c, hipGetLastError());
    CNIIC_HIP_TRY(c, hipMemcpyAsync(&plan->total, tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    timer.stop(2);
    return CNIIC_OK;
}

// out_d[0, base): the fill phase's text; the symbols' texts follow it, cut at `limit` (<= the buffer's size)
int zd_expand_copy(Ctx *c, const ZdExpand *plan, uint64_t base, uint8_t *out_d, uint64_t limit) {
    if (!plan->nsym || limit <= base) return CNIIC_OK;
    ScopedKernelTimer timer(c, "zd_copy");
    hipLaunchKernelGGL(k_zd_dec_copy, dim3(plan->nchunks), dim3(kZdThreads), 0, c->stream, plan->syms_d, plan->nsym, (const uint64_t *)plan->tab.as<uint64_t>(),
                       (const uint64_t *)plan->tab.as<uint64_t>() + 65536, (const uint64_t *)plan->chunk_off.as<uint64_t>(), base, out_d, limit);
    CNIIC_HIP_TRY(c, hipGetLastError());
    timer.stop();
    return CNIIC_OK;
}

}  // namespace cniic
