// kmeans_rgbw.hpp -- what the two K-means-on-colours translation units share (k_kmeans_rgbw.hip: the launch-per-iteration
// kernels, the set-up and the host side; k_kmeans_persist.hip: the whole loop as ONE launch with the points resident in LDS):
// the state, the packed distance key, the exact cube-against-pivot pruning tests and the packed point word.
// (reference: src/kmeans.rs:21-143, 330-416 with Point = ColorCount, src/codec/clusterc.rs:68-114, src/geom.rs:8-24)
#pragma once
#include <cstdlib>
#include <memory>
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "ps_bounds.hpp"

namespace cniic {

constexpr uint32_t kBias = 1u << 18;  // > max |c|^2 = 195075
constexpr int kPPT = 8;               // colours per thread per sweep (brute kernel)
constexpr int kAssignThreads = 256;
constexpr uint32_t kMaxBlocks = 512;
constexpr int kCellWaves = 8;                                 // waves per block (narrow labels); they share the block's cell range
// LDS strips of a wave: the super-cell list (scap) and the cell's candidates (ccap).  K <= 256: half the table and the whole table -- nothing
// can overflow.  Larger K (u16 labels): both capped (round 4; whole-table strips left a block TWO waves at K = 2048, 0.27 ms an iteration against
// 0.07 at K = 1024): a longer list falls back to the table, a longer strip too (the table IS a candidate list: ascending ids, the same records).
__host__ __device__ constexpr uint32_t km_scap(uint32_t K) { return K <= 256 ? (K + 1) / 2 : (K + 1) / 2 < 512u ? (K + 1) / 2 : 512u; }
__host__ __device__ constexpr uint32_t km_ccap(uint32_t K) { return K <= 256 ? K : 256u; }
constexpr uint32_t kCellWavesBig = 12;                        // ... and in the settled part of a run (launch_assign):
constexpr uint32_t kBigBlocksFrom = 10;                       // launches from this one on run in blocks of kCellWavesBig waves
constexpr uint32_t kAggLaunches = 3;                          // launches 1 .. kAggLaunches book their movers round by round
constexpr uint32_t kCellBlocks = 256 * 3;                     // three blocks of kCellWaves per CU: every block resident at once (LDS, K <= 256)
constexpr int kSweep = 4;                  // points per lane per sweep (cells kernel)
// The full schedule's split of the cells into ranges of equal estimated cost: a cell costs its candidate build plus one sweep
// per 256 points (a sweep of 3 points takes as long as one of 256) -- 2 : 1 measured on the headline encode (assign launches
// 1.87 ms with "1024 + points", 1.825 with 512 + 256 per sweep; 384 / 640 / 768 + 256: 1.87 / 1.84 / 1.85).
constexpr uint32_t kCellFixedCost = 512;  // per cell
constexpr uint32_t kCellSweepCost = 256;  // per sweep of 64 x kSweep points

struct KmRgbwState {
    Ctx *c = nullptr;
    uint64_t U = 0, lo = 0, hi = 0, seed = 0, max_iters = 0;
    uint32_t K = 0, Kpad = 0, idbits = 8, nblocks = 1;
    bool wide = false;   // u16 labels
    bool big = false;    // K > 2048: k_rgbw_assign_big (k_kmeans_wide.hip)
    bool cells = true;   // cell-pruned assign (default) vs brute force
    bool profile = false; // per-launch event timing of the assign kernel (CNIIC_KM_PROFILE)
    bool no_skip = false; // CNIIC_KM_NO_SKIP: always run the full schedule (A/B measurement)
    const uint32_t *keys = nullptr, *weight = nullptr;  // device, canonical order [0,U)
    DevBuf labels;       // canonical-order labels of [lo,hi) (brute path) / cell-major labels of [0,U) (cells path)
    DevBuf cconst, slabs, partials_own, dstate, cent, members_last, wsum_last;  // the last four are views into resblk
    DevBuf arena;        // every zero-initialised buffer of the state in one allocation (resblk, partials_own, running, fused_*, moved_list are views)
    DevBuf resblk;       // [KmDevState | cent u32[K] | members u64[K] | wsum u64[K]]: one copy brings the result to the host
    uint64_t res_cent = 0, res_members = 0, res_wsum = 0, res_bytes = 0;
    std::unique_ptr<LaggedPoll> lagged;  // cniic_cc_poll_lagged
    DevBuf ckeys, cweight, crank, cell_start, running, ne_cell, ne_start, ne_cost, ne_count, wfirst;
    DevBuf cell_rec, moved_list;  // skip schedule state
    uint32_t wfirst_waves = 0;    // != 0: wfirst has not been computed yet for this many waves (ensure_wave_ranges)
    GIdx gidx{nullptr, nullptr, 0};  // several GPUs: the points are this rank's share of gidx.U colours
    DevBuf fused_partials, fused_running, fused_cent;  // km_rgbw_run with the update folded into the assign launches (3 / 2 / 2 buffers)
    bool fused = false;
    cniic_kmeans_stats run_stats{};  // the statistics km_rgbw_run ended on
    bool run_stats_valid = false;
    uint32_t max_skip = 64;  // (= kMaxMovedSkip) skip schedule when at most this many centroids moved (CNIIC_KM_MAXSKIP)
    long fail_at = -1;           // fault injection for the multi-rank tests (CNIIC_TEST_FAIL_AT_LAUNCH), read once as well
    uint32_t shard = 0, nshards = 1;
    uint64_t *partials = nullptr;  // device: 5K+2 words (per-iteration sums or deltas)
    // the loop as ONE launch (k_kmeans_persist.hip): K <= 256, one shard, no communicator
    bool ps = false, ps_tried = false;
    bool ps_pending = false;     // the persistent launch is in the stream and nobody has looked at how it ended yet (km_rgbw_run with may_defer): km_rgbw_result_end does
    std::shared_ptr<void> ps_hold;   // the CUs promised to that launch, given back when the verdict is in (or the state goes)
    uint32_t ps_blocks = 0;
    DevBuf ps_arena;             // [PsBar | 3 x kPsPartWords sums | PsDev | chunk boundaries] (kPsArena*, below)
    DevBuf ps_pk;                // packed words of the points that do not fit their block's LDS
    uint64_t ps_o_part = 0, ps_o_fail = 0, ps_o_rng = 0;
    uint32_t ps_budget = 0;      // bytes of dynamic LDS the block ranges were made for
    bool started = false;        // an assign has been enqueued (or the persistent launch): too late for km_rgbw_set_centroids
    DevBuf given;                // km_rgbw_set_centroids: the caller's K centroids as 0xRRGGBB words, and the host copy the upload reads
    std::vector<uint32_t> given_h;
    // ckeys / cweight / labels have not been written: the persistent launch reads the staged colours of lazy_plan (PsDevPtrs::sbin), and
    // whoever else wants the arrays asks km_rgbw_need_arrays first (the classic loop after a launch that gave up, above all)
    const SpPlan *lazy_plan = nullptr;
    // U (and gidx.U) is still the upper bound the state was created with: the count lies at count_dev and the host has not looked.  The
    // persistent launch reads it there; km_rgbw_set_points ends this (cc_finish, where the count's copy arrives -- or, before the loop of
    // launches, km_rgbw_fetch_points)
    const uint64_t *count_dev = nullptr;
    bool ps_done = false;        // the persistent launch ran to its end: labels holds the result
};

// ---- k_kmeans_persist.hip: the LDS of a block and what the launch shares with its set-up
constexpr uint32_t kPsChunks = 24;                      // chunks of the cell list a block owns (interleaved with the other blocks').  24 by measurement (16 / 20 / 24 / 28 / 32 / 48 on
                                                        // six images, profiles/r05_persist_chunks_probe.txt: finer chunks spread a moved centroid's dirty cells over more blocks; beyond ~28 a block's
                                                        // cells lie in more super-cells than it has shared lists)
constexpr uint32_t kPsSlotsMax = 32;                    // shared super-cell lists of a block (cells of further super-cells build from the table)
constexpr uint32_t kPsScap = 96;                        // members a shared list holds (a longer list: its cells build from the table)
constexpr uint32_t kPsRecWords = 11;                    // a cell's record: pivot colour, common label | pivot id << 16 | candidates << 24 | kRecComplete, 8 mask words, four candidate ids
constexpr uint32_t kPsMaxCells = 2048;                  // cells a block may own (two per thread of its set-up)
constexpr uint32_t kPsOffCell = 5 * 256 * 8 + 256 * 8 + kPsSlotsMax * kPsScap * 4;   // accumulators, table, the shared lists (id << 24 | colour)
constexpr uint32_t kPsDynBytes = 160 * 1024 - 3072;     // the launch's dynamic LDS (the kernel's static variables take the rest)
constexpr uint32_t kPsRunWords = 5 * 256;               // u64 running sums of the clusters (K <= 256): the top of the dynamic LDS, behind ...
constexpr uint32_t kPsBudget = kPsDynBytes - kPsRunWords * 8;   // ... what the block ranges are made for and a block's cells and points may take (the tests shrink it)
constexpr uint32_t kPsPartWords = 5 * 256 + 8;          // u64 words of one buffer of sums (5K + 2, padded)
// per cell (C rounded up to a multiple of 4): first point u32 (own numbering; + 4 words), first point u32 (cell-major), record, id u16, work list u16, list slot u8
__host__ __device__ constexpr uint32_t ps_cell_bytes(uint32_t C) { return 16u + ((C + 3u) & ~3u) * (4u + 4u + kPsRecWords * 4u + 2u + 2u + 1u); }
static_assert(kPsOffCell + ps_cell_bytes(kPsMaxCells) <= kPsBudget, "a full block's descriptors fit the budget");
struct alignas(128) PsLine { uint32_t v; uint32_t pad[31]; };
struct PsBar { PsLine xcount[8], xgen[8], xblocks[8], top, topgen, count, gen, abort_; };   // every counter on a line of its own
// the launch's arena (KmRgbwState::ps_arena): [PsBar | 3 x kPsPartWords sums | PsDev | chunk boundaries u32[ps_blocks x kPsChunks + 1]]; everything in front of
// the boundaries is zero when k_ps_ranges starts
struct PsDevPtrs {                        // what only the launch's set-up and write-out read (k_ps_ranges leaves it in device memory)
    const uint32_t *ckeys, *cweight;      // cell-major colours and pixel counts
    uint8_t *labels;                      // cell-major labels: the initial assignment on entry, the result on a regular exit
    const uint32_t *ne_cell, *ne_start;   // compacted non-empty cells: id, first position
    const uint2 *cconst0;                 // the initial centroids (k_rgbw_init_cent)
    // The large cluster-colors encode (cc_prepare_image) gives the points a second source, sbin set: the histogram's staged (bin, count)
    // pairs (k_sp_hist, k_points.hip), which lie in cell-major order already -- bucket b's entries at sstart[b] + (i - cell_start[64 b]) --
    // so nothing copies them into ckeys / cweight / labels first: the set-up makes key and initial label itself (sp_key, gidx_rank,
    // init_label24 with the count of colours at U_dev) and leaves in cweight_rw only the counts a packed word cannot hold.
    const uint32_t *sstart; const uint16_t *sbin; const uint32_t *scnt; const uint32_t *cell_start;
    const unsigned long long *gbits; const uint32_t *gprefix; const uint64_t *U_dev;
    uint32_t *cweight_rw;
    const uint64_t *count_dev;            // set: the host enqueued the launch without having seen the count (fewer than K: every block leaves at once)
};
struct PsDev { uint32_t fail, pad; PsDevPtrs p; };   // fail: some block's cells do not fit its LDS (k_ps_ranges): no block starts
constexpr uint32_t kPsArenaPart = (sizeof(PsBar) + 255u) & ~255u, kPsArenaFail = kPsArenaPart + ((3u * kPsPartWords * 8u + 255u) & ~255u), kPsArenaRng = kPsArenaFail + 256u;
static_assert(sizeof(PsDev) <= 256, "PsDev has 256 bytes of the arena");
constexpr uint32_t kPsStatusDone = 1, kPsStatusAborted = 2, kPsStatusRanges = 3, kPsStatusFew = 4;   // (Few: fewer points than clusters, seen by the launch itself)
struct PsExit { uint32_t status, pad; uint64_t iter, moved_last, reseeds, active, pair_evals; uint32_t group_iters[3], pad2; };   // pinned: how the launch ended (group_iters: block 0's skip-schedule iterations with 4, 8, 16 lanes per cell)
void launch_rgbw_assign_big(Ctx *c, const uint32_t *ckeys, const uint32_t *cweight, uint64_t U, uint32_t K, const uint32_t *cent, uint16_t *labels,
                            unsigned long long *partials, const KmDevState *st);
struct PsSetup {                          // ps_decide's answer.  on: there is a persistent launch; then [zero_p, + zero_bytes) of its arena must be zeroed and
    bool on = false;                      // k_ps_ranges run with (G, budget, cb, dev, ptrs) before it
    uint32_t G = 0, budget = 0;
    uint32_t *cb = nullptr; PsDev *dev = nullptr; PsDevPtrs ptrs{};
    void *zero_p = nullptr; uint64_t zero_bytes = 0;
};
int ps_decide(KmRgbwState *s, PsSetup *out);
int ps_enqueue(KmRgbwState *s, const PsSetup &p);
void ps_launch_ranges(Ctx *c, const uint32_t *ne_cost, const uint32_t *ne_count, uint32_t G, uint32_t budget, uint32_t *cb, PsDev *dev, const PsDevPtrs &ptrs);
int km_rgbw_run_persistent(KmRgbwState *s, bool *ran, bool may_defer);
int km_rgbw_persistent_verdict(KmRgbwState *s, bool *retry);   // for km_rgbw_result_end: how a deferred launch ended
constexpr uint32_t kAggMin = 16;  // points that must share the first mover's (old, new) pair for a round of aggregated booking to be worth it


__device__ __forceinline__ uint32_t dot4u8(uint32_t a, uint32_t b, uint32_t acc) {
    return __builtin_amdgcn_udot4(a, b, acc, false);
}

// (packed centroid key, const term) for cluster k
__device__ __forceinline__ uint2 make_cconst(uint32_t ckey, uint32_t k, uint32_t idbits) {
    uint32_t h = dot4u8(ckey, ckey, 0);
    uint32_t idmask = (1u << idbits) - 1;
    return make_uint2(ckey, ((kBias - h) << idbits) | (idmask - k));
}

// ---- the set-up kernels' bodies.  Each is launched on its own (k_rgbw_init_cent, k_cell_totals, k_cell_scan: k_kmeans_rgbw.hip;
// k_ps_ranges: k_kmeans_persist.hip) and as a role of the large cluster-colors encode's set-up launches (k_cc_front_*: k_points.hip).
// init (kmeans.rs:61-108), thread k of Kpad
__device__ __forceinline__ void rgbw_init_cent_body(uint32_t k, const uint32_t *__restrict__ keys, uint64_t U, uint32_t K, uint32_t Kpad, uint32_t idbits,
                                                    uint2 *__restrict__ cconst, uint32_t *__restrict__ cent, const GIdx &gx, uint32_t *__restrict__ cent_copy,
                                                    uint32_t *__restrict__ moved_list, const uint64_t *__restrict__ U_dev) {
    if (U_dev) U = max(*U_dev, (uint64_t)K);  // the count is still on its way to the host (fewer points than clusters: refused there)
    if (k == 0 && moved_list) moved_list[0] = K;  // before the first update every centroid counts as moved
    if (k < K) {
        // init_centroids (kmeans.rs:101-108): first element of chunk k
        uint64_t ppc = U / K;
        uint64_t first = (k < K - 1) ? U - ((uint64_t)k + 1) * ppc : 0;
        uint32_t ck = gx.bits ? gidx_select(gx, first) : keys[first];
        cent[k] = ck;
        if (cent_copy) cent_copy[k] = ck;
        cconst[k] = make_cconst(ck, k, idbits);
    } else if (k < Kpad) {
        cconst[k] = make_uint2(0u, 0u);  // padding: key 0 never wins
    }
}

// Exclusive scan of the cell counts in two steps of kNumCells / 64 waves: per 64 cells (points, non-empty cells), then every wave
// adds up the groups before its own (k_kmeans_rgbw.hip has the whole story).  A wave per group `grp`, lane <-> cell.
constexpr uint32_t kCellGroups = kNumCells / 64;
// (tot[kCellGroups + g]: the group's sweeps, ceil(points / 256) per cell -- the full schedule's cost model counts them)
__device__ __forceinline__ void cell_totals_body(uint32_t grp, uint32_t lane, const uint32_t *__restrict__ cell_count, uint2 *__restrict__ tot) {
    const uint32_t v = cell_count[grp * 64 + lane];
    const uint32_t sum = wave_reduce_sum(v), sweeps = wave_reduce_sum((v + 64 * kSweep - 1) / (64 * kSweep));
    const uint32_t ne = (uint32_t)__popcll(__ballot(v != 0));
    if (lane == 0) { tot[grp] = make_uint2(sum, ne); tot[kCellGroups + grp] = make_uint2(sweeps, 0u); }
}
// (cb, when set: the persistent launch's NC + 1 chunk boundaries as well, every cell those that fall on it -- ps_bounds.hpp; what
// k_ps_ranges bisects for, word for word)
struct CellScanOut { uint32_t *cell_start, *cursor, *ne_cell, *ne_start, *ne_cost, *ne_count; uint32_t *cb; uint32_t NC; };
__device__ __forceinline__ void cell_scan_body(uint32_t grp, uint32_t lane, const uint32_t *__restrict__ cell_count, const uint2 *__restrict__ tot,
                                               const CellScanOut &o, uint32_t fixed_cost, uint32_t sweep_cost) {
    // cost of a cell in the full schedule's split: fixed_cost + points if sweep_cost == 0, else fixed_cost + sweep_cost * sweeps
    uint32_t ps = 0, pn = 0, pw = 0, an = 0, aw = 0, ap = 0;   // (a*: over all the groups, for the total cost the boundaries are cut from)
    if (o.cb) {
        static_assert(kCellGroups % 64 == 0, "every lane looks at the same number of groups");
#pragma unroll
        for (uint32_t g0 = 0; g0 < kCellGroups; g0 += 64) {   // (the loads of all trips issued together)
            const uint32_t g = g0 + lane;
            const uint2 t = tot[g];
            const uint32_t w = tot[kCellGroups + g].x;
            ap += t.x; an += t.y; aw += w;
            if (g < grp) { ps += t.x; pn += t.y; pw += w; }
        }
    } else {
        for (uint32_t g = lane; g < grp; g += 64) { const uint2 t = tot[g]; ps += t.x; pn += t.y; pw += tot[kCellGroups + g].x; }
    }
    const uint32_t base = wave_reduce_sum(ps), nbase = wave_reduce_sum(pn), wbase = wave_reduce_sum(pw);
    const uint32_t cell = grp * 64 + lane, v = cell_count[cell], sw = (v + 64 * kSweep - 1) / (64 * kSweep);
    const uint32_t start = base + wave_inclusive_scan(v) - v, swb = wbase + wave_inclusive_scan(sw) - sw;
    o.cell_start[cell] = start;
    if (o.cursor) o.cursor[cell] = start;
    const unsigned long long nzm = __ballot(v != 0);
    if (v) {
        const uint32_t m = nbase + (uint32_t)__popcll(nzm & ((1ull << lane) - 1ull));
        o.ne_cell[m] = cell; o.ne_start[m] = start; o.ne_cost[m] = (sweep_cost ? swb * sweep_cost : start) + m * fixed_cost;
    }
    if (o.cb) {
        const uint32_t Mall = wave_reduce_sum(an);
        const uint64_t total = (sweep_cost ? wave_reduce_sum(aw) * sweep_cost : wave_reduce_sum(ap)) + Mall * fixed_cost;   // = ne_cost[M], the u32 the last lane writes
        if (v) {
            const uint32_t m = nbase + (uint32_t)__popcll(nzm & ((1ull << lane) - 1ull));
            const uint32_t mine = (sweep_cost ? swb * sweep_cost : start) + m * fixed_cost, next = mine + (sweep_cost ? sw * sweep_cost : v) + fixed_cost;   // ne_cost[m], ne_cost[m + 1]
            if (m == 0) { const PsBoundRun r = ps_bounds_upto(mine, total, o.NC); for (uint32_t j = 0; j < r.count; j++) o.cb[r.first + j] = 0u; }
            const PsBoundRun r = ps_bounds_between(mine, next, total, o.NC);
            for (uint32_t j = 0; j < r.count; j++) o.cb[r.first + j] = m + 1;
        }
    }
    if (grp == kCellGroups - 1 && lane == 63) {
        const uint32_t U = start + v, M = nbase + (uint32_t)__popcll(nzm);
        o.cell_start[kNumCells] = U;
        o.ne_start[M] = U;
        o.ne_cost[M] = (sweep_cost ? (swb + sw) * sweep_cost : U) + M * fixed_cost;
        *o.ne_count = M;
    }
}

// the chunk boundaries of the persistent launch (k_kmeans_persist.hip: "who owns what"): ONE block of 1024 threads -- the barrier and the
// fit check behind it see this block's own stores
__device__ __forceinline__ void ps_ranges_body(const uint32_t *__restrict__ ne_cost, const uint32_t *__restrict__ ne_count, uint32_t G, uint32_t dyn_bytes,
                                               uint32_t *__restrict__ cb, PsDev *__restrict__ dev, const PsDevPtrs &ptrs) {
    uint32_t *fail = &dev->fail;
    if (threadIdx.x == 0) dev->p = ptrs;
    const uint32_t M = *ne_count, NC = G * kPsChunks;
    const uint64_t total = ne_cost[M];
    // (a thread's boundaries searched TOGETHER, eight at a time: one after the other the 4097 bisections of the headline image were 60
    // dependent reads a thread, 21 us in front of the launch)
    for (uint32_t g0 = threadIdx.x; g0 <= NC; g0 += 8 * blockDim.x) {
        uint32_t a[8], b[8];
        uint64_t c_lo[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t g = g0 + r * blockDim.x;
            c_lo[r] = ps_bound_target(total, g, NC);
            a[r] = 0; b[r] = g <= NC ? M : 0u;   // first cell whose cost prefix is >= c_lo
        }
        bool more = true;
        while (more) {
            more = false;
            uint32_t mid[8], v[8];
#pragma unroll
            for (int r = 0; r < 8; r++) { mid[r] = (a[r] + b[r]) >> 1; v[r] = a[r] < b[r] ? ne_cost[mid[r]] : 0u; }
#pragma unroll
            for (int r = 0; r < 8; r++)
                if (a[r] < b[r]) { if (v[r] < c_lo[r]) a[r] = mid[r] + 1; else b[r] = mid[r]; more = more || a[r] < b[r]; }
        }
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t g = g0 + r * blockDim.x;
            if (g <= NC) cb[g] = g == NC ? M : a[r];
        }
    }
    __syncthreads();   // (one block: its own stores are visible to it behind the barrier)
    for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) {
        uint32_t C = 0;
        for (uint32_t r = 0; r < kPsChunks; r++) C += cb[r * G + g + 1] - cb[r * G + g];
        if (C > kPsMaxCells || kPsOffCell + ps_cell_bytes(C) > dyn_bytes) atomicAdd(fail, 1u);
    }
}

// ... and what is left of it when the cell scan has written the boundaries (CellScanOut::cb): the launch's pointers and the fit check, a
// block's 2 x kPsChunks boundaries asked for together.  Any number of threads of ONE block.
__device__ __forceinline__ void ps_fit_body(uint32_t G, uint32_t dyn_bytes, const uint32_t *__restrict__ cb, PsDev *__restrict__ dev, const PsDevPtrs &ptrs) {
    if (threadIdx.x == 0) dev->p = ptrs;
    for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) {
        uint32_t lo[kPsChunks], hi[kPsChunks];
#pragma unroll
        for (uint32_t r = 0; r < kPsChunks; r++) { lo[r] = cb[r * G + g]; hi[r] = cb[r * G + g + 1]; }
        uint32_t C = 0;
#pragma unroll
        for (uint32_t r = 0; r < kPsChunks; r++) C += hi[r] - lo[r];
        if (C > kPsMaxCells || kPsOffCell + ps_cell_bytes(C) > dyn_bytes) atomicAdd(&dev->fail, 1u);
    }
}

// What km_rgbw_create leaves to its caller when asked to (points_follow only): the set-up dispatches it would enqueue, described
// instead.  The caller enqueues them -- as the roles of k_cc_front_* or, km_front_enqueue_split, as the kernels create itself launches --
// before anything else touches the state.
struct KmFront {
    void *arena = nullptr; uint64_t arena_bytes = 0;          // to be zeroed ...
    void *ps_arena = nullptr; uint64_t ps_zero_bytes = 0;     // ... and, with ranges, the head of the persistent launch's arena
    // k_rgbw_init_cent (behind the zeroing: it writes into the arena)
    uint64_t Ulist = 0; uint32_t K = 0, Kpad = 0, idbits = 0;
    uint2 *cconst = nullptr; uint32_t *cent = nullptr, *cent_copy = nullptr, *moved_list = nullptr;
    GIdx gx{nullptr, nullptr, 0}; const uint64_t *U_dev = nullptr;
    // k_cell_totals / k_cell_scan
    const uint32_t *cell_count = nullptr; DevBuf cell_tot; CellScanOut scan{};
    // k_ps_ranges (ranges: there is a persistent launch)
    bool ranges = false; uint32_t G = 0, budget = 0; uint32_t *cb = nullptr; PsDev *dev = nullptr; PsDevPtrs ptrs{};
};
int km_rgbw_create_deferred(Ctx *c, uint64_t Umax, uint32_t K, const cniic_kmeans_opts *opts, KmRgbwState **out, const uint32_t *cell_count_d,
                            const void *gbits_d, const uint32_t *gprefix_d, uint64_t Ug, const uint64_t *points_dev, KmFront *front);
int km_front_enqueue_split(Ctx *c, const KmFront &f);   // the fills and the four kernels, in create's own order
// cc_prepare_image, with a persistent launch to come: the cell-major arrays are not written -- the launch takes its points from plan's
// staging (front->ptrs is completed here), and plan outlives the state's last use of it
void km_rgbw_points_from_staging(KmRgbwState *s, const SpPlan *plan, KmFront *front);
bool km_rgbw_arrays_pending(const KmRgbwState *s);
void km_rgbw_count_stays_on_device(KmRgbwState *s, const uint64_t *count_dev);   // (in the place of km_rgbw_set_points, until the count has arrived)
int km_rgbw_fetch_points(KmRgbwState *s);   // a state that still waits for its count: fetches it, now, and sets the points
// the arrays after all: k_sp_emit, once, on the state's stream (the labels only while they do not hold a result).  Not while a
// deferred launch's verdict is out.
int km_rgbw_need_arrays(KmRgbwState *s);

struct CellBox { int32_t r0, g0, b0; };  // low corner of a cube of colours
__device__ __forceinline__ CellBox super_box(uint32_t sup) {
    return CellBox{(int32_t)((sup / (kSupersPerDim * kSupersPerDim)) << (kCellShift + 2)),
                   (int32_t)(((sup / kSupersPerDim) % kSupersPerDim) << (kCellShift + 2)),
                   (int32_t)((sup % kSupersPerDim) << (kCellShift + 2))};
}
__device__ __forceinline__ CellBox cell_box(uint32_t c) {
    const CellBox sb = super_box(c >> kSuperShift);
    return CellBox{sb.r0 + (int32_t)(((c >> 4) & 3) << kCellShift), sb.g0 + (int32_t)(((c >> 2) & 3) << kCellShift),
                   sb.b0 + (int32_t)((c & 3) << kCellShift)};
}

constexpr uint32_t kRecComplete = 0x80000000u;  // word 1 of a record: the mask holds EVERY centroid its pivot does not dominate (skip schedule, K <= 256)
__host__ __device__ constexpr uint32_t cell_rec_words(uint32_t MW) { return (2 + 2 * MW + 15) & ~15u; }  // u32 words of a cell's skip record (CellState below)
constexpr uint32_t kMaxMovedSkip = 64;  // skip schedule when at most this many centroids moved (one per lane of the test; measured on the
                                        // headline encode: 128 -> 1.92 ms of assign launches, 96 -> 1.90, 64 -> 1.88, 40 -> 1.88: above ~60 moved
                                        // centroids a third of the cells are dirty and dealing them round-robin costs more than the full schedule's ranges)

// Both tests of the pruning on PACKED colour bytes (round 4; until then three field extractions, three products and their sums each: 10 and 21
// vector instructions, a third of a candidate build).  r | g | b in bytes 2, 1, 0 of a key, byte 3 zero; a cube is aligned, so lo + ext <= 255.
__device__ __forceinline__ uint32_t pack_rgb(int32_t r, int32_t g, int32_t b) { return ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b; }

// squared distance from colour key ck to the centre of the cube with low corner bx and side ext + 1:
// |v - c|^2 = v.v - 2 v.c + c.c, three byte dot products (two of them per candidate)
__device__ __forceinline__ uint32_t centre_dist(uint32_t ck, const CellBox &bx, int32_t ext) {
    const int32_t h = (ext + 1) >> 1;
    const uint32_t c = pack_rgb(bx.r0 + h, bx.g0 + h, bx.b0 + h);
    return dot4u8(ck, ck, dot4u8(c, c, 0)) - 2u * dot4u8(ck, c, 0);
}

// a pivot centroid p against one cube [lo, lo + ext]^3.  max over the cube of d(x, p) - d(x, v) -- v can be nearest (or tie) somewhere in the
// cube only if it is >= 0 -- is, per channel with d = p - v, max(d (v + p - 2 lo), d (v + p - 2 hi)) = d (v + p - 2 lo) + 2 ext max(0, -d);
// summed: (p.p - 2 p.lo - ext sum(p)) - v.v + v.lo + v.hi + ext sad(p, v)      [sum max(0, -d) = (sad(p, v) - sum(p) + sum(v)) / 2]
// -- a constant of the pivot, three byte dot products, one sum of absolute differences and one multiply-add per candidate.
struct Dominance {
    uint32_t ppk, lopk, hipk;
    int32_t cp, ext;
    __device__ __forceinline__ void set(const CellBox &bx, int32_t e, uint32_t pivot) {
        ppk = pivot & 0xffffffu;
        ext = e;
        lopk = pack_rgb(bx.r0, bx.g0, bx.b0);
        hipk = pack_rgb(bx.r0 + e, bx.g0 + e, bx.b0 + e);
        cp = (int32_t)dot4u8(ppk, ppk, 0) - 2 * (int32_t)dot4u8(ppk, lopk, 0) - e * (int32_t)dot4u8(ppk, 0x010101u, 0);
    }
    __device__ __forceinline__ int32_t worst(uint32_t ck) const {
        const uint32_t v = ck;   // (a colour key: byte 3 is zero)
        return cp - (int32_t)dot4u8(v, v, 0) + (int32_t)dot4u8(v, hipk, dot4u8(v, lopk, 0)) + __mul24(ext, (int32_t)__builtin_amdgcn_sad_u8(ppk, v, 0u));
    }
};

__device__ __forceinline__ uint32_t wave_all_min(uint32_t v) { return wave_reduce_min(v); }  // (DPP: the result is in every lane)

// position in `list` (n entries, ascending cluster id) of the centroid nearest the cube centre; lowest position on ties
// (ONE reduction over distance << 12 | position: a distance is below 3 * 255^2 < 2^18 and a list holds at most 4096 entries; until round 4 two
// reductions, first the distance, then the position among the lanes that had it -- a sixth of a candidate build's vector instructions)
__device__ __forceinline__ uint32_t nearest_to_centre(const uint2 *list, uint32_t n, const CellBox &bx, int32_t ext, int lane) {
    uint32_t bd = 0xfffffu, be = 4095u;
    for (uint32_t e = lane; e < n; e += 64) {
        const uint32_t d = centre_dist(list[e].x, bx, ext);
        if (d < bd) { bd = d; be = e; }
    }
    return wave_all_min((bd << 12) | be) & 4095u;
}

// S = the centroids of `tab` (ascending id) that can be nearest somewhere in super-cell `sup`; returns |S| >= 1
// set bits of a ballot below this lane: v_mbcnt (two instructions, and no 64-bit lane mask kept in registers)
__device__ __forceinline__ uint32_t lanes_below(unsigned long long bm) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
}

__device__ __forceinline__ uint32_t build_super(const uint2 *tab, uint32_t K, uint32_t sup, int lane, unsigned long long lt_mask,
                                                uint2 *S, uint32_t cap) {
    constexpr int32_t ext = (1 << (kCellShift + 2)) - 1;
    const CellBox bx = super_box(sup);
    Dominance dm;
    dm.set(bx, ext, tab[nearest_to_centre(tab, K, bx, ext, lane)].x);
    uint32_t n = 0;
    for (uint32_t k0 = 0; k0 < K; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint2 cc = make_uint2(0u, 0u);
        bool keep = false;
        if (k < K) { cc = tab[k]; keep = dm.worst(cc.x) >= 0; }
        const unsigned long long bm = __ballot(keep);
        const uint32_t pos = n + lanes_below(bm);
        if (keep && pos < cap) S[pos] = cc;  // a longer list is not kept: the caller falls back to the whole table
        n += (uint32_t)__popcll(bm);
    }
    __builtin_amdgcn_wave_barrier();
    return n;
}

// ---- the packed point word of the resident points (k_kmeans_persist.hip)
__device__ __forceinline__ uint32_t pk_make(uint32_t key, uint32_t w, uint32_t label) {
    return (((key >> 16) & 7u) << 6) | (((key >> 8) & 7u) << 3) | (key & 7u) | (min(w, 255u) << 16) | (label << 24);
}
__device__ __forceinline__ uint32_t pk_key(uint32_t pw, uint32_t cell_base) {   // cell_base = the cell's low corner r0 << 16 | g0 << 8 | b0
    return cell_base | ((pw & 0x1c0u) << 10) | ((pw & 0x38u) << 5) | (pw & 7u);
}
__device__ __forceinline__ uint32_t cell_base_key(uint32_t c) {
    const CellBox b = cell_box(c);
    return ((uint32_t)b.r0 << 16) | ((uint32_t)b.g0 << 8) | (uint32_t)b.b0;
}

}  // namespace cniic
