// common.hpp -- shared host-side plumbing of libcniic_hip.so (context, scratch HBM, error
// handling).  gfx950 only; no CPU fallback anywhere in this library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cniic_hip.h"

namespace cniic {

constexpr uint64_t kDefaultSeed = 0x636E696963ULL;

struct KernelTime {
    double   ms = 0.0;
    uint64_t launches = 0;
};

struct Ctx;

// Caching HBM allocator: hipMalloc / hipFree cost tens of microseconds and hipFree synchronises
// the device, so scratch buffers are recycled per context (a codec call allocates ~20 of them).
struct DevPool {
    struct Block { void *p; uint64_t cap; };
    std::vector<Block> free_blocks;
    uint64_t cached_bytes = 0;
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { trim(); }   // (every DevBuf that took a block from this pool has given it back: Ctx's member order)
    hipError_t get(uint64_t bytes, void **p, uint64_t *cap) {
        // best fit among cached blocks that are not more than 2x too large
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < free_blocks.size(); i++)
            if (free_blocks[i].cap >= bytes && free_blocks[i].cap <= 2 * bytes + 4096 &&
                (best == SIZE_MAX || free_blocks[i].cap < free_blocks[best].cap))
                best = i;
        if (best != SIZE_MAX) {
            *p = free_blocks[best].p;
            *cap = free_blocks[best].cap;
            cached_bytes -= *cap;
            free_blocks.erase(free_blocks.begin() + (long)best);
            return hipSuccess;
        }
        const uint64_t rounded = (bytes + 255) & ~255ull;
        hipError_t e = hipMalloc(p, rounded);
        if (e != hipSuccess && !free_blocks.empty()) {  // out of memory: drop the cache and retry
            trim();
            e = hipMalloc(p, rounded);
        }
        *cap = rounded;
        return e;
    }
    void put(void *p, uint64_t cap) {
        free_blocks.push_back({p, cap});
        cached_bytes += cap;
    }
    void trim() {
        for (auto &b : free_blocks) (void)hipFree(b.p);
        free_blocks.clear();
        cached_bytes = 0;
    }
};

// the pool of the context whose call is running on this thread (set by the ABI entry points)
inline DevPool *&current_pool() {
    static thread_local DevPool *p = nullptr;
    return p;
}

// DevBufs allocated while this lives come from pool p (an ABI call: its context's pool) -- or, PoolScope keep(nullptr), straight from
// hipMalloc: buffers that live as long as the context and are not recycled
struct PoolScope {
    DevPool *prev;
    explicit PoolScope(DevPool *p) : prev(current_pool()) { current_pool() = p; }
    PoolScope(const PoolScope &) = delete;
    PoolScope &operator=(const PoolScope &) = delete;
    ~PoolScope() { current_pool() = prev; }
};

// RAII device allocation on the context's device (recycled through the context's pool).
struct DevBuf {
    void    *p = nullptr;
    uint64_t bytes = 0;
    uint64_t cap = 0;
    DevPool *pool = nullptr;
    bool     owned = true;   // false: a view into another DevBuf (never released)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), cap(o.cap), pool(o.pool), owned(o.owned) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; cap = o.cap; pool = o.pool; owned = o.owned; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(uint64_t n) {
        release();
        if (n == 0) n = 16;
        pool = current_pool();
        hipError_t e;
        if (pool) e = pool->get(n, &p, &cap);
        else { e = hipMalloc(&p, n); cap = n; }
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    void view(void *ptr, uint64_t n) { release(); p = ptr; bytes = n; cap = 0; pool = nullptr; owned = false; }
    void release() {
        if (!p) return;
        if (owned) { if (pool) pool->put(p, cap); else (void)hipFree(p); }
        p = nullptr; bytes = 0; owned = true;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// A block of pinned host memory that a context owns.
struct PinnedBuf {
    void    *p = nullptr;
    uint64_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    // at least `need` bytes: a block that is too small is freed and one of `want` (>= need) bytes takes its place, contents lost
    hipError_t reserve(uint64_t need, uint64_t want) {
        if (bytes >= need) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0;
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) bytes = want; else p = nullptr;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// An event that a context owns, created at its first use.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t ensure(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// The stream a context made for itself (none when the host gave it one).
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    OwnedStream &operator=(const OwnedStream &) = delete;
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
};

// Knobs of the test-suite and the probes under tools/ (CNIIC_TEST_* hooks, route forcing, the persistent launch's timeout) are
// read from the environment ONLY by the testing build (-DCNIIC_TESTING: libcniic_hip_testing.so, which tests/conftest.py and tools/ ask
// for with CNIIC_USE_TESTING_LIB=1).  In the release library test_env() is a constant nullptr: no getenv, and the names are not even in
// the binary (tests/test_abi.py checks `strings`).  What a host may set on a release build are the context options of the ABI, whose
// documented environment fallbacks (Ctx::opt below) stay.
#ifdef CNIIC_TESTING
inline const char *test_env(const char *name) { return getenv(name); }
#else
inline const char *test_env(const char *) { return nullptr; }
#endif
// Two shapes that most knobs of the small-frame routes have.  Both are inline so that the release library folds them to their last
// argument and keeps none of the names.
// A scratch budget of `cap` bytes that the tests make small (CNIIC_TEST_MEASURE_BUDGET, bytes; never above cap)
inline uint64_t test_budget(uint64_t cap) {
    if (const char *e = test_env("CNIIC_TEST_MEASURE_BUDGET")) return std::min<uint64_t>(strtoull(e, nullptr, 10), cap);
    return cap;
}
// The most pixels of a frame that takes a route whose own bound is `bound`: 0 with off_env=1 (the route is off), max_px_env (may be null:
// no such knob) lowers it
inline uint64_t small_route_max_px(const char *off_env, const char *max_px_env, uint64_t bound) {
    if (const char *e = test_env(off_env)) if (atoi(e) != 0) return 0;
    if (const char *e = max_px_env ? test_env(max_px_env) : nullptr) return std::min<uint64_t>(strtoull(e, nullptr, 10), bound);
    return bound;
}

// Every resource below is owned by its member's type and released by that type's destructor, in reverse order of declaration: the order
// of the members IS the order of the teardown.  What it must keep: the workers go first (they hold views of scan_xy), every DevBuf that
// may hold a block of `pool` goes before `pool` (whose destructor frees what it caches), the stream the context made goes last.
struct Ctx {
    int         device = 0;
    OwnedStream own_stream;        // declared before everything that may have work on it
    hipStream_t stream = nullptr;  // the stream the calls run on: own_stream.s, or the host's
    std::mutex  mu;
    std::string err;
    std::map<std::string, KernelTime> ktimes;  // per-call dominant-kernel timings (HIP events)
    Event   ev0, ev1;       // the stage timers' pair (default flags: they read elapsed time), created with the context
    bool    timers = getenv("CNIIC_KERNEL_TIMERS") != nullptr;  // per-stage HIP-event timers (they synchronise)
    // cniic_ctx_set_opt: values a host set for this context (bit i of opt_set); unset options read their environment variable per call
    uint64_t opt_val[CNIIC_OPT_COUNT] = {};
    uint32_t opt_set = 0;
    uint64_t opt(int id, const char *env, uint64_t dflt) const {
        if (id > 0 && id < CNIIC_OPT_COUNT && ((opt_set >> id) & 1u)) return opt_val[id];
        const char *e = env ? getenv(env) : nullptr;
        return e ? strtoull(e, nullptr, 10) : dflt;
    }
    DevPool pool;           // recycled scratch HBM (all DevBufs created inside an ABI call)
    // persistent scratch: dense symbol tables (zeroed on demand), grown lazily
    DevBuf dense;           // u32[2^24] or u32[2^27]
    DevBuf dense27, dense27_pages;  // `delta`: u32[2^27] SignedColor counts + a flag per 4096-entry page, all zero between calls (k_delta.hip)
    bool   dense27_clean = false;
    DevBuf hilbert_lut;     // state-machine tables of the 2^n Hilbert scan (k_hilbert.hip)
    PinnedBuf pinned;       // 4 KiB of pinned host memory: two KmDevState slots for lagged convergence polling
    PinnedBuf pinned_ps;    // 1 KiB: how the persistent K-means launch ended (PsExit, k_kmeans_persist.hip)
    uint32_t ps_div = 1;         // the persistent K-means launch takes 1 / ps_div of the CUs (worker contexts of a batch encode)
    uint32_t ps_backoff = 0, ps_backoff_left = 0;   // after a persistent launch whose grid was not resident together in time (somebody else's kernels on the CUs: a 2 s
                                                    // wait before the launches take over) the next 4, 8, ... 256 K-means runs of this context do not try one
    Event poll_ev[2];
    PinnedBuf pinned_res;   // pinned landing area of K-means result blocks (grown on demand)
    Event res_ev;
    PinnedBuf pinned_u;     // 64 KiB of pinned host memory (u64 words) for small answers from the GPU: who owns which words is the PuSlot table below
    Event u_ev;             // behind a copy into pinned_u that the host waits for later (kPuSpCount, kPuPaletteWeights)
    std::shared_ptr<void> trie_scratch; // the decoder's parsed leaf table (LeafTable, codec.cpp), kept between calls: 90 MB of fresh pages cost 25 ms
    std::shared_ptr<void> huf_scratch;  // host arrays of the Huffman tree build, kept between calls (HuffScratch, codec.cpp)
    PinnedBuf pinned_huf;   // pinned host memory, grown on demand (pinned_huf_want): the Huffman code stage's counts, tree and codes (HuffCodeStage, codec.cpp); a decode's stream heads
    Event huf_ev;           // behind the D2H copies of the compacted histogram (huf_encode_all_dev)
    Event surf_ev;          // behind the upload of a surface call's frame and chunk tables: the call returns while its kernel runs, not before that copy has read the host's vectors (k_surface.hip)
    std::shared_ptr<void> scan_leaves;  // the built-in scan of large rectangles: per image size, the recursion's leaves and class tables (k_hilbert.hip)
    DevBuf scan_xy;         // cniic_ctx_set_scan: an injected scan of scan_w x scan_h images, (x, y) per position (uint2[w h])
    uint32_t scan_w = 0, scan_h = 0;
    DevBuf batch_stage;     // a worker of cniic_codec_encode_batch_var: the 16-byte aligned copy of a frame that lies at another address
    const void *poll_owner = nullptr;  // the K-means state whose lagged polls own `pinned` / poll_ev (one loop at a time per context)
    std::vector<std::unique_ptr<cniic_ctx>> batch_workers;  // the batch calls' worker contexts, created on first use; the last member: destroyed first

    ~Ctx();   // (below cniic_ctx)

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

}  // namespace cniic
struct cniic_ctx : cniic::Ctx {};   // the ABI's handle
namespace cniic {

// waits for the context's work; the members' destructors release everything after it
inline Ctx::~Ctx() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
}

#define CNIIC_HIP_TRY(ctx, expr)                                                          \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return (ctx)->fail(CNIIC_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, \
                               hipGetErrorString(_e));                                    \
    } while (0)

// Waits for the context's stream without giving the core up: a blocking wait of a few hundred microseconds sends the core to
// sleep, and the host work that follows (the Huffman tree of a `delta` encode) then runs at half speed.
inline hipError_t ctx_spin_sync(Ctx *c) {
    hipError_t e;
    while ((e = hipStreamQuery(c->stream)) == hipErrorNotReady) {}
    return e;
}

constexpr uint64_t pinned_huf_want(uint64_t bytes) { return bytes + bytes / 4 + 65536; }   // what Ctx::pinned_huf grows to when `bytes` are asked of it

// Ctx::pinned_u in u64 words.  Every user has words of its own: a copy into one may still be on its way for one session of a context
// (cc_image_begin ... cc_finish) when another call on that context starts, so no two meanings share a word.
struct PuSlot { uint32_t at, words; };
constexpr uint32_t kPinnedUWords = 64 * 1024 / 8, kPinnedUBytes = kPinnedUWords * 8;
constexpr PuSlot kPuSpCount{0, 1};            // sp_build: distinct colours of the image (k_points.hip)
constexpr PuSlot kPuPointCount{1, 1};         // cc_image_create: length of the point list, the colours of all images
constexpr PuSlot kPuImageCount{2, 1};         // cc_image_create: this image's own distinct colours, fetched again
constexpr PuSlot kPuHufTotals{3, 2};          // the Huffman code stage: payload bits, "a code is too long" (huff_tree_codes)
constexpr PuSlot kPuDeltaOverflow{5, 1};      // encode_delta: a chunk with more than 64 symbols outside the cube
constexpr PuSlot kPuDeltaPacked{6, 1};        // encode_delta: bits the pack wrote
constexpr PuSlot kPuPaletteWeights{8, 4096};  // cc_finish: this image's pixels per cluster (shared palette, K <= 4096)
constexpr PuSlot kPuHdecode{4104, 3};         // huff_decode_dev: total symbols, "an end moved", blocks that gave the stream up (k_hdecode.hip)
constexpr PuSlot kPuTrieTotals{4108, 6};      // huff_parse_leaves_dev: TpTotals (k_trieparse.hip)
constexpr PuSlot kPuLeafRuns{4114, 3};        // huff_tree_from_runs: number of runs, then bits / too long / longest (k_huff.hip)
constexpr PuSlot kPuCcUpload{4120, 1024};     // cc_finish: codes, lengths and header for k_sp_pixpack, which reads them here (kCcUp*)
constexpr PuSlot kPuCcPacked{5144, 2};        // cc_finish: "a block of k_sp_pixpack gave up", the bits it wrote
constexpr PuSlot kPuSlots[] = {kPuSpCount, kPuPointCount, kPuImageCount, kPuHufTotals, kPuDeltaOverflow, kPuDeltaPacked,
                               kPuPaletteWeights, kPuHdecode, kPuTrieTotals, kPuLeafRuns, kPuCcUpload, kPuCcPacked};   // in ascending order
constexpr bool pu_slots_disjoint() {
    uint32_t end = 0;
    for (const PuSlot &s : kPuSlots) {
        if (s.at < end || s.words == 0) return false;
        end = s.at + s.words;
    }
    return end <= kPinnedUWords;
}
static_assert(pu_slots_disjoint(), "Ctx::pinned_u: two slots overlap, or the last one ends behind the 64 KiB block");
static_assert(kPuPaletteWeights.words >= 4096, "Ctx::pinned_u: the shared-palette weights need room for K = 4096");

#define CNIIC_TRY(expr)              \
    do {                             \
        int _rc = (expr);            \
        if (_rc != CNIIC_OK) return _rc; \
    } while (0)

// Is p device-accessible memory (hipMalloc / torch allocation)?  Host pointers unknown to HIP
// report hipErrorInvalidValue, which is cleared.
inline bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Input view: device pointer used as is, host pointer staged into an owned HBM buffer.
template <class T> struct In {
    const T *d = nullptr;
    DevBuf   own;
    int bind(Ctx *c, const T *p, uint64_t n) {
        if (n == 0 || !p) { d = nullptr; return CNIIC_OK; }
        if (is_device_ptr(p)) { d = p; return CNIIC_OK; }
        CNIIC_HIP_TRY(c, own.alloc(n * sizeof(T)));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(own.p, p, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        d = own.as<T>();
        return CNIIC_OK;
    }
};

// Output view: device pointer written in place, host pointer filled by a D2H copy in finish().
template <class T> struct Out {
    T       *d = nullptr;
    T       *host = nullptr;
    uint64_t n = 0;
    DevBuf   own;
    int bind(Ctx *c, T *p, uint64_t count) {
        n = count;
        if (!p || count == 0) { d = nullptr; host = nullptr; return CNIIC_OK; }
        if (is_device_ptr(p)) { d = p; host = nullptr; return CNIIC_OK; }
        CNIIC_HIP_TRY(c, own.alloc(count * sizeof(T)));
        d = own.as<T>();
        host = p;
        return CNIIC_OK;
    }
    // copy the first `count` elements back (async; caller syncs the stream)
    int finish(Ctx *c, uint64_t count) {
        if (host && count) CNIIC_HIP_TRY(c, hipMemcpyAsync(host, d, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        return CNIIC_OK;
    }
    int finish(Ctx *c) { return finish(c, n); }
};

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// check_enough_active_clusters (kmeans.rs:41-57): at least 99 % of the K clusters (or every one of fewer points) must have members
inline int check_enough_active(Ctx *c, uint32_t K, uint64_t npoints, uint64_t active) {
    const uint64_t min_cc = std::min<uint64_t>((uint64_t)(0.99 * (double)K), npoints);
    if (active < min_cc)
        return c->fail(CNIIC_ERR_FEW_ACTIVE, "Not enough active clusters: requested %u, got %llu (min allowed: %llu)", K,
                       (unsigned long long)active, (unsigned long long)min_cc);
    return CNIIC_OK;
}

// body(i, t) for every i in [0, count), dealt out one at a time to `threads` threads; t: which thread (0 is the caller's)
template <class Body> void parallel_for(uint32_t count, uint32_t threads, Body body) {
    std::atomic<uint32_t> next{0};
    auto work = [&](uint32_t t) { for (uint32_t i; (i = next.fetch_add(1)) < count;) body(i, t); };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
}

// Device-resident state of a K-means loop (kmeans.rs:21-39): lets iterations be enqueued back to
// back; kernels of iterations past convergence exit on `done`.
constexpr uint32_t kHistRing = 64;
struct KmDevState {
    uint64_t iter;         // iterations completed
    uint32_t done;         // 1 once an iteration moved nothing (kmeans.rs:26) or max_iters was hit
    uint32_t pad;
    uint64_t moved_last;
    uint64_t reseeds;
    uint64_t active;
    uint64_t pair_evals;
    uint64_t changed_ring[kHistRing];
    uint32_t nmoved_ring[kHistRing];  // centroids whose value changed in the update that closed iteration i (colour K-means: picks the schedule of the next launch)
};

// One launch's view of the scalar state, written by that launch into slot (launch number % kPollRing) of a pinned ring:
// what the host reads for launch L is then the same on every rank, whatever the timing (multi-GPU loops must all leave
// after the same batch), without a copy kernel in the stream.
struct PollRec { uint64_t iter; uint32_t done; uint32_t seq; uint64_t moved_last, reseeds, active, pair_evals; };
constexpr uint32_t kPollRing = 16;

struct Comm;
void comm_abort(Comm *cm);
int comm_async_error(Comm *cm);
uint64_t comm_timeout_ms(const Comm *cm);

// Lagged convergence polling.  The K-means loops enqueue batches of (assign, update) launches; every
// kernel exits at once when the device-side `done` flag is set.  After each batch the state is copied to
// a pinned slot and an event recorded, but the host only waits for the copy of the PREVIOUS batch, so the
// GPU never idles for a host round trip; the price is at most one extra batch of no-op launches.
struct LaggedPoll {
    Ctx *c;
    const void *dstate;
    int slot = 0, pending = 0;
    bool mapped = false;  // the kernels write the state into the third pinned slot themselves: no copy to enqueue
    bool ring = false;    // ... or every launch into its own slot of the ring behind the three slots (deterministic per launch)
    uint32_t last_prev = 0;
    Comm *watch = nullptr;  // set by loops with collectives
    bool owner = false;     // this poll holds the context's slots (Ctx::poll_owner)
    LaggedPoll(Ctx *ctx, const void *dstate_d) : c(ctx), dstate(dstate_d) {}
    LaggedPoll(const LaggedPoll &) = delete;
    LaggedPoll &operator=(const LaggedPoll &) = delete;
    ~LaggedPoll() { if (owner && c->poll_owner == dstate) c->poll_owner = nullptr; }
    static constexpr size_t ring_offset() { return (3 * sizeof(KmDevState) + 63) & ~size_t(63); }
    int ring_slot(PollRec **dev_ptr) {
        static_assert(ring_offset() + kPollRing * sizeof(PollRec) <= 4096, "the poll ring must fit the pinned page");
        PollRec *r = reinterpret_cast<PollRec *>(c->pinned.as<uint8_t>() + ring_offset());
        memset(r, 0xff, kPollRing * sizeof(PollRec));  // no slot carries a valid launch number yet
        void *d = nullptr;
        CNIIC_HIP_TRY(c, hipHostGetDevicePointer(&d, r, 0));
        *dev_ptr = static_cast<PollRec *>(d);
        ring = true;
        return CNIIC_OK;
    }
    // device address of the slot the kernels write in mapped mode (zeroed here)
    int mapped_slot(KmDevState **dev_ptr) {
        KmDevState *slots = c->pinned.as<KmDevState>();
        memset(&slots[2], 0, sizeof(KmDevState));
        void *d = nullptr;
        CNIIC_HIP_TRY(c, hipHostGetDevicePointer(&d, &slots[2], 0));
        *dev_ptr = static_cast<KmDevState *>(d);
        mapped = true;
        return CNIIC_OK;
    }
    int prepare() {
        static_assert(3 * sizeof(KmDevState) <= 4096, "the poll slots must fit the pinned page");
        // The slots, the ring and the two events are the CONTEXT's: one K-means loop at a time polls through them.  A second
        // state that starts polling while another still holds them would read the first one's records -- refused instead.
        if (c->poll_owner && c->poll_owner != dstate)
            return c->fail(CNIIC_ERR_BAD_ARG, "kmeans: another K-means state of this context is polling (one lagged-poll loop per context at a time; "
                                              "destroy it, or give the second session its own context)");
        c->poll_owner = dstate;
        owner = true;
        CNIIC_HIP_TRY(c, c->pinned.reserve(4096, 4096));
        for (Event &e : c->poll_ev) CNIIC_HIP_TRY(c, e.ensure(hipEventDisableTiming));
        return CNIIC_OK;
    }
    // call after enqueuing a batch; returns the state as of the batch BEFORE it in *h (valid when *have).
    // last_launch: number of the batch's last launch (ring mode)
    int after_batch(KmDevState *h, bool *have, uint32_t last_launch = 0) {
        KmDevState *slots = c->pinned.as<KmDevState>();
        if (!mapped && !ring) CNIIC_HIP_TRY(c, hipMemcpyAsync(&slots[slot], dstate, sizeof(KmDevState), hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipEventRecord(c->poll_ev[slot], c->stream));
        *have = pending > 0;
        if (pending) {
            if (watch) {  // a loop with collectives: a peer that failed leaves this rank's stream stuck in an all-reduce -- look at the communicator while waiting
                // A dead peer is not always reported through ncclCommGetAsyncError (intra-node P2P / SHM transports), so the wait has
                // a deadline of its own: when a batch has not finished after watch_timeout_ms (cniic_comm_set_timeout /
                // CNIIC_COLLECTIVE_TIMEOUT_MS, default 120 s; 0 = wait for ever) the communicator is aborted -- by km_rgbw_run, on any
                // error return -- and the call ends with CNIIC_ERR_RCCL instead of hanging.
                const uint64_t limit_ms = comm_timeout_ms(watch);
                const auto t_wait = std::chrono::steady_clock::now();
                for (;;) {
                    const hipError_t q = hipEventQuery(c->poll_ev[slot ^ 1]);
                    if (q == hipSuccess) break;
                    if (q != hipErrorNotReady) return c->fail(CNIIC_ERR_HIP, "kmeans: waiting for a batch: %s", hipGetErrorString(q));
                    CNIIC_TRY(comm_async_error(watch));
                    if (limit_ms && std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_wait).count() >= (long long)limit_ms)
                        return c->fail(CNIIC_ERR_RCCL, "kmeans: a batch with collectives did not finish within %llu ms (a peer is gone?): communicator aborted",
                                       (unsigned long long)limit_ms);
                    std::this_thread::sleep_for(std::chrono::microseconds(20));
                }
            }
            CNIIC_HIP_TRY(c, hipEventSynchronize(c->poll_ev[slot ^ 1]));
            if (ring) {  // the record the previous batch's last launch wrote: complete before its event, untouched for kPollRing launches
                const volatile PollRec *r = reinterpret_cast<const volatile PollRec *>(c->pinned.as<uint8_t>() + ring_offset()) + last_prev % kPollRing;
                if (r->seq != last_prev) return c->fail(CNIIC_ERR_HIP, "kmeans: launch %u left no state record (found %u)", last_prev, r->seq);
                KmDevState t{};
                t.done = r->done; t.iter = r->iter; t.moved_last = r->moved_last; t.reseeds = r->reseeds; t.active = r->active; t.pair_evals = r->pair_evals;
                *h = t;
            } else if (mapped) {  // at least as new as that batch; the flag is read first, the scalars it guards after it
                volatile KmDevState *m = &slots[2];
                KmDevState t{};
                t.done = m->done;
                std::atomic_thread_fence(std::memory_order_acquire);
                t.iter = m->iter; t.moved_last = m->moved_last; t.reseeds = m->reseeds; t.active = m->active; t.pair_evals = m->pair_evals;
                *h = t;
            } else {
                *h = slots[slot ^ 1];
            }
        }
        slot ^= 1;
        pending = 1;
        last_prev = last_launch;
        return CNIIC_OK;
    }
    // state after everything enqueued so far
    int drain(KmDevState *h) {
        KmDevState *slots = c->pinned.as<KmDevState>();
        CNIIC_HIP_TRY(c, hipEventSynchronize(c->poll_ev[slot ^ 1]));
        *h = slots[slot ^ 1];
        return CNIIC_OK;
    }
};

// ---- host-side stage marks (CNIIC_TRACE_HOST=1): where an ABI call spends its wall time ----
struct HostTrace {
    bool on;
    std::vector<std::pair<const char *, double>> marks;
    HostTrace() : on(test_env("CNIIC_TRACE_HOST") != nullptr) {}
    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void mark(const char *what) { if (on) marks.emplace_back(what, now()); }
    void dump() {
        if (!on || marks.empty()) return;
        for (size_t i = 1; i < marks.size(); i++) fprintf(stderr, "[host] %-28s %8.1f us\n", marks[i].first, marks[i].second - marks[i - 1].second);
        fprintf(stderr, "[host] %-28s %8.1f us\n", "total", marks.back().second - marks.front().second);
        marks.clear();
    }
};
HostTrace &host_trace();

// ---- kernel timing of the dominant kernels (HIP events on the ctx stream) ----
struct ScopedKernelTimer {
    Ctx        *c;
    const char *name;
    bool        on;
    // stop() waits for the GPU, so stage timers are off unless asked for (CNIIC_KM_PROFILE in the call's
    // options, or CNIIC_KERNEL_TIMERS=1 in the environment)
    ScopedKernelTimer(Ctx *ctx, const char *nm) : ScopedKernelTimer(ctx, nm, ctx->timers) {}
    ScopedKernelTimer(Ctx *ctx, const char *nm, bool enable) : c(ctx), name(nm), on(enable) {
        if (on) (void)hipEventRecord(c->ev0, c->stream);
    }
    // must be called after the launch; synchronises on the stop event
    void stop(uint64_t launches = 1) {
        if (!on) return;
        (void)hipEventRecord(c->ev1, c->stream);
        (void)hipEventSynchronize(c->ev1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
        KernelTime &kt = c->ktimes[name];
        kt.ms += ms;
        kt.launches += launches;
        on = false;
    }
};

// =========================================================================== device entry points
// (host launchers implemented in the .hip files)

// ---- k_hist.hip ----
// Dense-table histogram of packed keys.  table: u32[1<<bits], must be zero on entry.
int hist_rgb_dense(Ctx *c, const uint8_t *rgb_d, uint64_t npx, uint32_t *table_d);
int hist_syms_dense(Ctx *c, const uint32_t *syms_d, uint64_t n, uint32_t *table_d, uint32_t bits);
// Compaction of a dense count table into ascending (key,count) pairs (3-phase scan).
struct CompactPlan {
    DevBuf   blockoff, blockmax;
    uint64_t n_unique = 0;
    uint64_t max_count = 0;          // the largest count in the table (how many radix passes the leaves' sort by count needs)
    uint32_t bits = 0;
    const uint8_t *pages = nullptr;  // (optional) a flag per 4096-entry page: pages without one are skipped
};
// occupancy across ranks: nibble per key (k_hist.hip), and the index of all occupied keys built from the summed nibbles
int occupancy_pack(Ctx *c, const uint32_t *table_d, uint32_t *occ_d);  // u32[2^24] counts -> u32[2^21] nibble words
int gidx_build(Ctx *c, const uint32_t *occ_d, DevBuf &bits, DevBuf &wprefix, uint64_t *U_h, DevBuf *total_keep = nullptr);
int gidx_finish(Ctx *c, uint32_t *wprefix_d, const uint32_t *blocktot_d, uint64_t *total_d);  // 256 blocks of 1024 words

// ---- k_points.hip: pixels partitioned by colour super-cell (large cluster-colors encodes) ----
struct SpPlan {
    uint64_t npx = 0, U = 0;     // pixels, distinct colours
    uint32_t nchunks = 0;
    DevBuf cnt, pre, bstart;     // pixels per (chunk, bucket), those in earlier chunks, first entry of every bucket
    DevBuf part, prank;          // u16 per pixel: colour inside its bucket (bucket order), place in its chunk's bucket-sorted order (pixel order)
    DevBuf cell_count;           // distinct colours per K-means cell
    DevBuf sstart, sbin, scnt;   // per bucket: its distinct colours (colour inside the bucket, pixel count) staged in cell-major order
    DevBuf bits, wprefix;        // occupancy bitmap of the 2^24 colours + popcount prefix (GIdx)
    DevBuf total;                // u64 on the device: distinct colours (the kernels of the set-up read it there)
};
int sp_build(Ctx *c, const uint8_t *rgb_d, uint64_t npx, SpPlan *plan, bool hist_only = false);  // asynchronous: the count arrives with sp_wait_count
struct KmFront;  // kmeans_rgbw.hpp: the K-means' set-up dispatches, left to the caller
// behind sp_build(hist_only): the rest of it, the K-means' set-up and the emit, in three launches (fused) or as ever
int sp_front(Ctx *c, SpPlan *plan, const KmFront &f, uint32_t *ckeys_d, uint32_t *cweight_d, void *labels_d, bool wide, bool fused,
             bool emit = true /* false (fused only): no emit -- the persistent launch reads the staging, km_rgbw_points_from_staging */,
             bool count_copy = true /* false (fused only): the count's copy is the caller's to enqueue, sp_enqueue_count */);
int sp_enqueue_count(Ctx *c, SpPlan *plan);                               // the count's copy to the host and its event, behind what is enqueued
bool sp_front_fits(const KmFront &f);
int sp_wait_count(Ctx *c, SpPlan *plan);                                  // plan->U on the host (waits for its copy only)
// distinct colours, counts, initial labels -> the K-means state's cell-major arrays; (gbits, gprefix, Ug): index of the point list
int sp_emit(Ctx *c, const SpPlan *plan, const uint32_t *cell_start_d, uint32_t *ckeys_d, uint32_t *cweight_d, void *labels_d, bool wide,
            uint32_t K, const void *gbits_d, const uint32_t *gprefix_d, uint64_t Ug, const uint64_t *Ug_dev /* overrides Ug when set */);
int sp_occupancy(Ctx *c, const SpPlan *plan, uint32_t *occ_d);  // this image's colours as summable nibbles, u32[2^21]
// final cell-major labels -> label of every pixel, image order
int sp_pixel_labels(Ctx *c, const SpPlan *plan, const uint8_t *rgb_d, const uint32_t *cell_start_d, const uint32_t *ckeys_d,
                    const void *labels_d, bool wide, void *pixlab_d);
// ... in its two steps (partition order, then image order), and the second step fused with the Huffman pack for narrow labels (k_sp_pixpack)
int sp_part_labels(Ctx *c, const SpPlan *plan, const uint32_t *cell_start_d, const uint32_t *ckeys_d, const void *labels_d, bool wide, DevBuf &partlab,
                   DevBuf *look /* optional: sp_pixpack's ticket and look-back words, zeroed by the kernel */,
                   bool staged = false /* the colours from plan's staging, not from ckeys_d (a state whose arrays were not emitted) */);
int sp_pixlab(Ctx *c, const SpPlan *plan, const uint8_t *rgb_d, const void *partlab_d, bool wide, void *pixlab_d);
int sp_pixpack(Ctx *c, const SpPlan *plan, const void *partlab_d, DevBuf &look, const uint8_t *upl_h, uint32_t hdr_bytes, uint8_t *out_d, uint64_t *done_h);
// the block cc_finish fills for sp_pixpack (pinned: kPuCcUpload; the kernel reads it there): the K <= 256 clusters' codes and lengths, the stream's header
constexpr uint32_t kCcUpCode = 0, kCcUpLen = 2048, kCcUpHdrBytes = 2304 /* u32 */, kCcUpHdr = 2312 /* zero-padded to whole words */, kCcUpBytes = 8192;
// cell_count_d (optional, 24-bit tables): zeroed u32[32768] receiving the occupied bins per K-means colour cell
int hist_compact_count(Ctx *c, const uint32_t *table_d, uint32_t bits, CompactPlan *plan, uint32_t *cell_count_d = nullptr,
                       const uint8_t *pages_d = nullptr);
// After this call the table holds, for every occupied bin, its RANK (index into the compacted
// list) + 1; empty bins stay 0.  Outputs are optional device arrays of plan->n_unique entries.
int hist_compact_write(Ctx *c, uint32_t *table_d, const CompactPlan *plan, uint32_t *keys_d, uint64_t *counts_d,
                       uint32_t *weights_d);
int dense_table(Ctx *c, uint32_t bits, uint32_t **table_d);  // zeroed scratch table of the ctx

// ---- k_kmeans_rgbw.hip ----
struct KmRgbwState;  // opaque device state of one rgbw K-means problem
int km_rgbw_create(Ctx *c, const uint32_t *keys_d, const uint32_t *weight_d, uint64_t U, uint32_t shard,
                   uint32_t nshards, uint32_t K, const cniic_kmeans_opts *opts, void *partials_dev,
                   const uint32_t *rank_table_d /* dense key -> rank+1 table, or null */, KmRgbwState **out,
                   const uint32_t *cell_count_d = nullptr /* with rank_table_d: points per cell, if already counted */,
                   const void *gbits_d = nullptr, const uint32_t *gprefix_d = nullptr, uint64_t Ug = 0
                   /* the points are this rank's share of Ug colours: positions in the list of all occupied keys */,
                   bool points_follow = false /* keys_d / weight_d null: the caller writes the cell-major arrays (sp_emit) */,
                   const uint64_t *points_dev = nullptr /* with points_follow: U and Ug are upper bounds, the count is here
                                                           on the device; km_rgbw_set_points before anything else */);
int km_rgbw_set_points(KmRgbwState *s, uint64_t U, uint64_t Ulist = 0 /* 0: the points are the whole list */);
void km_rgbw_cell_arrays(KmRgbwState *s, uint32_t **cell_start_d, uint32_t **ckeys_d, uint32_t **cweight_d);
void km_rgbw_destroy(KmRgbwState *s);
int km_rgbw_set_state(KmRgbwState *s, const uint8_t *centroids_h, const uint32_t *labels_d_u32);
// kmeans::cluster from K centroids of the caller's (host, K x 3 bytes) instead of init_centroids; before the first assign / run only (BAD_ARG after)
int km_rgbw_set_centroids(KmRgbwState *s, const uint8_t *init_h);
int km_rgbw_assign(KmRgbwState *s);                       // async: assign + partial sums -> partials
int km_rgbw_update(KmRgbwState *s);                       // async: centroids from partials
// ---- comm.cpp: RCCL on the context's stream (bound at run time) ----
struct Comm;
int comm_unique_id(uint8_t *id128);
int comm_create(Ctx *c, const uint8_t *id128, uint32_t rank, uint32_t nranks, Comm **out);
int comm_create_host(Ctx *c, uint32_t rank, uint32_t nranks, int32_t (*fn)(void *, void *, uint64_t, int32_t), void *user, Comm **out);
void comm_destroy(Comm *cm);
Ctx *comm_ctx(Comm *cm);
uint32_t comm_size(const Comm *cm);
int comm_all_reduce(Comm *cm, void *buf_d, uint64_t count, int kind);  // in place, sum; kind 0 = u8, 1 = u32, 2 = u64
void comm_abort(Comm *cm);        // after a failure on this rank: the peers' collectives end with an error instead of hanging
int comm_async_error(Comm *cm);   // CNIIC_OK while healthy; an error once this rank aborted or the transport reports a peer's failure
uint64_t comm_timeout_ms(const Comm *cm);           // deadline of a loop's wait for a batch with collectives (0: none)
void comm_set_timeout_ms(Comm *cm, uint64_t ms);
int comm_create_mailbox(Ctx *c, uint32_t rank, uint32_t nranks, uint64_t max_bytes, uint8_t *handle64, Comm **out);
int comm_connect_mailbox(Comm *cm, const uint8_t *handles);

// ---- k_mailbox.hip: the one-shot exchange (every rank writes its buffer into a slot of every peer's mailbox)
struct Mailbox;
int mailbox_create(Ctx *c, uint32_t rank, uint32_t nranks, uint64_t cap_bytes, uint8_t *handle64, Mailbox **out);
int mailbox_connect(Mailbox *m, const uint8_t *handles);  // nranks x 64 bytes, in rank order
int mailbox_all_reduce(Mailbox *m, void *buf_d, uint64_t count, int kind, uint64_t timeout_ms);
int mailbox_status(const Mailbox *m);  // 0 healthy, 1 a wait ran out, 2 a peer aborted
void mailbox_abort(Mailbox *m);
void mailbox_destroy(Mailbox *m);

constexpr int kKmRetry = 1000;    // km_rgbw_result_end after a deferred run: the persistent launch had given up, the launch-per-iteration loop has run since -- what the
                                  // caller enqueued on the labels must be enqueued again (never returned through the C ABI)
int km_rgbw_run(KmRgbwState *s, Comm *cm = nullptr, bool may_defer = false);   // full loop to convergence; with cm the partial sums are all-reduced in-stream each iteration;
                                                           // may_defer: the caller goes on to km_rgbw_result_begin / _end (which may answer kKmRetry, kmeans_rgbw.hpp) and wants no wait in between
int km_rgbw_poll_changed(KmRgbwState *s, uint64_t *changed);  // syncs
int km_rgbw_poll(KmRgbwState *s, cniic_kmeans_stats *st, uint32_t *done);  // syncs
bool km_rgbw_run_stats(KmRgbwState *s, cniic_kmeans_stats *st);  // of the last km_rgbw_run; no stream work
int km_rgbw_poll_lagged(KmRgbwState *s, cniic_kmeans_stats *st, uint32_t *done, uint32_t *have);  // waits for the previous call's copy only
int km_rgbw_result(KmRgbwState *s, uint8_t *centroids_h, uint32_t *labels_d_u32, uint64_t *members_h,
                   uint64_t *wsum_h, cniic_kmeans_stats *stats);
// the same in two halves: _begin enqueues the copy of the result block, _end waits for it (work enqueued
// in between overlaps the wait and whatever the host does with the result)
int km_rgbw_result_begin(KmRgbwState *s);
int km_rgbw_result_end(KmRgbwState *s, uint8_t *centroids_h, uint64_t *members_h, uint64_t *wsum_h, cniic_kmeans_stats *stats);
int km_rgbw_time_assign(KmRgbwState *s, int reps, double *ms_per_launch);
int km_rgbw_partials(KmRgbwState *s, uint64_t *sums_h, uint64_t *wsum_h, uint64_t *members_h, uint64_t *changed_h);
void *km_rgbw_partials_dev(KmRgbwState *s);
const uint32_t *km_rgbw_centroids_dev(KmRgbwState *s);
bool km_rgbw_is_wide(KmRgbwState *s);                     // u16 labels (K > 256) instead of u8
int km_rgbw_labels_canonical(KmRgbwState *s, void *dst_d); // u8/u16 labels of all points, canonical order
void *km_rgbw_labels_internal(KmRgbwState *s, uint64_t *elem_bytes);
int km_rgbw_fold_initial(KmRgbwState *s);
// sharded runs: labels of this shard's cells (zeros elsewhere) out of / merged labels into the state
int km_rgbw_export_labels(KmRgbwState *s, void *dst_d);
int km_rgbw_import_labels(KmRgbwState *s, const void *src_d);
uint64_t km_rgbw_points(KmRgbwState *s);

// ---- k_kmeans_xyrgb.hip ----
// init_h (optional; host, K entries with x < w and y < h): the run starts from these centroids instead of init_centroids (kmeans.rs:101-108)
int km_xyrgb_run(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t K,
                 const cniic_kmeans_opts *opts, cniic_colorpos *centroids_h, uint32_t *labels_d_u32,
                 uint64_t *members_h, cniic_kmeans_stats *stats, const cniic_colorpos *init_h = nullptr);
int km_xyrgb_run_wide(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t K, const cniic_kmeans_opts *opts, cniic_colorpos *centroids_h,
                      uint32_t *labels_d_u32, uint64_t *members_h, cniic_kmeans_stats *stats, const cniic_colorpos *init_h = nullptr);   // k_kmeans_wide.hip: any K, any sides
int km_xyrgb_step(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t K,
                  const cniic_colorpos *centroids_h, uint32_t *labels_d_u32, uint64_t *sums_h,
                  uint64_t *wsum_h, uint64_t *members_h, uint64_t *changed_h, const cniic_kmeans_opts *opts);

// ---- k_misc.hip ----
// per-pixel colour -> centroid colour through the rank table left by hist_compact
int remap_rgb(Ctx *c, const uint8_t *rgb_d, uint64_t npx, const uint32_t *rank_table_d,
              const uint32_t *lut_rgb_d /* packed centroid colour per unique colour rank */, uint8_t *out_d);
int expand_codes_by_label(Ctx *c, const uint8_t *labels8_d, const uint16_t *labels16_d, uint64_t U, const uint8_t *clen_d,
                          const uint64_t *ccode_d, uint8_t *len_d, uint64_t *code_d);
// (local_counts_d == nullptr: the weights come from weights_d[i] instead of local_counts_d[keys_d[i]])
int local_cluster_weights(Ctx *c, const uint32_t *keys_d, const void *labels_d, bool wide, uint64_t U,
                          const uint32_t *local_counts_d, uint32_t K, uint64_t *out_d, const uint32_t *weights_d = nullptr);
int label_lut(Ctx *c, const uint32_t *labels_d, uint64_t U, const uint32_t *cent_d, uint32_t *lut_d);
int rank_from_keys(Ctx *c, const uint32_t *keys_d, uint64_t U, uint32_t *table_d);
int voronoi_paint(Ctx *c, const cniic_colorpos *cent_d, uint32_t K, uint32_t w, uint32_t h, uint8_t *out_d, bool small_coords = false);
int mse_rgb(Ctx *c, const uint8_t *a_d, const uint8_t *b_d, uint64_t npx, double *mse_h);
int mse_rgb_batch(Ctx *c, const uint8_t *a_d, const uint8_t *b_d, uint64_t npx, uint32_t frames, double *mse_h);  // F pairs, one result each
// pairs of different sizes in one launch: pair f is npx[f] pixels at a_d + a_off[f], b_d + b_off[f] (host arrays of `frames` entries)
int mse_rgb_batch_var(Ctx *c, const uint8_t *a_d, const uint8_t *b_d, const uint64_t *a_off, const uint64_t *b_off, const uint64_t *npx,
                      uint32_t frames, double *mse_h);
int synth_image(Ctx *c, int kind, uint64_t seed, uint32_t w, uint32_t h, uint8_t *out_d);

// ---- k_surface.hip: pitched surfaces <-> packed RGB24 frames (cniic_frames_from_surfaces / cniic_frames_to_surfaces) ----
// a validated cniic_surface (offsets from the surface side's device pointer) + where its packed frame starts (from the packed side's)
struct SurfFrame { uint64_t off, pitch, off_uv, pitch_uv, rgb_off; uint32_t w, h; int32_t format, matrix; };
// one launch for all frames; to_surfaces: in_d = the packed frames, out_d = the surfaces (alpha: the fourth byte of RGBA8 / BGRA8)
int surf_convert(Ctx *c, bool to_surfaces, const uint8_t *in_d, uint8_t *out_d, const SurfFrame *fr_h, uint32_t frames, uint32_t alpha);
int rgb_to_keys(Ctx *c, const uint8_t *rgb_d, uint64_t npx, uint32_t *keys_d);

// ---- colour-space cells of the cluster-colors K-means (numbering: cell_of in device_utils.hpp) ----
constexpr int kCellShift = 3;                                   // 2^shift colours per cell side
constexpr uint32_t kCellsPerDim = 256 >> kCellShift;           // 32
constexpr uint32_t kNumCells = kCellsPerDim * kCellsPerDim * kCellsPerDim;  // 32768

// ---- k_hdecode.hip: parallel Huffman decode (self-synchronising subsequences), keys -> pixels, FromDiff as a scan ----
struct LeafTable;
struct UdSums { DevBuf buf; bool filled = false; };   // FromDiff's channel sums per 4096 symbols, added up by the decoder while it writes them (k_hdecode.hip)
// payload in host memory, or (payload_dev) anywhere in HBM; mode 0: out_d = nsyms packed keys (u32, 16-byte aligned), mode 1: nsyms RGB
// triples (4-byte aligned).  status: 0 ok, 1 stream ends early, 2 did not settle (decode on the host)
int huff_decode_dev(Ctx *c, const LeafTable &lt, const uint8_t *payload, bool payload_dev, uint64_t payload_bytes, uint64_t nsyms,
                    int mode, void *out_d, int *status, UdSums *sums = nullptr);
// many RGB-symbol streams (mode 1) in one set of launches (k_hdecode.hip, cniic_codec_decode_batch): per frame the host's leaf table
// (not too_deep, codes of at most 32 bits, fewer than 2^20 leaves), the payload in HBM, nsyms > 0 and a 4-byte aligned output in HBM.
// status (out): 0 = decoded, 1 = the stream ends early, 2 = did not settle (the caller decodes that frame again on its own)
struct HdBatchFrame {
    const LeafTable *lt = nullptr;
    const uint8_t *payload = nullptr;
    uint64_t payload_bytes = 0, nsyms = 0;
    uint8_t *out_d = nullptr;
    int status = 0;
};
int huff_decode_batch_dev(Ctx *c, std::vector<HdBatchFrame> &frames);
// ... with the table of leaves already in HBM (code u64[n] | key u32[n] at off_key | len u8[n] at off_len)
int huff_decode_tables_dev(Ctx *c, const uint8_t *tab_d, uint64_t n, uint64_t off_key, uint64_t off_len, uint32_t max_len, uint32_t first_key,
                           const uint8_t *payload, bool payload_dev, uint64_t payload_bytes, uint64_t nsyms, int mode, void *out_d, int *status, UdSums *sums = nullptr);
// k_trieparse.hip: Dec::deserialize on the GPU (decoders of millions of leaves).  status: 0 ok, 1 malformed / truncated, 2 too deep
int huff_parse_leaves_dev(Ctx *c, int sym_kind, const uint8_t *stream_d, uint64_t nbytes, uint64_t pos0, DevBuf *tab, uint64_t *n_leaves,
                          uint64_t *off_key, uint64_t *off_len, uint32_t *max_len, uint64_t *payload_pos, int *status);
int keys_to_rgb(Ctx *c, const uint32_t *keys_d, uint64_t n, uint8_t *rgb_d);
int delta_undiff_dev(Ctx *c, const uint32_t *keys_d, uint64_t n, uint8_t *lin_d, uint32_t *bad_h);
int delta_undiff_scatter_dev(Ctx *c, const uint32_t *keys_d, uint32_t w, uint32_t h, uint8_t *rgb_out_d, uint32_t *bad_h, UdSums *sums = nullptr);  // + the walk along the scan

// ---- k_rle.hip: exact run-length coding of a linearised image (hilbertc.rs:100-196) ----
struct RlePlan { uint64_t n = 0, nruns = 0; uint32_t nchunks = 0; DevBuf flags, run_off; };
int rle_plan(Ctx *c, const uint8_t *lin_d, uint64_t n, RlePlan *plan);                       // counts the runs (syncs)
int rle_emit(Ctx *c, const uint8_t *lin_d, const RlePlan *plan, uint32_t *out_words_d);      // 12-byte records
int rle_expand_dev(Ctx *c, const uint8_t *rec_d, uint64_t R, uint64_t tail_bytes, uint64_t n, uint8_t *lin_d, int *status);  // RleDecoder
// ... of many streams in one set of launches (cniic_codec_decode_batch): enqueued, not waited for; the statuses after the caller's wait
struct RleBatchFrame {
    const uint8_t *rec_d = nullptr;   // the complete records in HBM, any alignment
    uint64_t R = 0, tail_bytes = 0, n = 0;   // 0 < n < 2^32
    uint8_t *lin_d = nullptr;         // n colours in scan order (16-byte aligned)
    int status = 0;                   // 0 ok, 1 bad, as rle_expand_dev's (a bad frame's colours are zeros)
};
struct RleBatchScratch { DevBuf buf; std::vector<uint8_t> table, verdicts; };   // kept by the caller until it has waited for the stream
int rle_expand_batch_dev(Ctx *c, std::vector<RleBatchFrame> &frames, RleBatchScratch *keep);
void rle_expand_batch_status(std::vector<RleBatchFrame> &frames, const RleBatchScratch *keep);
int rle_offsets(Ctx *c, const uint32_t *chunk_runs_d, uint32_t nchunks, uint64_t *run_off_d, uint64_t *total_d);  // runs before each chunk
// ---- k_rle_approx.hip: run-length coding with the running-average test, d != 0 (hilbertc.rs:200-299); same plan, same records ----
double rla_threshold(double d);                                                                // largest s with sqrt_rn(s) <= d
int rle_approx_plan(Ctx *c, const uint8_t *lin_d, uint64_t n, double d, RlePlan *plan);        // counts the runs (syncs)
int rle_approx_emit(Ctx *c, const uint8_t *lin_d, const RlePlan *plan, uint32_t *out_words_d);  // 12-byte records, average colours

// the scan of the maps (k_rla_compose / k_rla_down over levels of 64): maps0_d holds a map of 256 u8 per piece -- the offset in the next
// piece at which a chain that enters this piece at offset e (0..254) arrives; *ent0_d: every piece's entry offset, the chain starting at
// offset 0 of piece 0.  Enqueued; `keep` holds the levels until the caller is done with *ent0_d.
struct RlaLevels { std::vector<DevBuf> maps, ent; };
int rla_chain_entries(Ctx *c, const uint8_t *maps0_d, uint32_t npieces, RlaLevels *keep, const uint8_t **ent0_d);

// ---- k_zipdict.hip: the dictionary coder of zip(dict) (src/zip/dict.rs) once its dictionary is full; zipdict.cpp has the part before ----
// an edge of the frozen trie in the open-addressed table: key = node << 8 | byte (kZdEmpty: free slot), child node (0: none), symbol
// (kZdNoSym: the text that ends here has none)
struct ZdEdge { uint32_t key, child, sym, pad; };
constexpr uint32_t kZdEmpty = 0xffffffffu, kZdNoSym = 0xffffu;
constexpr uint32_t kZdMaxNodes = (1u << 24) - 2;   // node ids must leave room for the byte in the key (and for kZdEmpty)
// k_zd_match walks an entry's whole length at every position where the text spells it: a stretch of one colour behind the hand-over costs
// its length times the longest entry.  Entries beyond this (a flat stretch of 64 KB of text, six rows of a 1024-wide image, BEFORE the
// dictionary filled) keep the coder on the host to the end of the text.
constexpr uint64_t kZdMaxEntry = 32768;
constexpr uint64_t kZdSat = 1ull << 62;            // where the decoder's sums of text lengths stop growing
constexpr uint64_t kZdLenClamp = 1ull << 38;       // ... and what a single text's length is cut to in the device table (no buffer is that long)
__host__ __device__ inline uint32_t zd_hash(uint32_t key, uint32_t bits) { return (key * 2654435761u) >> (32 - bits); }
// text = [w, h as u32 when dims] + 11 bytes per pixel (u64 3, r, g, b); and back: *first_bad_h = the first record whose length is not 3 (npx: none)
// (stage: the stage timer's name -- zip(back) shares both kernels and times them under names of its own)
int zd_serialize(Ctx *c, const uint8_t *px_d, uint64_t npx, bool dims, uint32_t w, uint32_t h, uint8_t *text_d, const char *stage = "zd_serialize");
int zd_unserialize(Ctx *c, const uint8_t *rec_d, uint64_t npx, uint8_t *px_d, uint64_t *first_bad_h, const char *stage = nullptr);
// the greedy parse of text_d[P0, N) against the frozen trie (table_h: 2^bits edges, at most half of them used; max_entry: its longest text)
struct ZdFrozen { uint64_t M = 0, nsyms = 0; uint32_t nchunks = 0; bool windowed = false; DevBuf sym, mark, chunk_off; };
int zd_frozen_plan(Ctx *c, const uint8_t *text_d, uint64_t N, uint64_t P0, const ZdEdge *table_h, uint32_t bits, uint64_t max_entry, ZdFrozen *plan);  // counts the symbols (syncs)
int zd_frozen_emit(Ctx *c, const ZdFrozen *plan, uint16_t *out_d);   // nsyms symbols, and 0xFFFF behind an odd number of them
// the texts of nsym symbols read with a full dictionary (syms_d: 2 nsym bytes in HBM, any alignment; tab_*_h: 65536 entries each)
struct ZdExpand { uint64_t nsym = 0, total = 0; uint32_t nchunks = 0; const uint8_t *syms_d = nullptr; DevBuf tab, chunk_off; };
int zd_expand_plan(Ctx *c, const uint8_t *syms_d, uint64_t nsym, const uint64_t *tab_off_h, const uint64_t *tab_len_h, ZdExpand *plan);   // total (saturating; syncs)
int zd_expand_copy(Ctx *c, const ZdExpand *plan, uint64_t base, uint8_t *out_d, uint64_t limit);

// ---- k_zipback.hip: the look-back coder of zip(back) (src/zip/back.rs), one workgroup per stream; zipback.cpp has the host side ----
// a stream of a call, in HBM: encode reads the text in[0, n) and writes symbols to out[0, cap); decode reads the symbols in[0, n) and
// writes text to out[0, cap), whole symbols while fewer than `need` bytes are there
struct ZbStream { const uint8_t *in; uint64_t n; uint8_t *out; uint64_t cap, need; };
// where a stream stands between two launches.  encode: p bytes of text accepted, o bytes of stream made (counted behind cap too), e of
// them an explicit run whose header is still open.  decode: p bytes of stream read, o bytes of text made.
struct ZbState { uint64_t p, o; uint32_t e, status; };
// status: over for good unless kZbRunning.  BadExplicit / BadLookback: encode -- a length of 32 768 or more, which the reference's header
// cannot say (back.rs:45); decode -- an explicit symbol cut short (:97), a `back` behind the start of the text (:466)
constexpr uint32_t kZbRunning = 0, kZbDone = 1, kZbBadExplicit = 2, kZbBadLookback = 3;
// A launch takes every stream this far at most (NOTES.md L has the measurements): bytes of text accepted in encode; bytes of stream
// read, and bytes of text made, in decode.
constexpr uint64_t kZbEncodeSlice = 256 << 10, kZbDecodeSlice = 4 << 20;
// the most text n bytes of stream can spell (a look-back of four bytes: 32 767), and the most stream n bytes of text can take (two
// explicit bytes and a look-back of six: eight bytes for eight; two more for a last explicit symbol)
inline uint64_t zb_text_bound(uint64_t n) { return n < (1ull << 48) ? (n / 4 + 1) * 32767 : ~0ull; }
inline uint64_t zb_stream_bound(uint64_t n) { return n + n / 4 + 16; }
int zb_encode_streams(Ctx *c, const ZbStream *streams_h, uint32_t F, ZbState *states_h);   // to the end of every stream (syncs)
int zb_decode_streams(Ctx *c, const ZbStream *streams_h, uint32_t F, ZbState *states_h);
// k_zipback_par.hip: one stream decoded by the whole GPU (zb_par.hpp), to the state k_zb_decode would leave; in / out: HBM, 1 <= n < 2^32.
// handed: the stream is the serial kernel's after all (min(made, cap) of 2^32 or more, or text tables above kZbParScratchMax; pointers
// left after round_cap <= 32 jump rounds)
// and what lies below cap is to be written again.  zb_par_stream_scratch: the bytes of its tables before the text's are known.
// the classes that take it: calls of ONE stream, streams of 512 KiB or more.  Measured (profiles/zip_back_probe.json, NOTES AW): single
// decodes of photo-like and noise images from 462 993 / 510 257 bytes of stream (256 x 256) to 7.5 / 8.1 MB (1024 x 1024) ran in
// 0.39 - 1.5 ms against the serial walk's 61 - 1087 ms, the ranges of 5 runs far apart for both contents.  Calls of 8, 32 and 100
// streams of 148 - 450 KB won too (2.8 / 11 / 35 ms against 52 / 59 / 64) but were measured on photo-like frames only, and shorter
// streams not at all: they stay with the serial kernel.
constexpr uint32_t kZbParMaxStreams = 1;
constexpr uint64_t kZbParFloorBytes = 512 << 10;
// a stream whose tables (9 B per stream byte) would take more than this stays serial; one whose text tables (8 B per text byte below
// cap) would is handed back
constexpr uint64_t kZbParScratchMax = 8ull << 30;
uint64_t zb_par_stream_scratch(uint64_t n);
int zb_par_decode_stream(Ctx *c, const ZbStream &s, uint32_t round_cap, ZbState *st, uint32_t *rounds, bool *handed);

// ---- k_linearize.hip: hilbert.rs:10-32 linearize_rect / _small / _large, and the per-channel difference histogram of a linear stream ----
int linearize_count(int32_t method, uint32_t w, uint32_t h, uint64_t *npx);   // host only: pixels the method yields (CNIIC_LIN_*)
int linearize_as(Ctx *c, int32_t method, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out_d);   // out_d: linearize_count pixels
int channel_diff_hist(Ctx *c, const uint8_t *lin_d, uint64_t npx, uint64_t *counts_d);   // counts_d: u64[3][511]

// ---- k_hilbert.hip ----
int hilbert_xy(Ctx *c, uint32_t w, uint32_t h, uint32_t *xy_d);
int hilbert_linearize(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out_d);
// gather + delta; syms_d (packed SIGNED keys, may be null) and/or histogram into table_d (u32[2^27], may be null)
int hilbert_delta(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t *syms_d, uint32_t *table_d);
int hilbert_scatter(Ctx *c, const uint8_t *lin_d, uint32_t w, uint32_t h, uint8_t *rgb_out_d);
int scan_inject(Ctx *c, uint32_t w, uint32_t h, const uint32_t *xy, bool xy_dev);   // cniic_ctx_set_scan (xy == null: the built-in scan again)
int hilbert_undiff_scatter(Ctx *c, const uint32_t *keys_d, const int32_t *chunk_off_d, uint32_t w, uint32_t h, uint8_t *rgb_out_d, uint32_t *bad_d, bool *fused);

// ---- k_delta.hip: the `delta` encoder's passes over a 16-bit symbol stream ----
constexpr uint32_t kPageShift = 12;  // a page of a dense table = the 4096 entries one block of the compaction reads
int delta_table(Ctx *c, uint32_t **table_d, uint8_t **pages_d);  // the context's clean 2^27-bin table + page flags
int delta_table_clean(Ctx *c);                                   // touched pages back to zero (enqueued)
uint64_t delta_stream_len(uint64_t n);                           // u16 entries of the symbol stream of n pixels
int delta_gather_hist(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint16_t *hot16_d, uint32_t *table_d, uint8_t *pages_d,
                      uint32_t *coldkeys_d, uint8_t *chunk_cold_d, uint32_t *overflow_d);
struct DeltaPackScratch { DevBuf cb, co, edge, hot, hotlen; };
int delta_pack16_count(Ctx *c, const uint16_t *hot16_d, uint64_t n, uint32_t *coldkeys_d, const uint8_t *chunk_cold_d, uint32_t *dense_d,
                       const uint32_t *keys_d, const uint8_t *len_d, const uint64_t *code_d, uint64_t U, uint64_t *total_d, DeltaPackScratch *keep);
int delta_pack16_write(Ctx *c, const uint16_t *hot16_d, uint64_t n, const uint32_t *coldkeys_d, const uint8_t *len_d, const uint64_t *code_d, uint8_t *out_d,
                       uint64_t bit_base, DeltaPackScratch *keep);

// ---- k_huff.hip ----
// the leaves count << 32 | rank sorted by (count, rank): stable radix sort (see k_huff.hip); the result is in *out_d = buf_a or buf_b
int huff_sort_leaves_dev(Ctx *c, const uint64_t *counts_d, uint32_t n, uint64_t max_count, uint64_t *buf_a, uint64_t *buf_b, uint64_t **out_d);
int huff_sort_u64(Ctx *c, uint64_t *buf_a, uint64_t *buf_b, uint32_t n, uint32_t lo_bit, uint64_t **out_d);
// the tree, the codes and every leaf's place in the serialised decoder from the sorted leaves, the host merging RUNS of equal count only
int huff_tree_from_runs(Ctx *c, const uint64_t *sorted_d, const uint64_t *counts_d, uint32_t n, int sym_kind, uint8_t *len_d, uint64_t *code_d,
                        uint64_t *off_d, uint64_t *nbits_h, bool *built);
// codes and the serialised decoder of a tree the host built, for large alphabets (see k_huff.hip)
int huff_tree_codes(Ctx *c, const uint32_t *left_d, const uint32_t *right_d, const uint32_t *nleaves_d, const uint64_t *counts_d, uint32_t n,
                    uint32_t root, int sym_kind, uint8_t *len_d, uint64_t *code_d, uint64_t *off_d, uint64_t *totals_d);
int huff_tree_serialize_dev(Ctx *c, const uint32_t *keys_d, const uint64_t *off_d, uint32_t n, int sym_kind, uint8_t *trie_d, uint64_t trie_bytes);
// chunk_off[i] = exclusive prefix (u64) of chunk_bits[0 .. nchunks); *total_d = the sum
int pack_scan(Ctx *c, const uint32_t *chunk_bits_d, uint32_t nchunks, uint64_t *chunk_off_d, uint64_t *total_d);
uint32_t pack_img_cap();  // tests: CNIIC_TEST_PACK_IMG_WORDS caps the packs' LDS bit image
// MSB-first bit-pack of n symbols at bit offset bit_base of out_d (4-byte aligned, pre-zeroed,
// large enough; bytes before bit_base may already hold the stream header).
// Generic path: symbol -> rank (dense table left by the compaction) -> len_d / code_d per rank.
int huff_pack_keys(Ctx *c, const uint32_t *keys_or_null_d, const uint8_t *rgb_or_null_d, uint64_t n,
                   const uint32_t *rank_table_d, const uint8_t *len_d, const uint64_t *code_d,
                   uint8_t *out_d, uint64_t bit_base, uint64_t *nbits_h);
// the same in two steps: the symbols' ranks as a stream (needs no code: runs while the host builds the tree), then the pack
int huff_rank_stream(Ctx *c, const uint32_t *keys_or_null_d, const uint8_t *rgb_or_null_d, uint64_t n, const uint32_t *rank_table_d,
                     uint32_t *ranks_d, bool one_based);
int huff_pack_ranks(Ctx *c, const uint32_t *ranks_d, uint64_t n, const uint8_t *len_d, const uint64_t *code_d, uint8_t *out_d,
                    uint64_t bit_base, uint64_t *nbits_h);
// same result with one random read per symbol (needs every code length <= 26): the dense table is
// overwritten with len<<26|code per key; packed_d = n u32 of scratch (may alias syms)
int huff_pack_code32(Ctx *c, const uint32_t *syms_or_null_d, const uint8_t *rgb_or_null_d, uint64_t n, uint32_t *table_d,
                     const uint32_t *keys_d, const uint8_t *len_d, const uint64_t *code_d, uint64_t U, uint32_t *packed_d,
                     uint8_t *out_d, uint64_t bit_base, uint64_t *nbits_h);
// the same for SignedColor (`delta`) symbols: the (length, code) words of the cube of small differences sit in LDS
int huff_pack_code32_hot(Ctx *c, const uint32_t *syms_d, uint64_t n, uint32_t *dense_d, const uint32_t *keys_d, const uint8_t *len_d,
                         const uint64_t *code_d, uint64_t U, uint32_t *packed_d, uint8_t *out_d, uint64_t bit_base, uint64_t *nbits_h);
// cluster-colors path: pixel -> cluster label through a dense colour->label table, codes per cluster
int pixel_labels(Ctx *c, const uint8_t *rgb_d, uint64_t n, const void *key2label_d, bool wide, void *pixlab_d);
int huff_pack_labels(Ctx *c, const void *pixlab_d, uint64_t n, bool wide, uint32_t K, const uint8_t *clen_d,
                     const uint64_t *ccode_d, uint8_t *out_d, uint64_t bit_base, uint64_t *nbits_h);
int scatter_labels_by_key(Ctx *c, const uint32_t *keys_d, const void *labels_d, bool wide, uint64_t U, void *key2label_d);
// a batch of equally sized frames sharing one palette: labels per (frame, cluster), and the label pack of every frame in one go
int frame_label_hist(Ctx *c, const void *pixlab_d, uint64_t npf, uint64_t lab_stride, uint32_t frames, bool wide, uint32_t K, uint32_t *out_d /* u32[frames][K] */);
int huff_pack_labels_frames(Ctx *c, const void *pixlab_d, uint64_t npf, uint64_t lab_stride, uint32_t frames, bool wide, uint32_t K, const uint8_t *clen_d,
                            const uint64_t *ccode_d, uint8_t *out_d, uint64_t stride, const uint64_t *bit_base_h, uint64_t *totals_h, const uint64_t *bit_base_d = nullptr);
// ---- a batch of frames of ANY sizes sharing one palette (cc_finish_frames_var).  One table row per frame, built on the host, uploaded once:
// every kernel of the route runs a 1-D grid over the chunks (or histogram blocks) of all frames and finds its frame by a binary search in
// chunk0 (hblock0); a block never spans two frames.
struct FrameVar {
    uint64_t npx;        // w h
    uint64_t lab_base;   // first label, in elements of the label buffer the pack reads: on a 16-byte boundary
    uint64_t src_base;   // first label where the pixel-label kernels wrote it: the pixels before this frame
    uint32_t chunk0;     // first pack chunk: the sum of ceil(npx / 4096) over the frames before
    uint32_t hblock0;    // first histogram block: the sum of ceil(npx / 2^16)
    uint32_t w, h;
};
constexpr uint32_t kFrameVarChunk = 4096, kFrameVarHistSpan = 1u << 16;   // (= kPackChunk, kHistSpan of k_huff.hip)
// the frame whose row of chunks (FIRST = &FrameVar::chunk0) or of histogram blocks (hblock0) holds block b: the LAST f with fr[f].*FIRST <= b
// (every frame has at least one pixel, so the firsts rise strictly; the loads depend on the block alone)
template <uint32_t FrameVar::*FIRST>
__device__ __forceinline__ uint32_t frame_of_block(const FrameVar *__restrict__ fr, uint32_t frames, uint32_t b) {
    uint32_t f = 0;
    for (uint32_t hi = frames; hi - f > 1;) {   // fr[f].*FIRST <= b < fr[hi].*FIRST
        const uint32_t mid = f + (hi - f) / 2;
        if (fr[mid].*FIRST <= b) f = mid; else hi = mid;
    }
    return f;
}
// the Huffman codes and stream headers of a batch's frames on the GPU (K <= 256; k_huff.hip k_frame_trees)
int frame_trees(Ctx *c, const uint32_t *cnt_d, const uint32_t *cent_d, uint32_t frames, uint32_t K, uint32_t w, uint32_t h, uint8_t *out_d, uint64_t stride,
                uint8_t *clen_d, uint64_t *ccode_d, uint64_t *bit_base_d, uint64_t *nbits_d, uint64_t *lens_d, uint32_t *err_d,
                const FrameVar *fr_d = nullptr /* frames of any sizes: w, h per frame from the table */,
                uint32_t pal_stride = 0 /* 0: the K entries at cent_d for every frame; K: frame f's own at cent_d + f K */);
int frame_labels_align_var(Ctx *c, const void *src_d, void *dst_d, const FrameVar *fr_d, uint32_t frames, uint32_t chunks, bool wide);
int frame_label_hist_var(Ctx *c, const void *labs_d, const FrameVar *fr_d, uint32_t frames, uint32_t hblocks, bool wide, uint32_t K, uint32_t *out_d /* u32[frames][K] */);
int huff_pack_labels_frames_var(Ctx *c, const void *labs_d, const FrameVar *fr_d, uint32_t frames, uint32_t chunks, bool wide, uint32_t K, const uint8_t *clen_d,
                                const uint64_t *ccode_d, uint8_t *out_d, uint64_t stride, const uint64_t *bit_base_h, uint64_t *totals_h, const uint64_t *bit_base_d = nullptr);
int sum_u32_dev(Ctx *c, const uint32_t *v_d, uint64_t n, uint64_t *out_d);   // *out_d = the sum of n u32
// ---- k_cc_small.hip: cluster-colors(K <= 256) of small frames, one workgroup per frame (cc_small.hpp has the arithmetic and the limits).
// A row per frame: its pixels (device memory, any alignment) and where its u8 labels go in labels_d (a multiple of 16; room for the
// pixel count rounded up to 16).  The frame's K centroids land at cent_d + row * K as 0xRRGGBB words.
struct CcSmallRow { const uint8_t *src; uint64_t lab_base; uint32_t w, h; };
struct CcSmallResult { uint32_t U, iterations, moved_last, reseeds, active, status; };   // status 1: U / K == 0, nothing else was computed
struct CcSmallPlace { uint64_t src_off; uint8_t *dst; uint64_t len; };                   // a stream in the tail's scratch, and where it belongs
int cc_small_run(Ctx *c, const CcSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint32_t K, uint64_t seed, uint64_t max_iters,
                 uint8_t *labels_d, uint32_t *cent_d, CcSmallResult *res_d);
int cc_small_place(Ctx *c, const CcSmallPlace *pl_d, uint32_t n, const uint8_t *scratch_d /* 16-byte aligned offsets, 16 spare bytes behind */);
// ---- k_delta_small.hip: `delta` of small frames, one workgroup per frame (delta_small.hpp has the arithmetic and the limits).  A row per
// frame: its pixels (device memory, any alignment).  Frame f's finished stream lands at scratch_d + f * sstride (sstride >= ds_stride of
// the largest frame, a multiple of 16), its length in res_d[f]; tmp_d holds 3 * tmp_px words per frame (tmp_px >= the largest frame's pixels).
struct DeltaSmallRow { const uint8_t *src; uint32_t w, h; };
struct DeltaSmallResult { uint32_t U, len; };   // distinct symbols, bytes of the stream
int delta_small_run(Ctx *c, const DeltaSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint8_t *scratch_d, uint64_t sstride,
                    uint32_t *tmp_d, uint64_t tmp_px, DeltaSmallResult *res_d);
// the same for `hufman` (k_huf_small, the same body over the pixels' colours; huf_small.hpp): sstride >= hs_stride(max_px)
int huf_small_run(Ctx *c, const DeltaSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint8_t *scratch_d, uint64_t sstride,
                  uint32_t *tmp_d, uint64_t tmp_px, DeltaSmallResult *res_d);
// ---- k_rle_small.hip: `hilbert(rle)` / `hilbert(rle(d))` of small frames, one workgroup per frame (rle_small.hpp has the arithmetic and
// the limits).  A row per frame: its pixels (device memory, any alignment).  Frame f's finished stream lands at scratch_d + f * sstride
// (sstride >= rs_stride of the largest frame, a multiple of 16), its runs and its length in res_d[f].  T, mode: rla_threshold(d) and
// rs_mode(d, T), the same for every frame of the launch.
struct RleSmallRow { const uint8_t *src; uint32_t w, h; };
struct RleSmallResult { uint32_t runs, len; };   // records, bytes of the stream
int rle_small_run(Ctx *c, const RleSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, double T, int mode, uint8_t *scratch_d, uint64_t sstride,
                  RleSmallResult *res_d);
// ---- k_zd_small.hip: `zip(dict)` of small frames, one workgroup per frame (zd_small.hpp has the arithmetic and the limits).  A row per
// frame: its pixels (device memory, any alignment).  Frame f's finished stream lands at scratch_d + f * sstride (sstride >= zs_stride of
// the largest frame's text, a multiple of 16), its trie in tables_d + (f << bits) (bits >= zs_table_bits of that text; zeroed here), its
// pairs, its length and its verdict (kZsOk, or kZsHandedBack: a match longer than giveup bytes, nothing of the stream is valid) in
// res_d[f].  spec: the bytes a speculating walk reads at most.
struct ZdSmallRow { const uint8_t *src; uint32_t w, h; };
struct ZdSmallResult { uint32_t pairs, len, verdict, finished; };   // ..., walks the commit finished behind the speculation's cap
int zd_small_run(Ctx *c, const ZdSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint32_t spec, uint32_t giveup, uint64_t *tables_d,
                 uint32_t bits, uint8_t *scratch_d, uint64_t sstride, ZdSmallResult *res_d);
// the same for Hilbert { compress: Zip } (k_hz_small, hz_small.hpp): sstride >= hz_stride, bits >= zs_table_bits of the largest frame's 11 n
// bytes of text; the stream in the slot is the 8 raw bytes of the dimensions and the pairs, len = 8 + 4 pairs
int hz_small_run(Ctx *c, const ZdSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint32_t spec, uint32_t giveup, uint64_t *tables_d,
                 uint32_t bits, uint8_t *scratch_d, uint64_t sstride, ZdSmallResult *res_d);
// ---- k_zd_small_dec.hip: the decode of small `zip(dict)` frames, one workgroup per frame from its pairs to its pixels (zd_small_dec.hpp
// has the arithmetic, the limits and the verdicts).  A row per frame: its stream (device memory, any alignment; len bytes, of which the
// kernel looks at `pairs` = min(len / 4, the pair cap) pairs), where its w x h x 3 image goes (device memory, any alignment; written whole
// and only with verdict kZsdOk), and whether the pair words are staged in LDS (the host says so where they fit).  lds_bytes: dynamic LDS of
// the launch, at least every row's zsd_lds_bytes(pairs, w h) + 4 pairs where staged, a multiple of 16, zd_small_dec_lds_max() at most.
// res_d[f]: the verdict and the numbers of its message (kZsdBadSymbol: a = the pair; kZsdShort: a of b bytes; kZsdBadRecord: a = the pixel).
struct ZdSmallDecRow { const uint8_t *stream; uint8_t *dst; uint64_t len; uint32_t pairs, w, h, staged; };
struct ZdSmallDecResult { uint32_t verdict, a, b, pad; };
uint32_t zd_small_dec_lds_max();
int zd_small_dec_run(Ctx *c, const ZdSmallDecRow *rows_d, uint32_t frames, uint32_t lds_bytes, uint32_t hops, uint32_t rounds, ZdSmallDecResult *res_d);
// the same for Hilbert { compress: Zip } (k_hz_small_dec, hz_small.hpp): stream / len are the PAIRS behind the 8 raw bytes of the dimensions,
// w and h what those bytes say; the verdicts are kHzdOk (the image is written whole, zeros where the text gives no colour), kHzdHandedBack,
// kHzdBadSymbol (a = the pair) and kHzdDangling; lds_bytes is hz_small_dec_lds_max() at most
uint32_t hz_small_dec_lds_max();
int hz_small_dec_run(Ctx *c, const ZdSmallDecRow *rows_d, uint32_t frames, uint32_t lds_bytes, uint32_t hops, uint32_t rounds, ZdSmallDecResult *res_d);
// ---- k_delta_small_dec.hip: the decode of small `delta` frames, one workgroup per frame (delta_small_dec.hpp has the arithmetic and the
// limits).  A row per frame: its payload (device memory, any alignment; payload_bytes to the stream's end), where its w x h x 3 image goes
// (device memory, any alignment) and its decoder as `leaves` words of left-aligned codes, ascending, and as many key | length << 27 words
// (no code longer than kDeltaSmallMaxCodeLen).  status_d[f]: kDsdOk (the image is written), kDsdShort / kDsdRange (it is not: the single
// decode's two failures), kDsdUnsettled (not written: the caller decodes the frame on its own).  max_rounds >= 1: settle rounds per frame.
struct DeltaSmallDecRow { const uint8_t *payload; uint8_t *dst; const uint32_t *code, *keylen; uint32_t payload_bytes, leaves, w, h, max_len /* the longest code */; };
int delta_small_dec_run(Ctx *c, const DeltaSmallDecRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint32_t max_rounds, uint32_t *status_d);
// the same for RGB symbols (k_huf_small_dec: small `hufman` and `cluster-colors` frames; key = r << 16 | g << 8 | b, position d is pixel d,
// no FromDiff): status_d[f] is kDsdOk, kDsdShort or kDsdUnsettled
int huf_small_dec_run(Ctx *c, const DeltaSmallDecRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint32_t max_rounds, uint32_t *status_d);
// ---- k_small_trie.hip: the parse of small frames' decoders, one workgroup per frame (small_trie.hpp has the arithmetic and the
// limits).  sym_bytes = S: 6 for the SignedColor leaves of `delta` streams, 11 for the Rgb leaves of `hufman` and `cluster-colors` streams
// (no scan test: scan_w and scan_h are not looked at).  A row per frame: its stream (device memory, any alignment; `bytes` of it may be
// read) and where its table goes -- room for st_leaves_room<S>(bytes) leaves of two words, 4-byte aligned: the left-aligned codes, then as many key | length << 27 words, which is what
// DeltaSmallDecRow points at.  res_d[f]: the header's w and h (when there are 8 bytes), the verdict (small_trie.hpp), and of a parsed
// decoder the leaves, the longest code and the payload's offset in the stream.  A frame of 0 or more than max_px pixels, of more than
// img_stride bytes or of the size scan_w x scan_h (0 x 0: none) is skipped (kStSkipped).
struct SmallTrieRow { const uint8_t *stream; uint32_t *table; uint64_t bytes; };
struct SmallTrieResult { uint32_t w, h, verdict, leaves, max_len, payload_at; };
int small_trie_run(Ctx *c, uint32_t sym_bytes, const SmallTrieRow *rows_d, uint32_t frames, uint64_t max_bytes /* of the longest stream */, uint32_t max_px, uint64_t img_stride,
                   uint32_t scan_w, uint32_t scan_h, SmallTrieResult *res_d);
// ---- k_vor_small.hip: voronoi(K <= 256) of small frames, one workgroup per frame (vor_small.hpp has the arithmetic, the limits and the
// stream's layout).  A row per frame: its pixels (device memory, any alignment).  Frame f's finished stream (16 + 19 K bytes) lands at
// scratch_d + f * sstride, its K-means outcome in res_d[f].  stay_test: points well inside their cell skip the search (vs_stays; the
// outcome is the same without it, res_d[f].evals is not).
struct VorSmallRow { const uint8_t *src; uint32_t w, h; };
struct VorSmallResult { uint32_t status /* 1: n / K == 0, nothing else was computed */, n, iterations, moved_last, reseeds, active; uint64_t evals; };
int vor_small_run(Ctx *c, const VorSmallRow *rows_d, uint32_t frames, uint32_t max_px /* of the largest frame */, uint32_t K, uint64_t seed, uint64_t max_iters,
                  bool stay_test, uint8_t *scratch_d, uint64_t sstride, VorSmallResult *res_d);
// The repaint of such frames' streams.  A row per frame: where its w x h x 3 image goes (device memory, any alignment) and its K centroids
// (1 .. 256) in table_d from centroid cent0 on, three words each: x, y (any u32: the squares wrap as the reference's do) and 0xRRGGBB.
// A row is a slice of a frame, a workgroup's share: the pixels from px0 (a multiple of kVorSmallDecSlice) on, at most kVorSmallDecSlice of them.
constexpr uint32_t kVorSmallDecSlice = 2048;
struct VorSmallDecRow { uint8_t *dst /* the frame's */; uint32_t cent0, K, w, h, px0, pad; };
int vor_small_dec_run(Ctx *c, const VorSmallDecRow *rows_d, uint32_t slices, uint32_t max_px /* of the largest frame */, const uint32_t *table_d);
// ---- k_palette.hip: the colour -> label table of a frozen palette (every colour's nearest entry, lowest index among equals).  table_d: 2^24
// labels of 1 (K <= 256) or 2 bytes; list_max: candidates of a cell kept in LDS (<= kPalListMax, pal_bounds.hpp), a longer list sends the cell
// down the plain route; plain_cells_d (optional): a zeroed counter of such cells
int palette_lut(Ctx *c, const uint32_t *cent_d, uint32_t K, bool wide, void *table_d, uint32_t list_max, uint32_t *plain_cells_d);
// the fit of a batch of frames (the frame table's rows, `chunks` chunks of 4096 pixels) under that table: sse_d[f] += the frame's summed squared
// distance to its pixels' entries, pixels_d[k] (optional) += the pixels whose entry is k; one launch
int palette_fit(Ctx *c, const uint8_t *rgb_d, const FrameVar *fr_d, uint32_t frames, uint32_t chunks, const void *table_d, bool wide, const uint32_t *cent_d, uint32_t K,
                uint64_t *sse_d, uint64_t *pixels_d);

}  // namespace cniic
