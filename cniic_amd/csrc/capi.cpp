// capi.cpp -- the extern "C" surface declared in include/cniic_hip.h.
// Every entry point: lock the context, bind host-or-device buffers, run the HIP path, report an
// error code.  Nothing here computes on the CPU what the reference computes per pixel.
#include <algorithm>
#include <cstring>
#include <limits>
#include <map>
#include <memory>

#include "codec.hpp"
#include <atomic>
#include <thread>

#include "common.hpp"
#include "huff_host.hpp"
#include "surf_index.hpp"
#include "cc_small.hpp"
#include "vor_small.hpp"
#include "delta_small.hpp"
#include "huf_small.hpp"
#include "rle_small.hpp"
#include "hz_small.hpp"
#include "zd_small.hpp"

using namespace cniic;

struct cniic_km {
    Ctx *c = nullptr;
    KmRgbwState *st = nullptr;
    In<uint32_t> keys, weight;
    uint64_t lo = 0, hi = 0, U = 0;
    uint32_t K = 0;
};

#define LOCK(ctx)                          \
    if (!(ctx)) return CNIIC_ERR_BAD_ARG;  \
    std::lock_guard<std::mutex> _lk((ctx)->mu); \
    (ctx)->err.clear();                    \
    PoolScope _ps(&(ctx)->pool);           /* every DevBuf allocated during the call comes from the context's caching pool */ \
    do { hipError_t _e = hipSetDevice((ctx)->device); if (_e != hipSuccess) return (ctx)->fail(CNIIC_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(_e)); } while (0)

// results computed into host vectors -> caller buffer (host or device)
static int to_caller(Ctx *c, void *dst, const void *src_host, uint64_t bytes) {
    if (!bytes || !dst) return CNIIC_OK;
    if (is_device_ptr(dst)) CNIIC_HIP_TRY(c, hipMemcpy(dst, src_host, bytes, hipMemcpyHostToDevice));
    else memcpy(dst, src_host, bytes);
    return CNIIC_OK;
}
// small caller arrays (host or device) -> host vector
static int from_caller(Ctx *c, void *dst_host, const void *src, uint64_t bytes) {
    if (!bytes) return CNIIC_OK;
    if (is_device_ptr(src)) CNIIC_HIP_TRY(c, hipMemcpy(dst_host, src, bytes, hipMemcpyDeviceToHost));
    else memcpy(dst_host, src, bytes);
    return CNIIC_OK;
}

extern "C" {

int32_t cniic_version(void) { return 100; }
int32_t cniic_is_testing_build(void) {
#ifdef CNIIC_TESTING
    return 1;
#else
    return 0;
#endif
}

int32_t cniic_ctx_create(int32_t device, void *stream, cniic_ctx **out) {
    if (!out) return CNIIC_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CNIIC_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return CNIIC_ERR_HIP;
    std::unique_ptr<cniic_ctx> c(new cniic_ctx());   // (a failure below gives back what has been created: ~Ctx and its members)
    c->device = device;
    if (stream) c->stream = reinterpret_cast<hipStream_t>(stream);
    else {
        if (hipStreamCreateWithFlags(&c->own_stream.s, hipStreamNonBlocking) != hipSuccess) return CNIIC_ERR_HIP;
        c->stream = c->own_stream.s;
    }
    if (c->ev0.ensure(hipEventDefault) != hipSuccess || c->ev1.ensure(hipEventDefault) != hipSuccess) return CNIIC_ERR_HIP;
    *out = c.release();
    return CNIIC_OK;
}

void cniic_ctx_destroy(cniic_ctx *c) {
    if (c) delete c;   // ~Ctx (common.hpp)
}

const char *cniic_last_error(const cniic_ctx *c) { return c ? c->err.c_str() : "null context"; }

int32_t cniic_sync(cniic_ctx *c) {
    LOCK(c);
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_dev_alloc(cniic_ctx *c, uint64_t bytes, void **dptr) {
    LOCK(c);
    if (!dptr) return c->fail(CNIIC_ERR_BAD_ARG, "dev_alloc: null out pointer");
    CNIIC_HIP_TRY(c, hipMalloc(dptr, bytes ? bytes : 16));
    return CNIIC_OK;
}

int32_t cniic_dev_free(cniic_ctx *c, void *dptr) {
    LOCK(c);
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    CNIIC_HIP_TRY(c, hipFree(dptr));
    return CNIIC_OK;
}

int32_t cniic_memcpy(cniic_ctx *c, void *dst, const void *src, uint64_t bytes) {
    LOCK(c);
    if (!bytes) return CNIIC_OK;
    CNIIC_HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_ctx_set_opt(cniic_ctx *c, int32_t opt, uint64_t value) {
    if (!c) return CNIIC_ERR_BAD_ARG;
    LOCK(c);
    if (opt <= 0 || opt >= CNIIC_OPT_COUNT) return c->fail(CNIIC_ERR_BAD_ARG, "ctx_set_opt: unknown option %d", opt);
    c->opt_val[opt] = value;
    c->opt_set |= 1u << opt;
    if (opt == CNIIC_OPT_STAGE_TIMERS) c->timers = value != 0;
    return CNIIC_OK;
}

int32_t cniic_ctx_unset_opt(cniic_ctx *c, int32_t opt) {
    if (!c) return CNIIC_ERR_BAD_ARG;
    LOCK(c);
    if (opt <= 0 || opt >= CNIIC_OPT_COUNT) return c->fail(CNIIC_ERR_BAD_ARG, "ctx_unset_opt: unknown option %d", opt);
    c->opt_set &= ~(1u << opt);
    if (opt == CNIIC_OPT_STAGE_TIMERS) c->timers = getenv("CNIIC_KERNEL_TIMERS") != nullptr;
    return CNIIC_OK;
}

int32_t cniic_ctx_set_scan(cniic_ctx *c, uint32_t w, uint32_t h, const uint32_t *xy) {
    LOCK(c);
    return scan_inject(c, w, h, xy, xy && is_device_ptr(xy));
}

int32_t cniic_ctx_get_opt(cniic_ctx *c, int32_t opt, uint64_t *value) {
    if (!c || !value) return CNIIC_ERR_BAD_ARG;
    LOCK(c);
    static const struct { const char *env; uint64_t dflt; } k[CNIIC_OPT_COUNT] = {
        {nullptr, 0}, {"CNIIC_SP_MIN_PIXELS", 1ull << 20}, {"CNIIC_HUF_GPU_CODES_MIN", 32768}, {"CNIIC_GPU_DECODE_MIN", 1ull << 14},
        {"CNIIC_DELTA_ROUTE", 0}, {nullptr, 0}, {"CNIIC_FRAME_TREES_HOST", 0}, {nullptr, 8}, {"CNIIC_KM_MAX_BLOCKS", 0}, {"CNIIC_KM_LOOP", 0}};
    if (opt <= 0 || opt >= CNIIC_OPT_COUNT) return c->fail(CNIIC_ERR_BAD_ARG, "ctx_get_opt: unknown option %d", opt);
    *value = opt == CNIIC_OPT_STAGE_TIMERS ? (c->timers ? 1 : 0) : c->opt(opt, k[opt].env, k[opt].dflt);
    return CNIIC_OK;
}

int32_t cniic_last_kernel_time(cniic_ctx *c, const char *which, double *ms, uint64_t *launches) {
    if (!c || !which) return CNIIC_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->ktimes.find(which);
    if (it == c->ktimes.end()) { if (ms) *ms = 0; if (launches) *launches = 0; return CNIIC_ERR_BAD_ARG; }
    if (ms) *ms = it->second.ms;
    if (launches) *launches = it->second.launches;
    return CNIIC_OK;
}

// ------------------------------------------------------------------ H1
static int hist_common(Ctx *c, uint32_t bits, uint32_t *table, uint32_t *keys, uint64_t *counts, uint64_t cap, uint64_t *n_unique) {
    CompactPlan plan;
    CNIIC_TRY(hist_compact_count(c, table, bits, &plan));
    if (n_unique) *n_unique = plan.n_unique;
    if (!keys && !counts) return CNIIC_OK;
    if (plan.n_unique > cap)
        return c->fail(CNIIC_ERR_CAPACITY, "histogram has %llu distinct symbols, capacity %llu", (unsigned long long)plan.n_unique,
                       (unsigned long long)cap);
    Out<uint32_t> ko;
    Out<uint64_t> co;
    CNIIC_TRY(ko.bind(c, keys, plan.n_unique));
    CNIIC_TRY(co.bind(c, counts, plan.n_unique));
    CNIIC_TRY(hist_compact_write(c, table, &plan, ko.d, co.d, nullptr));
    CNIIC_TRY(ko.finish(c));
    CNIIC_TRY(co.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_hist_rgb24(cniic_ctx *c, const uint8_t *rgb, uint64_t npx, uint32_t *keys, uint64_t *counts, uint64_t cap,
                         uint64_t *n_unique) {
    LOCK(c);
    c->ktimes.clear();
    if (npx && !rgb) return c->fail(CNIIC_ERR_BAD_ARG, "hist_rgb24: null image");
    if (npx >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "hist_rgb24: too many pixels");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, npx * 3));
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, 24, &table));
    {
        ScopedKernelTimer t(c, "hist_rgb");
        CNIIC_TRY(hist_rgb_dense(c, in.d, npx, table));
        t.stop(1);
    }
    return hist_common(c, 24, table, keys, counts, cap, n_unique);
}

int32_t cniic_hist_syms(cniic_ctx *c, int32_t sym_kind, const uint32_t *syms, uint64_t n, uint32_t *keys, uint64_t *counts,
                        uint64_t cap, uint64_t *n_unique) {
    LOCK(c);
    c->ktimes.clear();
    if (sym_kind != CNIIC_SYM_RGB && sym_kind != CNIIC_SYM_SIGNED) return c->fail(CNIIC_ERR_BAD_ARG, "hist_syms: bad symbol kind");
    if (n && !syms) return c->fail(CNIIC_ERR_BAD_ARG, "hist_syms: null stream");
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "hist_syms: too many symbols");
    const uint32_t bits = sym_kind == CNIIC_SYM_RGB ? 24 : 27;
    In<uint32_t> in;
    CNIIC_TRY(in.bind(c, syms, n));
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, bits, &table));
    CNIIC_TRY(hist_syms_dense(c, in.d, n, table, bits));
    return hist_common(c, bits, table, keys, counts, cap, n_unique);
}

// ------------------------------------------------------------------ K-means
// cniic_kmeans_rgbw (init == nullptr: init_centroids, kmeans.rs:101-108) and cniic_kmeans_rgbw_from (init: K x 3 bytes, host), the mutex held
static int32_t kmeans_rgbw_locked(cniic_ctx *c, const uint32_t *keys, const uint32_t *weight, uint64_t U, uint32_t K,
                                  const cniic_kmeans_opts *opts, const uint8_t *init, uint8_t *centroids, uint32_t *labels, uint64_t *members,
                                  cniic_kmeans_stats *stats) {
    c->ktimes.clear();
    if (!keys || !weight || !centroids) return c->fail(CNIIC_ERR_BAD_ARG, "kmeans_rgbw: null argument");
    In<uint32_t> k, w;
    CNIIC_TRY(k.bind(c, keys, U));
    CNIIC_TRY(w.bind(c, weight, U));
    KmRgbwState *km = nullptr;
    CNIIC_TRY(km_rgbw_create(c, k.d, w.d, U, 0, 1, K, opts, nullptr, nullptr, &km));
    std::unique_ptr<KmRgbwState, void (*)(KmRgbwState *)> guard(km, km_rgbw_destroy);
    if (init) CNIIC_TRY(km_rgbw_set_centroids(km, init));
    CNIIC_TRY(km_rgbw_run(km));
    Out<uint32_t> lo;
    CNIIC_TRY(lo.bind(c, labels, U));
    cniic_kmeans_stats st{};
    std::vector<uint8_t> cent(3 * (size_t)K);
    std::vector<uint64_t> mem(K);
    CNIIC_TRY(km_rgbw_result(km, cent.data(), lo.d, mem.data(), nullptr, &st));
    CNIIC_TRY(lo.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    CNIIC_TRY(to_caller(c, centroids, cent.data(), cent.size()));
    CNIIC_TRY(to_caller(c, members, mem.data(), mem.size() * 8));
    if (stats) *stats = st;
    return check_enough_active(c, K, U, st.active);   // (the caller has centroids, labels, members and stats of a failed run too)
}

int32_t cniic_kmeans_rgbw(cniic_ctx *c, const uint32_t *keys, const uint32_t *weight, uint64_t U, uint32_t K,
                          const cniic_kmeans_opts *opts, uint8_t *centroids, uint32_t *labels, uint64_t *members,
                          cniic_kmeans_stats *stats) {
    LOCK(c);
    return kmeans_rgbw_locked(c, keys, weight, U, K, opts, nullptr, centroids, labels, members, stats);
}

int32_t cniic_kmeans_rgbw_from(cniic_ctx *c, const uint32_t *keys, const uint32_t *weight, uint64_t U, uint32_t K,
                               const cniic_kmeans_opts *opts, const uint8_t *init, uint8_t *centroids, uint32_t *labels, uint64_t *members,
                               cniic_kmeans_stats *stats) {
    LOCK(c);
    if (!init || is_device_ptr(init)) return c->fail(CNIIC_ERR_BAD_ARG, "kmeans_rgbw_from: init is K x 3 bytes of host memory");
    return kmeans_rgbw_locked(c, keys, weight, U, K, opts, init, centroids, labels, members, stats);
}

int32_t cniic_kmeans_step_rgbw(cniic_ctx *c, const uint32_t *keys, const uint32_t *weight, uint64_t U, uint32_t K,
                               const uint8_t *centroids, uint32_t *labels, uint64_t *sums, uint64_t *wsum, uint64_t *members,
                               uint64_t *changed) {
    LOCK(c);
    c->ktimes.clear();
    if (!keys || !weight || !centroids || !labels) return c->fail(CNIIC_ERR_BAD_ARG, "kmeans_step_rgbw: null argument");
    In<uint32_t> k, w, lin;
    CNIIC_TRY(k.bind(c, keys, U));
    CNIIC_TRY(w.bind(c, weight, U));
    CNIIC_TRY(lin.bind(c, labels, U));
    std::vector<uint8_t> cent(3 * (size_t)K);
    CNIIC_TRY(from_caller(c, cent.data(), centroids, cent.size()));
    KmRgbwState *km = nullptr;
    cniic_kmeans_opts step_opts{0, 0, CNIIC_KM_BRUTE_FORCE, 0};  // explicit centroids + labels: full-sum kernel
    CNIIC_TRY(km_rgbw_create(c, k.d, w.d, U, 0, 1, K, &step_opts, nullptr, nullptr, &km));
    std::unique_ptr<KmRgbwState, void (*)(KmRgbwState *)> guard(km, km_rgbw_destroy);
    CNIIC_TRY(km_rgbw_set_state(km, cent.data(), lin.d));
    CNIIC_TRY(km_rgbw_assign(km));
    std::vector<uint64_t> s(3 * (size_t)K), ws(K), mem(K);
    uint64_t ch = 0;
    CNIIC_TRY(km_rgbw_partials(km, s.data(), ws.data(), mem.data(), &ch));
    Out<uint32_t> lo;
    CNIIC_TRY(lo.bind(c, labels, U));
    CNIIC_TRY(km_rgbw_result(km, nullptr, lo.d, nullptr, nullptr, nullptr));
    CNIIC_TRY(lo.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    CNIIC_TRY(to_caller(c, sums, s.data(), s.size() * 8));
    CNIIC_TRY(to_caller(c, wsum, ws.data(), ws.size() * 8));
    CNIIC_TRY(to_caller(c, members, mem.data(), mem.size() * 8));
    if (changed) *changed = ch;
    return CNIIC_OK;
}

// cniic_kmeans_xyrgb (init == nullptr) and cniic_kmeans_xyrgb_from (init: K cniic_colorpos, host), the mutex held
static int32_t kmeans_xyrgb_locked(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t K, const cniic_kmeans_opts *opts, const cniic_colorpos *init,
                                   cniic_colorpos *centroids, uint32_t *labels, uint64_t *members, cniic_kmeans_stats *stats) {
    c->ktimes.clear();
    if (!rgb || !centroids) return c->fail(CNIIC_ERR_BAD_ARG, "kmeans_xyrgb: null argument");
    const uint64_t N = (uint64_t)w * h;
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, N * 3));
    Out<uint32_t> lo;
    CNIIC_TRY(lo.bind(c, labels, N));
    std::vector<cniic_colorpos> cent(K ? K : 1);
    std::vector<uint64_t> mem(K ? K : 1);
    cniic_kmeans_stats st{};
    CNIIC_TRY(km_xyrgb_run(c, in.d, w, h, K, opts, cent.data(), lo.d, mem.data(), &st, init));
    CNIIC_TRY(lo.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    CNIIC_TRY(to_caller(c, centroids, cent.data(), (size_t)K * sizeof(cniic_colorpos)));
    CNIIC_TRY(to_caller(c, members, mem.data(), (size_t)K * 8));
    if (stats) *stats = st;
    return check_enough_active(c, K, N, st.active);
}

int32_t cniic_kmeans_xyrgb(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t K, const cniic_kmeans_opts *opts,
                           cniic_colorpos *centroids, uint32_t *labels, uint64_t *members, cniic_kmeans_stats *stats) {
    LOCK(c);
    return kmeans_xyrgb_locked(c, rgb, w, h, K, opts, nullptr, centroids, labels, members, stats);
}

int32_t cniic_kmeans_xyrgb_from(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t K, const cniic_kmeans_opts *opts, const cniic_colorpos *init,
                                cniic_colorpos *centroids, uint32_t *labels, uint64_t *members, cniic_kmeans_stats *stats) {
    LOCK(c);
    if (!init || is_device_ptr(init)) return c->fail(CNIIC_ERR_BAD_ARG, "kmeans_xyrgb_from: init is K entries of host memory");
    return kmeans_xyrgb_locked(c, rgb, w, h, K, opts, init, centroids, labels, members, stats);
}

int32_t cniic_kmeans_step_xyrgb(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t K,
                                const cniic_colorpos *centroids, uint32_t *labels, uint64_t *sums, uint64_t *wsum,
                                uint64_t *members, uint64_t *changed) {
    LOCK(c);
    c->ktimes.clear();
    if (!rgb || !centroids || !labels) return c->fail(CNIIC_ERR_BAD_ARG, "kmeans_step_xyrgb: null argument");
    const uint64_t N = (uint64_t)w * h;
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, N * 3));
    // labels are in/out: stage a device copy when the caller's buffer is host memory
    DevBuf lab_own;
    uint32_t *lab_d = labels;
    const bool lab_dev = is_device_ptr(labels);
    if (!lab_dev) {
        CNIIC_HIP_TRY(c, lab_own.alloc(N * 4));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(lab_own.p, labels, N * 4, hipMemcpyHostToDevice, c->stream));
        lab_d = lab_own.as<uint32_t>();
    }
    std::vector<cniic_colorpos> cent(K ? K : 1);
    CNIIC_TRY(from_caller(c, cent.data(), centroids, (size_t)K * sizeof(cniic_colorpos)));
    std::vector<uint64_t> s(5 * (size_t)K + 1), ws(K + 1), mem(K + 1);
    uint64_t ch = 0;
    CNIIC_TRY(km_xyrgb_step(c, in.d, w, h, K, cent.data(), lab_d, s.data(), ws.data(), mem.data(), &ch, nullptr));
    if (!lab_dev) CNIIC_HIP_TRY(c, hipMemcpy(labels, lab_d, N * 4, hipMemcpyDeviceToHost));
    CNIIC_TRY(to_caller(c, sums, s.data(), 5 * (size_t)K * 8));
    CNIIC_TRY(to_caller(c, wsum, ws.data(), (size_t)K * 8));
    CNIIC_TRY(to_caller(c, members, mem.data(), (size_t)K * 8));
    if (changed) *changed = ch;
    return CNIIC_OK;
}

// ------------------------------------------------------------------ sharded session
uint64_t cniic_km_partial_words(uint32_t K, uint32_t D) { return (uint64_t)K * D + 2ull * K + 2; }

int32_t cniic_km_create_rgbw(cniic_ctx *c, const uint32_t *keys, const uint32_t *weight, uint64_t U, uint32_t shard, uint32_t nshards,
                             uint32_t K, const cniic_kmeans_opts *opts, void *partials_dev, cniic_km **out) {
    LOCK(c);
    if (!out || !keys || !weight) return c->fail(CNIIC_ERR_BAD_ARG, "km_create_rgbw: null argument");
    if (partials_dev && !is_device_ptr(partials_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "km_create_rgbw: partials must be device memory");
    auto km = std::make_unique<cniic_km>();
    km->c = c; km->K = K; km->U = U;
    CNIIC_TRY(km->keys.bind(c, keys, U));
    CNIIC_TRY(km->weight.bind(c, weight, U));
    CNIIC_TRY(km_rgbw_create(c, km->keys.d, km->weight.d, U, shard, nshards, K, opts, partials_dev, nullptr, &km->st));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *out = km.release();
    return CNIIC_OK;
}

int32_t cniic_km_partials(cniic_km *km, void **dev_ptr) {
    if (!km || !dev_ptr) return CNIIC_ERR_BAD_ARG;
    *dev_ptr = km_rgbw_partials_dev(km->st);
    return CNIIC_OK;
}

int32_t cniic_km_begin(cniic_km *km) {
    if (!km) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(km->c);
    LOCK(c);
    return km_rgbw_fold_initial(km->st);
}

int32_t cniic_km_labels_internal(cniic_km *km, void **dev_ptr, uint64_t *elem_bytes) {
    if (!km || !dev_ptr) return CNIIC_ERR_BAD_ARG;
    *dev_ptr = km_rgbw_labels_internal(km->st, elem_bytes);
    return CNIIC_OK;
}

int32_t cniic_km_assign(cniic_km *km) {
    if (!km) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(km->c);
    LOCK(c);
    return km_rgbw_assign(km->st);
}

int32_t cniic_km_update(cniic_km *km, uint64_t *changed) {
    if (!km) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(km->c);
    LOCK(c);
    CNIIC_TRY(km_rgbw_update(km->st));
    uint64_t ch = 0;
    CNIIC_TRY(km_rgbw_poll_changed(km->st, &ch));
    if (changed) *changed = ch;
    return CNIIC_OK;
}

int32_t cniic_km_result(cniic_km *km, uint8_t *centroids, uint32_t *labels_slice, uint64_t *members, cniic_kmeans_stats *stats) {
    if (!km) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(km->c);
    LOCK(c);
    Out<uint32_t> lo;
    CNIIC_TRY(lo.bind(c, labels_slice, km->U));
    std::vector<uint8_t> cent(3 * (size_t)km->K);
    std::vector<uint64_t> mem(km->K);
    cniic_kmeans_stats st{};
    CNIIC_TRY(km_rgbw_result(km->st, cent.data(), lo.d, mem.data(), nullptr, &st));
    CNIIC_TRY(lo.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    CNIIC_TRY(to_caller(c, centroids, cent.data(), cent.size()));
    CNIIC_TRY(to_caller(c, members, mem.data(), mem.size() * 8));
    if (stats) *stats = st;
    return CNIIC_OK;
}

int32_t cniic_km_time_assign(cniic_km *km, int32_t reps, double *ms_per_launch) {
    if (!km || !ms_per_launch || reps <= 0) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(km->c);
    LOCK(c);
    return km_rgbw_time_assign(km->st, reps, ms_per_launch);
}

void cniic_km_destroy(cniic_km *km) {
    if (!km) return;
    {
        std::lock_guard<std::mutex> lk(km->c->mu);
        (void)hipSetDevice(km->c->device);
        (void)hipStreamSynchronize(km->c->stream);
        PoolScope ps(&km->c->pool);
        km_rgbw_destroy(km->st);
        km->keys.own.release();
        km->weight.own.release();
    }
    delete km;
}

// ------------------------------------------------------------------ sharded cluster-colors session
struct cniic_cc {
    Ctx *c = nullptr;
    CcSession *s = nullptr;
};

int32_t cniic_hist_rgb24_dense(cniic_ctx *c, const uint8_t *rgb, uint64_t npx, uint32_t *table_dev) {
    LOCK(c);
    c->ktimes.clear();
    if (!table_dev || !is_device_ptr(table_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "hist_rgb24_dense: table must be device memory (u32[2^24])");
    if (npx && !rgb) return c->fail(CNIIC_ERR_BAD_ARG, "hist_rgb24_dense: null image");
    if (npx >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "hist_rgb24_dense: too many pixels");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, npx * 3));
    CNIIC_HIP_TRY(c, hipMemsetAsync(table_dev, 0, (1ull << 24) * 4, c->stream));
    ScopedKernelTimer t(c, "hist_rgb");
    CNIIC_TRY(hist_rgb_dense(c, in.d, npx, table_dev));
    t.stop(1);
    return CNIIC_OK;
}

int32_t cniic_cc_create(cniic_ctx *c, uint32_t *table_dev, uint32_t K, const cniic_kmeans_opts *opts, uint32_t shard,
                        uint32_t nshards, void *partials_dev, cniic_cc **out) {
    LOCK(c);
    if (!out || !table_dev || !is_device_ptr(table_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_create: table must be device memory");
    if (partials_dev && !is_device_ptr(partials_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_create: partials must be device memory");
    CcSession *s = nullptr;
    CNIIC_TRY(cc_prepare(c, table_dev, K, opts, shard, nshards, partials_dev, &s));
    auto *cc = new cniic_cc();
    cc->c = c; cc->s = s;
    *out = cc;
    return CNIIC_OK;
}

uint64_t cniic_cc_unique(cniic_cc *cc) { return cc && cc->s ? cc->s->U : 0; }
uint32_t cniic_cc_label_bytes(cniic_cc *cc) { return cc && cc->s && cc->s->km && km_rgbw_is_wide(cc->s->km) ? 2 : 1; }

int32_t cniic_cc_assign(cniic_cc *cc) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    return km_rgbw_assign(cc->s->km);
}

int32_t cniic_cc_set_centroids(cniic_cc *cc, const uint8_t *init) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    if (!init || is_device_ptr(init)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_set_centroids: init is K x 3 bytes of host memory");
    return km_rgbw_set_centroids(cc->s->km, init);
}

int32_t cniic_cc_update(cniic_cc *cc, uint64_t *changed) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    CNIIC_TRY(km_rgbw_update(cc->s->km));
    if (!changed) return CNIIC_OK;  // asynchronous: the caller polls later with cniic_cc_poll
    uint64_t ch = 0;
    CNIIC_TRY(km_rgbw_poll_changed(cc->s->km, &ch));
    *changed = ch;
    return CNIIC_OK;
}

int32_t cniic_cc_poll(cniic_cc *cc, uint64_t *iterations, uint32_t *done) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    cniic_kmeans_stats st{};
    uint32_t d = 0;
    CNIIC_TRY(km_rgbw_poll(cc->s->km, &st, &d));
    if (iterations) *iterations = st.iterations;
    if (done) *done = d;
    return CNIIC_OK;
}

int32_t cniic_occupancy_pack(cniic_ctx *c, const uint32_t *table_dev, uint32_t *occ_dev) {
    LOCK(c);
    if (!table_dev || !occ_dev || !is_device_ptr(table_dev) || !is_device_ptr(occ_dev))
        return c->fail(CNIIC_ERR_BAD_ARG, "occupancy_pack: device buffers u32[2^24] and u32[2^21]");
    return occupancy_pack(c, table_dev, occ_dev);
}

int32_t cniic_cc_create_local(cniic_ctx *c, uint32_t *table_dev, const uint32_t *occ_dev, uint32_t K, const cniic_kmeans_opts *opts,
                              void *partials_dev, cniic_cc **out) {
    LOCK(c);
    if (!table_dev || !occ_dev || !out || !is_device_ptr(table_dev) || !is_device_ptr(occ_dev))
        return c->fail(CNIIC_ERR_BAD_ARG, "cc_create_local: device table, device occupancy and an out pointer are needed");
    if (partials_dev && !is_device_ptr(partials_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_create_local: partials must be device memory");
    CcSession *s = nullptr;
    CNIIC_TRY(cc_prepare(c, table_dev, K, opts, 0, 1, partials_dev, &s, occ_dev));
    *out = new cniic_cc{c, s};
    return CNIIC_OK;
}

int32_t cniic_cc_image_begin(cniic_ctx *c, const uint8_t *rgb_dev, uint64_t npx, cniic_cc **out) {
    LOCK(c);
    if (!rgb_dev || !out || npx == 0 || !is_device_ptr(rgb_dev) || (reinterpret_cast<uintptr_t>(rgb_dev) & 15))
        return c->fail(CNIIC_ERR_BAD_ARG, "cc_image_begin: a non-empty, 16-byte aligned device image and an out pointer are needed");
    if (npx >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_image_begin: too many pixels");
    c->ktimes.clear();
    CcSession *s = nullptr;
    CNIIC_TRY(cc_image_begin(c, rgb_dev, npx, &s));
    *out = new cniic_cc{c, s};
    return CNIIC_OK;
}

int32_t cniic_cc_image_occupancy(cniic_cc *cc, uint32_t *occ_dev) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->sp_mode || !occ_dev || !is_device_ptr(occ_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_image_occupancy: image session and device buffer needed");
    return sp_occupancy(c, &cc->s->sp, occ_dev);
}

int32_t cniic_cc_image_create(cniic_cc *cc, const uint32_t *occ_dev, uint32_t K, const cniic_kmeans_opts *opts, void *partials_dev) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!occ_dev || !is_device_ptr(occ_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_image_create: device occupancy needed");
    if (partials_dev && !is_device_ptr(partials_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_image_create: partials must be device memory");
    return cc_image_create(cc->s, occ_dev, K, opts, partials_dev);
}

int32_t cniic_cc_poll_lagged(cniic_cc *cc, uint64_t *iterations, uint32_t *done, uint32_t *valid) {
    if (!cc || !done || !valid) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    cniic_kmeans_stats st{};
    CNIIC_TRY(km_rgbw_poll_lagged(cc->s->km, &st, done, valid));
    if (iterations) *iterations = st.iterations;
    return CNIIC_OK;
}

// ---- RCCL communicator on the context's stream
struct cniic_comm { Comm *m = nullptr; };

int32_t cniic_comm_unique_id(uint8_t id[128]) {
    if (!id) return CNIIC_ERR_BAD_ARG;
    return comm_unique_id(id);
}

int32_t cniic_comm_create(cniic_ctx *c, const uint8_t id[128], uint32_t rank, uint32_t nranks, cniic_comm **out) {
    if (!c || !id || !out) return CNIIC_ERR_BAD_ARG;
    LOCK(c);
    Comm *m = nullptr;
    CNIIC_TRY(comm_create(c, id, rank, nranks, &m));
    *out = new cniic_comm{m};
    return CNIIC_OK;
}

int32_t cniic_comm_create_host(cniic_ctx *c, uint32_t rank, uint32_t nranks, cniic_host_sum_fn fn, void *user, cniic_comm **out) {
    if (!c || !out) return CNIIC_ERR_BAD_ARG;
    LOCK(c);
    Comm *m = nullptr;
    CNIIC_TRY(comm_create_host(c, rank, nranks, fn, user, &m));
    *out = new cniic_comm{m};
    return CNIIC_OK;
}

int32_t cniic_comm_create_mailbox(cniic_ctx *c, uint32_t rank, uint32_t nranks, uint64_t max_bytes, uint8_t handle[64], cniic_comm **out) {
    if (!c || !handle || !out) return CNIIC_ERR_BAD_ARG;
    LOCK(c);
    Comm *m = nullptr;
    CNIIC_TRY(comm_create_mailbox(c, rank, nranks, max_bytes, handle, &m));
    *out = new cniic_comm{m};
    return CNIIC_OK;
}

int32_t cniic_comm_connect_mailbox(cniic_comm *cm, const uint8_t *handles) {
    if (!cm || !cm->m || !handles) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(comm_ctx(cm->m));
    LOCK(c);
    return comm_connect_mailbox(cm->m, handles);
}

void cniic_comm_destroy(cniic_comm *cm) {
    if (!cm) return;
    if (cm->m) {
        Ctx *c = comm_ctx(cm->m);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        comm_destroy(cm->m);
    }
    delete cm;
}

int32_t cniic_comm_all_reduce(cniic_comm *cm, void *buf_dev, uint64_t count, int32_t elem_bytes) {
    if (!cm || !cm->m || !buf_dev) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(comm_ctx(cm->m));
    LOCK(c);
    if (!is_device_ptr(buf_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "comm_all_reduce: buffer must be device memory");
    const int kind = elem_bytes == 1 ? 0 : elem_bytes == 4 ? 1 : elem_bytes == 8 ? 2 : -1;
    if (kind < 0) return c->fail(CNIIC_ERR_BAD_ARG, "comm_all_reduce: elements of 1, 4 or 8 bytes (unsigned sum)");
    return comm_all_reduce(cm->m, buf_dev, count, kind);
}

int32_t cniic_comm_set_timeout(cniic_comm *cm, uint64_t milliseconds) {
    if (!cm || !cm->m) return CNIIC_ERR_BAD_ARG;
    comm_set_timeout_ms(cm->m, milliseconds);
    return CNIIC_OK;
}

int32_t cniic_cc_run(cniic_cc *cc, cniic_comm *cm, cniic_kmeans_stats *stats) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    if (cm && cm->m && comm_ctx(cm->m) != cc->c) return c->fail(CNIIC_ERR_BAD_ARG, "cc_run: communicator of another context");
    host_trace().mark("cc_run: enter");
    CNIIC_TRY(km_rgbw_run(cc->s->km, cm ? cm->m : nullptr));
    host_trace().mark("cc_run: the loop");
    if (stats && !km_rgbw_run_stats(cc->s->km, stats)) {  // (the loop's own last look at the state; no wait for the launches past convergence)
        uint32_t d = 0;
        CNIIC_TRY(km_rgbw_poll(cc->s->km, stats, &d));
    }
    return CNIIC_OK;
}

int32_t cniic_cc_partials(cniic_cc *cc, void **dev_ptr) {
    if (!cc || !dev_ptr || !cc->s->km) return CNIIC_ERR_BAD_ARG;
    *dev_ptr = km_rgbw_partials_dev(cc->s->km);
    return CNIIC_OK;
}

int32_t cniic_cc_export_labels(cniic_cc *cc, void *dst_dev) {
    if (!cc || !dst_dev) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    return km_rgbw_export_labels(cc->s->km, dst_dev);
}

int32_t cniic_cc_import_labels(cniic_cc *cc, const void *src_dev) {
    if (!cc || !src_dev) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    return km_rgbw_import_labels(cc->s->km, src_dev);
}

int32_t cniic_cc_finish(cniic_cc *cc, const uint8_t *rgb, uint32_t w, uint32_t h, const uint32_t *local_table_dev, uint8_t *out,
                        uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    if (!rgb || !out || !len) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish: null argument");
    if (local_table_dev && !is_device_ptr(local_table_dev)) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish: local table must be device memory");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, (uint64_t)w * h * 3));
    return cc_finish(cc->s, in.d, w, h, local_table_dev, out, cap, len, stats);
}

int32_t cniic_cc_finish_frames(cniic_cc *cc, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t frames, uint8_t *out, uint64_t stride,
                               uint64_t *lens, cniic_kmeans_stats *stats) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    if (!rgb || !out || !lens || !frames) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames: null argument");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, (uint64_t)w * h * 3 * frames));
    return cc_finish_frames(cc->s, in.d, w, h, frames, out, stride, lens, stats);
}

int32_t cniic_cc_finish_frames_var(cniic_cc *cc, const uint8_t *rgb, const uint32_t *w, const uint32_t *h, uint32_t frames, uint8_t *out, uint64_t stride,
                                   uint64_t *lens, cniic_kmeans_stats *stats) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    if (!rgb || !w || !h || !out || !lens || !frames) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames_var: null argument");
    uint64_t n = 0;
    for (uint32_t f = 0; f < frames; f++) {
        const uint64_t np = (uint64_t)w[f] * h[f];
        if (!np) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames_var: frame %u is %u x %u", f, w[f], h[f]);
        if (__builtin_add_overflow(n, np, &n) || n > (~0ull) / 3) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames_var: too many pixels");
    }
    if (stride & 3) return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames_var: the stride between streams must be a multiple of 4");   // (before the image is bound)
    if (cc->s->sp_mode && cc->s->sp.npx != n)
        return c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames_var: the session was opened on %llu pixels, the batch has %llu", (unsigned long long)cc->s->sp.npx,
                       (unsigned long long)n);
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, n * 3));
    return cc_finish_frames_var(cc->s, in.d, w, h, frames, out, stride, lens, stats);
}

void cniic_cc_destroy(cniic_cc *cc) {
    if (!cc) return;
    {
        std::lock_guard<std::mutex> lk(cc->c->mu);
        (void)hipSetDevice(cc->c->device);
        (void)hipStreamSynchronize(cc->c->stream);
        PoolScope ps(&cc->c->pool);
        delete cc->s;
    }
    delete cc;
}

// ------------------------------------------------------------------ frozen palettes
int32_t cniic_cc_palette(cniic_cc *cc, uint8_t *centroids, uint64_t *pixels) {
    if (!cc) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(cc->c);
    LOCK(c);
    if (!cc->s->km) return c->fail(CNIIC_ERR_BAD_ARG, "the session has no K-means state yet (cniic_cc_image_create comes first)");
    if (!centroids) return c->fail(CNIIC_ERR_BAD_ARG, "cc_palette: null argument");
    return cc_palette(cc->s, centroids, pixels);
}

struct cniic_palette {
    Ctx *c = nullptr;
    Palette *p = nullptr;
};

int32_t cniic_palette_create(cniic_ctx *c, const uint8_t *centroids, uint32_t K, cniic_palette **out) {
    LOCK(c);
    c->ktimes.clear();
    if (!centroids || !out) return c->fail(CNIIC_ERR_BAD_ARG, "palette_create: null argument");
    if (!K || K > 65536u) return c->fail(CNIIC_ERR_BAD_ARG, "palette_create: K = %u (1 .. 65536)", K);
    std::vector<uint8_t> cent(3 * (size_t)K);
    CNIIC_TRY(from_caller(c, cent.data(), centroids, cent.size()));
    Palette *p = nullptr;
    CNIIC_TRY(palette_create(c, cent.data(), K, &p));
    *out = new cniic_palette{c, p};
    return CNIIC_OK;
}

uint32_t cniic_palette_label_bytes(cniic_palette *pal) { return pal && pal->p && pal->p->wide ? 2 : 1; }

int32_t cniic_palette_labels(cniic_palette *pal, const uint8_t *rgb, uint64_t npx, void *labels) {
    if (!pal) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(pal->c);
    LOCK(c);
    c->ktimes.clear();
    if (!npx) return CNIIC_OK;
    if (!rgb || !labels) return c->fail(CNIIC_ERR_BAD_ARG, "palette_labels: null argument");
    const uint64_t lb = pal->p->wide ? 2 : 1;
    if (npx > (~0ull) / 3) return c->fail(CNIIC_ERR_BAD_ARG, "palette_labels: too many pixels");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, npx * 3));
    // the gather stores 16 labels at a time: device memory on a 16-byte boundary is written in place, anything else through a copy
    const bool dev = is_device_ptr(labels), direct = dev && (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
    DevBuf stage;
    if (!direct) CNIIC_HIP_TRY(c, stage.alloc(npx * lb + 16));
    CNIIC_TRY(palette_labels(pal->p, in.d, npx, direct ? labels : stage.p));
    if (!direct) {
        CNIIC_HIP_TRY(c, hipMemcpyAsync(labels, stage.p, npx * lb, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CNIIC_OK;
}

int32_t cniic_palette_encode_frames_var(cniic_palette *pal, const uint8_t *rgb, const uint32_t *w, const uint32_t *h, uint32_t frames, uint8_t *out,
                                        uint64_t stride, uint64_t *lens) {
    if (!pal) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(pal->c);
    LOCK(c);
    c->ktimes.clear();
    if (!rgb || !w || !h || !out || !lens || !frames) return c->fail(CNIIC_ERR_BAD_ARG, "palette_encode_frames_var: null argument");
    uint64_t n = 0;
    for (uint32_t f = 0; f < frames; f++) {
        const uint64_t np = (uint64_t)w[f] * h[f];
        if (!np) return c->fail(CNIIC_ERR_BAD_ARG, "palette_encode_frames_var: frame %u is %u x %u", f, w[f], h[f]);
        if (__builtin_add_overflow(n, np, &n) || n > (~0ull) / 3) return c->fail(CNIIC_ERR_BAD_ARG, "palette_encode_frames_var: too many pixels");
    }
    if (stride & 3) return c->fail(CNIIC_ERR_BAD_ARG, "palette_encode_frames_var: the stride between streams must be a multiple of 4");   // (before the image is bound)
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, n * 3));
    return palette_encode_frames_var(pal->p, in.d, w, h, frames, out, stride, lens);
}

int32_t cniic_palette_fit_frames_var(cniic_palette *pal, const uint8_t *rgb, const uint32_t *w, const uint32_t *h, uint32_t frames, uint64_t *sse,
                                     uint64_t *pixels) {
    if (!pal) return CNIIC_ERR_BAD_ARG;
    cniic_ctx *c = static_cast<cniic_ctx *>(pal->c);
    LOCK(c);
    c->ktimes.clear();
    if (!rgb || !w || !h || !sse || !frames) return c->fail(CNIIC_ERR_BAD_ARG, "palette_fit_frames_var: null argument");
    uint64_t n = 0;
    for (uint32_t f = 0; f < frames; f++) {
        const uint64_t np = (uint64_t)w[f] * h[f];
        if (!np) return c->fail(CNIIC_ERR_BAD_ARG, "palette_fit_frames_var: frame %u is %u x %u", f, w[f], h[f]);
        if (__builtin_add_overflow(n, np, &n) || n > (~0ull) / 3) return c->fail(CNIIC_ERR_BAD_ARG, "palette_fit_frames_var: too many pixels");
    }
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, n * 3));
    return palette_fit_frames_var(pal->p, in.d, w, h, frames, sse, pixels);
}

void cniic_palette_destroy(cniic_palette *pal) {
    if (!pal) return;
    {
        std::lock_guard<std::mutex> lk(pal->c->mu);
        (void)hipSetDevice(pal->c->device);
        (void)hipStreamSynchronize(pal->c->stream);
        PoolScope ps(&pal->c->pool);
        delete pal->p;
    }
    delete pal;
}

// ------------------------------------------------------------------ remap
int32_t cniic_remap_rgb(cniic_ctx *c, const uint8_t *rgb, uint64_t npx, const uint32_t *keys, const uint32_t *labels, uint64_t U,
                        const uint8_t *centroids, uint32_t K, uint8_t *out_rgb) {
    LOCK(c);
    c->ktimes.clear();
    if (!npx) return CNIIC_OK;
    if (!rgb || !keys || !labels || !centroids || !out_rgb) return c->fail(CNIIC_ERR_BAD_ARG, "remap_rgb: null argument");
    In<uint8_t> in;
    In<uint32_t> k, l;
    CNIIC_TRY(in.bind(c, rgb, npx * 3));
    CNIIC_TRY(k.bind(c, keys, U));
    CNIIC_TRY(l.bind(c, labels, U));
    std::vector<uint8_t> cent(3 * (size_t)K);
    CNIIC_TRY(from_caller(c, cent.data(), centroids, cent.size()));
    std::vector<uint32_t> ck(K);
    for (uint32_t i = 0; i < K; i++) ck[i] = ((uint32_t)cent[3 * i] << 16) | ((uint32_t)cent[3 * i + 1] << 8) | cent[3 * i + 2];
    DevBuf ck_d, lut_d;
    CNIIC_HIP_TRY(c, ck_d.alloc((uint64_t)K * 4));
    CNIIC_HIP_TRY(c, lut_d.alloc(U * 4));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(ck_d.p, ck.data(), (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, 24, &table));
    CNIIC_TRY(rank_from_keys(c, k.d, U, table));
    CNIIC_TRY(label_lut(c, l.d, U, ck_d.as<uint32_t>(), lut_d.as<uint32_t>()));
    Out<uint8_t> o;
    CNIIC_TRY(o.bind(c, out_rgb, npx * 3));
    {
        ScopedKernelTimer t(c, "remap_rgb");
        CNIIC_TRY(remap_rgb(c, in.d, npx, table, lut_d.as<uint32_t>(), o.d));
        t.stop(1);
    }
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// ------------------------------------------------------------------ Hilbert + delta
int32_t cniic_hilbert_xy(cniic_ctx *c, uint32_t w, uint32_t h, uint32_t *xy) {
    LOCK(c);
    const uint64_t n = (uint64_t)w * h;
    if (!n) return CNIIC_OK;
    if (!xy) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_xy: null output");
    Out<uint32_t> o;
    CNIIC_TRY(o.bind(c, xy, 2 * n));
    CNIIC_TRY(hilbert_xy(c, w, h, o.d));
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_hilbert_linearize(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out_rgb) {
    LOCK(c);
    const uint64_t n = (uint64_t)w * h;
    if (!n) return CNIIC_OK;
    if (!rgb || !out_rgb) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_linearize: null argument");
    In<uint8_t> in;
    Out<uint8_t> o;
    CNIIC_TRY(in.bind(c, rgb, 3 * n));
    CNIIC_TRY(o.bind(c, out_rgb, 3 * n));
    CNIIC_TRY(hilbert_linearize(c, in.d, w, h, o.d));
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// hilbert.rs:10-32: linearize_rect / linearize_small / linearize_large (k_linearize.hip)
int32_t cniic_hilbert_linearize_count(int32_t method, uint32_t w, uint32_t h, uint64_t *npx) { return linearize_count(method, w, h, npx); }

int32_t cniic_hilbert_linearize_as(cniic_ctx *c, int32_t method, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out_rgb, uint64_t cap_px,
                                   uint64_t *npx) {
    LOCK(c);
    c->ktimes.clear();
    uint64_t need = 0;
    if (linearize_count(method, w, h, &need) != CNIIC_OK)
        return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_linearize_as: unknown method %d, or a %ux%u image is too large", method, w, h);
    if (npx) *npx = need;
    if (cap_px < need)
        return c->fail(CNIIC_ERR_CAPACITY, "hilbert_linearize_as: %llu pixels, capacity %llu", (unsigned long long)need, (unsigned long long)cap_px);
    if (!need) return CNIIC_OK;
    if (!rgb || !out_rgb) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_linearize_as: null argument");
    In<uint8_t> in;
    Out<uint8_t> o;
    CNIIC_TRY(in.bind(c, rgb, 3 * (uint64_t)w * h));
    CNIIC_TRY(o.bind(c, out_rgb, 3 * need));
    CNIIC_TRY(linearize_as(c, method, in.d, w, h, o.d));
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// scripts/experiments/hilbert_distribution.py: how often each neighbour difference occurs along a linear stream, per channel
int32_t cniic_channel_diff_hist(cniic_ctx *c, const uint8_t *lin_rgb, uint64_t npx, uint64_t *counts) {
    LOCK(c);
    c->ktimes.clear();
    if (!counts || (npx && !lin_rgb)) return c->fail(CNIIC_ERR_BAD_ARG, "channel_diff_hist: null argument");
    In<uint8_t> in;
    Out<uint64_t> o;
    CNIIC_TRY(in.bind(c, lin_rgb, 3 * npx));
    CNIIC_TRY(o.bind(c, counts, 3 * 511));
    CNIIC_TRY(channel_diff_hist(c, in.d, npx, o.d));
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_hilbert_delta(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t *syms) {
    LOCK(c);
    c->ktimes.clear();
    const uint64_t n = (uint64_t)w * h;
    if (!n) return CNIIC_OK;
    if (!rgb || !syms) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_delta: null argument");
    In<uint8_t> in;
    Out<uint32_t> o;
    CNIIC_TRY(in.bind(c, rgb, 3 * n));
    CNIIC_TRY(o.bind(c, syms, n));
    CNIIC_TRY(hilbert_delta(c, in.d, w, h, o.d, nullptr));
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_hilbert_delta_hist(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t *keys, uint64_t *counts,
                                 uint64_t cap, uint64_t *n_unique, uint32_t *syms) {
    LOCK(c);
    c->ktimes.clear();
    const uint64_t n = (uint64_t)w * h;
    if (n_unique) *n_unique = 0;
    if (!n) return CNIIC_OK;
    if (!rgb) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_delta_hist: null image");
    In<uint8_t> in;
    Out<uint32_t> so;
    CNIIC_TRY(in.bind(c, rgb, 3 * n));
    CNIIC_TRY(so.bind(c, syms, n));
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, 27, &table));
    CNIIC_TRY(hilbert_delta(c, in.d, w, h, so.d, table));
    CNIIC_TRY(so.finish(c));
    return hist_common(c, 27, table, keys, counts, cap, n_unique);
}

// ------------------------------------------------------------------ H2
int32_t cniic_huf_encode_all(cniic_ctx *c, int32_t sym_kind, const uint32_t *syms, uint64_t n, uint8_t *out, uint64_t cap,
                             uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (sym_kind != CNIIC_SYM_RGB && sym_kind != CNIIC_SYM_SIGNED) return c->fail(CNIIC_ERR_BAD_ARG, "huf_encode_all: bad symbol kind");
    if (!syms || !len) return c->fail(CNIIC_ERR_BAD_ARG, "huf_encode_all: null argument");
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "huf_encode_all: too many symbols");
    In<uint32_t> in;
    CNIIC_TRY(in.bind(c, syms, n));
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, sym_kind == CNIIC_SYM_RGB ? 24 : 27, &table));
    std::vector<uint8_t> header;
    return huf_encode_all_dev(c, sym_kind, nullptr, const_cast<uint32_t *>(in.d), false, n, table, false, header, out, cap, len);
}

int32_t cniic_huf_size(int32_t sym_kind, const uint64_t *counts, uint64_t n, uint64_t *nbytes) {
    if (!counts || !nbytes || n == 0 || huff_symbol_size(sym_kind) < 0) return CNIIC_ERR_BAD_ARG;
    HuffTree t;
    std::vector<uint8_t> len;
    std::vector<uint64_t> code;
    if (!huff_build_tree(counts, n, t) || !huff_codes(t, len, code)) return CNIIC_ERR_BAD_ARG;
    *nbytes = huff_stream_size(sym_kind, counts, len.data(), n);
    return CNIIC_OK;
}

// ------------------------------------------------------------------ Codec trait
int32_t cniic_codec_parse(const char *expr, int32_t *kind, uint32_t *arg) {
    CodecDesc d;
    if (!parse_codec(expr, &d) || d.darg != 0.0) return CNIIC_ERR_BAD_ARG;   // (kind, arg) cannot say hilbert(rle(d)), d != 0: cniic_codec_parse_f64
    if (kind) *kind = d.kind;
    if (arg) *arg = d.arg;
    return CNIIC_OK;
}

int32_t cniic_codec_parse_f64(const char *expr, int32_t *kind, uint32_t *arg, double *darg) {
    CodecDesc d;
    if (!parse_codec(expr, &d)) return CNIIC_ERR_BAD_ARG;
    if (kind) *kind = d.kind;
    if (arg) *arg = d.arg;
    if (darg) *darg = d.darg;
    return CNIIC_OK;
}

int32_t cniic_codec_name(const char *expr, char *buf, uint64_t cap) {
    CodecDesc d;
    if (!parse_codec(expr, &d) || !buf) return CNIIC_ERR_BAD_ARG;
    std::string s = codec_name(d);
    if (s.size() + 1 > cap) return CNIIC_ERR_CAPACITY;
    memcpy(buf, s.c_str(), s.size() + 1);
    return CNIIC_OK;
}

int32_t cniic_codec_is_lossless(const char *expr) {
    CodecDesc d;
    if (!parse_codec(expr, &d)) return CNIIC_ERR_BAD_ARG;
    return codec_is_lossless(d) ? 1 : 0;
}

static int32_t decode_batch_locked(cniic_ctx *c, const CodecDesc &d, const char *who, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames,
                                   uint8_t *rgb, uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs, std::vector<std::string> *msgs_out);

// one image under a descriptor, the context's mutex held (the batch engines' workers: the expression was parsed once, by the call)
static int32_t encode_desc_locked(cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *opts, const uint8_t *rgb, uint32_t w, uint32_t h,
                                  uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats) {
    c->ktimes.clear();
    if (!len || (!rgb && (uint64_t)w * h) || !out) return c->fail(CNIIC_ERR_BAD_ARG, "codec_encode: null argument");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, (uint64_t)w * h * 3));
    return codec_encode(c, d, in.d, w, h, opts, out, cap, len, stats);
}

// cniic_codec_encode / cniic_codec_encode_opts, the context's mutex held
static int32_t encode_locked(cniic_ctx *c, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, uint32_t w, uint32_t h,
                             uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats) {
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    return encode_desc_locked(c, d, opts, rgb, w, h, out, cap, len, stats);
}

int32_t cniic_codec_encode(cniic_ctx *c, const char *expr, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap,
                           uint64_t *len, cniic_kmeans_stats *stats) {
    LOCK(c);
    return encode_locked(c, expr, nullptr, rgb, w, h, out, cap, len, stats);
}

int32_t cniic_hilbert_rle_approx_encode(cniic_ctx *c, double d, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap,
                                        uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!rgb && (uint64_t)w * h) || !out) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_rle_approx_encode: null argument");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, (uint64_t)w * h * 3));
    return encode_hilbert_rle(c, d, in.d, w, h, out, cap, len);
}

// ------------------------------------------------------------------ the dictionary coder (zipdict.cpp, k_zipdict.hip)
int32_t cniic_zip_dict_encode(cniic_ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!bytes && n) || (!out && n)) return c->fail(CNIIC_ERR_BAD_ARG, "zip_dict_encode: null argument");
    *len = 0;
    if (!n) return CNIIC_OK;   // (no input, no pair: dict.rs:69-75)
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, bytes, n));
    return zip_dict_encode_text(c, in.d, in.d == bytes ? nullptr : bytes, n, {}, out, cap, len);
}

int32_t cniic_zip_dict_decode(cniic_ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!bytes && n) || (!out && cap)) return c->fail(CNIIC_ERR_BAD_ARG, "zip_dict_decode: null argument");
    *len = 0;
    return zip_dict_decode_bytes(c, bytes, n, out, cap, len);
}

int32_t cniic_zip_dict_dims(const uint8_t *bytes, uint64_t n, uint32_t *w, uint32_t *h) {
    if ((!bytes && n) || !w || !h) return CNIIC_ERR_BAD_ARG;
    return zip_dict_dims(bytes, n, w, h);
}

int32_t cniic_hilbert_zip_encode(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!rgb && (uint64_t)w * h) || !out) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_zip_encode: null argument");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, (uint64_t)w * h * 3));
    return encode_hilbert_zip(c, in.d, w, h, out, cap, len);
}

int32_t cniic_hilbert_zip_decode(cniic_ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *rgb, uint64_t cap, uint32_t *w, uint32_t *h) {
    LOCK(c);
    c->ktimes.clear();
    if (!bytes || !w || !h) return c->fail(CNIIC_ERR_BAD_ARG, "hilbert_zip_decode: null argument");
    return decode_hilbert_zip(c, bytes, n, rgb, cap, w, h);
}

// ------------------------------------------------------------------ the look-back coder (zipback.cpp, k_zipback.hip)
int32_t cniic_zip_back_encode(cniic_ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!bytes && n) || (!out && n)) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_encode: null argument");
    *len = 0;
    if (!n) return CNIIC_OK;   // (no input, no symbol: back.rs:727-729)
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, bytes, n));
    return zip_back_encode_text(c, in.d, n, out, cap, len);
}

int32_t cniic_zip_back_decode(cniic_ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!bytes && n) || (!out && cap)) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_decode: null argument");
    *len = 0;
    if (!n) return CNIIC_OK;
    return zip_back_decode_bytes(c, bytes, n, out, cap, len);
}

int32_t cniic_zip_back_dims(const uint8_t *bytes, uint64_t n, uint32_t *w, uint32_t *h) {
    if ((!bytes && n) || !w || !h) return CNIIC_ERR_BAD_ARG;
    return zip_back_dims(bytes, n, n, w, h);
}

int32_t cniic_zip_back_image_encode(cniic_ctx *c, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    LOCK(c);
    c->ktimes.clear();
    if (!len || (!rgb && (uint64_t)w * h) || !out) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_image_encode: null argument");
    const uint64_t off = 0;
    return encode_zip_back_batch(c, rgb, &off, &w, &h, 1, out, cap, len, nullptr);
}

int32_t cniic_zip_back_image_decode(cniic_ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *rgb, uint64_t cap, uint32_t *w, uint32_t *h) {
    LOCK(c);
    c->ktimes.clear();
    if (!bytes || !w || !h) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_image_decode: null argument");
    return decode_zip_back_batch(c, bytes, 0, &n, 1, rgb, cap, w, h, nullptr);
}

int32_t cniic_zip_back_image_encode_batch_var(cniic_ctx *c, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                              uint8_t *out, uint64_t stride, uint64_t *lens, int32_t *rcs) {
    LOCK(c);
    c->ktimes.clear();
    if (!frames) return CNIIC_OK;
    if (!img_off || !w || !h || !out || !lens) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_image_encode_batch_var: null argument");
    for (uint32_t f = 0; f < frames; f++)
        if (!rgb && (uint64_t)w[f] * h[f]) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_image_encode_batch_var: null images");
    return encode_zip_back_batch(c, rgb, img_off, w, h, frames, out, stride, lens, rcs);
}

int32_t cniic_zip_back_image_decode_batch(cniic_ctx *c, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames, uint8_t *rgb,
                                          uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs) {
    LOCK(c);
    c->ktimes.clear();
    if (!frames) return CNIIC_OK;
    if (!bytes || !lens || !w || !h || (!rgb && img_stride)) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_image_decode_batch: null argument");
    return decode_zip_back_batch(c, bytes, stride, lens, frames, rgb, img_stride, w, h, rcs);
}

int32_t cniic_codec_encode_opts(cniic_ctx *c, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, uint32_t w,
                                uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats) {
    LOCK(c);
    return encode_locked(c, expr, opts, rgb, w, h, out, cap, len, stats);
}

int32_t cniic_codec_encode_warm(cniic_ctx *c, const char *expr, const cniic_kmeans_opts *opts, const void *init, const uint8_t *rgb, uint32_t w, uint32_t h,
                                uint8_t *out, uint64_t cap, uint64_t *len, void *centroids_out, cniic_kmeans_stats *stats) {
    LOCK(c);
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    if (!len || (!rgb && (uint64_t)w * h) || !out) return c->fail(CNIIC_ERR_BAD_ARG, "codec_encode_warm: null argument");
    if (!init || is_device_ptr(init) || (centroids_out && is_device_ptr(centroids_out)))
        return c->fail(CNIIC_ERR_BAD_ARG, "codec_encode_warm: init and centroids_out are host memory");
    In<uint8_t> in;
    CNIIC_TRY(in.bind(c, rgb, (uint64_t)w * h * 3));
    return codec_encode_warm(c, d, in.d, w, h, opts, init, out, cap, len, centroids_out, stats);
}

// The worker contexts of a batch call of n > 0 frames: S = min(n, CNIIC_OPT_BATCH_STREAMS, 8 unless set) of them, created on first use,
// with this context's route switches and its injected scan (a view of this context's table).  Returns S, or 0 when a worker could not be
// created: the message is set and the call's status is CNIIC_ERR_HIP (all that creating a context on this context's device can answer).
static uint32_t batch_workers_ready(cniic_ctx *c, uint32_t n, const char *who) {
    const uint32_t S = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(1, c->opt(CNIIC_OPT_BATCH_STREAMS, nullptr, 8)));
    while (c->batch_workers.size() < S) {
        cniic_ctx *wk = nullptr;
        const int32_t rc = cniic_ctx_create(c->device, nullptr, &wk);
        if (rc != CNIIC_OK) { c->fail(rc, "%s: cannot create worker context %zu", who, c->batch_workers.size()); return 0; }
        c->batch_workers.emplace_back(wk);
    }
    for (uint32_t i = 0; i < S; i++) {
        cniic_ctx *wk = c->batch_workers[i].get();
        memcpy(wk->opt_val, c->opt_val, sizeof c->opt_val);
        wk->opt_set = c->opt_set;
        wk->scan_xy.release();
        wk->scan_w = wk->scan_h = 0;
        if (c->scan_xy.p) { wk->scan_xy.view(c->scan_xy.p, c->scan_xy.bytes); wk->scan_w = c->scan_w; wk->scan_h = c->scan_h; }
    }
    return S;
}

// What a batch call answers from its n frames' codes and messages: the first frame that failed decides the call's status and its
// message; rcs_out (optional) takes every frame's code.
static int32_t fold_status(Ctx *c, const int32_t *rcs_in, const std::string *msgs, uint32_t n, int32_t *rcs_out) {
    if (rcs_out) std::copy(rcs_in, rcs_in + n, rcs_out);
    const int32_t *bad = std::find_if(rcs_in, rcs_in + n, [](int32_t rc) { return rc != CNIIC_OK; });
    if (bad == rcs_in + n) return CNIIC_OK;
    c->err = msgs[bad - rcs_in];
    return *bad;
}

// S workers encode side by side: what each gives up so that the others fit
static void batch_workers_share(cniic_ctx *c, uint32_t S) {
    for (uint32_t i = 0; i < S; i++) {
        cniic_ctx *wk = c->batch_workers[i].get();
        // several images in flight: half-size K-means grids, so that two images' launches are resident together (measured on 64 frames
        // 1920 x 1080 with 8 workers: 768 blocks 0.885 ms per frame, 384: 0.729, 192: 0.80, 96: 1.17)
        if (S > 1 && !((c->opt_set >> CNIIC_OPT_KM_MAX_BLOCKS) & 1u) && !getenv("CNIIC_KM_MAX_BLOCKS")) { wk->opt_val[CNIIC_OPT_KM_MAX_BLOCKS] = 384; wk->opt_set |= 1u << CNIIC_OPT_KM_MAX_BLOCKS; }
        wk->ps_div = S;                        // ... and the persistent K-means launch an S-th of the CUs, so that S of them are resident side by side
    }
}

int32_t cniic_codec_encode_batch(cniic_ctx *c, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, uint32_t w, uint32_t h,
                                 uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens, int32_t *rcs, cniic_kmeans_stats *stats) {
    LOCK(c);
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    if (!frames) return CNIIC_OK;
    if (!rgb || !out || !lens) return c->fail(CNIIC_ERR_BAD_ARG, "codec_encode_batch: null argument");
    const uint64_t img_bytes = (uint64_t)w * h * 3;
    const uint32_t S = batch_workers_ready(c, frames, "codec_encode_batch");
    if (!S) return CNIIC_ERR_HIP;
    batch_workers_share(c, S);
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));   // whatever produced the images on this context's stream is done
    std::vector<int32_t> status(frames, CNIIC_OK);
    std::vector<std::string> msg(frames);
    parallel_for(frames, S, [&](uint32_t f, uint32_t i) {
        cniic_ctx *wk = c->batch_workers[i].get();
        cniic_kmeans_stats st{};
        status[f] = cniic_codec_encode_opts(wk, expr, opts, rgb + (uint64_t)f * img_bytes, w, h, out + (uint64_t)f * stride, stride, &lens[f], &st);
        if (status[f] != CNIIC_OK) msg[f] = wk->err;   // (the worker's next frame clears it)
        if (stats) stats[f] = st;
    });
    return fold_status(c, status.data(), msg.data(), frames, rcs);
}

// ---- images of different sizes (cniic_codec_encode_batch_var, cniic_codec_measure_batch)
// (VarFrame, a frame's arguments and results: codec.hpp)

// One frame on a worker context.  A DEVICE image that does not start on a 16-byte boundary would leave the pixel partition of
// cluster-colors and the 16-byte tile reads of `delta` (same bytes, slower routes): it is copied into the worker's aligned scratch
// first, so that a frame costs what it costs alone at an aligned address wherever it lies in the caller's buffer.  (A host image is
// staged into fresh, aligned HBM by the single call already.)
static int32_t encode_var_frame(cniic_ctx *wk, const CodecDesc &d, const cniic_kmeans_opts *opts, bool src_dev, VarFrame &fr) {
    LOCK(wk);
    const uint64_t npx = (uint64_t)fr.w * fr.h;
    if (npx >= (1ull << 32)) return wk->fail(CNIIC_ERR_BAD_ARG, "image too large");   // (codec_encode's answer, before anything is staged)
    const uint8_t *src = fr.src;
    const bool stage = src_dev && npx && (reinterpret_cast<uintptr_t>(src) & 15);
    if (stage) {
        if (wk->batch_stage.bytes < npx * 3) {   // (the largest frames come first: grown once or twice in a batch)
            PoolScope keep(nullptr);             // lives as long as the worker
            CNIIC_HIP_TRY(wk, wk->batch_stage.alloc(npx * 3));
        }
        CNIIC_HIP_TRY(wk, hipMemcpyAsync(wk->batch_stage.p, src, npx * 3, hipMemcpyDeviceToDevice, wk->stream));
        src = wk->batch_stage.as<uint8_t>();
    }
    const int32_t rc = encode_desc_locked(wk, d, opts, src, fr.w, fr.h, fr.out, fr.cap, &fr.len, &fr.st);
    if (stage && wk->timers) wk->ktimes["batch_stage"].launches++;
    return rc;
}

// Every frame of the list encoded exactly as cniic_codec_encode_opts would.  SMALL frames in device memory of the codecs that have a
// small-frame route (kSmallRoutes below; codec.hpp has the routes' contract) are coded together on this context, a workgroup per frame;
// which route a frame took shows in no output byte.  Every other frame goes to the worker contexts of cniic_codec_encode_batch, handed out
// from one queue, LARGEST FIRST: with sizes that differ the last worker to finish then holds a small frame, and frames of one size follow
// one another, which keeps the few scan tables a context caches (`delta`, `hilbert(rle)`) in use.  Which worker takes which frame shows in
// no output.  With the stage timers on, the workers' timers are on too and the context's kernel times are the sums over all frames (a
// route's "<route>_batch": launches = the frames that took it).
//
// The floor of the `hufman` route.  The kernel's time is set by its largest frame (every frame has a CU of its own up to 256 frames: 0.05 ms at 32 x 32,
// 0.11 at 64 x 64, 0.38 - 0.40 from 128 x 96 on), what the workers cost grows with the number of frames.  Measured against the parent
// commit's library (tools/small_hufman_probe.py, profiles/small_hufman_probe.json; NOTES AF), whole call, parent's time / this route's:
//   1 frame:   32 x 32 and 64 x 64 won (1.5x .. 1.9x); 128 x 96, 128 x 128 and 16384 x 1 lost (0.68x .. 0.75x, beyond the spreads)
//   2 frames:  up to 64 x 64 won (2.2x .. 4.3x); the three larger sizes 0.87x .. 1.11x, within the spreads
//   4 frames:  every size won (1.27x .. 4.3x); 8 and more: 2.0x .. 68x
// So in a call with fewer than 4 candidate frames only the frames of at most 4096 pixels take the route (the largest size that won alone;
// the next one measured, 12 288 pixels, lost); with 4 or more every candidate does.  The testing library takes the floor away with
// CNIIC_TEST_HUF_SMALL_FLOOR_OFF=1.
constexpr uint32_t kHufSmallFloorFew = 4;
constexpr uint64_t kHufSmallFloorPxFew = 4096;
static uint64_t huf_small_floor_px(uint64_t candidates, const CodecDesc &) {
    if (const char *e = test_env("CNIIC_TEST_HUF_SMALL_FLOOR_OFF")) if (atoi(e) != 0) return ~0ull;
    return candidates >= kHufSmallFloorFew ? ~0ull : kHufSmallFloorPxFew;
}
// The floor of the voronoi route.  One workgroup on one CU is slower for ONE heavy frame than the workers' whole chip; what the route costs is set by
// its heaviest frame (every frame has a CU of its own up to 256 frames), what the workers cost grows with the number of frames.  Measured
// against the parent commit's library (tools/small_voronoi_probe.py, profiles/small_voronoi_probe.json; NOTES AD), in pixels x K of a frame,
// parent's time / this route's:
//   1 frame:    won at 16 384 .. 65 536 (1.8x .. 2.9x), mixed at 196 608 .. 262 144 (0.65x .. 1.9x), lost from 786 432 on (0.75x .. 0.05x)
//   8 frames:   won up to 786 432 (1.3x .. 7.4x); at 1 048 576 four shapes won (1.05x .. 1.9x) and 16384 x 1 noise lost (0.55x); lost at
//               3 .. 4 M (0.14x .. 0.82x; one shape 1.07x)
//   64 frames:  at 4 194 304 three shapes won (2.4x .. 3.8x) and 16384 x 1 noise lost (0.55x: 31 ms against 0.27 ms a frame on the workers,
//               which breaks even at 117 frames)
//   256 frames and more: every shape won (2.0x .. 126x)
// So a frame takes the route when its pixels x K are at most 131 072 (between the last product that always won and the first that lost) in a
// call with fewer than 8 candidate frames, at most 786 432 (the last that always won) with 8 .. 127, and whatever its product with 128 or
// more.  The other candidates go to the workers like every larger frame.  The testing library takes the floor away with
// CNIIC_TEST_VOR_SMALL_FLOOR_OFF=1.
constexpr uint32_t kVorSmallFloorFew = 8, kVorSmallFloorMany = 128;
constexpr uint64_t kVorSmallFloorWorkFew = 131072, kVorSmallFloorWorkSome = 786432;
static uint64_t vor_small_max_work(uint64_t candidates) {
    if (const char *e = test_env("CNIIC_TEST_VOR_SMALL_FLOOR_OFF")) if (atoi(e) != 0) return ~0ull;
    return candidates >= kVorSmallFloorMany ? ~0ull : candidates >= kVorSmallFloorFew ? kVorSmallFloorWorkSome : kVorSmallFloorWorkFew;
}
static uint64_t vor_small_floor_px(uint64_t candidates, const CodecDesc &d) { return vor_small_max_work(candidates) / d.arg; }   // (pixels x K <= the work)

// The floor of the `hilbert(rle)` / `hilbert(rle(d))` route.  The route's call costs 0.08 - 0.10 ms before the kernel does anything a frame can
// feel, the kernel's time is set by its heaviest frame (every frame has a CU of its own up to 256 frames: 0.04 - 0.05 ms up to 64 x 64;
// 0.08 - 0.11 at 128 x 128 and 16384 x 1; 0.24 at 128 x 96, whose general-rectangle walk is most of it; 0.47 - 0.92 for photo-like frames of
// 12 288 and 16 384 pixels at d = 16, where most starts run tens of f64 tests), what the workers cost grows with the number of frames.
// Measured against the parent commit's library (tools/small_rle_probe.py, profiles/small_rle_probe.json; NOTES AN), d in {0, 4, 16, 441.7},
// whole encode call, parent's time / this route's:
//   1 frame:    0.59x .. 1.27x up to 64 x 64 (5 rows of 16 lost beyond the spreads, 4 won); 0.25x .. 1.15x above (20 of 24 lost)
//   2 frames:   32 x 32 won (1.5x .. 2.2x), 64 x 64 won but for photo-like at d = 16 (0.76x, lost); above 4096 pixels 0.31x .. 0.97x
//               (10 of 24 lost) but for d = 441.7, which tests nothing, at 128 x 128 and 16384 x 1 (1.5x .. 1.7x)
//   4 frames:   up to 64 x 64 every row won (1.34x .. 3.1x; two of the 16 within the spreads, by one slow run of the parent's);
//               above, 128 x 96 lost (0.56x .. 0.79x) and photo-like 128 x 128 at d = 16 lost (0.53x)
//   8 frames:   up to 64 x 64 won (1.9x .. 4.4x); above, photo-like at d = 16 lost (0.75x, 0.77x), 128 x 96 at d = 0 tied (1.01x, 1.14x)
//   16 frames:  up to 64 x 64 won (2.2x .. 6.3x); above, photo-like 128 x 96 at d = 16 lost (0.90x), 128 x 128 tied (0.94x), all else 1.58x and up
//   32 frames:  every row won (1.22x .. 8.7x); 256: 6.9x .. 24x; 4096: 10x .. 29x
// The route's time is flat up to 256 frames and the workers' grows, so a class that won with n frames wins with more.  So: in a call with
// fewer than 4 candidate frames none takes the route; with 4 .. 31 those of at most 4096 pixels do (the largest size at which every d and
// both contents won from 4 frames on); with 32 or more every candidate does.  That leaves with the workers some classes that would have
// won (128 x 128 and 16384 x 1 at d <= 4 from 4 frames on, 1.35x .. 3.3x): the floor knows pixels, not contents, and d = 16 on photo-like
// frames of those sizes lost up to 16 frames.  The testing library takes the floor away with CNIIC_TEST_RLE_SMALL_FLOOR_OFF=1.
constexpr uint32_t kRleSmallFloorNone = 4;
constexpr uint32_t kRleSmallFloorFew = 32;
constexpr uint64_t kRleSmallFloorPxFew = 4096;
static uint64_t rle_small_floor_px(uint64_t candidates, const CodecDesc &) {
    if (const char *e = test_env("CNIIC_TEST_RLE_SMALL_FLOOR_OFF")) if (atoi(e) != 0) return ~0ull;
    return candidates >= kRleSmallFloorFew ? ~0ull : candidates >= kRleSmallFloorNone ? kRleSmallFloorPxFew : 0;
}

// The floor of the `zip(dict)` route.  The coder stays serial inside a frame: one workgroup needs 4.9 - 6.1 ms for a frame of 32 x 32,
// 16 - 22 ms for 64 x 64, 46 - 54 ms for 128 x 96 and 60 - 73 ms for 128 x 128 or 16384 x 1 (k_zd_small's own duration, flat up to 32
// frames; twice that with 256 frames of 12 288 pixels or more), where the host's walk on a worker needs 0.24 / 0.95 / 2.9 / 3.7 ms for one
// such frame and 9.5 / 31 / 95 / 123 ms for 256.  Measured against the parent commit's library (tools/small_zip_probe.py,
// profiles/small_zip_probe.json; NOTES AO), photo-like, uniform noise and photo-like with a flat band, whole encode call, parent's time /
// this route's:
//   1, 4, 8 frames:  every size lost (0.04x .. 0.10x; one row 0.40x by a slow run of the parent's)
//   32 frames:       every size lost (0.19x .. 0.29x)
//   256 frames:      32 x 32 won (1.62x .. 1.67x; the banded row within the spreads), 64 x 64 won (1.35x .. 1.60x); 128 x 96, 128 x 128 and
//                    16384 x 1 lost (0.81x .. 0.87x; banded frames of these sizes, which the kernel gives up half-way, 0.59x)
//   4096 frames:     32 x 32 won (4.1x .. 4.3x), 64 x 64 won (3.0x .. 3.1x); the larger sizes were not probed at this count
// cniic_codec_measure_batch follows (256 frames: 1.27x .. 1.46x; 4096: 1.9x .. 2.4x).  So a frame is a candidate with at most 4096 pixels
// -- the largest size that won -- and the candidates take the route in a call with 256 of them or more, the smallest probed count that
// won; every other frame stays with the workers.  FLAT frames, every one of which the kernel hands back after 3.4 - 3.6 ms (14 - 22 ms
// for 4096 of them), lose that attempt whatever the floor says, since it knows pixels and not contents: 256 flat frames of 32 x 32 0.62x
// (9.4 ms against 5.8), of 64 x 64 0.85x, 4096 of them 0.87x and 0.94x.  The testing library takes the floor away, the pixel bound
// included, with CNIIC_TEST_ZD_SMALL_FLOOR_OFF=1.
constexpr uint32_t kZdSmallFloorFrames = 256;
constexpr uint64_t kZdSmallFloorPx = 4096;
static bool zd_small_floor_off() {
    if (const char *e = test_env("CNIIC_TEST_ZD_SMALL_FLOOR_OFF")) return atoi(e) != 0;
    return false;
}
static uint64_t zd_small_max_px() {
    const uint64_t bound = small_route_max_px("CNIIC_TEST_ZD_SMALL_OFF", "CNIIC_TEST_ZD_SMALL_MAX_PX", kZdSmallMaxPx);
    return zd_small_floor_off() ? bound : std::min(bound, kZdSmallFloorPx);
}
static uint64_t zd_small_floor_px(uint64_t candidates, const CodecDesc &) { return zd_small_floor_off() || candidates >= kZdSmallFloorFrames ? ~0ull : 0; }

// The floor of the Hilbert { compress: Zip } route: NO class of calls takes it in the release library.  The rule is the decode route's (codec.cpp):
// a class, defined by frame count and pixel bound, takes the route only where the route's slowest run beat the workers' fastest for
// photo-like, noise AND flat frames -- and the floor knows pixels, not contents.  Measured against this build with the route off (the worker
// contexts) and against the parent commit's library, which can only loop over cniic_hilbert_zip_encode on one context
// (tools/small_zip_probe.py --codec hilbert-zip, profiles/small_hz_probe.json; NOTES AS), whole encode call, medians of 5, this route / the
// workers.  The coder is `zip(dict)`'s, serial inside a frame: one workgroup needs 4.7 - 5.0 ms for a frame of 32 x 32, 15 - 18 ms for 64 x 64,
// 43 - 50 ms for 128 x 96 and 56 - 66 ms for 128 x 128 or 16384 x 1.
//   1 .. 32 frames:  every size and content lost (4.3 - 66 ms against 0.2 - 23 ms)
//   256 frames:      photo-like and noise: 32 x 32 won (5.0 ms against 9.6 - 9.9), 64 x 64 won (16.8 - 18.7 against 30.1 - 34.3), 128 x 96,
//                    128 x 128 and 16384 x 1 did not (103 - 136 ms against 92 - 134).  FLAT frames, every one of which the kernel hands back
//                    after 3.3 - 3.7 ms, lost: 32 x 32 9.3 - 9.4 ms against 5.4 - 5.7, 64 x 64 24.5 - 27.1 against 20.4 - 20.8
//   4096 frames:     photo-like and noise: 32 x 32 won (31.1 - 33.3 ms against 143 - 146), 64 x 64 won (141 - 148 against 459 - 479).  Flat
//                    frames lost again: 32 x 32 103 - 104 ms against 87 - 90, 64 x 64 325 - 327 against 302 - 310
// So no probed class is clear for all three contents, and every frame stays with the workers.  What that leaves on the table: 1.6x - 4.6x
// for calls of 256 and more photo-like or noise frames of at most 4096 pixels; what it avoids: 0.6x - 0.9x for flat ones.  A check of the
// content cheap enough to go in front of the kernel would change this; none is built.  The route is reached with
// CNIIC_TEST_HZ_SMALL_FLOOR_OFF=1 (the testing library), which the tests and the probe set.
static bool hz_small_floor_off() {
    if (const char *e = test_env("CNIIC_TEST_HZ_SMALL_FLOOR_OFF")) return atoi(e) != 0;
    return false;
}
static uint64_t hz_small_max_px() { return small_route_max_px("CNIIC_TEST_HZ_SMALL_OFF", "CNIIC_TEST_HZ_SMALL_MAX_PX", kHzSmallMaxPx); }
static uint64_t hz_small_floor_px(uint64_t, const CodecDesc &) { return hz_small_floor_off() ? ~0ull : 0; }

// A small-frame route of encode_frames.  A frame is a CANDIDATE when the route applies to the call and the frame has 1 .. max_px() pixels;
// a candidate takes the route unless the floor or `takes` keeps it with the workers.  (max_px is a function, not its knobs' names: those
// must not be in the release library, and small_route_max_px folds them away only as arguments of a call.)
struct SmallRoute {
    bool (*applies)(const cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *opts);   // the codec, its argument, the call's options
    uint64_t (*max_px)();                                                                     // the route's bound under its _OFF and _MAX_PX knobs
    uint64_t (*floor)(uint64_t candidates, const CodecDesc &d);                               // null, or: the most pixels of a frame in a call with so many candidates
    bool (*takes)(const cniic_ctx *c, const VarFrame &f);                                     // null, or: a veto on one frame
    int (*run)(cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n);
};
static bool no_flags(const cniic_kmeans_opts *opts) { return !opts || opts->flags == 0; }
static const SmallRoute kSmallRoutes[] = {
    {[](const cniic_ctx *, const CodecDesc &d, const cniic_kmeans_opts *opts) { return d.kind == CODEC_CLUSTER_COLORS && d.arg >= 1 && d.arg <= kCcSmallMaxK && no_flags(opts); },
     [] { return small_route_max_px("CNIIC_TEST_CC_SMALL_OFF", "CNIIC_TEST_CC_SMALL_MAX_PX", kCcSmallMaxPx); }, nullptr, nullptr,
     [](cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n) { return cc_small_encode(c, d.arg, opts, fr, n); }},
    {[](const cniic_ctx *, const CodecDesc &d, const cniic_kmeans_opts *opts) { return d.kind == CODEC_VORONOI && d.arg >= 1 && d.arg <= kVorSmallMaxK && no_flags(opts); },
     [] { return small_route_max_px("CNIIC_TEST_VOR_SMALL_OFF", "CNIIC_TEST_VOR_SMALL_MAX_PX", kVorSmallMaxPx); }, vor_small_floor_px, nullptr,
     [](cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n) { return vor_small_encode(c, d.arg, opts, fr, n); }},
    // `delta`: not with the big encoder's route forced, and not a frame whose size has an injected scan
    {[](const cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *) { return d.kind == CODEC_DELTA && c->opt(CNIIC_OPT_DELTA_ROUTE, "CNIIC_DELTA_ROUTE", 0) != 32; },
     [] { return small_route_max_px("CNIIC_TEST_DELTA_SMALL_OFF", "CNIIC_TEST_DELTA_SMALL_MAX_PX", kDeltaSmallMaxPx); }, nullptr,
     [](const cniic_ctx *c, const VarFrame &f) { return !(c->scan_xy.p && c->scan_w == f.w && c->scan_h == f.h); },
     [](cniic_ctx *c, const CodecDesc &, const cniic_kmeans_opts *, VarFrame *const *fr, uint32_t n) { return delta_small_encode(c, fr, n); }},
    {[](const cniic_ctx *, const CodecDesc &d, const cniic_kmeans_opts *opts) { return d.kind == CODEC_HUFMAN && no_flags(opts); },
     [] { return small_route_max_px("CNIIC_TEST_HUF_SMALL_OFF", "CNIIC_TEST_HUF_SMALL_MAX_PX", kHufSmallMaxPx); }, huf_small_floor_px, nullptr,
     [](cniic_ctx *c, const CodecDesc &, const cniic_kmeans_opts *, VarFrame *const *fr, uint32_t n) { return huf_small_encode(c, fr, n); }},
    // `hilbert(rle)` and `hilbert(rle(d))`, any d: not a frame whose size has an injected scan, which the workers follow
    {[](const cniic_ctx *, const CodecDesc &d, const cniic_kmeans_opts *) { return d.kind == CODEC_HILBERT_RLE; },
     [] { return small_route_max_px("CNIIC_TEST_RLE_SMALL_OFF", "CNIIC_TEST_RLE_SMALL_MAX_PX", kRleSmallMaxPx); }, rle_small_floor_px,
     [](const cniic_ctx *c, const VarFrame &f) { return !(c->scan_xy.p && c->scan_w == f.w && c->scan_h == f.h); },
     [](cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *, VarFrame *const *fr, uint32_t n) { return rle_small_encode(c, d.darg, fr, n); }},
    // `zip(dict)`, whatever the options hold (the single call ignores them for this codec); a frame the kernel gives up comes back handed_back
    {[](const cniic_ctx *, const CodecDesc &d, const cniic_kmeans_opts *) { return d.kind == CODEC_ZIP_DICT; },
     zd_small_max_px, zd_small_floor_px, nullptr,
     [](cniic_ctx *c, const CodecDesc &, const cniic_kmeans_opts *, VarFrame *const *fr, uint32_t n) { return zd_small_encode(c, fr, n); }},
    // Hilbert { compress: Zip } (the internal kind of cniic_hilbert_zip_encode_batch_var): not a frame whose size has an injected scan, which the
    // workers follow; a frame the kernel gives up comes back handed_back
    {[](const cniic_ctx *, const CodecDesc &d, const cniic_kmeans_opts *) { return d.kind == CODEC_HILBERT_ZIP; },
     hz_small_max_px, hz_small_floor_px,
     [](const cniic_ctx *c, const VarFrame &f) { return !(c->scan_xy.p && c->scan_w == f.w && c->scan_h == f.h); },
     [](cniic_ctx *c, const CodecDesc &, const cniic_kmeans_opts *, VarFrame *const *fr, uint32_t n) { return hz_small_encode(c, fr, n); }},
};

static int32_t encode_frames(cniic_ctx *c, const CodecDesc &d, const cniic_kmeans_opts *opts, std::vector<VarFrame> &fr, bool src_dev, const char *who) {
    const uint32_t n = (uint32_t)fr.size();
    if (!n) return CNIIC_OK;
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const uint64_t px = (uint64_t)fr[x].w * fr[x].h, py = (uint64_t)fr[y].w * fr[y].h;
        if (px != py) return px > py;
        if (fr[x].w != fr[y].w) return fr[x].w > fr[y].w;
        return x < y;
    });
    std::map<std::string, KernelTime> kt;
    // ---- the small frames of a codec that has a route for them, together
    const bool routable = src_dev;
    for (const SmallRoute &r : kSmallRoutes) {
        if (!routable || !r.applies(c, d, opts)) continue;
        const uint64_t max_px = r.max_px();
        auto candidate = [&](const VarFrame &f) { const uint64_t px = (uint64_t)f.w * f.h; return px >= 1 && px <= max_px; };
        uint64_t candidates = 0;
        for (uint32_t j : order) candidates += candidate(fr[j]);
        const uint64_t floor_px = r.floor ? r.floor(candidates, d) : ~0ull;   // (the floor: few heavy frames -- the workers are faster)
        std::vector<VarFrame *> small;
        std::vector<uint32_t> rest;
        for (uint32_t j : order) {
            VarFrame &f = fr[j];
            if (candidate(f) && (uint64_t)f.w * f.h <= floor_px && (!r.takes || r.takes(c, f))) small.push_back(&f); else rest.push_back(j);
        }
        if (small.empty()) continue;
        std::map<std::string, KernelTime> mine;
        mine.swap(c->ktimes);   // (the route's stage times alone, added to the workers' below)
        const int32_t rc = r.run(c, d, opts, small.data(), (uint32_t)small.size());
        mine.swap(c->ktimes);
        CNIIC_TRY(rc);
        if (c->timers) for (const auto &e : mine) { kt[e.first].ms += e.second.ms; kt[e.first].launches += e.second.launches; }
        // (a frame the route handed back joins the workers' frames, at its place in the order)
        if (std::any_of(small.begin(), small.end(), [](const VarFrame *f) { return f->handed_back; })) {
            std::vector<uint8_t> stays(n, 0);
            for (uint32_t j : rest) stays[j] = 1;
            for (VarFrame *f : small) if (f->handed_back) { stays[f - fr.data()] = 1; f->handed_back = false; }
            rest.clear();
            for (uint32_t j : order) if (stays[j]) rest.push_back(j);
        }
        order.swap(rest);
    }
    const uint32_t nw = (uint32_t)order.size();
    if (!nw) {
        if (c->timers) c->ktimes.swap(kt);
        return CNIIC_OK;
    }
    const uint32_t S = batch_workers_ready(c, nw, who);
    if (!S) return CNIIC_ERR_HIP;
    batch_workers_share(c, S);
    std::vector<uint8_t> saved_timers(S);
    for (uint32_t i = 0; i < S; i++) {
        cniic_ctx *wk = c->batch_workers[i].get();
        saved_timers[i] = wk->timers;
        wk->timers = wk->timers || c->timers;
    }
    std::mutex kt_mu;
    parallel_for(nw, S, [&](uint32_t j, uint32_t i) {
        cniic_ctx *wk = c->batch_workers[i].get();
        VarFrame &f = fr[order[j]];
        f.rc = encode_var_frame(wk, d, opts, src_dev, f);
        if (f.rc != CNIIC_OK) f.msg = wk->err;
        if (c->timers) {
            std::lock_guard<std::mutex> lk(kt_mu);
            for (const auto &e : wk->ktimes) { kt[e.first].ms += e.second.ms; kt[e.first].launches += e.second.launches; }
        }
    });
    for (uint32_t i = 0; i < S; i++) c->batch_workers[i]->timers = saved_timers[i] != 0;
    if (c->timers) c->ktimes.swap(kt);
    return CNIIC_OK;
}

// cniic_codec_encode_batch_var under a descriptor, the context's mutex held (who: the entry point's name in its messages)
static int32_t encode_batch_var_locked(cniic_ctx *c, const CodecDesc &d, const char *who, const cniic_kmeans_opts *opts, const uint8_t *rgb, const uint64_t *img_off,
                                       const uint32_t *w, const uint32_t *h, uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens, int32_t *rcs,
                                       cniic_kmeans_stats *stats) {
    if (!frames) return CNIIC_OK;
    if (!rgb || !img_off || !w || !h || !out || !lens) return c->fail(CNIIC_ERR_BAD_ARG, "%s: null argument", who);
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));   // whatever produced the images on this context's stream is done
    std::vector<VarFrame> fr(frames);
    for (uint32_t f = 0; f < frames; f++) {
        fr[f].src = rgb + img_off[f]; fr[f].w = w[f]; fr[f].h = h[f];
        fr[f].out = out + (uint64_t)f * stride; fr[f].cap = stride;
    }
    CNIIC_TRY(encode_frames(c, d, opts, fr, is_device_ptr(rgb), who));
    std::vector<int32_t> status(frames);
    std::vector<std::string> msg(frames);
    for (uint32_t f = 0; f < frames; f++) {
        lens[f] = fr[f].len;
        if (stats) stats[f] = fr[f].st;
        status[f] = fr[f].rc;
        msg[f].swap(fr[f].msg);
    }
    return fold_status(c, status.data(), msg.data(), frames, rcs);
}

int32_t cniic_codec_encode_batch_var(cniic_ctx *c, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, const uint64_t *img_off,
                                     const uint32_t *w, const uint32_t *h, uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens,
                                     int32_t *rcs, cniic_kmeans_stats *stats) {
    LOCK(c);
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    return encode_batch_var_locked(c, d, "codec_encode_batch_var", opts, rgb, img_off, w, h, frames, out, stride, lens, rcs, stats);
}

// Hilbert { compress: Zip } of many images: the same engine under the internal descriptor (no options, no statistics)
static const CodecDesc kHilbertZipDesc = {CODEC_HILBERT_ZIP, 0, 0.0};
int32_t cniic_hilbert_zip_encode_batch_var(cniic_ctx *c, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t frames, uint8_t *out,
                                           uint64_t stride, uint64_t *lens, int32_t *rcs) {
    LOCK(c);
    c->ktimes.clear();
    return encode_batch_var_locked(c, kHilbertZipDesc, "hilbert_zip_encode_batch_var", nullptr, rgb, img_off, w, h, frames, out, stride, lens, rcs, nullptr);
}

int32_t cniic_codec_decode(cniic_ctx *c, const char *expr, const uint8_t *bytes, uint64_t n, uint8_t *rgb, uint64_t cap, uint32_t *w,
                           uint32_t *h) {
    LOCK(c);
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    if (!bytes || !w || !h) return c->fail(CNIIC_ERR_BAD_ARG, "codec_decode: null argument");
    return codec_decode(c, d, bytes, n, rgb, cap, w, h);  // (the stream may be in host memory or in HBM)
}

int32_t cniic_codec_decode_batch(cniic_ctx *c, const char *expr, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames,
                                 uint8_t *rgb, uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs) {
    LOCK(c);
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    return decode_batch_locked(c, d, "codec_decode_batch", bytes, stride, lens, frames, rgb, img_stride, w, h, rcs, nullptr);
}

int32_t cniic_hilbert_zip_decode_batch(cniic_ctx *c, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames, uint8_t *rgb, uint64_t img_stride,
                                       uint32_t *w, uint32_t *h, int32_t *rcs) {
    LOCK(c);
    return decode_batch_locked(c, kHilbertZipDesc, "hilbert_zip_decode_batch", bytes, stride, lens, frames, rgb, img_stride, w, h, rcs, nullptr);
}

// one stream under a descriptor on a worker context (cniic_codec_decode without the parse)
static int32_t decode_desc(cniic_ctx *c, const CodecDesc &d, const uint8_t *bytes, uint64_t n, uint8_t *rgb, uint64_t cap, uint32_t *w, uint32_t *h) {
    LOCK(c);
    c->ktimes.clear();
    if (!bytes || !w || !h) return c->fail(CNIIC_ERR_BAD_ARG, "codec_decode: null argument");
    return codec_decode(c, d, bytes, n, rgb, cap, w, h);
}

// cniic_codec_decode_batch under a descriptor, the context's mutex held (who: the entry point's name in its messages; msgs_out: every frame's own message)
static int32_t decode_batch_locked(cniic_ctx *c, const CodecDesc &d, const char *who, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames,
                                   uint8_t *rgb, uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs, std::vector<std::string> *msgs_out) {
    c->ktimes.clear();
    if (!frames) return CNIIC_OK;
    if (!bytes || !lens || !rgb || !w || !h) return c->fail(CNIIC_ERR_BAD_ARG, "%s: null argument", who);
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));   // whatever produced the streams on this context's stream is done
    // `hufman` / `cluster-colors` / `hilbert(rle)` and small `delta`, `voronoi` and `zip(dict)` frames: decoded together (codec_decode_batch_route;
    // "delta_small_dec_batch" counts the `delta` frames its one launch was given); the rest, each on its own on the workers
    std::vector<uint8_t> taken;
    std::vector<int32_t> status;
    std::vector<std::string> msg;
    CNIIC_TRY(codec_decode_batch_route(c, d, bytes, stride, lens, frames, rgb, img_stride, w, h, taken, status, msg));
    std::vector<uint32_t> rest;
    for (uint32_t f = 0; f < frames; f++) if (!taken[f]) rest.push_back(f);
    if (!rest.empty()) {
        const uint32_t S = batch_workers_ready(c, (uint32_t)rest.size(), who);
        if (!S) return CNIIC_ERR_HIP;
        parallel_for((uint32_t)rest.size(), S, [&](uint32_t j, uint32_t i) {
            cniic_ctx *wk = c->batch_workers[i].get();
            const uint32_t f = rest[j];
            status[f] = decode_desc(wk, d, bytes + (uint64_t)f * stride, lens[f], rgb + (uint64_t)f * img_stride, img_stride, &w[f], &h[f]);
            if (status[f] != CNIIC_OK) msg[f] = wk->err;
        });
    }
    const int32_t first = fold_status(c, status.data(), msg.data(), frames, rcs);
    if (msgs_out) msgs_out->swap(msg);
    return first;
}

int32_t cniic_mse(cniic_ctx *c, const uint8_t *a, const uint8_t *b, uint64_t npx, double *mse) {
    LOCK(c);
    if (!mse || ((!a || !b) && npx)) return c->fail(CNIIC_ERR_BAD_ARG, "mse: null argument");
    In<uint8_t> ia, ib;
    CNIIC_TRY(ia.bind(c, a, npx * 3));
    CNIIC_TRY(ib.bind(c, b, npx * 3));
    return mse_rgb(c, ia.d, ib.d, npx, mse);
}

int32_t cniic_mse_batch(cniic_ctx *c, const uint8_t *a, const uint8_t *b, uint64_t npx, uint32_t frames, double *mse) {
    LOCK(c);
    if (!frames) return CNIIC_OK;
    if (!mse || ((!a || !b) && npx)) return c->fail(CNIIC_ERR_BAD_ARG, "mse_batch: null argument");
    In<uint8_t> ia, ib;
    CNIIC_TRY(ia.bind(c, a, npx * 3 * frames));
    CNIIC_TRY(ib.bind(c, b, npx * 3 * frames));
    return mse_rgb_batch(c, ia.d, ib.d, npx, frames, mse);
}

// cniic_mse_batch_var, the context's mutex held.  A host side is staged as ONE range, from its first pair's first byte to its last pair's last.
static int32_t mse_batch_var_locked(cniic_ctx *c, const uint8_t *a, const uint64_t *a_off, const uint8_t *b, const uint64_t *b_off, const uint64_t *npx,
                                    uint32_t frames, double *mse) {
    uint64_t lo[2] = {~0ull, ~0ull}, hi[2] = {0, 0};
    for (uint32_t f = 0; f < frames; f++) {
        if (npx[f] >= (1ull << 61)) return c->fail(CNIIC_ERR_BAD_ARG, "mse_batch_var: pair %u has too many pixels", f);
        if (!npx[f]) continue;
        lo[0] = std::min(lo[0], a_off[f]); hi[0] = std::max(hi[0], a_off[f] + npx[f] * 3);
        lo[1] = std::min(lo[1], b_off[f]); hi[1] = std::max(hi[1], b_off[f] + npx[f] * 3);
    }
    if (hi[0] == 0) { for (uint32_t f = 0; f < frames; f++) mse[f] = 0.0; return CNIIC_OK; }
    if (!a || !b) return c->fail(CNIIC_ERR_BAD_ARG, "mse_batch_var: null argument");
    // (the kernel reads a + off: a staged side starts at lo, its offsets move down by lo)
    In<uint8_t> in[2];
    const uint8_t *base[2] = {a, b};
    const uint64_t *off[2] = {a_off, b_off};
    std::vector<uint64_t> moved[2];
    for (int s = 0; s < 2; s++) {
        if (is_device_ptr(base[s])) continue;
        CNIIC_TRY(in[s].bind(c, base[s] + lo[s], hi[s] - lo[s]));
        moved[s].assign(off[s], off[s] + frames);
        for (uint32_t f = 0; f < frames; f++) moved[s][f] = npx[f] ? moved[s][f] - lo[s] : 0;
        base[s] = in[s].d;
        off[s] = moved[s].data();
    }
    return mse_rgb_batch_var(c, base[0], base[1], off[0], off[1], npx, frames, mse);
}

int32_t cniic_mse_batch_var(cniic_ctx *c, const uint8_t *a, const uint64_t *a_off, const uint8_t *b, const uint64_t *b_off, const uint64_t *npx,
                            uint32_t frames, double *mse) {
    LOCK(c);
    c->ktimes.clear();
    if (!frames) return CNIIC_OK;
    if (!mse || !a_off || !b_off || !npx) return c->fail(CNIIC_ERR_BAD_ARG, "mse_batch_var: null argument");
    return mse_batch_var_locked(c, a, a_off, b, b_off, npx, frames, mse);
}

// ---- pitched surfaces <-> packed RGB24 frames (cniic_surface_span, cniic_frames_from_surfaces, cniic_frames_to_surfaces)
// one descriptor: nullptr if it is in order (then *first / *end = the bytes of the surface side it spans, *rgb_bytes = 3 w h), else what is wrong
static const char *surface_check(const cniic_surface &s, uint64_t *first, uint64_t *end, uint64_t *rgb_bytes) {
    const uint32_t bpp = surf_bpp(s.format);
    if (!bpp) return "unknown format";
    const uint64_t npx = (uint64_t)s.w * s.h;
    if (!npx || npx >> 32) return "w * h must be in [1, 2^32)";
    const uint64_t row = (uint64_t)s.w * bpp;
    if (s.pitch < row) return "pitch below the row's bytes";
    typedef unsigned __int128 u128;
    u128 e = (u128)s.off + (u128)(s.h - 1) * s.pitch + row;
    uint64_t lo = s.off;
    if (s.format == CNIIC_PX_NV12) {
        if (s.matrix < CNIIC_YUV_601_LIMITED || s.matrix > CNIIC_YUV_709_FULL) return "NV12 needs a CNIIC_YUV_* matrix";
        const uint64_t row_uv = 2 * (((uint64_t)s.w + 1) / 2);
        if (s.pitch_uv < row_uv) return "pitch_uv below the UV row's bytes";
        e = std::max(e, (u128)s.off_uv + (u128)(((uint64_t)s.h + 1) / 2 - 1) * s.pitch_uv + row_uv);
        lo = std::min(lo, s.off_uv);
    }
    if (e >> 64) return "the surface's end does not fit 64 bits";
    *first = lo; *end = (uint64_t)e; *rgb_bytes = npx * 3;
    return nullptr;
}

int32_t cniic_surface_span(const cniic_surface *s, uint64_t *src_end, uint64_t *rgb_bytes) {
    uint64_t first;
    if (!s || !src_end || !rgb_bytes || surface_check(*s, &first, src_end, rgb_bytes)) return CNIIC_ERR_BAD_ARG;
    return CNIIC_OK;
}

// both directions, the context's mutex held: surf = the surface side (read by the import, written by the export), rgb = the packed side
static int32_t surfaces_locked(cniic_ctx *c, const char *who, bool to_surfaces, uint8_t *surf, const cniic_surface *s, uint32_t frames, uint8_t *rgb,
                               const uint64_t *img_off, uint32_t alpha) {
    if (!frames) return CNIIC_OK;
    if (!surf || !s || !rgb || !img_off) return c->fail(CNIIC_ERR_BAD_ARG, "%s: null argument", who);
    if (to_surfaces && alpha > 255) return c->fail(CNIIC_ERR_BAD_ARG, "%s: alpha is a byte", who);
    std::vector<SurfFrame> fr(frames);
    uint64_t lo[2] = {~0ull, ~0ull}, hi[2] = {0, 0};   // [0]: the surface side, [1]: the packed side
    for (uint32_t f = 0; f < frames; f++) {
        uint64_t first, end, bytes;
        if (const char *why = surface_check(s[f], &first, &end, &bytes)) return c->fail(CNIIC_ERR_BAD_ARG, "%s: surface %u: %s", who, f, why);
        if (to_surfaces && (s[f].format == CNIIC_PX_L8 || s[f].format == CNIIC_PX_LA8 || s[f].format == CNIIC_PX_NV12))
            return c->fail(CNIIC_ERR_BAD_ARG, "%s: surface %u: only RGB8, BGR8, RGBA8 and BGRA8 can be written", who, f);
        if (img_off[f] + bytes < bytes) return c->fail(CNIIC_ERR_BAD_ARG, "%s: frame %u ends behind 2^64", who, f);
        fr[f] = {s[f].off, s[f].pitch, s[f].off_uv, s[f].pitch_uv, img_off[f], s[f].w, s[f].h, s[f].format, s[f].matrix};
        lo[0] = std::min(lo[0], first); hi[0] = std::max(hi[0], end);
        lo[1] = std::min(lo[1], img_off[f]); hi[1] = std::max(hi[1], img_off[f] + bytes);
    }
    // a host side lives in scratch from its first used byte to its last: its offsets move down by lo
    const bool surf_host = !is_device_ptr(surf), rgb_host = !is_device_ptr(rgb);
    DevBuf stage[2];
    uint8_t *base[2] = {surf, rgb};
    for (int side = 0; side < 2; side++) {
        if (!(side ? rgb_host : surf_host)) continue;
        CNIIC_HIP_TRY(c, stage[side].alloc(hi[side] - lo[side]));
        if ((side == 1) == to_surfaces)   // the side that is read
            CNIIC_HIP_TRY(c, hipMemcpyAsync(stage[side].p, base[side] + lo[side], hi[side] - lo[side], hipMemcpyHostToDevice, c->stream));
        base[side] = stage[side].as<uint8_t>();
        for (uint32_t f = 0; f < frames; f++) {
            if (side) fr[f].rgb_off -= lo[1];
            else { fr[f].off -= lo[0]; if (fr[f].format == CNIIC_PX_NV12) fr[f].off_uv -= lo[0]; }
        }
    }
    if (to_surfaces) CNIIC_TRY(surf_convert(c, true, base[1], base[0], fr.data(), frames, alpha));
    else CNIIC_TRY(surf_convert(c, false, base[0], base[1], fr.data(), frames, 0));
    // the written side back to a host caller: exactly the bytes the kernel wrote, frame by frame (row by row for a surface)
    if (!to_surfaces && rgb_host)
        for (uint32_t f = 0; f < frames; f++)
            CNIIC_HIP_TRY(c, hipMemcpyAsync(rgb + img_off[f], base[1] + fr[f].rgb_off, 3ull * fr[f].w * fr[f].h, hipMemcpyDeviceToHost, c->stream));
    if (to_surfaces && surf_host)
        for (uint32_t f = 0; f < frames; f++) {
            const uint64_t row = (uint64_t)s[f].w * surf_bpp(s[f].format);
            if (s[f].pitch == row || s[f].h == 1)
                CNIIC_HIP_TRY(c, hipMemcpyAsync(surf + s[f].off, base[0] + fr[f].off, (s[f].h - 1) * s[f].pitch + row, hipMemcpyDeviceToHost, c->stream));
            else
                CNIIC_HIP_TRY(c, hipMemcpy2DAsync(surf + s[f].off, s[f].pitch, base[0] + fr[f].off, s[f].pitch, row, s[f].h, hipMemcpyDeviceToHost, c->stream));
        }
    if (surf_host || rgb_host) CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_frames_from_surfaces(cniic_ctx *c, const uint8_t *src, const cniic_surface *s, uint32_t frames, uint8_t *rgb, const uint64_t *img_off) {
    LOCK(c);
    c->ktimes.clear();
    return surfaces_locked(c, "frames_from_surfaces", false, const_cast<uint8_t *>(src), s, frames, rgb, img_off, 0);
}

int32_t cniic_frames_to_surfaces(cniic_ctx *c, const uint8_t *rgb, const uint64_t *img_off, const cniic_surface *s, uint32_t frames, uint8_t *dst,
                                 uint32_t alpha) {
    LOCK(c);
    c->ktimes.clear();
    return surfaces_locked(c, "frames_to_surfaces", true, dst, s, frames, const_cast<uint8_t *>(rgb), img_off, alpha);
}

// ---- bench::measure_all's loop body for a whole folder (cniic_codec_measure_batch)
// Scratch HBM one chunk of frames may take (streams + decoded images, + the images themselves when they come from host memory); the
// header states it.  Tests make it small (CNIIC_TEST_MEASURE_BUDGET, bytes) so that a handful of small images takes several chunks.
constexpr uint64_t kMeasureBudget = 2ull << 30;
static uint64_t measure_budget() {
    const char *e = test_env("CNIIC_TEST_MEASURE_BUDGET");
    return e ? strtoull(e, nullptr, 10) : kMeasureBudget;
}
// room for any stream of an image of npx pixels (what the Python mirror gives a single encode; a stream that is longer all the same
// is encoded again with the size it asked for)
static uint64_t measure_stream_room(uint64_t npx) { return (64 + npx * 16 + (1ull << 16) + 3) & ~3ull; }

struct MeasureJob {
    cniic_ctx *c; CodecDesc d; const char *who, *who_decode; const cniic_kmeans_opts *opts; bool lossless, src_dev;
    const uint8_t *rgb; const uint64_t *img_off; const uint32_t *w, *h;
    cniic_measure_row *rows; uint8_t *out; uint64_t stride; uint64_t *lens;
    std::vector<std::string> msg;
    // frames `which` (largest first), `room` bytes for each stream: encode -> decode -> MSE with everything in HBM; frames whose stream
    // wants more room are left for the caller in `again` with rows[f].compressed_size = the bytes needed
    int32_t chunk(const std::vector<uint32_t> &which, uint64_t room, std::vector<uint32_t> *again) {
        const uint32_t n = (uint32_t)which.size();
        const uint64_t img_stride = std::max<uint64_t>(16, ((uint64_t)w[which[0]] * h[which[0]] * 3 + 15) & ~15ull);
        DevBuf sbuf, ibuf, hbuf;
        CNIIC_HIP_TRY(c, sbuf.alloc(room * n));
        CNIIC_HIP_TRY(c, ibuf.alloc(img_stride * n));
        std::vector<uint64_t> a_off(n), b_off(n), npx(n), slen(n);
        const uint8_t *a_base = rgb;
        if (!src_dev) {   // host images: uploaded once, 16-byte aligned, for the encode and for the MSE
            CNIIC_HIP_TRY(c, hbuf.alloc(img_stride * n));
            for (uint32_t j = 0; j < n; j++) {
                const uint64_t bytes = (uint64_t)w[which[j]] * h[which[j]] * 3;
                a_off[j] = img_stride * j;
                if (bytes < (3ull << 32))
                    CNIIC_HIP_TRY(c, hipMemcpyAsync(hbuf.as<uint8_t>() + a_off[j], rgb + img_off[which[j]], bytes, hipMemcpyHostToDevice, c->stream));
            }
            CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
            a_base = hbuf.as<uint8_t>();
        } else {
            for (uint32_t j = 0; j < n; j++) a_off[j] = img_off[which[j]];
        }
        std::vector<VarFrame> fr(n);
        for (uint32_t j = 0; j < n; j++) {
            fr[j].src = a_base + a_off[j]; fr[j].w = w[which[j]]; fr[j].h = h[which[j]];
            fr[j].out = sbuf.as<uint8_t>() + room * j; fr[j].cap = room;
        }
        CNIIC_TRY(encode_frames(c, d, opts, fr, true, who));
        std::map<std::string, KernelTime> enc_kt;   // (the decode below starts its stage times afresh: the encode's are added back)
        if (c->timers) enc_kt = c->ktimes;
        for (uint32_t j = 0; j < n; j++) slen[j] = fr[j].rc == CNIIC_OK ? fr[j].len : 0;
        std::vector<uint32_t> w2(n), h2(n);
        std::vector<int32_t> drc(n, CNIIC_OK);
        std::vector<std::string> dmsg;
        (void)decode_batch_locked(c, d, who_decode, sbuf.as<uint8_t>(), room, slen.data(), n, ibuf.as<uint8_t>(), img_stride, w2.data(), h2.data(), drc.data(), &dmsg);
        if (dmsg.size() != n) return CNIIC_ERR_HIP;   // (the batch as a whole failed: the message is the context's)
        for (const auto &e : enc_kt) { c->ktimes[e.first].ms += e.second.ms; c->ktimes[e.first].launches += e.second.launches; }
        for (uint32_t j = 0; j < n; j++) {
            b_off[j] = img_stride * j;
            npx[j] = fr[j].rc == CNIIC_OK && drc[j] == CNIIC_OK ? (uint64_t)fr[j].w * fr[j].h : 0;
        }
        std::vector<double> err(n);
        CNIIC_TRY(mse_batch_var_locked(c, a_base, a_off.data(), ibuf.as<uint8_t>(), b_off.data(), npx.data(), n, err.data()));
        const bool out_dev = out && is_device_ptr(out);
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t f = which[j];
            cniic_measure_row &r = rows[f];
            r.compressed_size = fr[j].len;
            r.kmeans = fr[j].st;
            if (fr[j].rc == CNIIC_ERR_CAPACITY && again) { again->push_back(f); continue; }
            if (lens) lens[f] = fr[j].len;
            r.rc = fr[j].rc != CNIIC_OK ? fr[j].rc : drc[j];
            msg[f] = fr[j].rc != CNIIC_OK ? fr[j].msg : dmsg[j];
            if (r.rc != CNIIC_OK) { if (fr[j].rc != CNIIC_OK) r.compressed_size = 0; continue; }
            r.compression_ratio = (double)fr[j].len / ((double)((uint64_t)fr[j].w * fr[j].h) * 24.0) * 100.0;
            r.error = err[j];
            r.lossless_mismatch = lossless && err[j] != 0.0;
            if (out) {
                if (fr[j].len > stride) {
                    r.rc = CNIIC_ERR_CAPACITY;
                    char buf[160];
                    snprintf(buf, sizeof buf, "measure: stream of frame %u is %llu bytes, %llu between streams", f, (unsigned long long)fr[j].len, (unsigned long long)stride);
                    msg[f] = buf;
                } else if (fr[j].len) {
                    CNIIC_HIP_TRY(c, hipMemcpyAsync(out + (uint64_t)f * stride, fr[j].out, fr[j].len, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
                }
            }
        }
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CNIIC_OK;
    }
};

// cniic_codec_measure_batch under a descriptor, the context's mutex held (who: the entry point's name in its messages)
static int32_t measure_batch_locked(cniic_ctx *c, const CodecDesc &d, const char *who, const cniic_kmeans_opts *opts, const uint8_t *rgb, const uint64_t *img_off,
                                    const uint32_t *w, const uint32_t *h, uint32_t frames, cniic_measure_row *rows, uint8_t *out, uint64_t stride, uint64_t *lens) {
    if (!frames) return CNIIC_OK;
    if (!rgb || !img_off || !w || !h || !rows) return c->fail(CNIIC_ERR_BAD_ARG, "%s: null argument", who);
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));   // whatever produced the images on this context's stream is done
    MeasureJob job{c, d, who, d.kind == CODEC_HILBERT_ZIP ? "hilbert_zip_decode_batch" : "codec_decode_batch", opts, codec_is_lossless(d), is_device_ptr(rgb), rgb, img_off, w, h, rows, out, stride, lens, std::vector<std::string>(frames)};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<uint32_t> order, big;
    for (uint32_t f = 0; f < frames; f++) {
        memset(&rows[f], 0, sizeof rows[f]);
        rows[f].compression_ratio = rows[f].error = nan;
        if (lens) lens[f] = 0;
        if ((uint64_t)w[f] * h[f] >= (1ull << 32)) { rows[f].rc = CNIIC_ERR_BAD_ARG; job.msg[f] = "image too large"; continue; }
        order.push_back(f);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const uint64_t px = (uint64_t)w[x] * h[x], py = (uint64_t)w[y] * h[y];
        return px != py ? px > py : w[x] != w[y] ? w[x] > w[y] : x < y;
    });
    // chunks of the list, largest frames first: as many frames as the budget holds at the size of the chunk's first (one at least)
    const uint64_t budget = measure_budget();
    std::vector<uint32_t> again;
    for (size_t i = 0; i < order.size();) {
        const uint64_t npx0 = (uint64_t)w[order[i]] * h[order[i]], room = measure_stream_room(npx0);
        const uint64_t per = room + (job.src_dev ? 1 : 2) * std::max<uint64_t>(16, (npx0 * 3 + 15) & ~15ull);
        const size_t n = (size_t)std::min<uint64_t>(order.size() - i, std::max<uint64_t>(1, budget / per));
        CNIIC_TRY(job.chunk(std::vector<uint32_t>(order.begin() + i, order.begin() + i + n), room, &again));
        i += n;
    }
    // streams that outgrew their room, with the room they asked for
    std::sort(again.begin(), again.end(), [&](uint32_t x, uint32_t y) { return rows[x].compressed_size != rows[y].compressed_size ? rows[x].compressed_size > rows[y].compressed_size : x < y; });
    for (size_t i = 0; i < again.size();) {
        const uint64_t room = (rows[again[i]].compressed_size + 3) & ~3ull;
        uint64_t img = 0;
        size_t n = 0;
        while (i + n < again.size()) {
            const uint64_t m = std::max(img, std::max<uint64_t>(16, ((uint64_t)w[again[i + n]] * h[again[i + n]] * 3 + 15) & ~15ull));
            if (n && (n + 1) * (room + (job.src_dev ? 1 : 2) * m) > budget) break;
            img = m;
            n++;
        }
        std::vector<uint32_t> part(again.begin() + i, again.begin() + i + n);
        std::sort(part.begin(), part.end(), [&](uint32_t x, uint32_t y) {
            const uint64_t px = (uint64_t)w[x] * h[x], py = (uint64_t)w[y] * h[y];
            return px != py ? px > py : x < y;
        });
        CNIIC_TRY(job.chunk(part, room, nullptr));
        i += n;
    }
    std::vector<int32_t> status(frames);
    for (uint32_t f = 0; f < frames; f++) status[f] = rows[f].rc;
    return fold_status(c, status.data(), job.msg.data(), frames, nullptr);
}

int32_t cniic_codec_measure_batch(cniic_ctx *c, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, const uint64_t *img_off,
                                  const uint32_t *w, const uint32_t *h, uint32_t frames, cniic_measure_row *rows, uint8_t *out, uint64_t stride,
                                  uint64_t *lens) {
    LOCK(c);
    c->ktimes.clear();
    CodecDesc d;
    if (!parse_codec(expr, &d)) return c->fail(CNIIC_ERR_BAD_ARG, "Malformed codec argument: %s", expr ? expr : "(null)");
    return measure_batch_locked(c, d, "codec_measure_batch", opts, rgb, img_off, w, h, frames, rows, out, stride, lens);
}

int32_t cniic_hilbert_zip_measure_batch(cniic_ctx *c, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                        cniic_measure_row *rows, uint8_t *out, uint64_t stride, uint64_t *lens) {
    LOCK(c);
    c->ktimes.clear();
    return measure_batch_locked(c, kHilbertZipDesc, "hilbert_zip_measure_batch", nullptr, rgb, img_off, w, h, frames, rows, out, stride, lens);
}

// Zip::Back has no CodecDesc, so its folder has a chunk loop of its own over the codec's batch calls (zipback.cpp).  A frame's scratch:
// its stream with room for the worst case, the encoder's and the decoder's text (8 + 11 w h bytes each), the decoded image, and the
// image itself when it comes from host memory.  No stream outgrows zb_stream_bound, so no frame is ever encoded twice.
static int32_t zip_back_measure_chunk(cniic_ctx *c, const std::vector<uint32_t> &which, bool src_dev, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w,
                                      const uint32_t *h, cniic_measure_row *rows, uint8_t *out, uint64_t stride, uint64_t *lens, std::vector<std::string> &msg) {
    const uint32_t n = (uint32_t)which.size();
    const uint64_t npx0 = (uint64_t)w[which[0]] * h[which[0]];
    const uint64_t room = (zb_stream_bound(8 + 11 * npx0) + 15) & ~15ull, img_stride = std::max<uint64_t>(16, (npx0 * 3 + 15) & ~15ull);
    DevBuf sbuf, ibuf, hbuf;
    CNIIC_HIP_TRY(c, sbuf.alloc(room * n));
    CNIIC_HIP_TRY(c, ibuf.alloc(img_stride * n));
    std::vector<uint64_t> a_off(n), b_off(n), npx(n), slen(n);
    std::vector<uint32_t> wv(n), hv(n), w2(n), h2(n);
    const uint8_t *a_base = rgb;
    if (!src_dev) CNIIC_HIP_TRY(c, hbuf.alloc(img_stride * n));
    for (uint32_t j = 0; j < n; j++) {
        wv[j] = w[which[j]]; hv[j] = h[which[j]];
        b_off[j] = img_stride * j;
        a_off[j] = src_dev ? img_off[which[j]] : img_stride * j;
        const uint64_t bytes = (uint64_t)wv[j] * hv[j] * 3;
        if (!src_dev && bytes) CNIIC_HIP_TRY(c, hipMemcpyAsync(hbuf.as<uint8_t>() + a_off[j], rgb + img_off[which[j]], bytes, hipMemcpyHostToDevice, c->stream));
    }
    if (!src_dev) {
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        a_base = hbuf.as<uint8_t>();
    }
    std::vector<int32_t> erc(n, CNIIC_OK), drc(n, CNIIC_OK);
    std::vector<std::string> emsg, dmsg;
    const int32_t e = encode_zip_back_batch(c, a_base, a_off.data(), wv.data(), hv.data(), n, sbuf.as<uint8_t>(), room, slen.data(), erc.data(), &emsg);
    if (emsg.size() != n) return e;   // (the batch as a whole failed: the message is the context's)
    std::vector<uint64_t> dlen(n);
    for (uint32_t j = 0; j < n; j++) dlen[j] = erc[j] == CNIIC_OK ? slen[j] : 0;
    const int32_t d = decode_zip_back_batch(c, sbuf.as<uint8_t>(), room, dlen.data(), n, ibuf.as<uint8_t>(), img_stride, w2.data(), h2.data(), drc.data(), &dmsg);
    if (dmsg.size() != n) return d;
    for (uint32_t j = 0; j < n; j++) npx[j] = erc[j] == CNIIC_OK && drc[j] == CNIIC_OK ? (uint64_t)wv[j] * hv[j] : 0;
    std::vector<double> err(n);
    CNIIC_TRY(mse_batch_var_locked(c, a_base, a_off.data(), ibuf.as<uint8_t>(), b_off.data(), npx.data(), n, err.data()));
    const bool out_dev = out && is_device_ptr(out);
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t f = which[j];
        cniic_measure_row &r = rows[f];
        r.rc = erc[j] != CNIIC_OK ? erc[j] : drc[j];
        msg[f] = erc[j] != CNIIC_OK ? emsg[j] : dmsg[j];
        if (r.rc != CNIIC_OK) continue;
        r.compressed_size = slen[j];
        if (lens) lens[f] = slen[j];
        r.compression_ratio = (double)slen[j] / ((double)((uint64_t)wv[j] * hv[j]) * 24.0) * 100.0;
        r.error = err[j];
        r.lossless_mismatch = err[j] != 0.0;
        if (!out) continue;
        if (slen[j] > stride) {
            r.rc = CNIIC_ERR_CAPACITY;
            char buf[160];
            snprintf(buf, sizeof buf, "measure: stream of frame %u is %llu bytes, %llu between streams", f, (unsigned long long)slen[j], (unsigned long long)stride);
            msg[f] = buf;
        } else if (slen[j]) {
            CNIIC_HIP_TRY(c, hipMemcpyAsync(out + (uint64_t)f * stride, sbuf.as<uint8_t>() + room * j, slen[j], out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        }
    }
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int32_t cniic_zip_back_image_measure_batch(cniic_ctx *c, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                           cniic_measure_row *rows, uint8_t *out, uint64_t stride, uint64_t *lens) {
    LOCK(c);
    c->ktimes.clear();
    if (!frames) return CNIIC_OK;
    if (!rgb || !img_off || !w || !h || !rows) return c->fail(CNIIC_ERR_BAD_ARG, "zip_back_image_measure_batch: null argument");
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));   // whatever produced the images on this context's stream is done
    const bool src_dev = is_device_ptr(rgb);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<std::string> msg(frames);
    std::vector<uint32_t> order;
    for (uint32_t f = 0; f < frames; f++) {
        memset(&rows[f], 0, sizeof rows[f]);
        rows[f].compression_ratio = rows[f].error = nan;
        if (lens) lens[f] = 0;
        if ((uint64_t)w[f] * h[f] >= (1ull << 32)) { rows[f].rc = CNIIC_ERR_BAD_ARG; msg[f] = "image too large"; continue; }
        order.push_back(f);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const uint64_t px = (uint64_t)w[x] * h[x], py = (uint64_t)w[y] * h[y];
        return px != py ? px > py : w[x] != w[y] ? w[x] > w[y] : x < y;
    });
    // chunks of the list, largest frames first: as many frames as the budget holds at the size of the chunk's first (one at least)
    const uint64_t budget = measure_budget();
    for (size_t i = 0; i < order.size();) {
        const uint64_t npx0 = (uint64_t)w[order[i]] * h[order[i]];
        const uint64_t per = zb_stream_bound(8 + 11 * npx0) + 16 + 2 * (8 + 11 * npx0 + 255) + (src_dev ? 1 : 2) * std::max<uint64_t>(16, (npx0 * 3 + 15) & ~15ull);
        const size_t n = (size_t)std::min<uint64_t>(order.size() - i, std::max<uint64_t>(1, budget / per));
        CNIIC_TRY(zip_back_measure_chunk(c, std::vector<uint32_t>(order.begin() + i, order.begin() + i + n), src_dev, rgb, img_off, w, h, rows, out, stride, lens, msg));
        i += n;
    }
    std::vector<int32_t> status(frames);
    for (uint32_t f = 0; f < frames; f++) status[f] = rows[f].rc;
    return fold_status(c, status.data(), msg.data(), frames, nullptr);
}

int32_t cniic_synth_image(cniic_ctx *c, int32_t kind, uint64_t seed, uint32_t w, uint32_t h, uint8_t *rgb) {
    LOCK(c);
    const uint64_t n = (uint64_t)w * h;
    if (!n) return CNIIC_OK;
    if (!rgb) return c->fail(CNIIC_ERR_BAD_ARG, "synth_image: null output");
    Out<uint8_t> o;
    CNIIC_TRY(o.bind(c, rgb, 3 * n));
    CNIIC_TRY(synth_image(c, kind, seed, w, h, o.d));
    CNIIC_TRY(o.finish(c));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

}  // extern "C"
