/*
 * cniic_hip.h -- C ABI of the MI355X-native (gfx950) implementation of cniic's per-pixel
 * compression hot path.  This is the drop-in boundary: the entry points are the cut points a
 * Rust `impl Codec` in the reference would bind over FFI (see INTEGRATION.md for the stub).
 * The reference has no FFI of its own (it is a single Rust crate), so each entry point cites the
 * reference function it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - Every function returns int32_t: 0 = OK, negative = error (table below).  Nothing throws or
 *     aborts across the ABI.  cniic_last_error(ctx) returns a message for the last failure.
 *   - The caller owns every buffer.  Unless stated otherwise a data pointer may be HOST memory
 *     or DEVICE (HBM) memory of the context's GPU; the library detects which
 *     (hipPointerGetAttributes) and stages host buffers over PCIe.  Scalar out-params (`uint64_t
 *     *n_unique`, stats structs, ...) are always host memory.
 *   - A cniic_ctx owns one HIP stream plus scratch HBM.  Calls on one ctx are serialised by an
 *     internal mutex; use one ctx per calling thread for concurrency (the reference calls
 *     encode/decode from rayon workers, src/bench.rs:24-28).  No process-global mutable state.
 *   - Functions return after their results are complete (stream synchronised) unless the name
 *     ends in _async.
 *   - STREAM ORDER OF DEVICE BUFFERS.  A context enqueues on ITS stream only (the one given to
 *     cniic_ctx_create, or its own).  A DEVICE buffer handed to any call must be complete with
 *     respect to that stream when the call is made: either the caller produced it on the same
 *     stream, or the caller has synchronised the producing stream (hipStreamSynchronize /
 *     hipDeviceSynchronize / an event the context's stream waits on) first.  The library does
 *     NOT wait for other streams: an image or byte stream still being filled by another stream
 *     is read half-written (round 3: a `delta` decode answered "colour out of range" once in
 *     40 000 fuzz cases because the test filled the stream's buffer on torch's stream and
 *     decoded on a private one; tests/test_stream_order.py replays that input).  Likewise a
 *     device OUTPUT buffer is complete when the call returns, for every stream.  Host buffers
 *     need nothing: they are staged by copies on the context's stream.
 *   - Images are RGB8, row-major, interleaved (image::DynamicImage::to_rgb, row-major pixels()).
 *   - The library fails (CNIIC_ERR_HIP) when no gfx950 device is usable; there is no CPU fallback.
 */
#ifndef CNIIC_HIP_H
#define CNIIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNIIC_OK                   0
#define CNIIC_ERR_BAD_ARG         -1
#define CNIIC_ERR_TOO_FEW_POINTS  -2  /* src/kmeans.rs:67-68   assert!(points_per_cluster > 0)     */
#define CNIIC_ERR_FEW_ACTIVE      -3  /* src/kmeans.rs:41-57   "Not enough active clusters"        */
#define CNIIC_ERR_HIP             -4  /* HIP runtime / no device                                    */
#define CNIIC_ERR_RCCL            -5
#define CNIIC_ERR_DECODE          -6  /* Option::None from a decode path                            */
#define CNIIC_ERR_NOMEM           -7
#define CNIIC_ERR_CAPACITY        -8  /* caller's output buffer too small (needed size is returned) */
#define CNIIC_ERR_UNSUPPORTED     -9

typedef struct cniic_ctx cniic_ctx;

/* ------------------------------------------------------------------ context */
/* device: HIP device ordinal.  stream: an existing hipStream_t to enqueue on (e.g. the caller's
 * torch stream), or NULL to let the context create its own non-blocking stream. */
int32_t     cniic_ctx_create(int32_t device, void *stream, cniic_ctx **out);
void        cniic_ctx_destroy(cniic_ctx *ctx);
const char *cniic_last_error(const cniic_ctx *ctx);
int32_t     cniic_version(void);
/* 1 for libcniic_hip_testing.so (built with -DCNIIC_TESTING: the test-suite's CNIIC_TEST_* / CNIIC_DBG_* / route-forcing environment
 * knobs are compiled in), 0 for the release library libcniic_hip.so, which reads only the option fallbacks documented below. */
int32_t     cniic_is_testing_build(void);
int32_t     cniic_sync(cniic_ctx *ctx);
/* optional helpers so callers without a HIP binding can keep images resident in HBM */
int32_t     cniic_dev_alloc(cniic_ctx *ctx, uint64_t bytes, void **dptr);
int32_t     cniic_dev_free(cniic_ctx *ctx, void *dptr);
int32_t     cniic_memcpy(cniic_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* Route switches and thresholds a host can set per context (a Rust caller has no other way: the CNIIC_* environment variables
 * named beside them are read per call ONLY while an option is unset, and exist for the test-suite).  value semantics per option;
 * cniic_ctx_get_opt returns the effective value (set, or the environment's, or the default). */
#define CNIIC_OPT_SP_MIN_PIXELS      1  /* cluster-colors: images of at least this many pixels take the pixel partition by colour        */
                                        /* super-cell (k_points.hip), smaller ones the dense 2^24 table.  Default 2^20. CNIIC_SP_MIN_PIXELS */
#define CNIIC_OPT_HUF_GPU_CODES_MIN  2  /* huf::encode_all: alphabets of at least this many symbols sort their leaves and derive codes  */
                                        /* and decoder on the GPU (the host only merges).  Default 32768.  CNIIC_HUF_GPU_CODES_MIN        */
#define CNIIC_OPT_GPU_DECODE_MIN     3  /* decode: streams of at least this many symbols use the parallel decoder, shorter ones the host  */
                                        /* walk.  Default 16384.  CNIIC_GPU_DECODE_MIN                                                      */
#define CNIIC_OPT_DELTA_ROUTE        4  /* delta: 0 = 16-bit symbol stream where the image allows (default), 32 = always the 32-bit route. */
                                        /* CNIIC_DELTA_ROUTE                                                                                */
#define CNIIC_OPT_STAGE_TIMERS       5  /* 1: HIP-event timers around the stages of every call (they synchronise; read with              */
                                        /* cniic_last_kernel_time).  Default 0.  CNIIC_KERNEL_TIMERS                                       */
#define CNIIC_OPT_FRAME_TREES_HOST   6  /* cniic_cc_finish_frames: 1 = the frames' Huffman trees on host threads instead of the GPU.       */
                                        /* Default 0.  CNIIC_FRAME_TREES_HOST                                                               */
#define CNIIC_OPT_BATCH_STREAMS      7  /* cniic_codec_encode_batch: images in flight at once (worker streams).  Default 8.               */
#define CNIIC_OPT_KM_MAX_BLOCKS      8  /* cluster-colors: cap on the K-means assign kernel's grid (a multiple of 3; 0 = none, 768 blocks  */
                                        /* on large inputs).  A smaller grid lets the launches of several contexts share the machine:     */
                                        /* cniic_codec_encode_batch gives its workers 384 unless this is set.  CNIIC_KM_MAX_BLOCKS          */
#define CNIIC_OPT_KM_LOOP             9  /* cluster-colors (K <= 256, one GPU): 0 = the K-means loop as ONE persistent launch with the       */
                                        /* points resident in LDS (default; falls back by itself when its grid cannot be resident),     */
                                        /* 1 = one launch per iteration.  CNIIC_KM_LOOP                                                    */
#define CNIIC_OPT_COUNT              10
int32_t     cniic_ctx_set_opt(cniic_ctx *ctx, int32_t opt, uint64_t value);
int32_t     cniic_ctx_unset_opt(cniic_ctx *ctx, int32_t opt);
int32_t     cniic_ctx_get_opt(cniic_ctx *ctx, int32_t opt, uint64_t *value);
/* dominant-kernel timing of the most recent call on this ctx, measured with HIP events on the
 * ctx stream: *ms = summed duration, *launches = number of launches of that kernel.
 * Names: "kmeans_rgbw_persist" (the colour K-means as one persistent launch; "kmeans_rgbw_persist_iters": the same duration, launches =
 * its iterations), "kmeans_rgbw_assign" (... as one launch per iteration), "kmeans_xyrgb_iter", "hist_rgb", "remap_rgb", "huff_pack", "hilbert_delta", "undiff_scatter", "hd_pass0" /
 * "hd_check" / "hd_write", and the five consecutive stages of a `delta` encode, which together are the whole call: "delta_gather",
 * "delta_hist", "delta_tree" (compaction, the leaves' sort, the host's merge, the codes), "huff_pack", "delta_finish".
 * With CNIIC_OPT_STAGE_TIMERS on, the Huffman code stage of a large alphabet adds three marks (launches only, no duration): "huf_tree_runs" =
 * 1 when the tree was built on the GPU from runs of equally frequent leaves, "huf_tree_host" = 1 when it came from the host's merge with
 * codes and decoder from the GPU, "huf_sort_passes" = the 8-bit radix passes of the leaves' sort by count.  None of them for a small
 * alphabet, whose tree and codes are the host's.
 * A single decode whose serialised decoder outgrew the host's looks at the stream, so that the GPU parse (k_trieparse.hip) was tried, adds
 * one of two marks (launches only, no duration): "trie_parse" = 1 when that parse's table decoded the payload, "trie_parse_host" = 1 when
 * the stream was handed to the host's node walk instead (a leaf deeper than 56, a stack deeper than 120, or a payload the table's decoder
 * gave up).  Neither when the host parsed the decoder in its first or second look.
 * The parallel payload decoder (k_hdecode.hip) adds the route it took (launches only, no duration): "hd_phases" = the times the phase maps
 * ran (a stream that does not fall into step), "hd_recheck" = the checks with a look at their result past the two blind ones, "hd_compact" =
 * 1 when the final write copied the kept symbols (k_hd_compact) and 0 when it decoded everything again; and the single decode
 * "hd_host_walk" = 1 when the host's node walk decoded the payload (an image below the GPU's minimum, a leaf deeper than 56, or a payload
 * the parallel decoder gave up with status 2).
 * The small-frame route of `hilbert(rle)` / `hilbert(rle(d))` in cniic_codec_encode_batch_var and cniic_codec_measure_batch (described
 * there): "rle_small_batch" = the duration of k_rle_small, with launches = the frames that took the route; "rle_small_place" = the copy of
 * the finished streams to their destinations, one launch per chunk (none for host destinations).
 * The small-frame route of `zip(dict)` there: "zd_small_batch" = the duration of k_zd_small (and of zeroing its trie tables), with
 * launches = the frames that took the route; "zd_small_place" = the copy of the finished streams to their destinations, one launch per
 * chunk; "zd_small_handback": launches = the frames of those the kernel gave up (a match longer than 1024 bytes) and the worker contexts
 * coded; "zd_small_finished": launches = the walks the kernel's commit wave finished behind the speculating lanes' cap of 32 bytes.
 * The small-frame decode route of `zip(dict)` in cniic_codec_decode_batch and cniic_codec_measure_batch (described there):
 * "zd_small_dec_batch" = the duration of k_zd_small_dec, with launches = the frames it was given; "zd_small_dec_handback": launches = the
 * frames of those the kernel handed back (pairs behind its cap of 24 576, 64 or more generations, a byte behind more than 64 pairs)
 * and the worker contexts decoded.
 * The small-frame routes of Hilbert { compress: Zip } in cniic_hilbert_zip_encode_batch_var, cniic_hilbert_zip_decode_batch and
 * cniic_hilbert_zip_measure_batch (described there) report the same marks under their own names: "hz_small_batch" = the duration of
 * k_hz_small (and of zeroing its trie tables), with launches = the frames given to the kernel; "hz_small_place"; "hz_small_handback";
 * "hz_small_finished"; "hz_small_dec_batch" = the duration of k_hz_small_dec, with launches = the frames it was given;
 * "hz_small_dec_handback".  No call that takes an expression reports any of them.
 * The chain of a `zip(dict)` / hilbert-zip encode whose longest entry has more than 255 bytes ("zd_chain_plain", launches = 1 whichever way
 * it ran) adds three marks when it ran as the hybrid chain (k_zipdict.hip, zd_chain.hpp) and none when the one-block walk ran:
 * "zd_chain_hybrid" = the duration of its launches, launches = 1; "zd_chain_breaks" (no duration): launches = the break pieces, i.e. the
 * 256-position pieces behind the fill end that hold a match of more than 255 bytes; "zd_chain_entered" (no duration): launches = the break
 * pieces the parse enters.  Its stages, in order, each with launches = 1: "zd_hy_breaks" (flags and their numbering), "zd_hy_maps",
 * "zd_hy_scan", "zd_hy_table", "zd_hy_walk", "zd_hy_patch" (patch and second scan), "zd_hy_marks"; a text without a break piece has no
 * table, walk and patch.
 * The repaint of a single `voronoi` decode (and of the frames a batch call leaves to its workers) marks the kernel it took (launches
 * only, no duration): "vor_paint_tiles" = 1 when the tile-pruned kernel painted (1 <= K <= 4096, sides up to 16 384, every centroid
 * coordinate below 16 384), "vor_paint_brute" = 1 when the brute-force kernel did; "vor_paint_overflow": launches = the 64 x 32-pixel
 * tiles of the tiled kernel whose kept list outgrew its 256 entries and that were painted by brute force (it exists, with 0, whenever
 * the tiled kernel ran). */
int32_t     cniic_last_kernel_time(cniic_ctx *ctx, const char *which, double *ms, uint64_t *launches);

/* ------------------------------------------------------------------ H1: utils::count_freqs */
/* Symbol kinds fix the 32-bit key packing and the wire size of a symbol. */
#define CNIIC_SYM_RGB    1  /* Rgb<u8>: key = r<<16|g<<8|b; 11 bytes on the wire (src/ser.rs:210-214)   */
#define CNIIC_SYM_SIGNED 2  /* SignedColor([i16;3]) (src/codec/hilbertc.rs:513-516):                    */
                            /* key = (dr+255)<<18|(dg+255)<<9|(db+255); 6 bytes (src/ser.rs:188-195)    */

/* utils::count_freqs over the pixels of an image (src/utils.rs:4-16; call sites src/huf.rs:30,
 * src/codec/clusterc.rs:21).  Output: distinct colours as packed keys in ASCENDING key order and
 * their occurrence counts.  keys/counts may be NULL to query *n_unique only. */
int32_t cniic_hist_rgb24(cniic_ctx *ctx, const uint8_t *rgb, uint64_t npx,
                         uint32_t *keys, uint64_t *counts, uint64_t cap, uint64_t *n_unique);
/* count_freqs over a stream of packed symbol keys of the given kind. */
int32_t cniic_hist_syms(cniic_ctx *ctx, int32_t sym_kind, const uint32_t *syms, uint64_t n,
                        uint32_t *keys, uint64_t *counts, uint64_t cap, uint64_t *n_unique);

/* ------------------------------------------------------------------ K-means: kmeans::cluster */
typedef struct {
    uint64_t seed;       /* seeds the deterministic empty-cluster reseed (replaces thread_rng,   */
                         /* src/kmeans.rs:123-133); 0 = library default                            */
    uint64_t max_iters;  /* 0 = run until no point moves (the reference has no cap, kmeans.rs:26) */
    uint32_t flags;      /* CNIIC_KM_* */
    uint32_t reserved;
} cniic_kmeans_opts;
#define CNIIC_KM_BRUTE_FORCE 1u  /* disable bound-based pruning (debug / A-B measurement) */
#define CNIIC_KM_PROFILE     2u  /* HIP-event pair around every assign launch -> cniic_last_kernel_time("kmeans_rgbw_assign") */
#define CNIIC_KM_NO_SKIP     4u  /* never use the skip schedule of the pruned assign (A-B measurement) */

typedef struct {
    uint64_t iterations;     /* src/kmeans.rs:33 "#iterations"                         */
    uint64_t moved_last;     /* points that changed cluster in the last iteration      */
    uint64_t empty_reseeds;  /* src/kmeans.rs:117-134 occurrences                      */
    uint64_t active;         /* clusters with >= 1 member (src/kmeans.rs:49-52)        */
    uint64_t pair_evals;     /* point-centroid distance evaluations (mirrors the       */
                             /* "tested neighbours" counters of src/kmeans.rs:401-413) */
} cniic_kmeans_stats;

typedef struct {  /* ColorPos, src/codec/clusterc.rs:200-204 */
    uint32_t x, y;
    uint8_t  rgb[3];
    uint8_t  pad;
} cniic_colorpos;

/* kmeans::cluster::<ColorCount> (src/kmeans.rs:21-39 with src/codec/clusterc.rs:68-114):
 * U distinct colours (packed keys, any order; the order IS the point order of the reference's
 * Vec<ColorCount>) with pixel-count weights.  Out: K centroid colours (K x 3 bytes, r,g,b),
 * final cluster of every input colour (labels[U]), members[K] = colours per cluster. */
int32_t cniic_kmeans_rgbw(cniic_ctx *ctx, const uint32_t *keys, const uint32_t *weight, uint64_t U,
                          uint32_t K, const cniic_kmeans_opts *opts,
                          uint8_t *centroids, uint32_t *labels, uint64_t *members,
                          cniic_kmeans_stats *stats);
/* kmeans::cluster::<ColorPos> over all pixels of an image, row-major point order
 * (src/codec/clusterc.rs:150-153).  labels (N u32) and members may be NULL. */
int32_t cniic_kmeans_xyrgb(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h,
                           uint32_t K, const cniic_kmeans_opts *opts,
                           cniic_colorpos *centroids, uint32_t *labels, uint64_t *members,
                           cniic_kmeans_stats *stats);

/* ---- K-means from given centroids -- an extension, as shared and frozen palettes are: the reference always starts from init_centroids.
 *
 * THE DEFINITION.  It is kmeans::cluster (kmeans.rs:21-39) with only init_centroids (kmeans.rs:101-108) replaced by the caller's K
 * centroids.  Everything else is unchanged: init_assignment by position in the point list (kmeans.rs:61-78), so the first assign starts
 * from the chunk labels; a point stays unless another centroid is STRICTLY nearer; the lowest index among equal minima; the integer
 * means; the seeded empty-cluster reseed with its iteration number; max_iters, CNIIC_ERR_TOO_FEW_POINTS, CNIIC_ERR_FEW_ACTIVE.  Two
 * consequences:
 *   - A run started from its own reference init centroids (the first element of chunk k) is the ordinary run, bit for bit.
 *   - A run started from a converged palette need not stop after one iteration: the initial labels are the chunk labels, not the
 *     assignment the palette converged with, so colours equidistant from two centroids resolve differently (they stay with their chunk's
 *     cluster where they can), the means move, and a few more iterations follow.
 * init is always HOST memory: K x 3 bytes r, g, b for colours, K cniic_colorpos for voronoi (pad ignored).  Equal entries are legal.
 * cniic_kmeans_xyrgb_from: init[k].x >= w or init[k].y >= h returns CNIIC_ERR_BAD_ARG (the tiled kernel's 24-bit coordinate products stand
 * on coordinates inside the image); it takes the tiled route and the exact slow route (K > 4096, a side above 16384) as cniic_kmeans_xyrgb
 * does.  Everything else as the calls above. */
int32_t cniic_kmeans_rgbw_from(cniic_ctx *ctx, const uint32_t *keys, const uint32_t *weight, uint64_t U,
                               uint32_t K, const cniic_kmeans_opts *opts, const uint8_t *init,
                               uint8_t *centroids, uint32_t *labels, uint64_t *members,
                               cniic_kmeans_stats *stats);
int32_t cniic_kmeans_xyrgb_from(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h,
                                uint32_t K, const cniic_kmeans_opts *opts, const cniic_colorpos *init,
                                cniic_colorpos *centroids, uint32_t *labels, uint64_t *members,
                                cniic_kmeans_stats *stats);

/* One assign step from given centroids and labels (src/kmeans.rs:330-416 + the sums consumed by
 * Point::mean): labels updated in place; sums[K x D] (D = 3 / 5), wsum[K] (sum of weights, or
 * member count), members[K], *changed.  Centroids are not updated.  For parity tests and for
 * callers that own the reduction (multi-GPU). */
int32_t cniic_kmeans_step_rgbw(cniic_ctx *ctx, const uint32_t *keys, const uint32_t *weight,
                               uint64_t U, uint32_t K, const uint8_t *centroids, uint32_t *labels,
                               uint64_t *sums, uint64_t *wsum, uint64_t *members, uint64_t *changed);
int32_t cniic_kmeans_step_xyrgb(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h,
                                uint32_t K, const cniic_colorpos *centroids, uint32_t *labels,
                                uint64_t *sums, uint64_t *wsum, uint64_t *members, uint64_t *changed);

/* Sharded K-means session (pixels / colours sharded over GPUs, one process per GPU): the library
 * owns assign + partial sums + centroid update on its shard; the CALLER all-reduces the partials
 * buffer (RCCL sum over int64 words) between cniic_km_assign and cniic_km_update.
 * All ranks pass the full point list (U colours); rank r of n passes shard = r, nshards = n and
 * works on its share of the colour-space cells. */
typedef struct cniic_km cniic_km;
int32_t cniic_km_create_rgbw(cniic_ctx *ctx, const uint32_t *keys, const uint32_t *weight, uint64_t U,
                             uint32_t shard, uint32_t nshards, uint32_t K, const cniic_kmeans_opts *opts,
                             void *partials_dev /* device buffer of cniic_km_partial_words(K,3) u64, or NULL */,
                             cniic_km **out);
uint64_t cniic_km_partial_words(uint32_t K, uint32_t D);   /* K*D sums + K wsum + K members + moved + evals */
int32_t cniic_km_partials(cniic_km *km, void **dev_ptr);
/* After create the partials buffer holds this shard's sums of the INITIAL assignment
 * (kmeans.rs:61-78); all-reduce it, then call cniic_km_begin once. */
int32_t cniic_km_begin(cniic_km *km);
/* Each iteration: cniic_km_assign (async; partials <- signed deltas of the points that moved),
 * all-reduce the partials, cniic_km_update. */
int32_t cniic_km_assign(cniic_km *km);                      /* async on the ctx stream */
int32_t cniic_km_update(cniic_km *km, uint64_t *changed);   /* syncs; *changed = global moved count */
/* The labels live on the device in the library's internal (cell-major) point order, all U of
 * them, of which this shard owns [lo,hi): all-gather that range before asking for the result. */
int32_t cniic_km_labels_internal(cniic_km *km, void **dev_ptr, uint64_t *elem_bytes);
/* labels: all U points, the caller's (canonical) order. */
int32_t cniic_km_result(cniic_km *km, uint8_t *centroids, uint32_t *labels, uint64_t *members,
                        cniic_kmeans_stats *stats);
/* average duration (ms) of the assign kernel alone over `reps` back-to-back launches, measured
 * with HIP events on the ctx stream (bench.py's roofline figure) */
int32_t cniic_km_time_assign(cniic_km *km, int32_t reps, double *ms_per_launch);
void    cniic_km_destroy(cniic_km *km);

/* ------------------------------------------------------------------ cluster-colors over several GPUs */
/* One process per GPU, every rank holds its own image(s); the ranks build ONE palette for the
 * union of their pixels (north_star config 4) and each encodes its own image with it.  The caller
 * owns the collectives (RCCL through torch.distributed, or ncclAllReduce directly):
 *
 *   cniic_hist_rgb24_dense(img)            -> local  u32[2^24] colour counts (device)
 *   all-reduce(sum) a COPY of it           -> global counts
 *   cniic_cc_create(global, K, rank, n)    -> distinct colours, K-means state; the global table
 *                                             is overwritten (key -> rank + 1)
 *   repeat: cniic_cc_assign; all-reduce(sum) the partials buffer (int64 words); cniic_cc_update
 *           until *changed == 0  (or update asynchronously and cniic_cc_poll every few iterations)
 *   cniic_cc_export_labels; all-reduce(sum) that buffer; cniic_cc_import_labels
 *   cniic_cc_finish(img, local counts)     -> this rank's Hufman stream (clusterc.rs:31-52)
 *
 * Integer sums make the palette bit-identical for any number of ranks. */
typedef struct cniic_cc cniic_cc;
int32_t  cniic_hist_rgb24_dense(cniic_ctx *ctx, const uint8_t *rgb, uint64_t npx, uint32_t *table_dev);
int32_t  cniic_cc_create(cniic_ctx *ctx, uint32_t *table_dev, uint32_t K, const cniic_kmeans_opts *opts,
                         uint32_t shard, uint32_t nshards,
                         void *partials_dev /* device, cniic_km_partial_words(K,3) u64, or NULL */, cniic_cc **out);
uint64_t cniic_cc_unique(cniic_cc *cc);        /* distinct colours U */
uint32_t cniic_cc_label_bytes(cniic_cc *cc);   /* 1 (K <= 256) or 2: element size of the label buffers */
int32_t  cniic_cc_partials(cniic_cc *cc, void **dev_ptr);
/* The session's K-means started from the caller's centroids ("K-means from given centroids" above; init: host, K x 3 bytes).  Valid on any
 * session that has its K-means state, however it was made (cniic_cc_create, cniic_cc_create_local, cniic_cc_image_create; any shard count:
 * every rank must pass the same bytes), and only before the session's first cniic_cc_assign / cniic_cc_run: afterwards it returns
 * CNIIC_ERR_BAD_ARG and the session stays as it was.  The loop, cniic_cc_finish* and cniic_cc_palette follow unchanged. */
int32_t  cniic_cc_set_centroids(cniic_cc *cc, const uint8_t *init);
int32_t  cniic_cc_assign(cniic_cc *cc);                        /* async on the ctx stream */
int32_t  cniic_cc_update(cniic_cc *cc, uint64_t *changed);     /* syncs; changed == NULL: asynchronous */
/* iterations completed so far and whether an iteration has moved nothing (syncs).  Iterations issued
 * after convergence are no-ops on the device, so callers may poll only every few iterations. */
int32_t  cniic_cc_poll(cniic_cc *cc, uint64_t *iterations, uint32_t *done);
/* The same without a GPU stall: returns the state as of the PREVIOUS call (*valid = 0 on the first call) and
 * enqueues the copy the next call will read.  Call it after every batch of iterations; every rank sees the
 * same sequence of answers, so all ranks stop after the same batch. */
int32_t  cniic_cc_poll_lagged(cniic_cc *cc, uint64_t *iterations, uint32_t *done, uint32_t *valid);
int32_t  cniic_cc_export_labels(cniic_cc *cc, void *dst_dev);  /* U labels, zero outside this shard */
int32_t  cniic_cc_import_labels(cniic_cc *cc, const void *src_dev);
int32_t  cniic_cc_finish(cniic_cc *cc, const uint8_t *rgb, uint32_t w, uint32_t h,
                         const uint32_t *local_table_dev /* this image's own counts, or NULL = single image */,
                         uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats);
/* A BATCH of equally sized frames, contiguous in memory, coded with the session's one palette (north_star: "pixels of an image
 * batch shard across the GPUs ... all-reduce of the K partial centroid sums"; the harness's many-images loop, bench.rs:24-35,
 * with a shared palette -- an extension, the reference has one palette per image).  Open the session on ALL the pixels
 * (cniic_cc_image_begin(frames, F * w * h), or the dense-table calls), run the loop, then this instead of cniic_cc_finish:
 * frame f's Hufman stream (clusterc.rs:31-52 applied to frame f: dims, its own tree, its payload) is written at
 * out + f * stride (stride: a multiple of 4, at least the longest stream rounded up to 4) and its length to lens[f]. */
int32_t  cniic_cc_finish_frames(cniic_cc *cc, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t frames,
                                uint8_t *out, uint64_t stride, uint64_t *lens, cniic_kmeans_stats *stats);
/* The same for frames of DIFFERENT sizes -- a folder, a sprite sheet, the tiles of a large image with ragged edge tiles -- under the
 * session's one palette (the harness's many-images loop, bench.rs:24-35, is run on such a folder; padding the frames instead would
 * change the histogram and so the palette).  Frame f is w[f] x h[f]; the frames lie back to back in rgb, in order: the contiguous
 * pixels the session was opened on (cniic_cc_image_begin(rgb, sum of w[f] h[f]), or the dense-table calls).  w, h and lens are host
 * arrays of `frames` entries; rgb and out may be host or device memory, as above.  Stream f is ClusterColors::encode
 * (clusterc.rs:31-52) applied to frame f with the session's palette -- the frame's own dimensions, its own tree over the clusters it
 * uses, its payload -- written at out + f * stride (stride: a multiple of 4), its length to lens[f]: the layout
 * cniic_codec_decode_batch reads.  Any number of frames (no 65 535 cap).
 * CNIIC_ERR_BAD_ARG: a null argument or frames == 0; any w[f] * h[f] == 0; stride & 3; the sum of w[f] h[f] different from the pixels
 * the session was opened on (cniic_last_error names both numbers).  A dense-table session knows its pixels when the table held its own
 * image's counts (cniic_cc_create_local, or cniic_cc_create with one shard); one made by cniic_cc_create from the all-reduced table of
 * several shards holds the union's counts only and, like cniic_cc_finish_frames, cannot check the total.  A stream that does not fit the stride:
 * CNIIC_ERR_CAPACITY as from cniic_cc_finish_frames, the lengths needed in lens, nothing packed. */
int32_t  cniic_cc_finish_frames_var(cniic_cc *cc, const uint8_t *rgb, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                    uint8_t *out, uint64_t stride, uint64_t *lens, cniic_kmeans_stats *stats);
void     cniic_cc_destroy(cniic_cc *cc);

/* ---- Frozen palettes: code further frames with a palette that already exists -- a video whose frames keep arriving, new tiles of the
 * same map, a folder whose palette was built on a sample, two ranks that agree on a palette by sending K x 3 bytes.
 *
 * THE RULE.  A pixel's label is the index k that minimises (r - R_k)^2 + (g - G_k)^2 + (b - B_k)^2 in integers; among equal minima it is
 * the lowest k.  This is Rgb<u8>::dist (geom.rs:8-24) compared as squared integers, with first-minimum ties.  Nothing else is defined:
 * there is no "stay" rule, because there is no previous assignment.  Two consequences:
 *   - For the frames a converged session was run on, this is the assignment the K-means ended with, except where a colour is equidistant
 *     from two entries: there the K-means keeps the older cluster and this rule takes the lower index.  So the streams can differ from
 *     cniic_cc_finish_frames_var's only at such ties.
 *   - The error can never be larger than the session's: every pixel gets a nearest entry.
 * Equal palette entries are legal; the lowest index wins.  The stream's alphabet is colours, as in clusterc.rs:31-52: two entries of
 * one colour are one symbol.  The streams are ordinary cluster-colors(K) streams, which cniic_codec_decode and cniic_codec_decode_batch
 * read.
 *
 * cniic_cc_palette (stands in for cniic_km_result, which a cniic_cc does not have): the session's centroids as of its last update into
 * centroids (host memory, K x 3 bytes: r, g, b) and, when pixels is not NULL, the pixels per cluster the session knows (its wsum; host
 * array of K entries).  Before the loop has finished it returns what the session's results are at that moment.  The session stays
 * usable for a later cniic_cc_finish*. */
int32_t  cniic_cc_palette(cniic_cc *cc, uint8_t *centroids, uint64_t *pixels);
/* A handle on K entries (centroids: host or device memory, K x 3 bytes; K from 1 to 65 536) and on the label of every one of the 2^24
 * colours under the rule: u8 for K <= 256, u16 above, built once here (k_palette.hip).  It belongs to its context and stream, like a
 * session; one handle is used from one thread at a time, for any number of calls.  CNIIC_ERR_BAD_ARG: K == 0, K > 65 536, a null
 * pointer.  With the stage timers on: "pal_lut" = the table kernel, "pal_lut_plain" (launches only) = the cells of the colour cube whose
 * candidate list was too long for LDS and which scanned all K entries instead. */
typedef struct cniic_palette cniic_palette;
int32_t  cniic_palette_create(cniic_ctx *ctx, const uint8_t *centroids, uint32_t K, cniic_palette **out);
void     cniic_palette_destroy(cniic_palette *pal);
uint32_t cniic_palette_label_bytes(cniic_palette *pal);   /* 1 (K <= 256) or 2: element size of the labels */
/* The index image (what remap's lookup stands on, clusterc.rs:43-47): labels receives npx entries of cniic_palette_label_bytes(pal)
 * bytes, host or device memory; rgb likewise.  Stage timer: "pal_labels". */
int32_t  cniic_palette_labels(cniic_palette *pal, const uint8_t *rgb, uint64_t npx, void *labels);
/* cniic_cc_finish_frames_var without a session: frame f is w[f] x h[f], the frames back to back in rgb, stream f (ClusterColors::encode,
 * clusterc.rs:31-52, applied to frame f with the handle's palette under the rule above) at out + f * stride, its length in lens[f].
 * Layout, the stride rule (a multiple of 4) and CNIIC_ERR_CAPACITY (the lengths needed in lens, nothing packed, out untouched) are those of
 * cniic_cc_finish_frames_var; so are the CNIIC_ERR_BAD_ARG cases -- a null argument or frames == 0, any w[f] * h[f] == 0, stride & 3 --
 * without the pixel total, which there is no session to hold against.  frames == 1 is the single image.  There is no active-cluster
 * check: that belongs to a K-means (kmeans.rs:41-57), not to a palette.  rgb and out may be host or device memory and are staged as
 * cniic_cc_finish_frames_var stages them.  Stage timers: "pal_labels", then the frames_var_* names of that call. */
int32_t  cniic_palette_encode_frames_var(cniic_palette *pal, const uint8_t *rgb, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                         uint8_t *out, uint64_t stride, uint64_t *lens);

/* How well the handle's palette fits a batch of frames, without coding them: frames back to back in rgb (host or device memory) as for
 * cniic_palette_encode_frames_var.  sse[f] (host, u64[frames]) = the exact integer sum over frame f's pixels of the squared distance to the
 * pixel's entry under THE RULE: 3 w[f] h[f] times the MSE of decoding that frame's cniic_palette_encode_frames_var stream.  pixels (host,
 * u64[K], may be NULL) = the pixels of all frames per entry; an entry shadowed by an equal one of lower index gets 0.  One kernel launch
 * whatever the number of frames, no label buffer.  CNIIC_ERR_BAD_ARG: a null argument or frames == 0, any w[f] * h[f] == 0.
 * Stage timer: "pal_fit". */
int32_t  cniic_palette_fit_frames_var(cniic_palette *pal, const uint8_t *rgb, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                      uint64_t *sse, uint64_t *pixels);

/* The same shared palette with every rank holding ONLY ITS OWN image's colours (per-rank work and memory do not
 * grow with the number of ranks, no label exchange).  The reference's point list -- the ascending list of the
 * distinct colours of all the pixels -- is then known to every rank as a bitmap:
 *   cniic_hist_rgb24_dense(img)         -> this image's counts, u32[2^24]
 *   cniic_occupancy_pack(counts, occ)   -> one nibble per colour (u32[2^21]), 1 where the colour occurs
 *   all-reduce(sum) occ                 -> non-zero where ANY rank has the colour (<= 15 ranks: nibbles cannot carry)
 *   cniic_cc_create_local(counts, occ)  -> this rank's points, initialised by their position in the list of all
 *                                          occupied colours (init_assignment / init_centroids, kmeans.rs:61-108; the
 *                                          empty-cluster reseed picks from the same list); counts is overwritten
 *   the loop as above (cniic_cc_run, or assign / all-reduce / update); then cniic_cc_finish(img, NULL)
 * A colour that occurs on several ranks is several points with one position: every copy takes the same decisions and
 * the integer sums are those of the single merged point, so centroids, iteration count and palette are bit-identical to
 * clustering the union (only the moved / member COUNTS, used for their zero-ness alone, see each copy). */
int32_t  cniic_occupancy_pack(cniic_ctx *ctx, const uint32_t *table_dev, uint32_t *occ_dev);
int32_t  cniic_cc_create_local(cniic_ctx *ctx, uint32_t *table_dev, const uint32_t *occ_dev, uint32_t K, const cniic_kmeans_opts *opts,
                               void *partials_dev /* u64[5K+2] the caller all-reduces, or NULL with cniic_cc_run */, cniic_cc **out);
/* The same without the dense table, for large images (16-byte aligned device image): the pixels are partitioned by colour
 * super-cell once (what ClusterColors::encode of a single image does here above 2^20 pixels), which gives this image's
 * colours, their occupancy and, after the K-means, every pixel's label without a random read.
 *   cniic_cc_image_begin(img)           -> session holding the partition (no K-means state yet)
 *   cniic_cc_image_occupancy(cc, occ)   -> the nibbles of this image's colours, u32[2^21]; all-reduce(sum) as above
 *   cniic_cc_image_create(cc, occ, K)   -> the K-means state, as cniic_cc_create_local
 *   the loop, then cniic_cc_finish(cc, img, NULL) with the same image */
int32_t  cniic_cc_image_begin(cniic_ctx *ctx, const uint8_t *rgb_dev, uint64_t npx, cniic_cc **out);
int32_t  cniic_cc_image_occupancy(cniic_cc *cc, uint32_t *occ_dev);
int32_t  cniic_cc_image_create(cniic_cc *cc, const uint32_t *occ_dev, uint32_t K, const cniic_kmeans_opts *opts,
                               void *partials_dev /* as cniic_cc_create_local */);

/* ---- RCCL on the context's own stream (ncclAllReduce of the K partial sums between assign and
 * update, no host round trip).  librccl is bound at run time; without it these return CNIIC_ERR_UNSUPPORTED
 * and the caller all-reduces the buffers itself (cniic_cc_assign / cniic_cc_update above).
 *   rank 0: cniic_comm_unique_id -> broadcast the 128 bytes by any means -> every rank: cniic_comm_create
 *   cniic_comm_all_reduce : in-place unsigned sum of a device buffer (elements of 1, 4 or 8 bytes)
 *   cniic_cc_run          : the whole `while changed_assignment` loop (kmeans.rs:26-32) of a cc session, with
 *                           the all-reduce in-stream when comm != NULL; identical on every rank */
typedef struct cniic_comm cniic_comm;
int32_t  cniic_comm_unique_id(uint8_t id[128]);
int32_t  cniic_comm_create(cniic_ctx *ctx, const uint8_t id[128], uint32_t rank, uint32_t nranks, cniic_comm **out);
void     cniic_comm_destroy(cniic_comm *comm);
int32_t  cniic_comm_all_reduce(cniic_comm *comm, void *buf_dev, uint64_t count, int32_t elem_bytes);
/* The same communicator over the caller's own transport (MPI, sockets, gloo ...) where RCCL is not wanted: every
 * all-reduce drains the stream, hands `count` elements of `elem_bytes` bytes to fn in HOST memory and expects the
 * in-place unsigned sum over all ranks there when fn returns 0.  Slower (a host round trip per iteration), same
 * results; cniic_cc_run / cniic_comm_all_reduce take it like the RCCL one.
 * Failures: a rank that fails inside cniic_cc_run (a launch error, a failed collective) aborts its communicator before
 * it returns, so that its peers leave their next all-reduce with CNIIC_ERR_RCCL instead of waiting for it for ever --
 * RCCL: ncclCommAbort here, ncclCommGetAsyncError polled by the peers while they wait for a batch; host transport: fn is
 * called once with (buf_host = NULL, count = 0, elem_bytes = -1) and should tear the caller's transport down (a peer
 * whose fn then fails returns non-zero, which ends that peer's loop the same way).  The communicator is unusable
 * afterwards (every call returns CNIIC_ERR_RCCL): destroy it.
 * A peer that dies WITHOUT aborting (killed process, lost node) is not always reported by RCCL's asynchronous error state
 * (intra-node P2P / SHM transports), so the wait for a batch of launches that contains collectives has a deadline of its own:
 * cniic_comm_set_timeout (default 120 000 ms, or CNIIC_COLLECTIVE_TIMEOUT_MS at creation; 0 = wait for ever).  When it expires
 * cniic_cc_run aborts the communicator and returns CNIIC_ERR_RCCL.  With a host transport every all-reduce is a blocking call
 * of fn: there the transport's own timeout bounds the wait (gloo: the process group's `timeout`). */
typedef int32_t (*cniic_host_sum_fn)(void *user, void *buf_host, uint64_t count, int32_t elem_bytes);
int32_t  cniic_comm_create_host(cniic_ctx *ctx, uint32_t rank, uint32_t nranks, cniic_host_sum_fn fn, void *user, cniic_comm **out);
int32_t  cniic_comm_set_timeout(cniic_comm *comm, uint64_t milliseconds);
/* The same communicator as a ONE-SHOT exchange over mailboxes (k_mailbox.hip), for buffers where RCCL's ring is all latency
 * (the K partial sums: 10 KiB an iteration): every rank owns a mailbox in fine-grained HBM that its peers map through HIP
 * IPC; an all-reduce is one kernel per rank that writes the buffer into a slot of EVERY peer's mailbox over the direct xGMI
 * links, raises a flag behind it, waits for the flags of its own mailbox and adds the slots in rank order (unsigned integer
 * sums: bit-identical to RCCL's result).  At most 16 ranks; buffers larger than max_bytes (0: 1 MiB) go in pieces.
 *   every rank: cniic_comm_create_mailbox -> all-gather the 64-byte handles by any means, in rank order ->
 *   every rank: cniic_comm_connect_mailbox -> cniic_comm_all_reduce / cniic_cc_run / cniic_comm_set_timeout as above
 * (one process per GPU; ranks inside one process find each other's mailboxes without IPC, and need streams that do not share a
 * hardware queue -- a process has four -- since each rank's kernel waits for the kernels of the others).  A wait is bounded INSIDE the
 * kernel by the communicator's timeout (0 or more than 600 000 ms: 600 000 ms), an abort by a peer ends it at once; both
 * surface as CNIIC_ERR_RCCL from cniic_cc_run or the next cniic_comm_all_reduce.  RCCL stays the default transport: this one
 * has only been run between processes that share ONE GPU (tests/test_mailbox.py), not yet across xGMI. */
#define CNIIC_MAILBOX_HANDLE_BYTES 64
int32_t  cniic_comm_create_mailbox(cniic_ctx *ctx, uint32_t rank, uint32_t nranks, uint64_t max_bytes,
                                   uint8_t handle[CNIIC_MAILBOX_HANDLE_BYTES], cniic_comm **out);
int32_t  cniic_comm_connect_mailbox(cniic_comm *comm, const uint8_t *handles /* nranks x 64 bytes, rank order */);
int32_t  cniic_cc_run(cniic_cc *cc, cniic_comm *comm /* NULL: one rank */, cniic_kmeans_stats *stats);

/* ------------------------------------------------------------------ cluster-colors remap */
/* src/codec/clusterc.rs:31-47: every pixel's colour -> the centroid colour of its cluster.
 * keys[U] ascending (as returned by cniic_hist_rgb24), labels[U], centroids[K x 3]. */
int32_t cniic_remap_rgb(cniic_ctx *ctx, const uint8_t *rgb, uint64_t npx, const uint32_t *keys,
                        const uint32_t *labels, uint64_t U, const uint8_t *centroids, uint32_t K,
                        uint8_t *out_rgb);

/* ------------------------------------------------------------------ Hilbert scan + delta */
/* hilbert::iter(w,h) (src/hilbert.rs:40-43): xy[2*d], xy[2*d+1] for d in 0..w*h.
 * The scan is the one frozen by this build (see DESIGN.md "Hilbert scan: parity unpinned"). */
int32_t cniic_hilbert_xy(cniic_ctx *ctx, uint32_t w, uint32_t h, uint32_t *xy);
/* The reference's scan is the un-vendored crate zhang_hilbert 0.1.1 (src/hilbert.rs:40-43, Cargo.toml:15), which this build
 * cannot reproduce (parity unpinned).  A host that HAS the crate injects its order: xy = w * h pairs (x, y), entry d =
 * where ArbHilbertScan32::new([w, h]) is at step d (host or device memory).  From then on every scan-dependent path of this
 * context -- cniic_hilbert_*, `delta`, `hilbert(rle)`, encode and decode -- follows that order for images of exactly w x h
 * (per-position kernels instead of the tile kernels of the built-in 2^n scan), and its streams are the reference's.  The order
 * must visit every pixel exactly once (CNIIC_ERR_BAD_ARG otherwise).  xy == NULL: back to the built-in scan. */
int32_t cniic_ctx_set_scan(cniic_ctx *ctx, uint32_t w, uint32_t h, const uint32_t *xy);
/* hilbert::linearize (src/hilbert.rs:10-12): pixels gathered in scan order. */
int32_t cniic_hilbert_linearize(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out_rgb);
/* The three linearisations `--special=hilbert` writes out (src/main.rs:23-55), by method:
 *   CNIIC_LIN_RECT  (src/hilbert.rs:10-12)  out[d] = img(scan of w x h at d): w h pixels, cniic_hilbert_linearize's byte for byte
 *   CNIIC_LIN_SMALL (src/hilbert.rs:15-22)  s = min(npot(w) >> 1, npot(h) >> 1), npot = u32::next_power_of_two: the scan of s x s over the
 *                   top-left s x s pixels, s^2 pixels.  For w an exact power of two that is w / 2, not w (4 x 4 gives its 2 x 2 corner,
 *                   a 1-wide image nothing: 0 pixels and CNIIC_OK) -- the reference's arithmetic, kept.
 *   CNIIC_LIN_LARGE (src/hilbert.rs:25-32)  S = max(npot(w), npot(h)): the scan of S x S, only the positions with x < w && y < h kept, in
 *                   their order: w h pixels.  The S^2 positions are not walked (a pixel's rank is computed from the curve's levels), unless
 *                   the context holds an injected scan for exactly S x S, whose order is then followed position by position.
 * "The scan of a x b" is what cniic_hilbert_xy answers on this context (an injected scan for exactly a x b included).
 * Limits as everywhere here: w, h < 2^30 and w h < 2^32. */
#define CNIIC_LIN_RECT  0
#define CNIIC_LIN_SMALL 1
#define CNIIC_LIN_LARGE 2
/* host only, no context: pixels the method yields; CNIIC_ERR_BAD_ARG for an unknown method or dimensions beyond the limits */
int32_t cniic_hilbert_linearize_count(int32_t method, uint32_t w, uint32_t h, uint64_t *npx);
/* rgb, out_rgb: host or device memory; *npx = pixels written.  cap_px < needed: CNIIC_ERR_CAPACITY with *npx = needed and nothing written.
 * Stage timers: lin_small, lin_large (launches: 1 on the computed route, 3 along an injected S x S scan). */
int32_t cniic_hilbert_linearize_as(cniic_ctx *ctx, int32_t method, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out_rgb, uint64_t cap_px,
                                   uint64_t *npx);
/* scripts/experiments/hilbert_distribution.py: for a linear RGB stream of npx pixels, counts[c][v + 255] = number of i in 1 .. npx-1 with
 * lin[i][c] - lin[i-1][c] == v, c = r, g, b; counts: u64[3][511], host or device.  npx <= 1: all zero; a channel's counts sum to npx - 1
 * (pandas.diff drops the first element: no START zero, unlike the DiffStream below).  Stage timer: chan_diff_hist. */
int32_t cniic_channel_diff_hist(cniic_ctx *ctx, const uint8_t *lin_rgb, uint64_t npx, uint64_t *counts);
/* DiffStream over the Hilbert-ordered pixels (src/codec/hilbertc.rs:449-477): N packed
 * CNIIC_SYM_SIGNED keys. */
int32_t cniic_hilbert_delta(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h, uint32_t *syms);
/* Fused gather + delta + count_freqs (the first pass of huf::encode_all inside Delta::encode,
 * src/codec/hilbertc.rs:405-415 -> src/huf.rs:30).  syms may be NULL. */
int32_t cniic_hilbert_delta_hist(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h,
                                 uint32_t *keys, uint64_t *counts, uint64_t cap, uint64_t *n_unique,
                                 uint32_t *syms);

/* ------------------------------------------------------------------ H2: huf::encode_all */
/* src/huf.rs:22-43: histogram -> tree -> serialised decoder -> MSB-first bit-packed payload.
 * Returns CNIIC_ERR_CAPACITY with *len = needed bytes when cap is too small. */
int32_t cniic_huf_encode_all(cniic_ctx *ctx, int32_t sym_kind, const uint32_t *syms, uint64_t n,
                             uint8_t *out, uint64_t cap, uint64_t *len);
/* size of that stream as a pure function of the histogram. */
int32_t cniic_huf_size(int32_t sym_kind, const uint64_t *counts, uint64_t n, uint64_t *nbytes);

/* ------------------------------------------------------------------ Codec trait (src/codec.rs:14-19) */
/* expr is the reference's --codec= expression: "hufman", "cluster-colors(256)" / "ccol(256)",
 * "voronoi(2048)", "delta", "hilbert(rle)" = "hilbert(rle(0))", "hilbert(rle(4))" (src/codec.rs:41-59, FromStr impls of each
 * codec; hilbertc.rs:341-397 for the last two: rle(<f64>) takes what Rust's f64::from_str takes -- "4", "+4", "4.", ".5", "1e-3",
 * "inf", "-infinity", "nan" -- and its name() is "hilbert-rle" for d == 0, else "hilbert-rle-approx_" + d as Rust's Display prints
 * it, which can be longer than 300 characters), "zip(dict)" (zipc.rs:62-80: exactly that; name() "zip-dict", lossless; zip(back) and
 * hilbert(zip) are built, but are not expressions here and every entry point that takes an expression rejects them: they have entry points
 * of their own, single and batched -- cniic_zip_back_image_encode, cniic_hilbert_zip_encode and their kin below).  Every entry point below
 * that takes an expression takes all of the expressions listed.  The dimensions of a zip(dict) stream are inside its compressed text: cniic_zip_dict_dims.
 * cniic_codec_parse describes a codec as (kind, u32 argument), which cannot carry the f64: it answers CNIIC_ERR_BAD_ARG for
 * hilbert(rle(d)) with d != 0.  cniic_codec_parse_f64 takes every expression; darg is d (0 for d == 0.0 and -0.0, for `hilbert(rle)`
 * and for the other codecs).  Any out-parameter may be NULL. */
int32_t cniic_codec_parse(const char *expr, int32_t *kind, uint32_t *arg);
int32_t cniic_codec_parse_f64(const char *expr, int32_t *kind, uint32_t *arg, double *darg);
int32_t cniic_codec_name(const char *expr, char *buf, uint64_t cap);   /* Codec::name()        */
int32_t cniic_codec_is_lossless(const char *expr);                     /* 1 / 0 / negative err */
/* Codec::encode: appends nothing, writes the whole stream to out[0..*len). */
int32_t cniic_codec_encode(cniic_ctx *ctx, const char *expr, const uint8_t *rgb, uint32_t w, uint32_t h,
                           uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats);
/* same, with explicit K-means options (seed, iteration cap) */
int32_t cniic_codec_encode_opts(cniic_ctx *ctx, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb,
                                uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len,
                                cniic_kmeans_stats *stats);
/* cniic_codec_encode_opts for cluster-colors(K) and voronoi(K) with the K-means started from init ("K-means from given centroids" above:
 * host memory, K x 3 bytes for cluster-colors, K cniic_colorpos for voronoi).  centroids_out (host, may be NULL) receives the final K
 * centroids in init's layout after a successful encode: what the caller passes as init for the next frame of a video.  The streams are
 * ordinary streams of those codecs; CNIIC_ERR_CAPACITY with *len = bytes needed as the cold call.  Any other expression: CNIIC_ERR_BAD_ARG. */
int32_t cniic_codec_encode_warm(cniic_ctx *ctx, const char *expr, const cniic_kmeans_opts *opts, const void *init, const uint8_t *rgb,
                                uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len, void *centroids_out,
                                cniic_kmeans_stats *stats);
/* The harness's many-images loop (src/bench.rs:24-35: `paths.into_par_iter()`, one Codec::encode per rayon worker) as ONE call, for
 * EQUALLY SIZED images (cniic_codec_encode_batch_var below takes a folder of any sizes):
 * `frames` images of w x h, contiguous in memory (image f at rgb + f * w * h * 3), each encoded on its own exactly as
 * cniic_codec_encode would -- its own histogram, its own palette, its own stream (byte for byte; tests) -- written at
 * out + f * stride with its length in lens[f].  The images are dealt to CNIIC_OPT_BATCH_STREAMS worker contexts of this context
 * (own HIP streams, own scratch; created on first use, destroyed with the context), so that the dependent launches of one
 * image's K-means fill the gaps between another's.  rcs (may be NULL): per-image status; the call returns the first failure.
 * stats (may be NULL): `frames` entries. */
int32_t cniic_codec_encode_batch(cniic_ctx *ctx, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, uint32_t w, uint32_t h,
                                 uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens, int32_t *rcs, cniic_kmeans_stats *stats);
/* The same loop (src/bench.rs:24-35) over images of DIFFERENT sizes, which is what the folder the harness was written for holds (DIV2K's
 * validation set, reference Makefile:14-18): image f is w[f] x h[f] and starts at rgb + img_off[f] (bytes; any alignment; rgb is host or
 * device memory; the images may not overlap the output).  img_off, w, h, lens, rcs and stats are HOST arrays of `frames` entries.  Stream
 * f is written at out + f * stride (any stride, like cniic_codec_decode_batch, which reads exactly this layout) and its length to
 * lens[f]; stream, rcs[f] and stats[f] are byte for byte what cniic_codec_encode_opts gives for image f alone, whatever img_off[f] is.
 * A stream longer than stride: rcs[f] = CNIIC_ERR_CAPACITY, lens[f] = bytes needed, the other frames are unaffected.  w[f] * h[f] >=
 * 2^32: rcs[f] = CNIIC_ERR_BAD_ARG, as the single call.  The frames are dealt to the worker contexts of cniic_codec_encode_batch
 * (CNIIC_OPT_BATCH_STREAMS, the same K-means grid shares) from one queue, largest first; a device image that does not start on a
 * 16-byte boundary is copied into aligned worker scratch first, so that it takes the routes it takes alone at an aligned address
 * (the pixel partition of cluster-colors, the tile reads of `delta`).  With CNIIC_OPT_STAGE_TIMERS on, cniic_last_kernel_time answers
 * with the SUMS over all frames, and knows two more names (launches only, no duration): "cc_pixel_partition" = cluster-colors encodes
 * that took the pixel partition, "batch_stage" = frames that were copied to aligned scratch.  rcs / stats may be NULL; the call returns
 * the first failure (lowest f) with that frame's message in cniic_last_error; frames == 0 returns CNIIC_OK.
 *
 * SMALL cluster-colors frames take a route of their own, here and in cniic_codec_measure_batch: with the expression cluster-colors(K),
 * 1 <= K <= 256, DEVICE images and opts NULL or opts->flags == 0 (seed and max_iters are honoured), every frame of 1 .. 16384 pixels is
 * coded on ONE workgroup (its distinct colours, their counts and labels and the K centroids in the CU's LDS: sort, exact brute-force
 * Lloyd, every pixel's label), all such frames of the call in one set of launches whatever their number, each with its own palette as
 * the reference has it.  Larger frames, host images, any CNIIC_KM_* flag, K = 0 or K > 256 and every other codec go to the worker
 * contexts as above; cniic_codec_encode_batch (equal sizes) does not take the route.  Which route a frame took shows in no output
 * byte, status or message.  Stage timers: "cc_small_batch" = the duration of that kernel, with launches = the frames that took the route;
 * "cc_small_place" = the copy of the finished streams to out + f * stride; the tail between them keeps the names "frames_var_hist",
 * "frames_var_trees" and "frames_var_pack".  stats[f].pair_evals counts what the route that ran evaluated -- on this route
 * iterations x distinct colours x K, on the workers what their pruned search evaluated; the other four fields do not depend on the route.
 *
 * SMALL `delta` frames likewise, here and in cniic_codec_measure_batch: with the expression `delta`, DEVICE images and CNIIC_OPT_DELTA_ROUTE
 * not 32, every frame of 1 .. 16384 pixels whose size has no injected scan (cniic_ctx_set_scan) is coded on ONE workgroup from its pixels
 * to its finished stream (symbols along the scan, sort, the Huffman tree, header and payload; no host round trip), all such frames of the
 * call in one launch whatever their number.  Larger frames, host images, a frame of exactly the injected scan's size and a forced 32-bit
 * route go to the worker contexts as above; cniic_codec_encode_batch (equal sizes) does not take the route.  Which route a frame took
 * shows in no output byte, status or message; stats[f] stays zero as the single call leaves it.  Stage timers: "delta_small_batch" = the
 * duration of that kernel, with launches = the frames that took the route; "delta_small_place" = the copy of the finished streams to
 * out + f * stride.
 *
 * SMALL `hufman` frames likewise, here and in cniic_codec_measure_batch: with the expression `hufman`, DEVICE images and opts NULL or
 * opts->flags == 0, every frame of 1 .. 16384 pixels is coded on ONE workgroup from its pixels to its finished stream by the `delta`
 * route's kernel body over the pixels' own colours (row-major order, key r << 16 | g << 8 | b: no scan; sort, the Huffman tree, the
 * header of 12-byte leaves and the payload; no dense table and no host round trip), all such frames of the call in one launch per
 * 2 GiB of scratch whatever their number.  Larger frames and host images go to the worker contexts as above, and so does a LARGE frame
 * in a call of FEW (measured: one CU is slower for it than the workers' whole chip): with fewer than 4 frames of 1 .. 16384 pixels in the
 * call, only those of at most 4096 pixels take the route.  cniic_codec_encode_batch (equal sizes) does not take the route.  Which route a frame took shows in no output byte, status or message (CNIIC_ERR_CAPACITY with
 * lens[f] = bytes needed and the frame's room untouched, as the single call); stats[f] stays zero.  Stage timers: "huf_small_batch" = the
 * duration of that kernel, with launches = the frames that took the route; "huf_small_place" = the copy of the finished streams to
 * out + f * stride; cniic_codec_measure_batch leaves both readable after its decode.
 *
 * SMALL `voronoi` frames likewise, here and in cniic_codec_measure_batch: with the expression voronoi(K), 1 <= K <= 256, DEVICE images and
 * opts NULL or opts->flags == 0 (seed and max_iters are honoured), every frame of 1 .. 16384 pixels is coded on ONE workgroup from its
 * pixels to its finished stream of 16 + 19 K bytes: the pixels, their labels, the K centroids and the clusters' sums stay in the CU's LDS
 * for the whole K-means (exact Lloyd over x, y, r, g, b in integers; a point whose squared distance to its own centroid, times four, does
 * not exceed that centroid's squared distance to its nearest neighbour stays without a search, which the triangle inequality makes
 * exact), with no launch boundary and no host round trip between iterations; all such frames of the call in one launch whatever their
 * number.  Larger frames, host images, any CNIIC_KM_* flag, K = 0 or K > 256 go to the worker contexts as above, and so do FEW HEAVY
 * frames, which the workers' whole chip codes faster than one CU each (measured): with n = the call's frames of 1 .. 16384 pixels, a frame
 * takes the route when its pixels x K are at most 131072 for n < 8, at most 786432 for 8 <= n < 128, and always for n >= 128.
 * cniic_codec_encode_batch (equal sizes) does not take the route.  Which route a frame took shows in no output byte, status or message
 * (CNIIC_ERR_TOO_FEW_POINTS before CNIIC_ERR_FEW_ACTIVE before CNIIC_ERR_CAPACITY with lens[f] = bytes needed, as the single call).
 * Stage timers: "vor_small_batch" = the duration of that kernel, with launches = the frames that took the route; "vor_small_place" = the
 * copy of the finished streams to out + f * stride.  stats[f].pair_evals counts what the route that ran evaluated -- on this route one
 * evaluation per point and iteration against its own centroid and K more for every point that was searched, on the workers what their
 * pruned search evaluated; the other four fields do not depend on the route.
 *
 * SMALL `hilbert(rle)` and `hilbert(rle(d))` frames likewise, here and in cniic_codec_measure_batch, for any d (0, finite, +inf, negative,
 * NaN): with DEVICE images every frame of 1 .. 16384 pixels is coded on ONE workgroup from its pixels to its finished stream -- the gather
 * along the scan, the length of the run that would start at every position (the accept test of the single call bit for bit), the chain of
 * true run starts, the rounded averages and the 12-byte records -- all such frames of the call in one launch, in chunks below 2 GiB of
 * scratch whatever their number.  Larger frames, host images and a frame whose size has an injected scan (cniic_ctx_set_scan), which the
 * workers follow, go to the worker contexts as above, and so do FEW or FEW LARGE
 * frames (measured: the call and one CU are slower for them than the workers' whole chip): with n = the call's frames of 1 .. 16384 pixels,
 * no frame takes the route for n < 4, those of at most 4096 pixels do for 4 <= n < 32, and every one for n >= 32.
 * cniic_codec_encode_batch (equal sizes) does not take the route.  Which route a frame took shows in no output byte, status or message
 * (CNIIC_ERR_CAPACITY with lens[f] = bytes needed and the frame's room untouched, as the single call); stats[f] stays zero.  Stage timers:
 * "rle_small_batch" = the duration of that kernel, with launches = the frames that took the route; "rle_small_place" = the copy of the
 * finished streams to out + f * stride; cniic_codec_measure_batch leaves both readable after its decode.
 *
 * SMALL `zip(dict)` frames likewise, here and in cniic_codec_measure_batch, whatever opts holds (the single call ignores it for this
 * codec): with DEVICE images a frame of 1 .. 4096 pixels (the kernel itself takes 16384) is coded on ONE workgroup from its pixels to its finished
 * stream -- the text is never written out, the dictionary's trie is a table of edges in device memory, and the coder's walks are speculated a window of 256
 * text positions at a time and repaired from the entries the window itself made -- all such frames of the call in one launch, in chunks
 * below 1 GiB of scratch.  A frame one of whose matches is longer than 1024 bytes (flat stretches: such a walk is one lane's chain of
 * dependent loads) is given up by the kernel and coded by the worker contexts, as are host images and, measured, LARGER and FEW frames
 * (one workgroup is slower for them than the workers' cores): the frames of at most 4096 pixels take the route when the call has 256 of
 * them or more.  Which route a frame took shows in no output byte,
 * status or message; stats[f] stays zero.  Stage timers: "zd_small_batch", "zd_small_place", "zd_small_handback" and "zd_small_finished"
 * (above cniic_last_kernel_time). */
int32_t cniic_codec_encode_batch_var(cniic_ctx *ctx, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, const uint64_t *img_off,
                                     const uint32_t *w, const uint32_t *h, uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens,
                                     int32_t *rcs, cniic_kmeans_stats *stats);
/* Hilbert { compress: RLE(d) }::encode (hilbertc.rs:26-45; rle_approx :200-299): runs along the Hilbert scan that a pixel joins while its
 * distance to the run's running average is <= d, recorded with the rounded average.  d == 0.0 (or -0.0) gives the `hilbert(rle)`
 * stream; d < 0 or NaN accepts nothing, +inf everything.  The same bytes as cniic_codec_encode(ctx, "hilbert(rle(<d>))", ...), for
 * a caller that holds d as a double.  Host or device buffers; CNIIC_ERR_CAPACITY with *len = bytes needed, like cniic_codec_encode.
 * The stream decodes with "hilbert(rle)" or "hilbert(rle(<any d>))": the records are the same (RleDecoder, hilbertc.rs:304-335). */
int32_t cniic_hilbert_rle_approx_encode(cniic_ctx *ctx, double d, const uint8_t *rgb, uint32_t w, uint32_t h,
                                        uint8_t *out, uint64_t cap, uint64_t *len);
/* The dictionary coder on plain bytes (zip::zip_dict_encode / zip_dict_decode, src/zip/dict.rs).  The stream is what the reference
 * writes: u16 little-endian symbols in pairs -- 0..255 the single bytes, 0xFFFF the empty text, 0x100.. the two texts of a pair joined,
 * one new symbol per pair until 0xFFFE has been handed out (65 279 pairs), after which the dictionary stays as it is.  Up to there the
 * coder is a serial walk and runs on the host; from there on the GPU parses the rest of the text against the frozen trie (encode) and
 * copies every symbol's text out of the part already decoded (decode).  A text whose dictionary never fills (a flat image: entries
 * double in length), or fills with an entry of more than 32 768 bytes or a trie of more than 2^24 nodes, is coded on the host to its
 * end (seconds for tens of megabytes).  Host or device buffers; CNIIC_ERR_CAPACITY with *len = bytes needed.
 * Decode answers CNIIC_ERR_DECODE where the reference panics: a symbol that has not been handed out yet, a first symbol without a
 * second.  0xFFFF is legal anywhere; a single byte behind the last whole pair ends the stream.  No memory is allocated from a size a
 * stream claims before the lengths have been summed and held against cap.
 * Stage timers (cniic_last_kernel_time): "zd_fill_host", "zd_table_host", "zd_match", "zd_chain" or "zd_chain_plain" (the longest
 * entry has more than 255 bytes; with "zd_chain_hybrid", "zd_chain_breaks" and "zd_chain_entered" when the hybrid chain carried the
 * parse across the long matches, without them when the one-block walk did: more than 174 082 break pieces), "zd_compact";
 * "zd_prefix_host", "zd_scan", "zd_copy"; the codecs add "zd_serialize". */
int32_t cniic_zip_dict_encode(cniic_ctx *ctx, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);
int32_t cniic_zip_dict_decode(cniic_ctx *ctx, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);
/* The dimensions of a zip(dict) stream: the first 8 bytes of its text, decoded from its first pairs.  HOST memory, no context.
 * CNIIC_ERR_DECODE when the stream is malformed before it has spelt 8 bytes, or ends there. */
int32_t cniic_zip_dict_dims(const uint8_t *bytes, uint64_t n, uint32_t *w, uint32_t *h);
/* Hilbert { compress: Zip } (hilbertc.rs:27-29,47-49,67-77; name "hilbert-zip", lossless): the 8 raw bytes of dimensions, then the
 * dictionary coder over the 11-byte records (u64 3, r, g, b) of the pixels in scan order -- cniic_hilbert_linearize's, injected scans
 * included.  Decode: CNIIC_ERR_DECODE where the coder's stream is malformed within the w h records the traversal asks for; colours the
 * text does not reach stay zero, as do those from a record on whose length is not 3 (the reference then reads that many items more
 * before it gives up: what is malformed behind such a record is not reported here).  Host or device buffers. */
int32_t cniic_hilbert_zip_encode(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len);
int32_t cniic_hilbert_zip_decode(cniic_ctx *ctx, const uint8_t *bytes, uint64_t n, uint8_t *rgb, uint64_t cap, uint32_t *w, uint32_t *h);
/* The harness's many-images loop (src/bench.rs:24-35; its measure_all loop body :41-60 for the third call) for Hilbert { compress: Zip }
 * (hilbertc.rs:27-29,47-49,58-62,73-77), the codec behind the reference Makefile's output/hilbert-zip.csv: the layouts, HOST arrays,
 * per-frame rcs, return of the first failure, frames == 0 and stage-timer sums of cniic_codec_encode_batch_var, cniic_codec_decode_batch
 * and cniic_codec_measure_batch (described there), without expr, opts and stats.
 * Stream f, lens[f] and rcs[f] are byte for byte what cniic_hilbert_zip_encode gives for image f alone (CNIIC_ERR_CAPACITY with lens[f] =
 * bytes needed and the frame's room untouched); image f, w[f], h[f] and rcs[f] are what cniic_hilbert_zip_decode gives for stream f alone,
 * with its lenient rules: colours the text does not reach stay zero, and so do the colours from the first record on whose length is not 3;
 * a malformed pair inside the needed 11 w h bytes is CNIIC_ERR_DECODE; nothing behind the pair that completes the last record is looked
 * at.  A frame that fails leaves the others as they are.  The measure call's rows are encode -> decode -> cniic_mse of every frame alone.
 * Small frames: DEVICE images of 1 .. 16 384 pixels whose size has no injected scan (cniic_ctx_set_scan: those stay with the worker
 * contexts, which follow the injection) are coded together, a workgroup per frame (k_hz_small: zip(dict)'s small-frame kernel over this
 * codec's text), and streams of such frames are decoded together (k_hz_small_dec); a frame the kernels give up (a match longer than 1024
 * bytes; pairs behind the cap of 24 576, 64 or more generations, a byte behind more than 64 pairs) is handed back to the workers.  The
 * floors from which the routes are taken were measured for this codec against the worker contexts (NOTES AS), under one rule: a class of
 * calls takes a route only where it beat the workers for photo-like, noise and flat frames alike.  The decode route takes the streams of at
 * most 4096 pixels from 4 candidate streams on and every routed size from 256 on.  The ENCODE route is taken by no class: flat frames, which
 * its kernel hands back, lost to the workers at every probed count (photo-like and noise frames of at most 4096 pixels won 1.6x - 4.6x from
 * 256 frames on), so in this library every image is coded by the worker contexts and the "hz_small_batch" marks are never reported; the
 * testing library reaches the route.  Which route a frame
 * took shows in no output byte, dimension, status or message.  Stage timers: "hz_small_batch", "hz_small_place", "hz_small_handback",
 * "hz_small_finished", "hz_small_dec_batch", "hz_small_dec_handback" (cniic_last_kernel_time). */
int32_t cniic_hilbert_zip_encode_batch_var(cniic_ctx *ctx, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h,
                                           uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens, int32_t *rcs);
int32_t cniic_hilbert_zip_decode_batch(cniic_ctx *ctx, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames,
                                       uint8_t *rgb, uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs);
/* The look-back coder on plain bytes (zip::zip_back_encode / zip_back_decode, src/zip/back.rs:5-21).  The stream is what the reference
 * writes: symbols headed by a little-endian u16 (bit 15 the kind, the low 15 bits len) -- explicit, len literal bytes behind it, or
 * look-back, a little-endian u16 `back` behind it: min(len, back) bytes from `back` bytes before the end of the text so far.  Encode
 * (Encoder::next_symbols, :148-212): with six bytes or more ahead, the longest common run of text[q, p) and text[p, n) over every q in
 * [p - 65535, p - 6] whose six bytes equal those at p, the smallest q among equals; none: max(e, 2) more explicit bytes, e the explicit
 * run so far, unprobed.  One workgroup walks a stream, its window in LDS, its lanes sharing each probe's scan of the window; a launch
 * takes the text 256 KiB further.  Host or device buffers; CNIIC_ERR_CAPACITY with *len = bytes needed and nothing written behind cap.
 * CNIIC_ERR_UNSUPPORTED where the reference panics: a look-back or an explicit symbol of 32 768 bytes or more, which the header cannot
 * say (assert in compress_len, back.rs:45) -- a flat stretch of about 3000 pixels, or 32 768 bytes without any repetition at the probed
 * places.  Decode (Decoder, :648-706): ends quietly where no whole header stands, at a look-back header without its `back`, and at a
 * symbol that stands for no byte (explicit of length 0, look-back with len or back 0: Decoder::next then answers None, :657-664);
 * CNIIC_ERR_DECODE where the reference panics: an explicit symbol with fewer than len bytes behind it (:97), a `back` greater than the
 * text so far (:466).  No memory is allocated from a size a stream claims.
 * Stage timers (cniic_last_kernel_time): "zb_encode", "zb_decode" (launches = the slices); the codec adds "zb_serialize", "zb_rebuild".
 * The decode is not inherently serial, and a second route decodes ONE stream with the whole GPU (k_zipback_par.hip): the symbol starts
 * by pointer doubling over next(p), the text positions by a 64-bit prefix sum, the first event in stream order by a minimum, and the
 * text -- a forest, since a copy of min(len, back) bytes never reaches itself -- by at most 32 jump rounds over a source pointer per
 * text byte below cap.  Status, *len, every byte below cap and both messages are the serial walk's.  Streams of 2^32 bytes or more,
 * texts with 2^32 bytes or more below cap, and streams whose tables (9 bytes per stream byte, 8 per text byte below cap) pass 8 GiB
 * are walked serially.
 * Stage timers: "zb_par_decode" (the route's launches; launches = the streams it decoded), "zb_par_handback" (no time; launches = the
 * streams it gave back to the serial walk after starting on them), "zb_par_rounds" (no time; launches = jump rounds run, summed);
 * "zb_decode" keeps its meaning for the streams the serial kernel walks.  Which calls take the route (one stream of 512 KiB or more):
 * at cniic_zip_back_image_decode_batch below. */
int32_t cniic_zip_back_encode(cniic_ctx *ctx, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);
int32_t cniic_zip_back_decode(cniic_ctx *ctx, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);
/* The dimensions of a zip-back stream: the first 8 bytes of its text, decoded from its first symbols (they lie within the first 64
 * bytes).  HOST memory, no context.  CNIIC_ERR_DECODE when the stream is malformed before it has spelt 8 bytes, or ends there. */
int32_t cniic_zip_back_dims(const uint8_t *bytes, uint64_t n, uint32_t *w, uint32_t *h);
/* Zip::Back (src/codec/zipc.rs:14-48; name "zip-back", lossless): the look-back coder over zip(dict)'s text -- (w, h) as two u32, then
 * the 11-byte records (u64 3, r, g, b) of the pixels row by row.  Decode is lazy (zipc.rs:28-36): exactly 8 + 11 w h bytes of text are
 * pulled, whole symbols as they are needed, and nothing behind the symbol that completes the last pixel is looked at; fewer bytes, or a
 * pixel record whose length is not 3, is CNIIC_ERR_DECODE; cap < 3 w h is CNIIC_ERR_CAPACITY.  Host or device buffers. */
int32_t cniic_zip_back_image_encode(cniic_ctx *ctx, const uint8_t *rgb, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len);
int32_t cniic_zip_back_image_decode(cniic_ctx *ctx, const uint8_t *bytes, uint64_t n, uint8_t *rgb, uint64_t cap, uint32_t *w, uint32_t *h);
/* The harness's many-images loop (src/bench.rs:24-35) for Zip::Back: the layouts and the per-frame rcs of cniic_codec_encode_batch_var
 * and cniic_codec_decode_batch (image f is w[f] x h[f] at rgb + img_off[f]; stream f at out + f * stride, its length in lens[f];
 * decoded image f at rgb + f * img_stride; img_off, w, h, lens, rcs: HOST arrays).  Every frame is one workgroup of the same launches,
 * whatever their number; stream, lens[f] and rcs[f] are what the single call gives for frame f, and a frame that fails (UNSUPPORTED,
 * CAPACITY with lens[f] = bytes needed, DECODE) leaves the others as they are.  rcs may be NULL; the call returns the first failure
 * (lowest f) with its message in cniic_last_error; frames == 0 returns CNIIC_OK.
 * Which decode calls take the whole-GPU route (cniic_zip_back_decode, cniic_zip_back_image_decode, cniic_zip_back_image_decode_batch
 * alike; a class of calls is (streams in the call that can be decoded, stream length), and it takes the route only where 5 runs of it
 * lay clear of 5 runs of the serial walk for photo-like AND noise; profiles/zip_back_probe.json, NOTES.md AW):
 *   1 stream, 512 KiB of stream or more     the route.  Measured from 463 / 510 KB (256 x 256, photo-like / noise) to 7.5 / 8.1 MB
 *                                           (1024 x 1024): 0.39 - 1.5 ms against the serial walk's 61 - 1087 ms
 *   1 stream below 512 KiB                  serial: not measured
 *   2 streams or more                       serial.  8 / 32 / 100 photo-like frames of 148 - 450 KB won (2.8 / 11 / 35 ms against
 *                                           52 / 59 / 64), one stream after the other, but no noise folder was measured
 * The route's tables are not part of cniic_zip_back_image_measure_batch's chunk budget: a chunk of several frames decodes serially;
 * a chunk of ONE frame (an image too large to share a chunk) takes the route, and its tables -- 9 bytes per stream byte, 8 per text
 * byte, each part at most 8 GiB -- come on top of the budget while that frame is decoded. */
int32_t cniic_zip_back_image_encode_batch_var(cniic_ctx *ctx, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h,
                                              uint32_t frames, uint8_t *out, uint64_t stride, uint64_t *lens, int32_t *rcs);
int32_t cniic_zip_back_image_decode_batch(cniic_ctx *ctx, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t frames,
                                          uint8_t *rgb, uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs);
/* (One call for a whole folder's encode -> decode -> MSE: cniic_zip_back_image_measure_batch, below beside cniic_hilbert_zip_measure_batch.) */
/* Codec::decode: CNIIC_ERR_DECODE where the reference returns None / panics.  zip(dict): the reader is lazy (zipc.rs:28-36) -- exactly
 * 8 + 11 w h bytes of text are pulled, whole pairs as they are needed, and nothing behind the pair that completes the last pixel is
 * looked at; fewer bytes, or a pixel record whose length is not 3, is CNIIC_ERR_DECODE. */
int32_t cniic_codec_decode(cniic_ctx *ctx, const char *expr, const uint8_t *bytes, uint64_t n,
                           uint8_t *rgb, uint64_t cap, uint32_t *w, uint32_t *h);
/* Codec::decode of `frames` streams: stream f at bytes + f * stride, lens[f] bytes (exactly what cniic_codec_encode_batch writes).
 * Image f goes to rgb + f * img_stride (capacity img_stride bytes); its dimensions go to w[f], h[f].  Host or device memory on either
 * side.  Streams of one batch may carry different dimensions.  `hufman` and `cluster-colors` frames, and `hilbert(rle)` /
 * `hilbert(rle(d))` frames of up to 2^18 pixels (larger ones measured no faster that way), are decoded together in one set of launches
 * (stage timers: "rle_dec_batch" for the last, launches = the frames decoded that way; a frame that fails there may leave zeros in
 * its own w * h * 3 bytes); other codecs, and the frames that route does not take, are decoded one by one on the worker contexts of
 * cniic_codec_encode_batch (CNIIC_OPT_BATCH_STREAMS at a time).  rcs (may be NULL): per-frame status, identical to what
 * cniic_codec_decode returns for that stream alone.  The call returns the first failure; cniic_last_error carries that frame's
 * message.  frames == 0 returns CNIIC_OK.
 *
 * SMALL `delta` frames of a decode, here and in cniic_codec_measure_batch, mirror the encode's: with the expression `delta`, every frame
 * of 1 .. 16 384 pixels whose image fits img_stride, whose size has no injected scan (cniic_ctx_set_scan) and whose decoder -- parsed on
 * the host with the others' -- has no code longer than 19 bits (no encoder of so few symbols makes one) is decoded on ONE workgroup from
 * its payload to its pixels in place (the payload's bits in 1024 subsequences that settle among themselves, FromDiff as a scan, the walk
 * along the scan, the image stored whole), all such frames of the call in one launch whatever their number.  Host or device memory on
 * either side, at any alignment.  Larger frames, a frame of exactly the injected scan's size, a decoder that does not parse or has a
 * longer code, and a frame whose subsequences have not settled within the kernel's rounds go to the worker contexts as above.  Which
 * route a frame took shows in no output byte, status or message, with one difference in a frame's favour: a frame that fails on this
 * route ("delta: cannot decode the difference stream", "delta: colour out of range (hilbertc.rs:505)") leaves its w * h * 3 bytes
 * untouched.  Stage timer: "delta_small_dec_batch" = the duration of that kernel, with launches = the frames it was given;
 * cniic_codec_measure_batch leaves it readable beside the encode's "delta_small_batch".
 * When the streams lie in device memory their decoders are parsed there as well, a workgroup per frame and all frames in one launch: the
 * block reads the header and the pre-order trie where the stream lies and leaves the leaves' codes and symbols for the decode kernel, so
 * that no byte of such a stream comes to the host.  A decoder that kernel does not finish -- more than 16 384 leaves, a code longer than
 * 19 bits, bytes that are no decoder -- is parsed on the host as before, and so is every decoder of a batch in host memory: the routed
 * frames, every status and every message are the same either way.  Stage timers, only when that parse ran: "delta_small_dec_parse" = the
 * duration of its launches, with launches = the frames it parsed; "delta_small_dec_parse_host" = no time, launches = the frames handed
 * back to the host's parse.
 *
 * SMALL `hufman` and `cluster-colors` frames of a decode likewise, here and in cniic_codec_measure_batch (a cluster-colors stream is a
 * Hufman stream of palette colours): every frame of 1 .. 16384 pixels whose image fits img_stride and whose decoder -- parsed on the
 * host, up to 16 threads -- has no code longer than 19 bits is decoded on ONE workgroup by the `delta` decode's kernel body over RGB
 * symbols (no FromDiff and no scan: position d is pixel d; the image stored whole, and a frame whose payload ends early, "Failed to
 * decode symbol", leaves its bytes untouched), all such frames of the call in one launch per chunk of scratch.  Host or device memory
 * on either side, at any alignment.  The decoders of such streams in device memory are most of the stream (12 bytes a leaf), so the
 * heads are looked at a second time in groups of as many frames as the pinned block holds at their full width, not cut to fit.  Larger
 * frames, a longer code, a decoder that does not parse and a frame that has not settled within the kernel's rounds keep the routes
 * above, and so do the small frames of a call that has fewer than 256 of them (measured: below that the batched route is as fast or faster).  Which route a frame took shows in no output byte, status or message.  Stage timer: "huf_small_dec_batch" = the duration of
 * that kernel, with launches = the frames it was given; cniic_codec_measure_batch leaves it readable beside the encode's
 * "huf_small_batch" (or, for cluster-colors, "cc_small_batch").
 * When the streams lie in device memory and the call has at least 256 of them that are short enough to be a small frame's (8 .. 251 911
 * bytes), their decoders are parsed there first, as the `delta` streams' are: a workgroup per frame reads the header and the pre-order
 * trie of Rgb leaves where the stream lies and leaves the table the decode kernel reads.  A frame that kernel does not finish -- too many
 * pixels for this route, more than 16 384 leaves, a code longer than 19 bits, bytes that are no decoder -- goes back to the host's parse
 * and the routes it had, and so does every frame when fewer than 256 turn out to be small; streams in host memory keep the host's parse.
 * The routed frames, every status and every message are the same either way.  Stage timers, only when that parse ran:
 * "huf_small_dec_parse" = the duration of its launches, with launches = the frames it parsed; "huf_small_dec_parse_host" = no time,
 * launches = the candidates handed back to the host's parse.
 *
 * SMALL `voronoi` frames of a decode, here and in cniic_codec_measure_batch: with the expression voronoi(K) (the stream carries its own
 * K), every frame whose header and whole centroid list are there and well formed, with 1 <= K <= 256 centroids, 1 .. 16384 pixels and an
 * image that fits img_stride, is repainted on ONE workgroup (its centroids in the CU's LDS; every pixel the colour of the FIRST centroid
 * with the smallest (c.x - x)^2 + (c.y - y)^2 in u32 arithmetic that wraps, as the single decode; the image stored whole, with 16-byte
 * stores where the address allows and not a byte outside its 3 w h), all such frames of the call in one launch whatever their number.
 * The heads come to the host as the other codecs' do (at most 16 + 19 * 256 = 4880 bytes of a stream in device memory, never more than
 * stride) and are parsed there.  Host or device memory on either side, at any alignment.  Every other frame -- larger, K = 0 or K > 256,
 * a truncated or malformed centroid, w h = 0, an image that does not fit, a head cut by a stride below the stream's length -- goes to
 * the worker contexts as above, with the single decode's status and message.  Which route a frame took shows in no output byte, status
 * or message.  Stage timer: "vor_small_dec_batch" = the duration of that kernel, with launches = the frames it was given;
 * cniic_codec_measure_batch leaves it readable beside the encode's "vor_small_batch".  (A decode evaluates no K-means: no pair_evals.)
 *
 * SMALL `zip(dict)` frames of a decode, here and in cniic_codec_measure_batch: the host reads the first 64 bytes -- 16 pairs -- of every
 * stream, and a frame whose head spells the 8 bytes of the dimensions, with 1 .. 16384 pixels, an image that fits img_stride and (in a
 * call of several frames) a stream that ends before the next one starts, is a candidate.  The decode of this coder is not serial: pair k
 * hands out symbol 0x100 + k whatever it holds, so a symbol is the text of an earlier pair, which already lies in the output.  A
 * candidate is decoded on ONE workgroup, from its pairs to its pixels: the pairs' lengths in rounds over the pairs they are made of,
 * their offsets as a saturating prefix sum, then every byte of the text by a binary search for its pair and hops from pair to pair down
 * to a literal -- no text is written out -- the records checked, the image assembled in the CU's LDS and stored whole, with 16-byte
 * stores where the address allows and not a byte outside its 3 w h.  All such frames of a chunk of scratch go in one launch per size
 * class of LDS (16, 32, 64 KiB, and up to a CU's 160), so that small frames share a CU.  The reader is lazy, as the single decode's:
 * nothing behind the pair that completes the text is looked at.  A frame with more than 24 576 pairs before its text is complete, with
 * pairs nested 64 or more generations deep, or with a byte that lies behind more than 64 pairs is handed back to the worker contexts,
 * as is every frame that is no candidate; they get the single decode's status and message, and so does a frame that fails on this
 * route, with the one difference that it leaves its 3 w h destination bytes untouched.  Host or device memory on either side, at any
 * alignment.  The floor, measured against the worker contexts: a call with fewer than 8 candidates keeps them all on the workers, one
 * with 8 .. 31 gives the route its candidates of at most 4096 pixels, one with 32 or more gives it all of them.  Which route a frame took
 * shows in no output byte, dimension, status or message.  Stage timers: "zd_small_dec_batch" = the duration of the kernel's launches,
 * with launches = the frames it was given; "zd_small_dec_handback" = no time, launches = the frames of those it handed back;
 * cniic_codec_measure_batch leaves both readable beside the encode's "zd_small_batch". */
int32_t cniic_codec_decode_batch(cniic_ctx *ctx, const char *expr, const uint8_t *bytes, uint64_t stride, const uint64_t *lens,
                                 uint32_t frames, uint8_t *rgb, uint64_t img_stride, uint32_t *w, uint32_t *h, int32_t *rcs);
/* bench::compute_error (src/bench.rs:95-104): MSE between two RGB8 images. */
int32_t cniic_mse(cniic_ctx *ctx, const uint8_t *a, const uint8_t *b, uint64_t npx, double *mse);
/* bench::compute_error for `frames` image pairs of npx pixels each (a + f*npx*3, b + f*npx*3): mse[f] == cniic_mse of that pair. */
int32_t cniic_mse_batch(cniic_ctx *ctx, const uint8_t *a, const uint8_t *b, uint64_t npx, uint32_t frames, double *mse);
/* bench::compute_error (src/bench.rs:95-104) for `frames` pairs of DIFFERENT sizes in one launch, whatever their number: pair f is
 * npx[f] pixels, a + a_off[f] against b + b_off[f] (bytes, any alignment on either side; a and b are host or device memory, a_off /
 * b_off / npx / mse HOST arrays).  mse[f] is bit-equal to cniic_mse of that pair (the exact integer sum over npx[f]); npx[f] == 0
 * gives 0.0.  One pair may be longer than 2^32 bytes.  Stage timers: "sqerr_batch_var". */
int32_t cniic_mse_batch_var(cniic_ctx *ctx, const uint8_t *a, const uint64_t *a_off, const uint8_t *b, const uint64_t *b_off,
                            const uint64_t *npx, uint32_t frames, double *mse);
/* The body of bench::measure_all's loop (src/bench.rs:28-76) for a whole folder in ONE call: encode, size, ratio, decode, MSE and
 * the lossless check, = cniic_codec_encode_batch_var -> cniic_codec_decode_batch -> cniic_mse_batch_var with the streams and the
 * decoded images staying in HBM.  Row f equals what cniic_codec_encode_opts, cniic_codec_decode and cniic_mse give for image f alone.
 * The folder is worked through largest image first in chunks of at most 2 GiB of scratch HBM (streams with room for the worst case +
 * decoded images; an image that needs more on its own is a chunk of its own), so a folder of any size works.  A frame that fails has
 * its rc set, compressed_size = 0 and compression_ratio = error = NaN, and the others go on (bench.rs:78 prints the error and
 * continues); the call returns the first failure (lowest f) with its message in cniic_last_error.
 * out / stride / lens (HOST array) may be NULL / 0 / NULL when the caller does not want the streams; with out, stream f is copied to
 * out + f * stride (host or device memory) if it fits, otherwise that row's rc is CNIIC_ERR_CAPACITY (its measurements are
 * still filled in) and lens[f] says what it needs. */
typedef struct {
    uint64_t compressed_size;    /* bench.rs:37                                                        */
    double   compression_ratio;  /* bench.rs:43,74: size / (w * h * 24) * 100, computed in 64 bits      */
    double   error;              /* bench.rs:48, = cniic_mse(image, decoded)                           */
    int32_t  rc;                 /* CNIIC_OK, or what the encode / the decode of this image returned   */
    uint32_t lossless_mismatch;  /* bench.rs:57-59: 1 = a lossless codec whose decode differs          */
    cniic_kmeans_stats kmeans;   /* of the encode                                                      */
} cniic_measure_row;
int32_t cniic_codec_measure_batch(cniic_ctx *ctx, const char *expr, const cniic_kmeans_opts *opts, const uint8_t *rgb, const uint64_t *img_off,
                                  const uint32_t *w, const uint32_t *h, uint32_t frames, cniic_measure_row *rows,
                                  uint8_t *out, uint64_t stride, uint64_t *lens);
/* The same for Hilbert { compress: Zip } (bench.rs:41-60 with that codec; described at cniic_hilbert_zip_encode_batch_var): row f equals
 * cniic_hilbert_zip_encode -> cniic_hilbert_zip_decode -> cniic_mse of image f alone; rows[f].kmeans stays zero. */
int32_t cniic_hilbert_zip_measure_batch(cniic_ctx *ctx, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t frames,
                                        cniic_measure_row *rows, uint8_t *out, uint64_t stride, uint64_t *lens);
/* The body of bench::measure_all's loop (src/bench.rs:28-76) for a whole folder of Zip::Back in ONE call: the arguments, layouts, HOST
 * arrays and rows (cniic_measure_row) of cniic_hilbert_zip_measure_batch.  Row f equals cniic_zip_back_image_encode ->
 * cniic_zip_back_image_decode -> cniic_mse of image f alone; rows[f].kmeans stays zero.  Streams, texts and decoded images stay in HBM
 * between the three steps.  The folder is worked through largest image first in chunks of at most 2 GiB of scratch HBM (per frame:
 * the stream with room for the worst case, the encoder's and the decoder's text at 11 B/px, the decoded image, and the image itself
 * when it comes from host memory; an image that needs more on its own is a chunk of its own).  A frame the reference panics on
 * (CNIIC_ERR_UNSUPPORTED, back.rs:45) has its rc set, compressed_size = 0 and compression_ratio = error = NaN, and the others go on;
 * the call returns the first failure (lowest f) with its message in cniic_last_error; frames == 0 returns CNIIC_OK.
 * out / stride / lens may be NULL / 0 / NULL; with out, stream f is copied to out + f * stride (host or device memory) if it fits,
 * otherwise that row's rc is CNIIC_ERR_CAPACITY (its measurements are still filled in) and lens[f] says what it needs. */
int32_t cniic_zip_back_image_measure_batch(cniic_ctx *ctx, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h,
                                           uint32_t frames, cniic_measure_row *rows, uint8_t *out, uint64_t stride, uint64_t *lens);

/* ------------------------------------------------------------------ surfaces: what a decoder or a crop hands over <-> packed RGB24 */
/* Every call above takes packed RGB24, rows back to back; the reference takes an image::DynamicImage and begins with px.to_rgb() per
 * pixel (clusterc.rs:19,151, hilbertc.rs:29,410, zipc.rs:19, bench.rs:97).  These two calls are that step for frames that already lie
 * in HBM the way a video pipeline delivers them: with a row pitch, as grey, RGBA, BGRA or NV12, or as a window of a larger image.
 * One kernel launch per call whatever the number of frames, written exactly where the *_batch_var, cniic_cc_*_var and
 * cniic_palette_*_var calls read (rgb + img_off[f], any alignment). */
#define CNIIC_PX_L8    1   /* 1 B/px: (l, l, l)              Luma<u8>::to_rgb()                 */
#define CNIIC_PX_LA8   2   /* 2 B/px: l, a -> (l, l, l)      alpha dropped                      */
#define CNIIC_PX_RGB8  3   /* 3 B/px: copy (a pitched image, a crop)                            */
#define CNIIC_PX_RGBA8 4   /* 4 B/px: alpha dropped          Rgba<u8>::to_rgb()                 */
#define CNIIC_PX_BGR8  5   /* 3 B/px: the ends swapped                                          */
#define CNIIC_PX_BGRA8 6   /* 4 B/px: the ends swapped, alpha dropped                           */
#define CNIIC_PX_NV12  7   /* Y plane + interleaved U,V plane at half resolution both ways      */
/* NV12: pixel (x, y) takes Y from the Y plane and (U, V) from pair x >> 1 of UV row y >> 1 (the nearest chroma sample, no
 * interpolation; the UV plane has ceil(h / 2) rows of ceil(w / 2) pairs).  With D = U - 128, E = V - 128, floor() a floor and every
 * result clipped to 0 ... 255, in 32-bit integers (the largest magnitude is below 2^18) and without any floating point:
 *   matrix         C        R                                  G                                          B
 *   601 limited    Y - 16   floor((298 C + 409 E + 128) / 256)  floor((298 C - 100 D - 208 E + 128) / 256)  floor((298 C + 516 D + 128) / 256)
 *   709 limited    Y - 16   floor((298 C + 459 E + 128) / 256)  floor((298 C -  55 D - 136 E + 128) / 256)  floor((298 C + 541 D + 128) / 256)
 *   601 full       Y        floor((256 C + 359 E + 128) / 256)  floor((256 C -  88 D - 183 E + 128) / 256)  floor((256 C + 454 D + 128) / 256)
 *   709 full       Y        floor((256 C + 403 E + 128) / 256)  floor((256 C -  48 D - 120 E + 128) / 256)  floor((256 C + 475 D + 128) / 256)
 * This table is the definition. */
#define CNIIC_YUV_601_LIMITED 1
#define CNIIC_YUV_601_FULL    2
#define CNIIC_YUV_709_LIMITED 3
#define CNIIC_YUV_709_FULL    4
typedef struct {
    uint64_t off;       /* first byte of row 0 (NV12: of the Y plane), from the base pointer  */
    uint64_t pitch;     /* bytes from one row to the next, >= w * bytes per pixel             */
    uint64_t off_uv;    /* NV12: first byte of the UV plane; otherwise ignored                */
    uint64_t pitch_uv;  /* NV12: >= 2 * ceil(w / 2); otherwise ignored                        */
    uint32_t w, h;
    int32_t  format;    /* CNIIC_PX_*  */
    int32_t  matrix;    /* NV12: CNIIC_YUV_*; otherwise ignored */
} cniic_surface;

/* HOST only, no context: validates one descriptor.  *src_end = one past the last byte the import may read (from the base pointer),
 * *rgb_bytes = 3 w h.  CNIIC_ERR_BAD_ARG for what the calls below refuse in a descriptor: a null argument, an unknown format, NV12
 * without a known matrix, w h == 0 or w h >= 2^32, a pitch below the row's bytes (pitch_uv below 2 ceil(w / 2)), a surface whose end
 * does not fit 64 bits. */
int32_t cniic_surface_span(const cniic_surface *s, uint64_t *src_end, uint64_t *rgb_bytes);
/* Frame f: surface s[f] of src -> packed RGB24 at rgb + img_off[f].  L8 / LA8 give r = g = b = l, RGB8 is a copy, RGBA8 drops a, BGR8 /
 * BGRA8 swap the ends, NV12 as above; bytes of a source row behind w * bytes per pixel (the pitch's padding) are never read.
 * s and img_off are HOST arrays of `frames` entries; src and rgb are host or device memory (host memory is staged through the context's
 * scratch: the source as ONE range from the first byte any surface reads to the last, a host rgb frame by frame, so that nothing
 * between the frames is written).  Any offsets, pitches and alignments are legal, and several surfaces may read the same bytes (32
 * windows of one image are 32 descriptors on it).  Source and destination may not overlap; this is not checked.  With device memory
 * on both sides the call returns once the launch is enqueued on the context's stream (cniic_sync waits for it; a later call on this
 * context is ordered behind it).  frames == 0 returns CNIIC_OK.  CNIIC_ERR_BAD_ARG with NOTHING written: a null argument, a descriptor
 * that cniic_surface_span refuses, a frame whose end (img_off[f] + 3 w h) does not fit 64 bits.  Stage timer: "surf_import", launches = 1. */
int32_t cniic_frames_from_surfaces(cniic_ctx *ctx, const uint8_t *src, const cniic_surface *s, uint32_t frames,
                                   uint8_t *rgb, const uint64_t *img_off);
/* The way back, for display: packed RGB24 at rgb + img_off[f] -> surface s[f] of dst; RGB8 / BGR8 / RGBA8 / BGRA8 only, and the alpha
 * byte written is `alpha`.  Bytes of a destination row behind w * bytes per pixel are not written.  Memory and arguments as above (a
 * host dst is filled row by row, so its padding stays as it was); a 4-byte format whose rows do not start on a multiple of 4 is
 * legal and written in byte stores.  CNIIC_ERR_BAD_ARG with nothing written: as above, and L8, LA8 or NV12, and alpha > 255.
 * Stage timer: "surf_export", launches = 1. */
int32_t cniic_frames_to_surfaces(cniic_ctx *ctx, const uint8_t *rgb, const uint64_t *img_off, const cniic_surface *s,
                                 uint32_t frames, uint8_t *dst, uint32_t alpha);

/* ------------------------------------------------------------------ synthetic inputs (bench/tests) */
#define CNIIC_SYNTH_UNIFORM 0  /* "U": splitmix64 byte stream                               */
#define CNIIC_SYNTH_PHOTO   1  /* "P": bilinear 64-px lattice + noise, photo-like statistics */
int32_t cniic_synth_image(cniic_ctx *ctx, int32_t kind, uint64_t seed, uint32_t w, uint32_t h, uint8_t *rgb);

#ifdef __cplusplus
}
#endif
#endif
