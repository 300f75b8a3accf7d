// codec.hpp -- the reference's Codec surface (src/codec.rs:14-19) for the hot-path codecs.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

namespace cniic {

// CODEC_HILBERT_ZIP is internal: Hilbert { compress: Zip } is no expression here (parse_codec never produces it, and the entry points that take an
// expression do not know it); cniic_hilbert_zip_*_batch* make the descriptor themselves and drive the batch engines with it.
enum CodecKind { CODEC_HUFMAN = 1, CODEC_CLUSTER_COLORS = 2, CODEC_VORONOI = 3, CODEC_DELTA = 4, CODEC_HILBERT_RLE = 5, CODEC_ZIP_DICT = 6, CODEC_HILBERT_ZIP = 7 };

struct CodecDesc {
    int      kind;
    uint32_t arg;  // K for cluster-colors / voronoi
    double   darg; // d of hilbert(rle(d)); 0 for `hilbert(rle)` (and for d == 0.0 or -0.0, which is the same codec) and every other kind
};

bool        parse_codec(const char *expr, CodecDesc *out);  // AnyCodec::from_str (codec.rs:41-59)
std::string codec_name(const CodecDesc &d);                 // Codec::name
std::string rust_f64_display(double d);                     // format!("{}", d) of an f64, as Codec::name of hilbert(rle(d)) prints it
bool        codec_is_lossless(const CodecDesc &d);          // Codec::is_lossless

// rgb_d is device memory; out / rgb_out may be host or device.
int codec_encode(Ctx *c, const CodecDesc &d, const uint8_t *rgb_d, uint32_t w, uint32_t h, const cniic_kmeans_opts *opts,
                 uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats);
// the same for cluster-colors(K) / voronoi(K) with the K-means started from init_h (host: K x 3 bytes / K cniic_colorpos); cent_out_h (may be null)
// receives the final centroids in the same layout
int codec_encode_warm(Ctx *c, const CodecDesc &d, const uint8_t *rgb_d, uint32_t w, uint32_t h, const cniic_kmeans_opts *opts, const void *init_h,
                      uint8_t *out, uint64_t cap, uint64_t *len, void *cent_out_h, cniic_kmeans_stats *stats);
// Hilbert { compress: RLE(d) }::encode for any d (d == 0.0: the `hilbert(rle)` stream); rgb_d is device memory, out host or device.
int encode_hilbert_rle(Ctx *c, double d, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len);
// bytes may be host or device memory: of a stream in HBM only the head comes to the host, the payload is decoded where it lies.
int codec_decode(Ctx *c, const CodecDesc &d, const uint8_t *bytes, uint64_t nbytes, uint8_t *rgb_out, uint64_t cap,
                 uint32_t *w, uint32_t *h);

// ---- a frame of cniic_codec_encode_batch_var / cniic_codec_measure_batch (capi.cpp encode_frames)
struct VarFrame {
    const uint8_t *src = nullptr;   // the image (host or device memory, any alignment)
    uint32_t w = 0, h = 0;
    uint8_t *out = nullptr;         // where its stream goes, cap bytes at most
    uint64_t cap = 0;
    uint64_t len = 0;               // results: what cniic_codec_encode_opts answers for this image alone
    int32_t rc = CNIIC_OK;
    cniic_kmeans_stats st{};
    std::string msg;
    bool handed_back = false;       // a small-frame route gave the frame up: encode_frames sends it to the workers
};
// ---- the small-frame encode routes (codec.cpp; capi.cpp kSmallRoutes picks the frames)
// Each codes n > 0 small frames (DEVICE images of 1 .. the route's bound pixels, largest first; all destinations host or all device memory)
// together, one workgroup per frame.  The frames go in chunks whose scratch stays below 2 GiB (for_chunks); a chunk is one upload of its
// rows, ONE launch of the route's kernel under the stage timer "<route>_batch" (launches = the chunk's frames), one copy down of its
// result rows (run_rows), then every stream from its slot of the scratch to its own destination unless it is longer than the frame's cap
// (place_streams: k_cc_small_place under "<route>_place" for device destinations, one copy down of the scratch for host destinations).
// Every frame's rc, len, st and msg are filled in as cniic_codec_encode_opts would for that frame alone; what a route returns is the
// status of the machinery, not of a frame.  The testing library can switch a route off (CNIIC_TEST_<ROUTE>_OFF=1) and lower its pixel
// bound (CNIIC_TEST_<ROUTE>_MAX_PX).  What differs:
//   cc_small     cluster-colors(K <= 256), kCcSmallMaxPx: k_cc_small runs the K-means with a palette per frame, frames_tail codes the frames that go on into the scratch
//   delta_small  `delta`, kDeltaSmallMaxPx: k_delta_small, from the pixels to the finished stream; st stays zero, as in the single call
//   huf_small    `hufman`, kHufSmallMaxPx: k_huf_small, the same kernel body over the pixels' own colours (huf_small.hpp); st stays zero; chunks: CNIIC_TEST_MEASURE_BUDGET
//   vor_small    voronoi(K <= 256), kVorSmallMaxPx: k_vor_small, from the pixels through the whole K-means to the finished stream (st.pair_evals: what
//                this route evaluated); chunks: CNIIC_TEST_MEASURE_BUDGET; without the stay test: CNIIC_TEST_VOR_SMALL_NO_STAY=1
int cc_small_encode(Ctx *c, uint32_t K, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n);
int delta_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n);
int huf_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n);
//   rle_small    `hilbert(rle)` and `hilbert(rle(d))`, any d, kRleSmallMaxPx: k_rle_small, from the pixels to the finished stream (rle_small.hpp); T(d) and the
//                mode are found once per call; st stays zero; chunks: CNIIC_TEST_MEASURE_BUDGET
int vor_small_encode(Ctx *c, uint32_t K, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n);
int rle_small_encode(Ctx *c, double d, VarFrame *const *fr, uint32_t n);
//   zd_small     `zip(dict)`, kZdSmallMaxPx: k_zd_small, from the pixels to the finished stream (zd_small.hpp), a trie table per frame in the chunk's scratch
//                (1 GiB; CNIIC_TEST_MEASURE_BUDGET); a frame with a match longer than kZsGiveUp bytes (the testing library: CNIIC_TEST_ZD_SMALL_CAP) comes back
//                with handed_back set and nothing else filled in ("zd_small_handback": launches = such frames; "zd_small_finished": launches = walks the
//                commit wave finished); st stays zero
int zd_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n);
//   hz_small     Hilbert { compress: Zip } (CODEC_HILBERT_ZIP), kHzSmallMaxPx: k_hz_small, zd_small's kernel body over the text of hz_small.hpp (the pixels in scan
//                order, no dimensions; the 8 raw bytes of the dimensions in front of the pairs); the same scratch, caps (CNIIC_TEST_HZ_SMALL_CAP) and marks
//                ("hz_small_handback", "hz_small_finished"); st stays zero
int hz_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n);

// ---- output assembly
// The encoded stream (host-built header + device-packed payload) is assembled in HBM: directly in
// the caller's buffer when that is 4-byte aligned device memory, otherwise in a staging buffer
// that is copied out once.
struct StreamOut {
    Ctx *c;
    uint8_t *caller;
    uint64_t cap;
    uint64_t *len;
    bool direct = false;
    DevBuf staging;
    uint8_t *dev = nullptr;
    uint64_t total = 0;
    StreamOut(Ctx *ctx, uint8_t *out, uint64_t capacity, uint64_t *len_out) : c(ctx), caller(out), cap(capacity), len(len_out) {}
    int begin(const std::vector<uint8_t> &header, uint64_t payload_bytes) {
        CNIIC_TRY(begin_sized(header.size(), payload_bytes));
        return put_header(header);
    }
    // the header's bytes may follow the payload (put_header): its size is enough to place the payload
    int put_header(const std::vector<uint8_t> &header) {
        if (!header.empty()) CNIIC_HIP_TRY(c, hipMemcpyAsync(dev, header.data(), header.size(), hipMemcpyHostToDevice, c->stream));
        return CNIIC_OK;
    }
    int begin_sized(uint64_t header_bytes, uint64_t payload_bytes, bool zero = true) {
        total = header_bytes + payload_bytes;
        *len = total;
        if (total > cap) return c->fail(CNIIC_ERR_CAPACITY, "encode: stream is %llu bytes, capacity %llu",
                                        (unsigned long long)total, (unsigned long long)cap);
        const uint64_t padded = (total + 3) & ~3ull;
        direct = is_device_ptr(caller) && (reinterpret_cast<uintptr_t>(caller) & 3) == 0 && padded <= cap;
        if (direct) dev = caller;
        else { CNIIC_HIP_TRY(c, staging.alloc(padded + 16)); dev = staging.as<uint8_t>(); }
        if (zero) CNIIC_HIP_TRY(c, hipMemsetAsync(dev, 0, padded, c->stream));
        return CNIIC_OK;
    }
    int finish() {
        if (!direct && total)
            CNIIC_HIP_TRY(c, hipMemcpyAsync(caller, dev, total, is_device_ptr(caller) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CNIIC_OK;
    }
};

// ---- zipdict.cpp: the dictionary coder (src/zip/dict.rs) and its two codecs.  The stream of a text is u16 symbols in pairs.
// text_d: the coder's input in HBM; text_h: the same bytes in host memory, when the caller has them there (else null); head: bytes the
// stream starts with, outside the coder.  out: host or device.
int zip_dict_encode_text(Ctx *c, const uint8_t *text_d, const uint8_t *text_h, uint64_t N, const std::vector<uint8_t> &head, uint8_t *out, uint64_t cap,
                         uint64_t *len);
int zip_dict_decode_bytes(Ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);   // the whole text; bytes / out: host or device
int zip_dict_dims(const uint8_t *bytes, uint64_t n, uint32_t *w, uint32_t *h);   // host memory: the first 8 bytes of the text
int encode_zip_dict(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len);
int decode_zip_dict(Ctx *c, const uint8_t *bytes, uint64_t nbytes, uint8_t *rgb_out, uint64_t cap, uint32_t *w, uint32_t *h);
int encode_hilbert_zip(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len);
int decode_hilbert_zip(Ctx *c, const uint8_t *bytes, uint64_t nbytes, uint8_t *rgb_out, uint64_t cap, uint32_t *w, uint32_t *h);

// ---- zipback.cpp: the look-back coder (src/zip/back.rs) and its codec Zip::Back, a batch at a time (k_zipback.hip: one workgroup per stream)
int zip_back_encode_text(Ctx *c, const uint8_t *text_d, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);   // text_d: HBM; out: host or device
int zip_back_decode_bytes(Ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len);    // the whole text; bytes / out: host or device
// host memory: the first 8 bytes of the text of a stream of `total` bytes, of which the first `avail` are at bytes (64 are always enough)
int zip_back_dims(const uint8_t *bytes, uint64_t avail, uint64_t total, uint32_t *w, uint32_t *h);
// the layouts of cniic_codec_encode_batch_var / cniic_codec_decode_batch; rgb, out, bytes: host or device; the other arrays on the host;
// msgs (optional): every frame's message, empty where it went well (cniic_zip_back_image_measure_batch folds them by frame)
int encode_zip_back_batch(Ctx *c, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t F, uint8_t *out, uint64_t stride,
                          uint64_t *lens, int32_t *rcs, std::vector<std::string> *msgs = nullptr);
int decode_zip_back_batch(Ctx *c, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t F, uint8_t *rgb, uint64_t img_stride, uint32_t *w,
                          uint32_t *h, int32_t *rcs, std::vector<std::string> *msgs = nullptr);

// cniic_codec_decode_batch's device route: the `hufman` / `cluster-colors` / `hilbert(rle)` frames and the small `delta`, `voronoi`, `zip(dict)`
// and (cniic_hilbert_zip_decode_batch) Hilbert { compress: Zip } frames of a batch decoded together (stream f at bytes + f *
// stride, lens[f] bytes; image f to rgb + f * img_stride).  taken[f] = 1: frame f was decoded here (rcs[f], msgs[f], w[f], h[f]); 0: the
// caller decodes it on its own (codec_decode).
int codec_decode_batch_route(Ctx *c, const CodecDesc &d, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t F, uint8_t *rgb,
                             uint64_t img_stride, uint32_t *w, uint32_t *h, std::vector<uint8_t> &taken, std::vector<int32_t> &rcs,
                             std::vector<std::string> &msgs);

// cluster-colors in pieces (see codec.cpp)
struct CcSession {
    Ctx *c = nullptr;
    uint32_t K = 0;
    uint32_t *table = nullptr;   // dense colour table: counts on entry of cc_prepare, key -> rank + 1 afterwards
    uint64_t U = 0;
    DevBuf keys_d, weight_d;
    bool counts_local = false;   // dense table: weight_d holds THIS session's pixels per colour (one rank, or the caller's own image), not the union's
    DevBuf gbits, gprefix, gtotal;  // shared palette over several images: index of the colours that occur in ANY of them (+ their number, on the device)
    bool local_points = false;   // ... and the points of this session are this image's colours only
    SpPlan sp;                   // large images: the pixels partitioned by colour super-cell (k_points.hip) instead of the dense table
    bool sp_mode = false;
    bool count_pending = false;  // cc_prepare_image did not wait for the colour count: U is an upper bound until cc_count_arrive (cc_finish) has run;
                                 // the caller enqueues the count's copy (sp_enqueue_count) behind the K-means launch
    KmRgbwState *km = nullptr;
    ~CcSession();
};
// occ_d (optional): summed occupancy nibbles of all ranks (occupancy_pack); the table then holds THIS image's counts
int cc_prepare(Ctx *c, uint32_t *table_counts_d, uint32_t K, const cniic_kmeans_opts *opts, uint32_t shard, uint32_t nshards,
               void *partials_dev, CcSession **out, const uint32_t *occ_d = nullptr);
// the same from the image itself, through the super-cell partition (no dense table; 16-byte aligned rgb_d)
int cc_prepare_image(Ctx *c, const uint8_t *rgb_d, uint64_t npx, uint32_t K, const cniic_kmeans_opts *opts, CcSession **out,
                     bool may_stage = true /* the persistent K-means may read the histogram's staged colours (no emit into its arrays) */);
// shared palette over several images, through the partition: begin (this image's pixels), the caller sums the occupancy of
// all ranks (sp_occupancy), create (K-means state over this image's colours placed in the list of all colours)
int cc_image_begin(Ctx *c, const uint8_t *rgb_d, uint64_t npx, CcSession **out);
int cc_image_create(CcSession *s, const uint32_t *occ_d, uint32_t K, const cniic_kmeans_opts *opts, void *partials_dev);
int cc_finish(CcSession *s, const uint8_t *rgb_d, uint32_t w, uint32_t h, const uint32_t *local_counts_d, uint8_t *out,
              uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats);
// a batch of F frames coded with the session's one palette: F Hufman streams, stream f at out + f * stride, its length in lens[f]
int cc_finish_frames(CcSession *s, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t F, uint8_t *out, uint64_t stride, uint64_t *lens,
                     cniic_kmeans_stats *stats);
// the same for frames of any sizes: frame f is w[f] x h[f] (host arrays), the frames back to back in rgb_d
int cc_finish_frames_var(CcSession *s, const uint8_t *rgb_d, const uint32_t *w, const uint32_t *h, uint32_t F, uint8_t *out, uint64_t stride, uint64_t *lens,
                         cniic_kmeans_stats *stats);

// the session's centroids (K x 3 bytes) and the pixels per cluster it knows (may be null), as of its last update
int cc_palette(CcSession *s, uint8_t *centroids_h, uint64_t *pixels_h);

// A frozen palette (cniic_palette_*): K entries and the label of every one of the 2^24 colours under "nearest entry in squared integer
// distance, lowest index among equals" (k_palette.hip).  It belongs to its context and stream; nothing of a K-means is behind it.
struct Palette {
    Ctx *c = nullptr;
    uint32_t K = 0;
    bool wide = false;             // two-byte labels (K > 256)
    DevBuf table;                  // u8 / u16 [2^24]: colour key -> label
    DevBuf cent_d;                 // u32[K] 0xRRGGBB, what k_frame_trees reads
    std::vector<uint8_t> cent_h;   // K x 3 bytes, what palette_code reads
};
int palette_create(Ctx *c, const uint8_t *cent_h, uint32_t K, Palette **out);
int palette_labels(Palette *p, const uint8_t *rgb_d, uint64_t n, void *labels_d /* 16-byte aligned */);
int palette_encode_frames_var(Palette *p, const uint8_t *rgb_d, const uint32_t *w, const uint32_t *h, uint32_t F, uint8_t *out, uint64_t stride, uint64_t *lens);
int palette_fit_frames_var(Palette *p, const uint8_t *rgb_d, const uint32_t *w, const uint32_t *h, uint32_t F, uint64_t *sse_h, uint64_t *pixels_h /* K entries, or null */);

// header carries any prefix already serialised (image dimensions); the decoder trie is appended
// to it and the whole stream lands in out[0..*len)  (out: host or device memory).
// syms_scratch: the symbol stream is ours and may be overwritten.
int huf_encode_all_dev(Ctx *c, int sym_kind, const uint8_t *rgb_d, uint32_t *syms_d, bool syms_scratch, uint64_t n, uint32_t *table_d,
                       bool have_hist, std::vector<uint8_t> &header, uint8_t *out, uint64_t cap, uint64_t *len);

}  // namespace cniic
