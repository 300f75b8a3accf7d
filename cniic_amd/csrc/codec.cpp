// codec.cpp -- host-side mirror of the reference's Codec trait (src/codec.rs:14-19) for the five
// codecs on the hot path, driving the HIP kernels.  Same names (Codec::name), same lossless flags,
// same --codec= expressions (FromStr impls), same wire format, same failure points.
//
//   Hufman          src/codec/hufc.rs        dims + huf::encode_all over row-major pixels
//   ClusterColors   src/codec/clusterc.rs:17 dedup -> K-means -> remap -> Hufman
//   VoronoiCluster  src/codec/clusterc.rs:147 5-D K-means, centroids only; Voronoi repaint on decode
//   Delta           src/codec/hilbertc.rs:404 Hilbert gather -> neighbour delta -> huf::encode_all
//   Hilbert{RLE(d)} src/codec/hilbertc.rs:12  Hilbert gather -> run-length records: exact for d == 0, else
//                                             the running average (k_rle_approx.hip): `hilbert(rle)` and `hilbert(rle(<f64>))`
//   Zip::Dict       src/codec/zipc.rs         `zip(dict)`: the dictionary coder over the serialised image (zipdict.cpp, k_zipdict.hip)
#include "codec.hpp"
#include "cc_small.hpp"
#include "vor_small.hpp"
#include "vor_paint.hpp"
#include "delta_small.hpp"
#include "delta_small_dec.hpp"
#include "huf_small.hpp"
#include "rle_small.hpp"
#include "hz_small.hpp"
#include "zd_small.hpp"
#include "zd_small_dec.hpp"
#include "small_trie.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>

#include "decode_batch_plan.hpp"
#include "huff_host.hpp"
#include "kmeans_rgbw.hpp"
#include "pal_bounds.hpp"

namespace cniic {

HostTrace &host_trace() { static thread_local HostTrace t; return t; }

// ------------------------------------------------------------------ FromStr (codec.rs:41-59)
static bool match_fun_u32(const std::string &s, const char *const *names, uint32_t *arg) {
    // Regex::captures is an unanchored search (clusterc.rs:125-127, 281-283)
    for (size_t p = 0; p < s.size(); p++)
        for (int i = 0; names[i]; i++) {
            const size_t l = strlen(names[i]);
            if (s.compare(p, l, names[i]) != 0 || p + l >= s.size() || s[p + l] != '(') continue;
            size_t q = p + l + 1;
            if (q >= s.size() || !isdigit((unsigned char)s[q])) continue;
            unsigned long long v = 0;
            bool ok = true;
            while (q < s.size() && isdigit((unsigned char)s[q])) {
                v = v * 10 + (unsigned)(s[q] - '0');
                if (v > 0xffffffffull) { ok = false; break; }
                q++;
            }
            if (!ok || q >= s.size() || s[q] != ')') continue;
            *arg = (uint32_t)v;
            return true;
        }
    return false;
}

// <f64> as Rust's f64::from_str reads it (hilbertc.rs:376): an optional sign, then `inf`, `infinity` or `nan` in any letter case, or
// decimal digits with an optional `.` and an optional e/E exponent -- at least one mantissa digit, at least one exponent digit; no
// blanks, no hex, no suffix, no nan(...).  The value is strtod's of that string: correctly rounded, out-of-range magnitudes to inf or 0.
static bool parse_rust_f64(const std::string &t, double *out) {
    size_t p = 0;
    if (p < t.size() && (t[p] == '+' || t[p] == '-')) p++;
    std::string rest = t.substr(p);
    std::transform(rest.begin(), rest.end(), rest.begin(), [](unsigned char ch) { return (char)tolower(ch); });
    if (rest != "inf" && rest != "infinity" && rest != "nan") {
        size_t q = p, digits = 0;
        while (q < t.size() && isdigit((unsigned char)t[q])) { q++; digits++; }
        if (q < t.size() && t[q] == '.') {
            q++;
            while (q < t.size() && isdigit((unsigned char)t[q])) { q++; digits++; }
        }
        if (!digits) return false;
        if (q < t.size() && (t[q] == 'e' || t[q] == 'E')) {
            q++;
            if (q < t.size() && (t[q] == '+' || t[q] == '-')) q++;
            size_t ed = 0;
            while (q < t.size() && isdigit((unsigned char)t[q])) { q++; ed++; }
            if (!ed) return false;
        }
        if (q != t.size()) return false;
    }
    *out = strtod(t.c_str(), nullptr);
    return true;
}

// Hilbert::from_str (hilbertc.rs:341-397): fun_call named ^[Hh]ilbert$ with one argument, `rle` or `rle(<f64>)`; zip is not built.
// *d: 0 for the exact method (`rle`, and d == 0.0 or -0.0: hilbertc.rs:33,82,91 compare with == 0.0), else d as written.
static bool match_hilbert_rle(const std::string &s, double *d) {
    *d = 0.0;
    if (s.compare(0, 8, "hilbert(") != 0 && s.compare(0, 8, "Hilbert(") != 0) return false;
    if (s.size() < 10 || s.back() != ')') return false;
    const std::string arg = s.substr(8, s.size() - 9);
    if (arg == "rle") return true;
    if (arg.size() > 5 && arg.compare(0, 4, "rle(") == 0 && arg.back() == ')') {
        const std::string num = arg.substr(4, arg.size() - 5);
        double v = 0.0;
        if (parse_rust_f64(num, &v)) {
            if (v != 0.0) *d = v;   // (NaN is "not zero")
            return true;
        }
        // (spellings of zero that strtod alone used to decide, a hex 0x0 or a leading blank among them, stay what they were: `hilbert(rle)`)
        char *end = nullptr;
        v = strtod(num.c_str(), &end);
        return end && *end == 0 && !num.empty() && v == 0.0;
    }
    return false;
}

bool parse_codec(const char *expr, CodecDesc *out) {
    if (!expr) return false;
    const std::string s(expr);
    // alternatives in the order of gen_all! (codec.rs:120-127); of Zip, zip(dict)
    static const char *const cc[] = {"cluster-colors", "cluster-col", "clustercolors", "clustercol",
                                     "c-colors", "c-col", "ccolors", "ccol", nullptr};  // c(?:luster)?-?col(?:ors)?
    static const char *const vo[] = {"voronoi", nullptr};
    uint32_t k = 0;
    double dv = 0.0;
    if (match_fun_u32(s, cc, &k)) { *out = {CODEC_CLUSTER_COLORS, k, 0.0}; return true; }
    if (match_fun_u32(s, vo, &k)) { *out = {CODEC_VORONOI, k, 0.0}; return true; }
    if (s == "delta") { *out = {CODEC_DELTA, 0, 0.0}; return true; }  // prs::expect_name: ^delta$
    if (match_hilbert_rle(s, &dv)) { *out = {CODEC_HILBERT_RLE, 0, dv}; return true; }
    // Zip::from_str (zipc.rs:62-80): fun_call named ^zip$ with the one argument `dict` (`back` is not built).  hilbert(zip) is reached through
    // cniic_hilbert_zip_encode / _decode, not through an expression.
    if (s == "zip(dict)") { *out = {CODEC_ZIP_DICT, 0, 0.0}; return true; }
    if (s.size() == 6) {                                         // hufc.rs:54-59 eq_ignore_ascii_case
        std::string t = s;
        std::transform(t.begin(), t.end(), t.begin(), [](unsigned char ch) { return (char)tolower(ch); });
        if (t == "hufman") { *out = {CODEC_HUFMAN, 0, 0.0}; return true; }
    }
    return false;
}

// f64's Display (format!("{}", d), hilbertc.rs:84): the shortest digits that read back as d, never an exponent; inf, -inf, NaN
std::string rust_f64_display(double d) {
    if (std::isnan(d)) return "NaN";
    if (std::isinf(d)) return d > 0 ? "inf" : "-inf";
    char buf[40];
    int prec = 1;
    for (; prec < 17; prec++) {   // (17 significant digits always read back)
        snprintf(buf, sizeof buf, "%.*e", prec - 1, d);
        if (strtod(buf, nullptr) == d) break;
    }
    snprintf(buf, sizeof buf, "%.*e", prec - 1, std::fabs(d));
    std::string digits;
    const char *q = buf;
    for (; *q && *q != 'e'; q++) if (isdigit((unsigned char)*q)) digits.push_back(*q);
    const int e10 = atoi(q + 1);   // d = digits[0] . digits[1..] x 10^e10
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int nd = (int)digits.size();
    std::string out = std::signbit(d) ? "-" : "";
    if (d == 0.0) return out + "0";
    if (e10 >= nd - 1) return out + digits + std::string((size_t)(e10 - (nd - 1)), '0');
    if (e10 >= 0) return out + digits.substr(0, (size_t)e10 + 1) + "." + digits.substr((size_t)e10 + 1);
    return out + "0." + std::string((size_t)(-e10 - 1), '0') + digits;
}

std::string codec_name(const CodecDesc &d) {
    switch (d.kind) {
    case CODEC_HUFMAN: return "Hufman";                                   // hufc.rs:42-44
    case CODEC_CLUSTER_COLORS: return "cluster-colors_" + std::to_string(d.arg);  // clusterc.rs:59-61
    case CODEC_VORONOI: return "voronoi_" + std::to_string(d.arg);        // clusterc.rs:191-193
    case CODEC_DELTA: return "delta";                                     // hilbertc.rs:433-435
    case CODEC_HILBERT_RLE: return d.darg == 0.0 ? "hilbert-rle" : "hilbert-rle-approx_" + rust_f64_display(d.darg);  // hilbertc.rs:80-86
    case CODEC_ZIP_DICT: return "zip-dict";                               // zipc.rs:50-55
    case CODEC_HILBERT_ZIP: return "hilbert-zip";                         // hilbertc.rs:80-86
    }
    return "";
}

bool codec_is_lossless(const CodecDesc &d) {   // (hilbertc.rs:88-93: RLE(d) is lossless iff d == 0.0 -- NaN is not)
    return d.kind == CODEC_HUFMAN || d.kind == CODEC_DELTA || d.kind == CODEC_ZIP_DICT || d.kind == CODEC_HILBERT_ZIP || (d.kind == CODEC_HILBERT_RLE && d.darg == 0.0);
}

// F streams at a fixed distance (cc_finish_frames): assembled where the caller wants them when that is 4-byte aligned device memory,
// otherwise in a staging buffer that is copied out once.
struct FramesOut {
    Ctx *c;
    uint8_t *out;
    uint64_t stride;
    uint32_t F;
    bool out_dev = false, direct = false;
    DevBuf staging;
    uint8_t *dev = nullptr;
    FramesOut(Ctx *ctx, uint8_t *caller, uint64_t stride_bytes, uint32_t frames) : c(ctx), out(caller), stride(stride_bytes), F(frames) {}
    int begin() {   // (zero padding behind a header = the pre-zeroed payload)
        out_dev = is_device_ptr(out);
        direct = out_dev && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
        dev = out;
        if (!direct) { CNIIC_HIP_TRY(c, staging.alloc(stride * F + 16)); dev = staging.as<uint8_t>(); }
        CNIIC_HIP_TRY(c, hipMemsetAsync(dev, 0, stride * F, c->stream));
        return CNIIC_OK;
    }
    // every stream, padded to whole words, must fit between two streams (too_long: somebody has already found one that does not)
    int check_lens(const uint64_t *lens, bool too_long = false) const {
        for (uint32_t f = 0; f < F; f++)
            if (too_long || ((lens[f] + 3) & ~3ull) > stride)
                return c->fail(CNIIC_ERR_CAPACITY, "encode: stream of frame %u is %llu bytes, %llu between streams", f, (unsigned long long)lens[f], (unsigned long long)stride);
        return CNIIC_OK;
    }
    // packed / predicted: every frame's payload bits as the pack counted them and as its histogram says
    int finish(const uint64_t *packed, const uint64_t *predicted) {
        for (uint32_t f = 0; f < F; f++)
            if (packed[f] != predicted[f])
                return c->fail(CNIIC_ERR_HIP, "cluster-colors: frame %u packed %llu bits, its histogram predicts %llu", f, (unsigned long long)packed[f], (unsigned long long)predicted[f]);
        if (!direct) {
            CNIIC_HIP_TRY(c, hipMemcpyAsync(out, dev, stride * F, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
            CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        return CNIIC_OK;
    }
};

// ------------------------------------------------------------------ the Huffman code stage: build() and the decoder (huf.rs:31-34)
// From the dense histogram's compaction to every distinct symbol's code in HBM (len_d / code_d, in the order of keys_d), the
// payload's bit count, and the serialised decoder.  A large alphabet (a photograph's colours or differences) leaves the host the
// merge of the tree at most: the leaves come back sorted by (count, key), codes and decoder are the GPU's.  A small one is built
// on the host.  The callers differ in what they enqueue, and where they wait, between the steps -- so the steps are theirs to call:
//   begin          the distinct symbols and their counts; large: the leaves sorted, and when the counts come in runs the whole
//                  tree on the GPU (tree_built); what the host's build reads starts towards pinned memory
//     (the caller waits for the stream)
//   build          large: the host's merge, the codes (huff_tree_codes), their totals start towards the host -- totals_pending:
//                  the caller waits once more before bits().  Small: tree and codes on the host.  tree_built: nothing left.
//   bits           the payload's bits
//   upload_codes   small: the host's codes to len_d / code_d (large: they are there)
//   write_decoder  the stream's header with the serialised decoder behind it, at the start of a StreamOut
struct HuffCodeStage {
    Ctx *c;
    int sym_kind;
    uint64_t U = 0;   // distinct symbols
    bool gpu_codes = false, tree_built = false, totals_pending = false;
    DevBuf keys_d, counts_d, len_d, code_d;
    HuffCodeStage(Ctx *ctx, int kind) : c(ctx), sym_kind(kind) {}
    uint64_t decoder_bytes() const { return huff_tree_bytes(sym_kind, U); }   // follows from U alone: U leaves and U - 1 branch tags

    // table_d / plan: the dense histogram after hist_compact_count; n: symbols in the stream
    int begin(uint32_t *table_d, const CompactPlan *plan, uint64_t n) {
        U = plan->n_unique;
        CNIIC_HIP_TRY(c, keys_d.alloc(U * 4));
        CNIIC_HIP_TRY(c, counts_d.alloc(U * 8));
        CNIIC_TRY(hist_compact_write(c, table_d, plan, keys_d.as<uint32_t>(), counts_d.as<uint64_t>(), nullptr));
        CNIIC_HIP_TRY(c, len_d.alloc(U));
        CNIIC_HIP_TRY(c, code_d.alloc(U * 8));
        // Counts (and codes) cross the bus through pinned memory.  From 32768 distinct symbols on -- any photograph -- the host only
        // merges the tree; codes, lengths and the serialised decoder come from the GPU (huff_tree_codes: 0.1 ms of host work less,
        // and no 0.13-0.28 ms of writing the decoder out beside the pack).  Large: [sorted leaves u64 | left, right, leaves below
        // each of the U - 1 branches u32].  Small: [counts u64 | code u64 | len u8]; the keys and the decoder in ordinary memory (the
        // host reads the keys at random and writes the decoder byte by byte: 0.20 ms in pinned memory, 0.12 there).
        gpu_codes = U >= c->opt(CNIIC_OPT_HUF_GPU_CODES_MIN, "CNIIC_HUF_GPU_CODES_MIN", 32768) && U >= 2 && U < (1ull << 30) && n < (1ull << 32);
        const uint64_t need = gpu_codes ? U * 8 + 3 * (U - 1) * 4 + 64 : U * 8 + U * 8 + U;
        CNIIC_HIP_TRY(c, c->pinned_huf.reserve(need, pinned_huf_want(need)));
        counts_h = c->pinned_huf.as<uint64_t>();
        left_h = reinterpret_cast<uint32_t *>(counts_h + U);
        right_h = left_h + (U - 1);
        nleaves_h = right_h + (U - 1);
        code_h = counts_h + U;
        len_h = reinterpret_cast<uint8_t *>(code_h + U);
        if (!gpu_codes) {
            keys_h.resize(U);
            CNIIC_HIP_TRY(c, hipMemcpyAsync(keys_h.data(), keys_d.p, U * 4, hipMemcpyDeviceToHost, c->stream));
            CNIIC_HIP_TRY(c, hipMemcpyAsync(counts_h, counts_d.p, U * 8, hipMemcpyDeviceToHost, c->stream));
            return CNIIC_OK;
        }
        uint64_t *sorted_d = nullptr;
        CNIIC_HIP_TRY(c, sort_a.alloc(U * 8));
        CNIIC_HIP_TRY(c, sort_b.alloc(U * 8));
        CNIIC_TRY(huff_sort_leaves_dev(c, counts_d.as<uint64_t>(), (uint32_t)U, plan->max_count ? plan->max_count : n, sort_a.as<uint64_t>(), sort_b.as<uint64_t>(), &sorted_d));
        // (round 3) the tree, the codes and the leaves' places in the decoder without the host's merge, when the counts come in runs
        CNIIC_HIP_TRY(c, off_d.alloc(U * 8));
        CNIIC_TRY(huff_tree_from_runs(c, sorted_d, counts_d.as<uint64_t>(), (uint32_t)U, sym_kind, len_d.as<uint8_t>(), code_d.as<uint64_t>(),
                                      off_d.as<uint64_t>(), &nbits, &tree_built));
        if (!tree_built) CNIIC_HIP_TRY(c, hipMemcpyAsync(counts_h, sorted_d, U * 8, hipMemcpyDeviceToHost, c->stream));
        if (c->timers && tree_built) c->ktimes["huf_tree_runs"].launches++;   // (stage timers: which route the tree took; no duration)
        return CNIIC_OK;
    }

    // totals_d: two u64 of the caller's in HBM (payload bits; "a code is too long"), written by huff_tree_codes
    int build(uint64_t *totals_d) {
        if (tree_built) return CNIIC_OK;
        if (!c->huf_scratch) c->huf_scratch = std::make_shared<HuffScratch>();
        HuffScratch *scratch = static_cast<HuffScratch *>(c->huf_scratch.get());
        if (!gpu_codes) {
            if (!huff_build_tree(counts_h, U, tree, scratch) || !huff_codes_into(tree, len_h, code_h)) return cannot_build();
            for (uint64_t i = 0; i < U; i++) nbits += counts_h[i] * len_h[i];
            host_trace().mark("huf: tree + codes (host)");
            return CNIIC_OK;
        }
        uint32_t root = 0;
        if (!huff_merge_sorted_into(counts_h /* sorted leaves */, U, left_h, right_h, nleaves_h, &root, scratch)) return cannot_build();
        host_trace().mark("huf: tree (host)");
        CNIIC_HIP_TRY(c, tree_d.alloc(3 * (U - 1) * 4));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(tree_d.p, left_h, 3 * (U - 1) * 4, hipMemcpyHostToDevice, c->stream));
        const uint32_t *left_d = tree_d.as<uint32_t>(), *right_d = left_d + (U - 1), *nleaves_d = right_d + (U - 1);
        CNIIC_TRY(huff_tree_codes(c, left_d, right_d, nleaves_d, counts_d.as<uint64_t>(), (uint32_t)U, root, sym_kind, len_d.as<uint8_t>(),
                                  code_d.as<uint64_t>(), off_d.as<uint64_t>(), totals_d));
        if (c->timers) c->ktimes["huf_tree_host"].launches++;   // (stage timers: the tree came from the host's merge; no duration)
        CNIIC_HIP_TRY(c, c->pinned_u.reserve(kPinnedUBytes, kPinnedUBytes));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuHufTotals.at, totals_d, 16, hipMemcpyDeviceToHost, c->stream));
        totals_pending = true;
        return CNIIC_OK;
    }

    int bits(uint64_t *payload_bits) {
        if (totals_pending) {
            totals_pending = false;
            if (c->pinned_u.as<uint64_t>()[kPuHufTotals.at + 1]) return cannot_build();
            nbits = c->pinned_u.as<uint64_t>()[kPuHufTotals.at];
            host_trace().mark("huf: codes (GPU)");
        }
        *payload_bits = nbits;
        return CNIIC_OK;
    }

    int upload_codes() {
        if (gpu_codes) return CNIIC_OK;
        CNIIC_HIP_TRY(c, hipMemcpyAsync(len_d.p, len_h, U, hipMemcpyHostToDevice, c->stream));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(code_d.p, code_h, U * 8, hipMemcpyHostToDevice, c->stream));
        return CNIIC_OK;
    }

    // header: whatever the stream starts with (the image's dimensions); so: begun for header.size() + decoder_bytes() + the payload.
    // Small alphabet: the decoder is appended to `header` on the host.
    int write_decoder(StreamOut &so, std::vector<uint8_t> &header) {
        const uint64_t head = header.size();
        if (!gpu_codes) huff_serialize_tree(tree, sym_kind, keys_h.data(), header);
        CNIIC_TRY(so.put_header(header));
        if (gpu_codes) CNIIC_TRY(huff_tree_serialize_dev(c, keys_d.as<uint32_t>(), off_d.as<uint64_t>(), (uint32_t)U, sym_kind, so.dev + head, decoder_bytes()));
        host_trace().mark("huf: serialise trie");
        return CNIIC_OK;
    }

    void release_tree() { tree_d.release(); off_d.release(); }   // (once the stream has been waited for behind write_decoder)

private:
    DevBuf sort_a, sort_b, tree_d, off_d;   // off_d: every leaf's place in the serialised decoder
    uint64_t nbits = 0;
    uint64_t *counts_h = nullptr, *code_h = nullptr;
    uint32_t *left_h = nullptr, *right_h = nullptr, *nleaves_h = nullptr;
    uint8_t *len_h = nullptr;
    std::vector<uint32_t> keys_h;
    HuffTree tree;
    int cannot_build() { return c->fail(CNIIC_ERR_BAD_ARG, "huffman: cannot build code (alphabet %llu)", (unsigned long long)U); }
};

// ------------------------------------------------------------------ huf::encode_all (huf.rs:22-43)
// Symbols come either as pixels (rgb_d) or as packed keys (syms_d).  table_d holds the dense
// histogram on entry when have_hist, otherwise it is built here.
int huf_encode_all_dev(Ctx *c, int sym_kind, const uint8_t *rgb_d, uint32_t *syms_d, bool syms_scratch, uint64_t n,
                       uint32_t *table_d, bool have_hist, std::vector<uint8_t> &header, uint8_t *out, uint64_t cap,
                       uint64_t *len) {
    if (n == 0) return c->fail(CNIIC_ERR_BAD_ARG, "huf::encode_all on an empty stream (src/huf.rs:99 asserts)");
    const uint32_t bits = sym_kind == CNIIC_SYM_RGB ? 24 : 27;
    host_trace().mark("huf: enter");
    // 1. utils::count_freqs (huf.rs:30)
    if (!have_hist) {
        if (rgb_d) CNIIC_TRY(hist_rgb_dense(c, rgb_d, n, table_d));
        else CNIIC_TRY(hist_syms_dense(c, syms_d, n, table_d, bits));
    }
    CompactPlan plan;
    CNIIC_TRY(hist_compact_count(c, table_d, bits, &plan));
    HuffCodeStage st(c, sym_kind);
    CNIIC_TRY(st.begin(table_d, &plan, n));
    const uint64_t U = st.U;
    CNIIC_HIP_TRY(c, c->huf_ev.ensure(hipEventDisableTiming));
    CNIIC_HIP_TRY(c, hipEventRecord(c->huf_ev, c->stream));
    // `delta` symbols on a buffer of ours: nothing to do while the host builds the tree -- the pack looks (length, code) up
    // in an LDS table of the cube of small differences (huff_pack_code32_hot).  Otherwise the GPU meanwhile turns every
    // symbol into its rank in the compacted list -- the one random read per symbol into the dense table (it now holds
    // rank + 1), which needs no code -- in place over the symbol stream when it is ours; the pack then reads that stream
    // and the small per-rank length / code tables.
    const bool hot_route = sym_kind == CNIIC_SYM_SIGNED && syms_d && syms_scratch && U < (1ull << 26) && (reinterpret_cast<uintptr_t>(syms_d) & 15) == 0;
    DevBuf ranks_own, totals_d;
    uint32_t *ranks = syms_d;
    const bool inline_codes = U < (1ull << 26);  // (len, code) of a symbol in one u32 looked up by rank; else per-rank tables
    // (round 3) with the tree on the GPU there is nothing for that pass to hide behind: the pack's first pass looks every symbol up in the
    // dense table itself, once it holds (length, code) words -- one random read per symbol instead of two (hufman 4096^2: -0.25 ms)
    const bool direct = st.gpu_codes && !hot_route && inline_codes;
    if (!hot_route) {
        if (!syms_d || !syms_scratch) { CNIIC_HIP_TRY(c, ranks_own.alloc(n * 4 + 16)); ranks = ranks_own.as<uint32_t>(); }
        if (!direct) CNIIC_TRY(huff_rank_stream(c, syms_d, rgb_d, n, table_d, ranks, !inline_codes));
    }
    CNIIC_HIP_TRY(c, hipEventSynchronize(c->huf_ev));
    host_trace().mark("huf: hist + compaction + D2H");
    // 2. build() (huf.rs:31)
    CNIIC_HIP_TRY(c, totals_d.alloc(16));
    CNIIC_TRY(st.build(totals_d.as<uint64_t>()));
    if (st.totals_pending) CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t nbits = 0;
    CNIIC_TRY(st.bits(&nbits));
    // 3. the serialised decoder (huf.rs:34); the payload (huf.rs:37-41) is packed in place behind it
    const uint64_t header_bytes = header.size() + st.decoder_bytes();
    StreamOut so(c, out, cap, len);
    CNIIC_TRY(so.begin_sized(header_bytes, (nbits + 7) / 8));
    CNIIC_TRY(st.write_decoder(so, header));
    CNIIC_TRY(st.upload_codes());
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the stage's tree goes back to the pool before the pack asks it for memory
    st.release_tree();
    uint64_t packed_bits = 0;
    ScopedKernelTimer timer(c, "huff_pack");
    uint32_t *const keys_d = st.keys_d.as<uint32_t>();
    const uint8_t *const len_d = st.len_d.as<uint8_t>();
    const uint64_t *const code_d = st.code_d.as<uint64_t>();
    if (hot_route) {
        CNIIC_TRY(huff_pack_code32_hot(c, syms_d, n, table_d, keys_d, len_d, code_d, U, syms_d, so.dev, header_bytes * 8, &packed_bits));
    } else if (direct) {
        CNIIC_TRY(huff_pack_code32(c, syms_d, rgb_d, n, table_d, keys_d, len_d, code_d, U, ranks, so.dev, header_bytes * 8, &packed_bits));
    } else if (inline_codes) {
        DevBuf code32;
        CNIIC_HIP_TRY(c, code32.alloc(U * 4));
        CNIIC_TRY(huff_pack_code32(c, ranks, nullptr, n, code32.as<uint32_t>(), nullptr, len_d, code_d, U, ranks, so.dev, header_bytes * 8, &packed_bits));
    } else {
        CNIIC_TRY(huff_pack_ranks(c, ranks, n, len_d, code_d, so.dev, header_bytes * 8, &packed_bits));
    }
    timer.stop(1);
    host_trace().mark("huf: pack");
    if (packed_bits != nbits)
        return c->fail(CNIIC_ERR_HIP, "huffman: packed %llu bits, histogram predicts %llu", (unsigned long long)packed_bits,
                       (unsigned long long)nbits);
    const int rc_fin = so.finish();
    host_trace().mark("huf: finish");
    host_trace().dump();
    return rc_fin;
}

// ------------------------------------------------------------------ Hufman::encode (hufc.rs:12-17)
static int encode_hufman(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    const uint64_t n = (uint64_t)w * h;
    std::vector<uint8_t> header;
    put_u32(header, w);  // img.dimensions().serialize (hufc.rs:13)
    put_u32(header, h);
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, 24, &table));
    return huf_encode_all_dev(c, CNIIC_SYM_RGB, rgb_d, nullptr, false, n, table, false, header, out, cap, len);
}

// ------------------------------------------------------------------ ClusterColors::encode (clusterc.rs:18-53)
// Split in two so that a multi-GPU caller can all-reduce between the pieces:
//   cc_prepare  dense colour counts -> distinct colours (ascending key = point order, clusterc.rs:21-24)
//               + K-means state (kmeans::init, kmeans.rs:80-90)
//   (K-means loop: km_rgbw_run on one GPU, or assign / all-reduce / update driven by the caller)
//   cc_finish   clusters -> colour lookup -> Hufman.encode of the reduced image (clusterc.rs:31-52)
CcSession::~CcSession() { if (km) km_rgbw_destroy(km); }

int cc_prepare(Ctx *c, uint32_t *table_counts_d, uint32_t K, const cniic_kmeans_opts *opts, uint32_t shard, uint32_t nshards,
               void *partials_dev, CcSession **out, const uint32_t *occ_d) {
    if (K == 0) return c->fail(CNIIC_ERR_BAD_ARG, "cluster-colors(0)");
    auto s = std::make_unique<CcSession>();
    s->c = c; s->K = K; s->table = table_counts_d;
    s->counts_local = occ_d != nullptr || nshards == 1;
    CompactPlan plan;
    DevBuf cell_count;  // occupied bins per K-means colour cell, counted by the compaction on its way
    CNIIC_HIP_TRY(c, cell_count.alloc((uint64_t)kNumCells * 4));
    CNIIC_HIP_TRY(c, hipMemsetAsync(cell_count.p, 0, (uint64_t)kNumCells * 4, c->stream));
    CNIIC_TRY(hist_compact_count(c, table_counts_d, 24, &plan, cell_count.as<uint32_t>()));
    host_trace().mark("compact_count+sync");
    const uint64_t U = plan.n_unique;
    s->U = U;
    uint64_t Ug = 0;
    if (occ_d) {  // the reference's point list is the union's; this rank holds its own share of it
        CNIIC_TRY(gidx_build(c, occ_d, s->gbits, s->gprefix, &Ug));
        s->local_points = true;
    }
    if ((occ_d ? Ug : U) / K == 0 || U == 0)
        return c->fail(CNIIC_ERR_TOO_FEW_POINTS, "kmeans: %llu distinct colours for %u clusters (src/kmeans.rs:68)",
                       (unsigned long long)(occ_d ? Ug : U), K);
    CNIIC_HIP_TRY(c, s->keys_d.alloc(U * 4));
    CNIIC_HIP_TRY(c, s->weight_d.alloc(U * 4));
    CNIIC_TRY(hist_compact_write(c, table_counts_d, &plan, s->keys_d.as<uint32_t>(), nullptr, s->weight_d.as<uint32_t>()));
    host_trace().mark("compact_write enq");
    // kmeans::cluster (clusterc.rs:28); the table now maps key -> rank + 1
    CNIIC_TRY(km_rgbw_create(c, s->keys_d.as<uint32_t>(), s->weight_d.as<uint32_t>(), U, shard, nshards, K, opts, partials_dev,
                             table_counts_d, &s->km, cell_count.as<uint32_t>(), occ_d ? s->gbits.p : nullptr,
                             occ_d ? s->gprefix.as<uint32_t>() : nullptr, Ug));
    host_trace().mark("km_create");
    *out = s.release();
    return CNIIC_OK;
}

int cc_prepare_image(Ctx *c, const uint8_t *rgb_d, uint64_t npx, uint32_t K, const cniic_kmeans_opts *opts, CcSession **out, bool may_stage) {
    if (K == 0) return c->fail(CNIIC_ERR_BAD_ARG, "cluster-colors(0)");
    auto s = std::make_unique<CcSession>();
    s->c = c; s->K = K; s->sp_mode = true;
    CNIIC_TRY(sp_build(c, rgb_d, npx, &s->sp, true));   // count_freqs (clusterc.rs:21): distinct colours per cell, occupancy bitmap (its prefix: below)
    // kmeans::cluster (clusterc.rs:28): the point list is known as the bitmap and its cell-major copy is written below.
    // The number of distinct colours is still on the device: the state is sized for the most there can be, its
    // set-up kernels read the count there, and the host only waits for it after all of them are enqueued.
    // The state enqueues nothing itself: what it would, the rest of sp_build and the emit into its arrays are three launches (sp_front).
    const uint64_t Umax = std::min<uint64_t>(npx, 1ull << 24);
    const uint64_t *U_dev = s->sp.total.as<uint64_t>();
    KmFront front;
    CNIIC_TRY(km_rgbw_create_deferred(c, Umax, K, opts, &s->km, s->sp.cell_count.as<uint32_t>(), s->sp.bits.p, s->sp.wprefix.as<uint32_t>(), Umax, U_dev, &front));
    uint32_t *cell_start, *ckeys, *cweight;
    km_rgbw_cell_arrays(s->km, &cell_start, &ckeys, &cweight);
    // (tests: CNIIC_TEST_CC_FRONT=split enqueues the dispatches one by one; =require makes a silent fall-back to them an error)
    bool fused = sp_front_fits(front);
    if (const char *e = test_env("CNIIC_TEST_CC_FRONT")) {
        if (!fused && !strcmp(e, "require")) return c->fail(CNIIC_ERR_HIP, "cluster-colors: the fused set-up launches cannot clear the K-means arenas (CNIIC_TEST_CC_FRONT=require)");
        fused = fused && strcmp(e, "split") != 0;
    }
    // With a persistent launch to come (narrow labels, this context's own CUs, no back-off) the distinct colours stay where the histogram
    // staged them: the launch's set-up and the pixel labels read them there, and the emit into the K-means arrays runs only if somebody
    // turns out to need the arrays (km_rgbw_need_arrays: the loop of launches behind a launch that gave up).
    // (tests: CNIIC_TEST_CC_POINTS=arrays always emits; =require makes it an error when an encode that could have left the emit out emits)
    bool staged = may_stage && fused && front.ranges;
    if (const char *e = test_env("CNIIC_TEST_CC_POINTS")) {
        if (!staged && may_stage && K <= 256 && !strcmp(e, "require"))
            return c->fail(CNIIC_ERR_HIP, "cluster-colors: the K-means would read its points from the arrays (CNIIC_TEST_CC_POINTS=require)");
        staged = staged && strcmp(e, "arrays") != 0;
    }
    if (staged) km_rgbw_points_from_staging(s->km, &s->sp, &front);
    if (c->timers && staged) c->ktimes["cc_points_staged"].launches++;   // (stage timers: which route the call took; no duration)
    if (staged) front.ptrs.count_dev = U_dev;
    CNIIC_TRY(sp_front(c, &s->sp, front, ckeys, cweight, km_rgbw_labels_internal(s->km, nullptr), km_rgbw_is_wide(s->km), fused, !staged, !staged));
    if (staged) {
        // ... and nothing waits for the count either: the launch reads it where it lies (fewer colours than clusters: every block leaves
        // at once), its copy to the host is enqueued BEHIND the launch (encode_cluster_colors) and looked at where the result is fetched
        // (cc_finish: cc_count_arrive).  Until then U is the upper bound everything here is sized by.
        s->U = Umax;
        s->count_pending = true;
        km_rgbw_count_stays_on_device(s->km, U_dev);
        host_trace().mark("km_create + front enq");
        *out = s.release();
        return CNIIC_OK;
    }
    CNIIC_TRY(sp_wait_count(c, &s->sp));
    s->U = s->sp.U;
    if (s->U / K == 0)
        return c->fail(CNIIC_ERR_TOO_FEW_POINTS, "kmeans: %llu distinct colours for %u clusters (src/kmeans.rs:68)", (unsigned long long)s->U, K);
    CNIIC_TRY(km_rgbw_set_points(s->km, s->U));
    host_trace().mark("km_create + emit enq");
    *out = s.release();
    return CNIIC_OK;
}

int cc_image_begin(Ctx *c, const uint8_t *rgb_d, uint64_t npx, CcSession **out) {
    auto s = std::make_unique<CcSession>();
    s->c = c; s->sp_mode = true; s->local_points = true;
    CNIIC_TRY(sp_build(c, rgb_d, npx, &s->sp));
    *out = s.release();
    return CNIIC_OK;
}

int cc_image_create(CcSession *s, const uint32_t *occ_d, uint32_t K, const cniic_kmeans_opts *opts, void *partials_dev) {
    Ctx *c = s->c;
    if (!s->sp_mode || s->km) return c->fail(CNIIC_ERR_BAD_ARG, "cc_image_create: needs a session from cc_image_begin, once");
    if (K == 0) return c->fail(CNIIC_ERR_BAD_ARG, "cluster-colors(0)");
    s->K = K;
    // The reference's point list is the colours of ALL images: the summed occupancy as a bitmap + prefix.  Its length (and
    // this image's own colour count) stay on the device while the state is set up -- sized for the most there can be, the
    // set-up kernels read the counts where they are -- and the host fetches both once everything is enqueued.
    CNIIC_HIP_TRY(c, c->pinned_u.reserve(kPinnedUBytes, kPinnedUBytes));
    uint64_t *Ug_h = c->pinned_u.as<uint64_t>() + kPuPointCount.at;
    CNIIC_TRY(gidx_build(c, occ_d, s->gbits, s->gprefix, Ug_h, &s->gtotal));
    const uint64_t Umax = std::min<uint64_t>(s->sp.npx, 1ull << 24);
    const uint64_t *Ug_dev = s->gtotal.as<uint64_t>();
    CNIIC_TRY(km_rgbw_create(c, nullptr, nullptr, Umax, 0, 1, K, opts, partials_dev, nullptr, &s->km, s->sp.cell_count.as<uint32_t>(), s->gbits.p,
                             s->gprefix.as<uint32_t>(), 1ull << 24, true, Ug_dev));
    uint32_t *cell_start, *ckeys, *cweight;
    km_rgbw_cell_arrays(s->km, &cell_start, &ckeys, &cweight);
    CNIIC_TRY(sp_emit(c, &s->sp, cell_start, ckeys, cweight, km_rgbw_labels_internal(s->km, nullptr), km_rgbw_is_wide(s->km), K, s->gbits.p,
                      s->gprefix.as<uint32_t>(), 0, Ug_dev));
    // this image's own colour count, fetched again here: the word sp_build copied it to (kPuSpCount) may have been
    // rewritten since by another session of the same context (a second cniic_cc_image_begin, a plain encode)
    CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuImageCount.at, s->sp.total.p, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the all-reduced occupancy had to arrive anyway)
    const uint64_t Ug = *Ug_h;
    s->sp.U = c->pinned_u.as<uint64_t>()[kPuImageCount.at];
    s->U = s->sp.U;
    if (Ug / K == 0 || s->U == 0)
        return c->fail(CNIIC_ERR_TOO_FEW_POINTS, "kmeans: %llu distinct colours for %u clusters (src/kmeans.rs:68)", (unsigned long long)Ug, K);
    return km_rgbw_set_points(s->km, s->U, Ug);
}

// The Hufman stream of a colour-reduced image, from its palette (clusterc.rs:52 -> hufc.rs:12-17).  The histogram count_freqs would
// find there (huf.rs:30) is the image's pixels per centroid COLOUR -- two clusters with one mean are one symbol; from it the tree,
// the stream's header (dimensions + serialised decoder), the payload's bits and every cluster's code: reduced_colors.get(original
// colour) (clusterc.rs:43-47) fused with Enc::encode (huf.rs:137-148).  cent: K centroids, 3 bytes each; pixels[k]: this image's
// pixels in cluster k (a cluster without any gets no code); clen / ccode: K entries.  false: no code can be built.
template <class Count>
static bool palette_code(const uint8_t *cent, const Count *pixels, uint32_t K, uint32_t w, uint32_t h, std::vector<uint8_t> &header,
                         uint8_t *clen, uint64_t *ccode, uint64_t *nbits) {
    auto colour = [&](uint32_t k) { return ((uint32_t)cent[3 * k] << 16) | ((uint32_t)cent[3 * k + 1] << 8) | cent[3 * k + 2]; };
    std::vector<std::pair<uint32_t, uint64_t>> kc;
    kc.reserve(K);
    for (uint32_t k = 0; k < K; k++)
        if (pixels[k]) kc.emplace_back(colour(k), pixels[k]);
    std::sort(kc.begin(), kc.end());  // ascending colour, equal colours adjacent
    std::vector<uint32_t> skeys;
    std::vector<uint64_t> scounts;
    for (auto &e : kc) {
        if (!skeys.empty() && skeys.back() == e.first) scounts.back() += e.second;
        else { skeys.push_back(e.first); scounts.push_back(e.second); }
    }
    HuffTree tree;
    std::vector<uint8_t> slen;
    std::vector<uint64_t> scode;
    if (!huff_build_tree(scounts.data(), scounts.size(), tree) || !huff_codes(tree, slen, scode)) return false;
    put_u32(header, w);
    put_u32(header, h);
    huff_serialize_tree(tree, CNIIC_SYM_RGB, skeys.data(), header);
    *nbits = 0;
    for (size_t i = 0; i < scounts.size(); i++) *nbits += scounts[i] * slen[i];
    for (uint32_t k = 0; k < K; k++) {
        const size_t si = std::lower_bound(skeys.begin(), skeys.end(), colour(k)) - skeys.begin();
        clen[k] = pixels[k] ? slen[si] : 0;
        ccode[k] = pixels[k] ? scode[si] : 0;
    }
    return true;
}

// a session whose colour count was left on the device (cc_prepare_image): the count's copy has been enqueued behind the K-means launch --
// wait for it, refuse fewer colours than clusters as cc_prepare_image does, and tell the state
static int cc_count_arrive(CcSession *s) {
    if (!s->count_pending) return CNIIC_OK;
    Ctx *c = s->c;
    s->count_pending = false;
    CNIIC_TRY(sp_wait_count(c, &s->sp));
    s->U = s->sp.U;
    if (s->U / s->K == 0)
        return c->fail(CNIIC_ERR_TOO_FEW_POINTS, "kmeans: %llu distinct colours for %u clusters (src/kmeans.rs:68)", (unsigned long long)s->U, s->K);
    return km_rgbw_set_points(s->km, s->U);
}

int cc_finish(CcSession *s, const uint8_t *rgb_d, uint32_t w, uint32_t h, const uint32_t *local_counts_d, uint8_t *out,
              uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats) {
    Ctx *c = s->c;
    const uint32_t K = s->K;
    uint64_t U = s->U;   // (an upper bound while the count is on its way: cc_count_arrive below)
    const uint64_t n = (uint64_t)w * h;
    KmRgbwState *km = s->km;
    std::vector<uint8_t> cent(3 * (size_t)K);
    std::vector<uint64_t> members(K), wsum(K);
    cniic_kmeans_stats st{};
    // The result block starts towards the host; behind it goes everything that needs no code table - the
    // colour -> label table and the label of every pixel (the one random read per pixel) - so that the GPU
    // is busy while the host waits for the block and builds the tree.
    const bool wide = km_rgbw_is_wide(km);
    // Narrow labels from the partition: the pixels' labels are never written out -- the kernel that picks them packs them
    // (k_sp_pixpack, k_points.hip), so only the labels in partition order need no code table and run under the host's wait.
    bool fused = s->sp_mode && !wide;
    if (const char *e = test_env("CNIIC_TEST_CC_TAIL")) fused = fused && strcmp(e, "split") != 0;
    DevBuf lab_d, key2label, pixlab, partlab, look;
    if (!fused) CNIIC_HIP_TRY(c, pixlab.alloc(n * (wide ? 2 : 1) + 16));
    DevBuf lw;
    bool lw_early = false;
    // (twice only if a persistent K-means launch that nobody had waited for turns out to have given up: km_rgbw_result_end has run the
    // launch-per-iteration loop by then and answers kKmRetry -- what was enqueued on the labels is enqueued again)
    for (int attempt = 0;; attempt++) {
    CNIIC_TRY(km_rgbw_result_begin(km));
    if (s->sp_mode) {  // every pixel's label from the partition: no table of 2^24 entries, no random read
        uint32_t *cell_start, *ckeys, *cweight;
        km_rgbw_cell_arrays(km, &cell_start, &ckeys, &cweight);
        if (s->local_points) CNIIC_TRY(km_rgbw_need_arrays(km));   // (the shared palette's sessions always have them: cc_image_create emits)
        if (s->local_points && K <= kPuPaletteWeights.words) {
            // shared palette: THIS image's pixels per cluster (below) -- asked for first, so that the answer travels while
            // the pixel labels are computed instead of stalling the stream after them
            CNIIC_HIP_TRY(c, c->pinned_u.reserve(kPinnedUBytes, kPinnedUBytes));
            CNIIC_HIP_TRY(c, lw.alloc((uint64_t)K * 8));
            CNIIC_HIP_TRY(c, hipMemsetAsync(lw.p, 0, (uint64_t)K * 8, c->stream));
            CNIIC_TRY(local_cluster_weights(c, ckeys, km_rgbw_labels_internal(km, nullptr), wide, U, nullptr, K, lw.as<uint64_t>(), cweight));
            CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuPaletteWeights.at, lw.p, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
            CNIIC_HIP_TRY(c, c->u_ev.ensure(hipEventDisableTiming));
            CNIIC_HIP_TRY(c, hipEventRecord(c->u_ev, c->stream));
            lw_early = true;
        }
        // (a state whose arrays were not emitted: the partition's colours come from the staging, as its points did; behind a launch that
        // gave up the arrays are there on the second attempt)
        const bool staged = km_rgbw_arrays_pending(km);
        if (fused) CNIIC_TRY(sp_part_labels(c, &s->sp, cell_start, ckeys, km_rgbw_labels_internal(km, nullptr), wide, partlab, &look, staged));
        else {
            DevBuf pl;
            CNIIC_TRY(sp_part_labels(c, &s->sp, cell_start, ckeys, km_rgbw_labels_internal(km, nullptr), wide, pl, nullptr, staged));
            CNIIC_TRY(sp_pixlab(c, &s->sp, rgb_d, pl.p, wide, pixlab.p));
        }
    } else {
        CNIIC_HIP_TRY(c, lab_d.alloc(U * (wide ? 2 : 1)));
        CNIIC_TRY(km_rgbw_labels_canonical(km, lab_d.p));
        CNIIC_HIP_TRY(c, key2label.alloc((1ull << 24) * (wide ? 2 : 1)));
        CNIIC_TRY(scatter_labels_by_key(c, s->keys_d.as<uint32_t>(), lab_d.p, wide, U, key2label.p));
        CNIIC_TRY(pixel_labels(c, rgb_d, n, key2label.p, wide, pixlab.p));
    }
    host_trace().mark("labels + pixel labels enq");
    CNIIC_TRY(cc_count_arrive(s));   // (the count's copy lies in the stream in front of the result block's: no wait of its own)
    U = s->U;
    const int rc_res = km_rgbw_result_end(km, cent.data(), members.data(), wsum.data(), &st);
    if (rc_res == kKmRetry && attempt == 0) continue;
    CNIIC_TRY(rc_res);
    break;
    }
    host_trace().mark("km_result");
    if (stats) *stats = st;
    CNIIC_TRY(check_enough_active(c, K, U, st.active));
    // wsum: the pixels per cluster of the image Hufman.encode sees (clusterc.rs:52).  One image: the member weights' sums, as they came.
    if (lw_early) {
        CNIIC_HIP_TRY(c, hipEventSynchronize(c->u_ev));
        for (uint32_t k = 0; k < K; k++) wsum[k] = c->pinned_u.as<uint64_t>()[kPuPaletteWeights.at + k];
    } else if (local_counts_d || s->local_points) {
        // shared palette over several images: THIS image's pixels per cluster, from its own colour counts
        CNIIC_HIP_TRY(c, lw.alloc((uint64_t)K * 8));
        CNIIC_HIP_TRY(c, hipMemsetAsync(lw.p, 0, (uint64_t)K * 8, c->stream));
        if (s->sp_mode) {  // cell-major colours, labels and pixel counts of this image: any common order will do
            uint32_t *cell_start, *ckeys, *cweight;
            km_rgbw_cell_arrays(km, &cell_start, &ckeys, &cweight);
            CNIIC_TRY(km_rgbw_need_arrays(km));
            CNIIC_TRY(local_cluster_weights(c, ckeys, km_rgbw_labels_internal(km, nullptr), wide, U, nullptr, K, lw.as<uint64_t>(), cweight));
        } else {
            CNIIC_TRY(local_cluster_weights(c, s->keys_d.as<uint32_t>(), lab_d.p, wide, U, local_counts_d, K, lw.as<uint64_t>(),
                                            s->weight_d.as<uint32_t>()));
        }
        CNIIC_HIP_TRY(c, hipMemcpyAsync(wsum.data(), lw.p, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    std::vector<uint8_t> header, clen(K);
    std::vector<uint64_t> ccode(K);
    uint64_t nbits = 0;
    if (!palette_code(cent.data(), wsum.data(), K, w, h, header, clen.data(), ccode.data(), &nbits))
        return c->fail(CNIIC_ERR_BAD_ARG, "huffman: cannot build code");
    host_trace().mark("tree+codes (host)");
    StreamOut so(c, out, cap, len);
    uint64_t packed_bits = 0;
    if (fused && header.size() <= kCcUpBytes - kCcUpHdr) {
        static_assert(kPuCcUpload.words * 8 == kCcUpBytes && kCcUpHdr >= kCcUpHdrBytes + 4 && kCcUpHdrBytes >= kCcUpLen + 256 && kCcUpLen >= kCcUpCode + 256 * 8, "the upload block's layout");
        CNIIC_TRY(so.begin_sized(header.size(), (nbits + 7) / 8));   // (the capacity check; the stream's bytes cleared)
        host_trace().mark("so.begin");
        // codes, lengths and header in one pinned block that the kernel reads where it lies (three pageable uploads before); its chunk 0
        // puts the header in front of the payload
        CNIIC_HIP_TRY(c, c->pinned_u.reserve(kPinnedUBytes, kPinnedUBytes));
        uint8_t *up = reinterpret_cast<uint8_t *>(c->pinned_u.as<uint64_t>() + kPuCcUpload.at);
        const uint32_t hb = (uint32_t)header.size();
        const size_t up_bytes = (kCcUpHdr + (size_t)hb + 3) & ~(size_t)3;
        memset(up, 0, up_bytes);
        memcpy(up + kCcUpCode, ccode.data(), (size_t)K * 8);
        memcpy(up + kCcUpLen, clen.data(), K);
        memcpy(up + kCcUpHdrBytes, &hb, 4);
        memcpy(up + kCcUpHdr, header.data(), hb);
        uint64_t *done = c->pinned_u.as<uint64_t>() + kPuCcPacked.at;
        {
            ScopedKernelTimer t(c, "huff_pack");
            CNIIC_TRY(sp_pixpack(c, &s->sp, partlab.p, look, up, hb, so.dev, done));
            host_trace().mark("pixpack enq");
            CNIIC_HIP_TRY(c, ctx_spin_sync(c));
            t.stop(1);
        }
        host_trace().mark("pack (+sync)");
        // a block that gave the look-back up (its wait ran out): the stream is incomplete -- the split kernels below, from the same partlab
        if (done[0]) fused = false;
        else packed_bits = done[1];
    } else {
        fused = false;
    }
    if (!fused) {
    // (tests: CNIIC_TEST_CC_TAIL=require makes the silent hand-over an error, as CNIIC_KM_PS_REQUIRE does for the persistent K-means)
    if (const char *e = test_env("CNIIC_TEST_CC_TAIL"))
        if (!strcmp(e, "require")) return c->fail(CNIIC_ERR_HIP, "cluster-colors: the fused pick-and-pack did not produce the stream (CNIIC_TEST_CC_TAIL=require)");
    if (partlab.p) {   // (the labels in partition order are there, the pixels' are not)
        CNIIC_HIP_TRY(c, pixlab.alloc(n + 16));
        CNIIC_TRY(sp_pixlab(c, &s->sp, rgb_d, partlab.p, wide, pixlab.p));
    }
    CNIIC_TRY(so.begin(header, (nbits + 7) / 8));
    host_trace().mark("so.begin");
    DevBuf clen_d, ccode_d;
    CNIIC_HIP_TRY(c, clen_d.alloc(K));
    CNIIC_HIP_TRY(c, ccode_d.alloc((uint64_t)K * 8));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(clen_d.p, clen.data(), K, hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(ccode_d.p, ccode.data(), (size_t)K * 8, hipMemcpyHostToDevice, c->stream));
    {
        ScopedKernelTimer t(c, "huff_pack");
        CNIIC_TRY(huff_pack_labels(c, pixlab.p, n, wide, K, clen_d.as<uint8_t>(), ccode_d.as<uint64_t>(), so.dev,
                                   (uint64_t)header.size() * 8, &packed_bits));
        t.stop(1);
    }
    host_trace().mark("pack (+sync)");
    }
    if (packed_bits != nbits)
        return c->fail(CNIIC_ERR_HIP, "cluster-colors: packed %llu bits, histogram predicts %llu",
                       (unsigned long long)packed_bits, (unsigned long long)nbits);
    const int rc_fin = so.finish();
    host_trace().mark("so.finish");
    return rc_fin;
}

// ---- the frames of a batch, as everything behind "every pixel has a label" needs them: F equally sized frames of w x h (wv == nullptr), or
// frame f of wv[f] x hv[f] with the table the kernels of the var route read (FrameVar, common.hpp).
struct FrameBatch {
    uint32_t w = 0, h = 0;                       // equally sized frames
    const uint32_t *wv = nullptr, *hv = nullptr;   // frames of any sizes (host arrays)
    uint32_t F = 0;
    std::vector<FrameVar> ft;
    DevBuf ft_d;
    uint64_t lab_total = 0;      // elements of the aligned label buffer
    uint32_t chunks = 0, hblocks = 0;
    bool runs_aligned = true;
    bool var() const { return wv != nullptr; }
    // frames of any sizes: the frame table.  Label bases on 16-byte boundaries (16 elements, for labels of either width); when every
    // run already starts on one where the pixel-label kernels write it, the bases are those and nothing is copied
    int build_table(Ctx *c, const char *who, uint64_t lb) {
        ft.resize(F);
        uint64_t src = 0, ch = 0, hb = 0;
        for (uint32_t f = 0; f < F; f++) {
            const uint64_t np = (uint64_t)wv[f] * hv[f];
            if ((src * lb) & 15) runs_aligned = false;
            ft[f] = FrameVar{np, lab_total, src, (uint32_t)ch, (uint32_t)hb, wv[f], hv[f]};
            src += np;
            lab_total += (np + 15) & ~15ull;
            ch += ceil_div(np, kFrameVarChunk);
            hb += ceil_div(np, kFrameVarHistSpan);
            if (ch > 0x7fffffffull) return c->fail(CNIIC_ERR_BAD_ARG, "%s: too many pixels for one batch", who);
        }
        chunks = (uint32_t)ch;
        hblocks = (uint32_t)hb;
        if (runs_aligned)
            for (uint32_t f = 0; f < F; f++) ft[f].lab_base = ft[f].src_base;
        return CNIIC_OK;
    }
    int upload_table(Ctx *c) {
        CNIIC_HIP_TRY(c, ft_d.alloc((uint64_t)F * sizeof(FrameVar)));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(ft_d.p, ft.data(), (size_t)F * sizeof(FrameVar), hipMemcpyHostToDevice, c->stream));
        return CNIIC_OK;
    }
};

// From the labels of every pixel of a batch (pixlab_d: the frames' labels back to back, as the pixel-label kernels write them) to the F
// streams at out + f * stride: per-frame label histograms, the frames' trees (k_frame_trees reading cent_d, the K palette entries as
// 0xRRGGBB words -- or palette_code on host threads reading cent_h, K x 3 bytes), the lengths held against the stride, the label pack.
// The two callers are a K-means session's finish_frames and a frozen palette's palette_encode_frames_var.  after_hist (optional) runs
// once the histograms are enqueued and before the host waits for them: a session collects its K-means result there -- which is when
// cent_h is filled in; nobody reads it earlier.  headers_aside: CNIIC_ERR_CAPACITY leaves `out` untouched on the k_frame_trees route as well (a
// session's calls write the headers in place and refuse afterwards, as they always have).  pal_stride: 0 = the one palette at cent_d / cent_h
// for every frame; K = a palette per frame, frame f's entries at cent_d + f K (cent_h + 3 f K): the small-frame route of cc_small_encode.
static int frames_tail(Ctx *c, const void *pixlab_d, bool wide, uint32_t K, const uint32_t *cent_d, const uint8_t *cent_h, const FrameBatch &fb, uint8_t *out,
                       uint64_t stride, uint64_t *lens, const std::function<int()> &after_hist, bool headers_aside = false, uint32_t pal_stride = 0) {
    const bool var = fb.var();
    const uint32_t F = fb.F, w = fb.w, h = fb.h, chunks = fb.chunks, hblocks = fb.hblocks;
    const uint32_t *wv = fb.wv, *hv = fb.hv;
    const uint64_t lb = wide ? 2 : 1, npf = var ? 0 : (uint64_t)w * h, lab_total = fb.lab_total;
    const bool runs_aligned = fb.runs_aligned;
    const FrameVar *fr_d = var ? fb.ft_d.as<FrameVar>() : nullptr;
    DevBuf pixlab_al, cnt_d;
    // frames whose label run does not start on a 16-byte boundary are moved apart (the pack reads 16 labels per load)
    const void *labs = pixlab_d;
    uint64_t lab_stride = npf;
    if (var) {
        if (!runs_aligned) {
            ScopedKernelTimer t(c, "frames_var_align");
            CNIIC_HIP_TRY(c, pixlab_al.alloc(lab_total * lb + 16));
            CNIIC_TRY(frame_labels_align_var(c, pixlab_d, pixlab_al.p, fr_d, F, chunks, wide));
            labs = pixlab_al.p;
            t.stop(1);
        }
    } else if ((npf * lb) & 15) {
        lab_stride = (npf + 15) & ~15ull;
        CNIIC_HIP_TRY(c, pixlab_al.alloc(lab_stride * lb * F + 16));
        CNIIC_HIP_TRY(c, hipMemcpy2DAsync(pixlab_al.p, lab_stride * lb, pixlab_d, npf * lb, npf * lb, F, hipMemcpyDeviceToDevice, c->stream));
        labs = pixlab_al.p;
    }
    CNIIC_HIP_TRY(c, cnt_d.alloc((uint64_t)F * K * 4));
    if (var) {
        ScopedKernelTimer t(c, "frames_var_hist");
        CNIIC_TRY(frame_label_hist_var(c, labs, fr_d, F, hblocks, wide, K, cnt_d.as<uint32_t>()));
        t.stop(1);
    } else {
        CNIIC_TRY(frame_label_hist(c, labs, npf, lab_stride, F, wide, K, cnt_d.as<uint32_t>()));
    }
    const bool gpu_trees = !wide && K <= 256 && c->opt(CNIIC_OPT_FRAME_TREES_HOST, "CNIIC_FRAME_TREES_HOST", 0) == 0;
    std::vector<uint32_t> cnt(gpu_trees ? 0 : (size_t)F * K);
    if (!gpu_trees) CNIIC_HIP_TRY(c, hipMemcpyAsync(cnt.data(), cnt_d.p, cnt.size() * 4, hipMemcpyDeviceToHost, c->stream));
    host_trace().mark("frames: hist enqueued");
    if (after_hist) CNIIC_TRY(after_hist());
    host_trace().mark("frames: result_end (sync)");
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    host_trace().mark("frames: wait for the histograms");
    FramesOut fo(c, out, stride, F);
    DevBuf clen_d, ccode_d;
    CNIIC_HIP_TRY(c, clen_d.alloc((size_t)F * K));
    CNIIC_HIP_TRY(c, ccode_d.alloc((size_t)F * K * 8));
    std::vector<uint64_t> totals(F, 0);
    // the label pack of every frame behind its header: bit bases on the host (bb_h) or already on the device (bb_d)
    auto pack = [&](const uint64_t *bb_h, const uint64_t *bb_d) {
        if (!var)
            return huff_pack_labels_frames(c, labs, npf, lab_stride, F, wide, K, clen_d.as<uint8_t>(), ccode_d.as<uint64_t>(), fo.dev, stride, bb_h, totals.data(), bb_d);
        ScopedKernelTimer t(c, "frames_var_pack");
        const int rc = huff_pack_labels_frames_var(c, labs, fr_d, F, chunks, wide, K, clen_d.as<uint8_t>(), ccode_d.as<uint64_t>(), fo.dev, stride, bb_h, totals.data(), bb_d);
        t.stop(3);
        return rc;
    };
    if (gpu_trees) {
        // ---- K <= 256: codes, code tables and stream headers of all frames by one kernel (k_frame_trees); the host sees the
        // lengths (it owes them to the caller and must hold them against the stride before anything is packed) and nothing else
        // (headers_aside: the headers are built beside the output and copied in once the lengths are known to fit, so that a refused call
        // leaves `out` as it was; a header is at most 8 + 12 K + (K - 1) bytes, and the pack wants the bytes behind it zero)
        DevBuf hdr_d;
        const uint64_t hstride = (8ull + 13ull * K + 3) & ~3ull;
        if (headers_aside) {
            CNIIC_HIP_TRY(c, hdr_d.alloc(hstride * F));
            CNIIC_HIP_TRY(c, hipMemsetAsync(hdr_d.p, 0, hstride * F, c->stream));
        } else {
            CNIIC_TRY(fo.begin());
        }
        DevBuf meta_d;
        CNIIC_HIP_TRY(c, meta_d.alloc((size_t)F * 24 + 8));  // bit base, payload bits, stream length per frame; error word
        uint64_t *bb_d = meta_d.as<uint64_t>(), *nb_d = bb_d + F, *ln_d = nb_d + F;
        uint32_t *err_d = reinterpret_cast<uint32_t *>(ln_d + F);
        CNIIC_HIP_TRY(c, hipMemsetAsync(err_d, 0, 8, c->stream));
        ScopedKernelTimer t_trees(c, "frames_var_trees", var && c->timers);
        CNIIC_TRY(frame_trees(c, cnt_d.as<uint32_t>(), cent_d, F, K, w, h, headers_aside ? hdr_d.as<uint8_t>() : fo.dev, headers_aside ? hstride : stride,
                              clen_d.as<uint8_t>(), ccode_d.as<uint64_t>(), bb_d, nb_d, ln_d, err_d, fr_d, pal_stride));
        t_trees.stop(1);
        std::vector<uint64_t> meta((size_t)F * 3 + 1);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(meta.data(), meta_d.p, (size_t)F * 24 + 8, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        host_trace().mark("frames: trees, codes, headers (GPU) + lengths back");
        const uint32_t err = (uint32_t)meta[(size_t)F * 3];
        if (err & 3u) return c->fail(CNIIC_ERR_BAD_ARG, "huffman: cannot build code");
        std::copy_n(meta.data() + 2 * (size_t)F, F, lens);
        CNIIC_TRY(fo.check_lens(lens, (err & 4u) != 0));
        if (headers_aside) {
            uint64_t hmax = 0;   // the longest header, in whole words: within hstride, and within the stride since every stream fits
            for (uint32_t f = 0; f < F; f++) hmax = std::max<uint64_t>(hmax, (meta[f] / 8 + 3) & ~3ull);
            CNIIC_TRY(fo.begin());
            CNIIC_HIP_TRY(c, hipMemcpy2DAsync(fo.dev, stride, hdr_d.p, hstride, hmax, F, hipMemcpyDeviceToDevice, c->stream));
        }
        CNIIC_TRY(pack(nullptr, bb_d));
        host_trace().mark("frames: pack (+sync)");
        CNIIC_TRY(fo.finish(totals.data(), meta.data() + F));
        host_trace().dump();
        return CNIIC_OK;
    }
    // ---- per frame on the host, on a few threads: tree, stream header and per-cluster codes from the frame's pixels per cluster
    std::vector<std::vector<uint8_t>> headers(F);
    std::vector<uint8_t> clen((size_t)F * K);
    std::vector<uint64_t> ccode((size_t)F * K), nbits(F, 0);
    std::atomic<int> bad{0};
    parallel_for(F, std::max(1u, std::min({F, 16u, std::thread::hardware_concurrency()})), [&](uint32_t f, uint32_t) {
        if (!palette_code(cent_h + 3 * (size_t)f * pal_stride, cnt.data() + (size_t)f * K, K, var ? wv[f] : w, var ? hv[f] : h, headers[f], &clen[(size_t)f * K], &ccode[(size_t)f * K],
                          &nbits[f]))
            bad = 1;
    });
    host_trace().mark("frames: trees, codes, headers (host threads)");
    if (bad) return c->fail(CNIIC_ERR_BAD_ARG, "huffman: cannot build code");
    uint64_t hmax = 0;
    for (uint32_t f = 0; f < F; f++) {
        lens[f] = headers[f].size() + (nbits[f] + 7) / 8;
        hmax = std::max<uint64_t>(hmax, headers[f].size());
    }
    CNIIC_TRY(fo.check_lens(lens));
    hmax = (hmax + 3) & ~3ull;
    CNIIC_TRY(fo.begin());
    DevBuf hdr_d;
    std::vector<uint8_t> hdr_all(hmax * F, 0);
    std::vector<uint64_t> bit_base(F);
    for (uint32_t f = 0; f < F; f++) { memcpy(hdr_all.data() + hmax * f, headers[f].data(), headers[f].size()); bit_base[f] = headers[f].size() * 8; }
    CNIIC_HIP_TRY(c, hdr_d.alloc(hdr_all.size()));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(hdr_d.p, hdr_all.data(), hdr_all.size(), hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemcpy2DAsync(fo.dev, stride, hdr_d.p, hmax, hmax, F, hipMemcpyDeviceToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(clen_d.p, clen.data(), clen.size(), hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(ccode_d.p, ccode.data(), ccode.size() * 8, hipMemcpyHostToDevice, c->stream));
    CNIIC_TRY(pack(bit_base.data(), nullptr));
    host_trace().mark("frames: copies + pack (+sync)");
    CNIIC_TRY(fo.finish(totals.data(), nbits.data()));
    host_trace().dump();
    return CNIIC_OK;
}

// A batch of F frames (contiguous in rgb_d) coded with ONE palette -- north_star config 4: the K-means ran over the union of all the
// pixels (of all ranks); every frame is then its own Hufman stream (clusterc.rs:31-52 per frame: the reduced frame's own histogram,
// tree and payload), written at out + f * stride.  One pass gives every pixel's label, one kernel the pixels per (frame, cluster), the
// trees are built by one kernel (or on a few host threads) and the F packs are enqueued back to back.
//   wv == nullptr  F equally sized frames of w x h (cc_finish_frames): grids of (chunk, frame)
//   wv, hv         frame f is wv[f] x hv[f] (cc_finish_frames_var): the host builds one table row per frame (FrameVar, common.hpp), uploads
//                  it once, and every kernel runs a 1-D grid over the chunks of all frames.  Stage timers (when on): frames_var_*
// Everything that does not depend on the frames' shapes is the same code for both.
static int finish_frames(CcSession *s, const uint8_t *rgb_d, uint32_t w, uint32_t h, const uint32_t *wv, const uint32_t *hv, uint32_t F, uint8_t *out,
                         uint64_t stride, uint64_t *lens, cniic_kmeans_stats *stats) {
    Ctx *c = s->c;
    const uint32_t K = s->K;
    const bool var = wv != nullptr;
    const char *who = var ? "cc_finish_frames_var" : "cc_finish_frames";
    const uint64_t U = s->U, npf = var ? 0 : (uint64_t)w * h;
    uint64_t n = npf * F;
    KmRgbwState *km = s->km;
    host_trace().mark("frames: enter");
    if (!F || (!var && !npf)) return c->fail(CNIIC_ERR_BAD_ARG, "%s: empty batch", who);
    if (var) {
        n = 0;
        for (uint32_t f = 0; f < F; f++) {
            const uint64_t np = (uint64_t)wv[f] * hv[f];
            if (!np) return c->fail(CNIIC_ERR_BAD_ARG, "%s: frame %u is %u x %u", who, f, wv[f], hv[f]);
            if (__builtin_add_overflow(n, np, &n)) return c->fail(CNIIC_ERR_BAD_ARG, "%s: too many pixels", who);
        }
    }
    if (stride & 3) return c->fail(CNIIC_ERR_BAD_ARG, "%s: the stride between streams must be a multiple of 4", who);
    if (s->sp_mode && s->sp.npx != n) return c->fail(CNIIC_ERR_BAD_ARG, "%s: the session was opened on %llu pixels, the batch has %llu", who,
                                                     (unsigned long long)s->sp.npx, (unsigned long long)n);
    if (var && !s->sp_mode && s->counts_local) {  // a dense-table session knows its pixels as the sum of its colours' counts
        DevBuf sum_d;
        uint64_t opened = 0;
        CNIIC_HIP_TRY(c, sum_d.alloc(8));
        CNIIC_TRY(sum_u32_dev(c, s->weight_d.as<uint32_t>(), U, sum_d.as<uint64_t>()));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(&opened, sum_d.p, 8, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (opened != n) return c->fail(CNIIC_ERR_BAD_ARG, "%s: the session was opened on %llu pixels, the batch has %llu", who,
                                        (unsigned long long)opened, (unsigned long long)n);
    }
    const bool wide = km_rgbw_is_wide(km);
    const uint64_t lb = wide ? 2 : 1;
    FrameBatch fb;
    fb.w = w; fb.h = h; fb.wv = wv; fb.hv = hv; fb.F = F;
    if (var) CNIIC_TRY(fb.build_table(c, who, lb));
    std::vector<uint8_t> cent(3 * (size_t)K);
    std::vector<uint64_t> members(K), wsum(K);
    cniic_kmeans_stats st{};
    CNIIC_TRY(km_rgbw_result_begin(km));
    DevBuf lab_d, key2label, pixlab;
    host_trace().mark("frames: result_begin");
    CNIIC_HIP_TRY(c, pixlab.alloc(n * lb + 16));
    host_trace().mark("frames: alloc pixel labels");
    if (var) CNIIC_TRY(fb.upload_table(c));
    ScopedKernelTimer t_labels(c, "frames_var_labels", var && c->timers);
    if (s->sp_mode) {
        uint32_t *cell_start, *ckeys, *cweight;
        km_rgbw_cell_arrays(km, &cell_start, &ckeys, &cweight);
        CNIIC_TRY(km_rgbw_need_arrays(km));
        CNIIC_TRY(sp_pixel_labels(c, &s->sp, rgb_d, cell_start, ckeys, km_rgbw_labels_internal(km, nullptr), wide, pixlab.p));
        host_trace().mark("frames: pixel labels enqueued");
    } else {
        CNIIC_HIP_TRY(c, lab_d.alloc(U * lb));
        CNIIC_TRY(km_rgbw_labels_canonical(km, lab_d.p));
        CNIIC_HIP_TRY(c, key2label.alloc((1ull << 24) * lb));
        CNIIC_TRY(scatter_labels_by_key(c, s->keys_d.as<uint32_t>(), lab_d.p, wide, U, key2label.p));
        CNIIC_TRY(pixel_labels(c, rgb_d, n, key2label.p, wide, pixlab.p));
    }
    t_labels.stop(1);
    return frames_tail(c, pixlab.p, wide, K, km_rgbw_centroids_dev(km), cent.data(), fb, out, stride, lens, [&]() -> int {
        CNIIC_TRY(km_rgbw_result_end(km, cent.data(), members.data(), wsum.data(), &st));
        if (stats) *stats = st;
        return check_enough_active(c, K, U, st.active);
    });
}

int cc_finish_frames(CcSession *s, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t F, uint8_t *out, uint64_t stride, uint64_t *lens,
                     cniic_kmeans_stats *stats) {
    return finish_frames(s, rgb_d, w, h, nullptr, nullptr, F, out, stride, lens, stats);
}

int cc_finish_frames_var(CcSession *s, const uint8_t *rgb_d, const uint32_t *w, const uint32_t *h, uint32_t F, uint8_t *out, uint64_t stride, uint64_t *lens,
                         cniic_kmeans_stats *stats) {
    if (!w || !h) return s->c->fail(CNIIC_ERR_BAD_ARG, "cc_finish_frames_var: null argument");
    return finish_frames(s, rgb_d, 0, 0, w, h, F, out, stride, lens, stats);
}

// ------------------------------------------------------------------ frozen palettes (cniic_palette_*, k_palette.hip)
// The session's centroids as of its last update and the pixels per cluster it knows (its wsum), through the session's own rule for results:
// km_rgbw_result_begin / _end, with the hand-over of a persistent launch that had given up (kKmRetry).  Nothing of the session changes.
int cc_palette(CcSession *s, uint8_t *centroids_h, uint64_t *pixels_h) {
    KmRgbwState *km = s->km;
    for (int attempt = 0;; attempt++) {
        CNIIC_TRY(km_rgbw_result_begin(km));
        const int rc = km_rgbw_result_end(km, centroids_h, nullptr, pixels_h, nullptr);
        if (rc == kKmRetry && attempt == 0) continue;
        return rc;
    }
}

// cent_h: K x 3 bytes on the host.  The colour -> label table of all 2^24 colours is built here, once; the handle keeps it, the entries as
// the 0xRRGGBB words k_frame_trees reads, and the host copy palette_code reads.
int palette_create(Ctx *c, const uint8_t *cent_h, uint32_t K, Palette **out) {
    if (!K || K > 65536u) return c->fail(CNIIC_ERR_BAD_ARG, "palette_create: K = %u (1 .. 65536)", K);
    std::unique_ptr<Palette> p(new Palette);
    p->c = c;
    p->K = K;
    p->wide = K > 256;
    p->cent_h.assign(cent_h, cent_h + 3 * (size_t)K);
    std::vector<uint32_t> words(K);
    for (uint32_t k = 0; k < K; k++) words[k] = ((uint32_t)cent_h[3 * k] << 16) | ((uint32_t)cent_h[3 * k + 1] << 8) | cent_h[3 * k + 2];
    CNIIC_HIP_TRY(c, p->cent_d.alloc((uint64_t)K * 4));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(p->cent_d.p, words.data(), (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, p->table.alloc((1ull << 24) * (p->wide ? 2 : 1)));
    uint32_t list_max = kPalListMax;   // (the testing build: a budget low enough for ordinary palettes to take the plain route)
    if (const char *e = test_env("CNIIC_TEST_PAL_LIST_MAX")) list_max = (uint32_t)std::min<unsigned long long>(strtoull(e, nullptr, 10), kPalListMax);
    DevBuf plain_d;
    if (c->timers) {
        CNIIC_HIP_TRY(c, plain_d.alloc(4));
        CNIIC_HIP_TRY(c, hipMemsetAsync(plain_d.p, 0, 4, c->stream));
    }
    {
        ScopedKernelTimer t(c, "pal_lut");
        CNIIC_TRY(palette_lut(c, p->cent_d.as<uint32_t>(), K, p->wide, p->table.p, list_max, c->timers ? plain_d.as<uint32_t>() : nullptr));
        t.stop(1);
    }
    uint32_t plain = 0;
    if (c->timers) CNIIC_HIP_TRY(c, hipMemcpyAsync(&plain, plain_d.p, 4, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the words above are this call's; a handle that comes back is complete)
    if (plain) c->ktimes["pal_lut_plain"].launches += plain;   // (stage timers: how many cells took the plain route; no duration)
    *out = p.release();
    return CNIIC_OK;
}

// the index image: labels_d receives n labels of 1 or 2 bytes (16-byte aligned device memory)
int palette_labels(Palette *p, const uint8_t *rgb_d, uint64_t n, void *labels_d) {
    Ctx *c = p->c;
    ScopedKernelTimer t(c, "pal_labels");
    CNIIC_TRY(pixel_labels(c, rgb_d, n, p->table.p, p->wide, labels_d));
    t.stop(1);
    return CNIIC_OK;
}

// cc_finish_frames_var with the gather through the handle's table in the place of a session's labels: no K-means state, no pixel total
// to hold the batch against, no active-cluster check
int palette_encode_frames_var(Palette *p, const uint8_t *rgb_d, const uint32_t *wv, const uint32_t *hv, uint32_t F, uint8_t *out, uint64_t stride, uint64_t *lens) {
    Ctx *c = p->c;
    const char *who = "palette_encode_frames_var";
    if (!wv || !hv || !F) return c->fail(CNIIC_ERR_BAD_ARG, "%s: empty batch", who);
    uint64_t n = 0;
    for (uint32_t f = 0; f < F; f++) {
        const uint64_t np = (uint64_t)wv[f] * hv[f];
        if (!np) return c->fail(CNIIC_ERR_BAD_ARG, "%s: frame %u is %u x %u", who, f, wv[f], hv[f]);
        if (__builtin_add_overflow(n, np, &n)) return c->fail(CNIIC_ERR_BAD_ARG, "%s: too many pixels", who);
    }
    if (stride & 3) return c->fail(CNIIC_ERR_BAD_ARG, "%s: the stride between streams must be a multiple of 4", who);
    const uint64_t lb = p->wide ? 2 : 1;
    FrameBatch fb;
    fb.wv = wv; fb.hv = hv; fb.F = F;
    CNIIC_TRY(fb.build_table(c, who, lb));
    DevBuf pixlab;
    CNIIC_HIP_TRY(c, pixlab.alloc(n * lb + 16));
    CNIIC_TRY(fb.upload_table(c));
    CNIIC_TRY(palette_labels(p, rgb_d, n, pixlab.p));
    return frames_tail(c, pixlab.p, p->wide, p->K, p->cent_d.as<uint32_t>(), p->cent_h.data(), fb, out, stride, lens, nullptr, true);
}

// ---- small frames of a batch call, a workgroup per frame: what the encode routes share (codec.hpp)
static uint64_t frame_px(const VarFrame &f) { return (uint64_t)f.w * f.h; }

// The frames (largest first) in chunks: a chunk takes as many as frames_that_fit(its first, largest frame) says -- one at least --, and
// body(the chunk's frames, how many) encodes it.
template <class Fit, class Body>
static int for_chunks(VarFrame *const *fr, uint32_t n, Fit frames_that_fit, Body body) {
    for (uint32_t at = 0; at < n;) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(n - at, std::max<uint64_t>(1, frames_that_fit(*fr[at])));
        CNIIC_TRY(body(fr + at, cnt));
        at += cnt;
    }
    return CNIIC_OK;
}

// A chunk's rows go up, launch(rows, result rows) runs under the stage timer `timer` (launches = the rows), the result rows come down: one wait
template <class Row, class Result, class Launch>
static int run_rows(Ctx *c, const char *timer, const std::vector<Row> &rows, std::vector<Result> &res, Launch launch) {
    const size_t n = rows.size();
    DevBuf rows_d, res_d;
    CNIIC_HIP_TRY(c, rows_d.alloc(n * sizeof(Row)));
    CNIIC_HIP_TRY(c, res_d.alloc(n * sizeof(Result)));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(rows_d.p, rows.data(), n * sizeof(Row), hipMemcpyHostToDevice, c->stream));
    {
        ScopedKernelTimer t(c, timer);
        CNIIC_TRY(launch(rows_d.as<Row>(), res_d.as<Result>()));
        t.stop(n);
    }
    res.resize(n);
    CNIIC_HIP_TRY(c, hipMemcpyAsync(res.data(), res_d.p, n * sizeof(Result), hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// A frame's K-means outcome as the single call reports it: too few points (`what` they are called there), else the stats and the check
// of the active clusters.  Returns whether the frame goes on.
static bool report_kmeans_outcome(Ctx *c, uint32_t K, VarFrame &f, uint32_t status, uint64_t points, uint64_t iterations, uint64_t moved_last, uint64_t reseeds,
                                  uint64_t active, uint64_t pair_evals, const char *what) {
    if (status) {
        f.rc = c->fail(CNIIC_ERR_TOO_FEW_POINTS, "kmeans: %llu %s for %u clusters (src/kmeans.rs:68)", (unsigned long long)points, what, K);
        f.msg = c->err;
        return false;
    }
    f.st.iterations = iterations; f.st.moved_last = moved_last; f.st.empty_reseeds = reseeds; f.st.active = active;
    f.st.pair_evals = pair_evals;
    f.rc = check_enough_active(c, K, points, active);
    if (f.rc != CNIIC_OK) f.msg = c->err;
    return f.rc == CNIIC_OK;
}

// Every finished stream of a chunk to its frame's own place, unless it is longer than the caller's room.  The streams lie in `scratch`, a
// slot of sstride bytes each, `slots` of them; a SmallStream says which slot holds whose stream and how long it is.  Device destinations:
// one launch of cc_small_place under the stage timer t_place; host destinations: the whole scratch comes down once.
struct SmallStream { uint32_t slot; VarFrame *f; uint64_t len; };
static int place_streams(Ctx *c, const DevBuf &scratch, uint64_t sstride, uint32_t slots, const std::vector<SmallStream> &streams, const char *t_place) {
    std::vector<CcSmallPlace> pl;
    for (const SmallStream &s : streams) {
        VarFrame &f = *s.f;
        f.len = s.len;
        if (f.len > f.cap) {
            f.rc = c->fail(CNIIC_ERR_CAPACITY, "encode: stream is %llu bytes, capacity %llu", (unsigned long long)f.len, (unsigned long long)f.cap);
            f.msg = c->err;
            continue;
        }
        pl.push_back(CcSmallPlace{sstride * s.slot, f.out, f.len});
    }
    if (pl.empty()) return CNIIC_OK;
    if (is_device_ptr(pl[0].dst)) {   // (all destinations host or all device memory)
        DevBuf pl_d;
        CNIIC_HIP_TRY(c, pl_d.alloc(pl.size() * sizeof(CcSmallPlace)));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(pl_d.p, pl.data(), pl.size() * sizeof(CcSmallPlace), hipMemcpyHostToDevice, c->stream));
        ScopedKernelTimer t(c, t_place);
        CNIIC_TRY(cc_small_place(c, pl_d.as<CcSmallPlace>(), (uint32_t)pl.size(), scratch.as<uint8_t>()));
        t.stop(1);
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
        std::vector<uint8_t> host(sstride * slots);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(host.data(), scratch.p, host.size(), hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (const CcSmallPlace &p : pl) memcpy(p.dst, host.data() + p.src_off, p.len);
    }
    return CNIIC_OK;
}

// ---- small cluster-colors frames of a batch call, all at once (k_cc_small.hip)
// The stride of the tail's scratch is one no stream of a frame of npx pixels can exceed: the header is at most 8 + 13 K bytes (the tail's
// own hstride), the payload fewer than (log2 256 + 1) npx = 9 npx bits (Huffman's redundancy bound over at most 256 symbols).
static uint64_t cc_small_stream_bound(uint64_t npx, uint32_t K) { return (8ull + 13ull * K + (9 * npx + 7) / 8 + 15) & ~15ull; }

static int cc_small_chunk(Ctx *c, uint32_t K, uint64_t seed, uint64_t max_iters, VarFrame *const *fr, uint32_t n) {
    // ---- k_cc_small: rows, labels, palettes, results
    std::vector<CcSmallRow> rows(n);
    uint64_t lab_total = 0;
    for (uint32_t i = 0; i < n; i++) {
        rows[i] = CcSmallRow{fr[i]->src, lab_total, fr[i]->w, fr[i]->h};
        lab_total += ((uint64_t)fr[i]->w * fr[i]->h + 15) & ~15ull;
    }
    DevBuf labels_d, cent_d;
    CNIIC_HIP_TRY(c, labels_d.alloc(lab_total + 16));
    CNIIC_HIP_TRY(c, cent_d.alloc((uint64_t)n * K * 4));
    std::vector<CcSmallResult> res;
    CNIIC_TRY(run_rows(c, "cc_small_batch", rows, res, [&](const CcSmallRow *rows_d, CcSmallResult *res_d) {
        return cc_small_run(c, rows_d, n, fr[0]->w * fr[0]->h, K, seed, max_iters, labels_d.as<uint8_t>(), cent_d.as<uint32_t>(), res_d);   // (largest first)
    }));
    // ---- every frame's K-means outcome, as the single call reports it; the frames that go on
    std::vector<uint32_t> ok;
    for (uint32_t i = 0; i < n; i++) {
        const CcSmallResult &r = res[i];
        if (report_kmeans_outcome(c, K, *fr[i], r.status, r.U, r.iterations, r.moved_last, r.reseeds, r.active, (uint64_t)r.iterations * r.U * K, "distinct colours"))
            ok.push_back(i);
    }
    const uint32_t F = (uint32_t)ok.size();
    if (!F) return CNIIC_OK;
    // ---- the tail over those frames, a palette each, into scratch
    std::vector<uint32_t> wv(F), hv(F);
    FrameBatch fb;
    fb.F = F;
    fb.ft.resize(F);
    uint64_t ch = 0, hb = 0;
    for (uint32_t j = 0; j < F; j++) {
        const VarFrame &f = *fr[ok[j]];
        const uint64_t np = (uint64_t)f.w * f.h;
        wv[j] = f.w; hv[j] = f.h;
        fb.ft[j] = FrameVar{np, rows[ok[j]].lab_base, rows[ok[j]].lab_base, (uint32_t)ch, (uint32_t)hb, f.w, f.h};
        ch += ceil_div(np, kFrameVarChunk);
        hb += ceil_div(np, kFrameVarHistSpan);
    }
    fb.wv = wv.data(); fb.hv = hv.data();
    fb.lab_total = lab_total; fb.chunks = (uint32_t)ch; fb.hblocks = (uint32_t)hb;
    CNIIC_TRY(fb.upload_table(c));
    // the palettes of the frames that go on, in the tail's frame order (all of them: where they are)
    DevBuf cent_ok;
    const uint32_t *cent_tail = cent_d.as<uint32_t>();
    if (F != n) {
        CNIIC_HIP_TRY(c, cent_ok.alloc((uint64_t)F * K * 4));
        for (uint32_t j = 0; j < F;) {   // (runs of neighbours move together)
            uint32_t e = j + 1;
            while (e < F && ok[e] == ok[e - 1] + 1) e++;
            CNIIC_HIP_TRY(c, hipMemcpyAsync(cent_ok.as<uint32_t>() + (size_t)j * K, cent_d.as<uint32_t>() + (size_t)ok[j] * K, (size_t)(e - j) * K * 4,
                                            hipMemcpyDeviceToDevice, c->stream));
            j = e;
        }
        cent_tail = cent_ok.as<uint32_t>();
    }
    std::vector<uint8_t> cent_h;
    if (c->opt(CNIIC_OPT_FRAME_TREES_HOST, "CNIIC_FRAME_TREES_HOST", 0) != 0) {   // the trees on host threads: they read K x 3 bytes per frame
        std::vector<uint32_t> words((size_t)F * K);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(words.data(), cent_tail, words.size() * 4, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        cent_h.resize(words.size() * 3);
        for (size_t k = 0; k < words.size(); k++) { cent_h[3 * k] = (uint8_t)(words[k] >> 16); cent_h[3 * k + 1] = (uint8_t)(words[k] >> 8); cent_h[3 * k + 2] = (uint8_t)words[k]; }
    }
    const uint64_t sstride = cc_small_stream_bound((uint64_t)fr[ok[0]]->w * fr[ok[0]]->h, K);   // (largest first)
    DevBuf scratch;
    CNIIC_HIP_TRY(c, scratch.alloc(sstride * F + 16));
    std::vector<uint64_t> lens(F);
    CNIIC_TRY(frames_tail(c, labels_d.p, false, K, cent_tail, cent_h.data(), fb, scratch.as<uint8_t>(), sstride, lens.data(), nullptr, false, K));
    std::vector<SmallStream> streams(F);
    for (uint32_t j = 0; j < F; j++) streams[j] = SmallStream{j, fr[ok[j]], lens[j]};
    return place_streams(c, scratch, sstride, F, streams, "cc_small_place");
}

int cc_small_encode(Ctx *c, uint32_t K, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n) {
    const uint64_t seed = (opts && opts->seed) ? opts->seed : kDefaultSeed, max_iters = opts ? opts->max_iters : 0;
    // the tail's scratch stays below 2 GiB
    return for_chunks(fr, n, [&](const VarFrame &first) { return (2ull << 30) / cc_small_stream_bound(frame_px(first), K); },
                      [&](VarFrame *const *chunk, uint32_t cnt) { return cc_small_chunk(c, K, seed, max_iters, chunk, cnt); });
}

// ---- small `delta` frames of a batch call, all at once (codec.hpp; k_delta_small.hip)
// what a frame of the chunk whose largest frame has npx pixels takes in HBM: its stream's slot and the kernel's three arrays of a word per pixel
static uint64_t delta_small_tmp_px(uint64_t npx) { return (npx + 3) & ~3ull; }
static uint64_t delta_small_frame_bytes(uint64_t npx) { return ds_stride(npx) + 12 * delta_small_tmp_px(npx); }

// The two codecs of the route (k_delta_small.hip: one body, two symbol kinds) differ on the host by the slot, the launch and the names
struct SmallHuffKind {
    const char *name, *t_batch, *t_place;
    uint64_t (*stride)(uint64_t npx);
    int (*run)(Ctx *, const DeltaSmallRow *, uint32_t, uint32_t, uint8_t *, uint64_t, uint32_t *, uint64_t, DeltaSmallResult *);
    uint64_t min_len;   // one leaf and no payload
};
static const SmallHuffKind kSmallDelta = {"delta_small", "delta_small_batch", "delta_small_place", ds_stride, delta_small_run, 15};
static const SmallHuffKind kSmallHuf = {"huf_small", "huf_small_batch", "huf_small_place", hs_stride, huf_small_run, 20};

static int delta_small_chunk(Ctx *c, const SmallHuffKind &kind, VarFrame *const *fr, uint32_t n) {
    const uint64_t max_px = frame_px(*fr[0]);   // (largest first)
    const uint64_t sstride = kind.stride(max_px), tmp_px = delta_small_tmp_px(max_px);
    std::vector<DeltaSmallRow> rows(n);
    for (uint32_t i = 0; i < n; i++) rows[i] = DeltaSmallRow{fr[i]->src, fr[i]->w, fr[i]->h};
    DevBuf scratch, tmp;
    CNIIC_HIP_TRY(c, scratch.alloc(sstride * n + 16));
    CNIIC_HIP_TRY(c, tmp.alloc(12 * tmp_px * n));
    std::vector<DeltaSmallResult> res;
    CNIIC_TRY(run_rows(c, kind.t_batch, rows, res, [&](const DeltaSmallRow *rows_d, DeltaSmallResult *res_d) {
        return kind.run(c, rows_d, n, (uint32_t)max_px, scratch.as<uint8_t>(), sstride, tmp.as<uint32_t>(), tmp_px, res_d);
    }));
    std::vector<SmallStream> streams(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = res[i].len;
        if (len < kind.min_len || len > sstride) return c->fail(CNIIC_ERR_HIP, "%s: a stream of %llu bytes in a slot of %llu", kind.name, (unsigned long long)len, (unsigned long long)sstride);
        streams[i] = SmallStream{i, fr[i], len};
    }
    return place_streams(c, scratch, sstride, n, streams, kind.t_place);
}

int delta_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n) {
    // the scratch stays below 2 GiB
    return for_chunks(fr, n, [](const VarFrame &first) { return (2ull << 30) / delta_small_frame_bytes(frame_px(first)); },
                      [&](VarFrame *const *chunk, uint32_t cnt) { return delta_small_chunk(c, kSmallDelta, chunk, cnt); });
}

// ---- small `hufman` frames of a batch call, all at once (k_huf_small in k_delta_small.hip): the chunk above under the other kind.
// A frame of the chunk whose largest frame has npx pixels takes its slot (hs_stride), the kernel's three words per pixel, its row and its
// result row; the chunks stay below 2 GiB (the testing library: below CNIIC_TEST_MEASURE_BUDGET bytes, a frame at least).
constexpr uint64_t kHufSmallScratch = 2ull << 30;
static uint64_t huf_small_frame_bytes(uint64_t npx) { return hs_stride(npx) + 12 * delta_small_tmp_px(npx) + sizeof(DeltaSmallRow) + sizeof(DeltaSmallResult); }

int huf_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n) {
    const uint64_t budget = test_budget(kHufSmallScratch);
    return for_chunks(fr, n, [&](const VarFrame &first) { return budget / huf_small_frame_bytes(frame_px(first)); },
                      [&](VarFrame *const *chunk, uint32_t cnt) { return delta_small_chunk(c, kSmallHuf, chunk, cnt); });
}

// ---- small `hilbert(rle)` / `hilbert(rle(d))` frames of a batch call, all at once (k_rle_small.hip)
// A frame of the chunk whose largest frame has npx pixels takes its slot (rs_stride: a run per pixel), its row and its result row; the
// chunks stay below 2 GiB (the testing library: below CNIIC_TEST_MEASURE_BUDGET bytes, a frame at least).
constexpr uint64_t kRleSmallScratch = 2ull << 30;
static uint64_t rle_small_frame_bytes(uint64_t npx) { return rs_stride(npx) + sizeof(RleSmallRow) + sizeof(RleSmallResult); }

static int rle_small_chunk(Ctx *c, double T, int mode, VarFrame *const *fr, uint32_t n) {
    const uint64_t max_px = frame_px(*fr[0]);   // (largest first)
    const uint64_t sstride = rs_stride(max_px);
    std::vector<RleSmallRow> rows(n);
    for (uint32_t i = 0; i < n; i++) rows[i] = RleSmallRow{fr[i]->src, fr[i]->w, fr[i]->h};
    DevBuf scratch;
    CNIIC_HIP_TRY(c, scratch.alloc(sstride * n + 16));
    std::vector<RleSmallResult> res;
    CNIIC_TRY(run_rows(c, "rle_small_batch", rows, res, [&](const RleSmallRow *rows_d, RleSmallResult *res_d) {
        return rle_small_run(c, rows_d, n, (uint32_t)max_px, T, mode, scratch.as<uint8_t>(), sstride, res_d);
    }));
    std::vector<SmallStream> streams(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t len = res[i].len;   // one record at least
        if (len < 20 || len > sstride) return c->fail(CNIIC_ERR_HIP, "rle_small: a stream of %llu bytes in a slot of %llu", (unsigned long long)len, (unsigned long long)sstride);
        streams[i] = SmallStream{i, fr[i], len};
    }
    return place_streams(c, scratch, sstride, n, streams, "rle_small_place");
}

int rle_small_encode(Ctx *c, double d, VarFrame *const *fr, uint32_t n) {
    const double T = rla_threshold(d);   // (once per call)
    const int mode = rs_mode(d, T);
    const uint64_t budget = test_budget(kRleSmallScratch);
    return for_chunks(fr, n, [&](const VarFrame &first) { return budget / rle_small_frame_bytes(frame_px(first)); },
                      [&](VarFrame *const *chunk, uint32_t cnt) { return rle_small_chunk(c, T, mode, chunk, cnt); });
}

// ---- small `zip(dict)` frames of a batch call, all at once (k_zd_small.hip)
// A frame of the chunk whose largest frame has npx pixels takes its slot (zs_stride: 4 bytes a pair), its trie table (8 bytes a slot, at
// least two slots per byte of text), its row and its result row; the chunks stay below 1 GiB -- 235 frames of 16 384 pixels -- (the
// testing library: below CNIIC_TEST_MEASURE_BUDGET bytes, a frame at least).
constexpr uint64_t kZdSmallScratch = 1ull << 30;
static uint64_t zd_small_frame_bytes(uint64_t npx) {
    const uint64_t N = zs_text_len((uint32_t)npx);
    return zs_stride(N) + (8ull << zs_table_bits(N)) + sizeof(ZdSmallRow) + sizeof(ZdSmallResult);
}
// the same for Hilbert { compress: Zip }: 11 bytes of text a pixel, and the 8 bytes of the head in the slot (hz_small.hpp)
static uint64_t hz_small_frame_bytes(uint64_t npx) {
    const uint64_t N = hz_text_len((uint32_t)npx);
    return hz_stride(N) + (8ull << zs_table_bits(N)) + sizeof(ZdSmallRow) + sizeof(ZdSmallResult);
}
// a stage mark that is a count, not a time
static void stage_count(Ctx *c, const char *name, uint64_t n) {
    if (c->timers && n) c->ktimes[name].launches += n;
}

// The two codecs of the route (k_zd_small.hip: one body, two text kinds) differ on the host by the text's length, the slot, the launch and the names
struct SmallZipKind {
    const char *name, *t_batch, *t_place, *t_handback, *t_finished;
    uint32_t (*text_len)(uint32_t npx);
    uint64_t (*stride)(uint64_t N);
    uint64_t (*frame_bytes)(uint64_t npx);
    int (*run)(Ctx *, const ZdSmallRow *, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t *, uint32_t, uint8_t *, uint64_t, ZdSmallResult *);
    uint32_t head;   // bytes of the stream in front of the pairs
};
static const SmallZipKind kSmallZipDict = {"zd_small", "zd_small_batch", "zd_small_place", "zd_small_handback", "zd_small_finished", zs_text_len, zs_stride, zd_small_frame_bytes, zd_small_run, 0};
static const SmallZipKind kSmallHilbertZip = {"hz_small", "hz_small_batch", "hz_small_place", "hz_small_handback", "hz_small_finished", hz_text_len, hz_stride, hz_small_frame_bytes, hz_small_run, kHzHead};

static int zd_small_chunk(Ctx *c, const SmallZipKind &kind, uint32_t spec, uint32_t giveup, VarFrame *const *fr, uint32_t n) {
    const uint64_t max_px = frame_px(*fr[0]);   // (largest first)
    const uint64_t N = kind.text_len((uint32_t)max_px), sstride = kind.stride(N);
    const uint32_t bits = zs_table_bits(N);
    std::vector<ZdSmallRow> rows(n);
    for (uint32_t i = 0; i < n; i++) rows[i] = ZdSmallRow{fr[i]->src, fr[i]->w, fr[i]->h};
    DevBuf scratch, tables;
    CNIIC_HIP_TRY(c, scratch.alloc(sstride * n + 16));
    CNIIC_HIP_TRY(c, tables.alloc(((uint64_t)n << bits) * sizeof(uint64_t)));
    std::vector<ZdSmallResult> res;
    CNIIC_TRY(run_rows(c, kind.t_batch, rows, res, [&](const ZdSmallRow *rows_d, ZdSmallResult *res_d) {
        return kind.run(c, rows_d, n, (uint32_t)max_px, spec, giveup, tables.as<uint64_t>(), bits, scratch.as<uint8_t>(), sstride, res_d);
    }));
    std::vector<SmallStream> streams;
    uint64_t back = 0, finished = 0;
    for (uint32_t i = 0; i < n; i++) {
        finished += res[i].finished;
        if (res[i].verdict == kZsHandedBack) { fr[i]->handed_back = true; back++; continue; }
        const uint64_t len = res[i].len;   // one pair at least
        if (res[i].verdict != kZsOk || len < kind.head + 4 || len != kind.head + 4ull * res[i].pairs || len > sstride)
            return c->fail(CNIIC_ERR_HIP, "%s: a stream of %llu bytes in a slot of %llu", kind.name, (unsigned long long)len, (unsigned long long)sstride);
        streams.push_back(SmallStream{i, fr[i], len});
    }
    stage_count(c, kind.t_handback, back);
    stage_count(c, kind.t_finished, finished);
    return place_streams(c, scratch, sstride, n, streams, kind.t_place);
}

// the give-up cap of a call: the testing library lowers both caps with one knob (never above the kernel's own)
static uint32_t small_zip_giveup(const char *e) { return e ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), kZsGiveUp) : kZsGiveUp; }
static int small_zip_encode(Ctx *c, const SmallZipKind &kind, uint32_t giveup, VarFrame *const *fr, uint32_t n) {
    const uint32_t spec = std::min(kZsSpecCap, giveup);
    const uint64_t budget = test_budget(kZdSmallScratch);
    return for_chunks(fr, n, [&](const VarFrame &first) { return budget / kind.frame_bytes(frame_px(first)); },
                      [&](VarFrame *const *chunk, uint32_t cnt) { return zd_small_chunk(c, kind, spec, giveup, chunk, cnt); });
}

int zd_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n) { return small_zip_encode(c, kSmallZipDict, small_zip_giveup(test_env("CNIIC_TEST_ZD_SMALL_CAP")), fr, n); }

// ---- small Hilbert { compress: Zip } frames of a batch call, all at once (k_hz_small in k_zd_small.hip): the chunk above under the other kind
int hz_small_encode(Ctx *c, VarFrame *const *fr, uint32_t n) { return small_zip_encode(c, kSmallHilbertZip, small_zip_giveup(test_env("CNIIC_TEST_HZ_SMALL_CAP")), fr, n); }

// ---- small voronoi(K) frames of a batch call, all at once (k_vor_small.hip)
// A chunk's scratch is a slot per frame for the stream (16 + 19 K bytes, rounded up to 16), its row and its result row; the chunks stay
// below 2 GiB (the testing library: below CNIIC_TEST_MEASURE_BUDGET bytes, a frame at least).
constexpr uint64_t kVorSmallScratch = 2ull << 30;
static uint64_t vor_small_slot(uint32_t K) { return ((uint64_t)vs_stream_len(K) + 15) & ~15ull; }

static int vor_small_chunk(Ctx *c, uint32_t K, uint64_t seed, uint64_t max_iters, bool stay_test, VarFrame *const *fr, uint32_t n) {
    const uint64_t sstride = vor_small_slot(K);
    std::vector<VorSmallRow> rows(n);
    for (uint32_t i = 0; i < n; i++) rows[i] = VorSmallRow{fr[i]->src, fr[i]->w, fr[i]->h};
    DevBuf scratch;
    CNIIC_HIP_TRY(c, scratch.alloc(sstride * n + 16));
    std::vector<VorSmallResult> res;
    CNIIC_TRY(run_rows(c, "vor_small_batch", rows, res, [&](const VorSmallRow *rows_d, VorSmallResult *res_d) {
        return vor_small_run(c, rows_d, n, fr[0]->w * fr[0]->h, K, seed, max_iters, stay_test, scratch.as<uint8_t>(), sstride, res_d);   // (largest first)
    }));
    // ---- every frame's K-means outcome, as the single call reports it; the frames whose streams stand
    std::vector<SmallStream> streams;
    for (uint32_t i = 0; i < n; i++) {
        const VorSmallResult &r = res[i];
        if (r.status > 1 || r.n != frame_px(*fr[i])) return c->fail(CNIIC_ERR_HIP, "vor_small: frame %u of the chunk reported no result", i);
        if (report_kmeans_outcome(c, K, *fr[i], r.status, r.n, r.iterations, r.moved_last, r.reseeds, r.active, r.evals, "points"))
            streams.push_back(SmallStream{i, fr[i], vs_stream_len(K)});
    }
    return place_streams(c, scratch, sstride, n, streams, "vor_small_place");
}

int vor_small_encode(Ctx *c, uint32_t K, const cniic_kmeans_opts *opts, VarFrame *const *fr, uint32_t n) {
    const uint64_t seed = (opts && opts->seed) ? opts->seed : kDefaultSeed, max_iters = opts ? opts->max_iters : 0;
    bool stay_test = true;
    if (const char *e = test_env("CNIIC_TEST_VOR_SMALL_NO_STAY")) stay_test = atoi(e) == 0;
    const uint64_t room = test_budget(kVorSmallScratch) / (vor_small_slot(K) + sizeof(VorSmallRow) + sizeof(VorSmallResult));   // (whatever the frames' sizes)
    return for_chunks(fr, n, [&](const VarFrame &) { return room; },
                      [&](VarFrame *const *chunk, uint32_t cnt) { return vor_small_chunk(c, K, seed, max_iters, stay_test, chunk, cnt); });
}

// How well the handle's palette fits a batch of frames: sse_h[f] = the exact sum over frame f's pixels of the squared distance to the pixel's entry
// under the rule (3 w h times the MSE of decoding that frame's palette_encode_frames_var stream), pixels_h[k] (may be null) = the pixels of all
// frames whose entry is k.  One launch (k_palette_fit) over the frame table of the var route; no labels are stored.
int palette_fit_frames_var(Palette *p, const uint8_t *rgb_d, const uint32_t *wv, const uint32_t *hv, uint32_t F, uint64_t *sse_h, uint64_t *pixels_h) {
    Ctx *c = p->c;
    const char *who = "palette_fit_frames_var";
    if (!wv || !hv || !F || !sse_h) return c->fail(CNIIC_ERR_BAD_ARG, "%s: empty batch", who);
    uint64_t n = 0;
    for (uint32_t f = 0; f < F; f++) {
        const uint64_t np = (uint64_t)wv[f] * hv[f];
        if (!np) return c->fail(CNIIC_ERR_BAD_ARG, "%s: frame %u is %u x %u", who, f, wv[f], hv[f]);
        if (__builtin_add_overflow(n, np, &n)) return c->fail(CNIIC_ERR_BAD_ARG, "%s: too many pixels", who);
    }
    FrameBatch fb;
    fb.wv = wv; fb.hv = hv; fb.F = F;
    CNIIC_TRY(fb.build_table(c, who, p->wide ? 2 : 1));
    CNIIC_TRY(fb.upload_table(c));
    const uint64_t words = (uint64_t)F + (pixels_h ? p->K : 0);
    DevBuf res;
    CNIIC_HIP_TRY(c, res.alloc(words * 8));
    CNIIC_HIP_TRY(c, hipMemsetAsync(res.p, 0, words * 8, c->stream));
    {
        ScopedKernelTimer t(c, "pal_fit");
        CNIIC_TRY(palette_fit(c, rgb_d, fb.ft_d.as<FrameVar>(), F, fb.chunks, p->table.p, p->wide, p->cent_d.as<uint32_t>(), p->K, res.as<uint64_t>(),
                              pixels_h ? res.as<uint64_t>() + F : nullptr));
        t.stop(1);
    }
    std::vector<uint64_t> host(words);
    CNIIC_HIP_TRY(c, hipMemcpyAsync(host.data(), res.p, words * 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(sse_h, host.data(), (size_t)F * 8);
    if (pixels_h) memcpy(pixels_h, host.data() + F, (size_t)p->K * 8);
    return CNIIC_OK;
}

// images of at least this many pixels take the super-cell partition (k_points.hip); CNIIC_SP_MIN_PIXELS overrides (tests: 0)
static uint64_t sp_min_pixels(const Ctx *c) { return c->opt(CNIIC_OPT_SP_MIN_PIXELS, "CNIIC_SP_MIN_PIXELS", 1ull << 20); }

// init_h (codec_encode_warm; host, K x 3 bytes): the K-means starts from these centroids; cent_out_h (host, may be null) receives the palette
static int encode_cluster_colors(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t K,
                                 const cniic_kmeans_opts *opts, uint8_t *out, uint64_t cap, uint64_t *len,
                                 cniic_kmeans_stats *stats, const uint8_t *init_h = nullptr, uint8_t *cent_out_h = nullptr) {
    const uint64_t n = (uint64_t)w * h;
    host_trace().mark("enter");
    if (n >= sp_min_pixels(c) && (reinterpret_cast<uintptr_t>(rgb_d) & 15) == 0 && !(opts && (opts->flags & CNIIC_KM_BRUTE_FORCE))) {
        if (c->timers) c->ktimes["cc_pixel_partition"].launches++;   // (stage timers: which route the call took; no duration)
        CcSession *raw = nullptr;
        CNIIC_TRY(cc_prepare_image(c, rgb_d, n, K, opts, &raw, /*may_stage=*/init_h == nullptr));   // (given centroids: the arrays as ever)
        std::unique_ptr<CcSession> s(raw);
        if (init_h) CNIIC_TRY(km_rgbw_set_centroids(s->km, init_h));
        CNIIC_TRY(km_rgbw_run(s->km, nullptr, /*may_defer=*/true));   // (cc_finish looks at how a persistent launch ended where it fetches the result)
        if (s->count_pending) CNIIC_TRY(sp_enqueue_count(c, &s->sp));
        host_trace().mark("km_run");
        const int rc_all = cc_finish(s.get(), rgb_d, w, h, nullptr, out, cap, len, stats);
        if (rc_all == CNIIC_OK && cent_out_h) CNIIC_TRY(cc_palette(s.get(), cent_out_h, nullptr));
        host_trace().dump();
        return rc_all;
    }
    // count_freqs over the pixels (clusterc.rs:21)
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, 24, &table));
    {
        ScopedKernelTimer t(c, "hist_rgb");
        CNIIC_TRY(hist_rgb_dense(c, rgb_d, n, table));
        t.stop(1);
    }
    host_trace().mark("hist (+timer sync)");
    CcSession *raw = nullptr;
    CNIIC_TRY(cc_prepare(c, table, K, opts, 0, 1, nullptr, &raw));
    std::unique_ptr<CcSession> s(raw);
    if (init_h) CNIIC_TRY(km_rgbw_set_centroids(s->km, init_h));
    CNIIC_TRY(km_rgbw_run(s->km, nullptr, /*may_defer=*/true));
    host_trace().mark("km_run");
    const int rc_all = cc_finish(s.get(), rgb_d, w, h, nullptr, out, cap, len, stats);
    if (rc_all == CNIIC_OK && cent_out_h) CNIIC_TRY(cc_palette(s.get(), cent_out_h, nullptr));
    host_trace().dump();
    return rc_all;
}

// ------------------------------------------------------------------ VoronoiCluster::encode (clusterc.rs:148-166)
static int encode_voronoi(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint32_t K, const cniic_kmeans_opts *opts,
                          uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats, const cniic_colorpos *init_h = nullptr,
                          cniic_colorpos *cent_out_h = nullptr) {
    if (K == 0) return c->fail(CNIIC_ERR_BAD_ARG, "voronoi(0)");
    std::vector<cniic_colorpos> cent(K);
    cniic_kmeans_stats st{};
    CNIIC_TRY(km_xyrgb_run(c, rgb_d, w, h, K, opts, cent.data(), nullptr, nullptr, &st, init_h));
    if (cent_out_h) memcpy(cent_out_h, cent.data(), (size_t)K * sizeof(cniic_colorpos));
    if (stats) *stats = st;
    CNIIC_TRY(check_enough_active(c, K, (uint64_t)w * h, st.active));
    std::vector<uint8_t> header;
    put_u32(header, w);            // clusterc.rs:156-158
    put_u32(header, h);
    put_u64(header, K);            // clusterc.rs:161 (usize -> u64)
    for (uint32_t k = 0; k < K; k++) {  // ColorPos::serialize clusterc.rs:250-257
        put_u32(header, cent[k].x);
        put_u32(header, cent[k].y);
        put_u64(header, 3);        // Rgb<u8> as a length-prefixed slice (ser.rs:210-214)
        header.push_back(cent[k].rgb[0]); header.push_back(cent[k].rgb[1]); header.push_back(cent[k].rgb[2]);
    }
    StreamOut so(c, out, cap, len);
    CNIIC_TRY(so.begin(header, 0));
    return so.finish();
}

// ------------------------------------------------------------------ Delta::encode (hilbertc.rs:405-415)
// The 32-bit route: symbols as packed keys (hilbert_delta + huf_encode_all_dev).  Taken when many differences fall
// outside the cube [-16, 15]^3 (a noisy image), or with CNIIC_DELTA_ROUTE=32.
static int encode_delta_syms32(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, std::vector<uint8_t> &header, uint8_t *out, uint64_t cap,
                               uint64_t *len) {
    const uint64_t n = (uint64_t)w * h;
    uint32_t *table = nullptr;
    CNIIC_TRY(dense_table(c, 27, &table));
    DevBuf syms;
    CNIIC_HIP_TRY(c, syms.alloc(n * 4));
    // one fused pass: Hilbert gather + DiffStream + count_freqs; the symbol stream is kept for the
    // second (bit-pack) pass instead of recomputing the scan as the reference does (huf.rs:30,38)
    CNIIC_TRY(hilbert_delta(c, rgb_d, w, h, syms.as<uint32_t>(), table));
    return huf_encode_all_dev(c, CNIIC_SYM_SIGNED, nullptr, syms.as<uint32_t>(), true, n, table, true, header, out, cap, len);
}

static int encode_delta(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    const uint64_t n = (uint64_t)w * h;
    std::vector<uint8_t> header;
    put_u32(header, w);
    put_u32(header, h);
    if (n == 0) return c->fail(CNIIC_ERR_BAD_ARG, "delta: empty image (src/huf.rs:99 asserts)");
    if (c->opt(CNIIC_OPT_DELTA_ROUTE, "CNIIC_DELTA_ROUTE", 0) == 32)  // the 32-bit route whatever the image (tests)
        return encode_delta_syms32(c, rgb_d, w, h, header, out, cap, len);
    host_trace().mark("delta: enter");
    // 1. linearize + DiffStream + count_freqs (hilbertc.rs:408-410, huf.rs:30): the symbols as a 16-bit stream (k_delta.hip)
    uint32_t *table = nullptr;
    uint8_t *pages = nullptr;
    CNIIC_TRY(delta_table(c, &table, &pages));
    DevBuf hot16, coldkeys, chunk_cold, small;
    const uint64_t nchunks = delta_stream_len(n) / 512;
    CNIIC_HIP_TRY(c, hot16.alloc(delta_stream_len(n) * 2));
    CNIIC_HIP_TRY(c, coldkeys.alloc(nchunks * 64 * 4));  // (written where cold symbols are)
    CNIIC_HIP_TRY(c, chunk_cold.alloc(nchunks));
    CNIIC_HIP_TRY(c, small.alloc(32));  // u64 [0]: a chunk with more than 64 cold symbols, [2]: the codes' totals, then bits packed, [3]: a code is too long
    CNIIC_HIP_TRY(c, hipMemsetAsync(small.p, 0, 32, c->stream));
    uint64_t *const packed_d = small.as<uint64_t>() + 2;
    CNIIC_TRY(delta_gather_hist(c, rgb_d, w, h, hot16.as<uint16_t>(), table, pages, coldkeys.as<uint32_t>(), chunk_cold.as<uint8_t>(),
                                small.as<uint32_t>()));
    CNIIC_HIP_TRY(c, c->pinned_u.reserve(kPinnedUBytes, kPinnedUBytes));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuDeltaOverflow.at, small.p, 8, hipMemcpyDeviceToHost, c->stream));
    host_trace().mark("delta: gather + hist enqueued");
    // (stage timers, bench.py --config c5: everything between the histogram and the pack -- compaction, the leaves' sort, the host's merge with
    // the GPU idle, the codes -- as ONE stage, so that the stages account for the whole call)
    ScopedKernelTimer timer_tree(c, "delta_tree");
    CompactPlan plan;
    CNIIC_TRY(hist_compact_count(c, table, 27, &plan, nullptr, pages));  // (waits for the stream)
    host_trace().mark("delta: ... + count of the distinct (wait)");
    const bool overflow = c->pinned_u.as<uint64_t>()[kPuDeltaOverflow.at] != 0;
    if (host_trace().on) fprintf(stderr, "[host] delta: %llu symbols, %llu distinct%s\n", (unsigned long long)n, (unsigned long long)plan.n_unique,
                                 overflow ? " (a chunk with more than 64 symbols outside the cube: the 32-bit route)" : "");
    if (plan.n_unique >= (1ull << 26) || overflow) {
        CNIIC_TRY(delta_table_clean(c));
        return encode_delta_syms32(c, rgb_d, w, h, header, out, cap, len);
    }
    HuffCodeStage st(c, CNIIC_SYM_SIGNED);
    CNIIC_TRY(st.begin(table, &plan, n));
    const uint64_t U = st.U, header_bytes = header.size() + st.decoder_bytes();
    uint32_t *const keys_d = st.keys_d.as<uint32_t>();
    const uint8_t *const len_d = st.len_d.as<uint8_t>();
    const uint64_t *const code_d = st.code_d.as<uint64_t>();
    CNIIC_HIP_TRY(c, ctx_spin_sync(c));
    host_trace().mark("delta: compaction + D2H (wait)");
    // 2. build() (huf.rs:31); 3. the payload (huf.rs:37-41) behind the serialised decoder (huf.rs:34)
    CNIIC_TRY(st.build(packed_d));
    DeltaPackScratch scratch;
    bool counted = false;   // the first half of the pack is already in the stream
    if (st.totals_pending) {
        // (round 4) the payload's size is on its way to the host: the first half of the pack, which wants the codes and nothing else, is
        // enqueued behind it, and the host waits for the size while the GPU counts
        CNIIC_HIP_TRY(c, c->res_ev.ensure(hipEventDisableTiming));
        CNIIC_HIP_TRY(c, hipEventRecord(c->res_ev, c->stream));
        if (!c->timers) {   // (with the stage timers on the whole pack is timed as one stage below)
            CNIIC_HIP_TRY(c, hipMemsetAsync(packed_d, 0, 8, c->stream));
            CNIIC_TRY(delta_pack16_count(c, hot16.as<uint16_t>(), n, coldkeys.as<uint32_t>(), chunk_cold.as<uint8_t>(), table, keys_d, len_d, code_d, U, packed_d, &scratch));
            counted = true;
        }
        hipError_t e;
        while ((e = hipEventQuery(c->res_ev)) == hipErrorNotReady) {}
        CNIIC_HIP_TRY(c, e);
    }
    uint64_t nbits = 0;
    CNIIC_TRY(st.bits(&nbits));
    CNIIC_TRY(st.upload_codes());
    StreamOut so(c, out, cap, len);
    CNIIC_TRY(so.begin_sized(header_bytes, (nbits + 7) / 8, /*zero=*/false));  // (the pack stores every word of the payload)
    if (!counted) CNIIC_HIP_TRY(c, hipMemsetAsync(packed_d, 0, 8, c->stream));
    timer_tree.stop(1);
    if (nbits) {  // (a single symbol: the zero-length code and no payload, huf.rs:140-142)
        ScopedKernelTimer timer(c, "huff_pack");   // (with the count already enqueued this times the second half alone; bench.py's stage figure says so)
        if (!counted)
            CNIIC_TRY(delta_pack16_count(c, hot16.as<uint16_t>(), n, coldkeys.as<uint32_t>(), chunk_cold.as<uint8_t>(), table, keys_d, len_d, code_d, U, packed_d, &scratch));
        CNIIC_TRY(delta_pack16_write(c, hot16.as<uint16_t>(), n, coldkeys.as<uint32_t>(), len_d, code_d, so.dev, header_bytes * 8, &scratch));
        timer.stop(1);
    }
    ScopedKernelTimer timer_fin(c, "delta_finish");   // (the table's sweep, the header, the decoder, the last wait)
    CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_u.as<uint64_t>() + kPuDeltaPacked.at, packed_d, 8, hipMemcpyDeviceToHost, c->stream));
    CNIIC_TRY(delta_table_clean(c));
    host_trace().mark("delta: pack enqueued");
    // the decoder goes in AFTER the pack, whose first word comes out with zeros where the decoder's last bytes are
    // (a small alphabet's is written out by the host here, while the GPU packs)
    CNIIC_TRY(st.write_decoder(so, header));
    if (!st.gpu_codes && header.size() != header_bytes)
        return c->fail(CNIIC_ERR_HIP, "delta: decoder of %llu bytes, expected %llu", (unsigned long long)header.size(), (unsigned long long)header_bytes);
    const int rc_fin = so.finish();  // (waits for the stream)
    timer_fin.stop(1);
    host_trace().mark("delta: pack + finish");
    host_trace().dump();
    if (rc_fin != CNIIC_OK) return rc_fin;
    const uint64_t packed_bits = c->pinned_u.as<uint64_t>()[kPuDeltaPacked.at];
    if (packed_bits != nbits)
        return c->fail(CNIIC_ERR_HIP, "huffman: packed %llu bits, histogram predicts %llu", (unsigned long long)packed_bits, (unsigned long long)nbits);
    return CNIIC_OK;
}

// ------------------------------------------------------------------ Hilbert{RLE(d)}::encode (hilbertc.rs:26-45): d == 0.0 (-0.0 too) takes the
// exact branch (:33-39), any other d (negative, NaN and infinite ones included) the running average (:40-45, rle_approx :200-299)
int encode_hilbert_rle(Ctx *c, double d, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    const uint64_t n = (uint64_t)w * h;
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "image too large");
    const bool exact = d == 0.0;
    std::vector<uint8_t> header;
    put_u32(header, w);  // img.dimensions().serialize (:27)
    put_u32(header, h);
    StreamOut so(c, out, cap, len);
    if (n == 0) {
        CNIIC_TRY(so.begin(header, 0));
        return so.finish();
    }
    DevBuf lin;
    CNIIC_HIP_TRY(c, lin.alloc(n * 3));
    CNIIC_TRY(hilbert_linearize(c, rgb_d, w, h, lin.as<uint8_t>()));  // hilbert::linearize (:29)
    RlePlan plan;
    CNIIC_TRY(exact ? rle_plan(c, lin.as<uint8_t>(), n, &plan) : rle_approx_plan(c, lin.as<uint8_t>(), n, d, &plan));  // rle_exact (:34) / rle_approx (:41)
    CNIIC_TRY(so.begin_sized(header.size(), plan.nruns * 12, /*zero=*/false));  // count.serialize + color.serialize per run (:35-36, :42-43):
    CNIIC_TRY(so.put_header(header));                                            // three whole words each, nothing left to clear
    uint32_t *const records = reinterpret_cast<uint32_t *>(so.dev + header.size());
    CNIIC_TRY(exact ? rle_emit(c, lin.as<uint8_t>(), &plan, records) : rle_approx_emit(c, lin.as<uint8_t>(), &plan, records));
    return so.finish();
}

int codec_encode(Ctx *c, const CodecDesc &d, const uint8_t *rgb_d, uint32_t w, uint32_t h, const cniic_kmeans_opts *opts,
                 uint8_t *out, uint64_t cap, uint64_t *len, cniic_kmeans_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if ((uint64_t)w * h >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "image too large");
    struct TimersScope {  // stage timers for this call when the options ask for profiling
        Ctx *c; bool saved;
        TimersScope(Ctx *ctx, bool on) : c(ctx), saved(ctx->timers) { c->timers = saved || on; }
        ~TimersScope() { c->timers = saved; }
    } timers_scope(c, opts && (opts->flags & CNIIC_KM_PROFILE));
    switch (d.kind) {
    case CODEC_HUFMAN: return encode_hufman(c, rgb_d, w, h, out, cap, len);
    case CODEC_CLUSTER_COLORS: return encode_cluster_colors(c, rgb_d, w, h, d.arg, opts, out, cap, len, stats);
    case CODEC_VORONOI: return encode_voronoi(c, rgb_d, w, h, d.arg, opts, out, cap, len, stats);
    case CODEC_DELTA: return encode_delta(c, rgb_d, w, h, out, cap, len);
    case CODEC_HILBERT_RLE: return encode_hilbert_rle(c, d.darg, rgb_d, w, h, out, cap, len);
    case CODEC_ZIP_DICT: return encode_zip_dict(c, rgb_d, w, h, out, cap, len);
    case CODEC_HILBERT_ZIP: return encode_hilbert_zip(c, rgb_d, w, h, out, cap, len);
    }
    return c->fail(CNIIC_ERR_BAD_ARG, "unknown codec");
}

// codec_encode for the two K-means codecs with the run started from the caller's centroids (cniic_codec_encode_warm): init_h / cent_out_h are host
// arrays of K entries, K x 3 bytes for cluster-colors and K cniic_colorpos for voronoi; cent_out_h may be null.  Any other codec: BAD_ARG.
int codec_encode_warm(Ctx *c, const CodecDesc &d, const uint8_t *rgb_d, uint32_t w, uint32_t h, const cniic_kmeans_opts *opts, const void *init_h,
                      uint8_t *out, uint64_t cap, uint64_t *len, void *cent_out_h, cniic_kmeans_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (d.kind != CODEC_CLUSTER_COLORS && d.kind != CODEC_VORONOI)
        return c->fail(CNIIC_ERR_BAD_ARG, "codec_encode_warm: only cluster-colors(K) and voronoi(K) run a K-means");
    if ((uint64_t)w * h >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "image too large");
    if (d.kind == CODEC_CLUSTER_COLORS)
        return encode_cluster_colors(c, rgb_d, w, h, d.arg, opts, out, cap, len, stats, static_cast<const uint8_t *>(init_h), static_cast<uint8_t *>(cent_out_h));
    return encode_voronoi(c, rgb_d, w, h, d.arg, opts, out, cap, len, stats, static_cast<const cniic_colorpos *>(init_h), static_cast<cniic_colorpos *>(cent_out_h));
}

// ------------------------------------------------------------------ decode
// below this many symbols the parallel decoder's fixed cost is not worth it (CNIIC_GPU_DECODE_MIN overrides: tests)
static uint64_t gpu_decode_min_symbols(const Ctx *c) { return c->opt(CNIIC_OPT_GPU_DECODE_MIN, "CNIIC_GPU_DECODE_MIN", 1ull << 14); }

static int put_image(Ctx *c, const uint8_t *src, bool src_dev, uint64_t bytes, uint8_t *dst) {
    if (!bytes) return CNIIC_OK;
    const bool dst_dev = is_device_ptr(dst);
    hipMemcpyKind kind = src_dev ? (dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)
                                 : (dst_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost);
    CNIIC_HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// The stream may live in host memory or in HBM (bytes_dev).  Only the HEAD of a device-resident stream comes to the host -- the
// dimensions and, for the Huffman codecs, the serialised decoder, which is parsed there (O(alphabet)); the payload is decoded
// where it lies.  head_h / head_n: the part of the stream the host can read (all of it for a host stream).
struct StreamHead {
    const uint8_t *p = nullptr;
    uint64_t n = 0;
};
// the first `want` bytes of the stream where the host can read them: the stream itself, or (device-resident) a copy in the
// context's pinned block (a pageable landing buffer costs the copy a staging pass and ~40 us)
static int stream_head(Ctx *c, const uint8_t *bytes, bool bytes_dev, uint64_t nbytes, uint64_t want, StreamHead *h) {
    want = std::min(want, nbytes);
    // (a host stream is all there, but the decoder is looked for in its head only, like a device stream's: one that does not end
    // there has hundreds of thousands of leaves and is parsed faster on the GPU than by this core)
    if (!bytes_dev) { h->p = bytes; h->n = std::max(h->n, want); return CNIIC_OK; }
    if (h->n >= want) return CNIIC_OK;
    CNIIC_HIP_TRY(c, c->pinned_huf.reserve(want, pinned_huf_want(want)));
    CNIIC_HIP_TRY(c, hipMemcpyAsync(c->pinned_huf.p, bytes, want, hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    h->p = c->pinned_huf.as<const uint8_t>();
    h->n = want;
    return CNIIC_OK;
}

constexpr uint64_t kTrieSecondLook = 512ull << 10;   // bytes of a `delta` stream the host parses before the GPU is asked (~7 10^4 leaves)
int codec_decode(Ctx *c, const CodecDesc &d, const uint8_t *bytes, uint64_t nbytes, uint8_t *rgb_out, uint64_t cap,
                 uint32_t *w, uint32_t *h) {
    if (d.kind == CODEC_ZIP_DICT) return decode_zip_dict(c, bytes, nbytes, rgb_out, cap, w, h);   // (its dimensions are inside the compressed text)
    if (d.kind == CODEC_HILBERT_ZIP) return decode_hilbert_zip(c, bytes, nbytes, rgb_out, cap, w, h);   // (lenient: its own rules from the dimensions on)
    const bool bytes_dev = is_device_ptr(bytes);
    StreamHead head;
    // (the serialised decoder of a Huffman stream is at most a few per cent of it, for the images these codecs are meant for)
    CNIIC_TRY(stream_head(c, bytes, bytes_dev, nbytes, std::min<uint64_t>(std::max<uint64_t>(nbytes / 48, 8192), 4ull << 20), &head));
    uint64_t pos = 0;
    if (!get_u32(head.p, head.n, pos, *w) || !get_u32(head.p, head.n, pos, *h))  // create_image_buffer_standard codec.rs:22-26
        return c->fail(CNIIC_ERR_DECODE, "decode: truncated dimensions");
    const uint64_t n = (uint64_t)*w * *h;
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_DECODE, "decode: image too large");
    if (n * 3 > cap) return c->fail(CNIIC_ERR_CAPACITY, "decode: image needs %llu bytes, capacity %llu",
                                    (unsigned long long)(n * 3), (unsigned long long)cap);
    switch (d.kind) {
    case CODEC_HUFMAN:
    case CODEC_CLUSTER_COLORS:   // clusterc.rs:55-57 delegates to Hufman.decode (hufc.rs:19-40)
    case CODEC_DELTA: {          // hilbertc.rs:417-431
        const bool delta = d.kind == CODEC_DELTA;
        const int sym_kind = delta ? CNIIC_SYM_SIGNED : CNIIC_SYM_RGB;
        const char *bad_stream = delta ? "delta: cannot decode the difference stream" : "Failed to decode symbol";
        host_trace().mark("decode: enter");
        if (!c->trie_scratch) c->trie_scratch = std::make_shared<LeafTable>();
        LeafTable &lt = *static_cast<LeafTable *>(c->trie_scratch.get());
        // the decoder: parsed from what the host holds of the stream; a device-resident stream whose decoder is longer than
        // that is fetched further (a failed parse of a TRUNCATED head says nothing: only the whole stream's verdict counts)
        uint64_t tpos = pos;
        bool parsed = huff_parse_leaves(sym_kind, head.p, head.n, tpos, lt);
        const bool dst_dev = is_device_ptr(rgb_out);
        int status = 2;
        DevBuf keys_d, lin_d, img_d, stream_up, tab_big;
        UdSums ud_sums;   // (delta: FromDiff's chunk sums, when the decoder added them up on its way)
        uint8_t *dst = rgb_out;
        auto need_image = [&]() -> int {   // where the pixels are produced: the caller's image if it is in HBM and word-aligned
            if (!img_d.p && (!dst_dev || (reinterpret_cast<uintptr_t>(rgb_out) & 3))) { CNIIC_HIP_TRY(c, img_d.alloc(n * 3)); dst = img_d.as<uint8_t>(); }
            return CNIIC_OK;
        };
        const bool force_gpu_parse = test_env("CNIIC_TEST_TRIE_GPU") != nullptr;   // tests: every decoder through k_trieparse.hip
        // A `delta` decoder of a photograph has 4-6 10^4 leaves (0.3-0.5 MB): more than the head that was looked at, far fewer than the
        // GPU parse needs to pay for its launches and waits (0.49 ms at 4 10^4 leaves; this core parses them in 0.15) -- a second, longer
        // look before the stream goes to k_trieparse.hip.  (`hufman` decoders that outgrow the first look are ten times that size.)
        if (!parsed && !force_gpu_parse && head.n < nbytes) {
            const char *e2 = test_env("CNIIC_TRIE_HOST_SECOND");
            // (whatever the stream's length: the decoder's share of it grows as the image shrinks -- 57 % at 512^2 -- and a photograph's
            // alphabet stays under 6 10^4 differences at any size.  Uniform noise, whose decoder is most of the stream, paid for the look in
            // vain -- 0.33 ms; see `worth`.)
            // A stream of more than 6 bytes a pixel is mostly decoder (the payload has at most 27 bits a symbol): more leaves than the look
            // could hold, unless the whole stream fits into it.
            const bool worth = nbytes <= kTrieSecondLook || nbytes <= 6 * n;
            const uint64_t second = e2 ? strtoull(e2, nullptr, 10) : delta && worth ? std::min<uint64_t>(kTrieSecondLook, nbytes) : 0;
            if (second > head.n) {
                CNIIC_TRY(stream_head(c, bytes, bytes_dev, nbytes, second, &head));
                tpos = pos;
                parsed = huff_parse_leaves(sym_kind, head.p, head.n, tpos, lt);
                host_trace().mark("decode: second look at the decoder (host)");
            }
        }
        if (force_gpu_parse || (!parsed && head.n < nbytes)) {
            // The decoder is longer than the head of the stream that was looked at (4 MiB at most): an alphabet of hundreds of
            // thousands of symbols -- `hufman` on a photograph.  Parsed on the GPU (k_trieparse.hip), from the stream in HBM.
            bool done_dev = false;
            if (n >= gpu_decode_min_symbols(c)) {
                const uint8_t *sd = bytes;
                if (!bytes_dev) {
                    CNIIC_HIP_TRY(c, stream_up.alloc(nbytes + 16));
                    CNIIC_HIP_TRY(c, hipMemcpyAsync(stream_up.p, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
                    sd = stream_up.as<uint8_t>();
                }
                uint64_t nl = 0, off_key = 0, off_len = 0, ppos = 0;
                uint32_t max_len = 0;
                int pst = 1;
                CNIIC_TRY(huff_parse_leaves_dev(c, sym_kind, sd, nbytes, pos, &tab_big, &nl, &off_key, &off_len, &max_len, &ppos, &pst));
                host_trace().mark("decode: parse the decoder (GPU)");
                if (pst == 1) return c->fail(CNIIC_ERR_DECODE, bad_stream);
                if (pst == 0) {
                    if (!n) return CNIIC_OK;
                    CNIIC_TRY(need_image());
                    if (delta) CNIIC_HIP_TRY(c, keys_d.alloc(n * 4));
                    uint32_t key0 = 0;   // (a one-symbol alphabet is filled in, not decoded: its key is wanted here)
                    if (nl == 1) {
                        CNIIC_HIP_TRY(c, hipMemcpyAsync(&key0, tab_big.as<uint8_t>() + off_key, 4, hipMemcpyDeviceToHost, c->stream));
                        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
                    }
                    CNIIC_TRY(huff_decode_tables_dev(c, tab_big.as<uint8_t>(), nl, off_key, off_len, max_len, key0, sd + ppos, true, nbytes - ppos, n,
                                                     delta ? 0 : 1, delta ? keys_d.p : (void *)dst, &status, delta ? &ud_sums : nullptr));
                    done_dev = status != 2;
                }
                // which parse answered (tests): the GPU's table, or the host's walk after the GPU parse was tried
                if (c->timers) c->ktimes[done_dev ? "trie_parse" : "trie_parse_host"].launches += 1;
            }
            if (!done_dev) {  // the host's way: the whole stream there
                if (bytes_dev) head.n = 0;
                CNIIC_TRY(stream_head(c, bytes, bytes_dev, nbytes, nbytes, &head));
                tpos = pos;
                parsed = huff_parse_leaves(sym_kind, head.p, head.n, tpos, lt);
                if (!parsed) return c->fail(CNIIC_ERR_DECODE, bad_stream);
                lt.too_deep = true;   // (whatever was tried on the GPU did not work out: the node walk below)
            }
        } else {
            if (!parsed) return c->fail(CNIIC_ERR_DECODE, bad_stream);
            host_trace().mark("decode: parse the decoder (host)");
            if (!lt.too_deep) {
                if (!n) return CNIIC_OK;
                CNIIC_TRY(need_image());
                if (delta) CNIIC_HIP_TRY(c, keys_d.alloc(n * 4));
                // symbols on the GPU (parallel, self-synchronising), straight from the stream where it lies; small inputs and codes
                // that do not settle go through the host walk (same answers)
                if (n >= gpu_decode_min_symbols(c))
                    CNIIC_TRY(huff_decode_dev(c, lt, bytes + tpos, bytes_dev, nbytes - tpos, n, delta ? 0 : 1, delta ? keys_d.p : (void *)dst, &status, delta ? &ud_sums : nullptr));
            }
        }
        if (status == 2) {  // the node walk on the host: needs the whole stream there
            if (c->timers) c->ktimes["hd_host_walk"].launches++;   // (stage timers: the host's walk decoded the payload; no duration)
            ud_sums.filled = false;
            if (bytes_dev) head.n = 0;  // (the pinned block the head was fetched into has served other purposes since: fetch again)
            CNIIC_TRY(stream_head(c, bytes, bytes_dev, nbytes, nbytes, &head));
            std::vector<TrieNode> trie;
            if (!huff_parse_trie(sym_kind, head.p, head.n, pos, trie)) return c->fail(CNIIC_ERR_DECODE, bad_stream);
            if (!n) return CNIIC_OK;
            CNIIC_TRY(need_image());
            CNIIC_HIP_TRY(c, keys_d.alloc(n * 4));
            std::vector<uint32_t> keys(n);
            if (!huff_decode_host(trie, head.p + pos, head.n - pos, n, keys.data(), nullptr)) status = 1;
            else {
                status = 0;
                CNIIC_HIP_TRY(c, hipMemcpyAsync(keys_d.p, keys.data(), n * 4, hipMemcpyHostToDevice, c->stream));
                CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
                if (!delta) CNIIC_TRY(keys_to_rgb(c, keys_d.as<uint32_t>(), n, dst));
            }
        }
        if (status == 1) return c->fail(CNIIC_ERR_DECODE, bad_stream);
        host_trace().mark("decode: symbols");
        if (delta) {
            uint32_t bad = 0;  // START (hilbertc.rs:445); FromDiff (hilbertc.rs:496-508); then follow the traversal (hilbertc.rs:426-428)
            ScopedKernelTimer tu(c, "undiff_scatter");
            CNIIC_TRY(delta_undiff_scatter_dev(c, keys_d.as<uint32_t>(), *w, *h, dst, &bad, &ud_sums));
            tu.stop();
            if (bad) return c->fail(CNIIC_ERR_DECODE, "delta: colour out of range (hilbertc.rs:505)");
        }
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        host_trace().mark("decode: pixels");
        const int rc_put = dst == rgb_out ? CNIIC_OK : put_image(c, dst, true, n * 3, rgb_out);
        host_trace().mark("decode: image out");
        host_trace().dump();
        return rc_put;
    }
    case CODEC_HILBERT_RLE: {  // hilbertc.rs:53-79: RleDecoder (:304-337) zipped with hilbert::iter
        if (!n) return CNIIC_OK;
        // pixels the stream does not reach stay zero (ImageBuffer::new); RepCount::deserialize(..)? ends it quietly
        const uint64_t body = nbytes - pos, R = body / 12, tail = body % 12;
        DevBuf rec_d, lin_d, img_d;
        const uint8_t *recs = bytes + pos;   // (a stream in HBM whose records are 4-byte aligned is read where it lies: 3.2 GB at 16384^2)
        if (!bytes_dev || (reinterpret_cast<uintptr_t>(recs) & 3)) {
            CNIIC_HIP_TRY(c, rec_d.alloc(std::max<uint64_t>(R * 12, 16)));
            if (R) CNIIC_HIP_TRY(c, hipMemcpyAsync(rec_d.p, bytes + pos, R * 12, bytes_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
            recs = rec_d.as<uint8_t>();
        }
        CNIIC_HIP_TRY(c, lin_d.alloc(n * 3));
        int status = 0;
        CNIIC_TRY(rle_expand_dev(c, recs, R, tail, n, lin_d.as<uint8_t>(), &status));
        if (status)
            return c->fail(CNIIC_ERR_DECODE, "hilbert-rle: bad run record (assert!(count > 0) / unwrap, hilbertc.rs:327-328)");
        uint8_t *dst = rgb_out;
        const bool dst_dev = is_device_ptr(rgb_out);
        if (!dst_dev) { CNIIC_HIP_TRY(c, img_d.alloc(n * 3)); dst = img_d.as<uint8_t>(); }
        CNIIC_TRY(hilbert_scatter(c, lin_d.as<uint8_t>(), *w, *h, dst));  // follow the traversal (:58-61)
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!dst_dev) return put_image(c, dst, true, n * 3, rgb_out);
        return CNIIC_OK;
    }
    case CODEC_ZIP_DICT: break;   // (taken above)
    case CODEC_HILBERT_ZIP: break;
    case CODEC_VORONOI: {  // clusterc.rs:168-189
        CNIIC_TRY(stream_head(c, bytes, bytes_dev, nbytes, nbytes, &head));  // 16 + 19 K bytes: parsed on the host
        const uint8_t *hb = head.p;
        uint64_t K;
        std::vector<cniic_colorpos> cent;
        switch (vor_parse_head(hb, nbytes, pos, &K, [&](uint64_t k, uint32_t x, uint32_t y, uint8_t r, uint8_t g, uint8_t b) {
                    if (!k) cent.reserve(K);
                    cent.push_back(cniic_colorpos{x, y, {r, g, b}, 0});
                })) {
        case VorHead::Truncated: return c->fail(CNIIC_ERR_DECODE, "voronoi: truncated");
        case VorHead::TruncatedList: return c->fail(CNIIC_ERR_DECODE, "voronoi: truncated centroid list");
        case VorHead::BadCentroid: return c->fail(CNIIC_ERR_DECODE, "voronoi: bad centroid");
        case VorHead::Ok: break;
        }
        if (!n) return CNIIC_OK;
        if (K == 0) return c->fail(CNIIC_ERR_DECODE, "voronoi: no centroids (min_by_key().unwrap(), clusterc.rs:184)");
        if (K > 0xffffffffull) return c->fail(CNIIC_ERR_DECODE, "voronoi: too many centroids");
        DevBuf cent_d, img_d;
        CNIIC_HIP_TRY(c, cent_d.alloc(K * sizeof(cniic_colorpos)));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(cent_d.p, cent.data(), K * sizeof(cniic_colorpos), hipMemcpyHostToDevice, c->stream));
        uint8_t *dst = rgb_out;
        const bool dst_dev = is_device_ptr(rgb_out);
        if (!dst_dev) { CNIIC_HIP_TRY(c, img_d.alloc(n * 3)); dst = img_d.as<uint8_t>(); }
        bool small_coords = vp_sides_small(*w, *h);  // then the pruned repaint is exact (vor_paint.hpp, k_misc.hip)
        for (uint64_t k = 0; k < K && small_coords; k++) small_coords = vp_coord_small(cent[k].x, cent[k].y);
        CNIIC_TRY(voronoi_paint(c, cent_d.as<cniic_colorpos>(), (uint32_t)K, *w, *h, dst, small_coords));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!dst_dev) return put_image(c, dst, true, n * 3, rgb_out);
        return CNIIC_OK;
    }
    }
    return c->fail(CNIIC_ERR_BAD_ARG, "unknown codec");
}

// ------------------------------------------------------------------ decode of many streams: what the routes of a batch share
// One cniic_codec_decode_batch call.  codec_decode_batch_route (at the end of this file) builds it once; every route takes it by reference.
struct DecodeBatch {
    Ctx *c;
    const uint8_t *bytes; bool bytes_dev; uint64_t stride; const uint64_t *lens; uint32_t F;   // the streams: frame f at f * stride, lens[f] bytes of it
    uint8_t *rgb; bool dst_dev; uint64_t img_stride; uint32_t *w, *h;                           // the images: frame f at f * img_stride
    std::vector<uint8_t> &taken; std::vector<int32_t> &rcs; std::vector<std::string> &msgs;     // per frame: the route's, its status, its message
    std::vector<uint8_t> off_route;   // tests (CNIIC_TEST_DECODE_BATCH_OFF=i,j,..): these frames through the single-stream decode
    const uint8_t *stream(uint32_t f) const { return bytes + (uint64_t)f * stride; }
    uint8_t *image(uint32_t f) const { return rgb + (uint64_t)f * img_stride; }
    uint64_t view(uint32_t f) const { return std::min(lens[f], stride); }   // what a look at frame f alone may read of a batch in HBM
    uint64_t pixels(uint32_t f) const { return (uint64_t)w[f] * h[f]; }
    uint64_t image_bytes(uint32_t f) const { return pixels(f) * 3; }
    void decode_error(uint32_t f, const char *msg) const { rcs[f] = CNIIC_ERR_DECODE; msgs[f] = msg; }
};

// The streams of frames first .. last (ascending) in HBM: *base + f * stride is frame f's.  A batch in HBM is read where it lies; a host
// batch goes up from the first frame to the last one's end, in one copy, into `keep`.
static int streams_in_hbm(const DecodeBatch &b, uint32_t first, uint32_t last, DevBuf &keep, const uint8_t **base) {
    *base = b.bytes;
    if (b.bytes_dev) return CNIIC_OK;
    const ByteSpan s = frames_span(first, last, b.stride, b.lens);
    CNIIC_HIP_TRY(b.c, keep.alloc(s.hi - s.lo + 16));
    CNIIC_HIP_TRY(b.c, hipMemcpyAsync(keep.p, b.bytes + s.lo, s.hi - s.lo, hipMemcpyHostToDevice, b.c->stream));
    *base = keep.as<uint8_t>() - s.lo;
    return CNIIC_OK;
}

// The images of a chunk's frames that cannot be written where the caller wants them: slots of one block in HBM (SlotLayout), and the two ways
// the routes bring them down -- the whole block in one copy before the wait and a memcpy per frame behind it (down_block, put), or a copy
// per frame (down_each).
struct StagedImages {
    SlotLayout lay;
    DevBuf dev;
    std::vector<uint8_t> host;
    explicit StagedImages(size_t frames) : lay(frames) {}
    void plan(size_t i, uint64_t bytes, bool needed) { lay.plan(i, bytes, needed); }
    hipError_t alloc(Ctx *) { return lay.total ? dev.alloc(lay.total) : hipSuccess; }   // (nothing when no frame needed a slot)
    uint8_t *dst(size_t i, uint8_t *own) const { return lay.has(i) ? dev.as<uint8_t>() + lay.at[i] : own; }
    hipError_t down_block(Ctx *c) { host.resize(lay.total); return lay.total ? hipMemcpyAsync(host.data(), dev.p, lay.total, hipMemcpyDeviceToHost, c->stream) : hipSuccess; }
    void put(size_t i, uint8_t *own, uint64_t n) const { if (lay.has(i)) memcpy(own, host.data() + lay.at[i], n); }
    hipError_t down_each(Ctx *c, size_t i, uint8_t *own, uint64_t n, hipMemcpyKind kind) const {
        return lay.has(i) ? hipMemcpyAsync(own, dev.as<uint8_t>() + lay.at[i], n, kind, c->stream) : hipSuccess;
    }
};

// The heads: where the host reads frame f (head_p[f], head_n[f] bytes of it; nothing until a look has been taken).  A host batch is read
// where it lies.  The heads of a batch in HBM come into the context's pinned block, c->pinned_huf, and that block has other users:
// delta_small_decode assembles its upload block there, small_parse_dev its rows.  The order of the calls is what keeps them apart -- a
// route runs only when the host's parse of the heads is done, and small_parse_dev reads rows[i].table before it calls delta_small_decode.
constexpr uint64_t kBatchHeadsMax = 256ull << 20;   // pinned bytes the heads of one batch may take (a second look is cut to fit)
struct Heads {
    const DecodeBatch &b;
    std::vector<const uint8_t *> head_p;
    std::vector<uint64_t> head_n;
    explicit Heads(const DecodeBatch &batch) : b(batch), head_p(batch.F), head_n(batch.F) {}
    void in_place() { for (uint32_t f = 0; f < b.F; f++) { head_p[f] = b.stream(f); head_n[f] = b.lens[f]; } }
    // the first W bytes of frames [f0, f1] into the pinned block, row f at (f - f0) W
    int fetch(uint64_t W, uint32_t f0, uint32_t f1) {
        Ctx *c = b.c;
        const uint32_t F = b.F;
        CNIIC_HIP_TRY(c, c->pinned_huf.reserve(W * (f1 - f0 + 1), pinned_huf_want(W * (f1 - f0 + 1))));
        uint8_t *ph = c->pinned_huf.as<uint8_t>();
        const uint32_t last = F >= 2 ? std::min(f1, F - 2) : 0;   // (the batch's last frame may end before W bytes: a copy of its own)
        if (F >= 2 && f0 <= last)
            CNIIC_HIP_TRY(c, hipMemcpy2DAsync(ph, W, b.stream(f0), b.stride, W, last - f0 + 1, hipMemcpyDeviceToHost, c->stream));
        if (f1 == F - 1) {
            const uint64_t n1 = std::min(W, b.lens[F - 1]);
            if (n1) CNIIC_HIP_TRY(c, hipMemcpyAsync(ph + (uint64_t)(F - 1 - f0) * W, b.stream(F - 1), n1, hipMemcpyDeviceToHost, c->stream));
        }
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (uint32_t f = f0; f <= f1; f++) { head_p[f] = ph + (uint64_t)(f - f0) * W; head_n[f] = std::min(W, b.lens[f]); }
        return CNIIC_OK;
    }
    bool dims(uint32_t f, uint32_t *fw, uint32_t *fh, uint64_t *pos) const { return frame_dims(head_p[f], head_n[f], fw, fh, pos); }
};

// ------------------------------------------------------------------ `hilbert(rle)` frames of a batch (whatever d they were written with)
// The same 12-byte records at a fixed place behind the 8-byte header: nothing to parse.  A frame is taken when its header is there
// (lens[f] >= 8), 0 < w h <= kRleBatchMaxPx and the image fits img_stride; the others are the caller's (its single decode answers for
// them).  kRleBatchMaxPx is where the route stopped paying when it was measured against the worker contexts on batches of one frame
// size (tools/batch_var_probe.py --hilbert --sweep, profiles/batch_var_probe_hilbert.json): 5.3x at 64 x 64, 3.9x at 256 x 256 and 1.23x
// at 512 x 384 (196 608 pixels), but 0.92x at 800 x 600 (480 000) and 0.87x on 100 images of DIV2K's sizes -- from there on a frame's
// time is its scatter along the scan, which this route runs one after the other on one stream and eight workers run side by side.  The
// taken frames are worked through in sets -- at most kBatchRouteFrames frames and kRleSetScratch bytes of scratch (records' offsets +
// colours in scan order; a frame that needs more is a set of its own) -- each of them ONE set of launches for the expansion
// (rle_expand_batch_dev), then a scatter per frame along its scan on the same stream (an injected scan applies to the frames of its
// size), the copies out, and one wait.
constexpr size_t kBatchRouteFrames = 4096;          // frames per set of launches
constexpr uint64_t kRleSetScratch = 2ull << 30;
constexpr uint64_t kRleBatchMaxPx = 1ull << 18;   // 2^18 = 262 144 pixels: between the last size that won and the first that lost
static int rle_batch(DecodeBatch &b) {
    Ctx *c = b.c;
    Heads heads(b);   // the records follow the dimensions: the host reads those 8 bytes and nothing else
    if (!b.bytes_dev) heads.in_place();
    else if (b.stride >= 8 || b.F == 1) CNIIC_TRY(heads.fetch(8, 0, b.F - 1));   // (else headers that overlap: every frame to the single decode)
    std::vector<uint32_t> route;
    for (uint32_t f = 0; f < b.F; f++) {
        if (b.off_route[f] || b.lens[f] < 8) continue;
        uint64_t pos;
        uint32_t fw, fh;
        if (!heads.dims(f, &fw, &fh, &pos) || !dims_fit((uint64_t)fw * fh, kRleBatchMaxPx, b.img_stride)) continue;
        b.w[f] = fw; b.h[f] = fh;
        route.push_back(f);
    }
    auto scratch_of = [&](uint32_t f) {   // offsets (4 bytes per record) + colours + a staged image, each rounded up
        return (b.lens[f] - 8) / 12 * 4 + 2 * SlotLayout::room(b.image_bytes(f)) + (b.bytes_dev ? 0 : b.lens[f]);
    };
    for (size_t i0 = 0; i0 < route.size();) {
        const size_t i1 = take_chunk(i0, std::min(route.size(), i0 + kBatchRouteFrames), kRleSetScratch, [&](size_t i) { return scratch_of(route[i]); });
        const size_t S = i1 - i0;
        // ---- the streams in HBM, the colours and staged images
        DevBuf up_d, lin_d;
        const uint8_t *base;
        CNIIC_TRY(streams_in_hbm(b, route[i0], route[i1 - 1], up_d, &base));
        std::vector<RleBatchFrame> bf(S);
        SlotLayout lin(S);
        StagedImages staged(S);
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i];
            const uint64_t body = b.lens[f] - 8;
            bf[i].rec_d = base + (uint64_t)f * b.stride + 8;
            bf[i].R = body / 12; bf[i].tail_bytes = body % 12; bf[i].n = b.pixels(f);
            lin.plan(i, b.image_bytes(f), true);
            staged.plan(i, b.image_bytes(f), !b.dst_dev);
        }
        CNIIC_HIP_TRY(c, lin_d.alloc(lin.total));
        CNIIC_HIP_TRY(c, staged.alloc(c));
        for (size_t i = 0; i < S; i++) bf[i].lin_d = lin_d.as<uint8_t>() + lin.at[i];
        RleBatchScratch keep;
        ScopedKernelTimer timer(c, "rle_dec_batch");
        CNIIC_TRY(rle_expand_batch_dev(c, bf, &keep));
        for (size_t i = 0; i < S; i++)   // follow the traversal (hilbertc.rs:58-61)
            CNIIC_TRY(hilbert_scatter(c, bf[i].lin_d, b.w[route[i0 + i]], b.h[route[i0 + i]], staged.dst(i, b.image(route[i0 + i]))));
        timer.stop(S);
        for (size_t i = 0; i < S; i++) CNIIC_HIP_TRY(c, staged.down_each(c, i, b.image(route[i0 + i]), bf[i].n * 3, hipMemcpyDeviceToHost));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        rle_expand_batch_status(bf, &keep);
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i];
            b.taken[f] = 1;
            if (bf[i].status) b.decode_error(f, "hilbert-rle: bad run record (assert!(count > 0) / unwrap, hilbertc.rs:327-328)");
        }
        i0 = i1;
    }
    return CNIIC_OK;
}

// ------------------------------------------------------------------ small `delta` frames of a batch (k_delta_small_dec.hip)
// codec_decode_batch_route has parsed the decoders; what it hands over are the frames of 1 .. kDeltaSmallDecMaxPx pixels whose size has no
// injected scan and whose decoder has no code longer than kDeltaSmallMaxCodeLen (delta_small.hpp proves that no encoder of so few symbols
// makes one; a hostile stream that has one is the single decode's).  They are worked through in chunks whose scratch -- the tables of
// leaves, the rows, the status words, and for a host destination the staged images -- stays below kDeltaSmallDecScratch: per chunk one
// copy up for the tables and rows (and one for host streams, from the chunk's first frame to its last), ONE launch with a workgroup per
// frame, one copy down for the status words (and one for a host destination's images, which a memcpy per frame then puts in place), one
// wait.  A frame the kernel hands back (not settled within its rounds) is left to the caller like everything else not taken.
// Frames whose decoders k_small_trieparse / k_small_trieparse_rgb have parsed (small_parse_dev below) come with their tables in HBM: nothing of those goes up.
// The testing library can switch the route off (CNIIC_TEST_DELTA_SMALL_DEC_OFF=1), lower its bound (CNIIC_TEST_DELTA_SMALL_DEC_MAX_PX) and its
// settle rounds (CNIIC_TEST_DELTA_SMALL_DEC_ROUNDS), and make the chunks small (CNIIC_TEST_MEASURE_BUDGET, bytes).
constexpr uint64_t kDeltaSmallDecScratch = 2ull << 30;
static uint64_t delta_small_dec_max_px() { return small_route_max_px("CNIIC_TEST_DELTA_SMALL_DEC_OFF", "CNIIC_TEST_DELTA_SMALL_DEC_MAX_PX", kDeltaSmallDecMaxPx); }
// A decoder that the parse kernel has left in HBM (small_parse_dev below): its codes, then as many key | length words
struct DeltaSmallDevTab { const uint32_t *code; uint32_t leaves, max_len; };
// Small `hufman` and `cluster-colors` frames take the same route under the other symbol kind (k_huf_small_dec: RGB keys, no FromDiff, no
// scan): frames of 1 .. kHufSmallMaxPx pixels whose decoder the host has parsed and has no code longer than kDeltaSmallMaxCodeLen; larger
// frames, longer codes and everything unparsed keep huff_decode_batch_dev.  Stage timer "huf_small_dec_batch"; the testing library can
// switch it off (CNIIC_TEST_HUF_SMALL_DEC_OFF=1) and lower its bound (CNIIC_TEST_HUF_SMALL_DEC_MAX_PX); the rounds' knob above caps both.
static uint64_t huf_small_dec_max_px() { return small_route_max_px("CNIIC_TEST_HUF_SMALL_DEC_OFF", "CNIIC_TEST_HUF_SMALL_DEC_MAX_PX", kHufSmallMaxPx); }
// The floor of that route.  Most of the call is the host's parse of the decoders either way; what the kernel adds for few frames is its settle
// rounds (0.35 ms for one 32 x 32 frame, whatever the number of frames up to the CUs) against launches that the batched route shares among
// its frames.  Measured against the parent commit's library (tools/small_hufman_probe.py, profiles/small_hufman_probe.json; NOTES AF), whole
// call, parent's time / this route's, `hufman` streams:
//   1 .. 4 frames:   32 x 32, 64 x 64 and one 128 x 96 frame lost (0.63x .. 0.78x, most beyond the spreads); 128 x 128 and 16384 x 1 won or tied (0.99x .. 2.3x)
//   16, 64 frames:   0.93x .. 2.35x, and photo-like 128 x 96 lost beyond the spreads (0.76x, 0.86x)
//   256, 4096:       every class won: 1.01x .. 4.08x
// and cluster-colors(256) streams: 0.80x .. 1.82x up to 64 frames (two classes of 16 frames lost beyond the spreads), 0.88x .. 1.38x from 256 on with
// no class beyond the spreads.  So the frames take this route in a call with at least 256 small frames (the first count at which every class won) and
// keep the batched route otherwise.  The testing library takes the floor away with CNIIC_TEST_HUF_SMALL_FLOOR_OFF=1.
constexpr uint32_t kHufSmallDecFloorFrames = 256;
static uint32_t huf_small_dec_floor() {
    if (const char *e = test_env("CNIIC_TEST_HUF_SMALL_FLOOR_OFF")) if (atoi(e) != 0) return 0;
    return kHufSmallDecFloorFrames;
}
struct SmallDecKind {
    const char *name, *timer, *short_msg;
    int (*run)(Ctx *, const DeltaSmallDecRow *, uint32_t, uint32_t, uint32_t, uint32_t *);
    uint32_t last_status;
};
static const SmallDecKind kSmallDecDelta = {"delta_small_dec", "delta_small_dec_batch", "delta: cannot decode the difference stream", delta_small_dec_run, kDsdRange};
static const SmallDecKind kSmallDecRgb = {"huf_small_dec", "huf_small_dec_batch", "Failed to decode symbol", huf_small_dec_run, kDsdUnsettled};
// dev != nullptr: the routed frames' tables lie in HBM already ((*dev)[f]), and `tabs` is not looked at
static int delta_small_decode(DecodeBatch &b, const SmallDecKind &kind, const std::vector<uint32_t> &route, const std::vector<std::vector<uint32_t>> &tabs,
                              const std::vector<DeltaSmallDevTab> *dev, const std::vector<uint64_t> &pay) {
    Ctx *c = b.c;
    uint32_t max_rounds = kDsdMaxRounds;
    if (const char *e = test_env("CNIIC_TEST_DELTA_SMALL_DEC_ROUNDS")) max_rounds = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), kDsdMaxRounds);
    const uint64_t budget = test_budget(kDeltaSmallDecScratch);
    auto tab_words = [&](uint32_t f) -> uint64_t { return dev ? 0 : tabs[f].size(); };
    auto scratch_of = [&](uint32_t f) { return tab_words(f) * 4 + sizeof(DeltaSmallDecRow) + 4 + (b.dst_dev ? 0 : SlotLayout::room(b.image_bytes(f))); };
    for (size_t i0 = 0; i0 < route.size();) {
        const size_t i1 = take_chunk(i0, route.size(), budget, [&](size_t i) { return scratch_of(route[i]); });
        const size_t S = i1 - i0;
        // ---- the streams in HBM
        DevBuf up_d, tab_d;
        const uint8_t *base;
        CNIIC_TRY(streams_in_hbm(b, route[i0], route[i1 - 1], up_d, &base));
        // ---- one block for the rows, the status words and every frame's leaves; the staged images of a host destination
        uint64_t words = 0;
        uint32_t max_px = 0;
        StagedImages staged(S);
        std::vector<uint64_t> tab_word(S, 0);
        for (size_t i = 0; i < S; i++) { tab_word[i] = words; words += tab_words(route[i0 + i]); staged.plan(i, b.image_bytes(route[i0 + i]), !b.dst_dev); }
        const uint64_t rows_at = 0, status_at = (S * sizeof(DeltaSmallDecRow) + 15) & ~15ull, tab_at = (status_at + S * 4 + 15) & ~15ull;
        // (assembled in the context's pinned block, which held the streams' heads until the decoders were parsed: nothing reads those any more)
        const uint64_t up_bytes = tab_at + words * 4;
        CNIIC_HIP_TRY(c, c->pinned_huf.reserve(up_bytes, pinned_huf_want(up_bytes)));
        uint8_t *up = c->pinned_huf.as<uint8_t>();
        CNIIC_HIP_TRY(c, tab_d.alloc(up_bytes));
        CNIIC_HIP_TRY(c, staged.alloc(c));
        DeltaSmallDecRow *rows = reinterpret_cast<DeltaSmallDecRow *>(up + rows_at);
        std::vector<uint32_t> longest(S, 0);
        if (!dev)
            parallel_for((uint32_t)S, (uint32_t)std::min<size_t>(16, std::max<uint64_t>(1, words >> 16)), [&](uint32_t i, uint32_t) {
                const std::vector<uint32_t> &t = tabs[route[i0 + i]];
                memcpy(up + tab_at + tab_word[i] * 4, t.data(), t.size() * 4);
                for (size_t k = t.size() / 2; k < t.size(); k++) longest[i] = std::max(longest[i], dsd_keylen_len(t[k]));
            });
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i];
            const uint32_t n = b.w[f] * b.h[f], L = dev ? (*dev)[f].leaves : (uint32_t)(tabs[f].size() / 2);
            DeltaSmallDecRow r;
            r.payload = base + (uint64_t)f * b.stride + pay[f];
            r.payload_bytes = dsd_stage_bytes(n, b.lens[f] - pay[f]);
            r.code = dev ? (*dev)[f].code : reinterpret_cast<const uint32_t *>(tab_d.as<uint8_t>() + tab_at) + tab_word[i];
            r.keylen = r.code + L;
            r.leaves = L; r.w = b.w[f]; r.h = b.h[f]; r.max_len = dev ? (*dev)[f].max_len : longest[i];
            r.dst = staged.dst(i, b.image(f));
            rows[i] = r;
            max_px = std::max(max_px, n);
        }
        memset(up + status_at, 0xff, S * 4);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(tab_d.p, up, up_bytes, hipMemcpyHostToDevice, c->stream));
        {
            ScopedKernelTimer t(c, kind.timer);
            CNIIC_TRY(kind.run(c, reinterpret_cast<const DeltaSmallDecRow *>(tab_d.as<uint8_t>() + rows_at), (uint32_t)S, max_px, max_rounds,
                                          reinterpret_cast<uint32_t *>(tab_d.as<uint8_t>() + status_at)));
            t.stop(S);
        }
        std::vector<uint32_t> st(S);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(st.data(), tab_d.as<uint8_t>() + status_at, S * 4, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, staged.down_block(c));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i];
            if (st[i] == kDsdUnsettled) continue;   // the caller's
            if (st[i] > kind.last_status) return c->fail(CNIIC_ERR_HIP, "%s: frame %u reported no status", kind.name, f);
            b.taken[f] = 1;
            if (st[i] == kDsdShort) b.decode_error(f, kind.short_msg);
            else if (st[i] == kDsdRange) b.decode_error(f, "delta: colour out of range (hilbertc.rs:505)");
            else staged.put(i, b.image(f), b.image_bytes(f));
        }
        i0 = i1;
    }
    return CNIIC_OK;
}

// ------------------------------------------------------------------ the decoders of small frames, parsed where the streams lie
// Streams in device memory (k_small_trie.hip): no head of a stream comes to the host.  Two kinds: `delta` (SignedColor leaves, S = 6 symbol
// bytes, k_small_trieparse) and the RGB kinds `hufman` / `cluster-colors` (Rgb leaves, S = 11, k_small_trieparse_rgb).  What the kernel
// may read of frame f is what the host's looks below get to see of it, min(lens[f], stride) bytes.  The candidates are worked through in
// chunks whose scratch -- 8 bytes per leaf a stream has room for, at most kSmallTrieMaxLeaves, and the rows -- stays below the budget: per
// chunk one copy up of the rows, ONE launch with a workgroup per frame, one copy down of the result rows, one wait; then
// delta_small_decode for the chunk's parsed frames, whose rows point at the tables where the kernel left them.  A parsed frame is routed
// under the host parse's conditions (no code longer than kDeltaSmallMaxCodeLen -- the kernel finishes no other --, more leaves than one
// only with a payload).  `host` gets the frames the caller runs the host's looks and parse for, and those alone, which keeps the routed
// frames, every status and every message what they are without this parse.
//   `delta`: every frame with a header (lens[f] >= 8, not named by CNIIC_TEST_DECODE_BATCH_OFF) is a candidate.  A frame the kernel
//     skips on its header (its size, an injected scan) is dropped: the host's parse would not look at it either.  Handed back: not a
//     decoder, not ours.
//   RGB kinds: a candidate is also no longer than the longest stream of a small frame (huf_small.hpp), and the parse runs only in a call
//     with at least `floor` candidates (kHufSmallDecFloorFrames; a pure host test).  A skipped frame is too large for the small route,
//     and the batched route takes such frames: it is handed back with everything else that was not routed.  The floor is then held on
//     the result rows: frames are routed once `floor` frames with a verdict other than skipped have been seen.  A chunk that ends before
//     that keeps its tables for nothing, so its parsed frames (fewer than `floor`) are parsed once more behind the last chunk; with
//     fewer such frames in the whole call nothing is routed and every frame takes the host's path.
// Stage timers, per kind (they exist only when the parse ran): "delta_small_dec_parse" / "huf_small_dec_parse" (the launches' time;
// launches = frames parsed) and "delta_small_dec_parse_host" / "huf_small_dec_parse_host" (no time; launches = candidates handed back).
// The testing library keeps the host's parse for everything with CNIIC_TEST_DELTA_SMALL_DEC_PARSE_OFF=1 / CNIIC_TEST_HUF_SMALL_DEC_PARSE_OFF=1.
static bool delta_small_parse_off() {
    if (const char *e = test_env("CNIIC_TEST_DELTA_SMALL_DEC_PARSE_OFF")) return atoi(e) != 0;
    return false;
}
static bool huf_small_parse_off() {
    if (const char *e = test_env("CNIIC_TEST_HUF_SMALL_DEC_PARSE_OFF")) return atoi(e) != 0;
    return false;
}
struct SmallParseKind {
    uint32_t sym_bytes;   // S of small_trie.hpp
    const SmallDecKind *dec;
    const char *timer, *timer_host;
    bool rgb;             // skipped frames and everything else not routed go back to the host's path; the length gate and the floor
};
static const SmallParseKind kSmallParseDelta = {6, &kSmallDecDelta, "delta_small_dec_parse", "delta_small_dec_parse_host", false};
static const SmallParseKind kSmallParseRgb = {11, &kSmallDecRgb, "huf_small_dec_parse", "huf_small_dec_parse_host", true};
static int small_parse_dev(DecodeBatch &b, const SmallParseKind &kind, uint64_t max_px, uint32_t floor, std::vector<uint32_t> &host) {
    Ctx *c = b.c;
    const uint32_t F = b.F;
    host.clear();
    std::vector<uint32_t> cands;
    auto room_of = [&](uint32_t f) { return kind.sym_bytes == 6 ? st_leaves_room<6>(b.view(f)) : st_leaves_room<11>(b.view(f)); };
    auto everything = [&]() { host.resize(F); for (uint32_t f = 0; f < F; f++) host[f] = f; };
    const uint64_t longest_small = kind.rgb ? hs_stream_bytes(max_px, (uint64_t)kDeltaSmallMaxCodeLen * max_px) : ~0ull;
    for (uint32_t f = 0; f < F; f++) if (!b.off_route[f] && b.lens[f] >= 8 && b.lens[f] <= longest_small && b.view(f) >= 8) cands.push_back(f);
    if (kind.rgb && (cands.empty() || cands.size() < floor)) { everything(); return CNIIC_OK; }   // (the parse does not run: no stage of its)
    if (c->timers) { (void)c->ktimes[kind.timer]; (void)c->ktimes[kind.timer_host]; }
    if (cands.empty()) return CNIIC_OK;
    const uint64_t budget = test_budget(kDeltaSmallDecScratch);
    auto scratch_of = [&](uint32_t f) { return (uint64_t)room_of(f) * 8 + sizeof(SmallTrieRow) + sizeof(SmallTrieResult); };
    const bool scan = c->scan_xy.p != nullptr;
    std::vector<DeltaSmallDevTab> dev(F);
    std::vector<uint64_t> pay(F, 0);
    std::vector<uint8_t> back(F, kind.rgb ? 1 : 0);   // the frames of `host`
    std::vector<uint32_t> late;                        // parsed in a chunk that ended below the floor
    const std::vector<std::vector<uint32_t>> no_tabs;
    uint64_t parsed = 0, handed = 0, seen = 0;
    auto run_list = [&](const std::vector<uint32_t> &list, bool first) -> int {
        for (size_t i0 = 0; i0 < list.size();) {
            const size_t i1 = take_chunk(i0, list.size(), budget, [&](size_t i) { return scratch_of(list[i]); });
            uint64_t longest = 0;
            const size_t S = i1 - i0;
            // ---- one block: the rows, the result rows, every frame's table
            const uint64_t res_at = (S * sizeof(SmallTrieRow) + 15) & ~15ull, tab_at = (res_at + S * sizeof(SmallTrieResult) + 15) & ~15ull;
            uint64_t words = 0;
            for (size_t i = 0; i < S; i++) words += 2ull * room_of(list[i0 + i]);
            DevBuf blk_d;
            CNIIC_HIP_TRY(c, blk_d.alloc(tab_at + words * 4 + 16));
            CNIIC_HIP_TRY(c, c->pinned_huf.reserve(res_at, pinned_huf_want(res_at)));
            SmallTrieRow *rows = c->pinned_huf.as<SmallTrieRow>();
            uint32_t *tab0 = reinterpret_cast<uint32_t *>(blk_d.as<uint8_t>() + tab_at);
            uint64_t wat = 0;
            for (size_t i = 0; i < S; i++) {
                const uint32_t f = list[i0 + i];
                rows[i].stream = b.stream(f);
                rows[i].table = tab0 + wat;
                rows[i].bytes = b.view(f);
                wat += 2ull * room_of(f);
                longest = std::max(longest, b.view(f));
            }
            CNIIC_HIP_TRY(c, hipMemcpyAsync(blk_d.p, rows, S * sizeof(SmallTrieRow), hipMemcpyHostToDevice, c->stream));
            {
                ScopedKernelTimer t(c, kind.timer);
                CNIIC_TRY(small_trie_run(c, kind.sym_bytes, blk_d.as<SmallTrieRow>(), (uint32_t)S, longest, (uint32_t)max_px, b.img_stride, scan ? c->scan_w : 0,
                                         scan ? c->scan_h : 0, reinterpret_cast<SmallTrieResult *>(blk_d.as<uint8_t>() + res_at)));
                t.stop(0);
            }
            std::vector<SmallTrieResult> res(S);
            CNIIC_HIP_TRY(c, hipMemcpyAsync(res.data(), blk_d.as<uint8_t>() + res_at, S * sizeof(SmallTrieResult), hipMemcpyDeviceToHost, c->stream));
            CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (first) for (size_t i = 0; i < S; i++) seen += res[i].verdict != kStSkipped;
            const bool met = seen >= floor;
            std::vector<uint32_t> route;
            for (size_t i = 0; i < S; i++) {
                const uint32_t f = list[i0 + i];
                const SmallTrieResult &r = res[i];
                if (r.verdict == kStSkipped) { handed += first && kind.rgb; continue; }   // (`delta`: the host's parse would not look at it either)
                if (r.verdict != kStParsed) { back[f] = 1; handed += first; continue; }
                parsed += first;
                if (r.leaves == 0 || r.leaves > room_of(f) || r.max_len > kDeltaSmallMaxCodeLen || r.payload_at > b.view(f))
                    return c->fail(CNIIC_ERR_HIP, "small_trieparse: frame %u reported a decoder outside its stream", f);
                if (r.leaves > 1 && r.payload_at >= b.lens[f]) continue;   // (symbols, and no payload: the single decode answers)
                if (!met) { late.push_back(f); continue; }
                b.w[f] = r.w; b.h[f] = r.h;
                pay[f] = r.payload_at;
                dev[f] = DeltaSmallDevTab{rows[i].table, r.leaves, r.max_len};
                back[f] = 0;
                route.push_back(f);
            }
            if (!route.empty()) CNIIC_TRY(delta_small_decode(b, *kind.dec, route, no_tabs, &dev, pay));
            i0 = i1;
        }
        return CNIIC_OK;
    };
    CNIIC_TRY(run_list(cands, true));
    if (seen < floor) {   // (fewer small frames than the floor: nothing is routed from here)
        everything();
        handed = cands.size();
    } else {
        if (!late.empty()) { const std::vector<uint32_t> again(late); CNIIC_TRY(run_list(again, false)); }
        for (uint32_t f = 0; f < F; f++) if (back[f]) host.push_back(f);
    }
    if (c->timers) { c->ktimes[kind.timer].launches += parsed; c->ktimes[kind.timer_host].launches += handed; }
    return CNIIC_OK;
}

// ------------------------------------------------------------------ small `voronoi` frames of a batch (k_vor_small.hip k_vor_small_dec)
// voronoi_batch has parsed the heads exactly as codec_decode does; what it hands over are the frames whose header and whole
// centroid list are there and well formed, with 1 <= K <= kVorSmallMaxK, 1 <= w h <= kVorSmallMaxPx and an image that fits img_stride:
// cent[f] = where frame f's centroids start in `table` (three words each: x, y, 0xRRGGBB), Ks[f] = how many.  They are worked through in
// chunks whose scratch -- the centroids, the rows, and for a host destination the staged images -- stays below the budget: per chunk one
// copy up, ONE launch with a workgroup per slice of kVorSmallDecSlice pixels of a frame, for a host destination one copy down (a memcpy per frame then puts the images in place),
// one wait.  Every routed frame decodes: there is no status to fetch.
static uint64_t vor_small_dec_max_px() { return small_route_max_px("CNIIC_TEST_VOR_SMALL_DEC_OFF", nullptr, kVorSmallMaxPx); }
static int vor_small_decode(DecodeBatch &b, const std::vector<uint32_t> &route, const std::vector<uint32_t> &table, const std::vector<uint64_t> &cent,
                            const std::vector<uint32_t> &Ks) {
    Ctx *c = b.c;
    const uint32_t *w = b.w, *h = b.h;
    const uint64_t budget = test_budget(kVorSmallScratch);
    auto slices_of = [&](uint32_t f) { return (w[f] * h[f] + kVorSmallDecSlice - 1) / kVorSmallDecSlice; };   // (a workgroup's share of a frame: k_vor_small.hip)
    auto scratch_of = [&](uint32_t f) { return (uint64_t)Ks[f] * 12 + slices_of(f) * sizeof(VorSmallDecRow) + (b.dst_dev ? 0 : SlotLayout::room(b.image_bytes(f))); };
    for (size_t i0 = 0; i0 < route.size();) {
        const size_t i1 = take_chunk(i0, route.size(), budget, [&](size_t i) { return scratch_of(route[i]); });
        const size_t S = i1 - i0;
        uint64_t cents = 0, slices = 0;
        StagedImages staged(S);
        for (size_t i = 0; i < S; i++) { cents += Ks[route[i0 + i]]; slices += slices_of(route[i0 + i]); staged.plan(i, b.image_bytes(route[i0 + i]), !b.dst_dev); }
        const uint64_t tab_at = (slices * sizeof(VorSmallDecRow) + 15) & ~15ull, up_bytes = tab_at + cents * 12;
        std::vector<uint8_t> up(up_bytes);
        DevBuf up_d;
        CNIIC_HIP_TRY(c, up_d.alloc(up_bytes));
        CNIIC_HIP_TRY(c, staged.alloc(c));
        VorSmallDecRow *rows = reinterpret_cast<VorSmallDecRow *>(up.data());
        uint64_t cat = 0, rat = 0;
        uint32_t max_px = 0;
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i];
            memcpy(up.data() + tab_at + cat * 12, table.data() + 3 * cent[f], (size_t)Ks[f] * 12);
            for (uint32_t px0 = 0; px0 < w[f] * h[f]; px0 += kVorSmallDecSlice)
                rows[rat++] = VorSmallDecRow{staged.dst(i, b.image(f)), (uint32_t)cat, Ks[f], w[f], h[f], px0, 0u};
            cat += Ks[f];
            max_px = std::max(max_px, w[f] * h[f]);
        }
        CNIIC_HIP_TRY(c, hipMemcpyAsync(up_d.p, up.data(), up_bytes, hipMemcpyHostToDevice, c->stream));
        {
            ScopedKernelTimer t(c, "vor_small_dec_batch");
            CNIIC_TRY(vor_small_dec_run(c, up_d.as<VorSmallDecRow>(), (uint32_t)slices, max_px, reinterpret_cast<const uint32_t *>(up_d.as<uint8_t>() + tab_at)));
            t.stop(S);
        }
        CNIIC_HIP_TRY(c, staged.down_block(c));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i];
            b.taken[f] = 1;
            staged.put(i, b.image(f), b.image_bytes(f));
        }
        i0 = i1;
    }
    return CNIIC_OK;
}

// `voronoi`: a stream is its header and at most 16 + 19 K bytes of centroids.  The heads of streams in HBM come down in groups of as many
// rows as the pinned block holds (never wider than the stride, the source pitch of the strided copy); a group is parsed before the
// next one takes its place.  A frame is the route's when the single decode's parse (codec_decode) goes through on what was looked
// at and the frame is small; every other frame is the caller's, with that decode's status and message.
static int voronoi_batch(DecodeBatch &b) {
    Heads heads(b);
    std::vector<uint32_t> route, table, Ks(b.F, 0);
    std::vector<uint64_t> cent(b.F, 0);
    const uint64_t max_px = vor_small_dec_max_px();
    auto classify = [&](uint32_t f) {
        if (b.off_route[f]) return;
        uint64_t pos, K;
        uint32_t fw, fh;
        if (!heads.dims(f, &fw, &fh, &pos) || !dims_fit((uint64_t)fw * fh, max_px, b.img_stride)) return;
        const size_t at = table.size();
        const VorHead v = vor_parse_head(heads.head_p[f], heads.head_n[f], pos, &K, [&](uint64_t, uint32_t x, uint32_t y, uint8_t r, uint8_t g, uint8_t bl) {
            table.push_back(x); table.push_back(y);
            table.push_back((uint32_t)r << 16 | (uint32_t)g << 8 | bl);
        });
        if (v != VorHead::Ok || !K || K > kVorSmallMaxK) { table.resize(at); return; }   // the caller's
        b.w[f] = fw; b.h[f] = fh;
        cent[f] = at / 3; Ks[f] = (uint32_t)K;
        route.push_back(f);
    };
    if (b.bytes_dev) {
        const uint64_t W = std::min<uint64_t>(vs_stream_len(kVorSmallMaxK), b.stride);
        if (!W && b.F > 1) return CNIIC_OK;   // (streams on top of one another: every frame to the single decode)
        const uint64_t Wf = W ? W : vs_stream_len(kVorSmallMaxK);   // (one frame: its stride does not matter)
        const uint32_t group = (uint32_t)std::max<uint64_t>(1, kBatchHeadsMax / Wf);
        for (uint32_t f0 = 0; f0 < b.F;) {
            const uint32_t f1 = (uint32_t)std::min<uint64_t>((uint64_t)f0 + group, b.F) - 1;
            CNIIC_TRY(heads.fetch(Wf, f0, f1));
            for (uint32_t f = f0; f <= f1; f++) classify(f);
            f0 = f1 + 1;
        }
    } else {
        heads.in_place();
        for (uint32_t f = 0; f < b.F; f++) classify(f);
    }
    if (route.empty()) return CNIIC_OK;
    return vor_small_decode(b, route, table, cent, Ks);
}

// ------------------------------------------------------------------ small `zip(dict)` frames of a batch (k_zd_small_dec.hip)
// The host reads the head of every stream -- kZdDecHead bytes, 16 pairs -- and finds what zip_dict_dims finds on it (zsd_head_dims); a frame is a candidate when the head
// spells the 8 bytes of the dimensions, 1 <= w h <= kZdSmallDecMaxPx, the image fits img_stride and (in a call of several frames) the
// stream ends before the next one starts.  Every other frame is the caller's, with the single decode's status and message.  The candidates
// at or below the floor's pixel bound for their count (zd_small_dec_floor_px) are worked through in chunks whose scratch -- rows, result
// rows, for a host batch the streams and for a host destination the staged images -- stays below 1 GiB (the testing library: below
// CNIIC_TEST_MEASURE_BUDGET bytes, a frame at least): per chunk one copy up, one launch per SIZE CLASS of dynamic LDS (a frame's offsets and
// image, and its pair words where they fit beside them; the classes keep one large frame from sizing the LDS of every workgroup, so that
// small frames share a CU), one copy down, one wait.  A frame the kernel hands back (pairs behind the cap, more than kZsdRounds generations,
// a byte behind more than kZsdHops pairs) is the caller's.
//
// The floor.  Measured against the parent commit's library (tools/small_zip_probe.py --calls decode, profiles/small_zip_dec_probe.json; NOTES
// AR), photo-like, uniform noise and flat frames in device memory, whole decode call, medians of 5, parent's time / this route's; a class
// takes the route only where this build's slowest run beat the parent's fastest for all three contents:
//   1 frame:      32 x 32 1.04x .. 1.32x (the flat row's ranges touch); every larger size lost (0.13x .. 0.62x): one workgroup needs 0.13 ..
//                 0.63 ms for 4096 .. 16 384 pixels, a worker 0.09 .. 0.29 ms
//   8 frames:     32 x 32 won (3.6x .. 4.0x), 64 x 64 won (1.85x .. 2.4x); 128 x 96, 128 x 128 and 16384 x 1 did not (0.44x .. 1.24x, no row clear)
//   32 frames:    every size won: 8.0x .. 8.7x, 4.0x .. 4.7x, and 1.11x .. 2.4x for 12 288 and 16 384 pixels (flat frames the closest: 0.712 ms at
//                 the slowest against 0.762 at the parent's fastest)
//   256 frames:   every size won (6.1x .. 33x);  4096 frames: 32 x 32 46x .. 55x, 64 x 64 28x .. 32x (larger sizes not probed at this count)
// Host memory on both sides follows (64 x 64: 0.5x .. 0.6x, 1.3x .. 1.8x, 2.4x .. 3.0x, 5.8x .. 6.8x, 1.5x .. 3.3x at 1, 8, 32, 256, 4096 frames).
// So: fewer than kZdSmallDecFloorFew candidates stay with the workers; from there on the candidates of at most kZdSmallDecFloorPxFew
// pixels take the route, and from kZdSmallDecFloorMany candidates on all of them.  Counts between the probed ones keep the lower class's
// bound.  The floor knows pixels, not contents.  The testing library takes it away with CNIIC_TEST_ZD_SMALL_DEC_FLOOR_OFF=1.
constexpr uint64_t kZdDecHead = 64;
static_assert(kZdDecHead == 4 * kZsdHeadPairs, "the head is the pairs zsd_head_dims looks at");
constexpr uint64_t kZdSmallDecScratch = 1ull << 30;
constexpr uint32_t kZsdLdsClasses[] = {16u << 10, 32u << 10, 64u << 10};   // and zd_small_dec_lds_max()
static uint64_t zd_small_dec_max_px() { return small_route_max_px("CNIIC_TEST_ZD_SMALL_DEC_OFF", "CNIIC_TEST_ZD_SMALL_DEC_MAX_PX", kZdSmallDecMaxPx); }
// a cap the testing library may lower, never raise
inline uint32_t test_lower_cap(const char *env, uint32_t bound) {
    if (const char *e = test_env(env)) return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), bound);
    return bound;
}
constexpr uint32_t kZdSmallDecFloorFew = 8, kZdSmallDecFloorMany = 32;
constexpr uint64_t kZdSmallDecFloorPxFew = 4096, kZdSmallDecFloorPxMany = 16384;
static uint64_t zd_small_dec_floor_px(uint64_t candidates) {
    if (const char *e = test_env("CNIIC_TEST_ZD_SMALL_DEC_FLOOR_OFF")) if (atoi(e) != 0) return ~0ull;
    return candidates >= kZdSmallDecFloorMany ? kZdSmallDecFloorPxMany : candidates >= kZdSmallDecFloorFew ? kZdSmallDecFloorPxFew : 0;
}
// The two codecs of the route (k_zd_small_dec.hip: one body, two text kinds).  Hilbert { compress: Zip } (cniic_hilbert_zip_decode_batch)
// differs on the host in this: the dimensions are the stream's first 8 bytes, raw, and the pairs follow them; a frame whose size has an
// injected scan is the caller's (its single decode follows the injection); the lenient verdicts of hz_small.hpp.  Its floor is
// hz_small_dec_floor_px below, measured for this codec.  (The knobs are functions, not names: the names must not be in the release library.)
static_assert(kHzdOk == kZsdOk && kHzdHandedBack == kZsdHandedBack && kHzdBadSymbol == kZsdBadSymbol && kHzdDangling == kZsdDangling, "one set of verdicts for both kinds");
struct SmallZipDecKind {
    bool hilbert;
    const char *name, *t_batch, *t_handback;
    uint64_t (*max_px)();
    uint64_t (*floor_px)(uint64_t candidates);
    uint32_t (*max_pairs)();
    uint32_t (*hops)();
    uint32_t (*rounds)();
    uint32_t (*lds_max)();
    int (*run)(Ctx *, const ZdSmallDecRow *, uint32_t, uint32_t, uint32_t, uint32_t, ZdSmallDecResult *);
};
static const SmallZipDecKind kSmallDecZipDict = {
    false, "zd_small_dec", "zd_small_dec_batch", "zd_small_dec_handback", zd_small_dec_max_px, zd_small_dec_floor_px,
    [] { return test_lower_cap("CNIIC_TEST_ZD_SMALL_DEC_MAX_PAIRS", kZsdMaxPairs); }, [] { return test_lower_cap("CNIIC_TEST_ZD_SMALL_DEC_HOPS", kZsdHops); },
    [] { return test_lower_cap("CNIIC_TEST_ZD_SMALL_DEC_ROUNDS", kZsdRounds); }, zd_small_dec_lds_max, zd_small_dec_run};

// The floor of the Hilbert { compress: Zip } decode route.  Measured against this build with the route off (the worker contexts) and against
// the parent commit's library, which can only loop over cniic_hilbert_zip_decode on one context (tools/small_zip_probe.py --codec hilbert-zip,
// profiles/small_hz_probe.json; NOTES AS), photo-like, uniform noise and flat frames in device memory, whole decode call, medians of 5; a class
// takes the route only where this route's slowest run beat the workers' fastest for all three contents:
//   1 frame:      32 x 32 0.08 - 0.10 ms against 0.09 - 0.11 (the flat row's ranges touch); every larger size lost (0.17 - 0.93 ms against 0.09 - 0.30)
//   4 frames:     32 x 32 won (0.09 - 0.10 ms against 0.21 - 0.35), 64 x 64 won (0.17 - 0.22 against 0.23 - 0.31; flat frames the closest: 0.22
//                 at the slowest against 0.26 at the workers' fastest); the larger sizes lost (0.61 - 0.94 against 0.21 - 0.53)
//   8 frames:     32 x 32 won (0.09 - 0.10 against 0.35 - 0.40), 64 x 64 won (0.17 - 0.21 against 0.36 - 0.54); 12 288 and 16 384 pixels did not
//                 (0.61 - 0.94 against 0.31 - 0.58 and one slow run of 2.8)
//   32 frames:    up to 64 x 64 won (4x - 9x); 128 x 128 and 16384 x 1 won (0.62 - 0.74 against 0.80 - 1.43), 128 x 96 did not: its general
//                 walk makes the kernel 0.86 - 0.94 ms, and flat frames decode in 0.91 - 1.05 on the workers
//   256 frames:   every size won (6x - 40x);  4096 frames: 32 x 32 1.4 - 1.6 ms against 80 - 93, 64 x 64 2.9 - 3.5 against 77 - 89 (larger sizes
//                 not probed at this count)
// The kernel's time is set by its heaviest frame; the workers' grows with the count, so a class that won with n frames wins with more.
// So: fewer than kHzSmallDecFloorFew candidates stay with the workers; from there on the candidates of at most kHzSmallDecFloorPxFew
// pixels take the route, and from kHzSmallDecFloorMany on all of them (a floor knows pixels, not shapes: 12 288 pixels lost at 32 frames,
// so 16 384 waits for 256).  The testing library takes the floor away with CNIIC_TEST_HZ_SMALL_DEC_FLOOR_OFF=1.
constexpr uint32_t kHzSmallDecFloorFew = 4, kHzSmallDecFloorMany = 256;
constexpr uint64_t kHzSmallDecFloorPxFew = 4096, kHzSmallDecFloorPxMany = 16384;
static uint64_t hz_small_dec_max_px() { return small_route_max_px("CNIIC_TEST_HZ_SMALL_DEC_OFF", "CNIIC_TEST_HZ_SMALL_DEC_MAX_PX", kHzSmallMaxPx); }
static uint64_t hz_small_dec_floor_px(uint64_t candidates) {
    if (const char *e = test_env("CNIIC_TEST_HZ_SMALL_DEC_FLOOR_OFF")) if (atoi(e) != 0) return ~0ull;
    return candidates >= kHzSmallDecFloorMany ? kHzSmallDecFloorPxMany : candidates >= kHzSmallDecFloorFew ? kHzSmallDecFloorPxFew : 0;
}
static const SmallZipDecKind kSmallDecHilbertZip = {
    true, "hz_small_dec", "hz_small_dec_batch", "hz_small_dec_handback", hz_small_dec_max_px, hz_small_dec_floor_px,
    [] { return test_lower_cap("CNIIC_TEST_HZ_SMALL_DEC_MAX_PAIRS", kZsdMaxPairs); }, [] { return test_lower_cap("CNIIC_TEST_HZ_SMALL_DEC_HOPS", kZsdHops); },
    [] { return test_lower_cap("CNIIC_TEST_HZ_SMALL_DEC_ROUNDS", kZsdRounds); }, hz_small_dec_lds_max, hz_small_dec_run};

static int zip_dict_batch(DecodeBatch &b, const SmallZipDecKind &kind) {
    Ctx *c = b.c;
    const uint64_t max_px = kind.max_px();
    const uint64_t head = kind.hilbert ? kHzHead : 0;   // bytes of a stream in front of its pairs
    Heads heads(b);
    std::vector<uint32_t> cand, cw, ch;
    auto classify = [&](uint32_t f) {
        if (b.off_route[f] || (b.F > 1 && b.stride < b.lens[f])) return;
        uint32_t fw = 0, fh = 0;
        if (kind.hilbert) {
            uint64_t pos;
            if (b.lens[f] < kHzHead || !heads.dims(f, &fw, &fh, &pos)) return;
            if (c->scan_xy.p && c->scan_w == fw && c->scan_h == fh) return;   // (a size with an injected scan: the single decode follows it)
        } else if (!zsd_head_dims(heads.head_p[f], std::min(heads.head_n[f], kZdDecHead), &fw, &fh)) return;   // (zip_dict_dims on the same bytes, without its table)
        if (!dims_fit((uint64_t)fw * fh, max_px, b.img_stride)) return;
        cand.push_back(f); cw.push_back(fw); ch.push_back(fh);
    };
    if (b.bytes_dev) {
        const uint64_t look = kind.hilbert ? kHzHead : kZdDecHead;
        const uint64_t W = b.F == 1 ? look : std::min(look, b.stride);   // (a look is never wider than the stride)
        if (!W) return CNIIC_OK;
        const uint32_t group = (uint32_t)(kBatchHeadsMax / W);
        for (uint32_t f0 = 0; f0 < b.F;) {
            const uint32_t f1 = (uint32_t)std::min<uint64_t>((uint64_t)f0 + group, b.F) - 1;
            CNIIC_TRY(heads.fetch(W, f0, f1));
            for (uint32_t f = f0; f <= f1; f++) classify(f);
            f0 = f1 + 1;
        }
    } else {
        heads.in_place();
        for (uint32_t f = 0; f < b.F; f++) classify(f);
    }
    const uint64_t floor_px = kind.floor_px(cand.size());
    std::vector<uint32_t> route;
    for (size_t i = 0; i < cand.size(); i++) {
        if ((uint64_t)cw[i] * ch[i] > floor_px) continue;
        b.w[cand[i]] = cw[i]; b.h[cand[i]] = ch[i];
        route.push_back(cand[i]);
    }
    if (route.empty()) return CNIIC_OK;

    const uint32_t max_pairs = kind.max_pairs(), hops = kind.hops(), rounds = kind.rounds();
    const uint32_t lds_max = kind.lds_max();
    const uint64_t budget = test_budget(kZdSmallDecScratch);
    auto pairs_of = [&](uint32_t f) { return (uint32_t)std::min<uint64_t>((b.lens[f] - head) / 4, max_pairs); };
    auto scratch_of = [&](uint32_t f) {
        return sizeof(ZdSmallDecRow) + sizeof(ZdSmallDecResult) + (b.dst_dev ? 0 : SlotLayout::room(b.image_bytes(f))) + (b.bytes_dev ? 0 : b.lens[f]);
    };
    for (size_t i0 = 0; i0 < route.size();) {
        const size_t i1 = take_chunk(i0, route.size(), budget, [&](size_t i) { return scratch_of(route[i]); });
        const size_t S = i1 - i0;
        DevBuf up_d, rows_d, res_d;
        const uint8_t *base;
        CNIIC_TRY(streams_in_hbm(b, route[i0], route[i1 - 1], up_d, &base));
        StagedImages staged(S);
        for (size_t i = 0; i < S; i++) staged.plan(i, b.image_bytes(route[i0 + i]), !b.dst_dev);
        CNIIC_HIP_TRY(c, staged.alloc(c));
        // ---- a row per frame, by size class: what the frame needs of LDS, with its pair words where they fit as well
        std::vector<uint32_t> lds(S), order(S);
        std::vector<uint8_t> stage_pairs(S);
        for (size_t i = 0; i < S; i++) {
            const uint32_t f = route[i0 + i], plain = zsd_lds_bytes(pairs_of(f), (uint32_t)b.pixels(f));
            stage_pairs[i] = plain + 4 * pairs_of(f) <= lds_max;
            const uint32_t want = plain + (stage_pairs[i] ? 4 * pairs_of(f) : 0);
            lds[i] = lds_max;
            for (int k = 2; k >= 0; k--) if (want <= kZsdLdsClasses[k]) lds[i] = kZsdLdsClasses[k];
            order[i] = (uint32_t)i;
        }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return lds[x] < lds[y]; });
        std::vector<ZdSmallDecRow> rows(S);
        for (size_t j = 0; j < S; j++) {
            const size_t i = order[j];
            const uint32_t f = route[i0 + i];
            rows[j] = ZdSmallDecRow{base + (uint64_t)f * b.stride + head, staged.dst(i, b.image(f)), b.lens[f] - head, pairs_of(f), b.w[f], b.h[f], stage_pairs[i]};
        }
        CNIIC_HIP_TRY(c, rows_d.alloc(S * sizeof(ZdSmallDecRow)));
        CNIIC_HIP_TRY(c, res_d.alloc(S * sizeof(ZdSmallDecResult)));
        CNIIC_HIP_TRY(c, hipMemcpyAsync(rows_d.p, rows.data(), S * sizeof(ZdSmallDecRow), hipMemcpyHostToDevice, c->stream));
        {
            ScopedKernelTimer t(c, kind.t_batch);
            for (size_t j0 = 0; j0 < S;) {
                size_t j1 = j0 + 1;
                while (j1 < S && lds[order[j1]] == lds[order[j0]]) j1++;
                CNIIC_TRY(kind.run(c, rows_d.as<ZdSmallDecRow>() + j0, (uint32_t)(j1 - j0), lds[order[j0]] & ~15u, hops, rounds, res_d.as<ZdSmallDecResult>() + j0));
                j0 = j1;
            }
            t.stop(S);
        }
        std::vector<ZdSmallDecResult> res(S);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(res.data(), res_d.p, S * sizeof(ZdSmallDecResult), hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, staged.down_block(c));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        uint64_t back = 0;
        for (size_t j = 0; j < S; j++) {
            const size_t i = order[j];
            const uint32_t f = route[i0 + i];
            const ZdSmallDecResult &r = res[j];
            char text[160];
            switch (r.verdict) {
            case kZsdOk: b.taken[f] = 1; staged.put(i, b.image(f), b.image_bytes(f)); continue;
            case kZsdHandedBack: back++; continue;   // the caller's
            case kZsdBadSymbol: snprintf(text, sizeof text, "zip-dict: pair %llu uses a symbol that has not been handed out", (unsigned long long)r.a); break;
            case kZsdDangling: snprintf(text, sizeof text, "zip-dict: a first symbol without a second at the end of the stream"); break;
            case kZsdShort: snprintf(text, sizeof text, "zip-dict: the text ends after %llu of %llu bytes", (unsigned long long)r.a, (unsigned long long)r.b); break;
            case kZsdBadRecord: snprintf(text, sizeof text, "zip-dict: pixel %llu is not a record of 3 bytes (ser.rs:216-221)", (unsigned long long)r.a); break;
            default: return c->fail(CNIIC_ERR_HIP, "%s: verdict %u", kind.name, r.verdict);
            }
            b.taken[f] = 1;
            b.decode_error(f, text);
        }
        stage_count(c, kind.t_handback, back);
        i0 = i1;
    }
    return CNIIC_OK;
}

// ------------------------------------------------------------------ `hufman`, `cluster-colors` and `delta` frames of a batch
// The batched route of the RGB kinds (huff_decode_batch_dev): the frames of `route` (ascending), whose decoders are lts[f] and whose
// payloads start at pay[f], in parts of kBatchRouteFrames.
static int huffman_tail(DecodeBatch &b, const std::vector<uint32_t> &route, const std::vector<LeafTable> &lts, const std::vector<uint64_t> &pay) {
    Ctx *c = b.c;
    // ---- payloads in HBM, outputs in HBM (4-byte aligned)
    DevBuf up_d;
    const uint8_t *base;
    CNIIC_TRY(streams_in_hbm(b, route.front(), route.back(), up_d, &base));
    std::vector<HdBatchFrame> bf(route.size());
    StagedImages staged(route.size());
    for (size_t i = 0; i < route.size(); i++)
        staged.plan(i, b.image_bytes(route[i]), !b.dst_dev || (reinterpret_cast<uintptr_t>(b.image(route[i])) & 3));
    CNIIC_HIP_TRY(c, staged.alloc(c));
    for (size_t i = 0; i < route.size(); i++) {
        const uint32_t f = route[i];
        bf[i].lt = &lts[f];
        bf[i].payload = base + (uint64_t)f * b.stride + pay[f];
        bf[i].payload_bytes = b.lens[f] - pay[f];
        bf[i].nsyms = b.pixels(f);
        bf[i].out_d = staged.dst(i, b.image(f));
    }
    for (size_t i0 = 0; i0 < bf.size(); i0 += kBatchRouteFrames) {   // (the frame is a grid dimension of the launches)
        std::vector<HdBatchFrame> part(bf.begin() + i0, bf.begin() + std::min(bf.size(), i0 + kBatchRouteFrames));
        CNIIC_TRY(huff_decode_batch_dev(c, part));
        for (size_t i = 0; i < part.size(); i++) bf[i0 + i].status = part[i].status;
    }
    for (size_t i = 0; i < route.size(); i++) {
        const uint32_t f = route[i];
        if (bf[i].status == 2) continue;   // not settled: the caller's
        b.taken[f] = 1;
        if (bf[i].status == 1) { b.decode_error(f, "Failed to decode symbol"); continue; }
        CNIIC_HIP_TRY(c, staged.down_each(c, i, b.image(f), b.image_bytes(f), b.dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    }
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// What the host's parse makes of a frame: the caller's; on the route; the decoder runs past the head (a second look); a small RGB frame, on the workgroup-per-frame route
enum class Cand : uint8_t { NotRouted, Batched, PastHead, SmallRgb };

// The heads of all frames come to the host together (one strided copy for streams in HBM), every decoder is parsed there (up to 16
// threads), and the frames whose symbols are RGB keys decode in one set of launches (huff_decode_batch_dev); `delta` frames of at most
// kDeltaSmallDecMaxPx pixels go to delta_small_decode with their tables of leaves, a workgroup per frame (larger `delta` frames are the
// caller's).
// `delta` streams that lie in device memory are parsed there first (small_parse_dev), and so are `hufman` and `cluster-colors` streams in
// a call with at least kHufSmallDecFloorFrames frames short enough to be small; the heads and the host's parse below are then for the
// frames that parse hands back, and for those alone.  Streams in host memory keep the host's parse: the bytes are where the parser is.
static int huffman_batch(DecodeBatch &b, bool delta) {
    Ctx *c = b.c;
    const uint32_t F = b.F;
    const uint64_t *lens = b.lens;
    const uint64_t delta_max_px = delta ? delta_small_dec_max_px() : 0;
    uint64_t rgb_max_px = delta ? 0 : huf_small_dec_max_px();   // small `hufman` / `cluster-colors` frames: a workgroup per frame (delta_small_decode)
    // ---- 1. streams in device memory: the decoders of small frames are parsed there, and the host looks only at the frames that parse hands back
    std::vector<uint32_t> all;
    const SmallParseKind *parse = !b.bytes_dev ? nullptr : delta ? (delta_small_parse_off() ? nullptr : &kSmallParseDelta) : (rgb_max_px && !huf_small_parse_off() ? &kSmallParseRgb : nullptr);
    if (parse) {
        CNIIC_TRY(small_parse_dev(b, *parse, delta ? delta_max_px : rgb_max_px, delta ? 0 : huf_small_dec_floor(), all));
        if (all.empty()) return CNIIC_OK;
    } else {
        all.resize(F);
        for (uint32_t f = 0; f < F; f++) all[f] = f;
    }
    // ---- 2. the first look
    Heads heads(b);
    const std::vector<const uint8_t *> &head_p = heads.head_p;
    const std::vector<uint64_t> &head_n = heads.head_n;
    const uint32_t fa = all.front(), fb = all.back();   // (ascending)
    if (b.bytes_dev) {
        uint64_t W = 0;   // (as a single decode looks: 1/48 of the stream, 8 KiB at least, 4 MiB at most)
        for (uint32_t f : all) W = std::max(W, std::min<uint64_t>(lens[f], std::min<uint64_t>(std::max<uint64_t>(lens[f] / 48, 8192), 4ull << 20)));
        if (delta) W = std::min<uint64_t>(W, 8192);   // (what a single decode first looks at of a stream of a frame this route takes; a larger frame only shows its header)
        // (never wider than the stride, which is the source pitch of the strided copy: a stride below a header's 8 bytes reads fewer,
        // and every frame goes to the single decode)
        W = std::min<uint64_t>(std::max<uint64_t>(8, std::min(W, kBatchHeadsMax / (fb - fa + 1))), b.stride);
        if (W) CNIIC_TRY(heads.fetch(W, fa, fb));
    } else {
        heads.in_place();
    }
    // ---- 3. the floor: a call with few small frames keeps the batched route for them
    if (rgb_max_px) {
        uint32_t candidates = 0;
        for (uint32_t f : all) {
            uint64_t pos;
            uint32_t fw, fh;
            if (b.off_route[f] || !heads.dims(f, &fw, &fh, &pos)) continue;
            candidates += (uint64_t)fw * fh >= 1 && (uint64_t)fw * fh <= rgb_max_px;
        }
        if (candidates < huf_small_dec_floor()) rgb_max_px = 0;
    }
    // ---- 4. the decoders, parsed on the host
    std::vector<LeafTable> lts(delta ? 16 : F);   // (`delta`: one per parsing thread; a frame keeps its leaves in two words each, delta_tabs)
    std::vector<std::vector<uint32_t>> delta_tabs(delta || rgb_max_px ? F : 0);   // (and of the small RGB frames)
    std::vector<uint64_t> pay(F);      // where the payload starts
    std::vector<uint64_t> npx(F, 0);   // the header's pixels, of a frame whose header was read
    std::vector<Cand> cand(F, Cand::NotRouted);
    auto classify = [&](uint32_t f, uint32_t thread) {
        cand[f] = Cand::NotRouted;
        if (b.off_route[f]) return;
        uint64_t pos;
        uint32_t fw, fh;
        if (!heads.dims(f, &fw, &fh, &pos)) return;
        const uint64_t n = (uint64_t)fw * fh;
        if (!dims_fit(n, 0xffffffffull, b.img_stride)) return;
        if (delta && (n > delta_max_px || (c->scan_xy.p && c->scan_w == fw && c->scan_h == fh))) return;   // (a size with an injected scan: the single decode follows it)
        npx[f] = n;
        LeafTable &lt = lts[delta ? thread : f];
        if (!huff_parse_leaves(delta ? CNIIC_SYM_SIGNED : CNIIC_SYM_RGB, head_p[f], head_n[f], pos, lt)) { if (head_n[f] < lens[f]) cand[f] = Cand::PastHead; return; }
        if (lt.too_deep || lt.max_len > (delta ? kDeltaSmallMaxCodeLen : 32u) || lt.n() >= (1u << 20) || (lt.n() > 1 && pos >= lens[f])) return;
        const bool small_rgb = !delta && n <= rgb_max_px && lt.max_len <= kDeltaSmallMaxCodeLen;
        if (delta || small_rgb) {   // codes left-aligned in 32 bits, then key | length << 27 (delta_small_dec.hpp; an RGB key has 24 bits)
            const uint32_t L = (uint32_t)lt.n();
            std::vector<uint32_t> &tab = delta_tabs[f];
            tab.resize(2 * (size_t)L);
            for (uint32_t i = 0; i < L; i++) { tab[i] = (uint32_t)(lt.code[i] >> 32); tab[L + i] = dsd_keylen(lt.key[i], lt.len[i]); }
            if (small_rgb) lt = LeafTable();   // (the two words per leaf are all the route needs)
        }
        b.w[f] = fw; b.h[f] = fh;
        pay[f] = pos;
        cand[f] = small_rgb ? Cand::SmallRgb : Cand::Batched;
    };
    auto parse_all = [&](const std::vector<uint32_t> &which) {
        parallel_for((uint32_t)which.size(), (uint32_t)std::min<size_t>(16, which.size()), [&](uint32_t i, uint32_t thread) { classify(which[i], thread); });
    };
    parse_all(all);
    // (the frames of the workgroup-per-frame routes -- `delta`, and the RGB kinds' frames that are small by their headers -- apart from the others)
    std::vector<uint32_t> again, again_small;
    uint64_t W2 = 0, W2s = 0;
    for (uint32_t f = 0; f < F; f++)
        if (cand[f] == Cand::PastHead) {
            const bool small = delta || (npx[f] && npx[f] <= rgb_max_px);
            (small ? again_small : again).push_back(f);
            (small ? W2s : W2) = std::max(small ? W2s : W2, std::min<uint64_t>(lens[f], 4ull << 20));
        }
    if (!again_small.empty()) {
        // A small frame's decoder is most of its stream (`delta`: a leaf's 7 bytes against a code of a dozen bits; `hufman`: 12 bytes), so
        // the second look is the rule, and 4096 frames of 128 x 128 would share kBatchHeadsMax at 64 KiB each, less than their decoders.  The
        // frames are looked at again in groups of as many rows as the pinned block holds at the full width (the tables parsed from a group
        // are the frames' own)
        W2s = std::min(W2s, b.stride);
        const uint64_t rows = std::max<uint64_t>(1, kBatchHeadsMax / std::max<uint64_t>(W2s, 1));
        for (size_t g0 = 0; g0 < again_small.size();) {
            size_t g1 = g0 + 1;
            while (g1 < again_small.size() && (uint64_t)again_small[g1] - again_small[g0] + 1 <= rows) g1++;
            const uint32_t f0 = again_small[g0], f1 = again_small[g1 - 1];
            if (W2s > head_n[f0] || W2s > head_n[f1]) {
                CNIIC_TRY(heads.fetch(W2s, f0, f1));
                parse_all(std::vector<uint32_t>(again_small.begin() + g0, again_small.begin() + g1));
            }
            g0 = g1;
        }
    }
    if (!again.empty()) {   // a second, longer look at the frames whose decoders ran past the first one (one strided copy again)
        const uint32_t f0 = again.front(), f1 = again.back();
        W2 = std::min({W2, b.stride, kBatchHeadsMax / (f1 - f0 + 1)});
        if (!again_small.empty() || W2 > head_n[f0] || W2 > head_n[f1]) {   // (the small frames' look has taken the pinned block since the first one)
            CNIIC_TRY(heads.fetch(W2, f0, f1));
            parse_all(again);
        }
    }
    // ---- 5. the routes
    std::vector<uint32_t> route, small_route;
    for (uint32_t f = 0; f < F; f++) if (cand[f] == Cand::Batched) route.push_back(f); else if (cand[f] == Cand::SmallRgb) small_route.push_back(f);
    if (!small_route.empty()) CNIIC_TRY(delta_small_decode(b, kSmallDecRgb, small_route, delta_tabs, nullptr, pay));
    if (route.empty()) return CNIIC_OK;
    if (delta) return delta_small_decode(b, kSmallDecDelta, route, delta_tabs, nullptr, pay);
    return huffman_tail(b, route, lts, pay);
}

// ------------------------------------------------------------------ decode of many streams (cniic_codec_decode_batch)
// `hilbert(rle)` frames have no decoder to parse and go to rle_batch, `voronoi` frames to voronoi_batch, `zip(dict)` frames to zip_dict_batch, the others to
// huffman_batch.  Whatever
// this route does not take -- another codec, a malformed or oversized header, a decoder longer than the head that was looked at, codes of more
// than 32 bits, a frame that has not settled -- is left to the caller, which decodes it on its own (codec_decode): same bytes, same status.
int codec_decode_batch_route(Ctx *c, const CodecDesc &d, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t F, uint8_t *rgb,
                             uint64_t img_stride, uint32_t *w, uint32_t *h, std::vector<uint8_t> &taken, std::vector<int32_t> &rcs,
                             std::vector<std::string> &msgs) {
    taken.assign(F, 0);
    rcs.assign(F, CNIIC_OK);
    msgs.assign(F, std::string());
    if (!F || (d.kind != CODEC_HUFMAN && d.kind != CODEC_CLUSTER_COLORS && d.kind != CODEC_HILBERT_RLE && d.kind != CODEC_DELTA && d.kind != CODEC_VORONOI &&
               d.kind != CODEC_ZIP_DICT && d.kind != CODEC_HILBERT_ZIP))
        return CNIIC_OK;
    if (d.kind == CODEC_VORONOI && !vor_small_dec_max_px()) return CNIIC_OK;
    if (d.kind == CODEC_ZIP_DICT && !zd_small_dec_max_px()) return CNIIC_OK;
    if (d.kind == CODEC_HILBERT_ZIP && !hz_small_dec_max_px()) return CNIIC_OK;
    const bool delta = d.kind == CODEC_DELTA;
    if (delta && !delta_small_dec_max_px()) return CNIIC_OK;
    DecodeBatch b{c, bytes, is_device_ptr(bytes), stride, lens, F, rgb, is_device_ptr(rgb), img_stride, w, h, taken, rcs, msgs, std::vector<uint8_t>(F, 0)};
    if (const char *e = test_env("CNIIC_TEST_DECODE_BATCH_OFF"))
        for (const char *q = e; *q;) {
            char *end = nullptr;
            const unsigned long v = strtoul(q, &end, 10);
            if (end == q) break;
            if (v < F) b.off_route[v] = 1;
            q = *end ? end + 1 : end;
        }
    if (d.kind == CODEC_HILBERT_RLE) return rle_batch(b);
    if (d.kind == CODEC_VORONOI) return voronoi_batch(b);
    if (d.kind == CODEC_ZIP_DICT) return zip_dict_batch(b, kSmallDecZipDict);
    if (d.kind == CODEC_HILBERT_ZIP) return zip_dict_batch(b, kSmallDecHilbertZip);
    return huffman_batch(b, delta);
}

}  // namespace cniic

