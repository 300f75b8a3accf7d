// zipback.cpp -- the host side of zip(back): the look-back coder on plain bytes (reference: src/zip/back.rs) and the codec Zip::Back
// (src/codec/zipc.rs:14-48) for one image and for a folder of them.  k_zipback.hip parses and expands; the text of an image and the way
// back from it are zip(dict)'s (zd_serialize, zd_unserialize in k_zipdict.hip).
//
// Everything here is a batch: the single calls are batches of one.  The streams of a call are the blocks of the same launches, so a
// folder of images keeps as many CUs busy as it has images.
#include "codec.hpp"

namespace cniic {

namespace {

struct Verdict { int32_t rc = CNIIC_OK; std::string msg; };

Verdict verdict(int32_t rc, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return Verdict{rc, buf};
}

// the call's answer from its frames': the first failure and its message
int first_failure(Ctx *c, const std::vector<Verdict> &v, int32_t *rcs, std::vector<std::string> *msgs) {
    int rc = CNIIC_OK;
    if (msgs) msgs->assign(v.size(), std::string());
    for (size_t f = 0; f < v.size(); f++) {
        if (rcs) rcs[f] = v[f].rc;
        if (msgs) (*msgs)[f] = v[f].msg;
        if (rc == CNIIC_OK && v[f].rc != CNIIC_OK) rc = c->fail(v[f].rc, "%s", v[f].msg.c_str());
    }
    return rc;
}

int copy_out(Ctx *c, uint8_t *dst, const uint8_t *src_d, uint64_t bytes) {   // enqueued
    if (bytes) CNIIC_HIP_TRY(c, hipMemcpyAsync(dst, src_d, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    return CNIIC_OK;
}

// One text of an encode call: text_d[0, n) in HBM to out[0, cap), host or device.
struct EncJob { const uint8_t *text_d = nullptr; uint64_t n = 0; uint8_t *out = nullptr; uint64_t cap = 0; uint64_t len = 0; Verdict v; };

// zip_back_encode (back.rs:5-16) of every job whose verdict is still CNIIC_OK; len: the stream's length, also where it did not fit
int encode_jobs(Ctx *c, std::vector<EncJob> &jobs) {
    std::vector<ZbStream> streams;
    std::vector<uint32_t> who;
    std::vector<DevBuf> staging(jobs.size());
    for (uint32_t j = 0; j < jobs.size(); j++) {
        EncJob &job = jobs[j];
        if (job.v.rc != CNIIC_OK) continue;
        ZbStream s{job.text_d, job.n, job.out, job.cap, 0};
        if (!is_device_ptr(job.out)) {   // (no stream is longer than zb_stream_bound: room for that much is room for all of it)
            s.cap = std::min(job.cap, zb_stream_bound(job.n));
            CNIIC_HIP_TRY(c, staging[j].alloc(s.cap));
            s.out = staging[j].as<uint8_t>();
        }
        streams.push_back(s);
        who.push_back(j);
    }
    std::vector<ZbState> states(streams.size());
    CNIIC_TRY(zb_encode_streams(c, streams.data(), (uint32_t)streams.size(), states.data()));
    for (uint32_t i = 0; i < who.size(); i++) {
        EncJob &job = jobs[who[i]];
        const ZbState &st = states[i];
        job.len = st.o;
        if (st.status == kZbBadExplicit)
            job.v = verdict(CNIIC_ERR_UNSUPPORTED, "zip-back: an explicit symbol of 32768 bytes at text position %llu: the reference's header cannot say it and its assertion fails (back.rs:45)",
                            (unsigned long long)(st.p - st.e));
        else if (st.status == kZbBadLookback)
            job.v = verdict(CNIIC_ERR_UNSUPPORTED, "zip-back: a look-back of 32768 bytes or more at text position %llu: the reference's header cannot say it and its assertion fails (back.rs:45)",
                            (unsigned long long)st.p);
        else if (st.o > job.cap)
            job.v = verdict(CNIIC_ERR_CAPACITY, "encode: stream is %llu bytes, capacity %llu", (unsigned long long)st.o, (unsigned long long)job.cap);
        else if (streams[i].out != job.out)
            CNIIC_TRY(copy_out(c, job.out, streams[i].out, st.o));
        if (job.v.rc != CNIIC_OK && job.v.rc != CNIIC_ERR_CAPACITY) job.len = 0;
    }
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// One stream of a decode call: bytes_d[0, n) in HBM, its text to out_d[0, cap) in HBM, whole symbols while fewer than need are there.
struct DecJob { const uint8_t *bytes_d = nullptr; uint64_t n = 0, need = 0; uint8_t *out_d = nullptr; uint64_t cap = 0; uint64_t made = 0; Verdict v; };

// The floor of the whole-GPU decode (k_zipback_par.hip), in stream bytes, for a call of `streams` streams: a stream below it is walked by
// the serial kernel.  kZbParMaxStreams / kZbParFloorBytes (common.hpp) are the classes tools/zip_back_probe.py found clear of the serial
// walk for photo-like and noise alike (NOTES AW): calls of one stream of 512 KiB or more.  The testing library can turn the route off
// (CNIIC_TEST_ZB_PAR_OFF=1; a run with CNIIC_TEST_ZB_SLICE set counts the serial kernel's launches and takes it off too) and lower the
// floor (CNIIC_TEST_ZB_PAR_MIN, bytes, for calls of any number of streams; never higher).
uint64_t zb_par_floor(uint32_t streams) {
    if (const char *e = test_env("CNIIC_TEST_ZB_PAR_OFF")) if (atoi(e) != 0) return ~0ull;
    if (test_env("CNIIC_TEST_ZB_SLICE")) return ~0ull;
    uint64_t floor = streams <= kZbParMaxStreams ? kZbParFloorBytes : ~0ull;
    if (const char *e = test_env("CNIIC_TEST_ZB_PAR_MIN")) floor = std::min<uint64_t>(floor, strtoull(e, nullptr, 10));
    return floor;
}

int decode_jobs(Ctx *c, std::vector<DecJob> &jobs) {
    std::vector<ZbStream> streams;
    std::vector<uint32_t> who;
    for (uint32_t j = 0; j < jobs.size(); j++) {
        if (jobs[j].v.rc != CNIIC_OK) continue;
        streams.push_back(ZbStream{jobs[j].bytes_d, jobs[j].n, jobs[j].out_d, jobs[j].cap, jobs[j].need});
        who.push_back(j);
    }
    std::vector<ZbState> states(streams.size());
    // the whole-GPU route (k_zipback_par.hip), a stream at a time; what it does not take, or hands back, is the serial kernel's
    std::vector<uint32_t> serial;
    const uint64_t floor = zb_par_floor((uint32_t)streams.size());
    uint32_t round_cap = 32;
    if (const char *e = test_env("CNIIC_TEST_ZB_PAR_ROUNDS")) round_cap = std::min<uint32_t>(round_cap, (uint32_t)strtoul(e, nullptr, 10));
    uint64_t decoded = 0, handed_back = 0, rounds_all = 0;
    {
        ScopedKernelTimer timer(c, "zb_par_decode");
        for (uint32_t i = 0; i < streams.size(); i++) {
            const ZbStream &s = streams[i];
            if (s.n < floor || s.n < 1 || s.n >= (1ull << 32) || zb_par_stream_scratch(s.n) > kZbParScratchMax) { serial.push_back(i); continue; }
            uint32_t rounds = 0;
            bool handed = false;
            CNIIC_TRY(zb_par_decode_stream(c, s, round_cap, &states[i], &rounds, &handed));
            rounds_all += rounds;
            if (handed) { handed_back++; serial.push_back(i); } else decoded++;
        }
        if (decoded + handed_back) timer.stop(decoded);
    }
    if (c->timers && decoded + handed_back) { c->ktimes["zb_par_handback"].launches += handed_back; c->ktimes["zb_par_rounds"].launches += rounds_all; }
    if (serial.size() == streams.size()) {
        CNIIC_TRY(zb_decode_streams(c, streams.data(), (uint32_t)streams.size(), states.data()));
    } else if (!serial.empty()) {
        std::vector<ZbStream> rest(serial.size());
        std::vector<ZbState> rest_states(serial.size());
        for (uint32_t i = 0; i < serial.size(); i++) rest[i] = streams[serial[i]];
        CNIIC_TRY(zb_decode_streams(c, rest.data(), (uint32_t)rest.size(), rest_states.data()));
        for (uint32_t i = 0; i < serial.size(); i++) states[serial[i]] = rest_states[i];
    }
    for (uint32_t i = 0; i < who.size(); i++) {
        DecJob &job = jobs[who[i]];
        const ZbState &st = states[i];
        job.made = st.o;
        if (st.status == kZbBadExplicit)
            job.v = verdict(CNIIC_ERR_DECODE, "zip-back: the explicit symbol at stream byte %llu is cut short (back.rs:97)", (unsigned long long)st.p);
        else if (st.status == kZbBadLookback)
            job.v = verdict(CNIIC_ERR_DECODE, "zip-back: the look-back at stream byte %llu reaches behind the start of the text (back.rs:466)", (unsigned long long)st.p);
    }
    return CNIIC_OK;
}

// the streams of a decode call where the kernel can read them: as they lie (HBM), or copied into one buffer
int streams_to_device(Ctx *c, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t F, DevBuf *store, std::vector<const uint8_t *> *at) {
    at->assign(F, nullptr);
    if (is_device_ptr(bytes)) {
        for (uint32_t f = 0; f < F; f++) (*at)[f] = bytes + f * stride;
        return CNIIC_OK;
    }
    uint64_t total = 0;
    for (uint32_t f = 0; f < F; f++) total += lens[f];
    CNIIC_HIP_TRY(c, store->alloc(total));
    uint64_t off = 0;
    for (uint32_t f = 0; f < F; f++) {
        (*at)[f] = store->as<uint8_t>() + off;
        if (lens[f]) CNIIC_HIP_TRY(c, hipMemcpyAsync(store->as<uint8_t>() + off, bytes + f * stride, lens[f], hipMemcpyHostToDevice, c->stream));
        off += lens[f];
    }
    return CNIIC_OK;
}

// The first 8 bytes of the text of a stream of `total` bytes whose first `avail` are at p, decoded as the lazy reader would for 8 bytes.
constexpr uint64_t kZbFront = 64;   // (an explicit symbol of one byte and seven look-backs of one: 31 bytes of stream at the most, then a header)
bool text_front(const uint8_t *p, uint64_t avail, uint64_t total, uint8_t *t) {
    uint64_t pos = 0, o = 0;
    while (o < 8) {
        if (pos + 2 > total || pos + 2 > avail) return false;
        const uint32_t head = p[pos] | (p[pos + 1] << 8), len = head & 0x7fffu;
        pos += 2;
        uint32_t k;
        if (head & 0x8000u) {
            if (pos + 2 > total || pos + 2 > avail) return false;
            const uint32_t back = p[pos] | (p[pos + 1] << 8);
            pos += 2;
            if (back > o) return false;
            k = std::min(len, back);
            for (uint32_t i = 0; i < k && o + i < 8; i++) t[o + i] = t[o - back + i];
        } else {
            if (pos + len > total) return false;
            k = len;
            for (uint32_t i = 0; i < k && o + i < 8; i++) {
                if (pos + i >= avail) return false;
                t[o + i] = p[pos + i];
            }
            pos += len;
        }
        if (!k) return false;
        o += k;
    }
    return true;
}

}  // namespace

int zip_back_encode_text(Ctx *c, const uint8_t *text_d, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    std::vector<EncJob> jobs(1);
    jobs[0].text_d = text_d; jobs[0].n = n; jobs[0].out = out; jobs[0].cap = cap;
    CNIIC_TRY(encode_jobs(c, jobs));
    *len = jobs[0].len;
    return jobs[0].v.rc == CNIIC_OK ? CNIIC_OK : c->fail(jobs[0].v.rc, "%s", jobs[0].v.msg.c_str());
}

int zip_back_decode_bytes(Ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    DevBuf store, text;
    std::vector<const uint8_t *> at;
    CNIIC_TRY(streams_to_device(c, bytes, 0, &n, 1, &store, &at));
    std::vector<DecJob> jobs(1);
    jobs[0].bytes_d = at[0]; jobs[0].n = n; jobs[0].need = ~0ull;
    jobs[0].out_d = out;
    jobs[0].cap = cap;
    if (!is_device_ptr(out)) {   // (nothing is allocated from a size the stream claims: zb_text_bound is what n bytes can spell)
        jobs[0].cap = std::min(cap, zb_text_bound(n));
        CNIIC_HIP_TRY(c, text.alloc(jobs[0].cap));
        jobs[0].out_d = text.as<uint8_t>();
    }
    CNIIC_TRY(decode_jobs(c, jobs));
    if (jobs[0].v.rc != CNIIC_OK) return c->fail(jobs[0].v.rc, "%s", jobs[0].v.msg.c_str());
    *len = jobs[0].made;
    if (*len > cap) return c->fail(CNIIC_ERR_CAPACITY, "zip-back: the text has %llu bytes, capacity %llu", (unsigned long long)*len, (unsigned long long)cap);
    if (jobs[0].out_d != out) CNIIC_TRY(copy_out(c, out, jobs[0].out_d, *len));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

// the first 8 bytes of the text: Deserialize for (u32, u32) at the head of rebuild_image (zipc.rs:28-30)
int zip_back_dims(const uint8_t *bytes, uint64_t avail, uint64_t total, uint32_t *w, uint32_t *h) {
    uint8_t t[8];
    if (!text_front(bytes, avail, total, t)) return CNIIC_ERR_DECODE;
    *w = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
    *h = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    return CNIIC_OK;
}

// ---------------------------------------------------------------- Zip::Back (zipc.rs:14-48), a folder at a time
int encode_zip_back_batch(Ctx *c, const uint8_t *rgb, const uint64_t *img_off, const uint32_t *w, const uint32_t *h, uint32_t F, uint8_t *out, uint64_t stride,
                          uint64_t *lens, int32_t *rcs, std::vector<std::string> *msgs) {
    std::vector<EncJob> jobs(F);
    std::vector<In<uint8_t>> img(F);
    std::vector<uint64_t> text_at(F, 0);
    uint64_t total = 0;
    for (uint32_t f = 0; f < F; f++) {
        const uint64_t n = (uint64_t)w[f] * h[f];
        lens[f] = 0;
        if (n >= (1ull << 32)) { jobs[f].v = verdict(CNIIC_ERR_BAD_ARG, "image too large"); continue; }
        text_at[f] = total;
        total += (8 + 11 * n + 255) & ~255ull;
    }
    DevBuf text;
    CNIIC_HIP_TRY(c, text.alloc(total));
    for (uint32_t f = 0; f < F; f++) {
        if (jobs[f].v.rc != CNIIC_OK) continue;
        const uint64_t n = (uint64_t)w[f] * h[f];
        CNIIC_TRY(img[f].bind(c, rgb + img_off[f], n * 3));
        jobs[f].text_d = text.as<uint8_t>() + text_at[f];
        jobs[f].n = 8 + 11 * n;
        jobs[f].out = out + f * stride;
        jobs[f].cap = stride;
        // SerStream of the dimensions, then of the pixels (zipc.rs:16-19)
        CNIIC_TRY(zd_serialize(c, img[f].d, n, true, w[f], h[f], text.as<uint8_t>() + text_at[f], "zb_serialize"));
    }
    CNIIC_TRY(encode_jobs(c, jobs));
    std::vector<Verdict> v(F);
    for (uint32_t f = 0; f < F; f++) { lens[f] = jobs[f].len; v[f] = jobs[f].v; }
    return first_failure(c, v, rcs, msgs);
}

int decode_zip_back_batch(Ctx *c, const uint8_t *bytes, uint64_t stride, const uint64_t *lens, uint32_t F, uint8_t *rgb, uint64_t img_stride, uint32_t *w,
                          uint32_t *h, int32_t *rcs, std::vector<std::string> *msgs) {
    std::vector<DecJob> jobs(F);
    DevBuf store, text, img_d;
    std::vector<const uint8_t *> at;
    CNIIC_TRY(streams_to_device(c, bytes, stride, lens, F, &store, &at));
    // the dimensions: the head of every stream on the host
    const bool bytes_dev = is_device_ptr(bytes);
    std::vector<uint8_t> fronts;
    if (bytes_dev) {
        fronts.resize((uint64_t)F * kZbFront);
        for (uint32_t f = 0; f < F; f++)
            if (lens[f]) CNIIC_HIP_TRY(c, hipMemcpyAsync(fronts.data() + f * kZbFront, at[f], std::min(lens[f], kZbFront), hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    std::vector<uint64_t> text_at(F, 0);
    uint64_t total = 0, img_total = 0;
    const bool rgb_dev = is_device_ptr(rgb);
    for (uint32_t f = 0; f < F; f++) {
        w[f] = h[f] = 0;
        const uint8_t *front = bytes_dev ? fronts.data() + f * kZbFront : bytes + f * stride;
        if (zip_back_dims(front, bytes_dev ? std::min(lens[f], kZbFront) : lens[f], lens[f], &w[f], &h[f]) != CNIIC_OK) {
            jobs[f].v = verdict(CNIIC_ERR_DECODE, "zip-back: no dimensions");
            continue;
        }
        const uint64_t n = (uint64_t)w[f] * h[f];
        if (n >= (1ull << 32)) { jobs[f].v = verdict(CNIIC_ERR_DECODE, "decode: image too large"); continue; }
        if (n * 3 > img_stride) {
            jobs[f].v = verdict(CNIIC_ERR_CAPACITY, "decode: image needs %llu bytes, capacity %llu", (unsigned long long)(n * 3), (unsigned long long)img_stride);
            continue;
        }
        // rebuild_image pulls exactly 8 + 11 w h bytes (zipc.rs:28-36): what lies behind the symbol that completes them is never looked at
        jobs[f].bytes_d = at[f];
        jobs[f].n = lens[f];
        jobs[f].need = jobs[f].cap = 8 + 11 * n;
        text_at[f] = total;
        total += (jobs[f].need + 255) & ~255ull;
        img_total += (n * 3 + 255) & ~255ull;
    }
    CNIIC_HIP_TRY(c, text.alloc(total));
    if (!rgb_dev) CNIIC_HIP_TRY(c, img_d.alloc(img_total));
    for (uint32_t f = 0; f < F; f++) jobs[f].out_d = text.as<uint8_t>() + text_at[f];
    CNIIC_TRY(decode_jobs(c, jobs));
    uint64_t img_at = 0;
    for (uint32_t f = 0; f < F; f++) {
        DecJob &job = jobs[f];
        if (job.v.rc != CNIIC_OK) continue;
        const uint64_t n = (uint64_t)w[f] * h[f];
        if (job.made < job.need) {
            job.v = verdict(CNIIC_ERR_DECODE, "zip-back: the text ends after %llu of %llu bytes", (unsigned long long)job.made, (unsigned long long)job.need);
            continue;
        }
        if (!n) continue;
        uint8_t *dst = rgb_dev ? rgb + f * img_stride : img_d.as<uint8_t>() + img_at;
        img_at += (n * 3 + 255) & ~255ull;
        uint64_t bad = n;
        CNIIC_TRY(zd_unserialize(c, job.out_d + 8, n, dst, &bad, "zb_rebuild"));
        if (bad < n) {
            job.v = verdict(CNIIC_ERR_DECODE, "zip-back: pixel %llu is not a record of 3 bytes (ser.rs:216-221)", (unsigned long long)bad);
            continue;
        }
        if (!rgb_dev) CNIIC_TRY(copy_out(c, rgb + f * img_stride, dst, n * 3));
    }
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<Verdict> v(F);
    for (uint32_t f = 0; f < F; f++) v[f] = jobs[f].v;
    return first_failure(c, v, rcs, msgs);
}

}  // namespace cniic
