// zipdict.cpp -- the dictionary coder of zip(dict) (reference: src/zip/dict.rs) up to the moment its dictionary is full, the hand-over
// to k_zipdict.hip, and the two codecs built on the coder: Zip::Dict (src/codec/zipc.rs) and Hilbert { compress: Zip }
// (src/codec/hilbertc.rs:47-49,73-77).
//
// The coder hands out u16 symbols, 0x100 upwards, one per emitted pair; after 0xFFFE -- 65 279 pairs -- Abbrev::next (dict.rs:280-290)
// answers None for good.  Until then every pair depends on the dictionary the pair before it left: that part is a serial walk and runs
// here, on one core, over a text that comes from HBM in chunks (nobody knows in advance how much of it the fill phase eats: 0.6 MB of a
// photograph, all of a flat image, whose entries double in length and never use the symbols up).  What follows it is a parse against a
// read-only trie (encode) or copies out of a text that is already there (decode): k_zipdict.hip.
#include <chrono>

#include "codec.hpp"
#include "huff_host.hpp"

namespace cniic {

namespace {

constexpr uint32_t kFirstNew = 0x100, kEof = 0xFFFF;   // Abbrev::start_after_trivial, ZIP_SPECIAL_EOF (dict.rs:6,274-278)
constexpr uint64_t kFillPairs = kEof - kFirstNew;      // 65 279

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
void host_stage(Ctx *c, const char *name, double ms) {   // a host stage among the kernel timers
    if (!c->timers) return;
    KernelTime &kt = c->ktimes[name];
    kt.ms += ms;
    kt.launches += 1;
}

// ---------------------------------------------------------------- TrieMap (dict.rs:296-323, 442-445, 604-608) as a table of edges
// An edge (node, byte) carries a child node, a symbol, both or -- never -- neither: Node::children and Node::values are independent.
// Nodes are numbered as they are made (the root is 0); there are at most as many as the fill phase read bytes.
struct HostEdge { uint32_t node, child; uint16_t sym; uint8_t byte, used; };
struct HostTrie {
    std::vector<HostEdge> tab;
    uint32_t bits = 12;
    uint64_t used = 0;
    uint32_t nnodes = 1;
    bool overflow = false;   // more than 2^32 - 2 nodes
    HostTrie() {
        tab.assign(1ull << bits, HostEdge{0, 0, (uint16_t)kEof, 0, 0});
        for (uint32_t b = 0; b < 256; b++) edge(0, (uint8_t)b).sym = (uint16_t)b;   // DictEncoder::new (dict.rs:43-47)
    }
    // Sixteen nodes numbered in a row (and one byte) share a block of sixteen slots, and the blocks are scattered: the walk along a long
    // single path (a flat image: a node per text byte, numbered as they are made) finds its next edges in lines it has just read, and
    // no run of occupied slots grows longer than hashing makes it.  Timed on one core against hashing (node, byte) as a whole: a flat
    // 2048 x 2048 image 14 s instead of 30, 34 MB of one byte 4.1-4.5 s instead of 16.4; noise a little slower (0.18-0.26 s for 4 MB against 0.16).
    uint64_t slot(uint32_t node, uint8_t b) const {
        const uint64_t block = (((((uint64_t)node >> 4) << 8) | b) * 0x9E3779B97F4A7C15ull) >> (64 - bits);
        return (block & ~15ull) | (node & 15u);
    }
    const HostEdge *find(uint32_t node, uint8_t b) const {
        const uint64_t mask = tab.size() - 1;
        for (uint64_t h = slot(node, b);; h = (h + 1) & mask) {
            const HostEdge &e = tab[h];
            if (!e.used) return nullptr;
            if (e.node == node && e.byte == b) return &e;
        }
    }
    HostEdge &edge(uint32_t node, uint8_t b) {   // found or made (the reference is good until the next call)
        if ((used + 1) * 10 > tab.size() * 7) grow();
        const uint64_t mask = tab.size() - 1;
        for (uint64_t h = slot(node, b);; h = (h + 1) & mask) {
            HostEdge &e = tab[h];
            if (!e.used) { e = HostEdge{node, 0, (uint16_t)kEof, b, 1}; used++; return e; }
            if (e.node == node && e.byte == b) return e;
        }
    }
    void grow() {
        std::vector<HostEdge> old;
        old.swap(tab);
        bits++;
        tab.assign(1ull << bits, HostEdge{0, 0, (uint16_t)kEof, 0, 0});
        const uint64_t mask = tab.size() - 1;
        for (const HostEdge &e : old) {
            if (!e.used) continue;
            uint64_t h = slot(e.node, e.byte);
            while (tab[h].used) h = (h + 1) & mask;
            tab[h] = e;
        }
    }
    // TrieMap::insert (dict.rs:308-323): the nodes on the way are made without a symbol, the last byte's edge gets it
    void insert(const uint8_t *seq, uint64_t n, uint16_t sym) {
        uint32_t node = 0;
        for (uint64_t j = 0; j + 1 < n; j++) {
            HostEdge &e = edge(node, seq[j]);
            if (!e.child) {
                if (nnodes == 0xffffffffu) { overflow = true; return; }
                e.child = nnodes++;
            }
            node = e.child;
        }
        edge(node, seq[n - 1]).sym = sym;
    }
    // the frozen trie as k_zipdict.hip reads it: at most half full
    void device_table(std::vector<ZdEdge> *out, uint32_t *out_bits) const {
        uint32_t b = 10;
        while ((1ull << b) < 2 * used) b++;
        out->assign(1ull << b, ZdEdge{kZdEmpty, 0, kZdNoSym, 0});
        const uint32_t mask = (1u << b) - 1u;
        for (const HostEdge &e : tab) {
            if (!e.used) continue;
            const uint32_t key = (e.node << 8) | e.byte;
            uint32_t h = zd_hash(key, b);
            while ((*out)[h].key != kZdEmpty) h = (h + 1) & mask;
            (*out)[h] = ZdEdge{key, e.child, e.sym, 0};
        }
        *out_bits = b;
    }
};

// the coder's input where the host can read it: all of it (a host text), or as much as has been fetched from HBM so far
struct HostText {
    Ctx *c;
    const uint8_t *dev;
    const uint8_t *p;      // avail bytes
    uint64_t avail, N;
    std::vector<uint8_t> buf;
    HostText(Ctx *ctx, const uint8_t *text_d, const uint8_t *text_h, uint64_t n) : c(ctx), dev(text_d), p(text_h), avail(text_h ? n : 0), N(n) {}
    int more() {   // the next chunk: 1 MiB, then as much again as is there, 64 MiB at most
        const uint64_t want = std::min<uint64_t>(N - avail, std::min<uint64_t>(std::max<uint64_t>(avail, 1ull << 20), 64ull << 20));
        buf.resize(avail + want);
        CNIIC_HIP_TRY(c, hipMemcpyAsync(buf.data() + avail, dev + avail, want, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
        avail += want;
        p = buf.data();
        return CNIIC_OK;
    }
};

// DictEncoder::find_symbol (dict.rs:96-136) at text position pos: the walk goes down while the node has a child for the next byte and
// remembers the deepest symbol on its way; the bytes read past it are "pushed back", i.e. the next walk starts at *end.
int longest(HostText &t, const HostTrie &trie, uint64_t pos, uint16_t *sym, uint64_t *end) {
    uint32_t node = 0;
    *end = pos;
    for (uint64_t j = pos; j < t.N;) {
        if (j >= t.avail) CNIIC_TRY(t.more());
        const HostEdge *e = trie.find(node, t.p[j]);
        j++;
        if (!e) break;
        if (e->sym != kEof) { *sym = e->sym; *end = j; }
        if (!e->child) break;
        node = e->child;
    }
    return CNIIC_OK;
}

// ---------------------------------------------------------------- DictDecoder's table (dict.rs:174-260)
// Every entry as (offset, length) of the place in the decoded text where it first stood: the output position of the pair that created
// it.  Lengths and positions saturate at kZdSat: 27 pairs can claim 2^27 bytes, 65 279 pairs 2^65279.
struct HostDec {
    std::vector<uint64_t> off, len;
    uint32_t counter = kFirstNew;
    uint64_t pairs = 0, produced = 0;
    HostDec() : off(65536, 0), len(65536, 0) {
        for (uint32_t b = 0; b < 256; b++) len[b] = 1;   // (their text is the byte itself: off unused)
    }
    static uint64_t sat(uint64_t a) { return a < kZdSat ? a : kZdSat; }
    // whole pairs of p[0, 4 npairs) from where the last call stopped, while fewer than `need` bytes are there (DictDecoder::next reads
    // a pair only when asked for a byte it does not have) and, with stop_full, while symbols are still being handed out.
    // false: a symbol that has not been handed out (mapping.get(..).unwrap(), dict.rs:238-242)
    bool scan(const uint8_t *p, uint64_t npairs, uint64_t need, bool stop_full) {
        while (pairs < npairs && produced < need && !(stop_full && counter == kEof)) {
            const uint8_t *q = p + 4 * pairs;
            const uint32_t s1 = q[0] | (q[1] << 8), s2 = q[2] | (q[3] << 8);
            if ((s1 != kEof && s1 >= counter) || (s2 != kEof && s2 >= counter)) return false;
            const uint64_t l = sat(len[s1] + len[s2]);
            if (counter != kEof) { off[counter] = produced; len[counter] = l; counter++; }
            produced = sat(produced + l);
            pairs++;
        }
        return true;
    }
    // the text of the pairs scanned so far, as far as it lies below `limit`, into out
    void write(const uint8_t *p, uint8_t *out, uint64_t limit) const {
        uint64_t o = 0;
        for (uint64_t k = 0; k < pairs && o < limit; k++)
            for (int i = 0; i < 2 && o < limit; i++) {
                const uint32_t s = p[4 * k + 2 * i] | (p[4 * k + 2 * i + 1] << 8);
                if (s == kEof) continue;
                if (s < 256) { out[o++] = (uint8_t)s; continue; }
                const uint64_t n = std::min(len[s], limit - o);
                memcpy(out + o, out + off[s], n);   // (the source ends where the pair that made s ended: before o)
                o += n;
            }
    }
};

// the first `want` bytes of a stream where the host can read them
int stream_front(Ctx *c, const uint8_t *bytes, bool bytes_dev, uint64_t n, uint64_t want, std::vector<uint8_t> *store, const uint8_t **p, uint64_t *pn) {
    if (!bytes_dev) { *p = bytes; *pn = n; return CNIIC_OK; }   // (all of it)
    *pn = std::min(n, want);
    store->resize(*pn);
    if (*pn) {
        CNIIC_HIP_TRY(c, hipMemcpyAsync(store->data(), bytes, *pn, hipMemcpyDeviceToHost, c->stream));
        CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *p = store->data();
    return CNIIC_OK;
}

// The text of the stream bytes[0, n) -- all of it (need == ~0: zip_dict_decode(..).collect()), or what the reference's lazy reader has
// decoded when it has handed out `need` bytes: whole pairs while fewer than `need` are there, nothing behind them looked at.  *text_len
// = min(the text's length, need) bytes in *text (HBM).  room: the most the text may take (CNIIC_ERR_CAPACITY, *text_len = its length).
// CNIIC_ERR_DECODE where the reference panics on the way.  front / front_n: the stream's first bytes on the host (4 kFillPairs, or all).
int decode_text(Ctx *c, const uint8_t *bytes, bool bytes_dev, uint64_t n, const uint8_t *front, uint64_t front_n, uint64_t need, uint64_t room,
                DevBuf *text, uint64_t *text_len) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t npairs = n / 4;
    const bool dangling = (n & 3) >= 2;   // a first symbol without a second (next_symbol().unwrap(), dict.rs:193); one byte alone ends the stream (:192)
    HostDec dec;
    if (!dec.scan(front, std::min({npairs, kFillPairs, front_n / 4}), need, true))
        return c->fail(CNIIC_ERR_DECODE, "zip-dict: pair %llu uses a symbol that has not been handed out", (unsigned long long)dec.pairs);
    uint64_t total = dec.produced;
    ZdExpand ex;
    DevBuf up;
    if (dec.produced < need && dec.pairs < npairs) {   // the dictionary is full and the stream goes on
        const uint64_t nsym = 2 * (npairs - dec.pairs);
        const uint8_t *syms_d = bytes + 4 * dec.pairs;
        if (!bytes_dev) {
            CNIIC_HIP_TRY(c, up.alloc(2 * nsym));
            CNIIC_HIP_TRY(c, hipMemcpyAsync(up.p, syms_d, 2 * nsym, hipMemcpyHostToDevice, c->stream));
            syms_d = up.as<uint8_t>();
        }
        std::vector<uint64_t> dlen(dec.len);
        for (uint64_t &l : dlen) l = std::min(l, kZdLenClamp);
        host_stage(c, "zd_prefix_host", ms_since(t0));
        CNIIC_TRY(zd_expand_plan(c, syms_d, nsym, dec.off.data(), dlen.data(), &ex));
        total = HostDec::sat(total + ex.total);
    } else {
        host_stage(c, "zd_prefix_host", ms_since(t0));
    }
    if (total < need && dangling) return c->fail(CNIIC_ERR_DECODE, "zip-dict: a first symbol without a second at the end of the stream");
    *text_len = std::min(total, need);
    if (*text_len > room) return c->fail(CNIIC_ERR_CAPACITY, "zip-dict: the text has %llu bytes, capacity %llu", (unsigned long long)*text_len, (unsigned long long)room);
    // (nothing has been allocated from a claimed size up to here)
    CNIIC_HIP_TRY(c, text->alloc(*text_len));
    const auto t1 = std::chrono::steady_clock::now();
    const uint64_t base = std::min(dec.produced, *text_len);
    std::vector<uint8_t> prefix(base);
    dec.write(front, prefix.data(), base);
    if (base) CNIIC_HIP_TRY(c, hipMemcpyAsync(text->p, prefix.data(), base, hipMemcpyHostToDevice, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    host_stage(c, "zd_prefix_host", ms_since(t1));
    if (ex.nsym) CNIIC_TRY(zd_expand_copy(c, &ex, dec.produced, text->as<uint8_t>(), *text_len));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

int put_pixels(Ctx *c, const uint8_t *src_d, uint64_t bytes, uint8_t *dst) {
    if (!bytes) return CNIIC_OK;
    CNIIC_HIP_TRY(c, hipMemcpyAsync(dst, src_d, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CNIIC_OK;
}

}  // namespace

// ---------------------------------------------------------------- zip_dict_encode (dict.rs:8-19)
int zip_dict_encode_text(Ctx *c, const uint8_t *text_d, const uint8_t *text_h, uint64_t N, const std::vector<uint8_t> &head, uint8_t *out, uint64_t cap,
                         uint64_t *len) {
    const auto t0 = std::chrono::steady_clock::now();
    HostText text(c, text_d, text_h, N);
    HostTrie trie;
    std::vector<uint8_t> header(head);
    auto put_sym = [&](uint32_t s) { header.push_back((uint8_t)s); header.push_back((uint8_t)(s >> 8)); };
    uint32_t counter = kFirstNew;
    uint64_t pos = 0, max_entry = 1;
    bool frozen = false;
    // DictEncoder::next_pair (dict.rs:66-94), until the pair that hands out 0xFFFE.  A trie the device table cannot number (a flat
    // stretch of 32 M bytes before the dictionary filled), or one with an entry so long that the match kernel's walks would not end in
    // reasonable time (kZdMaxEntry), stays here to the end of the text: the same answers, one core.
    while (pos < N) {
        if (counter == kEof && trie.nnodes <= kZdMaxNodes && max_entry <= kZdMaxEntry) { frozen = true; break; }
        uint16_t s1 = 0, s2 = (uint16_t)kEof;
        uint64_t mid = pos, end = pos;
        CNIIC_TRY(longest(text, trie, pos, &s1, &mid));
        end = mid;
        if (mid < N) CNIIC_TRY(longest(text, trie, mid, &s2, &end));   // (else: (symbol1, ZIP_SPECIAL_EOF), dict.rs:81-86)
        put_sym(s1);
        put_sym(s2);
        if (mid < N && counter != kEof) {   // create_symbol(seq1 ++ seq2) behind both walks (dict.rs:90-92)
            trie.insert(text.p + pos, end - pos, (uint16_t)counter++);
            if (trie.overflow) return c->fail(CNIIC_ERR_UNSUPPORTED, "zip-dict: more than 2^32 trie nodes");
            max_entry = std::max(max_entry, end - pos);
        }
        pos = end;
    }
    host_stage(c, "zd_fill_host", ms_since(t0));
    StreamOut so(c, out, cap, len);
    if (!frozen) {
        CNIIC_TRY(so.begin(header, 0));
        return so.finish();
    }
    std::vector<ZdEdge> table;
    uint32_t bits = 0;
    const auto t1 = std::chrono::steady_clock::now();
    trie.device_table(&table, &bits);
    host_stage(c, "zd_table_host", ms_since(t1));
    ZdFrozen plan;
    CNIIC_TRY(zd_frozen_plan(c, text_d, N, pos, table.data(), bits, max_entry, &plan));
    CNIIC_TRY(so.begin_sized(header.size(), 2 * (plan.nsyms + (plan.nsyms & 1)), /*zero=*/false));   // (whole pairs behind an even header: every byte is written)
    CNIIC_TRY(so.put_header(header));
    CNIIC_TRY(zd_frozen_emit(c, &plan, reinterpret_cast<uint16_t *>(so.dev + header.size())));
    return so.finish();
}

int zip_dict_decode_bytes(Ctx *c, const uint8_t *bytes, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *len) {
    const bool bytes_dev = is_device_ptr(bytes);
    std::vector<uint8_t> store;
    const uint8_t *front = nullptr;
    uint64_t front_n = 0;
    CNIIC_TRY(stream_front(c, bytes, bytes_dev, n, 4 * kFillPairs, &store, &front, &front_n));
    DevBuf text;
    CNIIC_TRY(decode_text(c, bytes, bytes_dev, n, front, front_n, ~0ull, cap, &text, len));
    return put_pixels(c, text.as<uint8_t>(), *len, out);
}

// the first 8 bytes of the text: Deserialize for (u32, u32) at the head of rebuild_image (zipc.rs:28-30)
int zip_dict_dims(const uint8_t *bytes, uint64_t n, uint32_t *w, uint32_t *h) {
    HostDec dec;
    if (!dec.scan(bytes, n / 4, 8, false) || dec.produced < 8) return CNIIC_ERR_DECODE;
    uint8_t t[8];
    dec.write(bytes, t, 8);
    *w = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
    *h = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    return CNIIC_OK;
}

// ---------------------------------------------------------------- Zip::Dict (zipc.rs:14-48)
int encode_zip_dict(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    const uint64_t n = (uint64_t)w * h, N = 8 + 11 * n;
    DevBuf text;
    CNIIC_HIP_TRY(c, text.alloc(N));
    CNIIC_TRY(zd_serialize(c, rgb_d, n, true, w, h, text.as<uint8_t>()));   // SerStream of the dimensions, then of the pixels (zipc.rs:16-19)
    return zip_dict_encode_text(c, text.as<uint8_t>(), nullptr, N, {}, out, cap, len);
}

int decode_zip_dict(Ctx *c, const uint8_t *bytes, uint64_t nbytes, uint8_t *rgb_out, uint64_t cap, uint32_t *w, uint32_t *h) {
    const bool bytes_dev = is_device_ptr(bytes);
    std::vector<uint8_t> store;
    const uint8_t *front = nullptr;
    uint64_t front_n = 0;
    CNIIC_TRY(stream_front(c, bytes, bytes_dev, nbytes, 4 * kFillPairs, &store, &front, &front_n));
    int rc_dims = zip_dict_dims(front, front_n, w, h);
    if (rc_dims != CNIIC_OK && front_n < nbytes) {   // (65 279 pairs that spell fewer than 8 bytes: empty texts.  The whole stream then.)
        CNIIC_TRY(stream_front(c, bytes, bytes_dev, nbytes, nbytes, &store, &front, &front_n));
        rc_dims = zip_dict_dims(front, front_n, w, h);
    }
    if (rc_dims != CNIIC_OK) return c->fail(CNIIC_ERR_DECODE, "zip-dict: no dimensions");
    const uint64_t n = (uint64_t)*w * *h;
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_DECODE, "decode: image too large");
    if (n * 3 > cap) return c->fail(CNIIC_ERR_CAPACITY, "decode: image needs %llu bytes, capacity %llu", (unsigned long long)(n * 3), (unsigned long long)cap);
    // rebuild_image pulls exactly 8 + 11 w h bytes (zipc.rs:28-36): what lies behind the pair that completes them is never looked at
    const uint64_t need = 8 + 11 * n;
    DevBuf text, img_d;
    uint64_t got = 0;
    CNIIC_TRY(decode_text(c, bytes, bytes_dev, nbytes, front, front_n, need, need, &text, &got));
    if (got < need) return c->fail(CNIIC_ERR_DECODE, "zip-dict: the text ends after %llu of %llu bytes", (unsigned long long)got, (unsigned long long)need);
    if (!n) return CNIIC_OK;
    uint8_t *dst = rgb_out;
    const bool dst_dev = is_device_ptr(rgb_out);
    if (!dst_dev) { CNIIC_HIP_TRY(c, img_d.alloc(n * 3)); dst = img_d.as<uint8_t>(); }
    uint64_t bad = n;
    CNIIC_TRY(zd_unserialize(c, text.as<uint8_t>() + 8, n, dst, &bad));
    if (bad < n) return c->fail(CNIIC_ERR_DECODE, "zip-dict: pixel %llu is not a record of 3 bytes (ser.rs:216-221)", (unsigned long long)bad);
    return dst_dev ? CNIIC_OK : put_pixels(c, dst, n * 3, rgb_out);
}

// ---------------------------------------------------------------- Hilbert { compress: Zip } (hilbertc.rs:27-29,47-49,67-77)
int encode_hilbert_zip(Ctx *c, const uint8_t *rgb_d, uint32_t w, uint32_t h, uint8_t *out, uint64_t cap, uint64_t *len) {
    const uint64_t n = (uint64_t)w * h;
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_BAD_ARG, "image too large");
    std::vector<uint8_t> header;
    put_u32(header, w);   // img.dimensions().serialize (:27), outside the coder
    put_u32(header, h);
    DevBuf lin, text;
    CNIIC_HIP_TRY(c, lin.alloc(n * 3));
    CNIIC_HIP_TRY(c, text.alloc(11 * n));
    if (n) CNIIC_TRY(hilbert_linearize(c, rgb_d, w, h, lin.as<uint8_t>()));   // hilbert::linearize (:29)
    CNIIC_TRY(zd_serialize(c, lin.as<uint8_t>(), n, false, 0, 0, text.as<uint8_t>()));
    return zip_dict_encode_text(c, text.as<uint8_t>(), nullptr, 11 * n, header, out, cap, len);
}

int decode_hilbert_zip(Ctx *c, const uint8_t *bytes, uint64_t nbytes, uint8_t *rgb_out, uint64_t cap, uint32_t *w, uint32_t *h) {
    const bool bytes_dev = is_device_ptr(bytes);
    std::vector<uint8_t> store;
    const uint8_t *front = nullptr;
    uint64_t front_n = 0, pos = 0;
    CNIIC_TRY(stream_front(c, bytes, bytes_dev, nbytes, 8 + 4 * kFillPairs, &store, &front, &front_n));
    if (!get_u32(front, front_n, pos, *w) || !get_u32(front, front_n, pos, *h)) return c->fail(CNIIC_ERR_DECODE, "decode: truncated dimensions");
    const uint64_t n = (uint64_t)*w * *h;
    if (n >= (1ull << 32)) return c->fail(CNIIC_ERR_DECODE, "decode: image too large");
    if (n * 3 > cap) return c->fail(CNIIC_ERR_CAPACITY, "decode: image needs %llu bytes, capacity %llu", (unsigned long long)(n * 3), (unsigned long long)cap);
    if (!n) return CNIIC_OK;
    // the traversal asks for w h colours and no more (:59-62); colours the text does not reach stay zero (ImageBuffer::new), and so
    // do those from a record on whose length is not 3, which ends deser_stream (ser.rs:216-221, :269-271)
    const uint64_t need = 11 * n;
    DevBuf text, lin, img_d;
    uint64_t got = 0;
    CNIIC_TRY(decode_text(c, bytes + 8, bytes_dev, nbytes - 8, front + 8, front_n - 8, need, need, &text, &got));
    CNIIC_HIP_TRY(c, lin.alloc(n * 3));
    uint64_t have = got / 11, bad = have;
    CNIIC_TRY(zd_unserialize(c, text.as<uint8_t>(), have, lin.as<uint8_t>(), &bad));
    have = std::min(have, bad);
    if (have < n) CNIIC_HIP_TRY(c, hipMemsetAsync(lin.as<uint8_t>() + 3 * have, 0, 3 * (n - have), c->stream));
    uint8_t *dst = rgb_out;
    const bool dst_dev = is_device_ptr(rgb_out);
    if (!dst_dev) { CNIIC_HIP_TRY(c, img_d.alloc(n * 3)); dst = img_d.as<uint8_t>(); }
    CNIIC_TRY(hilbert_scatter(c, lin.as<uint8_t>(), *w, *h, dst));   // follow the traversal (:58-61)
    CNIIC_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return dst_dev ? CNIIC_OK : put_pixels(c, dst, n * 3, rgb_out);
}

}  // namespace cniic
