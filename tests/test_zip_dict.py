"""zip(dict) and hilbert-zip on the GPU against the CPU restatement of the reference's dictionary coder (tests/zip_dict_ref.py / .c):
byte-exact streams, images back, the reference's verdict on hostile streams.  Each image is the smallest that reaches the code it
names (the byte positions come from the restatement and are asserted as properties: which side of the hand-over, how long the longest
entry).  The edges of those code paths -- the thresholds the kernels switch on -- are tests/test_zip_dict_edges.py's."""
import struct

import numpy as np
import pytest

import zip_dict_ref as Z

pytestmark = pytest.mark.gpu

EXPR = "zip(dict)"
FILL_BYTES = 4 * Z.MAX_PAIRS    # a stream's first 261 116 bytes are written while the dictionary fills


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_dict_ref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


IMAGES = {
    "1x1": lambda: Z.noise(1, 1),
    "3x2": lambda: Z.noise(3, 2),
    "flat 256x192": lambda: Z.flat(256, 192),
    "noise 256x192": lambda: Z.noise(256, 192),
    "noise 320x200": lambda: Z.noise(320, 200),
    "photo-like 320x200": lambda: Z.photo_like(320, 200),
    "photo-like 512x384": lambda: Z.photo_like(512, 384),
    "band": Z.band,
}
_cache = {}


def case(clib, name):
    """(image, text, reference stream, info) -- computed once, never changed"""
    if name not in _cache:
        img = IMAGES[name]()
        text = Z.zip_text(img)
        info = {}
        stream = Z.encode_c(clib, text, info)
        img.setflags(write=False)
        _cache[name] = (img, text, stream, info)
    return _cache[name]


def last_symbol(stream):
    return struct.unpack_from("<H", stream, len(stream) - 2)[0]


def ref_decode(clib, stream):
    return Z.codec_decode(lambda s, need: Z.decode_c(clib, s, need), stream)


# ---------------------------------------------------------------- the images are what they are meant to be
def test_images_land_where_intended(clib):
    for name in ("1x1", "3x2", "flat 256x192", "noise 256x192"):
        assert case(clib, name)[3]["fill_end"] is None, name                 # the fill phase alone
    img, text, stream, info = case(clib, "flat 256x192")
    assert info["longest"] > len(text) // 4 and len(stream) < 200            # entries as long as the stream
    img, text, stream, info = case(clib, "noise 256x192")
    assert 0 < Z.MAX_PAIRS - len(stream) // 4 < 2000                         # ends a little short of full
    img, text, stream, info = case(clib, "noise 320x200")
    assert info["fill_end"] is not None and info["fill_end"] < len(text) and info["longest"] < 256
    assert last_symbol(stream) == Z.EOF                                      # odd symbol count: the frozen phase appends 0xFFFF
    img, text, stream, info = case(clib, "photo-like 320x200")
    assert info["fill_end"] is not None and info["fill_end"] < len(text) and info["longest"] < 256
    assert last_symbol(stream) != Z.EOF                                      # even
    img, text, stream, info = case(clib, "photo-like 512x384")
    assert info["fill_end"] < 0.4 * len(text) and info["longest"] < 256     # most of the stream is frozen
    img, text, stream, info = case(clib, "band")
    tail = 8 + 11 * 216 * 320
    assert info["fill_end"] < tail < len(text) and 4096 < info["longest"] <= 32768   # the flat tail lies in the frozen phase; the chain's plain route


# ---------------------------------------------------------------- the coder on plain bytes
@pytest.mark.parametrize("data,symbols", Z.KNOWN_ANSWERS)
def test_raw_known_answers(ctx, data, symbols):
    rc, stream = ctx.zip_dict_encode(bytes(data))
    assert rc == 0 and stream == struct.pack("<%dH" % len(symbols), *symbols)
    rc, back = ctx.zip_dict_decode(stream)
    assert rc == 0 and back == bytes(data)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 100000])
def test_raw_random_bytes(ctx, clib, n):
    data = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8).tobytes()
    ref = Z.encode_c(clib, data)
    rc, stream = ctx.zip_dict_encode(data)
    assert rc == 0 and stream == ref
    rc, back = ctx.zip_dict_decode(ref)
    assert rc == 0 and back == data


@pytest.mark.parametrize("name", ["noise 320x200", "band"])
def test_raw_frozen_phase_device_buffers(ctx, clib, name):
    import torch
    from cniic_amd import _lib
    img, text, ref, info = case(clib, name)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    out = torch.empty(2 * len(text) + 4, dtype=torch.uint8, device="cuda")
    rc, ln = ctx.zip_dict_encode(t, out=out)
    assert rc == 0 and out[:ln].cpu().numpy().tobytes() == ref
    back = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    rc, ln2 = ctx.zip_dict_decode(out, n=ln, out=back)
    assert rc == 0 and ln2 == len(text) and back.cpu().numpy().tobytes() == text
    # a text that exceeds cap: CAPACITY, with the bytes needed
    small = torch.empty(len(text) - 1, dtype=torch.uint8, device="cuda")
    rc, need = ctx.zip_dict_decode(out, n=ln, out=small, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(text)
    rc, need = ctx.zip_dict_encode(t, out=small[:100], allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(ref)


@pytest.mark.parametrize("flat_bytes", [100000])
def test_raw_dictionary_full_but_not_handed_over(ctx, clib, flat_bytes):
    """The dictionary fills in the noise behind a stretch of equal bytes, but the coder stays on the host to the end of the text -- the
    same stream.  100 000 equal bytes: an entry of 32 768 bytes and more, which the match kernel is not given.  (The other reason to
    stay, a trie of more than 2^24 nodes, needs an entry of 2^24 bytes -- 2^25 equal bytes, five seconds of host walk -- and takes
    the same branch: it is left to a run by hand, flat_bytes = 34000000.)"""
    rng = np.random.default_rng(1)
    data = np.concatenate([np.full(flat_bytes, 7, np.uint8), rng.integers(0, 256, 1200000, dtype=np.uint8)])
    info = {}
    ref = Z.encode_c(clib, data, info)
    assert info["fill_end"] is not None and info["fill_end"] < data.size - 100000 and info["longest"] > 32768
    assert (info["nodes"] > (1 << 24)) == (flat_bytes > 1 << 25)
    rc, stream = ctx.zip_dict_encode(data)
    assert rc == 0 and stream == ref
    back = np.empty(data.size, np.uint8)
    rc, ln = ctx.zip_dict_decode(ref, out=back)
    assert rc == 0 and ln == data.size and np.array_equal(back, data)


def test_raw_claimed_size_is_summed_before_anything_is_allocated(ctx):
    from cniic_amd import _lib
    syms = [1, 1]
    for k in range(60):                       # every pair doubles the last entry: 2^61 bytes from 61 pairs
        syms += [0x100 + k, 0x100 + k]
    stream = struct.pack("<%dH" % len(syms), *syms)
    rc, need = ctx.zip_dict_decode(stream, out=np.empty(1 << 20, np.uint8), allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need >= 1 << 61


# ---------------------------------------------------------------- the codec
@pytest.mark.parametrize("name", list(IMAGES))
def test_codec_host_buffers(ctx, clib, name):
    img, text, ref, info = case(clib, name)
    rc, stream, _ = ctx.encode(EXPR, img)
    assert rc == 0 and stream == ref
    rc, back = ctx.decode(EXPR, ref)
    assert rc == 0 and np.array_equal(back, img)


@pytest.mark.parametrize("name", list(IMAGES))
def test_codec_device_buffers(ctx, clib, name):
    import torch
    img, text, ref, info = case(clib, name)
    h, w = img.shape[:2]
    d_img = torch.from_numpy(img.copy()).cuda()
    d_out = torch.empty(2 * len(text) + 4, dtype=torch.uint8, device="cuda")
    rc, ln, _ = ctx.encode(EXPR, d_img, w=w, h=h, out=d_out)
    assert rc == 0 and d_out[:ln].cpu().numpy().tobytes() == ref
    d_back = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    rc, cw, ch = ctx.decode_into(EXPR, d_out, ln, d_back)
    assert rc == 0 and (cw, ch) == (w, h) and np.array_equal(d_back.cpu().numpy().reshape(h, w, 3), img)


# ---------------------------------------------------------------- hostile streams: the restatement's verdict
def check_verdict(ctx, clib, stream, what):
    from cniic_amd import _lib
    want = ref_decode(clib, stream)
    rc, got = ctx.decode(EXPR, stream, allow=(_lib.DECODE,))
    if want is None:
        assert rc == _lib.DECODE, what
    else:
        assert rc == 0 and np.array_equal(got, want), what
    return want


def test_truncated(ctx, clib):
    img, text, ref, info = case(clib, "3x2")
    for n in range(0, min(64, len(ref)) + 1):
        check_verdict(ctx, clib, ref[:n], "3x2 cut to %d" % n)
    img, text, ref, info = case(clib, "noise 320x200")
    for n in range(0, 65):
        assert check_verdict(ctx, clib, ref[:n], "cut to %d" % n) is None
    for n in (FILL_BYTES - 4, FILL_BYTES, FILL_BYTES + 1, FILL_BYTES + 2, FILL_BYTES + 4, 300001, 300002, len(ref) - 4, len(ref) - 3, len(ref) - 2, len(ref) - 1):
        assert check_verdict(ctx, clib, ref[:n], "cut to %d" % n) is None
    # the last pair of this stream is (symbol, 0xFFFF): without the empty second symbol the first stands alone
    assert check_verdict(ctx, clib, ref, "whole") is not None


def test_symbol_not_handed_out(ctx, clib):
    img, text, ref, info = case(clib, "noise 320x200")
    for pair in (0, 5, 1000, Z.MAX_PAIRS - 1):                                # the fill phase: pair k may use symbols below 0x100 + k
        for second in (0, 1):
            bad = bytearray(ref)
            struct.pack_into("<H", bad, 4 * pair + 2 * second, 0x100 + pair)
            assert check_verdict(ctx, clib, bytes(bad), "pair %d" % pair) is None
    for pair in (Z.MAX_PAIRS, Z.MAX_PAIRS + 777):                             # the frozen phase: every symbol has been handed out; 0xFFFF is the
        for sym in (0xFFFE, 0xFFFF, 0x100):                                   # empty text -- the text changes, and the records behind it with it
            bad = bytearray(ref)
            struct.pack_into("<H", bad, 4 * pair, sym)
            check_verdict(ctx, clib, bytes(bad), "frozen pair %d <- %#x" % (pair, sym))


def test_empty_symbol_mid_stream(ctx, clib):
    img, text, ref, info = case(clib, "3x2")
    # every byte of the text as (byte, 0xFFFF): the entries these pairs make are never used
    stream = b"".join(struct.pack("<HH", b, Z.EOF) for b in text)
    want = check_verdict(ctx, clib, stream, "bytes paired with the empty text")
    assert want is not None and np.array_equal(want, img)
    stream = struct.pack("<HH", Z.EOF, Z.EOF) * 3 + b"".join(struct.pack("<HH", Z.EOF, b) for b in text)
    assert check_verdict(ctx, clib, stream, "empty pairs in front") is not None
    img, text, ref, info = case(clib, "noise 320x200")
    bad = bytearray(ref)
    struct.pack_into("<H", bad, 4 * 2000, Z.EOF)                              # a text goes missing: the stream now spells fewer bytes
    assert check_verdict(ctx, clib, bytes(bad), "0xFFFF in place of a symbol") is None


def test_record_length_not_three(ctx, clib):
    for name, px in (("3x2", 4), ("noise 320x200", 10), ("noise 320x200", 63000)):
        img, text, ref, info = case(clib, name)
        for byte, value in ((0, 4), (0, 2), (5, 1)):
            t = bytearray(text)
            t[8 + 11 * px + byte] = value
            assert check_verdict(ctx, clib, Z.encode_c(clib, bytes(t)), "%s pixel %d" % (name, px)) is None


def test_garbage_behind_the_last_needed_pair(ctx, clib):
    for name in ("3x2", "noise 256x192", "photo-like 320x200"):
        img, text, ref, info = case(clib, name)
        for tail in (b"\xfe", b"\xfe\xff", b"\xfe\xff\xfd\xff" * 5, bytes(range(256)) * 3):
            want = check_verdict(ctx, clib, ref + tail, "%s + %d bytes" % (name, len(tail)))
            assert want is not None and np.array_equal(want, img)


def test_capacity(ctx, clib):
    from cniic_amd import _lib
    img, text, ref, info = case(clib, "noise 320x200")
    out = np.zeros(img.size - 3, np.uint8)
    rc, w, h = ctx.decode_into(EXPR, np.frombuffer(ref, np.uint8), len(ref), out, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY
    small = np.zeros(1000, np.uint8)
    rc, ln, _ = ctx.encode(EXPR, img, out=small, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and ln == len(ref)


# ---------------------------------------------------------------- hilbert-zip
@pytest.mark.parametrize("name,make", [("64x64", lambda: Z.photo_like(64, 64)), ("100x37", lambda: Z.noise(100, 37)), ("band", Z.band)])
def test_hilbert_zip(ctx, clib, name, make):
    import cniic_amd
    import oracle_lib as O
    img = make()
    h, w = img.shape[:2]
    ref = Z.hilbert_encode(lambda t: Z.encode_c(clib, t), O.hilbert_linearize(img), w, h)
    codec = cniic_amd.HilbertZip(ctx)
    assert codec.encode(img) == ref
    back = codec.decode(ref)
    assert back is not None and np.array_equal(back, img)
    assert codec.decode(ref[:7]) is None
    if name == "100x37":   # the colours a short text does not reach stay zero; a malformed pair inside the needed part is an error
        dec = lambda s, need: Z.decode_c(clib, s, need)
        lin = Z.hilbert_decode_lin(dec, ref)
        assert lin is not None and np.array_equal(lin[2], O.hilbert_linearize(img).reshape(-1, 3))
        bad = bytearray(ref)
        struct.pack_into("<H", bad, 8 + 4 * 10, 0x100 + 10)
        assert codec.decode(bytes(bad)) is None and Z.hilbert_decode_lin(dec, bytes(bad)) is None
        t = bytearray(Z.records(O.hilbert_linearize(img)))
        t[11 * 1234] = 4                                                    # pixel 1234's record claims four bytes: the colours end there
        short_rec = struct.pack("<II", w, h) + Z.encode_c(clib, bytes(t))
        hostile = [ref[:8], ref[:8 + 4 * 100], ref[:8 + 4 * 100 + 1], ref[:8 + 4 * 100 + 2], ref[:8 + 4 * 100 + 3], ref[:len(ref) - 4], short_rec]
        zero_filled = 0
        for i, stream in enumerate(hostile):
            want = Z.hilbert_decode_lin(dec, stream)
            got = codec.decode(stream)
            if want is None:
                assert got is None, i
                continue
            assert got is not None and np.array_equal(O.hilbert_linearize(got).reshape(-1, 3), want[2]), i
            zero_filled += int(not want[2][-1].any() and want[2][0].any())
        assert zero_filled >= 4                                              # (the two cuts that leave a first symbol alone are errors)


# ---------------------------------------------------------------- batches
def test_batches_equal_single_calls(ctx, clib):
    names = ["3x2", "noise 320x200", "flat 256x192", "photo-like 320x200"]
    cases = [case(clib, n) for n in names]
    imgs = [c[0] for c in cases]
    refs = [c[2] for c in cases]
    buf = np.concatenate([im.reshape(-1) for im in imgs] + [np.zeros(1, np.uint8)])
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
    stride = (max(len(r) for r in refs) + 3) & ~3
    out = np.zeros(stride * len(imgs), np.uint8)
    rc, lens, rcs, _ = ctx.encode_batch_var(EXPR, buf, offs, ws, hs, out, stride)
    assert rc == 0 and rcs == [0] * len(imgs) and lens == [len(r) for r in refs]
    for f, r in enumerate(refs):
        assert out[f * stride:f * stride + lens[f]].tobytes() == r
    img_stride = max(im.size for im in imgs)
    back = np.zeros(img_stride * len(imgs), np.uint8)
    rc, dw, dh, drcs = ctx.decode_batch(EXPR, out, stride, lens, len(imgs), back, img_stride)
    assert rc == 0 and drcs == [0] * len(imgs) and dw == ws and dh == hs
    for f, im in enumerate(imgs):
        assert np.array_equal(back[f * img_stride:f * img_stride + im.size].reshape(im.shape), im)
    out2 = np.zeros_like(out)
    rc, rows, lens2 = ctx.measure_batch(EXPR, buf, offs, ws, hs, out=out2, stride=stride)
    assert rc == 0 and lens2 == lens and np.array_equal(out2, out)
    for f, row in enumerate(rows):
        assert row["rc"] == 0 and row["lossless_mismatch"] == 0 and row["error"] == 0.0 and row["compressed_size"] == len(refs[f])
        assert row["compression_ratio"] == len(refs[f]) / (ws[f] * hs[f] * 24.0) * 100.0
    # the Python codec object sizes its outputs from the dimensions inside the compressed text
    import cniic_amd
    codec = cniic_amd.AnyCodec.from_str(EXPR, ctx)
    assert codec.encode_batch(imgs) == refs
    for im, got in zip(imgs, codec.decode_batch(refs)):
        assert np.array_equal(got, im)
    assert codec.name() == "zip-dict" and codec.is_lossless()
