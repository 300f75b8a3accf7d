"""zip(back) on the GPU against the CPU restatement of the reference's look-back coder (tests/zip_back_ref.py / .c): byte-exact streams,
texts and images back, the reference's verdicts -- where it panics on encode (CNIIC_ERR_UNSUPPORTED), on hostile streams
(CNIIC_ERR_DECODE) -- on host and on device buffers.  The crafted texts are tests/zip_back_edges.py's; tests/test_zip_back_cpu.py holds
each of them to what it claims.  Every text is the smallest that reaches the code it names."""
import struct

import numpy as np
import pytest

import zip_back_edges as E
import zip_back_ref as Z

pytestmark = pytest.mark.gpu

SLICE = "CNIIC_TEST_ZB_SLICE"      # the testing build's knob: bytes a launch takes a stream forward


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_back_ref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


def L():
    from cniic_amd import _lib
    return _lib


_ref = {}


def ref(clib, key, make):
    """(text, reference stream or PANICS) of a named text -- computed once, never changed"""
    if key not in _ref:
        text = make()
        _ref[key] = (text, Z.encode_c(clib, text))
    return _ref[key]


def dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda() if len(data) else torch.zeros(1, dtype=torch.uint8, device="cuda")


def check_text(ctx, text, want, device_too=True):
    """encode and decode of a plain text on host buffers and on device buffers, against the reference's stream or its panic"""
    import torch
    _lib = L()
    rc, got = ctx.zip_back_encode(text, allow=(_lib.UNSUPPORTED,))
    if want == Z.PANICS:
        assert rc == _lib.UNSUPPORTED
        if device_too and len(text):
            out = torch.zeros(len(text) + len(text) // 4 + 16, dtype=torch.uint8, device="cuda")
            assert ctx.zip_back_encode(dev(text), n=len(text), out=out, allow=(_lib.UNSUPPORTED,))[0] == _lib.UNSUPPORTED
        return
    assert rc == _lib.OK and got == want
    rc, back = ctx.zip_back_decode(got, cap=len(text) + 64)
    assert rc == _lib.OK and back == bytes(text)
    if device_too and len(text):
        out = torch.zeros(len(text) + len(text) // 4 + 16, dtype=torch.uint8, device="cuda")
        rc, n = ctx.zip_back_encode(dev(text), n=len(text), out=out)
        assert rc == _lib.OK and out[:n].cpu().numpy().tobytes() == want
        txt = torch.zeros(len(text) + 1, dtype=torch.uint8, device="cuda")
        rc, m = ctx.zip_back_decode(out, n=n, out=txt)
        assert rc == _lib.OK and txt[:m].cpu().numpy().tobytes() == bytes(text)


# ---------------------------------------------------------------- the reference's known answers, window and distance edges, doubling
@pytest.mark.parametrize("i", range(len(Z.KNOWN_ANSWERS)))
def test_known_answers(ctx, i):
    text, stream = Z.KNOWN_ANSWERS[i]
    check_text(ctx, text, stream)


@pytest.mark.parametrize("name", sorted(E.SMALL))
def test_small_edges(ctx, clib, name):
    text, want = ref(clib, name, lambda: E.SMALL[name][0])
    assert E.symbols(want) == E.SMALL[name][1]
    check_text(ctx, text, want)


@pytest.mark.parametrize("distance", [65535, 65536])
def test_window_edge(ctx, clib, distance):
    text, want = ref(clib, ("window", distance), lambda: E.window_edge(distance))
    assert E.symbols(want)[-2] == {65535: ("L", 16, 65535), 65536: ("L", 8, 65496)}[distance]
    check_text(ctx, text, want)


# ---------------------------------------------------------------- the reference's limits
@pytest.mark.parametrize("length", [32767, 32768])
def test_longest_lookback(ctx, clib, length):
    text, want = ref(clib, ("long", length), lambda: E.long_match(length))
    assert (want == Z.PANICS) == (length == 32768)
    check_text(ctx, text, want)
    if want == Z.PANICS:
        with pytest.raises(Exception, match="back.rs:45"):
            ctx.zip_back_encode(text)


@pytest.mark.parametrize("n", [32767, 32768])
def test_longest_explicit(ctx, clib, n):
    text, want = ref(clib, ("explicit", n), lambda: E.rnd(n, 5))
    assert (want == Z.PANICS) == (n == 32768)
    check_text(ctx, text, want)
    if want == Z.PANICS:
        with pytest.raises(Exception, match="back.rs:45"):
            ctx.zip_back_encode(text)


# ---------------------------------------------------------------- the LDS ring, its refills, the slices
@pytest.mark.parametrize("rings", [1, 2, 3])
def test_ring_lengths(ctx, clib, rings):
    text, want = ref(clib, ("ring", rings), lambda: E.ring_text(rings))
    check_text(ctx, text, want, device_too=rings == 3)


def test_match_across_refills(ctx, clib):
    text, want = ref(clib, "mid", E.long_match_mid)
    assert ("L", 30000, 35900) in E.symbols(want)
    check_text(ctx, text, want)


@pytest.mark.parametrize("slice_bytes", [1000, 40000])
@pytest.mark.parametrize("which", ["mid", "long", "ring", "explicit"])
def test_slice_boundaries(ctx, clib, monkeypatch, which, slice_bytes):
    """a launch ends every slice_bytes: inside the 30 000-byte match and the literals around it, inside the longest look-back, inside
    an explicit run of 32 767 bytes (whose header is written 33 launches after its slot was left open), and all along a ring length"""
    text, want = {"mid": lambda: ref(clib, "mid", E.long_match_mid), "long": lambda: ref(clib, ("long", 32767), lambda: E.long_match(32767)),
                  "ring": lambda: ref(clib, ("ring", 1), lambda: E.ring_text(1)), "explicit": lambda: ref(clib, ("explicit", 32767), lambda: E.rnd(32767, 5))}[which]()
    monkeypatch.setenv(SLICE, str(slice_bytes))
    check_text(ctx, text, want, device_too=False)


def test_slices_are_launches(ctx, clib, monkeypatch):
    _lib = L()
    text, want = ref(clib, "mid", E.long_match_mid)
    monkeypatch.setenv(SLICE, "20000")
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, got = ctx.zip_back_encode(text)
        enc = ctx.kernel_time("zb_encode")[1]
        rc, back = ctx.zip_back_decode(got, cap=len(text))
        dec = ctx.kernel_time("zb_decode")[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert got == want and back == text
    # a launch ends a stream or takes it a slice further (the 30 000-byte match is one step: it may end far behind the slice's end)
    assert 3 <= enc <= len(text) // 20000 + 2 and 3 <= dec <= len(text) // 20000 + len(got) // 20000 + 2, (enc, dec)


# ---------------------------------------------------------------- decode: hostile and lazy
LIT = Z.explicit(b"abcdefgh")
HOSTILE = [
    ("back > produced", LIT + Z.lookback(4, 9)),
    ("back == produced", LIT + Z.lookback(4, 8)),
    ("back == 0", LIT + Z.lookback(4, 0) + LIT),
    ("len == 0", LIT + Z.lookback(0, 4) + LIT),
    ("empty explicit", LIT + Z.explicit(b"") + LIT),
    ("len > back", LIT + Z.lookback(7, 3) + Z.lookback(32767, 11)),
    ("truncated literal", LIT + b"\x04\x00abc"),
    ("one trailing byte", LIT + b"\x05"),
    ("header without back", LIT + b"\x04\x80\x03"),
    ("first symbol looks back", Z.lookback(1, 1)),
    ("a literal across stages", Z.explicit(E.rnd(20000, 3)) + Z.lookback(30000, 20000) + Z.explicit(E.rnd(17000, 4)) + Z.lookback(9, 57000)),
    ("back beyond the ring", Z.explicit(E.rnd(30000, 3)) * 3 + Z.lookback(5, 65535) + Z.lookback(100, 50)),
]


@pytest.mark.parametrize("what,stream", HOSTILE, ids=[h[0] for h in HOSTILE])
@pytest.mark.parametrize("slice_bytes", [None, 7000])
def test_hostile_streams(ctx, monkeypatch, what, stream, slice_bytes):
    import torch
    _lib = L()
    if slice_bytes:
        monkeypatch.setenv(SLICE, str(slice_bytes))
    try:
        want = Z.decode_py(stream)
    except Z.ZipError:
        want = None
    rc, got = ctx.zip_back_decode(stream, cap=1 << 20, allow=(_lib.DECODE,))
    out = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    rcd, n = ctx.zip_back_decode(dev(stream), n=len(stream), out=out, allow=(_lib.DECODE,))
    if want is None:
        assert rc == _lib.DECODE and rcd == _lib.DECODE
    else:
        assert rc == _lib.OK and got == want
        assert rcd == _lib.OK and out[:n].cpu().numpy().tobytes() == want


def raw(ctx, fn, data, n, out, cap):
    """a coder entry point with the caller's buffers as they are -> (rc, *len)"""
    _lib = L()
    ln = _lib.C.c_uint64(0)
    rc = getattr(ctx._L, fn)(ctx.h, _lib._ptr(data), _lib.C.c_uint64(n), _lib._ptr(out), _lib.C.c_uint64(cap), _lib.C.byref(ln))
    return rc, ln.value


def test_capacity_both_sides(ctx, clib):
    """cap too small: CNIIC_ERR_CAPACITY, the size needed, what fits written and nothing behind cap"""
    import torch
    _lib = L()
    text, want = ref(clib, "mid", E.long_match_mid)
    text_h, want_h = np.frombuffer(text, np.uint8), np.frombuffer(want, np.uint8)
    for fn, src, full in (("cniic_zip_back_encode", text_h, want), ("cniic_zip_back_decode", want_h, text)):
        for cap in (1, 7, len(full) - 1):
            out = np.full(cap + 8, 0xAB, np.uint8)
            assert raw(ctx, fn, src, src.size, out, cap) == (_lib.CAPACITY, len(full)) and (out[cap:] == 0xAB).all()
            outd = torch.full((cap + 8,), 0xAB, dtype=torch.uint8, device="cuda")
            assert raw(ctx, fn, dev(src.tobytes()), src.size, outd, cap) == (_lib.CAPACITY, len(full))
            got = outd.cpu().numpy()
            assert (got[cap:] == 0xAB).all() and got[:cap].tobytes() == full[:cap]
        outd = torch.full((8,), 0xAB, dtype=torch.uint8, device="cuda")
        assert raw(ctx, fn, src, src.size, outd, 0) == (_lib.CAPACITY, len(full)) and (outd.cpu().numpy() == 0xAB).all()


# ---------------------------------------------------------------- images
IMAGES = {
    "noise 64x48": lambda: Z.noise(64, 48), "photo-like 64x48": lambda: Z.photo_like(64, 48), "band 64x48": lambda: Z.band(64, 48),
    "noise 320x240": lambda: Z.noise(320, 240), "photo-like 320x240": lambda: Z.photo_like(320, 240), "band 320x240": lambda: Z.band(320, 240),
    "1x1": lambda: Z.noise(1, 1), "0x5": lambda: np.zeros((5, 0, 3), np.uint8), "5x0": lambda: np.zeros((0, 5, 3), np.uint8),
    "1x300": lambda: Z.photo_like(1, 300), "300x1": lambda: Z.photo_like(300, 1),
    "flat 16x16": lambda: Z.flat(16, 16), "flat 100x100": lambda: Z.flat(100, 100),
}
_img = {}


def image_case(clib, name):
    if name not in _img:
        img = IMAGES[name]()
        img.setflags(write=False)
        _img[name] = (img, Z.codec_encode(lambda d: Z.encode_c(clib, d), img))
    return _img[name]


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_images(ctx, clib, name):
    import torch
    import cniic_amd
    _lib = L()
    img, want = image_case(clib, name)
    h, w = img.shape[:2]
    codec = cniic_amd.ZipBack(ctx)
    if want == Z.PANICS:
        assert name in ("band 320x240", "flat 100x100")
        with pytest.raises(cniic_amd.CniicError, match="back.rs:45") as e:
            codec.encode(img)
        assert e.value.code == _lib.UNSUPPORTED
        return
    got = codec.encode(img)
    assert got == want
    assert _lib.zip_back_dims(got) == (w, h)
    back = codec.decode(got)
    assert back is not None and back.shape == img.shape and np.array_equal(back, img)
    if w * h:
        out = torch.zeros(len(want) + 8, dtype=torch.uint8, device="cuda")
        rc, n = ctx.zip_back_image_encode(dev(img.tobytes()), w=w, h=h, out=out)
        assert rc == _lib.OK and out[:n].cpu().numpy().tobytes() == want
        px = torch.zeros(img.size, dtype=torch.uint8, device="cuda")
        rc, dw, dh = ctx.zip_back_image_decode_into(out, n, px)
        assert (rc, dw, dh) == (_lib.OK, w, h) and px.cpu().numpy().tobytes() == img.tobytes()


def test_image_decode_is_lazy_and_strict(ctx, clib):
    import cniic_amd
    _lib = L()
    img, s = image_case(clib, "photo-like 64x48")
    codec = cniic_amd.ZipBack(ctx)
    # garbage behind the symbol that completes the last pixel is not looked at
    assert np.array_equal(codec.decode(s + Z.lookback(4, 65535) + b"\x09\x00ab"), img)
    text = Z.zip_text(img)
    more = Z.encode_c(clib, struct.pack("<II", 64, 49) + text[8:])       # claims a row more than it carries
    fewer = Z.encode_c(clib, struct.pack("<II", 64, 47) + text[8:])      # ... a row fewer: the rest is never pulled
    assert codec.decode(more) is None and Z.codec_decode(Z.decode_py, more) is None
    assert np.array_equal(codec.decode(fewer), img[:47])
    bad = bytearray(text)
    bad[8 + 11 * 100] = 4                                                  # pixel 100 is not a record of 3 bytes
    assert codec.decode(Z.encode_c(clib, bytes(bad))) is None
    assert codec.decode(s[:len(s) // 2]) is None and codec.decode(b"") is None and codec.decode(s[:5]) is None
    out = np.zeros(img.size - 1, np.uint8)                                 # room for one byte less than the image
    assert ctx.zip_back_image_decode_into(np.frombuffer(s, np.uint8), len(s), out, allow=(_lib.CAPACITY,))[0] == _lib.CAPACITY
    rc, n = ctx.zip_back_image_encode(img, out=np.zeros(len(s) - 1, np.uint8), allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and n == len(s)


# ---------------------------------------------------------------- batches
def batch_arrays(imgs, pad=0):
    offs, blob, at = [], [], 0
    for i, im in enumerate(imgs):
        at += (i * 5) % 3 if pad else 0     # any alignment
        offs.append(at)
        at += im.size
    buf = np.zeros(max(at, 1), np.uint8)
    for o, im in zip(offs, imgs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]


def mixed_images():
    rng = np.random.default_rng(9)
    imgs = []
    for i in range(40):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 70))
        imgs.append([Z.noise, Z.photo_like, Z.band][i % 3](w, h))
    imgs[3] = Z.noise(1, 1)
    imgs[7] = np.zeros((0, 9, 3), np.uint8)
    imgs[11] = Z.photo_like(1, 300)
    imgs[13] = Z.photo_like(300, 1)
    imgs[17] = Z.flat(100, 100)             # the reference panics on this one
    imgs[19] = Z.photo_like(200, 150)
    return imgs


@pytest.mark.parametrize("on_device", [False, True])
def test_batch_mixed(ctx, clib, on_device):
    import torch
    _lib = L()
    imgs = mixed_images()
    want = [Z.codec_encode(lambda d: Z.encode_c(clib, d), im) for im in imgs]
    buf, offs, ws, hs = batch_arrays(imgs, pad=1)
    stride = max(len(s) for s in want if s != Z.PANICS) + 3
    largest = 19
    out = torch.zeros(stride * len(imgs), dtype=torch.uint8, device="cuda") if on_device else np.zeros(stride * len(imgs), np.uint8)
    src = torch.from_numpy(buf).cuda() if on_device else buf
    rc, lens, rcs = ctx.zip_back_encode_batch_var(src, offs, ws, hs, out, stride, allow=(_lib.UNSUPPORTED,))
    assert rc == _lib.UNSUPPORTED
    got = out.cpu().numpy() if on_device else out
    for f, s in enumerate(want):
        if s == Z.PANICS:
            assert f == 17 and rcs[f] == _lib.UNSUPPORTED
            continue
        single_rc, single = ctx.zip_back_image_encode(imgs[f])
        assert rcs[f] == _lib.OK == single_rc and lens[f] == len(s) and got[f * stride:f * stride + lens[f]].tobytes() == s == single
    # a stride too small for one frame: that frame says what it needs, the others are as before
    tight = len(want[largest]) - 1
    assert sum(len(s) > tight for s in want if s != Z.PANICS) == 1
    out2 = np.zeros(tight * len(imgs), np.uint8)
    rc, lens2, rcs2 = ctx.zip_back_encode_batch_var(buf, offs, ws, hs, out2, tight, allow=(_lib.UNSUPPORTED, _lib.CAPACITY))
    assert rcs2[largest] == _lib.CAPACITY and lens2[largest] == len(want[largest])
    assert all(rcs2[f] == rcs[f] and lens2[f] == lens[f] and out2[f * tight:f * tight + lens2[f]].tobytes() == want[f] for f in range(len(imgs)) if f not in (largest, 17))
    # decode: frame 17's slot holds a malformed stream, the others come back; the MSEs are zero
    bad = LIT + Z.lookback(4, 9)
    got[17 * stride:17 * stride + len(bad)] = np.frombuffer(bad, np.uint8)
    lens[17] = len(bad)
    img_stride = max(im.size for im in imgs) + 1
    streams = torch.from_numpy(got).cuda() if on_device else got
    px = torch.zeros(img_stride * len(imgs), dtype=torch.uint8, device="cuda") if on_device else np.zeros(img_stride * len(imgs), np.uint8)
    rc, dw, dh, drcs = ctx.zip_back_decode_batch(streams, stride, lens, len(imgs), px, img_stride, allow=(_lib.DECODE,))
    assert rc == _lib.DECODE and drcs[17] == _lib.DECODE
    good = [f for f in range(len(imgs)) if f != 17]
    assert all(drcs[f] == _lib.OK and (dw[f], dh[f]) == (ws[f], hs[f]) for f in good)
    mse = ctx.mse_batch_var(src, [offs[f] for f in good], px, [f * img_stride for f in good], [ws[f] * hs[f] for f in good])
    assert mse == [0.0] * len(good)
    host = px.cpu().numpy() if on_device else px
    assert all(host[f * img_stride:f * img_stride + imgs[f].size].tobytes() == imgs[f].tobytes() for f in good)


def test_batch_more_frames_than_cus(ctx, clib):
    _lib = L()
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 4, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 3), dtype=np.uint8) for _ in range(300)]
    want = [Z.codec_encode(Z.encode_py, im) for im in imgs]
    buf, offs, ws, hs = batch_arrays(imgs)
    stride = max(len(s) for s in want)
    out = np.zeros(stride * 300, np.uint8)
    rc, lens, rcs = ctx.zip_back_encode_batch_var(buf, offs, ws, hs, out, stride)
    assert rc == _lib.OK and rcs == [0] * 300
    assert all(out[f * stride:f * stride + lens[f]].tobytes() == want[f] for f in range(300))
    img_stride = 8 * 8 * 3
    px = np.zeros(img_stride * 300, np.uint8)
    rc, dw, dh, drcs = ctx.zip_back_decode_batch(out, stride, lens, 300, px, img_stride)
    assert rc == _lib.OK and drcs == [0] * 300 and dw == ws and dh == hs
    assert all(px[f * img_stride:f * img_stride + imgs[f].size].tobytes() == imgs[f].tobytes() for f in range(300))


def test_batch_of_none(ctx):
    _lib = L()
    assert ctx.zip_back_encode_batch_var(np.zeros(1, np.uint8), [], [], [], np.zeros(1, np.uint8), 1)[0] == _lib.OK
    assert ctx.zip_back_decode_batch(np.zeros(1, np.uint8), 1, [], 0, np.zeros(1, np.uint8), 1)[0] == _lib.OK
    import cniic_amd
    assert cniic_amd.ZipBack(ctx).encode_batch([]) == [] and cniic_amd.ZipBack(ctx).decode_batch([]) == []


def test_class_batches(ctx, clib):
    import cniic_amd
    codec = cniic_amd.ZipBack(ctx)
    imgs = [Z.photo_like(40, 30), Z.flat(100, 100), Z.noise(3, 2)]
    streams = codec.encode_batch(imgs)
    assert streams[1] is None and streams[0] == Z.codec_encode(lambda d: Z.encode_c(clib, d), imgs[0])
    back = codec.decode_batch([streams[0], b"\x01", streams[2]])
    assert np.array_equal(back[0], imgs[0]) and back[1] is None and np.array_equal(back[2], imgs[2])
