"""zip(back) without a GPU: the two restatements of the look-back coder (tests/zip_back_ref.py, zip_back_ref.c) against the reference's
own known answers (back.rs:726-825) and against each other, the decoder's rules, and every crafted text of tests/test_zip_back.py held
to what it claims (tests/zip_back_edges.py)."""
import struct

import numpy as np
import pytest

import zip_back_edges as E
import zip_back_ref as Z


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zbref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


@pytest.mark.parametrize("text,stream", Z.KNOWN_ANSWERS)
def test_known_answers(clib, text, stream):
    assert Z.encode_py(text) == stream and Z.encode_c(clib, text) == stream
    assert Z.decode_py(stream) == text and Z.decode_c(clib, stream) == text


def test_python_equals_c_on_random_texts(clib):
    rng = np.random.default_rng(7)
    for i in range(80):
        n, k = int(rng.integers(0, 4000)), int(rng.integers(1, 6))
        text = rng.integers(0, k + 1, n, dtype=np.uint8).tobytes()    # few distinct bytes: repetitions at every distance
        a = Z.encode_py(text)
        assert a == Z.encode_c(clib, text), (i, n, k)
        if a != Z.PANICS:
            assert Z.decode_py(a) == text and Z.decode_c(clib, a) == text
            for need in (0, 1, n // 2, n):
                assert Z.decode_py(a, need) == Z.decode_c(clib, a, need)


@pytest.mark.parametrize("img", ["noise", "photo_like", "band"])
def test_python_equals_c_on_an_image(clib, img):
    im = getattr(Z, img)(64, 48)
    s = Z.codec_encode(Z.encode_py, im)
    assert s == Z.codec_encode(lambda d: Z.encode_c(clib, d), im) and s != Z.PANICS
    assert np.array_equal(Z.codec_decode(Z.decode_py, s), im)


# ---------------------------------------------------------------- the decoder's rules, one stream each
LIT = Z.explicit(b"abcdefgh")
DECODER_RULES = [
    ("one trailing byte ends the stream", LIT + b"\x05", b"abcdefgh"),
    ("a look-back header without its back ends the stream", LIT + b"\x04\x80", b"abcdefgh"),
    ("... with one byte of it", LIT + b"\x04\x80\x03", b"abcdefgh"),
    ("a truncated literal", LIT + b"\x04\x00abc", None),
    ("back > produced", LIT + Z.lookback(4, 9), None),
    ("back == produced", LIT + Z.lookback(4, 8), b"abcdefghabcd"),
    ("len > back copies back bytes", LIT + Z.lookback(7, 3), b"abcdefghfgh"),
    ("back == 0 brings no byte: the reader reports the end", LIT + Z.lookback(4, 0) + LIT, b"abcdefgh"),
    ("len == 0 brings no byte", LIT + Z.lookback(0, 4) + LIT, b"abcdefgh"),
    ("an empty explicit symbol brings no byte", LIT + Z.explicit(b"") + LIT, b"abcdefgh"),
    ("a first symbol that looks back", Z.lookback(1, 1), None),
]


@pytest.mark.parametrize("what,stream,text", DECODER_RULES, ids=[r[0] for r in DECODER_RULES])
def test_decoder_rules(clib, what, stream, text):
    for dec in (Z.decode_py, lambda s, need=None: Z.decode_c(clib, s, need)):
        if text is None:
            with pytest.raises(Z.ZipError):
                dec(stream)
        else:
            assert dec(stream) == text


def test_decoder_is_lazy(clib):
    bad = LIT + Z.lookback(4, 200)              # malformed behind the first symbol
    for dec in (Z.decode_py, lambda s, need=None: Z.decode_c(clib, s, need)):
        assert dec(bad, 8) == b"abcdefgh" and dec(bad, 3) == b"abcdefgh"    # whole symbols, nothing behind them
        with pytest.raises(Z.ZipError):
            dec(bad, 9)


# ---------------------------------------------------------------- the crafted texts stand where they claim
@pytest.mark.parametrize("name", sorted(E.SMALL))
def test_small_edge_texts(clib, name):
    text, claim = E.SMALL[name]
    for enc in (Z.encode_py, lambda d: Z.encode_c(clib, d)):
        s = enc(text)
        assert E.symbols(s) == claim
        assert Z.decode_py(s) == text


def test_probes_double():
    syms, probes = Z.parse_py(E.SMALL["unprobed_offset"][0])
    assert probes == E.UNPROBED_PROBES and syms == [("E", E.SMALL["unprobed_offset"][0])]


def test_window_edges(clib):
    s = E.symbols(Z.encode_c(clib, E.window_edge(65535)))
    assert s[-2:] == [("L", 16, 65535), ("E", 10)]
    s = E.symbols(Z.encode_c(clib, E.window_edge(65536)))
    # the marker at 0 is out of reach; the copy of its first 8 bytes that chunk 1 carries (at 40) is what is left
    assert s[-2:] == [("L", 8, 65496), ("E", 18)]


def test_reference_limits(clib):
    info = {}
    s = Z.encode_c(clib, E.long_match(32767), info)
    assert E.symbols(s)[-1] == ("L", 32767, 32784) and info["longest"] == 32767
    assert Z.encode_c(clib, E.long_match(32768)) == Z.PANICS
    assert Z.encode_c(clib, E.rnd(32767, 5)) == Z.explicit(E.rnd(32767, 5))
    assert Z.encode_c(clib, E.rnd(32768, 5)) == Z.PANICS
    assert Z.encode_py(E.rnd(32768, 5)) == Z.PANICS and Z.encode_py(b"\x07" * 70000) == Z.PANICS
    assert ("L", 30000, 35900) in E.symbols(Z.encode_c(clib, E.long_match_mid()))


@pytest.mark.parametrize("rings", [1, 2, 3])
def test_ring_texts(clib, rings):
    text, info = E.ring_text(rings), {}
    s = Z.encode_c(clib, text, info)
    assert s != Z.PANICS and len(text) > rings * E.RING and Z.decode_c(clib, s) == text
    assert info["explicit"] == 64 and info["farthest"] == (E.FAR * E.CHUNK + 16 if rings * E.RING > E.FAR * E.CHUNK else 40)


def test_images_of_the_gpu_tests(clib):
    enc = lambda d: Z.encode_c(clib, d)                                     # noqa: E731
    assert Z.codec_encode(enc, Z.flat(16, 16)) != Z.PANICS
    assert Z.codec_encode(enc, Z.flat(100, 100)) == Z.PANICS               # a look-back of 32 768 bytes: 2979 pixels
    assert Z.codec_encode(enc, Z.band(320, 240)) == Z.PANICS               # (its flat rows)
    for img in (Z.noise(320, 240), Z.photo_like(320, 240), Z.band(64, 48)):
        assert Z.codec_encode(enc, img) != Z.PANICS


# ---------------------------------------------------------------- the library's host side
def test_class_and_dims():
    import cniic_amd
    from cniic_amd import _lib
    c = cniic_amd.ZipBack()
    assert c.name() == "zip-back" and c.is_lossless()
    s = Z.codec_encode(Z.encode_py, Z.noise(7, 5))
    assert _lib.zip_back_dims(s) == (7, 5)
    assert _lib.zip_back_dims(s[:9]) is None and _lib.zip_back_dims(b"") is None
    assert _lib.zip_back_dims(Z.explicit(struct.pack("<I", 300)) + Z.lookback(4, 4) + b"junk") == (300, 300)
    assert _lib.zip_back_dims(Z.explicit(b"abc") + Z.lookback(9, 4)) is None          # back > produced
    assert _lib.zip_back_dims(Z.explicit(b"abcd") + Z.lookback(4, 0) + LIT) is None    # the reader ends at a symbol without bytes
    assert _lib.zip_back_dims(b"\x09\x00abcdefgh") is None                             # a literal cut short
    assert _lib.codec_parse("zip(back)") is None                                       # still no expression
