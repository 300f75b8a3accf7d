"""zip(dict) without a GPU: the restatements the GPU tests compare against (tests/zip_dict_ref.py, tests/zip_dict_ref.c) reproduce the
reference's known answers (the tests of src/zip/dict.rs) and agree with each other; the codec surface parses `zip(dict)` and nothing
near it; cniic_zip_dict_dims reads the dimensions out of the compressed text."""
import struct

import numpy as np
import pytest

import zip_dict_ref as Z


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_dict_ref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


@pytest.mark.parametrize("data,symbols", Z.KNOWN_ANSWERS)
def test_known_answers(clib, data, symbols):
    data = bytes(data)
    assert Z.encode_symbols(data) == symbols
    stream = struct.pack("<%dH" % len(symbols), *symbols)
    assert Z.encode_py(data) == stream and Z.encode_c(clib, data) == stream
    assert Z.decode_py(stream) == data and Z.decode_c(clib, stream) == data


# the eight images of the GPU tests (tests/test_zip_dict.py): for every one of them the C restatement, which those tests compare the
# library with, is held against the Python one -- dictionaries of tuples, nothing shared with the C code or the library's
IMAGES = [("1x1", lambda: Z.noise(1, 1)), ("3x2", lambda: Z.noise(3, 2)), ("flat 256x192", lambda: Z.flat(256, 192)),
          ("noise 256x192", lambda: Z.noise(256, 192)), ("noise 320x200", lambda: Z.noise(320, 200)),
          ("photo-like 320x200", lambda: Z.photo_like(320, 200)), ("photo-like 512x384", lambda: Z.photo_like(512, 384)), ("band", Z.band)]


@pytest.mark.parametrize("name,make", IMAGES, ids=[n for n, _ in IMAGES])
def test_python_and_c_agree(clib, name, make):
    img = make()
    text = Z.zip_text(img)
    ip, ic = {}, {}
    stream = Z.encode_py(text, ip)
    assert Z.encode_c(clib, text, ic) == stream
    assert ip == ic
    assert Z.decode_c(clib, stream) == text
    assert Z.decode_py(stream) == text                       # (five of the eight streams go on behind the pair that fills the dictionary)
    if ip["fill_end"] is not None:
        assert len(stream) > 4 * Z.MAX_PAIRS
        need = 8 + 11 * img.shape[0] * img.shape[1]
        assert Z.decode_py(stream + b"\xee\xee\xee\xee", need) == text   # the lazy reader stops at the pair that completes the image
    back = Z.codec_decode(lambda s, need: Z.decode_c(clib, s, need), stream)
    assert back is not None and np.array_equal(back, img)


def test_restatement_failures(clib):
    good = Z.encode_py(b"abcabcabcabc")
    for dec in (Z.decode_py, lambda s, need=None: Z.decode_c(clib, s, need)):
        assert dec(good + b"\x07") == b"abcabcabcabc"                   # a single byte behind the last pair ends the stream
        with pytest.raises(Z.ZipError):
            dec(good + b"\x07\x00")                                       # a first symbol without a second
        with pytest.raises(Z.ZipError):
            dec(struct.pack("<4H", 1, 2, 0x101, 3))                       # 0x101 is handed out by the second pair, not before it
        assert dec(struct.pack("<4H", 1, 2, 0x100, 0xFFFF)) == bytes([1, 2, 1, 2])
        assert dec(struct.pack("<4H", 0xFFFF, 1, 0xFFFF, 0xFFFF)) == bytes([1])
        assert dec(good, 3) == b"abcab"                                 # lazy: whole pairs while fewer than 3 bytes are there
        assert dec(good[:8] + b"\xee\xee\xee\xee", 3) == b"abcab"       # ... and what lies behind them is not looked at


def test_parse_name_lossless():
    from cniic_amd import _lib
    p = _lib.codec_parse("zip(dict)")
    assert p is not None and p[0] == _lib.KIND_ZIP_DICT
    assert _lib.codec_parse_f64("zip(dict)") == (_lib.KIND_ZIP_DICT, 0, 0.0)
    assert _lib.codec_name("zip(dict)") == "zip-dict"
    assert _lib.codec_is_lossless("zip(dict)") is True


@pytest.mark.parametrize("expr", ["zip(back)", "zip", "zip()", "Zip(dict)", "zip(dict,dict)", "zip(dict)x", "zip-dict", "hilbert(zip)", " zip(dict)",
                                  "zip(dict) ", "zip( dict)"])
def test_still_malformed(expr):
    from cniic_amd import _lib
    assert _lib.codec_parse(expr) is None and _lib.codec_parse_f64(expr) is None
    with pytest.raises(_lib.CniicError):
        _lib.codec_name(expr)


def test_hilbert_zip_class_surface():
    import cniic_amd
    c = cniic_amd.HilbertZip()
    assert c.name() == "hilbert-zip" and c.is_lossless() is True


def test_dims(clib):
    from cniic_amd import _lib
    for w, h in ((1, 1), (3, 2), (320, 200), (0, 7), (70000, 3)):
        text = struct.pack("<II", w, h) + Z.records(np.zeros((min(w * h, 64), 3), np.uint8))
        stream = Z.encode_c(clib, text)
        assert _lib.zip_dict_dims(stream) == (w, h)
        assert _lib.stream_dims("zip(dict)", stream) == (w, h)
    stream = Z.encode_c(clib, Z.zip_text(Z.noise(3, 2)))
    assert _lib.zip_dict_dims(stream + b"\xff\xfe\xfd") == (3, 2)
    # streams that spell fewer than 8 bytes, or break before they have
    for k in range(8):
        assert _lib.zip_dict_dims(Z.encode_py(bytes(range(k)))) is None
    assert _lib.zip_dict_dims(b"") is None
    assert _lib.zip_dict_dims(struct.pack("<4H", 1, 2, 0x101, 3) + Z.encode_py(bytes(8))) is None      # a symbol not handed out yet
    # 0xFFFF is the empty text anywhere: three empty pairs, then eight single bytes
    s = struct.pack("<6H", *([0xFFFF] * 6)) + struct.pack("<8H", 5, 0, 0, 0, 6, 0, 0, 0)
    assert _lib.zip_dict_dims(s) == (5, 6)
    # eight bytes out of entries: (1, 2) makes 0x100 = [1 2]; (0x100, 0x100) makes 0x101 = [1 2 1 2]; 0x101 0xFFFF
    s = struct.pack("<6H", 1, 2, 0x100, 0x100, 0x101, 0xFFFF)
    assert Z.decode_py(s) == bytes([1, 2, 1, 2, 1, 2, 1, 2, 1, 2])
    assert _lib.zip_dict_dims(s) == struct.unpack("<II", bytes([1, 2, 1, 2, 1, 2, 1, 2]))
