"""hilbert(rle(d)) as a --codec= expression (src/codec/hilbertc.rs:341-397; f64::from_str for d, f64's Display in the name) without a
GPU: the library's parser, name and lossless flag against cniic_amd.codec.rust_f64_display and the literal names of
test_rle_approx_cpu.py's table, the spellings Rust's f64::from_str takes and refuses, cniic_codec_parse_f64 in header, exports and
SYMBOLS, and the Python classes."""
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (d, the name where test_rle_approx_cpu.py::test_name_and_lossless_flag states it literally, lossless)
TABLE = [
    (1.0, "hilbert-rle-approx_1", False), (16.0, "hilbert-rle-approx_16", False), (0.5, "hilbert-rle-approx_0.5", False),
    (1e-7, "hilbert-rle-approx_0.0000001", False), (1e21, "hilbert-rle-approx_1000000000000000000000", False),
    (math.inf, "hilbert-rle-approx_inf", False), (-math.inf, "hilbert-rle-approx_-inf", False), (math.nan, "hilbert-rle-approx_NaN", False),
    (-1.0, "hilbert-rle-approx_-1", False), (math.sqrt(2.0), "hilbert-rle-approx_1.4142135623730951", False),
    (441.7, "hilbert-rle-approx_441.7", False), (123456789.125, "hilbert-rle-approx_123456789.125", False),
    (0.0, "hilbert-rle", True), (-0.0, "hilbert-rle", True),
    (5e-324, None, False), (1.7976931348623157e308, None, False)]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("d,name,lossless", TABLE)
def test_name_lossless_and_value_of_the_expression(d, name, lossless):
    from cniic_amd import _lib
    from cniic_amd.codec import rust_f64_display
    expr = "hilbert(rle(%r))" % d
    want = "hilbert-rle" if d == 0.0 else "hilbert-rle-approx_" + rust_f64_display(d)
    assert name is None or name == want
    assert _lib.codec_name(expr) == want
    assert _lib.codec_is_lossless(expr) is lossless
    kind, arg, got = _lib.codec_parse_f64(expr)
    assert (kind, arg) == _lib.codec_parse("hilbert(rle)")
    assert _same(got, 0.0 if d == 0.0 else d)
    assert d == 0.0 or math.isnan(d) or math.copysign(1.0, got) == math.copysign(1.0, d)


def test_longest_name_needs_more_than_the_first_buffer():
    from cniic_amd import _lib
    name = _lib.codec_name("hilbert(rle(5e-324))")
    assert len(name) > 330 and name == "hilbert-rle-approx_0." + "0" * 323 + "5"
    big = _lib.codec_name("hilbert(rle(1.7976931348623157e308))")
    assert big == "hilbert-rle-approx_17976931348623157" + "0" * 292


def test_out_of_range_magnitudes():
    from cniic_amd import _lib
    assert _lib.codec_parse_f64("hilbert(rle(1e400))")[2] == math.inf
    assert _lib.codec_name("hilbert(rle(1e400))") == "hilbert-rle-approx_inf"
    assert _lib.codec_parse_f64("hilbert(rle(-1e400))")[2] == -math.inf
    for expr in ("hilbert(rle(1e-400))", "hilbert(rle(-1e-400))"):
        assert _lib.codec_parse_f64(expr)[2] == 0.0
        assert _lib.codec_name(expr) == "hilbert-rle" and _lib.codec_is_lossless(expr) is True
        assert _lib.codec_parse(expr) == _lib.codec_parse("hilbert(rle)")


@pytest.mark.parametrize("expr,d", [
    ("Hilbert(rle(4))", 4.0), ("hilbert(rle(+4))", 4.0), ("hilbert(rle(4.))", 4.0), ("hilbert(rle(.5))", 0.5), ("hilbert(rle(4e0))", 4.0),
    ("hilbert(rle(INF))", math.inf), ("hilbert(rle(-infinity))", -math.inf), ("hilbert(rle(nan))", math.nan), ("hilbert(rle(NaN))", math.nan),
    ("hilbert(rle(1E+2))", 100.0), ("hilbert(rle(25e-1))", 2.5), ("hilbert(rle(0004))", 4.0), ("hilbert(rle(-0))", 0.0)])
def test_accepted_spellings(expr, d):
    from cniic_amd import _lib
    from cniic_amd.codec import rust_f64_display
    got = _lib.codec_parse_f64(expr)
    assert got is not None and _same(got[2], d)
    assert _lib.codec_name(expr) == ("hilbert-rle" if d == 0.0 else "hilbert-rle-approx_" + rust_f64_display(d))


@pytest.mark.parametrize("expr", [
    "hilbert(rle())", "hilbert(rle(4,5))", "hilbert(rle(0x10))", "hilbert(rle(4f))", "hilbert(rle(nan(1)))", "hilbert(rle(.))",
    "hilbert(rle(e5))", "hilbert(rle(4))x", "HILBERT(rle(4))", "hilbert(zip)", "hilbert(rle( 4))", "hilbert(rle(4 ))", "hilbert(rle(4e))",
    "hilbert(rle(4e+))", "hilbert(rle(+))", "hilbert(rle(1_0))", "hilbert(rle(infinit))", "hilbert(rle(4)", "hilbert(RLE(4))"])
def test_rejected_spellings(expr):
    from cniic_amd import _lib
    assert _lib.codec_parse_f64(expr) is None
    assert _lib.codec_parse(expr) is None
    assert _lib.lib().cniic_codec_is_lossless(expr.encode()) == _lib.BAD_ARG
    with pytest.raises(_lib.CniicError):
        _lib.codec_name(expr)


def test_whatever_parsed_before_parses_as_before():
    from cniic_amd import _lib
    for expr, want in (("hufman", (1, 0)), ("HuFmAn", (1, 0)), ("cluster-colors(256)", (2, 256)), ("ccol(7)", (2, 7)), ("voronoi(2048)", (3, 2048)),
                       ("delta", (4, 0)), ("hilbert(rle)", (5, 0)), ("Hilbert(rle)", (5, 0)), ("hilbert(rle(0))", (5, 0)), ("hilbert(rle(0.0))", (5, 0)),
                       ("hilbert(rle(-0.0))", (5, 0)), ("hilbert(rle(0e7))", (5, 0))):
        assert _lib.codec_parse(expr) == want, expr
        assert _lib.codec_parse_f64(expr) == want + (0.0,), expr
    assert _lib.codec_name("hilbert(rle(0.0))") == "hilbert-rle" and _lib.codec_is_lossless("hilbert(rle(0))") is True


def test_u32_parse_still_refuses_a_nonzero_d():
    from cniic_amd import _lib
    assert _lib.codec_parse("hilbert(rle(0.5))") is None
    assert _lib.codec_parse("hilbert(rle(4))") is None and _lib.codec_parse("hilbert(rle(nan))") is None
    assert _lib.codec_parse_f64("hilbert(rle(0.5))") == (5, 0, 0.5)
    L = _lib.lib()
    assert L.cniic_codec_parse_f64(b"hilbert(rle(2))", None, None, None) == 0     # any out-parameter may be NULL
    assert L.cniic_codec_parse_f64(b"hilbert(zip)", None, None, None) == _lib.BAD_ARG


def test_symbol_declared_and_exported():
    from cniic_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cniic_hip.h")).read(), flags=re.S)
    assert re.search(r"int32_t\s+cniic_codec_parse_f64\s*\(\s*const\s+char\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", text)
    assert "cniic_codec_parse_f64" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "cniic_codec_parse_f64")
    header = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    assert "has its own entry point" not in header and "does not take `hilbert(rle(d))`" not in header


def test_python_classes():
    from cniic_amd import AnyCodec, HilbertRleApprox, _lib
    c = AnyCodec.from_str("hilbert(rle(2))")
    assert c.name() == "hilbert-rle-approx_2" and c.is_lossless() is False
    assert AnyCodec.from_str("hilbert(rle(0))").is_lossless() is True
    with pytest.raises(ValueError):
        AnyCodec.from_str("hilbert(rle(4f))")
    assert HilbertRleApprox(2.0).measure([]) == [] and HilbertRleApprox(2.0).encode_batch([]) == []
    for d, _, _ in TABLE:   # the expression the class builds reads back as exactly its d
        got = _lib.codec_parse_f64(HilbertRleApprox(d).expr)
        assert got is not None and _same(got[2], 0.0 if d == 0.0 else d), d
        assert _lib.codec_name(HilbertRleApprox(d).expr) == HilbertRleApprox(d).name()
