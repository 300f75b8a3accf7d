"""hilbert(rle(d)) with d != 0 (src/codec/hilbertc.rs:26-45, rle_approx :200-299) without a GPU: the two CPU restatements the GPU
tests compare against agree with each other and, at d == 0, with the oracle's `hilbert(rle)`; the codec's name and lossless flag
are the reference's; the library declares and exports the new encode entry point."""
import math
import os

import numpy as np
import pytest

import oracle_lib as O
import rle_approx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = R.compile_c(tmp_path_factory.mktemp("rla"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


def _images(w, h, seed):
    from cniic_amd import synth
    return {"photo": synth.photo(w, h, synth.SEED0 + seed), "flat": R.flat(w, h), "ramp": R.ramp(w, h), "checker": R.checker(w, h),
            "noise": R.noise(w, h, seed), "distinct": R.distinct(w, h)}


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (37, 29), (64, 64), (96, 40)])
def test_python_and_c_restatements_agree(clib, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    ds = R.D_VALUES + [0.0, -0.0] + list(rng.uniform(0.0, 60.0, 4))
    for name, img in _images(w, h, w + h).items():
        lin = O.hilbert_linearize(img)
        for d in ds:
            py = R.encode_py(lin, w, h, d)
            assert py == R.encode_c(clib, lin, w, h, d), (name, d)
            assert len(py) >= 8 and (len(py) - 8) % 12 == 0
            counts = py[8::12]
            assert sum(counts) == w * h and all(0 < c <= 255 for c in counts), (name, d)


@pytest.mark.parametrize("w,h", [(1, 1), (300, 1), (37, 29), (64, 64)])
def test_zero_is_the_oracles_exact_stream(clib, w, h):
    for name, img in _images(w, h, 3 * w + h).items():
        rc, exp, _ = O.encode("hilbert(rle)", img)
        assert rc == 0
        lin = O.hilbert_linearize(img)
        for d in (0.0, -0.0):
            assert R.encode_py(lin, w, h, d) == exp, name
            assert R.encode_c(clib, lin, w, h, d) == exp, name


def test_edge_values_of_d():
    img = R.noise(23, 17)
    lin = O.hilbert_linearize(img)
    n = 23 * 17
    for d in (-1.0, math.nan, -1e-300):   # nothing is accepted, not even an equal colour
        assert R.encode_py(lin, 23, 17, d)[8::12] == bytes([1] * n)
    flat = R.flat(40, 30)
    lf = O.hilbert_linearize(flat)
    assert R.encode_py(lf, 40, 30, -1.0)[8::12] == bytes([1] * 1200)
    for d in (math.inf, math.sqrt(3.0) * 255.0, 1e300):   # everything is: runs of 255
        assert R.encode_py(lin, 23, 17, d)[8::12] == bytes([255] * (n // 255) + [n % 255])


def test_round_half_away_from_zero():
    # two pixels (0, 1, 3) and (1, 2, 4): averages 0.5, 1.5, 3.5 -> 1, 2, 4 (Python's round() would give 0, 2, 4)
    lin = np.array([[0, 1, 3], [1, 2, 4]], np.uint8)
    data = R.encode_py(lin, 2, 1, 2.0)
    assert data[8] == 2 and tuple(data[17:20]) == (1, 2, 4)


@pytest.mark.parametrize("d,name,lossless", [
    (1.0, "hilbert-rle-approx_1", False), (16.0, "hilbert-rle-approx_16", False), (0.5, "hilbert-rle-approx_0.5", False),
    (1e-7, "hilbert-rle-approx_0.0000001", False), (1e21, "hilbert-rle-approx_1000000000000000000000", False),
    (math.inf, "hilbert-rle-approx_inf", False), (-math.inf, "hilbert-rle-approx_-inf", False), (math.nan, "hilbert-rle-approx_NaN", False),
    (-1.0, "hilbert-rle-approx_-1", False), (math.sqrt(2.0), "hilbert-rle-approx_1.4142135623730951", False),
    (441.7, "hilbert-rle-approx_441.7", False), (123456789.125, "hilbert-rle-approx_123456789.125", False),
    (0.0, "hilbert-rle", True), (-0.0, "hilbert-rle", True)])
def test_name_and_lossless_flag(d, name, lossless):
    from cniic_amd import HilbertRleApprox
    c = HilbertRleApprox(d)
    assert c.name() == name
    assert c.is_lossless() is lossless


def test_symbol_declared_and_exported():
    import re
    from cniic_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cniic_hip.h")).read(), flags=re.S)
    assert re.search(r"int32_t\s+cniic_hilbert_rle_approx_encode\s*\(\s*cniic_ctx\s*\*\s*\w+\s*,\s*double\s", text)
    assert "cniic_hilbert_rle_approx_encode" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "cniic_hilbert_rle_approx_encode")
    assert hasattr(_lib.Context, "hilbert_rle_approx_encode")


def test_parse_still_rejects_the_expression():
    from cniic_amd import _lib
    assert _lib.codec_parse("hilbert(rle(0.5))") is None
    assert _lib.codec_parse("hilbert(rle)") is not None
