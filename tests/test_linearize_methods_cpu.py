"""cniic_hilbert_linearize_count (host only, no context) against the restatement of src/hilbert.rs:10-32 in linearize_ref.py, and the
restatement itself against answers spelled out here.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import linearize_ref as R
import oracle_lib as O

SMALL_SIDE = {0: 0, 1: 0, 2: 1, 3: 2, 4: 2, 5: 4, 8: 4, 9: 8}      # min(npot(w) >> 1, ...) for one dimension (hilbert.rs:18)


def lib_count(method, w, h):
    from cniic_amd import _lib
    n = C.c_uint64(0xDEAD)
    rc = _lib.lib().cniic_hilbert_linearize_count(C.c_int32(method), C.c_uint32(w), C.c_uint32(h), C.byref(n))
    return rc, n.value


def test_small_side_known_answers():
    from cniic_amd import _lib
    for w, sw in SMALL_SIDE.items():
        assert R.small_side(w, 1 << 20) == sw
        for h, sh in SMALL_SIDE.items():
            s = min(sw, sh)                                      # the side is the min over both dimensions
            assert R.small_side(w, h) == s
            assert lib_count(_lib.LIN_SMALL, w, h) == (0, s * s), (w, h)
            assert _lib.linearize_count("small", w, h) == R.count("small", w, h)


@pytest.mark.parametrize("w,h", [(0, 0), (0, 7), (1, 1), (5, 3), (64, 129), (1000, 600), (1, 65536), (65535, 65535), ((1 << 30) - 1, 3)])
def test_count_against_the_restatement(w, h):
    from cniic_amd import _lib
    assert lib_count(_lib.LIN_RECT, w, h) == (0, w * h)
    assert lib_count(_lib.LIN_LARGE, w, h) == (0, w * h)
    for m in R.METHODS:
        assert _lib.linearize_count(m, w, h) == R.count(m, w, h)


def test_count_refuses_unknown_methods_and_oversized_images():
    from cniic_amd import _lib
    for m in (-1, 3, 99):
        assert lib_count(m, 4, 4)[0] == _lib.BAD_ARG
    for m in (_lib.LIN_RECT, _lib.LIN_SMALL, _lib.LIN_LARGE):
        assert lib_count(m, 1 << 30, 1)[0] == _lib.BAD_ARG
        assert lib_count(m, 1, 1 << 30)[0] == _lib.BAD_ARG
        assert lib_count(m, 1 << 16, 1 << 16)[0] == _lib.BAD_ARG   # w h = 2^32
        assert lib_count(m, (1 << 30) - 1, 4)[0] == 0
    from cniic_amd import CniicError
    with pytest.raises(CniicError):
        _lib.linearize_count("large", 1 << 30, 1)


def _img(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_restatement_small_on_4x4_is_the_2x2_scan_of_the_top_left_square():
    img = _img(4, 4)
    scan22 = [(0, 0), (0, 1), (1, 1), (1, 0)]                       # (x, y): the oracle's 2 x 2 scan
    assert O.hilbert_iter(2, 2).tolist() == [list(p) for p in scan22]
    assert np.array_equal(R.linearize(img, "small"), np.array([img[y, x] for x, y in scan22]))


@pytest.mark.parametrize("n", [4, 8])
def test_restatement_large_equals_rect_on_power_of_two_squares(n):
    img = _img(n, n, n)
    assert np.array_equal(R.linearize(img, "large"), R.linearize(img, "rect"))
    assert np.array_equal(R.linearize(img, "rect"), O.hilbert_linearize(img).reshape(-1, 3))


def test_restatement_large_on_5x3():
    img = _img(5, 3, 53)
    lin = R.linearize(img, "large")
    # a permutation of the image's pixels
    assert lin.shape == (15, 3)
    key = lambda a: np.sort(a.reshape(-1, 3).astype(np.int64) @ np.array([65536, 256, 1]))
    assert np.array_equal(key(lin), key(img))
    # the 8 x 8 scan filtered: the oracle's orc_hilbert_iter(8, 8), the positions with x < 5 and y < 3 in its order
    kept = [(0, 0), (0, 1), (1, 1), (1, 0), (2, 0), (3, 0), (3, 1), (2, 1), (2, 2), (3, 2), (1, 2), (0, 2), (4, 2), (4, 1), (4, 0)]
    assert R.positions("large", 5, 3).tolist() == [list(p) for p in kept]
    assert np.array_equal(lin, np.array([img[y, x] for x, y in kept]))


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (8, 8), (37, 20), (64, 64), (65, 64), (1, 300)])
def test_restatement_by_position_equals_the_filtered_scan(w, h):
    """classic_xy2d (used where the square's positions cannot be listed) is the oracle's scan of a 2^n square"""
    img = _img(w, h, w * h)
    assert np.array_equal(R.large_by_position(img), R.linearize(img, "large"))


def test_restatement_diff_hist():
    lin = np.array([[10, 0, 255], [12, 0, 0], [12, 0, 255]], np.uint8)
    c = R.channel_diff_hist(lin)
    assert c.sum(axis=1).tolist() == [2, 2, 2]
    assert c[0, 255 + 2] == 1 and c[0, 255] == 1 and c[1, 255] == 2 and c[2, 0] == 1 and c[2, 510] == 1
    assert R.channel_diff_hist(lin[:1]).sum() == 0 and R.channel_diff_hist(lin[:0]).sum() == 0
