"""Pure-numpy restatement of the reference's three linearisations (src/hilbert.rs:10-32) and of the difference distribution its
experiment script computes (scripts/experiments/hilbert_distribution.py), built on the oracle's scan (orc_hilbert_iter) for the
a x b scans.  What tests/test_linearize_methods*.py compare the library with."""
import numpy as np

import oracle_lib as O

METHODS = ("rect", "small", "large")


def npot(v):
    """u32::next_power_of_two (npot(0) = 1)"""
    p = 1
    while p < v:
        p <<= 1
    return p


def small_side(w, h):
    return min(npot(w) >> 1, npot(h) >> 1)              # hilbert.rs:18


def large_side(w, h):
    return max(npot(w), npot(h))                        # hilbert.rs:27


def count(method, w, h):
    if method == "small":
        return small_side(w, h) ** 2
    assert method in ("rect", "large")
    return w * h


def oracle_scan(a, b):
    """hilbert::iter(a, b) (hilbert.rs:40-43) as the oracle walks it: (a b, 2) positions (x, y)"""
    if a * b == 0:
        return np.zeros((0, 2), np.uint32)
    return O.hilbert_iter(a, b)


def positions(method, w, h, scan=oracle_scan):
    """the (x, y) the method visits, in its order; scan(a, b): the scan of a x b"""
    if method == "rect":
        return scan(w, h)
    if method == "small":
        s = small_side(w, h)
        return scan(s, s)
    assert method == "large"
    S = large_side(w, h)
    xy = scan(S, S)
    return xy[(xy[:, 0] < w) & (xy[:, 1] < h)]          # hilbert.rs:30


def linearize(img, method, scan=oracle_scan):
    h, w = img.shape[:2]
    xy = positions(method, w, h, scan)
    return np.ascontiguousarray(img[xy[:, 1], xy[:, 0]]).reshape(-1, 3)


def classic_xy2d(order, x, y):
    """position of (x, y) on the classic Hilbert curve of the 2^order square (the textbook xy2d, vectorised): what the oracle's scan
    of a 2^n square is (checked in test_linearize_methods_cpu.py).  For squares whose positions cannot be listed."""
    n = 1 << order
    x = np.asarray(x, np.int64).copy()
    y = np.asarray(y, np.int64).copy()
    d = np.zeros(x.shape, np.int64)
    s = n >> 1
    while s > 0:
        rx = ((x & s) > 0).astype(np.int64)
        ry = ((y & s) > 0).astype(np.int64)
        d += s * s * ((3 * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x = np.where(flip, n - 1 - x, x)
        y = np.where(flip, n - 1 - y, y)
        swap = ry == 0
        x, y = np.where(swap, y, x), np.where(swap, x, y)
        s >>= 1
    return d


def large_by_position(img):
    """`large` without listing the square: the image's pixels sorted by their position on the square's curve"""
    h, w = img.shape[:2]
    order = large_side(w, h).bit_length() - 1
    ys, xs = np.divmod(np.arange(w * h, dtype=np.int64), w)
    d = classic_xy2d(order, xs, ys)
    return np.ascontiguousarray(img.reshape(-1, 3)[np.argsort(d, kind="stable")])


def channel_diff_hist(lin):
    """counts[c][v + 255] = #{i in 1..n-1: lin[i][c] - lin[i-1][c] == v} (pandas.diff drops the first element) -> int64 [3, 511]"""
    lin = np.asarray(lin, np.uint8).reshape(-1, 3)
    out = np.zeros((3, 511), np.int64)
    if lin.shape[0] > 1:
        dd = np.diff(lin.astype(np.int64), axis=0) + 255
        for c in range(3):
            out[c] = np.bincount(dd[:, c], minlength=511)
    return out
