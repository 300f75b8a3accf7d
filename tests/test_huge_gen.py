"""tests/huge_gen.py's generators, numpy against torch: the oracle's digests (tests/golden/huge_digests.json) are made from the numpy
rows, tests/test_gpu_huge.py draws the same images with torch on the device.  Held to each other byte for byte on crops that reach
the images' last rows and columns, on the CPU and (-m gpu) on the device."""
import math

import numpy as np
import pytest

import huge_gen as G

SIDE = 46341
CROPS = [(0, 7), (1021, 1059), (SIDE - 40, SIDE)]


def _torch_rows(kind, y0, y1, device):
    import torch
    if kind == "fib":
        return G.fib_rows(torch, y0, y1, device=device).cpu().numpy()
    return G.tiles_rows(torch, SIDE, y0, y1, kind, device=device).cpu().numpy()


def _numpy_rows(kind, y0, y1):
    return G.fib_rows(np, y0, y1) if kind == "fib" else G.tiles_rows(np, SIDE, y0, y1, kind)


def _crops(kind):
    return [(G.FIB_H - 25, G.FIB_H), (0, 5), (31337, 31350)] if kind == "fib" else CROPS


@pytest.mark.parametrize("kind", ["tiles", "ripple", "bg", "fib"])
def test_numpy_and_torch_rows_agree_on_the_cpu(kind):
    for y0, y1 in _crops(kind):
        a = _numpy_rows(kind, y0, y1)
        assert a.dtype == np.uint8 and a.shape == (y1 - y0, G.FIB_W if kind == "fib" else SIDE, 3)
        assert np.array_equal(a, _torch_rows(kind, y0, y1, "cpu")), (kind, y0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tiles", "ripple", "bg", "fib"])
def test_numpy_and_torch_rows_agree_on_the_device(kind):
    for y0, y1 in _crops(kind):
        assert np.array_equal(_numpy_rows(kind, y0, y1), _torch_rows(kind, y0, y1, "cuda")), (kind, y0)


def test_what_the_images_are():
    f = G.fib_counts()
    assert len(f) == 45 and f[:4] == [1, 1, 2, 3] and sum(f) == G.FIB_W * G.FIB_H == 2971215072
    assert math.gcd(G.FIB_P, sum(f)) == 1                       # i -> i P mod N is a permutation: the counts are exact
    assert (G.FIB_W * G.FIB_H - 1) * G.FIB_P < (1 << 63)         # and its products fit int64
    assert len(set(G.fib_palette())) == 45
    a = G.tiles_rows(np, SIDE, 4096, 4096 + 256, "bg")
    bg = np.all(a == np.array(G.BG_RGB, np.uint8), axis=-1).mean()
    assert 0.45 < bg < 0.65                                      # about 55 % background
    r = G.tiles_rows(np, SIDE, 0, 64, "ripple").astype(np.int16) - G.tiles_rows(np, SIDE, 0, 64, "tiles").astype(np.int16)
    assert r.min() >= -2 and r.max() <= 2 and r.min() < 0 < r.max()
