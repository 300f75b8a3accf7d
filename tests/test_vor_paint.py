"""The voronoi repaint of the single decode (k_voronoi_paint_tiles and k_voronoi_paint, cniic_amd/csrc/k_misc.hip, with the arithmetic of
vor_paint.hpp and the gate of codec.cpp) at its pruning, list and coordinate limits.  Every decode is compared byte for byte with the
oracle's decode and with the numpy brute force of tests/vor_paint_ref.py; there are no tolerances.  Every case also asserts the stage marks
"vor_paint_tiles", "vor_paint_brute" and "vor_paint_overflow" (the tiles whose kept list outgrew the LDS list) against the numpy model of
the prune, so a case cannot pass on the wrong kernel or the wrong path.  tests/test_vor_paint_cpu.py checks without a GPU that every case
has the property it is named for: the corner ties are the cases in which a keep predicate `f > 0` paints exactly one wrong pixel, the
256-entry lists the ones in which a cap test `n < cap` moves the overflow mark from 0 to 1 with every pixel still right."""
import numpy as np
import pytest

import oracle_lib as O
import vor_paint_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


def _marks(ctx):
    return tuple(int(ctx.kernel_time(n)[1]) for n in R.MARKS)


def _decode(ctx, c):
    """the decode of a case with the stage timers on -> (image, (tiles, brute, overflow))"""
    from cniic_amd import _lib
    data = R.case_stream(c)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, got = ctx.decode("voronoi(%d)" % len(c["xs"]), data)
        marks = _marks(ctx)
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert rc == 0 and got.shape == (c["h"], c["w"], 3), c["name"]
    return got, marks


def _check(ctx, c, oracle=True):
    got, marks = _decode(ctx, c)
    want = R.brute_labels(c["w"], c["h"], c["xs"], c["ys"])
    wrong = np.argwhere((got != R.image_of(want)).any(axis=2))
    assert len(wrong) == 0, (c["name"], len(wrong), wrong[:4].tolist())
    if oracle:
        rco, exp = O.decode("voronoi(%d)" % len(c["xs"]), R.case_stream(c))
        assert rco == 0 and np.array_equal(got, exp), c["name"]
    assert marks == R.expected_marks(c), (c["name"], marks)
    assert (marks[0], marks[1]) == ((1, 0) if c["route"] == "tiles" else (0, 1)), c["name"]
    if "overflow" in c:
        assert marks[2] == c["overflow"], c["name"]
    return got, want, marks


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.mark.parametrize("c", R.corner_ties(), ids=_ids(R.corner_ties()))
def test_corner_ties(ctx, c):
    """a centroid that ties the pivot at one corner pixel of a tile and loses everywhere else in it: f = 0 keeps it"""
    got, want, marks = _check(ctx, c)
    x, y, win, lose = c["tie"]
    assert tuple(got[y, x]) == R.colour(win) and marks == (1, 0, 0)


@pytest.mark.parametrize("c", R.list_cap(), ids=_ids(R.list_cap()))
def test_list_cap(ctx, c):
    """255, 256 and 257 kept entries: the last slot of the LDS list, and the first tile that goes to brute force"""
    _check(ctx, c)


@pytest.mark.parametrize("c", R.k_limits(), ids=_ids(R.k_limits()))
def test_k_limits(ctx, c):
    """K = 1; 255 .. 257 (one id a thread, then two); 4096 (16 ids a thread, 12 id bits) and 4097 (the brute-force kernel)"""
    got, want, marks = _check(ctx, c)
    K = len(c["xs"])
    if K >= 4096:
        assert tuple(got[15, 31]) == R.colour(K - 1)


@pytest.mark.parametrize("c", R.coordinate_switch(), ids=_ids(R.coordinate_switch()))
def test_coordinate_switch(ctx, c):
    """coordinates of 16383 and sides of 16384 on the tiled kernel, 16384 and 16385 on the brute-force one"""
    _check(ctx, c)


@pytest.mark.parametrize("c", R.clipped_tiles(), ids=_ids(R.clipped_tiles()))
def test_clipped_tiles(ctx, c):
    _check(ctx, c)


@pytest.mark.parametrize("c", R.lattice_ties(), ids=_ids(R.lattice_ties()))
def test_lattice_ties(ctx, c):
    """pixels equidistant from 2 or 4 sites (and from twice as many): the lowest id wins in either path"""
    _check(ctx, c)


def test_seeded_sweep(ctx):
    routes = {"tiles": 0, "brute": 0}
    overflowed = listed = 0
    for c in R.sweep():
        got, want, marks = _check(ctx, c, oracle=False)
        routes[c["route"]] += 1
        if c["route"] == "tiles":
            ntiles = len(R.tiles_of(c["w"], c["h"]))
            overflowed += marks[2] > 0
            listed += marks[2] < ntiles
    print("sweep: %s, %d decodes with an overflowing tile, %d with a listed one" % (routes, overflowed, listed))
    assert routes["tiles"] >= 1 and routes["brute"] >= 1 and overflowed >= 1 and listed >= 1


@pytest.mark.parametrize("host", (False, True), ids=("device destination", "host destination"))
@pytest.mark.parametrize("c", R.destinations(), ids=_ids(R.destinations()))
def test_destinations(ctx, c, host):
    """the image into caller-owned memory of either kind, sentinel bytes around it"""
    import torch
    from cniic_amd import _lib
    n = 3 * c["w"] * c["h"]
    pad = 64
    data = R.case_stream(c)
    raw = np.frombuffer(data, np.uint8)
    buf = np.full(n + 2 * pad, SENTINEL, np.uint8) if host else torch.full((n + 2 * pad,), SENTINEL, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, w, h = ctx.decode_into("voronoi(1)", raw, len(data), buf[pad:pad + n])
        marks = _marks(ctx)
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    torch.cuda.synchronize()
    out = buf if host else buf.cpu().numpy()
    assert rc == 0 and (w, h) == (c["w"], c["h"]) and marks == R.expected_marks(c)
    assert bool((out[:pad] == SENTINEL).all()) and bool((out[pad + n:] == SENTINEL).all())
    want = R.image_of(R.brute_labels(c["w"], c["h"], c["xs"], c["ys"]))
    assert np.array_equal(out[pad:pad + n].reshape(c["h"], c["w"], 3), want)
    rco, exp = O.decode("voronoi(1)", data)
    assert rco == 0 and np.array_equal(exp, want)
