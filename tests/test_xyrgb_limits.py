"""The tiled 5-D K-means (cniic_amd/csrc/k_kmeans_xyrgb.hip: voronoi(K), cniic_kmeans_xyrgb) at the edges it is built around, every case
bit for bit against the oracle (return code, iterations, empty_reseeds, centroids, labels, members; a step: labels, sums, members, changed).

  sides      x or y up to 16383 -- the kernel's 24-bit products, its 32-bit bound (xy_bounds.hpp) and the single-precision quotient of
             xy_div_floor were never compared with anything beyond 130 pixels; 16384 is the last tiled side, 16385 the first wide one.
  placed     one step with centroids the test places: opposite corners (the largest operands the bound and the score can see), twins (a tie goes
             to the lowest id; a point that is there stays), pairs mirrored about a tile edge and a super-tile edge with equal colours (a pixel
             on the bisector stays, kmeans.rs:375), K = 4096 random ones.
  table      xy_create keeps the centroid table in LDS, and folds the update into the assign launch, while
                 fixed + 16 K + 16 * 64 * 18 <= 153 KiB,   fixed = 4 * ((6 K + 3) & ~3) + 18 * 1024 + 16 * 512 + 16 * 8 * ceil(K / 64):
             K = 2656 gives 95744 + 42496 + 18432 = 156672 = 153 KiB exactly (strips of 64); K = 2657 gives 95776 + 42512 + 18432 = 156720,
             48 bytes over: the first K that reads centroids from memory, runs k_xy_update as a launch of its own and has strips of 192.
             K = 4096 (strips of 64) uses all four slots of mine[], all 12 id bits of the pivot key and all 64 words of s_smask.
             (xy_bounds_ref.lds_plan restates the formula; tests/test_xyrgb_arith_cpu.py asserts these figures.)
  lists      a super-tile list beyond kSCap = 1024 is brute-forced, a tile's strip beyond wcap sweeps the super-tile's list, and the folded-in
             update lists at most kXMaxMovedSkip = 512 moved centroids.  xy_bounds_ref.list_sizes says BEFORE a case runs that it crosses
             what it is there to cross, by a quarter of the cap at least.
  schedule   16384 x 272: 320 super-tiles for 256 blocks at the largest x, dealt statically, from the counter, and with the separate update.

The oracle is the slow side (seconds; the GPU takes milliseconds), so a result is computed once per case and shared by the flags and knobs."""
import struct

import numpy as np
import pytest

import oracle_lib as O
import xy_bounds_ref as R

pytestmark = pytest.mark.gpu

FLAGS3 = [0, 1, 4]   # 0, KM_BRUTE_FORCE, KM_NO_SKIP


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


def xy_pts(img):
    h, w = img.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    return np.concatenate([x.reshape(-1, 1), y.reshape(-1, 1), img.reshape(-1, 3)], axis=1).astype(np.int32)


_IMG, _RUN = {}, {}


def image(w, h, K):
    if (w, h, K) not in _IMG:
        _IMG[(w, h, K)] = R.case_image(w, h, K)
    return _IMG[(w, h, K)]


def oracle_run(w, h, K, max_iters):
    key = (w, h, K, max_iters)
    if key not in _RUN:
        _RUN[key] = O.kmeans(O.PT_XYRGB, O.MODE_L, xy_pts(image(w, h, K)), None, K, max_iters=max_iters)
    return _RUN[key]


def c5_of(cent):
    return np.concatenate([cent["x"][:, None], cent["y"][:, None], cent["rgb"]], axis=1).astype(np.int32)


def check_run(ctx, w, h, K, max_iters, flags):
    from cniic_amd import _lib
    rco, exp = oracle_run(w, h, K, max_iters)
    rc, got = ctx.kmeans_xyrgb(image(w, h, K), K, max_iters=max_iters, flags=flags, allow=(_lib.FEW_ACTIVE,))
    assert rc == rco and rc in (0, _lib.FEW_ACTIVE)
    assert _lib.FEW_ACTIVE == O.FEW_ACTIVE
    assert got["stats"]["iterations"] == exp["stats"]["iterations"]
    assert got["stats"]["empty_reseeds"] == exp["stats"]["empty_reseeds"]
    assert np.array_equal(c5_of(got["centroids"]), exp["centroids"])
    assert np.array_equal(got["labels"], exp["labels"])
    assert np.array_equal(got["members"], exp["members"])
    return exp


# ------------------------------------------------------------------ a. sides at the limit
SIDES = [(16384, 16, 16, 40), (16, 16384, 7, 0), (16383, 17, 33, 30), (16384, 1, 3, 0), (16384, 16, 1, 0), (16384, 16, 2, 0),
         (16384, 3, 9, 0), (16385, 3, 9, 0)]


@pytest.mark.parametrize("flags", FLAGS3)
@pytest.mark.parametrize("w,h,K,max_iters", SIDES)
def test_sides_at_the_limit(ctx, w, h, K, max_iters, flags):
    """the last tile of 16383 x 17 is 63 wide and its second tile row 1 high; K = 1 divides a sum of about 2 * 10^9 by m = 262144;
    16385 x 3 is the wide kernel's: both sides of the hand-over equal the oracle"""
    check_run(ctx, w, h, K, max_iters, flags)


@pytest.mark.parametrize("w,h,K,max_iters", SIDES[:2])
def test_sides_at_the_limit_with_the_separate_update(ctx, monkeypatch, w, h, K, max_iters):
    monkeypatch.setenv("CNIIC_XY_UNFUSED", "1")   # the table in LDS, k_xy_update a launch of its own
    check_run(ctx, w, h, K, max_iters, 0)


# ------------------------------------------------------------------ b. one step, centroids placed by the test
def check_step(ctx, img, c5, labels):
    from cniic_amd._lib import COLORPOS
    K = len(c5)
    c5 = np.asarray(c5, np.int32)
    cent = np.zeros(K, COLORPOS)
    cent["x"], cent["y"], cent["rgb"] = c5[:, 0], c5[:, 1], c5[:, 2:5]
    got = ctx.kmeans_step_xyrgb(img, K, cent, labels)
    exp = O.kmeans_step(O.PT_XYRGB, xy_pts(img), None, K, c5, labels)
    for f in ("labels", "sums", "members"):
        assert np.array_equal(got[f], exp[f]), f
    assert got["changed"] == exp["changed"]
    return got


LONG = [(16384, 16), (16, 16384)]


@pytest.mark.parametrize("w,h", LONG)
def test_step_centroids_at_opposite_corners(ctx, w, h):
    """(0, 0, black), (w - 1, h - 1, white) and their mirror images: the largest c* - k and c* + k - 2 p"""
    img = image(w, h, 4)
    c5 = [[0, 0, 0, 0, 0], [w - 1, h - 1, 255, 255, 255], [w - 1, 0, 0, 0, 0], [0, h - 1, 255, 255, 255]]
    rng = np.random.default_rng(w)
    for labels in (rng.integers(0, 4, w * h), np.zeros(w * h, np.int64), np.full(w * h, 1)):
        check_step(ctx, img, c5, labels.astype(np.uint32))


@pytest.mark.parametrize("w,h", LONG)
def test_step_twin_centroids_at_the_largest_coordinate(ctx, w, h):
    """two centroids equal in every coordinate, at x = 16383 (y = 16383 on the tall image): a point of the second twin stays with it, a point
    that comes from elsewhere goes to the first"""
    img = image(w, h, 3)
    far = [w - 1, h // 2, 128, 128, 128] if w > h else [w // 2, h - 1, 128, 128, 128]
    c5 = [far, far, [0, 0, 128, 128, 128]]
    labels = np.random.default_rng(h).integers(0, 3, w * h).astype(np.uint32)
    got = check_step(ctx, img, c5, labels)
    after = got["labels"]
    assert not np.any((labels != 1) & (after == 1)) and not np.any((labels == 1) & (after == 0))   # nobody joins the second twin, nobody leaves it for the first
    assert np.any((labels == 1) & (after == 1))
    assert np.any((labels == 2) & (got["labels"] == 0)) and np.any((labels == 0) & (got["labels"] == 2))


@pytest.mark.parametrize("w,h", LONG)
def test_step_pairs_mirrored_about_tile_and_super_tile_edges(ctx, w, h):
    """pairs of equal colour: straddling an edge (63 | 64, 4095 | 4096: the bisector runs between two tiles / super-tiles), two either side of it
    (the bisector IS the first column of the next tile / super-tile) and a diagonal pair whose bisector crosses the edge.  A pixel on a bisector
    is equally far from both whatever its colour: it keeps the label it has if that is one of the two, and otherwise takes the lower id."""
    wide = w > h
    tile, sup, n, o = (64, 256, w, h) if wide else (16, 64, h, w)   # along the long axis; o: the short one
    col = [90, 140, 200]
    along = [(tile - 1, 8), (tile, 8), (17 * tile - 2, 5), (17 * tile + 2, 5), (9 * sup - 2, 9), (9 * sup + 2, 9), (16 * sup - 1, 3), (16 * sup, 3),
             (32 * sup - 1, 4), (32 * sup, 3), (n - 1, 12), (n - 5, 12)]
    c5 = [([a, b] if wide else [b, a]) + col for (a, b) in along]
    K = len(c5)
    img = image(w, h, K)
    lab0 = np.random.default_rng(n + o).integers(0, K, (h, w)).astype(np.uint32)
    lines = ((17 * tile, (2, 3)), (9 * sup, (4, 5)), (n - 3, (10, 11)))   # the bisector columns (rows on the tall image) and their pairs
    for (pos, ids) in lines:   # on a bisector: pixels of either centroid of the pair, and pixels that come from far away (centroid 0)
        line = np.resize(np.array([ids[0], ids[1], ids[1], ids[0], 0], np.uint32), o)
        if wide:
            lab0[:, pos] = line
        else:
            lab0[pos, :] = line
    labels = lab0.reshape(-1)
    got = check_step(ctx, img, c5, labels)
    lab1 = got["labels"].reshape(h, w)
    for (pos, ids) in lines:
        b0, b1 = (lab0[:, pos], lab1[:, pos]) if wide else (lab0[pos, :], lab1[pos, :])
        mine = np.isin(b0, ids)
        assert np.array_equal(b0[mine], b1[mine])        # whoever is with one of the two stays with it
        assert np.all(b1[~mine] == ids[0])               # whoever arrives goes to the lower id


def test_step_4096_random_centroids_at_full_width(ctx):
    w, h, K = 16384, 4, 4096
    img = image(w, h, K)
    rng = np.random.default_rng(K)
    c5 = np.concatenate([rng.integers(0, w, (K, 1)), rng.integers(0, h, (K, 1)), rng.integers(0, 256, (K, 3))], axis=1)
    check_step(ctx, img, c5, rng.integers(0, K, w * h).astype(np.uint32))


# ------------------------------------------------------------------ c. K above the LDS table
ABOVE = [(128, 96, 2656, 12), (128, 96, 2657, 12), (128, 96, 4096, 0), (300, 100, 3000, 6)]


@pytest.mark.parametrize("flags", FLAGS3)
@pytest.mark.parametrize("w,h,K,max_iters", ABOVE)
def test_k_around_and_above_the_lds_table(ctx, w, h, K, max_iters, flags):
    assert R.lds_plan(K)[0] == (K <= 2656)
    check_run(ctx, w, h, K, max_iters, flags)


def voronoi_stream(w, h, c5):
    """VoronoiCluster::encode's stream (clusterc.rs:156-164): w, h, K as usize, then x, y and a 3-byte colour vector per centroid"""
    b = struct.pack("<IIQ", w, h, len(c5))
    for c in c5:
        b += struct.pack("<IIQ", int(c[0]), int(c[1]), 3) + bytes([int(c[2]), int(c[3]), int(c[4])])
    return b


def test_voronoi_3000_stream_equals_the_oracles(ctx):
    """The oracle's encoder takes no iteration cap; its stream is the serialisation of its K-means' centroids (shown first on a run short
    enough to leave uncapped), so the capped stream is that of the capped K-means."""
    from cniic_amd import synth
    small = synth.photo(32, 24, synth.SEED0 + 5)
    rcs, sdata, _ = O.encode("voronoi(4)", small, mode=O.MODE_L)
    rck, sk = O.kmeans(O.PT_XYRGB, O.MODE_L, xy_pts(small), None, 4)
    assert rcs == rck == 0 and sdata == voronoi_stream(32, 24, sk["centroids"])
    w, h, K, cap = 300, 100, 3000, 6
    rco, exp = oracle_run(w, h, K, cap)
    assert rco == 0
    edata = voronoi_stream(w, h, exp["centroids"])
    expr = "voronoi(%d)" % K
    rc, data, st = ctx.encode(expr, image(w, h, K), max_iters=cap)
    assert rc == 0 and st["iterations"] == exp["stats"]["iterations"] == cap
    assert len(data) == 16 + 19 * K and data == edata
    rc, back = ctx.decode(expr, data)
    rcd, eback = O.decode(expr, edata)
    assert rc == rcd == 0 and np.array_equal(back, eback)


# ------------------------------------------------------------------ d. list capacities, with a checked precondition
@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("w,h,K,max_iters,s_least,s_most,t_least", R.CAPACITY_CASES)
def test_lists_longer_than_their_capacity(ctx, w, h, K, max_iters, s_least, s_most, t_least, flags):
    R.capacity_precondition(image(w, h, K), K, s_least, s_most, t_least)   # (asserted without a GPU too: tests/test_xyrgb_arith_cpu.py)
    check_run(ctx, w, h, K, max_iters, flags)


@pytest.mark.parametrize("unfused", ["", "1"])
@pytest.mark.parametrize("K", [513, 600])
def test_more_moved_centroids_than_the_skip_schedule_lists(ctx, monkeypatch, K, unfused):
    """the first updates move more than kXMaxMovedSkip = 512 centroids (every one of them moves off its seed pixel), later ones fewer: the
    folded-in update's list must stop at 512 entries, and the schedule changes under way"""
    if unfused:
        monkeypatch.setenv("CNIIC_XY_UNFUSED", unfused)
    w, h = 520, 130
    _, one = oracle_run(w, h, K, 1)   # the precondition: the first update moves more centroids than the list holds (of K = 513 / 600 the oracle's
    # updates move 513 513 490 455 ... 225 / 600 572 488 422 ... 180)
    assert int((one["centroids"] != R.init_centroids(image(w, h, K), K)).any(axis=1).sum()) > R.MOVED_SKIP
    check_run(ctx, w, h, K, 12, 0)


# ------------------------------------------------------------------ e. several super-tiles per block at the largest coordinate
@pytest.mark.parametrize("knob", ["", "CNIIC_XY_DYN=0", "CNIIC_XY_DYN=100000", "CNIIC_XY_UNFUSED=1"])
def test_more_super_tiles_than_blocks_at_full_width(ctx, monkeypatch, knob):
    w, h, K = 16384, 272, 5
    assert ((w + 255) // 256) * ((h + 63) // 64) == 320   # super-tiles, for 256 blocks
    if knob:
        monkeypatch.setenv(*knob.split("="))
    check_run(ctx, w, h, K, 3, 0)
