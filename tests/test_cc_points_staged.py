"""The large cluster-colors encode's K-means takes its points from the histogram's staging (cniic_amd/csrc/codec.cpp: cc_prepare_image,
k_kmeans_persist.hip: the set-up's staged source, k_points.hip: k_sp_partlab's): no k_sp_emit copies the staged colours into the
K-means arrays first, the persistent launch makes every point's key and initial label itself, and the arrays are written only when
somebody needs them after all (km_rgbw_need_arrays: the loop of launches behind a launch that gave up).

Everything runs with CNIIC_SP_MIN_PIXELS = 0 and CNIIC_TEST_CC_FRONT = require.  The encodes that are to read the staging run under
CNIIC_TEST_CC_POINTS = require (the autouse fixture): an encode that could have left the emit out and did not is then an error, so no case
passes by comparing the arrays route with itself.  The witness of every case is the same library under CNIIC_TEST_CC_POINTS = arrays --
the parent's route: emit, arrays, the set-up reading them -- and the oracle (mode L, which accepts every input here): bytes, length and
statistics, all five against the arrays route (pair_evals too: the dealing of cells to blocks is the same), the three the oracle reports
against the oracle."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

STATS = ("iterations", "moved_last", "empty_reseeds", "active", "pair_evals")


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def staged_route(monkeypatch):
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    monkeypatch.setenv("CNIIC_TEST_CC_FRONT", "require")
    monkeypatch.setenv("CNIIC_TEST_CC_POINTS", "require")


def photo(w, h, seed=0):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + 70 + seed)


def rgb_of(px, w, h):
    px = np.asarray(px, np.uint32)
    assert px.size == w * h
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8).reshape(h, w, 3)


def from_keys(keys, w, h, seed):
    """an image of w x h pixels whose colours are exactly `keys` (0xRRGGBB), every one at least once, in a shuffled order"""
    keys = np.asarray(keys, np.uint32)
    assert len(keys) <= w * h
    rng = np.random.default_rng(seed)
    px = np.concatenate([keys, keys[rng.integers(0, len(keys), w * h - len(keys))]])
    rng.shuffle(px)
    return rgb_of(px, w, h)


def from_counts(keys, counts, seed):
    """a one-row image in which colour keys[i] has exactly counts[i] pixels"""
    px = np.repeat(np.asarray(keys, np.uint32), np.asarray(counts, np.int64))
    np.random.default_rng(seed).shuffle(px)
    return rgb_of(px, px.size, 1)


def keys_of(img):
    p = img.reshape(-1, 3).astype(np.uint32)
    return (p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2]


_oracle = {}


def oracle(name, img, K):
    if (name, K) not in _oracle:
        rc, data, st = O.encode("cluster-colors(%d)" % K, img, mode=O.MODE_L)
        assert rc == 0, (name, K, rc)
        _oracle[(name, K)] = (data, st)
    return _oracle[(name, K)]


def arrays(c, monkeypatch, img, K, **kw):
    with monkeypatch.context() as m:
        m.setenv("CNIIC_TEST_CC_POINTS", "arrays")
        return c.encode("cluster-colors(%d)" % K, img, **kw)


def marks(c):
    """(encodes whose K-means read the staging, emits on demand) of the last call, with the stage timers on"""
    return c.kernel_time("cc_points_staged")[1], c.kernel_time("cc_points_arrays_on_demand")[1]


def both_routes(c, monkeypatch, img, K, **kw):
    """staged and arrays: the same stream, length and all five statistics"""
    rc, data, st = c.encode("cluster-colors(%d)" % K, img, **kw)
    rca, adata, ast = arrays(c, monkeypatch, img, K, **kw)
    assert rc == rca == 0
    assert len(data) == len(adata) and data == adata
    for f in STATS:
        assert st[f] == ast[f], f
    return data, st


def three_ways(c, monkeypatch, name, img, K, **kw):
    data, st = both_routes(c, monkeypatch, img, K, **kw)
    edata, est = oracle(name, img, K)
    assert len(data) == len(edata) and data == edata
    for f in ("iterations", "moved_last", "empty_reseeds"):
        assert st[f] == est[f], f
    return data, st


def with_marks(c, fn):
    from cniic_amd import _lib
    c.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        out = fn()
        return out, marks(c)
    finally:
        c.set_opt(_lib.OPT_STAGE_TIMERS, None)


# ---- 1. initial labels: the edges of K on one chunk and on more than one; as many colours as clusters, and one fewer
@pytest.mark.parametrize("K", [2, 255, 256])
@pytest.mark.parametrize("w,h", [(64, 64), (300, 260)])
def test_photos_at_the_edges_of_k(ctx, monkeypatch, w, h, K):
    img = photo(w, h, 1)
    assert np.unique(keys_of(img)).size >= 256
    three_ways(ctx, monkeypatch, "photo%dx%d" % (w, h), img, K)


def test_the_route_is_taken_and_says_so(ctx, monkeypatch):
    img = photo(64, 64, 1)
    (rc, data, _), m = with_marks(ctx, lambda: ctx.encode("cluster-colors(16)", img))
    assert rc == 0 and m == (1, 0)
    (rca, adata, _), m = with_marks(ctx, lambda: arrays(ctx, monkeypatch, img, 16))
    assert rca == 0 and m == (0, 0) and adata == data


@pytest.mark.parametrize("K", [100, 256])
def test_as_many_colours_as_clusters_and_one_fewer(ctx, monkeypatch, K):
    from cniic_amd import _lib
    rng = np.random.default_rng(8)
    keys = rng.permutation(1 << 24)[:K].astype(np.uint32)
    img = from_keys(keys, 32, 32, 9)
    three_ways(ctx, monkeypatch, "u%d" % K, img, K)
    few = from_keys(keys[:K - 1], 32, 32, 9)
    rc, _, _ = ctx.encode("cluster-colors(%d)" % K, few, allow=(_lib.TOO_FEW_POINTS,))
    rca, _, _ = arrays(ctx, monkeypatch, few, K, allow=(_lib.TOO_FEW_POINTS,))
    assert rc == rca == _lib.TOO_FEW_POINTS
    three_ways(ctx, monkeypatch, "u%d" % K, img, K)   # the context is used again


# ---- 2. bucket bookkeeping: where a bucket's staged colours start against where its cells start
def test_first_and_last_bucket_with_empty_buckets_between(ctx, monkeypatch):
    b = np.arange(256, dtype=np.uint32)
    lo = ((b >> 5) << 16) | (((b >> 2) & 7) << 8) | ((b & 3) * 9)            # inside bucket 0: r, g, b < 32
    hi = 0xE0E0E0 | lo
    keys = np.unique(np.concatenate([lo, hi]))
    assert set(((keys >> 21) << 6 | ((keys >> 13) & 7) << 3 | (keys >> 5) & 7).tolist()) == {0, 511}
    three_ways(ctx, monkeypatch, "b0b511", from_keys(keys, 48, 32, 7), 16)


def test_a_full_super_cell_caps_the_staging_start(ctx, monkeypatch):
    """256 x 256 pixels, every colour of super-cell (2, 5, 3) twice: 2^15 distinct colours against a bucket total of 2^16 pixels (sstart
    counts min(total, 2^15) a bucket: the cap holds), every cell full at 512 points = two sweeps of 256"""
    c = np.arange(1 << 15, dtype=np.uint32)
    full = ((64 + (c >> 10)) << 16) | ((160 + ((c >> 5) & 31)) << 8) | (96 + (c & 31))
    px = np.concatenate([full, full])
    np.random.default_rng(3).shuffle(px)
    img = rgb_of(px, 256, 256)
    assert np.unique(keys_of(img)).size == 1 << 15
    three_ways(ctx, monkeypatch, "fullsuper", img, 64)


def test_300_colours_inside_one_cell(ctx, monkeypatch):
    rng = np.random.default_rng(5)
    bins = rng.permutation(512)[:300].astype(np.uint32)
    keys = (((bins >> 6) + 200) << 16) | ((((bins >> 3) & 7) + 8) << 8) | ((bins & 7) + 120)
    three_ways(ctx, monkeypatch, "onecell300", from_keys(keys, 40, 30, 6), 7)


# ---- 3. heavy movers: pixel counts of 255 and more do not fit the packed word; a point that moves looks its count up
@pytest.mark.parametrize("no_skip", [False, True])
@pytest.mark.parametrize("name", ["rgbw38", "rgbw621", "rgbw1268", "rgbw2355"])
def test_reseed_inputs_with_heavy_counts(ctx, monkeypatch, name, no_skip):
    import persist_trips_ref as P
    from cniic_amd import _lib
    keys, w, _ = P.input_of(name)
    counts = np.asarray(w, np.int64) * 9                                     # (the recorded counts reach a few dozen: times nine, 255 and more)
    assert (counts >= 255).sum() >= 3 and (counts < 255).sum() >= 3
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    data, st = three_ways(ctx, monkeypatch, name, from_counts(keys, counts, 2), P.case_K(name, None), flags=_lib.KM_NO_SKIP if no_skip else 0)
    assert st["iterations"] >= 3


# ---- 4. cells that are not resident: their packed words live in memory (pk), written by the staged set-up
def test_smallest_lds_budget_and_one_descriptor_below(ctx, monkeypatch):
    from cniic_amd import _lib, ps_layout
    img = photo(128, 128, 2)
    G = 16
    smallest = ps_layout.smallest_budget(keys_of(img), G)
    res, tot, refused = ps_layout.resident_points(keys_of(img), G, smallest)
    assert refused == 0 and res < tot // 4
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", str(G))
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_TEST_PS_LDS_BYTES", str(smallest))
    data, st = three_ways(ctx, monkeypatch, "photo128", img, 64)
    # one descriptor less: a block's cells do not fit -- the launch leaves at once (a ranges fail)
    monkeypatch.setenv("CNIIC_TEST_PS_LDS_BYTES", str(smallest - ps_layout.PS_CELL_DESC_BYTES))
    rc, _, _ = ctx.encode("cluster-colors(64)", img, allow=(_lib.HIP,))
    assert rc == _lib.HIP
    monkeypatch.delenv("CNIIC_KM_PS_REQUIRE")
    ((rc, ldata, lst), m) = with_marks(ctx, lambda: ctx.encode("cluster-colors(64)", img))
    assert rc == 0 and m == (1, 1)                                            # the classic loop, from arrays emitted on demand
    assert ldata == data and lst["iterations"] == st["iterations"]
    rca, adata, ast = arrays(ctx, monkeypatch, img, 64)
    assert rca == 0 and adata == ldata
    for f in STATS:
        assert lst[f] == ast[f], f


# ---- 5. fall-back: the launch gives up, the arrays are emitted on demand and the loop of launches runs from them
def test_an_aborted_launch_emits_the_arrays_on_demand(ctx, monkeypatch):
    img = photo(200, 280, 3)
    monkeypatch.delenv("CNIIC_KM_PS_REQUIRE", raising=False)
    monkeypatch.setenv("CNIIC_TEST_PS_ABORT_AT", "1")
    ((rc, data, st), m) = with_marks(ctx, lambda: ctx.encode("cluster-colors(48)", img))
    assert rc == 0 and m == (1, 1)
    rca, adata, ast = arrays(ctx, monkeypatch, img, 48)
    edata, est = oracle("photo200x280", img, 48)
    assert rca == 0 and data == adata == edata
    for f in STATS:
        assert st[f] == ast[f], f
    monkeypatch.delenv("CNIIC_TEST_PS_ABORT_AT")
    three_ways(ctx, monkeypatch, "photo200x280", img, 48)                     # ... and the context is fine afterwards


def test_one_block_for_uniform_noise_is_a_ranges_fail(ctx, monkeypatch):
    from cniic_amd import synth
    img = synth.uniform(256, 256, synth.SEED0 + 9)                           # ~all 32768 cells occupied: more than a block may own
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", "1")
    monkeypatch.delenv("CNIIC_KM_PS_REQUIRE", raising=False)
    ((rc, data, st), m) = with_marks(ctx, lambda: ctx.encode("cluster-colors(16)", img, max_iters=6))
    assert rc == 0 and m == (1, 1)
    rca, adata, ast = arrays(ctx, monkeypatch, img, 16, max_iters=6)
    assert rca == 0 and data == adata
    for f in STATS:
        assert st[f] == ast[f], f


# ---- 6. the dealing of cells to blocks
@pytest.mark.parametrize("blocks", ["1", "3", "16"])
def test_grids(ctx, monkeypatch, blocks):
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", blocks)
    data, st = three_ways(ctx, monkeypatch, "photo64x64", photo(64, 64, 1), 64)
    assert st["pair_evals"] > 0


@pytest.mark.parametrize("K", [2, 256])
def test_one_occupied_cell(ctx, monkeypatch, K):
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    rng = np.random.default_rng(5)
    bins = rng.permutation(512)[:300].astype(np.uint32)
    keys = ((bins >> 6) << 16) | (((bins >> 3) & 7) << 8) | (bins & 7)
    three_ways(ctx, monkeypatch, "onecell", from_keys(keys, 40, 30, 6), K)


def test_fewer_cells_than_chunks(ctx, monkeypatch):
    """five occupied cells in three buckets against 4 x 24 chunks: most chunks are empty, some blocks own nothing"""
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", "4")
    j = np.arange(60, dtype=np.uint32)
    base = np.array([0x000000, 0x000800, 0x7F7F78, 0xF8F8F0, 0xF8F8F8], np.uint32)
    keys = np.concatenate([b + ((j >> 3) << 8) + (j & 7) for b in base])
    assert np.unique(keys).size == 300
    three_ways(ctx, monkeypatch, "fivecells", from_keys(keys, 64, 40, 2), 12)


def test_every_cell_occupied(ctx, monkeypatch):
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", "64")
    rng = np.random.default_rng(12)
    i = rng.permutation(32768).astype(np.uint32)
    base = np.stack([(i >> 10) & 31, (i >> 5) & 31, i & 31], axis=1) << 3
    img = (base + rng.integers(0, 8, (32768, 3))).astype(np.uint8).reshape(128, 256, 3)
    three_ways(ctx, monkeypatch, "everycell", img, 8)


# ---- 7. routes that keep the arrays
def test_wide_labels_keep_the_arrays(ctx, monkeypatch):
    img = photo(128, 128, 2)
    ((rc, data, st), m) = with_marks(ctx, lambda: ctx.encode("cluster-colors(257)", img))
    assert rc == 0 and m == (0, 0)
    edata, est = oracle("photo128", img, 257)
    assert data == edata and st["iterations"] == est["iterations"]


def test_the_one_rank_shared_palette_keeps_the_arrays(monkeypatch):
    """cniic_cc_image_begin / _occupancy / _create on one rank: its own emit (cc_image_create) and its arrays, whatever CNIIC_TEST_CC_POINTS
    says -- the plain encode's stream on either route, and the oracle's"""
    import torch
    import cniic_amd
    from cniic_amd.dist import ShardedClusterColors
    img = photo(130, 96, 4)
    h, w = img.shape[:2]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    c = cniic_amd.Context(0, stream=stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            rc, plain, st = c.encode("cluster-colors(16)", img)
            assert rc == 0
            for mode in ("require", "arrays"):
                monkeypatch.setenv("CNIIC_TEST_CC_POINTS", mode)
                out = torch.zeros(w * h * 16, dtype=torch.uint8, device=dev)
                n, st2 = ShardedClusterColors(c, 16, None, dev).encode(torch.from_numpy(img).to(dev), w, h, out)
                assert bytes(out[:n].cpu().numpy().tobytes()) == plain and st2["iterations"] == st["iterations"], mode
        edata, est = oracle("photo130x96", img, 16)
        assert plain == edata and st["iterations"] == est["iterations"]
    finally:
        c.close()


# ---- 8. one context, encode after encode: the pool hands the same memory back, the staging of one image must not serve the next
@pytest.mark.parametrize("own_stream", [True, False])
def test_alternating_images_on_one_context(monkeypatch, own_stream):
    import torch
    from cniic_amd import Context
    rng = np.random.default_rng(3)
    small = from_keys(rng.permutation(1 << 24)[:250].astype(np.uint32), 64, 64, 4)
    large = photo(300, 260, 1)
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    stream = None if own_stream else torch.cuda.Stream(device=torch.device("cuda", 0))
    c = Context(0) if own_stream else Context(0, stream=stream.cuda_stream)
    try:
        want = [arrays(c, monkeypatch, im, 24) for im in (small, large)]
        assert all(rc == 0 for rc, _, _ in want) and want[0][1] != want[1][1]
        for turn in range(8):
            rc, data, st = c.encode("cluster-colors(24)", (small, large)[turn & 1])
            assert rc == 0 and data == want[turn & 1][1], turn
            for f in STATS:
                assert st[f] == want[turn & 1][2][f], (turn, f)
    finally:
        c.close()
