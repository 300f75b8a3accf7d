"""The set-up of a cluster-colors encode through the pixel partition between k_sp_hist and the K-means (cniic_amd/csrc/k_points.hip:
sp_front, codec.cpp: cc_prepare_image): three launches whose blocks take a role from blockIdx -- the bitmap's prefix, the scan of the
cells, the zeroing of the K-means arenas, the initial centroids, the persistent launch's chunk boundaries and the emit into the
K-means arrays -- where eleven dispatches stood.  Every role is the body of the kernel it replaces, so every result must be the same.

Everything runs with CNIIC_SP_MIN_PIXELS = 0.  The witness of every case is the same library enqueueing the dispatches one by one
(CNIIC_TEST_CC_FRONT=split) and, where it accepts the input, the oracle (mode L): bytes, length and statistics equal -- all five against
the split route, the three the oracle reports against the oracle.  The encodes that are to take the three launches run under
CNIIC_TEST_CC_FRONT=require (the autouse fixture): a silent fall-back to the split dispatches is then an error, so no case can pass by
comparing the split route with itself."""
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
def partition_route(monkeypatch):
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    monkeypatch.setenv("CNIIC_TEST_CC_FRONT", "require")


def photo(w, h, seed=0):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + 70 + seed)


def from_keys(keys, w, h, seed):
    """an image of w x h pixels whose colours are exactly `keys` (0xRRGGBB), every one at least once, in a shuffled order"""
    keys = np.asarray(keys, np.uint32)
    assert len(keys) <= w * h
    rng = np.random.default_rng(seed)
    px = np.concatenate([keys, keys[rng.integers(0, len(keys), w * h - len(keys))]])
    rng.shuffle(px)
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8).reshape(h, w, 3)


def keys_of(img):
    p = img.reshape(-1, 3).astype(np.uint32)
    return (p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2]


_oracle = {}


def oracle(name, img, K):
    if (name, K) not in _oracle:
        rc, data, st = O.encode("cluster-colors(%d)" % K, img, mode=O.MODE_L)
        assert rc == 0
        _oracle[(name, K)] = (data, st)
    return _oracle[(name, K)]


def split(c, monkeypatch, img, K, **kw):
    with monkeypatch.context() as m:
        m.setenv("CNIIC_TEST_CC_FRONT", "split")
        return c.encode("cluster-colors(%d)" % K, img, **kw)


def both_routes(c, monkeypatch, img, K, **kw):
    """fused and split: the same stream, length and all five statistics"""
    rc, data, st = c.encode("cluster-colors(%d)" % K, img, **kw)
    rcs, sdata, sst = split(c, monkeypatch, img, K, **kw)
    assert rc == rcs == 0
    assert len(data) == len(sdata) and data == sdata
    for f in STATS:
        assert st[f] == sst[f], f
    return data, st


def three_ways(c, monkeypatch, name, img, K):
    data, st = both_routes(c, monkeypatch, img, K)
    edata, est = oracle(name, img, K)
    assert len(data) == len(edata) and data == edata
    for f in ("iterations", "moved_last", "empty_reseeds"):
        assert st[f] == est[f], f
    return data, st


# ---- 1. the edges of K (255: Kpad = 256 and one padded entry; 256: the last narrow label) on one chunk and on more than one
@pytest.mark.parametrize("K", [2, 255, 256])
@pytest.mark.parametrize("w,h", [(64, 64), (300, 260)])
def test_photos_at_the_edges_of_k(ctx, monkeypatch, w, h, K):
    img = photo(w, h, 1)
    assert np.unique(keys_of(img)).size >= 256
    three_ways(ctx, monkeypatch, "photo%dx%d" % (w, h), img, K)


# ---- 2. one non-empty cell: M = 1, the ranges bisect a table of one entry, the emit sees one bucket
@pytest.mark.parametrize("K", [2, 256])
def test_one_cell(ctx, monkeypatch, K):
    rng = np.random.default_rng(5)
    bins = rng.permutation(512)[:300].astype(np.uint32)
    keys = ((bins >> 6) << 16) | (((bins >> 3) & 7) << 8) | (bins & 7)
    assert keys.size == 300 and int(((keys >> 16) | (keys >> 8) | keys).max() & 255) < 8
    three_ways(ctx, monkeypatch, "onecell", from_keys(keys, 40, 30, 6), K)


# ---- 3. the two ends of colour space: bitmap blocks 0 and 255 of the prefix roles, cells 0 and 32767, the sentinels behind the last group
@pytest.mark.parametrize("K", [16, 256])
def test_two_ends_of_colour_space(ctx, monkeypatch, K):
    b = np.arange(256, dtype=np.uint32)
    keys = np.concatenate([b, 0xFFFF00 | b])
    img = from_keys(keys, 48, 32, 7)
    assert {0x000000, 0xFFFFFF} <= set(keys_of(img).tolist())
    three_ways(ctx, monkeypatch, "twoends", img, K)


# ---- 4. as many colours as clusters (a point per chunk), and one fewer: refused on both routes, the context usable afterwards
def test_as_many_colours_as_clusters_and_one_fewer(ctx, monkeypatch):
    from cniic_amd import _lib
    rng = np.random.default_rng(8)
    keys = rng.permutation(1 << 24)[:100].astype(np.uint32)
    img = from_keys(keys, 32, 32, 9)
    three_ways(ctx, monkeypatch, "u100", img, 100)
    rc, _, _ = ctx.encode("cluster-colors(101)", img, allow=(_lib.TOO_FEW_POINTS,))
    rcs, _, _ = split(ctx, monkeypatch, img, 101, allow=(_lib.TOO_FEW_POINTS,))
    assert rc == rcs == _lib.TOO_FEW_POINTS
    three_ways(ctx, monkeypatch, "u100", img, 100)


# ---- 5. wide labels: no persistent launch, so the third launch has no ranges role, and the centroid role runs with Kpad = 260
def test_wide_labels_have_no_ranges_role(ctx, monkeypatch):
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")   # (asks for nothing where there is no persistent launch to be had)
    three_ways(ctx, monkeypatch, "photo300x260", photo(300, 260, 1), 257)


# ---- 6. one block for several thousand non-empty cells: the ranges role raises the fail word as k_ps_ranges does
def test_fail_word_of_the_ranges_role(ctx, monkeypatch):
    from cniic_amd import _lib, synth
    img = synth.uniform(256, 256, synth.SEED0 + 9)   # uniform noise: ~all 32768 cells occupied
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", "1")
    monkeypatch.delenv("CNIIC_KM_PS_REQUIRE", raising=False)
    both_routes(ctx, monkeypatch, img, 16, max_iters=6)   # the classic loop, from untouched arrays
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    rc, _, _ = ctx.encode("cluster-colors(16)", img, max_iters=6, allow=(_lib.HIP,))
    rcs, _, _ = split(ctx, monkeypatch, img, 16, max_iters=6, allow=(_lib.HIP,))
    assert rc == rcs == _lib.HIP


# ---- 7. the pool hands the same memory back encode after encode: a zeroing role that misses a word shows here
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
        want = [split(c, monkeypatch, im, 24) for im in (small, large)]
        assert all(rc == 0 for rc, _, _ in want) and want[0][1] != want[1][1]
        for turn in range(8):
            rc, data, st = c.encode("cluster-colors(24)", (small, large)[turn & 1])
            assert rc == 0 and data == want[turn & 1][1], turn
            for f in STATS:
                assert st[f] == want[turn & 1][2][f], (turn, f)
    finally:
        c.close()


# ---- 8. pair_evals depends on every chunk boundary the ranges role writes
@pytest.mark.parametrize("blocks", ["3", "16"])
def test_chunk_boundaries_by_pair_evals(ctx, monkeypatch, blocks):
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", blocks)
    data, st = three_ways(ctx, monkeypatch, "photo300x260", photo(300, 260, 1), 64)
    assert st["pair_evals"] > 0
