"""The persistent colour K-means (cniic_amd/csrc/k_kmeans_persist.hip) where its state lives and how its set-up is ordered: the
running sums and the run's totals in LDS instead of registers, the LDS budget beside them, the block ranges and set-up pointers that
k_ps_ranges leaves for the launch (one context, encodes of very different images in turn), and states that are made and never run.
Everything under CNIIC_KM_PS_REQUIRE=1 -- a silent hand-over to the launch-per-iteration loop is an error -- and against the oracle
(mode L), as tests/test_persistent_kmeans.py does; the launch-per-iteration loop (OPT_KM_LOOP = 1) is the second witness for the
codec's bytes.

pair_evals: the two loops do NOT count the same number -- each counts what ITS schedule evaluated (include/cniic_hip.h), and the
persistent launch leaves out cells the launches sweep (64 x 64 photo, K = 2: 35398 against 95900; 300 x 260, K = 64: 4215262 against
5695052).  The figure of the persistent launch is held to what the launch gave BEFORE its per-wave count became a scalar and its
total moved into LDS: tests/golden/persist_pair_evals.json, recorded from the library of the commit before this file with the
grid pinned (CNIIC_KM_PS_BLOCKS: the count depends on which block owns which cells) by the same case builders the tests use.  Where
the two loops do coincide (the re-seed inputs of LOOP_EQUAL) the launches' figure is asserted equal as well; everywhere the launches'
figure stays inside what any schedule keeps: iteration 0 sweeps every point against at least one candidate and its own centroid
(>= 2 U), and no iteration evaluates more than every point against every centroid and its own (<= iterations x U x (K + 1))."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reseed_golden.npz"))
RGBW = ["rgbw38", "rgbw621", "rgbw1268", "rgbw2355"]
PAIR_EVALS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persist_pair_evals.json")))["pair_evals"]
LOOP_EQUAL = ("rgbw38", "rgbw1268", "rgbw2355")   # inputs on which the launches count what the persistent launch counts
STATS = ("iterations", "moved_last", "empty_reseeds")   # ... and `active`, which the oracle gives as the clusters that end with members


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


def photo(h, w, seed):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + seed)


def keys_of(img):
    p = img.reshape(-1, 3).astype(np.uint32)
    return (p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2]


def pts_of_keys(keys):
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=1).astype(np.int32)


def colours_of(img):
    keys, counts = O.count_freqs(keys_of(img))
    return keys, counts.astype(np.uint32)


_oracle = {}


def oracle_run(name, keys, w, K):
    """the oracle's run of one input, computed once"""
    if (name, K) not in _oracle:
        _oracle[(name, K)] = O.kmeans(O.PT_RGBW, O.MODE_L, pts_of_keys(keys), w, K)
    return _oracle[(name, K)]


def assert_run_equals(got, exp):
    assert np.array_equal(got["centroids"].astype(np.int32), exp["centroids"])
    assert np.array_equal(got["labels"], exp["labels"])
    assert np.array_equal(got["members"], exp["members"])
    for f in STATS:
        assert got["stats"][f] == exp["stats"][f], f
    assert got["stats"]["active"] == int((exp["members"] > 0).sum())


# ---- the cases whose pair_evals are recorded: (id, oracle name, keys, counts, K, flags, environment).  The tests and the recording run these.
def sums_case(K, shape):
    keys, w = colours_of(photo(*shape, seed=40 + shape[0]))
    return ("sums-%d-%dx%d" % (K, shape[0], shape[1]), "photo%dx%d" % shape, keys, w, K, 0, {"CNIIC_KM_PS_BLOCKS": "8" if shape[0] == 64 else "32"})


def reseed_case(name, no_skip):
    from cniic_amd import _lib
    return ("reseed-%s-%d" % (name, no_skip), name, GOLD[name + "_keys"], GOLD[name + "_weight"], int(GOLD[name + "_K"][0]),
            _lib.KM_NO_SKIP if no_skip else 0, {"CNIIC_KM_PS_BLOCKS": "4"})


def budget_case(which, no_skip):
    from cniic_amd import _lib
    keys, w = colours_of(photo(300, 260, seed=5))
    return ("budget-%s-%d" % (which, no_skip), "photo300x260", keys, w, 64, _lib.KM_NO_SKIP if no_skip else 0,
            {"CNIIC_KM_PS_BLOCKS": "16", "CNIIC_TEST_PS_LDS_BYTES": str(budgets(keys)[which])})


def recorded_cases():
    return ([sums_case(K, shape) for K in (2, 255, 256) for shape in ((64, 64), (128, 128))]
            + [reseed_case(name, ns) for name in RGBW for ns in (False, True)]
            + [budget_case(which, ns) for which in ("full", "smallest") for ns in (False, True)])


def persistent_and_loop(ctx, monkeypatch, case):
    """the persistent launch and the launches against the oracle (results and the whole stats block); pair_evals of the persistent
    launch equal to the recorded figure, of the launches equal to it where the loops coincide and inside the bounds every schedule
    keeps (the module's docstring)"""
    from cniic_amd import _lib
    cid, name, keys, w, K, flags, env = case
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rco, exp = oracle_run(name, keys, w, K)
    rc, got = ctx.kmeans_rgbw(keys, w, K, flags=flags)
    assert rc == rco == 0
    assert_run_equals(got, exp)
    ctx.set_opt(_lib.OPT_KM_LOOP, 1)
    try:
        rcl, loop = ctx.kmeans_rgbw(keys, w, K, flags=flags)
    finally:
        ctx.set_opt(_lib.OPT_KM_LOOP, None)
    assert rcl == 0
    assert_run_equals(loop, exp)
    print("pair_evals %s: persistent %d, recorded %d, launches %d" % (cid, got["stats"]["pair_evals"], PAIR_EVALS[cid], loop["stats"]["pair_evals"]))
    assert got["stats"]["pair_evals"] == PAIR_EVALS[cid]
    if name in LOOP_EQUAL:
        assert loop["stats"]["pair_evals"] == got["stats"]["pair_evals"]
    U, it = int(np.asarray(keys).size), exp["stats"]["iterations"]
    assert 2 * U <= loop["stats"]["pair_evals"] <= it * U * (K + 1)
    return exp


# ------------------------------------------------------------------ 1. where the running sums and the totals live
@pytest.mark.parametrize("shape", [(64, 64), (128, 128)])
@pytest.mark.parametrize("K", [2, 255, 256])
def test_running_sums_in_lds_at_the_edges_of_k(ctx, monkeypatch, K, shape):
    """K = 255 / 256: the last clusters of the array of running sums (thread k < K owns cluster k)"""
    persistent_and_loop(ctx, monkeypatch, sums_case(K, shape))


@pytest.mark.parametrize("no_skip", [False, True])
@pytest.mark.parametrize("name", RGBW)
def test_empty_clusters_reseed_from_the_sums_in_lds(ctx, monkeypatch, name, no_skip):
    """the committed inputs whose runs meet empty clusters (a cluster's member count in the running sums is zero): the re-seeds,
    and their total, which now lives in one thread's LDS words"""
    exp = persistent_and_loop(ctx, monkeypatch, reseed_case(name, no_skip))
    assert exp["stats"]["empty_reseeds"] >= 2


# ------------------------------------------------------------------ 2. the LDS budget after the layout change
@pytest.fixture(scope="module")
def budget_input():
    keys, w = colours_of(photo(300, 260, seed=5))
    return keys, w


def budgets(keys):
    """full / the smallest the range check accepts / one cell's descriptor less, from the layout's constants (cniic_amd/ps_layout.py
    mirrors csrc/kmeans_rgbw.hpp) and the dealing of this image's cells to 16 blocks -- no trial runs"""
    from cniic_amd import ps_layout as L
    smallest = L.smallest_budget(keys, 16)
    assert L.PS_OFF_CELL < smallest < L.PS_BUDGET
    return {"full": L.PS_BUDGET, "smallest": smallest, "refused": smallest - L.PS_CELL_DESC_BYTES}


@pytest.mark.parametrize("no_skip", [False, True])
@pytest.mark.parametrize("which", ["full", "smallest"])
def test_lds_budget_accepted(ctx, monkeypatch, budget_input, which, no_skip):
    """smallest: the descriptors of the block with most cells just fit, so next to no cell keeps its points in LDS"""
    from cniic_amd import ps_layout as L
    keys, w = budget_input
    if which == "smallest":
        res, tot, refused = L.resident_points(keys, 16, budgets(keys)[which])
        assert refused == 0 and res < tot // 4
    persistent_and_loop(ctx, monkeypatch, budget_case(which, no_skip))


@pytest.mark.parametrize("no_skip", [False, True])
def test_lds_budget_one_descriptor_short_is_refused_before_any_block_waits(ctx, monkeypatch, budget_input, no_skip):
    """the fail word of k_ps_ranges: with REQUIRE an error, without it the launches give the oracle's run"""
    from cniic_amd import _lib
    keys, w = budget_input
    flags = _lib.KM_NO_SKIP if no_skip else 0
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", "16")
    monkeypatch.setenv("CNIIC_TEST_PS_LDS_BYTES", str(budgets(keys)["refused"]))
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    rc, _ = ctx.kmeans_rgbw(keys, w, 64, flags=flags, allow=(_lib.HIP,))
    assert rc == _lib.HIP
    monkeypatch.delenv("CNIIC_KM_PS_REQUIRE")
    rco, exp = oracle_run("photo300x260", keys, w, 64)
    rc, got = ctx.kmeans_rgbw(keys, w, 64, flags=flags)
    assert rc == rco == 0
    assert_run_equals(got, exp)


# ------------------------------------------------------------------ 3. what k_ps_ranges leaves for the launch, encode after encode
def few_colours(h, w, n, seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return pal[rng.integers(0, n, h * w)].reshape(h, w, 3)


@pytest.mark.parametrize("sp_min", ["0", str(1 << 40)])
@pytest.mark.parametrize("own_stream", [True, False])
def test_alternating_images_on_one_context(monkeypatch, own_stream, sp_min):
    """ranges or set-up pointers that were the encode's before would change the bytes or be refused: two images with very different
    numbers of non-empty cells in turn on one context, on its own stream and on the caller's (sp_min = 0: the pixel-partition
    route, where k_sp_emit fills the arrays between k_ps_ranges and the launch)"""
    import torch
    from cniic_amd import Context, _lib
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", sp_min)
    small, large = few_colours(64, 64, 250, 3), photo(300, 260, seed=5)
    assert np.unique(keys_of(small)).size < 300
    stream = None if own_stream else torch.cuda.Stream(device=torch.device("cuda", 0))
    c = Context(0) if own_stream else Context(0, stream=stream.cuda_stream)
    try:
        c.set_opt(_lib.OPT_KM_LOOP, 1)
        want = [c.encode("cluster-colors(24)", im) for im in (small, large)]
        c.set_opt(_lib.OPT_KM_LOOP, None)
        assert all(rc == 0 for rc, _, _ in want) and want[0][1] != want[1][1]
        for turn in range(8):
            rc, data, st = c.encode("cluster-colors(24)", (small, large)[turn & 1])
            assert rc == 0 and data == want[turn & 1][1] and st["iterations"] == want[turn & 1][2]["iterations"], turn
    finally:
        c.close()


# ------------------------------------------------------------------ 4. states that never launch
def test_states_that_are_made_and_never_run(monkeypatch):
    """cniic_cc_image_begin -> _create -> close: the block ranges are enqueued when the state gives its memory back"""
    import torch
    from cniic_amd import Context
    from cniic_amd.dist import HipBackend
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    img = photo(300, 260, seed=5)
    dev = torch.device("cuda", 0)
    c = Context(0)
    try:
        be = HipBackend(c, dev)
        t = torch.from_numpy(img).to(dev)
        for _ in range(20):
            h = be.image_begin(t, 300 * 260)
            assert h is not None
            try:
                be.image_create(h, be.image_occupancy(h), 32, be.new_partials(32))
            finally:
                be.destroy(h)
        rc, data, st = c.encode("cluster-colors(32)", img)
        rco, edata, est = O.encode("cluster-colors(32)", img, mode=O.MODE_L)
        assert rc == rco == 0 and data == edata and st["iterations"] == est["iterations"]
    finally:
        c.close()


def test_launch_loop_encodes_after_a_persistent_one(monkeypatch):
    """OPT_KM_LOOP = 1 on a context whose previous encode was persistent: no ranges are made, none are read"""
    from cniic_amd import Context, _lib
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    img = photo(128, 160, seed=9)
    rco, edata, est = O.encode("cluster-colors(32)", img, mode=O.MODE_L)
    assert rco == 0
    c = Context(0)
    try:
        rc, data, st = c.encode("cluster-colors(32)", img)
        assert rc == 0 and data == edata
        c.set_opt(_lib.OPT_KM_LOOP, 1)
        for _ in range(20):
            rc, data, st = c.encode("cluster-colors(32)", img)
            assert rc == 0 and data == edata and st["iterations"] == est["iterations"]
        c.set_opt(_lib.OPT_KM_LOOP, None)
        rc, data, st = c.encode("cluster-colors(32)", img)
        assert rc == 0 and data == edata and st["iterations"] == est["iterations"]
    finally:
        c.close()
