"""The skip schedule's row test of the persistent colour K-means (cniic_amd/csrc/k_kmeans_persist.hip) with its lanes per cell and its
trips sized by what moved: 4, 8 or 16 lanes a cell and ceil(nS / lanes) trips, chosen per iteration from nS and the block's cells
(ps_row_group), instead of 16 lanes and four trips whatever the iteration holds.  The verdict per cell is the same OR over the same
terms, so every case must give

  - the oracle's run bit for bit: centroids, labels, members, iterations, moved_last, empty_reseeds, active;
  - the `pair_evals` of the same case under CNIIC_TEST_PS_TRIPS=fixed (the fixed widths), and the recorded figure of
    tests/golden/persist_pair_evals.json where that file has the case;
  - the marks of a KM_PROFILE run -- `kmeans_rgbw_persist_g4 / _g8 / _g16`: block 0's skip-schedule iterations per group width -- that
    tests/persist_trips_ref.py predicts from the oracle's trajectory and the block's cells: the form that was asked for is the one that ran.

tests/test_persist_trips_cpu.py asserts without a GPU that the cases sit where they should: nS at and beside every CNIIC_KM_MAXSKIP of
THRESHOLDS, every forced width at nS = 1, L, L + 1 and 64, a block of 128 | 129 and 256 | 257 cells and one of fewer cells than a group
has lanes.  Two further measures of the same issue -- list builds of ceil(longest list / 16) trips, and drawing the next cell one ahead
-- were built, measured and taken out (NOTES AM); the list, slot and queue limits of the code they would have touched stay with
tests/test_rgbw_limits.py.  Every run is under CNIIC_KM_PS_REQUIRE=1 unless it is about the hand-over, and capped at the oracle's
iteration count + 8: a wrong kernel cannot loop inside a persistent launch."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import persist_trips_ref as P
import rgbw_lists_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("CNIIC_KM_PS_REQUIRE", "CNIIC_KM_PS_BLOCKS", "CNIIC_KM_MAXSKIP", "CNIIC_TEST_PS_ABORT_AT", "CNIIC_TEST_PS_LDS_BYTES", "CNIIC_TEST_PS_TRIPS",
         "CNIIC_TEST_PS_GROUP", "CNIIC_KM_PS_CLEANSKIP", "CNIIC_KM_UNFUSED", "CNIIC_KM_LOOP", "CNIIC_KM_MAX_BLOCKS")
PAIR_EVALS = json.load(open(os.path.join(P.HERE, "golden", "persist_pair_evals.json")))["pair_evals"]
MARKS = {4: "kmeans_rgbw_persist_g4", 8: "kmeans_rgbw_persist_g8", 16: "kmeans_rgbw_persist_g16"}


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


_ORACLE = {}


def oracle_run(name, K):
    if (name, K) not in _ORACLE:
        keys, w, _ = P.input_of(name)
        rc, exp = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(keys), w, K)
        assert rc == O.OK
        _ORACLE[(name, K)] = exp
    return _ORACLE[(name, K)]


def run(ctx, monkeypatch, name, K, env, flags=0, require=True):
    from cniic_amd import _lib
    keys, w, blocks = P.input_of(name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", str(blocks))
    if require:
        monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rc, got = ctx.kmeans_rgbw(keys, w, K, max_iters=oracle_run(name, K)["stats"]["iterations"] + 8, flags=flags | _lib.KM_PROFILE)
    assert rc == 0
    got["marks"] = {Lw: ctx.kernel_time(m)[1] for Lw, m in MARKS.items()}
    return got


def assert_oracle(got, exp):
    assert np.array_equal(got["centroids"].astype(np.int32), exp["centroids"])
    assert np.array_equal(got["labels"], exp["labels"])
    assert np.array_equal(got["members"], exp["members"])
    for f in ("iterations", "moved_last", "empty_reseeds"):
        assert got["stats"][f] == exp["stats"][f], f
    assert got["stats"]["active"] == int((exp["members"] > 0).sum())


def check(ctx, monkeypatch, name, K=None, env=None, flags=0, forced=None, gold=None):
    """the case in the form asked for and in the fixed one: both the oracle's run, the same pair_evals, the predicted marks"""
    from cniic_amd import _lib
    K, env = P.case_K(name, K), dict(env or {})
    exp = oracle_run(name, K)
    if forced:
        env["CNIIC_TEST_PS_GROUP"] = str(forced)
    max_skip = 0 if flags & _lib.KM_NO_SKIP else int(env.get("CNIIC_KM_MAXSKIP", P.MAX_MOVED_SKIP))
    got = run(ctx, monkeypatch, name, K, env, flags)
    assert_oracle(got, exp)
    fixed = run(ctx, monkeypatch, name, K, dict(env, CNIIC_TEST_PS_TRIPS="fixed", CNIIC_TEST_PS_GROUP=""), flags)
    assert_oracle(fixed, exp)
    print("pair_evals %s K %d %s: %d, fixed %d, recorded %s; marks %s" % (name, K, env, got["stats"]["pair_evals"], fixed["stats"]["pair_evals"],
                                                                       PAIR_EVALS.get(gold), got["marks"]))
    assert got["stats"]["pair_evals"] == fixed["stats"]["pair_evals"]
    if gold:
        assert got["stats"]["pair_evals"] == PAIR_EVALS[gold]
    assert got["marks"] == P.expected_marks(name, K, max_skip, forced=forced)
    assert fixed["marks"] == P.expected_marks(name, K, max_skip, fixed=True)


# ------------------------------------------------------------------ nS and the skip threshold
@pytest.mark.parametrize("max_skip", P.THRESHOLDS)
def test_skip_threshold_at_and_beside_what_an_update_moves(ctx, monkeypatch, max_skip):
    name, K = P.THRESHOLD_INPUT if max_skip != 64 else P.FULL_INPUT
    check(ctx, monkeypatch, name, K, env={"CNIIC_KM_MAXSKIP": str(max_skip)})


# ------------------------------------------------------------------ every forced width at nS = 1, L, L + 1, 64
@pytest.mark.parametrize("forced", P.WIDTHS)
@pytest.mark.parametrize("which", ["threshold", "full"])
def test_every_forced_width(ctx, monkeypatch, which, forced):
    name, K = P.THRESHOLD_INPUT if which == "threshold" else P.FULL_INPUT
    check(ctx, monkeypatch, name, K, forced=forced)


# ------------------------------------------------------------------ the existing builders' inputs, K = 2, 64, 255, 256
@pytest.mark.parametrize("shape", [(64, 64), (128, 128)])
@pytest.mark.parametrize("K", [2, 64, 255, 256])
def test_photos_at_the_edges_of_k(ctx, monkeypatch, K, shape):
    gold = "sums-%d-%dx%d" % (K, shape[0], shape[1])
    check(ctx, monkeypatch, "photo%dx%d" % shape, K, gold=gold if gold in PAIR_EVALS else None)


@pytest.mark.parametrize("no_skip", [False, True])
@pytest.mark.parametrize("name", P.RGBW)
def test_reseed_inputs(ctx, monkeypatch, name, no_skip):
    from cniic_amd import _lib
    check(ctx, monkeypatch, name, flags=_lib.KM_NO_SKIP if no_skip else 0, gold="reseed-%s-%d" % (name, no_skip))


# ------------------------------------------------------------------ cells per block
@pytest.mark.parametrize("forced", [None] + list(P.WIDTHS))
@pytest.mark.parametrize("M", P.BLOCK_CELLS)
def test_a_block_of_128_129_256_257_cells(ctx, monkeypatch, M, forced):
    check(ctx, monkeypatch, "cells%d" % M, forced=forced)


@pytest.mark.parametrize("forced", [None] + list(P.WIDTHS))
@pytest.mark.parametrize("M", sorted(P.FEW_CELLS.values()))
def test_a_block_of_fewer_cells_than_a_group_has_lanes(ctx, monkeypatch, M, forced):
    check(ctx, monkeypatch, "few%d" % M, forced=forced)


# ------------------------------------------------------------------ the LDS budget: the points live in memory
@pytest.mark.parametrize("forced", [None, 8])
def test_smallest_lds_budget(ctx, monkeypatch, forced):
    from cniic_amd import ps_layout as L
    keys, _, blocks = P.input_of("photo300x260")
    smallest = L.smallest_budget(keys, blocks)
    res, tot, refused = L.resident_points(keys, blocks, smallest)
    assert refused == 0 and res < tot // 4
    check(ctx, monkeypatch, "photo300x260", 64, env={"CNIIC_TEST_PS_LDS_BYTES": str(smallest)}, forced=forced, gold="budget-smallest-0")


# ------------------------------------------------------------------ the hand-over and the two schedules
def test_abort_at_the_first_barrier_hands_over_to_the_launches(ctx, monkeypatch):
    name, K = P.FULL_INPUT
    keys, w, blocks = P.input_of(name)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", str(blocks))
    monkeypatch.setenv("CNIIC_TEST_PS_ABORT_AT", "1")
    rc, got = ctx.kmeans_rgbw(keys, w, K)
    assert rc == 0
    assert_oracle(got, oracle_run(name, K))


@pytest.mark.parametrize("no_skip", [False, True])
def test_eight_alternating_encodes_on_one_context(monkeypatch, no_skip):
    """two images with very different numbers of cells in turn on one context, under the skip schedule and with KM_NO_SKIP (the full
    schedule in every iteration): the launch-per-iteration loop's bytes every time"""
    from cniic_amd import Context, _lib
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (250, 3)).astype(np.uint8)
    small, large = pal[rng.integers(0, 250, 64 * 64)].reshape(64, 64, 3), P.photo(300, 260, seed=5)
    flags = _lib.KM_NO_SKIP if no_skip else 0
    c = Context(0)
    try:
        c.set_opt(_lib.OPT_KM_LOOP, 1)
        want = [c.encode("cluster-colors(24)", im, flags=flags) for im in (small, large)]
        c.set_opt(_lib.OPT_KM_LOOP, None)
        assert all(rc == 0 for rc, _, _ in want) and want[0][1] != want[1][1]
        for turn in range(8):
            rc, data, st = c.encode("cluster-colors(24)", (small, large)[turn & 1], flags=flags)
            assert rc == 0 and data == want[turn & 1][1] and st["iterations"] == want[turn & 1][2]["iterations"], turn
    finally:
        c.close()
