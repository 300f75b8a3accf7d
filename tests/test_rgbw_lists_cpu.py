"""Without a GPU: tests/rgbw_lists_ref.py restates the kernels' constants as the headers have them, its pruning never drops a centroid that
brute force finds nearest somewhere in a cube, and every case of tests/test_rgbw_limits.py crosses -- on the oracle's own trajectory -- the
switch it is there for (the figures in the docstrings are what this file measured; the assertions are the conditions, not the figures)."""
import os

import numpy as np
import pytest

import oracle_lib as O
import rgbw_lists_ref as R
import warm_ref as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cniic_amd", "csrc")


def test_constants_are_the_headers():
    text = {h: " ".join(open(os.path.join(CSRC, h)).read().split()) for h in ("common.hpp", "device_utils.hpp", "kmeans_rgbw.hpp")}
    for name, (value, header, line) in R.CONSTANTS.items():
        assert line in text[header], "%s: %s no longer has `%s`" % (name, header, line)
        if value is not None:
            assert getattr(R, name) == value, name
    assert "constexpr uint32_t kSupersPerDim = kCellsPerDim / 4;" in text["device_utils.hpp"] and R.SUPERS_PER_DIM == 8
    assert "uint32_t max_skip = 64;" in text["kmeans_rgbw.hpp"]
    assert [R.km_scap(K) for K in (1, 96, 255, 256, 257, 300, 1023, 1024, 2048)] == [1, 48, 128, 128, 129, 150, 512, 512, 512]
    assert [R.km_ccap(K) for K in (1, 256, 257, 2048)] == [1, 256, 256, 256]
    assert R.kPsOffCell == 24576 and R.ps_cell_bytes(2048) == 16 + 2048 * 57 and R.ps_cell_bytes(2047) == R.ps_cell_bytes(2048) == R.ps_cell_bytes(2045)
    assert R.kPsOffCell + R.ps_cell_bytes(R.kPsMaxCells) == 141328 <= R.kPsDynBytes == 160768   # (a full block's descriptors fit the launch's LDS)


def test_cells_are_super_cell_major_and_the_boxes_hold_their_colours():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (4000, 3))
    c = R.cell_of(R.key_of(rgb))
    assert c.min() >= 0 and c.max() < 32768
    lo = R.cell_box(c)
    assert np.all((rgb >= lo) & (rgb <= lo + R.CELL_EXT))
    slo = R.super_box(c >> R.kSuperShift)
    assert np.all((rgb >= slo) & (rgb <= slo + R.SUPER_EXT)) and np.all(slo % 32 == 0) and np.all(lo % 8 == 0)
    assert len(np.unique(R.cell_of(R.key_of(np.stack(np.meshgrid(*[np.arange(0, 256, 8)] * 3, indexing="ij"), -1).reshape(-1, 3))))) == 32768
    assert R.cell_of(0x000000) == 0 and R.cell_of(0xffffff) == 32767 and R.cell_of(0x0000ff) == (7 << 6) | 3 and R.cell_of(0x000800) == 4


def brute_nearest(cent, lo, side):
    """the ids that are nearest (ties count) for some integer colour of the cube"""
    g = np.arange(side)
    cube = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + lo).astype(np.int32)   # (a squared distance is below 2^18)
    cent = cent.astype(np.int32)
    win = np.zeros(len(cent), bool)
    for a in range(0, len(cube), 4096):
        d = ((cube[a:a + 4096, None, :] - cent[None, :, :]) ** 2).sum(-1)
        win |= (d == d.min(axis=1, keepdims=True)).any(axis=0)
    return np.nonzero(win)[0]


def random_table(rng, K, lo, side):
    """centroids near the cube and far from it, some of them twice"""
    near = lo + rng.integers(-side, 2 * side, (K, 3))
    far = rng.integers(0, 256, (K, 3))
    cent = np.clip(np.where(rng.random((K, 1)) < 0.7, near, far), 0, 255).astype(np.int64)
    for _ in range(K // 8):
        cent[rng.integers(0, K)] = cent[rng.integers(0, K)]
    return cent


def test_the_restated_pruning_keeps_every_centroid_that_is_nearest_somewhere():
    """200 random (cube, table) pairs, 180 cells and 20 super-cells, K from 2 to 256, duplicates included: what brute force over every integer
    colour of the cube finds nearest (a tie counts) is in the kept set -- of the table, and for a cell of its super-cell's list as well"""
    rng = np.random.default_rng(2)
    pruned = 0
    for n in range(200):
        K = int(rng.integers(2, 257)) if n % 10 else (2, 256)[n // 10 % 2]
        if n < 180:
            cell = int(rng.integers(0, 32768))
            lo = R.cell_box(cell)
            cent = random_table(rng, K, lo, 8)
            need = brute_nearest(cent, lo, 8)
            S = R.super_list(cent, cell >> R.kSuperShift)
            kept, kept_s = R.cell_candidates(cent, cell), R.cell_candidates(cent, cell, S)
            assert np.all(np.isin(need, kept)) and np.all(np.isin(need, kept_s)) and np.all(np.isin(kept_s, S))
            assert R.pivot(cent, np.arange(K), lo, R.CELL_EXT) in kept
            pruned += K - len(kept)
        else:
            sup = int(rng.integers(0, 512))
            lo = R.super_box(sup)
            cent = random_table(rng, K, lo, 32)
            kept = R.super_list(cent, sup)
            assert np.all(np.isin(brute_nearest(cent, lo, 32), kept))
            pruned += K - len(kept)
    assert pruned > 0   # (a restatement that keeps everything would pass the above too)


def test_worst_is_the_maximum_it_says_it_is():
    rng = np.random.default_rng(3)
    g = np.arange(8)
    for _ in range(50):
        lo = rng.integers(0, 32, 3) * 8
        p, v = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
        cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + lo
        assert R.worst(p, lo, 7, v) == (((cube - p) ** 2).sum(-1) - ((cube - v) ** 2).sum(-1)).max()


# ------------------------------------------------------------------ the crossing conditions of tests/test_rgbw_limits.py's cases
def test_trajectory_is_the_oracles_run():
    for name in ("a97", "f512", "e"):
        c, r = R.case(name), R.report(name, lists=False)
        rc, exp = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(c["keys"]), c["w"], c["K"])
        assert rc == r["run"]["rc"] and exp["stats"]["iterations"] == r["iterations"] == len(r["tabs"]) - 1
        assert np.array_equal(exp["centroids"], r["tabs"][-1]) and np.array_equal(exp["labels"], r["labs"][-1])
        assert np.array_equal(r["labs"][0], O.init_labels(len(c["keys"]), c["K"]))


@pytest.mark.parametrize("K", [96, 97, 256])
def test_a_one_super_cell_whose_list_is_the_table(K):
    """6000 colours of one 32^3 cube: the list has K members in every iteration (27, 22 and 38 of them): 96 = kPsScap, the strip exactly full;
    97, the first table build; 256.  At K = 256 cells have up to 69 candidates: more than one 64-bit mask word's worth."""
    r = R.report("a%d" % K)
    sup = int(R.cell_of(R.key_of(np.array(R.A_CUBE)))) >> R.kSuperShift
    assert len(r["occ"]) == 64 and r["iterations"] >= 3
    assert all(s == {sup: K} for s in r["sizes"])
    assert (K <= R.kPsScap) == (K == 96) and K > R.km_scap(K)
    if K == 256:
        assert max(x.max() for x in r["ncand_ps"]) > 64 and max(x.max() for x in r["ncand_cl"]) > 64


@pytest.mark.parametrize("name,sizes", [("b128", (128, 128)), ("b129", (129, 127))])
def test_b_two_far_super_cells_around_km_scap(name, sizes):
    """(128, 128): the launches' strip exactly full; (129, 127): one table build; both in every iteration (26 and 22), and no reseed carries a
    centroid across"""
    r = R.report(name)
    assert R.km_scap(256) == 128
    assert all(s == {0: sizes[0], 511: sizes[1]} for s in r["sizes"]) and r["iterations"] >= 3 and r["run"]["empty_reseeds"] == 0


def test_c_one_cell_whose_candidates_are_the_table():
    """K = 256 on the 512 colours of one cell: 256 candidates, all eight mask words full -- in the only iteration of the run from the reference's
    init (the mean of two neighbours is the first of them), in all 6 of the run from placed centroids.  K = 300: 300 candidates > km_ccap and a
    300-member list > km_scap(300) = 150 in all 11 iterations.  256 placed in the cell and 44 far away: exactly 256, the strip full, in 6 of 6
    iterations; 257 + 43: 257, the first table sweep, in 8 of 8."""
    cell = int(R.cell_of(R.key_of(np.array(R.C_CELL))))
    for name, n, least in (("c256", 256, 1), ("c256p", 256, 6), ("c300", 300, 11), ("c300_256", 256, 6), ("c300_257", 257, 8)):
        r = R.report(name)
        i = int(np.nonzero(r["occ"] == cell)[0][0])
        assert r["pop"][i] == 512
        holds = 0
        while holds < r["iterations"] and r["ncand_cl"][holds][i] == n and r["ncand_ps"][holds][i] == n:
            holds += 1
        assert holds >= 1 and holds >= least, (name, holds)
        assert r["sizes"][0][cell >> R.kSuperShift] == n > R.km_scap(R.case(name)["K"])
    assert R.km_ccap(300) == 256 and R.km_scap(300) == 150


@pytest.mark.parametrize("name", ["d18", "f512"])
def test_d_cells_of_one_to_five_candidates_in_one_iteration(name):
    """case a's colours with K = 18, and the 512-super-cell case: iteration 0 has cells of exactly 1, 2, 3, 4 and 5 candidates (four id bytes,
    then the mask); later iterations have lone-candidate cells all of whose points already carry that candidate (68 and several thousand):
    ps_row_finish's no-sweep exit.  With K = 18, 353 points of 4-candidate cells move to the FOURTH candidate in iteration 0 (72, 38, 19 in the
    next three): the last id byte decides labels."""
    r = R.report(name)
    assert {1, 2, 3, 4, 5} <= set(r["ncand_ps"][0].tolist())
    exits, fourth = 0, []
    for j in range(r["iterations"]):
        for i in np.nonzero(r["ncand_ps"][j] == 1)[0] if j else ():
            exits += bool(np.all(r["labs"][j][r["cells"] == r["occ"][i]] == r["cand_ps"][j][i][0]))
        n = 0
        for i in np.nonzero(r["ncand_ps"][j] == 4)[0]:
            mine, k4 = r["cells"] == r["occ"][i], r["cand_ps"][j][i][3]
            n += int(((r["labs"][j + 1][mine] == k4) & (r["labs"][j][mine] != k4)).sum())
        fourth.append(n)
    assert exits > 0
    if name == "d18":
        assert fourth[0] >= 64 and sum(f > 0 for f in fourth) >= 3, fourth


def test_e_cell_populations_and_weights():
    """cells of 1, 255, 256, 257, 511 and 512 colours; points of every weight -- 1, 254, 255 (the escape), 256, 2^31, 2^32 - 1 -- change label
    after iteration 0 (131, 127, 115, 127, 123 and 110 times): the signed deltas carry 255 (2^32 - 1)"""
    c, r = R.case("e"), R.report("e", lists=False)
    assert sorted(r["pop"].tolist()) == sorted(R.E_POPULATIONS) and 64 * R.kSweep == 256
    for wv in R.E_WEIGHTS:
        assert sum(int(((r["labs"][j] != r["labs"][j + 1]) & (c["w"] == wv)).sum()) for j in range(1, r["iterations"])) > 0, wv


def test_f_runs_and_slots():
    """one colour per super-cell and one block: 32 runs (every cell has a list), 33 (one cell has none), 512 (480 have none); two cells per
    super-cell and two blocks: 16 super-cells are cut by a chunk boundary and take a slot on either side"""
    for name, nsup in (("f32", 32), ("f33", 33), ("f512", 512)):
        rg = R.report(name, lists=False)
        assert rg["G"] == 1 and rg["ranges"]["runs"] == [nsup] and len(rg["ranges"]["slotless"]) == max(0, nsup - R.kPsSlotsMax)
        assert len(rg["occ"]) == nsup == len(np.unique(rg["occ"] >> R.kSuperShift)) and R.case(name)["K"] <= 32
    r = R.report("f_split", lists=False)
    rg = r["ranges"]
    assert r["G"] == 2 and len(r["occ"]) == 1024 and np.all(np.unique(r["occ"] >> R.kSuperShift, return_counts=True)[1] == 2)
    assert len(rg["split"]) > 0 and sum(rg["runs"]) == 512 + len(rg["split"])
    # ... one of them among the first kPsSlotsMax runs of both blocks it lies in: both halves DO get a list
    cb, occ = rg["cb"], r["occ"]
    early = [m for m in cb[1:5] if 0 < m < len(occ) and (occ[m - 1] >> R.kSuperShift) == (occ[m] >> R.kSuperShift)]
    assert early and int(occ[early[0]]) not in rg["slotless"] and int(occ[early[0] - 1]) not in rg["slotless"]


def test_g_cells_per_block():
    """2047 and 2048 cells in one block run, 2049 are refused; 4088 cells in two blocks: 2048 and 2040"""
    for name, n, refused in (("g2047", 2047, False), ("g2048", 2048, False), ("g2049", 2049, True)):
        r = R.report(name, lists=False)
        assert r["G"] == 1 and r["ranges"]["ncells"] == [n] and r["ranges"]["refused"] == refused and np.all(r["pop"] == 1)
    r = R.report("g_two", lists=False)
    assert r["G"] == 2 and max(r["ranges"]["ncells"]) == R.kPsMaxCells and not r["ranges"]["refused"] and np.all(r["pop"] == 1)


def test_h_skip_threshold():
    """the K = 256 run of case a moves 237 174 133 116 101 85 73 63 56 59 45 40 36 35 31 22 26 25 20 21 22 24 27 26 14 13 13 13 9 10 10 8 6 2 2 1
    0 0 centroids: for every max_skip tried some update moves exactly that many (skip at equality) and some one more (full)"""
    nS = R.report("a256", lists=False)["nS"]
    for m in R.H_MAXSKIP:
        assert m <= 64 and m in nS and m + 1 in nS, m
    assert max(nS) > R.kMaxMovedSkip and any(0 < v <= R.kMaxMovedSkip for v in nS)


def test_i_aggregated_booking():
    """iterations 1 to kAggLaunches of a2 and e: cells with 16 and more movers sharing one (old, new) pair (62 and 40 at most), and cells whose pair
    has 1 to 15"""
    for name in ("a2", "e"):
        r = R.report(name, lists=False)
        counts = []
        for j in range(1, R.kAggLaunches + 1):
            counts += list(R.movers_by_pair(r["labs"][j], r["labs"][j + 1], r["cells"]).values())
        assert max(counts) >= R.kAggMin and any(1 <= v < R.kAggMin for v in counts)
    assert R.report("a2", lists=False)["pop"].max() <= 256   # (one sweep per cell: the cell's movers are the sweep's)


def test_j_k_as_many_clusters_as_points_and_one_more():
    c = R.case("j")
    assert c["K"] == len(c["keys"]) <= 256
    rc, _ = W.lloyd_from(O.PT_RGBW, R.pts_of_keys(c["keys"][:-1]), c["w"][:-1], c["K"], R.pts_of_keys(c["keys"]))
    rco, _ = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(c["keys"][:-1]), c["w"][:-1], c["K"])
    assert rc == rco == O.TOO_FEW_POINTS
