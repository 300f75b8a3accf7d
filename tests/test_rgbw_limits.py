"""The colour K-means -- the persistent launch (cniic_amd/csrc/k_kmeans_persist.hip) and the launch-per-iteration loop (k_rgbw_assign_cells,
k_kmeans_rgbw.hip) -- at the list, slot and schedule limits both are built around, every case bit for bit against the oracle: return code,
iterations, empty_reseeds, centroids, labels and members.  tests/rgbw_lists_ref.py builds the cases and tests/test_rgbw_lists_cpu.py asserts,
from the oracle's trajectory and without a GPU, that each of them crosses what it is here for:

  a  one super-cell whose list is the whole table: K = 96 = kPsScap (the shared strip exactly full), 97 (the first table build), 256 (cells of
     more than 64 candidates); K = 1, 2, 63, 64, 65, 255 around the 64-lane ballot rounds, label 255 and the lone-candidate exit
  b  two far super-cells with 128 + 128 placed centroids (km_scap(256): the launches' strip exactly full) and 129 + 127 (one table build)
  c  one cell whose candidates are the table: 256 (all eight mask words full); 300 (u16 labels: beyond km_ccap and km_scap); 256 / 257 of 300
     placed in the cell (the candidate strip exactly full / the first table sweep)
  d  cells of exactly 1, 2, 3, 4 and 5 candidates in one iteration, hundreds of points that move to a cell's FOURTH candidate (case a's
     colours with K = 18; f512 has the five counts too)
  e  cells of 1, 255, 256, 257, 511 and 512 colours; movers of weight 1, 254, 255, 256, 2^31 and 2^32 - 1
  f  32, 33 and 512 (chunk, super-cell) runs in one block for kPsSlotsMax = 32 lists; a super-cell cut by a chunk boundary
  g  2047 and 2048 = kPsMaxCells cells in one block, 2049 (refused), two blocks of which the larger has 2048
  h  max_skip at and one below the number of centroids an update moves
  i  16 and more movers sharing an (old, new) pair in iterations 1 to 3, and fewer (cases a2, e)
  j  K = U        k  U = K - 1

Every run is capped at the oracle's iteration count + 8: a correct kernel stops before, a wrong one cannot loop inside a persistent launch.
The oracle's run is computed once per case and shared by the routes."""
import numpy as np
import pytest

import oracle_lib as O
import rgbw_lists_ref as R
import warm_ref as W

pytestmark = pytest.mark.gpu

KNOBS = ("CNIIC_KM_PS_REQUIRE", "CNIIC_KM_UNFUSED", "CNIIC_KM_PS_CLEANSKIP", "CNIIC_KM_PS_BLOCKS", "CNIIC_KM_MAXSKIP", "CNIIC_KM_LOOP",
         "CNIIC_KM_MAX_BLOCKS", "CNIIC_TEST_PS_ABORT_AT", "CNIIC_TEST_PS_LDS_BYTES")
# route: (environment, flags, the context's loop option)
ROUTES = {
    "persistent": ({"CNIIC_KM_PS_REQUIRE": "1"}, 0, False),        # (REQUIRE: a silent hand-over to the launches is an error)
    "launches": ({}, 0, True),
    "unfused": ({"CNIIC_KM_UNFUSED": "1"}, 0, False),
    "persistent-noskip": ({"CNIIC_KM_PS_REQUIRE": "1"}, "KM_NO_SKIP", False),
    "persistent-nocleanskip": ({"CNIIC_KM_PS_REQUIRE": "1", "CNIIC_KM_PS_CLEANSKIP": "0"}, 0, False),
    "brute": ({}, "KM_BRUTE_FORCE", False),                         # a second witness that shares no list with the others
}
NARROW = list(ROUTES)                                  # K <= 256
WIDE = ["launches", "unfused", "brute"]                # u16 labels: the persistent launch does not take them


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


_RUN = {}


def oracle_run(name):
    """-> dict(rc, centroids, labels, members, iterations, empty_reseeds) of the case, computed once"""
    if name not in _RUN:
        c = R.case(name)
        pts = R.pts_of_keys(c["keys"])
        if c["init"] is None:
            rc, exp = O.kmeans(O.PT_RGBW, O.MODE_L, pts, c["w"], c["K"])
            ref = dict(rc=rc, centroids=exp["centroids"], labels=exp["labels"], members=exp["members"], iterations=exp["stats"]["iterations"],
                       empty_reseeds=exp["stats"]["empty_reseeds"])
        else:
            rc, ref = W.lloyd_from(O.PT_RGBW, pts, c["w"], c["K"], c["init"])
        assert rc in (O.OK, O.FEW_ACTIVE)
        _RUN[name] = ref
    return _RUN[name]


def run_case(ctx, monkeypatch, name, route, env=None, allow=()):
    from cniic_amd import _lib
    c, ref = R.case(name), oracle_run(name)
    renv, flags, loop = ROUTES[route]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if c["blocks"]:
        monkeypatch.setenv("CNIIC_KM_PS_BLOCKS", str(c["blocks"]))
    for k, v in list(renv.items()) + list((env or {}).items()):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    if loop:
        ctx.set_opt(_lib.OPT_KM_LOOP, 1)
    try:
        return ctx.kmeans_rgbw(c["keys"], c["w"], c["K"], max_iters=ref["iterations"] + 8, flags=getattr(_lib, flags) if flags else 0, init=c["init"],
                               allow=(_lib.FEW_ACTIVE,) + tuple(allow))
    finally:
        if loop:
            ctx.set_opt(_lib.OPT_KM_LOOP, None)


def check_case(ctx, monkeypatch, name, route, env=None):
    ref = oracle_run(name)
    rc, got = run_case(ctx, monkeypatch, name, route, env)
    assert rc == ref["rc"]
    assert got["stats"]["iterations"] == ref["iterations"]
    assert got["stats"]["empty_reseeds"] == ref["empty_reseeds"]
    assert np.array_equal(got["centroids"].astype(np.int32), ref["centroids"])
    assert np.array_equal(got["labels"], ref["labels"])
    assert np.array_equal(got["members"], ref["members"])


# ------------------------------------------------------------------ a. one super-cell, list = K
@pytest.mark.parametrize("route", NARROW)
@pytest.mark.parametrize("K", R.A_KS)
def test_a_one_super_cell_whose_list_is_the_table(ctx, monkeypatch, K, route):
    check_case(ctx, monkeypatch, "a%d" % K, route)


# ------------------------------------------------------------------ b. two far super-cells around km_scap(256)
@pytest.mark.parametrize("route", NARROW)
@pytest.mark.parametrize("name", ["b128", "b129"])
def test_b_two_far_super_cells_around_km_scap(ctx, monkeypatch, name, route):
    check_case(ctx, monkeypatch, name, route)


# ------------------------------------------------------------------ c. one cell, candidates = K
@pytest.mark.parametrize("route", NARROW)
@pytest.mark.parametrize("name", ["c256", "c256p"])
def test_c_one_cell_with_256_candidates(ctx, monkeypatch, name, route):
    check_case(ctx, monkeypatch, name, route)


@pytest.mark.parametrize("route", WIDE)
@pytest.mark.parametrize("name", ["c300", "c300_256", "c300_257"])
def test_c_one_cell_around_the_candidate_strip_with_wide_labels(ctx, monkeypatch, name, route):
    check_case(ctx, monkeypatch, name, route)


# ------------------------------------------------------------------ d. few candidates: the four id bytes of a record
@pytest.mark.parametrize("route", NARROW)
def test_d_cells_of_one_to_five_candidates(ctx, monkeypatch, route):
    check_case(ctx, monkeypatch, "d18", route)


# ------------------------------------------------------------------ e. cell populations and weights
@pytest.mark.parametrize("route", NARROW)
def test_e_cell_populations_and_heavy_movers(ctx, monkeypatch, route):
    check_case(ctx, monkeypatch, "e", route)


# ------------------------------------------------------------------ f. runs and slots of one block
@pytest.mark.parametrize("route", NARROW)
@pytest.mark.parametrize("name", ["f32", "f33", "f512", "f_split"])
def test_f_more_runs_than_shared_lists(ctx, monkeypatch, name, route):
    check_case(ctx, monkeypatch, name, route)


# ------------------------------------------------------------------ g. cells per block
@pytest.mark.parametrize("route", NARROW)
@pytest.mark.parametrize("name", ["g2047", "g2048", "g_two"])
def test_g_blocks_of_up_to_2048_cells(ctx, monkeypatch, name, route):
    check_case(ctx, monkeypatch, name, route)


def test_g_a_block_of_2049_cells_is_refused(ctx, monkeypatch):
    """the designed refusal: an error where the persistent launch is required, the launches' (and the oracle's) result where it is not"""
    from cniic_amd import _lib
    rc, _ = run_case(ctx, monkeypatch, "g2049", "persistent", allow=(_lib.HIP,))
    assert rc == _lib.HIP
    check_case(ctx, monkeypatch, "g2049", "persistent", env={"CNIIC_KM_PS_REQUIRE": None})
    for route in ("launches", "brute"):
        check_case(ctx, monkeypatch, "g2049", route)


# ------------------------------------------------------------------ h. the skip threshold
@pytest.mark.parametrize("route", ["persistent", "launches"])
@pytest.mark.parametrize("max_skip", list(R.H_MAXSKIP) + [None])
def test_h_max_skip_at_and_below_what_an_update_moves(ctx, monkeypatch, max_skip, route):
    check_case(ctx, monkeypatch, "a256", route, env=None if max_skip is None else {"CNIIC_KM_MAXSKIP": str(max_skip)})


# ------------------------------------------------------------------ j, k. K = U, U = K - 1
@pytest.mark.parametrize("route", NARROW)
def test_j_as_many_clusters_as_colours(ctx, monkeypatch, route):
    check_case(ctx, monkeypatch, "j", route)


def test_k_one_colour_too_few(ctx, monkeypatch):
    from cniic_amd import _lib
    c = R.case("j")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rc, _ = ctx.kmeans_rgbw(c["keys"][:-1], c["w"][:-1], c["K"], allow=(_lib.TOO_FEW_POINTS,))
    rco, _ = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(c["keys"][:-1]), c["w"][:-1], c["K"])
    assert rc == rco == O.TOO_FEW_POINTS == _lib.TOO_FEW_POINTS
