"""k_ps_ranges (cniic_amd/csrc/k_kmeans_persist.hip) bisects the cost prefix of the non-empty cells: the table's two ends and a size
in between.  M = 1 (every colour in one 8^3 cell: all boundaries of all chunks fall on the same two words), M = 32 768 = kNumCells
(one colour in every cell: the whole table, kNumCells + 1 words) and a photo of a few thousand cells.  Each is encoded through
the pixel partition (CNIIC_SP_MIN_PIXELS = 0) with the grid pinned (CNIIC_KM_PS_BLOCKS) and CNIIC_KM_PS_REQUIRE = 1, so that a range
the launch refuses is an error: the bytes equal the launch-per-iteration loop's (OPT_KM_LOOP = 1) and the oracle's, the iterations
too.

pair_evals depends on which block owns which cells, that is on every boundary k_ps_ranges writes, and the two loops do not count the
same number (tests/test_persistent_kmeans_state.py).  So the persistent launch's figure is held to what the library of the commit
BEFORE this file gave for the same case (a variant of the kernel that bisects a copy of the table in LDS was measured against these
figures, NOTES AG): tests/golden/ps_ranges_pair_evals.json, recorded on the MI355X by running this file as a script
(`python tests/test_ps_ranges_edges.py OUT.json`) against that commit's testing library."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ps_ranges_pair_evals.json")
NUM_CELLS = 32768


def cells_of(img):
    p = img.reshape(-1, 3).astype(np.uint32) >> 3
    return np.unique((p[:, 0] << 10) | (p[:, 1] << 5) | p[:, 2]).size


def one_cell():
    rng = np.random.default_rng(11)
    return rng.integers(0, 8, (64, 64, 3)).astype(np.uint8)


def every_cell():
    """256 x 128 pixels, pixel i in cell i, somewhere inside it"""
    rng = np.random.default_rng(12)
    i = rng.permutation(NUM_CELLS).astype(np.uint32)
    base = np.stack([(i >> 10) & 31, (i >> 5) & 31, i & 31], axis=1) << 3
    return (base + rng.integers(0, 8, (NUM_CELLS, 3))).astype(np.uint8).reshape(128, 256, 3)


def a_photo():
    from cniic_amd import synth
    return synth.photo(260, 300, synth.SEED0 + 5)


#        id           image       cells the image must have          K   blocks
CASES = [("one-cell", one_cell, lambda m: m == 1, 4, "4"),
         ("every-cell", every_cell, lambda m: m == NUM_CELLS, 8, "64"),
         ("photo", a_photo, lambda m: 1000 < m < NUM_CELLS // 2, 64, "16")]


def persistent_encode(ctx, case, setenv):
    """(image, (rc, bytes, stats)) of the persistent launch for one case; setenv(name, value): monkeypatch.setenv in a test"""
    cid, make, cells_ok, K, blocks = case
    img = make()
    assert cells_ok(cells_of(img)), (cid, cells_of(img))
    for k, v in (("CNIIC_KM_PS_REQUIRE", "1"), ("CNIIC_SP_MIN_PIXELS", "0"), ("CNIIC_KM_PS_BLOCKS", blocks)):
        setenv(k, v)
    return img, ctx.encode("cluster-colors(%d)" % K, img)


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ranges_at_the_ends_of_the_table(ctx, monkeypatch, case):
    import oracle_lib as O
    from cniic_amd import _lib
    cid, _, _, K, _ = case
    img, (rc, data, st) = persistent_encode(ctx, case, monkeypatch.setenv)
    ctx.set_opt(_lib.OPT_KM_LOOP, 1)
    try:
        rcl, ldata, lst = ctx.encode("cluster-colors(%d)" % K, img)
    finally:
        ctx.set_opt(_lib.OPT_KM_LOOP, None)
    rco, edata, est = O.encode("cluster-colors(%d)" % K, img, mode=O.MODE_L)
    assert rc == rcl == rco == 0
    assert data == ldata and data == edata
    assert st["iterations"] == lst["iterations"] == est["iterations"]
    want = json.load(open(GOLDEN))["pair_evals"][cid]
    print("pair_evals %s: persistent %d, recorded %d, launches %d" % (cid, st["pair_evals"], want, lst["pair_evals"]))
    assert st["pair_evals"] == want


if __name__ == "__main__":   # the recording: against the library whose figures are the reference (see the module's docstring)
    os.environ.setdefault("CNIIC_USE_TESTING_LIB", "1")
    from cniic_amd import Context
    c = Context(0)
    rec = {}
    for case in CASES:
        _, (rc, _, st) = persistent_encode(c, case, os.environ.__setitem__)
        assert rc == 0, case[0]
        rec[case[0]] = st["pair_evals"]
    c.close()
    json.dump({"pair_evals": rec}, open(sys.argv[1], "w"), indent=1)
    print(rec)
