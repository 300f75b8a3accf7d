"""The arithmetic of the voronoi repaint (cniic_amd/csrc/vor_paint.hpp) and what tests/test_vor_paint.py relies on, without a GPU.
tests/vor_paint_check.cpp is compiled against the header as a stand-alone program -- the keep predicate against every pixel of small
rectangles, the kernel's steps against the wrapping brute force on whole images, the pivot key and the keep predicate at coordinate 16383
-- and runs once plain and once under -fsanitize=address,undefined.  Then the numpy model of tests/vor_paint_ref.py: its painting equals
the numpy brute force (and the oracle's decode) for every case of the GPU tests, and every case has the property it is named for: the
kept count, the tie pixel that alone tells `f >= 0` from `f > 0`, the list of exactly 256 that alone tells `n <= cap` from `n < cap`,
the route."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O
import vor_paint_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vor_paint_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "cniic_amd", "csrc")
PARTS = ("equivalence", "tiles", "extremes", "gate", "total")


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln.split()[1].rstrip(":") for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert tuple(ok) == PARTS and "FAIL" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def test_header_against_every_pixel_and_the_wrapping_brute_force(tmp_path):
    exe = str(tmp_path / "vor_paint_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    m = re.search(r"largest key (\d+) <= (\d+), largest product (\d+) <= (\d+)", out)
    assert m, out[-2000:]
    key, key_bound, prod, prod_bound = (int(g) for g in m.groups())
    assert key == key_bound == 2 * 32766 ** 2 < 2 ** 31 and prod == 16383 ** 2 <= prod_bound == 16383 * 32766 < 2 ** 30
    assert re.search(r"ok equivalence: %d combinations" % (4 * 4 * 24 ** 4), out)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "vor_paint_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_model_restates_are_the_header_s():
    hdr = open(os.path.join(CSRC, "vor_paint.hpp")).read()
    assert "kVorPaintTileW = %d, kVorPaintTileH = %d;" % (R.TW, R.TH) in hdr
    assert "kVorPaintCap = %d;" % R.CAP in hdr and "kVorPaintMaxK = %d;" % R.MAX_K in hdr and "kVorPaintIdBits = 12;" in hdr
    assert "kVorPaintCoordBound = 1u << 14;" in hdr and R.BOUND == 1 << 14
    assert "vp_keep_f(px, py, kx, ky, r) >= 0;" in hdr and "return kept <= kVorPaintCap;" in hdr
    kern = open(os.path.join(CSRC, "k_misc.hip")).read()
    for name in R.MARKS:
        assert '"%s"' % name in kern
    assert "vp_keep(" in kern and "vp_pivot_key(" in kern and "vp_tile_rect(" in kern and "vp_list_fits(" in kern
    codec = open(os.path.join(CSRC, "codec.cpp")).read()
    assert "vp_sides_small(*w, *h)" in codec and "vp_coord_small(cent[k].x, cent[k].y)" in codec


def _check_case(c, oracle=True):
    """the model paints what the brute force paints (and the oracle decodes); the case's route and counts are what it says -> (labels, pivots, kept)"""
    w, h, xs, ys = c["w"], c["h"], c["xs"], c["ys"]
    want = R.brute_labels(w, h, xs, ys)
    assert R.route(w, h, xs, ys) == c["route"], c["name"]
    if oracle:
        rc, img = O.decode("voronoi(1)", R.case_stream(c))
        assert rc == 0 and np.array_equal(img, R.image_of(want)), c["name"]
    if c["route"] == "brute":
        assert R.expected_marks(c) == (0, 1, 0)
        return want, None, None
    labels, pivots, kept = R.model(w, h, xs, ys)
    assert np.array_equal(labels, want), c["name"]
    if "kept" in c:
        assert kept == c["kept"], (c["name"], kept)
    if "overflow" in c:
        assert R.overflow_of(kept) == c["overflow"], (c["name"], kept)
    if "pivot" in c:
        assert pivots[c["pivot"][0]] == c["pivot"][1], (c["name"], pivots)
    assert R.expected_marks(c) == (1, 0, R.overflow_of(kept))
    return labels, pivots, kept


def test_corner_ties_tell_the_two_comparisons_apart():
    cases = R.corner_ties()
    assert len(cases) == 20
    for c in cases:
        w, h, xs, ys = c["w"], c["h"], c["xs"], c["ys"]
        labels, pivots, kept = _check_case(c)
        x, y, win, lose = c["tie"]
        P, C = c["pivot_id"], c["c_id"]
        d = [(int(xs[k]) - x) ** 2 + (int(ys[k]) - y) ** 2 for k in (0, 1)]
        assert d == [25, 25] and labels[y, x] == win == 0                              # a tie, and the lower id takes it
        tiles = R.tiles_of(w, h)
        t = next(i for i, (x0, x1, y0, y1) in enumerate(tiles) if x0 <= x <= x1 and y0 <= y <= y1)
        assert (x in tiles[t][:2]) and (y in tiles[t][2:])                             # a corner pixel of its tile
        pivot, keep, f = R.prune(tiles[t], xs, ys)
        assert pivot == P and int(f[C]) == 0 and bool(keep.all())                      # f of C is exactly 0: `>=` keeps it, `>` drops it
        strict = R.model(w, h, xs, ys, strict=True)[0]
        diff = np.argwhere(strict != labels)
        if C == win:
            assert diff.tolist() == [[y, x]] and strict[y, x] == P                     # the mutant differs in the tie pixel alone
        else:
            assert len(diff) == 0 and not R.prune(tiles[t], xs, ys, strict=True)[1][C]   # P has the lower id: C is dropped and the pixel is P's either way
    assert sum(c["c_id"] == 0 for c in cases) == 10


def test_list_cap_cases_sit_on_the_cap():
    cases = R.list_cap()
    assert [(len(c["xs"]), c.get("kept"), c["overflow"]) for c in cases] == [(255, [255], 0), (256, [256], 0), (257, [257], 1), (300, [256], 0), (301, [257], 1), (260, None, 1)]
    for c in cases:
        labels, pivots, kept = _check_case(c)
        if c["w"] == R.TW:
            assert len(set(zip(c["xs"].tolist(), c["ys"].tolist()))) == len(c["xs"])  # distinct sites: each wins its own pixel
    four = R.model(cases[5]["w"], cases[5]["h"], cases[5]["xs"], cases[5]["ys"])[2]
    assert len(four) == 4 and four[0] > R.CAP and max(four[1:]) <= 8, four
    # the mutant `n < cap` moves the 256-entry cases to brute force: the pixels stay, the mark moves from 0 to 1
    for c in (cases[1], cases[3]):
        lab, _, kept = R.model(c["w"], c["h"], c["xs"], c["ys"], cap_lt=True)
        assert np.array_equal(lab, R.brute_labels(c["w"], c["h"], c["xs"], c["ys"])) and R.overflow_of(kept, cap_lt=True) == 1 and R.overflow_of(kept) == 0


def test_k_limit_cases():
    cases = R.k_limits()
    assert [len(c["xs"]) for c in cases] == [1, 255, 256, 257, 4096, 4096, 4097, 4097]
    assert [c["route"] for c in cases] == ["tiles"] * 6 + ["brute"] * 2
    for c in cases:
        labels, pivots, kept = _check_case(c)
        K = len(c["xs"])
        sites = list(zip(c["xs"].tolist(), c["ys"].tolist()))
        if K > 1:
            assert len(set(sites)) < K                                                 # duplicated sites ...
            first = {}
            for k, s in enumerate(sites):
                first.setdefault(s, k)
            assert set(np.unique(labels).tolist()) <= set(first.values())              # ... and only the lowest id of a site paints
        if c["name"].endswith("dense") and kept is not None:
            assert R.overflow_of(kept) == 8 and len(kept) == 9 and kept[8] <= R.CAP   # 130 x 70: nine tiles, all but the 2 x 6 corner by brute force
        if c["name"].endswith("sparse") and kept is not None:
            assert 2 <= max(kept) <= R.CAP
        if K >= 4096:
            assert labels[15, 31] == K - 1                                             # the last id is alone on its pixel and wins it


def test_coordinate_switch_cases():
    cases = R.coordinate_switch()
    by = {c["name"]: c for c in cases}
    for v, r in ((R.BOUND - 1, "tiles"), (R.BOUND, "brute")):
        for axis in ("x", "y", "x and y"):
            assert by["%s = %d beside sites inside" % (axis, v)]["route"] == r and by["%s = %d, all centroids far" % (axis, v)]["route"] == r
    assert by["16384 x 1"]["route"] == by["1 x 16384"]["route"] == "tiles" and by["16385 x 1"]["route"] == by["1 x 16385"]["route"] == "brute"
    assert by["wrapping to a tie"]["route"] == "brute"
    for c in cases:
        labels, pivots, kept = _check_case(c)
        if "x 1" in c["name"] or "1 x" in c["name"]:
            flat = labels.reshape(-1)
            assert flat[0] in (0, 5) and flat[-1] in (1, 4)                            # centroids at both ends, each twice
    for axis in ("x", "y", "x and y"):
        far = by["%s = 16383, all centroids far" % axis]
        assert max(int(far["xs"].max()), int(far["ys"].max())) == R.BOUND - 1
        lab = R.brute_labels(70, 40, far["xs"], far["ys"])
        assert 2 not in lab and min(int((lab == 0).sum()), int((lab == 1).sum())) >= 30   # the two far centroids share the image
    tie = R.brute_labels(70, 40, by["wrapping to a tie"]["xs"], by["wrapping to a tie"]["ys"])
    assert set(np.unique(tie).tolist()) == {0, 1, 2} and tie[1, 3] == 0                # (10, 0) never paints: its twin modulo 2^32 has the lower id
    tie = R.brute_labels(70, 40, by["wrapping to a tie, the small ones first"]["xs"], by["wrapping to a tie, the small ones first"]["ys"])
    assert set(np.unique(tie).tolist()) == {0, 2} and tie[1, 3] == 0                   # ... and here neither twin does


def test_clipped_tile_cases():
    cases = R.clipped_tiles()
    assert [(c["w"], c["h"]) for c in cases[::2]] == list(R.CLIPPED_SIZES)
    for c in cases:
        labels, pivots, kept = _check_case(c)
        x0, x1, y0, y1 = R.tiles_of(c["w"], c["h"])[0]
        a, b = c["mirrored"]
        key = lambda k: (2 * int(c["xs"][k]) - x0 - x1) ** 2 + (2 * int(c["ys"][k]) - y0 - y1) ** 2
        assert key(a) == key(b)                                                        # mirrored about the first tile's centre: one pivot key
        if len(c["xs"]) == 2:
            assert pivots[0] == 0


def test_lattice_cases():
    for c in R.lattice_ties():
        labels, pivots, kept = _check_case(c)
        step = 2 if "spacing 2" in c["name"] else 4
        # many pixels are equidistant from 2 or 4 sites
        d = (c["xs"].astype(np.int64)[:, None, None] - np.arange(96)[None, None, :]) ** 2 + (c["ys"].astype(np.int64)[:, None, None] - np.arange(48)[None, :, None]) ** 2
        ties = (d == d.min(axis=0)).sum(axis=0)
        twice = 2 if "twice" in c["name"] else 1
        assert int((ties >= 2 * twice).sum()) > 1000 and int((ties >= 4 * twice).sum()) > (400 if step == 2 else 100)
        # (a lattice prunes badly: tile 0 keeps every site.)  Spacing 2: every tile by brute force; spacing 4: tiles of either kind
        assert (R.overflow_of(kept) == len(kept) == 4) if step == 2 else (0 < R.overflow_of(kept) < len(kept) == 4)


def test_sweep_reaches_both_routes_and_both_paths():
    cases = R.sweep()
    assert len(cases) == R.SWEEP_CASES == 200
    n_tiles = n_brute = listed = over = 0
    for c in cases:
        assert 1 <= c["w"] <= 200 and 1 <= c["h"] <= 200 and c["w"] * c["h"] < 20000 and 1 <= len(c["xs"]) <= 600
        labels, pivots, kept = _check_case(c, oracle=False)
        if c["route"] == "tiles":
            n_tiles += 1
            over += R.overflow_of(kept) > 0
            listed += R.overflow_of(kept) < len(kept)
        else:
            n_brute += 1
    print("sweep: %d tiles (%d with an overflowing tile, %d with a listed one), %d brute" % (n_tiles, over, listed, n_brute))
    assert n_tiles >= 100 and n_brute >= 20 and over >= 5 and listed >= 100


def test_destination_cases_are_a_corner_tie_and_two_cap_cases():
    d = R.destinations()
    assert "tie" in d[0] and d[1]["kept"] == [256] and d[2]["kept"] == [257]
