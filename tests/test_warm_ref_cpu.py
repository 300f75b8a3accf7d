"""CPU side of K-means from given centroids and of a palette's fit: the yardstick the GPU tests hold the kernels against
(tests/warm_ref.py) is the oracle's own run when it starts from the oracle's own init centroids, and the new entry points are where
the header and the loader say they are."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import warm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cniic_kmeans_rgbw_from", "cniic_kmeans_xyrgb_from", "cniic_cc_set_centroids", "cniic_codec_encode_warm", "cniic_palette_fit_frames_var"]


def photo(w, h, seed):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + seed)


def same_run(ref, exp):
    assert np.array_equal(ref["centroids"], exp["centroids"])
    assert np.array_equal(ref["labels"], exp["labels"])
    assert np.array_equal(ref["members"], exp["members"])
    assert ref["iterations"] == exp["stats"]["iterations"]
    assert ref["empty_reseeds"] == exp["stats"]["empty_reseeds"]
    assert ref["moved_last"] == exp["stats"]["moved_last"]


@pytest.mark.parametrize("K,max_iters", [(1, 0), (7, 0), (16, 0), (16, 2), (40, 0)])
def test_lloyd_from_the_reference_init_is_the_oracles_run_rgbw(K, max_iters):
    keys, w = R.colour_points(photo(40, 30, 3))
    pts = R.pts_of_keys(keys)
    rco, exp = O.kmeans(O.PT_RGBW, O.MODE_L, pts, w, K, max_iters=max_iters)
    rc, ref = R.lloyd_from(O.PT_RGBW, pts, w, K, R.ref_init_centroids(pts, K), max_iters=max_iters)
    assert rc == rco and rc in (O.OK, O.FEW_ACTIVE)
    same_run(ref, exp)


def test_lloyd_from_reports_too_few_active_clusters():
    """check_enough_active_clusters (kmeans.rs:41-57, kmeans.c:428-434) on the members of the last step: from the reference's own init every
    cluster keeps at least its head, so the case is made with entries nobody prefers -- 3 of 16 white on an image below 128, one capped
    iteration: 13 active clusters against the 15 that 0.99 K asks for.  The results are there all the same."""
    keys, w = R.colour_points(photo(40, 30, 3) >> 1)
    pts = R.pts_of_keys(keys)
    K = 16
    init = R.ref_init_centroids(pts, K)
    init[[2, 7, 11]] = (255, 255, 255)
    rc, ref = R.lloyd_from(O.PT_RGBW, pts, w, K, init, max_iters=1)
    assert rc == O.FEW_ACTIVE and ref["rc"] == rc and ref["active"] == 13 and ref["empty_reseeds"] == 3
    assert int(ref["members"].sum()) == pts.shape[0] and [int(ref["members"][k]) for k in (2, 7, 11)] == [0, 0, 0]
    rc, ref = R.lloyd_from(O.PT_RGBW, pts, w, K, init)
    assert rc == O.OK and ref["active"] >= 15


@pytest.mark.parametrize("K,max_iters", [(1, 0), (5, 0), (12, 0), (12, 3)])
def test_lloyd_from_the_reference_init_is_the_oracles_run_xyrgb(K, max_iters):
    pts = R.xy_pts(photo(23, 17, 4))
    rco, exp = O.kmeans(O.PT_XYRGB, O.MODE_L, pts, None, K, max_iters=max_iters)
    rc, ref = R.lloyd_from(O.PT_XYRGB, pts, None, K, R.ref_init_centroids(pts, K), max_iters=max_iters)
    assert rc == rco and rc in (O.OK, O.FEW_ACTIVE)
    same_run(ref, exp)


def test_lloyd_from_reseeds_with_the_oracles_iteration_number():
    """an init centroid no point prefers is reseeded in iteration 0, from reseed_index(seed, 0, k, n) -- the count before the increment"""
    img = photo(24, 24, 5) >> 1                     # every channel below 128
    keys, w = R.colour_points(img)
    pts = R.pts_of_keys(keys)
    K = 4
    init = R.ref_init_centroids(pts, K)
    init[2] = (255, 255, 255)
    rc, one = R.lloyd_from(O.PT_RGBW, pts, w, K, init, max_iters=1)
    assert rc in (O.OK, O.FEW_ACTIVE) and one["empty_reseeds"] == 1
    assert np.array_equal(one["centroids"][2], pts[O.reseed_index(O.DEFAULT_SEED, 0, 2, pts.shape[0])])


def test_too_few_points():
    pts = R.pts_of_keys(np.arange(3, dtype=np.uint32))
    assert R.lloyd_from(O.PT_RGBW, pts, np.ones(3, np.uint32), 4, np.zeros((4, 3)))[0] == O.TOO_FEW_POINTS


def test_fit_reference_on_a_palette_with_equal_entries():
    cent = np.array([[0, 0, 0], [10, 0, 0], [0, 0, 0], [255, 255, 255]])
    frame = np.array([[[0, 0, 0], [5, 0, 0], [6, 0, 0], [250, 255, 255]]], np.uint8)
    sse, pixels = R.fit(cent, [frame])
    assert list(sse) == [0 + 25 + 16 + 25] and list(pixels) == [2, 1, 0, 1]    # 5 is as far from 0 as from 10: the lower index; entry 2 is shadowed


def test_the_new_symbols_are_declared_listed_and_exported():
    from cniic_amd import _lib
    text = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared in include/cniic_hip.h" % name
        assert name in _lib.SYMBOLS
    for so in ("libcniic_hip.so", "libcniic_hip_testing.so"):
        L = C.CDLL(os.path.join(ROOT, "cniic_amd", so))
        for name in NEW:
            assert hasattr(L, name), "%s does not export %s" % (so, name)
    assert "THE DEFINITION" in text and "need not stop after one iteration" in text and "bit for bit" in text
