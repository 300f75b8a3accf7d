"""The arithmetic of the small-frame cluster-colors kernel (cniic_amd/csrc/cc_small.hpp) and what tests/test_cc_small_batch.py relies on,
without a GPU.  tests/cc_small_check.cpp is compiled against the header as a stand-alone program: a scalar K-means built from the
header's functions runs beside a plain 64-bit restatement of kmeans::cluster on random point lists, ties (stay / lowest index), equal
points, weights up to 16 384, K = 1, 2, 255, 256 and U = K, K + 1, 2K - 1, K - 1; the same program runs once more under
-fsanitize=address,undefined.  Then, from the oracle alone: the reseed fixtures still reseed when they arrive as one-row images under
cluster-colors(K), rgbw_few stopped after two iterations answers FEW_ACTIVE, and the shaped frames of the GPU test succeed and fail
where that test says they do."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cc_small_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "cniic_amd", "csrc")
PARTS = ("random", "ties", "all_equal", "weights", "limits", "total")
G = np.load(os.path.join(HERE, "golden", "reseed_golden.npz"))
RGBW = ["rgbw38", "rgbw621", "rgbw1268", "rgbw2355"]


def image_of(keys, weight):
    """an image whose distinct colours are `keys` with pixel counts `weight` (one row)"""
    k = np.repeat(keys, weight.astype(np.int64))
    np.random.default_rng(1).shuffle(k)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], 1).astype(np.uint8).reshape(1, -1, 3)


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


def test_header_kmeans_against_the_plain_restatement(tmp_path):
    exe = str(tmp_path / "cc_small_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    assert "largest sum %d < 2^32" % (255 * 16384) in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "cc_small_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_cc_small_batch as T
    hdr = open(os.path.join(CSRC, "cc_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kCcSmallMaxPx = %d;" % T.MAX_PX, hdr)
    assert re.search(r"kCcSmallDefaultSeed = 0x%X" % O.DEFAULT_SEED, hdr)
    assert "%d pixels" % T.MAX_PX in re.sub(r"(\d) (\d)", r"\1\2", open(os.path.join(os.path.dirname(HERE), "include", "cniic_hip.h")).read())


def test_reseed_fixtures_as_one_row_images_still_reseed():
    for name in RGBW:
        K = int(G[name + "_K"][0])
        img = image_of(G[name + "_keys"], G[name + "_weight"]).copy()
        assert img.shape[0] * img.shape[1] <= 16384
        rc, data, st = O.encode("cluster-colors(%d)" % K, img, mode=O.MODE_L)
        assert rc == 0 and st["empty_reseeds"] >= 2, (name, rc, st)


def test_rgbw_few_stopped_after_two_iterations_has_too_few_active_clusters():
    K, mi = int(G["rgbw_few_K"][0]), int(G["rgbw_few_max_iters"][0])
    assert mi == 2
    img = image_of(G["rgbw_few_keys"], G["rgbw_few_weight"]).copy()
    assert img.shape[0] * img.shape[1] <= 16384
    px = img.reshape(-1, 3).astype(np.uint32)
    keys, weight = np.unique(px[:, 0] << 16 | px[:, 1] << 8 | px[:, 2], return_counts=True)      # the point list the codec builds
    assert np.array_equal(keys, G["rgbw_few_keys"]) and np.array_equal(weight, G["rgbw_few_weight"])
    pts = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=1).astype(np.int32)
    rc, r = O.kmeans(O.PT_RGBW, O.MODE_L, pts, weight.astype(np.uint32), K, max_iters=mi)
    assert rc == O.FEW_ACTIVE and np.array_equal(r["members"], G["rgbw_few_members"])


def test_shaped_frames_succeed_and_fail_where_the_gpu_test_says():
    import test_cc_small_batch as T
    imgs = T.shaped_images()
    assert [im.shape[:2] for im in imgs] == [(h, w) for w, h in T.SHAPES]
    distinct = [len(np.unique(im.reshape(-1, 3), axis=0)) for im in imgs]
    assert sum(d >= 256 for d in distinct) >= 6 and all(d >= 256 for d in distinct[4:])
    rcs = [O.encode("cluster-colors(16)", im, mode=O.MODE_L)[0] for im in imgs if im.shape[0] * im.shape[1] <= T.ORACLE_MAX_PX]
    assert sum(r == 0 for r in rcs) >= len(rcs) - 3 and rcs[:3] == [O.TOO_FEW_POINTS] * 3 and all(r == 0 for r in rcs[3:])
    further = T.further_images()
    assert [len(np.unique(im.reshape(-1, 3), axis=0)) for im in further] == [1, 2, 256, 64]
    assert T.routed(imgs) == [True] * 8 + [False] * 2
