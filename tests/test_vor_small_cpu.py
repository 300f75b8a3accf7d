"""The arithmetic of the small-frame voronoi kernels (cniic_amd/csrc/vor_small.hpp) and what tests/test_vor_small_batch.py and
tests/test_vor_small_decode.py rely on, without a GPU.  tests/vor_small_check.cpp is compiled against the header as a stand-alone program:
a scalar K-means built from the header's functions, with the stay test on and with it off, runs beside a plain 64-bit restatement of
kmeans::cluster over ColorPos points on random frames, flat frames (every distance a tie), duplicate centroids, K = 1, 2, 255, 256 with
n = K - 1, K, K + 1, 2K - 1, and 16384 x 1 and 1 x 16384; then the stay test alone against brute force, the stream's layout and the
decoder's wrapping squares.  The same program runs once more under -fsanitize=address,undefined.  Then, from the oracle alone (mode L):
the shaped frames of the GPU test succeed and fail where that test says they do, the checkerboard reseeds and stopped after two iterations
answers FEW_ACTIVE, and the 15 x 15 noise frame reseeds once."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vor_small_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "cniic_amd", "csrc")
PARTS = ("random", "flat", "duplicates", "limits", "long", "stay", "layout", "total")


def points_of(img):
    """the ColorPos points of an image, row-major: (x, y, r, g, b)"""
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    return np.concatenate([xx.reshape(-1, 1), yy.reshape(-1, 1), img.reshape(-1, 3)], axis=1).astype(np.int32)


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
    exe = str(tmp_path / "vor_small_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    m = re.search(r"largest distance (\d+) <= (\d+), largest sum (\d+) <= (\d+)", out)
    assert m, out[-2000:]
    dist, dist_bound, sums, sum_bound = (int(g) for g in m.groups())
    assert dist_bound == 16383 ** 2 + 3 * 255 ** 2 < 2 ** 29 and sum_bound == 16383 * 16384 < 2 ** 28
    assert dist == dist_bound and sums == 16383 * 16384 // 2       # the two ends of a 16384-pixel row, black and white; the whole row in one cluster


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "vor_small_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_vor_small_batch as T
    import test_vor_small_decode as D
    hdr = open(os.path.join(CSRC, "vor_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kVorSmallMaxPx = %d;" % T.MAX_PX, hdr) and T.MAX_PX == D.MAX_PX
    assert re.search(r"constexpr uint32_t kVorSmallMaxK = %d;" % D.MAX_K, hdr)
    assert re.search(r"kVorSmallDefaultSeed = 0x%X" % O.DEFAULT_SEED, hdr)
    assert "return 16u + 19u * K;" in hdr and T.stream_len(256) == D.stream_len(256) == 16 + 19 * 256
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "kVorSmallFloorFew = %d, kVorSmallFloorMany = %d;" % (T.FLOOR_FEW, T.FLOOR_MANY) in capi
    assert "kVorSmallFloorWorkFew = %d, kVorSmallFloorWorkSome = %d;" % (T.FLOOR_WORK_FEW, T.FLOOR_WORK_SOME) in capi
    api = re.sub(r"(\d) (\d)", r"\1\2", open(os.path.join(os.path.dirname(HERE), "include", "cniic_hip.h")).read())
    assert "SMALL `voronoi` frames" in api and api.count("SMALL `voronoi` frames") == 2 and "%d pixels" % T.MAX_PX in api


def test_shaped_frames_succeed_and_fail_where_the_gpu_test_says():
    import test_vor_small_batch as T
    imgs = T.shaped_images()
    assert [im.shape[:2] for im in imgs] == [(h, w) for w, h in T.SHAPES]
    assert T.routed(imgs) == [w * h <= T.MAX_PX for w, h in T.SHAPES] and sum(T.routed(imgs)) == len(imgs) - 2
    res = [O.encode("voronoi(16)", im, mode=O.MODE_L) for im in imgs]
    assert [r[0] for r in res] == [O.TOO_FEW_POINTS] * 3 + [0] * (len(imgs) - 3)
    its = [r[2]["iterations"] for r in res[3:]]
    assert all(len(r[1]) == T.stream_len(16) for r in res[3:])
    assert min(its) == 4 and max(its) == 213, its     # short runs and long ones
    assert [O.encode("voronoi(256)", im, mode=O.MODE_L)[0] for im in imgs[:4]] == [O.TOO_FEW_POINTS] * 4
    assert all(im.shape[0] * im.shape[1] >= 256 for im in imgs[4:])


def test_the_checkerboard_reseeds_and_stopped_after_two_iterations_has_too_few_active_clusters():
    import test_vor_small_batch as T
    board = T.further_images()[1]
    assert board.shape == (12, 23, 3)
    rc, data, st = O.encode("voronoi(128)", board, mode=O.MODE_L)
    assert rc == 0 and len(data) == T.stream_len(128)
    assert st["empty_reseeds"] == 149 and st["iterations"] == 7, st
    rc, r = O.kmeans(O.PT_XYRGB, O.MODE_L, points_of(board), None, 128, max_iters=2)
    assert rc == O.FEW_ACTIVE and r["stats"]["iterations"] == 2 and int((r["members"] > 0).sum()) == 12


def test_the_noise_frame_reseeds():
    import test_vor_small_batch as T
    noise = T.further_images()[2]
    assert noise.shape == (15, 15, 3)
    rc, data, st = O.encode("voronoi(100)", noise, mode=O.MODE_L)
    assert rc == 0 and st["empty_reseeds"] == 1, st
