"""The `delta` encoder's symbol arithmetic (cniic_amd/csrc/delta_sym.hpp) and the case table of tests/test_delta_limits.py, without a GPU.
tests/delta_sym_check.cpp is compiled against the header as a stand-alone program and checks every way the kernels go between a
difference's three forms -- field word, cube index, key -- against plain signed integers over all 511^3 differences, every per-channel
pixel pair (borrows between the fields), the cube's faces and the extreme keys; the same program runs once more under
-fsanitize=address,undefined.  Then the table (delta_limits_ref.py): every case's cold count per 512-symbol chunk, computed from the
oracle's own difference stream, is the one the case declares, and the route it declares follows from those counts -- so that the GPU
test's cases are known to stand where they claim to before any of them runs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import delta_limits_ref as R
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "delta_sym_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "cniic_amd", "csrc")
PARTS = ("all_diffs", "borrows", "faces", "keys")


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


def test_every_route_between_fields_index_and_key_against_plain_integers(tmp_path):
    exe = str(tmp_path / "delta_sym_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-o", exe, SRC])
    out = _run(exe)
    assert "ok all_diffs: %d differences, 32768 inside the cube" % 511 ** 3 in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "delta_sym_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_checks_restate_are_the_library_s():
    """the program's page size and the table's chunk, side-array and fold numbers are written out a second time: they must still be the kernels'"""
    common = open(os.path.join(CSRC, "common.hpp")).read()
    kernel = open(os.path.join(CSRC, "k_delta.hip")).read()
    assert re.search(r"constexpr uint32_t kPageShift = 12;", common)
    assert re.search(r"kPageShiftHere = 12;", open(SRC).read())
    assert re.search(r"constexpr int kChunk16 = %d;" % R.CHUNK, kernel) and re.search(r"constexpr uint32_t kColdPerChunk = %d;" % R.COLD_MAX, kernel)
    assert kernel.count("crank >= %d" % R.FOLD_FROM) == 1 and kernel.count("total >= %d" % R.FOLD_FROM) == 1
    assert kernel.count("> kColdPerChunk) *overflow = 1") == 2


def test_image_from_diffs_plants_exactly_the_sequence():
    """squares and rectangles alike: the oracle's differences of the linearised image are the planted ones"""
    rng = np.random.default_rng(5)
    for w, h in [(64, 64), (100, 75), (700, 1), (8, 8), (3, 5)]:
        v = rng.integers(0, 256, (w * h, 3))
        d = np.diff(v, axis=0, prepend=0)
        img = R.image_from_diffs(w, h, d)
        assert img.shape == (h, w, 3)
        assert np.array_equal(O.unpack_signed(O.delta_diff(O.hilbert_linearize(img))), d)
    with pytest.raises(AssertionError):
        R.image_from_diffs(2, 1, [[250, 0, 0], [10, 0, 0]])
    assert R.cold_per_chunk(R.smooth_image(100, 75))[0].tolist() == [0] * 15


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_stands_where_it_claims_to(name):
    case = R.BY_NAME[name]
    got, distinct = R.cold_per_chunk(R.case_image(name))
    assert got.tolist() == R.declared_counts(case).tolist()
    assert got.size == R.nchunks(case.shape)
    if case.route == 16:
        assert got.max() <= R.COLD_MAX
    else:   # the overflow, not the alphabet, is what sends it to the 32-bit route
        assert case.route == 32 and got.max() >= R.COLD_MAX + 1 and distinct < 1 << 26


def test_the_table_reaches_what_it_is_there_for():
    """every count next to a switch point, in the tile gather (s64, s128) and in the per-position gather (r100, l700), in a first, a middle and the
    last chunk; the partial chunks; the straddles over a mid-wave reset, a wave border and a tile border; the keys"""
    at = {}
    for c in R.CASES:
        for ch, n in c.counts.items():
            at.setdefault((c.shape, n), set()).add(ch)
    for shape in ("s64", "s128", "r100", "l700"):
        for n in (R.FOLD_FROM - 1, R.FOLD_FROM, R.COLD_MAX - 1, R.COLD_MAX, R.COLD_MAX + 1):
            assert set(R.PLACES[shape]) <= at[(shape, n)], (shape, n)
    assert {(R.FOLD_FROM - 1), R.FOLD_FROM, R.COLD_MAX - 1, R.COLD_MAX} <= {n for (s, n) in at if s == "t8"}
    assert R.chunk_len("r100", 14) == 332 and R.chunk_len("l700", 1) == 188 and R.chunk_len("t8", 0) == 64
    straddles = {(c.shape, min(c.counts)) for c in R.CASES if "straddle" in c.name}
    assert {("s64", 2), ("s64", 3), ("s128", 7), ("r100", 13), ("l700", 0)} <= straddles
    assert all(sorted(c.counts.values()) == [32, 33] and c.route == 16 for c in R.CASES if "straddle" in c.name)
    # keys: the 54 face differences are cold by exactly one channel at -17 or 16; the extremes hold all eight sign patterns, key 0 and the largest
    assert len(set(R.FACES)) == 54 and all(sum(x in (-17, 16) for x in f) == 1 and all(x in (-17, -16, 0, 15, 16) for x in f) for f in R.FACES)
    assert {f for f in R.EXTREMES if 0 not in f} == {(a, b, c) for a in (-255, 255) for b in (-255, 255) for c in (-255, 255)}
    syms = O.delta_diff(O.hilbert_linearize(R.case_image("s64-extremes11")))
    assert syms.min() == 0 and syms.max() == (510 << 18 | 510 << 9 | 510)
    for name, distinct_cold in (("s64-count64-first", 1), ("s64-count64-middle", 64), ("r100-count65-middle", 65), ("s128-packed64", 2)):
        syms = O.delta_diff(O.hilbert_linearize(R.case_image(name)))
        assert np.unique(syms[R.is_cold(O.unpack_signed(syms))]).size == distinct_cold, name
    assert sum(c.route == 32 for c in R.CASES) >= 16
