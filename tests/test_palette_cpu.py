"""The box-distance arithmetic behind the frozen-palette table (cniic_amd/csrc/pal_bounds.hpp), without a GPU: tests/palette_bounds_check.cpp is
compiled against the header as a stand-alone program and checks, for palettes of K = 1, 2, 16 and 256 (random; all entries equal; pairs mirrored
about a cell face; entries on cell corners; one tight cluster far from most cells), that the true lowest-index nearest entry of every one of the
2^24 colours is in its cell's candidate set, and that the candidate set's own lowest-index nearest is that entry.  The same program runs once
more as a host build under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "palette_bounds_check.cpp")
CASES = 5 * 4   # palette kinds x K


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert len(ok) == CASES and "FAIL" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def test_every_colours_nearest_entry_is_a_candidate_of_its_cell(tmp_path):
    exe = str(tmp_path / "palette_bounds_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-pthread", "-o", exe, SRC])
    out = _run(exe)
    # the budget is not vacuous: a random palette of 256 entries leaves a cell a handful of candidates, a palette of equal entries all of them
    rows = {(ln.split()[1], ln.split()[2]): float(ln.split(",")[1].split()[0]) for ln in out.splitlines() if ln.startswith("ok ")}
    assert rows[("random", "K=256:")] < 64 and rows[("equal", "K=256:")] == 256.0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "palette_bounds_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)
