"""The integer arithmetic of the tiled 5-D K-means (cniic_amd/csrc/xy_bounds.hpp), without a GPU: tests/xy_bounds_check.cpp is compiled against
the header as a stand-alone program -- its 24-bit multiply returns on the host what v_mul_i32_i24 returns -- and checks xy_div_floor against
64-bit division over every sum the kernel can form (with the reciprocal nudged an ulp either way), and Dominance::worst / centre_dist against
64-bit arithmetic over the corners of a million boxes with coordinates at 0, 1, 16382, 16383.  The same program runs once more under
-fsanitize=address,undefined.  Also here: the precondition counts of tests/test_xyrgb_limits.py's capacity cases (xy_bounds_ref.py) and the
figures of xy_create's LDS budget that its K = 2656 / 2657 pair rests on."""
import os
import shutil
import subprocess

import pytest

import xy_bounds_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "xy_bounds_check.cpp")
PARTS = ("mul24", "div_floor", "worst", "centre_dist")


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


def test_div_floor_and_the_box_bound_against_64_bit_arithmetic(tmp_path):
    exe = str(tmp_path / "xy_bounds_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-o", exe, SRC])
    _run(exe)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "xy_bounds_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)


@pytest.mark.parametrize("w,h,K,max_iters,s_least,s_most,t_least", R.CAPACITY_CASES)
def test_capacity_cases_cross_what_they_are_there_to_cross(w, h, K, max_iters, s_least, s_most, t_least):
    got = R.capacity_precondition(R.case_image(w, h, K), K, s_least, s_most, t_least)
    # the counts the cases were chosen by (NOTES.md); a change of synth.photo or of the model shows here first
    assert got == {(256, 2048): (2048, 1495), (520, 1100): (993, 578), (128, 4096): (4096, 3849)}[(w, K)]


def test_the_lds_budget_puts_the_table_boundary_at_2656():
    assert R.lds_plan(2656) == (True, 64, 153 * 1024)          # exactly the budget
    assert R.lds_plan(2657)[:2] == (False, 192) and R.lds_plan(4096)[:2] == (False, 64)
    assert R.lds_plan(2048)[:2] == (True, 128) and R.lds_plan(1100)[:2] == (True, 256)
    assert all(R.lds_plan(K)[2] <= 153 * 1024 and R.lds_plan(K)[1] >= 64 for K in range(1, 4097))
