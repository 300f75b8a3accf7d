"""The chunk boundaries of the persistent colour K-means without a search (cniic_amd/csrc/ps_bounds.hpp), without a GPU:
tests/ps_bounds_check.cpp is compiled against the header alone and run -- every cell names the boundaries that fall between its cost
prefix and the next, and the result is k_ps_ranges' bisection word for word, every boundary 0 .. NC written exactly once.  Inputs: random
cost arrays and hand-built ones (M = 1, M < NC, M = 32 768, one cell carrying nearly all the cost, G = 1, 3 and 256, totals near 2^32).
The same program again under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ps_bounds_check.cpp")
PARTS = ("hand-built", "random")


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln.split(" ", 1)[1] for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert tuple(ok) == PARTS and "FAIL" not in r.stdout, r.stdout[-4000:]


def test_the_direct_rule_gives_the_bisections_boundaries_each_written_once(tmp_path):
    exe = str(tmp_path / "ps_bounds_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC])
    _run(exe)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "ps_bounds_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    _run(exe)
