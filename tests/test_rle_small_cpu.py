"""What the small-frame `hilbert(rle)` / `hilbert(rle(d))` kernel computes per frame (cniic_amd/csrc/rle_small.hpp) and what
tests/test_rle_small_batch.py relies on, without a GPU.  tests/rle_small_check.cpp is compiled against the header as a stand-alone
program: a scalar encoder built from the header's functions in the kernel's phases (the lengths of all starts, the chain in pieces, the
records) runs beside a plain one-pass restatement with a real sqrt and f64 sums on random pixel lists, the content kinds of the GPU test
and every d, with T(d) checked against sqrt next to the exact distances of small integer triples and the rounding against f64::round for
every (sum, count); the same program runs once more under -fsanitize=address,undefined.  Then, from the CPU restatements alone: every
frame of the GPU test has the property and the run count that test claims, and the cross-compiled kernel has no scratch segment."""
import math
import os
import re
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rle_small_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
PARTS = ("random", "contents", "threshold", "rounding", "total")


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


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "rle_small.hpp"\nint main() { return cniic::rs_stride(cniic::kRleSmallMaxPx) == 196624 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.call([exe]) == 0


def test_header_encoder_against_the_plain_restatement(tmp_path):
    import test_rle_small_batch as T
    exe = str(tmp_path / "rle_small_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    assert "ok total: bound %d pixels, stride at the bound %d, piece %d, 0 mismatches" % (T.MAX_PX, T.STRIDE_AT_BOUND, T.PIECE) in out
    assert "flat 16384 = 64 runs of 255 and one of 64" in out
    assert "ok rounding: %d (sum, count) pairs" % sum(255 * c + 1 for c in range(1, 256)) in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "rle_small_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_rle_small_batch as T
    hdr = open(os.path.join(CSRC, "rle_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kRleSmallMaxPx = %d;" % T.MAX_PX, hdr)
    assert re.search(r"constexpr uint32_t kRleSmallMaxRun = %d;" % T.MAX_RUN, hdr)
    assert re.search(r"constexpr uint32_t kRleSmallPiece = %d;" % T.PIECE, hdr)
    assert "CNIIC_RS_HD uint64_t rs_stride(uint64_t n) { return (8 + 12 * n + 15) & ~15ull; }" in hdr
    assert T.STRIDE_AT_BOUND == (8 + 12 * T.MAX_PX + 15) // 16 * 16 == 196624
    kern = open(os.path.join(CSRC, "k_rle_small.hip")).read()
    assert re.search(r"constexpr int kRsThreads = %d;" % T.THREADS, kern) and "void k_rle_small(" in kern
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    assert "return rs_stride(npx) + sizeof(RleSmallRow) + sizeof(RleSmallResult); }" in src
    assert '"%s"' % T.TIMER in src and '"%s"' % T.PLACE in src
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert 'small_route_max_px("%s", "%s", kRleSmallMaxPx)' % (T.KNOB_OFF, T.KNOB_MAX_PX) in capi and 'test_env("%s")' % T.KNOB_FLOOR_OFF in capi
    assert re.search(r"constexpr uint32_t kRleSmallFloorNone = %d;" % T.FLOOR_NONE, capi) and re.search(r"constexpr uint32_t kRleSmallFloorFew = %d;" % T.FLOOR_FRAMES, capi) and re.search(r"constexpr uint64_t kRleSmallFloorPxFew = %d;" % T.FLOOR_PX, capi)
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    assert T.TIMER in api and T.PLACE in api
    # the large encoder takes the accept test, the threshold and the modes from the header
    big = open(os.path.join(CSRC, "k_rle_approx.hip")).read()
    assert '#include "rle_small.hpp"' in big and "bool rla_accept(" not in big and "bool rla_accept(" in hdr


def test_the_frames_at_the_bound_are_what_the_gpu_test_claims():
    import test_rle_small_batch as T
    frames = T.bound_frames()
    assert len(frames) == 6 + len(T.ODD_AT) and T.ODD_AT == [0, 1, 253, 254, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025]
    for d in T.D_BIG:
        claims = T.bound_claims(frames, d)
        by_name = dict(zip([name for name, _ in frames], claims))
        assert all(ln == 8 + 12 * runs for runs, ln in claims)
        if d in (0.0, 4.0):
            assert by_name["flat"] == (65, 788) and by_name["odd at 0"] == (66, 800) and by_name["odd at 255"] == (66, 800) and by_name["odd at 1"] == (67, 812)
        if d == 0.0:
            assert by_name["noise"] == by_name["alternating"] == (T.MAX_PX, 8 + 12 * T.MAX_PX)
        if not d >= 0.0:
            assert set(claims) == {(T.MAX_PX, 8 + 12 * T.MAX_PX)}
        if d >= 441.7:
            assert set(claims) == {(65, 788)}


def test_the_frames_under_every_d_are_what_the_gpu_test_claims():
    import test_rle_small_batch as T
    imgs = T.full_d_frames()
    assert len(T.D_ALL) == 15 and sum(1 for d in T.D_ALL if d == 0.0) == 2 and sum(1 for d in T.D_ALL if d != d) == 1
    for d in T.D_ALL:
        ramp, odd = T.restated(imgs[3], d), T.restated(imgs[5], d)
        assert T.counts(ramp) == ([T.MAX_RUN] * 29 + [105] if d >= math.sqrt(3.0) else [1] * 7500), d
        if 0.0 <= d < 100.0:
            assert T.counts(odd)[:2] == [T.MAX_RUN, 1] and T.records(odd)[1][2] == T.B, d
    # the exact codec's restatement and the running-average one agree where they must: d tiny
    for im in imgs:
        assert T.restated(im, 0.0)[8:] == T.restated(im, 1e-9)[8:]
    assert [T.expr_of(d) for d in (0.0, -0.0, 4.0, math.inf, math.nan)] == ["hilbert(rle)", "hilbert(rle(-0.0))", "hilbert(rle(4.0))", "hilbert(rle(inf))", "hilbert(rle(nan))"]


def test_shapes_and_machinery_frames_are_what_the_gpu_test_says():
    import test_rle_small_batch as T
    names, imgs = zip(*T.shaped())
    px = [im.shape[0] * im.shape[1] for im in imgs]
    assert px[:2] == [1, 2] and px[2:2 + 2 * len(T.ROWS)] == [n for n in T.ROWS for _ in range(2)] and px[-2:] == [16385, 19200]
    assert [im.shape[:2] for im in imgs[2:6]] == [(1, 254), (254, 1), (1, 255), (255, 1)]
    assert sum(T.routed(imgs)) == len(imgs) - 2
    # a flat row of 255 is one full run, of 256 a full run and one pixel; the odd pixel at the end of 257 is a run of its own
    flat255 = [im for nm, im in zip(names, imgs) if nm in ("255x1", "1x255") and len(np.unique(im)) == 1]
    assert all(T.counts(T.restated(im, 4.0)) == [255] for im in flat255)
    mach = T.machinery_frames()
    mpx = [im.shape[0] * im.shape[1] for im in mach]
    assert mpx == [4096, 1517, 1024, 1025, 7500, 1, 16384, 63, 12288, 16385, 19200] and sum(T.routed(mach, 1024)) == 3
    assert T.counts(T.restated(mach[2], 4.0)) == [255] * 4 + [4] and T.counts(T.restated(mach[3], 0.0))[:3] == [255, 1, 1]
    assert T.counts(T.restated(mach[6], 4.0)) == [1] * 16384
    kinds = T.placement_kinds()
    assert [len(T.restated(im, 0.0)) for im in kinds] == [8 + 12 * r for r in range(1, 8)]
    many = T.many()
    assert len(many) == 3000 and len({im.shape[:2] for im in many}) == 8 and max(im.shape[0] * im.shape[1] for im in many) == 192
    assert any(len(T.restated(im, 8.0)) < len(T.restated(im, 0.0)) for im in many[:16])


def test_the_kernel_has_no_scratch_segment_and_fits_one_cu():
    kern = os.path.join(CSRC, "k_rle_small.hip")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), kern, "k_rle_small"], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "k_rle_small" in ln]
    assert len(lines) == 1, out
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
    assert field("VGPRs") <= 128   # 1024 threads a block
    # the static part from the code object, the dynamic part at the bound from the kernel's own rule: 8 bytes a pixel
    assert "return std::max(cap_px, kRsMinCap) * 8; }" in open(kern).read()
    assert field("LDS Size [bytes/block]") + 8 * 16384 <= 160 * 1024
