"""What the small-frame `zip(dict)` kernel computes per frame (cniic_amd/csrc/zd_small.hpp) and what tests/test_zd_small_batch.py relies
on, without a GPU.  tests/zd_small_check.cpp is compiled against the header as a stand-alone program: the header's functions as a scalar
emulation of the kernel's three phases (W lanes that speculate, the commit with 64 lanes over the window's list, the flush in shuffled
orders) beside a one-pass coder written without the header, on the frames of the GPU test and on random frames, for W in {1, 2, 64, 256},
with both caps lowered and with the symbol limit lowered to 0x104, 0x140 and 0x1000; the same program runs once more under
-fsanitize=address,undefined.  The restated streams and texts it writes out are held against tests/zip_dict_ref.py here.  Then, from
zip_dict_ref alone: every claim the GPU test makes about a frame, and the cross-compiled kernel has no scratch segment."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

import zip_dict_ref as Z

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "zd_small_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
PARTS = ("text", "windows", "caps", "freeze", "total")


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln.split()[1].rstrip(":") for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert tuple(ok) == PARTS and "FAIL" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def _gpu_test_frames(max_px):
    """the frames of the GPU test of at most max_px pixels (each content and size once)"""
    import test_zd_small_batch as T
    imgs = [im for _, im in T.shaped()] + [im for _, im in T.cap_frames()] + T.machinery_frames() + T.placement_kinds() + T.many()[:16]
    seen, out = set(), []
    for im in imgs:
        key = (im.shape, im.tobytes())
        if im.shape[0] * im.shape[1] <= max_px and key not in seen:
            seen.add(key)
            out.append(im)
    return out


def _write_frames(path, imgs):
    with open(path, "wb") as fp:
        fp.write(struct.pack("<I", len(imgs)))
        for im in imgs:
            fp.write(struct.pack("<II", im.shape[1], im.shape[0]))
            fp.write(np.ascontiguousarray(im, np.uint8).tobytes())


def _fnv(data):
    h = 0xcbf29ce484222325
    for b in np.frombuffer(data, np.uint8).tolist():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "zd_small.hpp"\nint main() { return cniic::zs_stride(cniic::zs_text_len(cniic::kZdSmallMaxPx)) == 360480 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.call([exe]) == 0


def test_header_emulation_against_the_plain_restatement_and_zip_dict_ref(tmp_path):
    import test_zd_small_batch as T
    exe = str(tmp_path / "zd_small_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, SRC])
    imgs = _gpu_test_frames(T.MAX_PX)
    assert len(imgs) >= 4 * len(T.SIZES) and max(im.shape[0] * im.shape[1] for im in imgs) == T.MAX_PX
    frames, streams = str(tmp_path / "frames.bin"), str(tmp_path / "streams.bin")
    _write_frames(frames, imgs)
    out = _run(exe, frames, streams)
    assert "ok total: bound %d pixels, window %d, caps %d %d, stride at the bound %d, table bits at the bound %d, 0 mismatches" % (
        T.MAX_PX, T.WINDOW, T.SPEC_CAP, T.GIVE_UP, T.STRIDE_AT_BOUND, T.TABLE_BITS_AT_BOUND) in out
    # the program's own restatement says what zip_dict_ref says: the text byte for byte (by hash), the stream byte for byte
    blob = open(streams, "rb").read()
    at = 0
    for k, im in enumerate(imgs):
        h, ln = struct.unpack_from("<QI", blob, at)
        at += 12
        if im.shape[0] * im.shape[1] <= 4096:
            assert h == _fnv(Z.zip_text(im)), k
        assert blob[at:at + ln] == T.restated(im), k
        at += ln
    assert at == len(blob)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "zd_small_check_san")
    subprocess.check_call([_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    frames = str(tmp_path / "frames.bin")
    _write_frames(frames, _gpu_test_frames(4096))
    _run(exe, frames)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_zd_small_batch as T
    hdr = open(os.path.join(CSRC, "zd_small.hpp")).read()
    for name, val in (("kZdSmallMaxPx", T.MAX_PX), ("kZsWindow", T.WINDOW), ("kZsSpecCap", T.SPEC_CAP), ("kZsGiveUp", T.GIVE_UP)):
        assert re.search(r"constexpr uint32_t %s = %d;" % (name, val), hdr), name
    assert T.frame_bytes(T.MAX_PX) == T.STRIDE_AT_BOUND + (8 << T.TABLE_BITS_AT_BOUND) + 32
    kern = open(os.path.join(CSRC, "k_zd_small.hip")).read()
    assert "constexpr int kZsThreads = kZsWindow;" in kern and "void k_zd_small(" in kern
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    assert "return zs_stride(N) + (8ull << zs_table_bits(N)) + sizeof(ZdSmallRow) + sizeof(ZdSmallResult);" in src
    assert 'test_env("%s")' % T.KNOB_CAP in src
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert 'small_route_max_px("%s", "%s", kZdSmallMaxPx)' % (T.KNOB_OFF, T.KNOB_MAX_PX) in capi and 'test_env("%s")' % T.KNOB_FLOOR_OFF in capi
    assert re.search(r"constexpr uint32_t kZdSmallFloorFrames = %d;" % T.FLOOR_FRAMES, capi) and re.search(r"constexpr uint64_t kZdSmallFloorPx = %d;" % T.FLOOR_PX, capi)
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    for name in (T.TIMER, T.PLACE, T.HANDBACK, T.FINISHED):
        assert '"%s"' % name in src and name in api, name


def test_the_shaped_frames_are_what_the_gpu_test_claims():
    import test_zd_small_batch as T
    by = {nm: T.restated(im, "cpu " + nm) for nm, im in T.shaped()}
    # the small ones through the Python coder too
    for nm, im in T.shaped():
        if im.shape[0] * im.shape[1] <= 1024:
            assert Z.codec_encode(Z.encode_py, im) == by[nm], nm
    for nm in ("photo 5x1", "photo 13x5", "photo 32x32", "noise 2x1", "noise 8x8", "flat 7x3", "flat 8x8", "flat 32x32"):
        assert T.ends_in_eof(by[nm]), nm
    for nm in ("photo 1x1", "photo 8x8", "photo 64x64"):
        assert not T.ends_in_eof(by[nm]), nm
    assert len(Z.zip_text(Z.photo_like(1, 1))) == 19 and len(by["photo 1x1"]) == 4 * 7
    # a flat frame's longest entry, and every content's side of the cap
    lib = T._CLIB[0]
    for (w, h), longest in T.FLAT_LONGEST.items():
        info = {}
        Z.encode_c(lib, Z.zip_text(Z.flat(w, h)), info)
        assert info["longest"] == longest and info["fill_end"] is None, (w, h)
    back = {nm: T.handed_back(s) for nm, s in by.items()}
    assert not back["flat 8x8"] and T.longest_match(by["flat 8x8"]) > T.SPEC_CAP and back["flat 32x32"] and back["two-colour 128x128"]
    assert not any(b for nm, b in back.items() if nm.startswith(("photo", "noise")))
    assert max(T.longest_match(by[nm]) for nm in by if nm.startswith(("photo", "noise"))) <= T.SPEC_CAP
    # the matches of the frames that stay on the route end one before, on and one past a window's end, first and second ones
    first, second = set(), set()
    for nm, s in by.items():
        if not back[nm]:
            a, b = T.windows(s)
            first |= a
            second |= b
    assert first == second == {-1, 0, 1}
    # matches() adds up to the text
    for nm, im in T.shaped()[:20]:
        m = T.matches(by[nm])
        assert m[-1][0] + m[-1][1] == 8 + 11 * im.shape[0] * im.shape[1], nm


def test_the_cap_and_machinery_frames_are_what_the_gpu_test_claims():
    import test_zd_small_batch as T
    names, imgs = zip(*T.cap_frames())
    streams = [T.restated(im) for im in imgs]
    longest = dict(zip(names, (T.longest_match(s) for s in streams)))
    print(longest)
    assert longest["band 40"] < longest["band 300"] and longest["photo 64x64"] <= T.SPEC_CAP and longest["flat 2x1"] <= 8
    for cap in T.CAPS:
        back = [T.handed_back(s, cap) for s in streams]
        assert 0 < sum(back) < len(back) or cap == 8, (cap, back)
    # at every cap above the speculation's some frame that stays has a walk behind it (the commit wave finishes it)
    for cap in T.CAPS[2:]:
        assert any(T.SPEC_CAP < ln <= cap for ln in longest.values()), cap
    mach = T.machinery_frames()
    assert [im.shape[0] * im.shape[1] for im in mach] == [4096, 1600, 1517, 7500, 1, 64, 63, 1024, 12288, 16385, 19200]
    assert [T.handed_back(T.restated(im)) for im in mach[:9]] == [False, True] + [False] * 7 and sum(T.routed(mach, 1024)) == 4
    assert len({len(T.restated(im)) for im in T.placement_kinds()}) >= 5
    many = T.many()
    assert len(many) == 3000 and len({im.shape[:2] for im in many}) == 8 and max(im.shape[0] * im.shape[1] for im in many) == 1024
    assert not any(T.handed_back(T.restated(im)) for im in many[::59])


def test_the_kernel_has_no_scratch_segment_and_fits_one_cu():
    kern = os.path.join(CSRC, "k_zd_small.hip")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), kern, "k_zd_small"], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "k_zd_small" in ln]
    assert len(lines) == 1, out
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
    assert field("VGPRs") <= 128
    # the static part from the code object, the dynamic part at the bound from the kernel's own rule: 3 bytes a pixel
    assert "return (3 * max_px + 15) & ~15u; }" in open(kern).read()
    assert field("LDS Size [bytes/block]") + 3 * 16384 <= 160 * 1024
