"""What the small-frame `zip(dict)` decode kernel computes per frame (cniic_amd/csrc/zd_small_dec.hpp) and what tests/test_zd_small_decode.py
relies on, without a GPU.  tests/zd_small_dec_check.cpp is compiled against the header as a stand-alone program: the header's functions as a
scalar emulation of k_zd_small_dec's five phases, lane by lane and in shuffled order inside the rounds, against a one-pass table decoder
written without the header -- plain, and under the address and undefined-behaviour sanitizers.  Every claim of the GPU test (analyse: the
verdict, its numbers, the needed pairs, generations, visits, the chain frames) is recomputed here from tests/zip_dict_ref.py alone, the
constants the tests restate are held against the sources, and the kernel's registers, scratch and LDS are read from the code object."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

import zip_dict_ref as Z

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "zd_small_dec_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
VERDICTS = {-1: None, 0: "ok", 1: "back", 2: "symbol", 3: "dangling", 4: "short", 5: "record"}


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "ok total" in r.stdout and ", 0 mismatches" in r.stdout, r.stdout[-4000:]
    return r.stdout


def _gpu_test_streams():
    """every stream the GPU test decodes that is built by hand or cut, and the library's streams of at most 4096 pixels"""
    import test_zd_small_decode as T
    out = [s for _, im, s in T.library() if im.shape[0] * im.shape[1] <= 4096]
    out += [s for _, s in T.lazy_streams()[1]] + [s for _, s in T.verdict_streams()[1]] + [s for _, s in T.saturation_streams()]
    out += [s for _, s, _ in T.record_streams()] + [T.chain(D)[1] for D in T.DEPTHS + (3, 10, 11, 12, 30)] + T.placement_streams() + T.mutants()
    out += [T.with_empty_texts(T.encoded(im)) for im in (Z.photo_like(13, 5), Z.flat(8, 8))]
    return out


def _write_streams(path, streams):
    with open(path, "wb") as fp:
        fp.write(struct.pack("<I", len(streams)))
        for s in streams:
            fp.write(struct.pack("<I", len(s)))
            fp.write(bytes(s))


def _fnv(data):
    h = 0xcbf29ce484222325
    for b in np.frombuffer(bytes(data), np.uint8).tolist():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "zd_small_dec.hpp"\nint main() { return cniic::zsd_lds_bytes(cniic::kZsdMaxPairs, cniic::kZdSmallDecMaxPx) == 147476 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.call([exe]) == 0
    assert "#include" not in open(os.path.join(CSRC, "zd_small_dec.hpp")).read().replace("#include <stdint.h>", "")     # nothing of the library


def test_header_emulation_against_the_table_decoder_and_the_gpu_test_s_claims(tmp_path):
    import test_zd_small_decode as T
    exe = str(tmp_path / "zd_small_dec_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)                                                         # its own streams, mutants, lowered caps, the saturating sums
    assert "ok total: bound %d pixels, pairs %d, hops %d, rounds %d, LDS at the bounds 147476, 0 mismatches" % (T.MAX_PX, T.MAX_PAIRS, T.HOPS, T.ROUNDS) in out
    streams = _gpu_test_streams()
    assert len(streams) >= 280
    path = str(tmp_path / "streams.bin")
    _write_streams(path, streams)
    for caps in ((T.MAX_PAIRS, T.HOPS, T.ROUNDS), (T.MAX_PAIRS, 15, T.ROUNDS), (T.MAX_PAIRS, T.HOPS, 14), (120, 6, 6)):
        lines = [ln.split() for ln in _run(exe, path, *caps).splitlines() if ln[:1].isdigit()]
        assert len(lines) == len(streams)
        for ln, s in zip(lines, streams):
            a = T.analyse(s, max_pairs=caps[0], hops=caps[1], rounds=caps[2])
            assert VERDICTS[int(ln[1])] == a.get("verdict"), (caps, ln, a.get("verdict"))
            if a["cand"]:
                assert (int(ln[2]), int(ln[3]), int(ln[4]), int(ln[5])) == (a["a"], a["b"], a["w"], a["h"]), (caps, ln)
                assert int(ln[6], 16) == _fnv(a["pixels"] if a["verdict"] == "ok" else b""), (caps, ln)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    import test_zd_small_decode as T
    exe = str(tmp_path / "zd_small_dec_check_san")
    subprocess.check_call([_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)
    path = str(tmp_path / "streams.bin")
    _write_streams(path, [s for _, s in T.lazy_streams()[1]] + [s for _, s in T.verdict_streams()[1]] + [s for _, s in T.saturation_streams()] + T.mutants()[:60])
    _run(exe, path)
    _run(exe, path, 100, 5, 5)


def _by_the_reference(stream):
    """(verdict, a, b, pixels) of a candidate stream from zip_dict_ref.decode_py alone, at the single decode's order of errors"""
    head = Z.decode_py(stream[:64], 8)
    w, h = struct.unpack_from("<II", head)
    need = 8 + 11 * w * h
    pairs = len(stream) // 4
    try:
        text = Z.decode_py(stream, need)
    except Z.ZipError as e:
        if "without a second" in str(e):
            return "dangling", 0, 0, None
        k = next(k for k in range(pairs + 1) if _raises(stream[:4 * (k + 1)], need))     # the first pair the reader cannot take
        return "symbol", k, 0, None
    if len(text) < need:
        return "short", len(text), need, None
    rec = np.frombuffer(text[8:need], np.uint8).reshape(-1, 11)
    bad = np.flatnonzero((rec[:, 0] != 3) | rec[:, 1:8].any(axis=1))
    if bad.size:
        return "record", int(bad[0]), 0, None
    return "ok", 0, 0, rec[:, 8:11].reshape(-1)


def _raises(stream, need):
    try:
        Z.decode_py(stream, need)
    except Z.ZipError:
        return True
    return False


def test_the_claims_of_the_gpu_test_from_zip_dict_ref_alone():
    import test_zd_small_decode as T
    # every verdict, with its numbers
    named = T.lazy_streams()[1] + T.verdict_streams()[1] + [(n, s) for n, s, _ in T.record_streams()] + [("mutant %d" % k, s) for k, s in enumerate(T.mutants())]
    named += [s for s in T.saturation_streams()[1:]] + [("placement %d" % k, s) for k, s in enumerate(T.placement_streams())]
    seen = set()
    for name, s in named:
        a = T.analyse(s, hops=1 << 20, rounds=1 << 20)
        if not a["cand"]:
            assert name.startswith("a bad symbol in first pair") and _raises(s[:64], 8), name
            continue
        v, x, y, px = _by_the_reference(s)
        assert (a["verdict"], a["a"], a["b"]) == (v, x, y), (name, a["verdict"], a["a"], a["b"], v, x, y)
        if v == "ok":
            assert np.array_equal(a["pixels"], px), name
            # the needed pairs: one fewer and the reader comes up short
            assert len(Z.decode_py(s[:4 * a["needed"]], a["need"])) >= a["need"] > len(Z.decode_py(s[:4 * (a["needed"] - 1)], a["need"])), name
        seen.add(v)
    assert seen == {"ok", "symbol", "dangling", "short", "record"}
    needed, lazy = T.lazy_streams()
    assert needed == T.analyse(T.encoded(Z.photo_like(13, 5)))["needed"] and [len(s) - 4 * needed for _, s in lazy] == [0, 4, 5, 6, 7] * 1 + [4, 5, 6, 7]
    # the library: candidates, what rides along, the table of the issue
    lib = {nm: (im, s) for nm, im, s in T.library()}
    for nm, (im, s) in lib.items():
        a = T.analyse(s)
        assert a["cand"] == (im.shape[0] * im.shape[1] <= T.MAX_PX), nm
        if a["cand"]:
            assert a["verdict"] == "ok" and np.array_equal(a["pixels"], im.reshape(-1)) and a["gen"] <= 17 and a["visits"] <= 18, (nm, a["gen"], a["visits"])
            assert a["needed"] <= len(s) // 4 <= 23356 < T.MAX_PAIRS, nm
    assert [len(lib["photo %dx%d" % wh][1]) // 4 for wh in ((32, 32), (64, 64), (128, 96), (128, 128), (16384, 1))] == [1500, 5440, 14262, 18941, 21812]
    assert len(lib["noise 128x128"][1]) // 4 == 23310 and T.analyse(lib["photo 64x64"][1])["needed"] == 5440
    # generations are what a decoder that tracks them says, and a byte's visits never pass its pair's generation + 1
    for nm in ("photo 32x32", "flat 32x32", "two-colour 64x64", "noise 13x5"):
        s = lib[nm][1]
        gen = {}
        for k, (s1, s2) in enumerate(T.pairs_of(s)):
            gen[Z.FIRST_NEW + k] = 1 + max(gen.get(s1, -1), gen.get(s2, -1))
        a = T.analyse(s)
        assert a["gen"] == max(gen.values()) and a["visits"] <= a["gen"] + 1, nm
    # the chain frames
    for D in T.DEPTHS + (3, 10, 11, 12, 30):
        n, s = T.chain(D)
        text = Z.decode_py(s)
        assert len(text) == 8 + 11 * n and text[:8] == struct.pack("<II", n, 1) and text[8:] == (b"\x03" + bytes(10)) * n, D
        a = T.analyse(s, hops=1 << 20, rounds=1 << 20)
        assert (a["gen"], a["visits"], a["needed"], len(s) // 4) == (D + 3, D + 4, 11 + D, 11 + D), D
        assert T.back(s) == (D + 3 >= T.ROUNDS or D + 4 > T.HOPS) and T.back(s, rounds=D + 3) and not T.back(s, rounds=D + 4, hops=D + 4) and T.back(s, rounds=D + 4, hops=D + 3), D
    assert [T.chain(D)[0] for D in (63, 64, 65)] == [2082, 2147, 2213]
    # empty texts: the same text from more pairs
    for im in (Z.photo_like(13, 5), Z.noise(32, 32), Z.flat(8, 8), T.two_colour(7, 3)):
        p = T.encoded(im)
        s = T.with_empty_texts(p)
        assert Z.decode_py(s) == Z.decode_py(p) == Z.zip_text(im) and len(s) == len(p) + 8
        assert np.array_equal(Z.codec_decode(Z.decode_py, s), im)
    # saturation: what the streams claim
    sat = dict(T.saturation_streams())
    for nm, doublings in (("2^71 bytes", 70), ("2^41 bytes", 40)):
        pairs = T.pairs_of(sat[nm])
        length = {}
        for k, (s1, s2) in enumerate(pairs):
            length[Z.FIRST_NEW + k] = length.get(s1, 1) + length.get(s2, 1)
        assert max(length.values()) == 2 ** (doublings + 1), nm
    assert T.analyse(sat["200 pairs of at least need"])["need"] <= 128 and len(T.pairs_of(sat["200 pairs of at least need"])) == 211
    # the pair cap's frame
    photo = lib["photo 64x64"][1]
    needed = T.analyse(photo)["needed"]
    assert T.back(photo, max_pairs=needed - 1) and not T.back(photo, max_pairs=needed) and not T.back(photo, max_pairs=needed + 1)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_zd_small_decode as T
    hdr = open(os.path.join(CSRC, "zd_small_dec.hpp")).read()
    for name, val in (("kZdSmallDecMaxPx", T.MAX_PX), ("kZsdMaxPairs", T.MAX_PAIRS), ("kZsdHops", T.HOPS), ("kZsdRounds", T.ROUNDS)):
        assert re.search(r"constexpr uint32_t %s = %d;" % (name, val), hdr), name
    assert 24576 <= T.MAX_PAIRS < 65279 and "static_assert(kZsdMaxPairs < kZsdEof - kZsdFirstNew" in hdr
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    assert "constexpr uint64_t kZdDecHead = %d;" % T.HEAD in src
    assert 'small_route_max_px("%s", "%s", kZdSmallDecMaxPx)' % (T.KNOB_OFF, T.KNOB_MAX_PX) in src and 'test_env("%s")' % T.KNOB_FLOOR_OFF in src
    for knob, bound in ((T.KNOB_PAIRS, "kZsdMaxPairs"), (T.KNOB_HOPS, "kZsdHops"), (T.KNOB_ROUNDS, "kZsdRounds")):
        assert 'test_lower_cap("%s", %s)' % (knob, bound) in src, knob
    assert re.search(r"constexpr uint32_t kZdSmallDecFloorFew = %d, kZdSmallDecFloorMany = %d;" % (T.FLOOR_FEW, T.FLOOR_MANY), src)
    assert re.search(r"constexpr uint64_t kZdSmallDecFloorPxFew = %d, kZdSmallDecFloorPxMany = %d;" % (T.FLOOR_PX_FEW, T.FLOOR_PX_MANY), src)
    for text in T.MESSAGES.values():
        for piece in re.split(r"%d", text):
            assert piece in src and piece in open(os.path.join(CSRC, "zipdict.cpp")).read(), piece
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in (T.TIMER, T.HANDBACK):
        assert '"%s"' % name in src and name in api, name
    for knob in (T.KNOB_OFF, T.KNOB_MAX_PX, T.KNOB_FLOOR_OFF, T.KNOB_PAIRS, T.KNOB_HOPS, T.KNOB_ROUNDS):
        assert knob in readme, knob
    assert "k_zd_small_dec.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_kernel_has_no_scratch_segment_and_fits_one_cu():
    kern = os.path.join(CSRC, "k_zd_small_dec.hip")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), kern, "k_zd_small_dec"], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if "k_zd_small_dec" in ln]
    assert len(lines) == 1, out
    print(lines[0])
    field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
    src = open(kern).read()
    assert "constexpr int kZsdThreads = 1024;" in src and field("VGPRs") <= 128          # 16 waves of a block on four SIMDs
    # the static part from the code object, the dynamic part at the bounds from the header's rule, under the launcher's limit
    assert "constexpr uint32_t kZsdLdsMax = 160 * 1024 - 512;" in src and field("LDS Size [bytes/block]") <= 512
    assert 4 * (24576 + 1) + ((3 * 16384 + 16 + 15) & ~15) == 147476 <= 160 * 1024 - 512
