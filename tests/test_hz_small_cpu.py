"""What the small-frame kernels of Hilbert { compress: Zip } compute per frame (cniic_amd/csrc/hz_small.hpp beside zd_small.hpp and
zd_small_dec.hpp) and what tests/test_hz_small_batch.py and tests/test_hz_small_decode.py rely on, without a GPU.
tests/hz_small_check.cpp is compiled against the headers as a stand-alone program -- the encode's three phases over the new text kind for
W in {1, 2, 64, 256} with shuffled inserts and lowered caps beside a one-pass coder, the decode's five phases with 1, 7, 64 and 1024 lanes
in shuffled order under the lenient verdict and the record cut beside a one-pass table decoder, a few thousand mutants -- and runs plain
and once more under -fsanitize=address,undefined, as a program of its own.  Its restated streams and its verdicts are held against
tests/zip_dict_ref.py here.  Then, from zip_dict_ref alone: every claim the GPU tests make about a frame or a stream, with the exact sets
of frames handed back; the class surface, the three symbols, the expression that stays rejected, and the two cross-compiled kernels'
resources."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

import zip_dict_ref as Z

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hz_small_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
SELF_PARTS = ("text", "windows", "caps", "freeze", "decode", "decode", "total")
ENC_PARTS = ("text", "windows", "caps", "freeze", "total")
VERDICTS = {"ok": 0, "back": 1, "symbol": 2, "dangling": 3}


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


_EXE = {}


def _exe(tmp_path_factory, sanitized=False):
    if sanitized not in _EXE:
        exe = str(tmp_path_factory.mktemp("hz_small_check") / ("check_san" if sanitized else "check"))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2", "-Wall"]
        subprocess.check_call([_compiler(), "-std=c++17"] + flags + ["-I", CSRC, "-o", exe, SRC])
        _EXE[sanitized] = exe
    return _EXE[sanitized]


def _run(exe, parts, *args):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln.split()[1].rstrip(":") for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert tuple(ok) == parts and "FAIL" not in r.stdout, r.stdout[-4000:]
    return r.stdout


def _write_frames(path, imgs):
    """the frames in SCAN order (oracle_lib.hilbert_linearize): the program knows no scan"""
    import oracle_lib as O
    with open(path, "wb") as fp:
        fp.write(struct.pack("<I", len(imgs)))
        for im in imgs:
            fp.write(struct.pack("<II", im.shape[1], im.shape[0]))
            fp.write(np.ascontiguousarray(O.hilbert_linearize(im), np.uint8).tobytes())


def _write_streams(path, streams):
    with open(path, "wb") as fp:
        fp.write(struct.pack("<I", len(streams)))
        for s in streams:
            fp.write(struct.pack("<I", len(s)) + bytes(s))


def _fnv(data):
    h = 0xcbf29ce484222325
    for b in np.frombuffer(bytes(data), np.uint8).tolist():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _gpu_test_frames(max_px):
    """the frames of the GPU test of at most max_px pixels (each content and size once)"""
    import test_hz_small_batch as T
    imgs = [im for _, im in T.shaped()] + [im for _, im in T.cap_frames()] + T.machinery_frames() + T.placement_kinds()
    seen, out = set(), []
    for im in imgs:
        key = (im.shape, im.tobytes())
        if im.shape[0] * im.shape[1] <= max_px and key not in seen:
            seen.add(key)
            out.append(im)
    return out


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "hz_small.hpp"\nint main() { return cniic::hz_stride(cniic::hz_text_len(cniic::kHzSmallMaxPx)) == 360464 && cniic::hzd_cut(5, 9) == 5 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.call([exe]) == 0
    assert "#include" not in open(os.path.join(CSRC, "hz_small.hpp")).read().replace("#include <stdint.h>", "")


def test_the_program_on_frames_streams_and_mutants_of_its_own(tmp_path_factory):
    import test_hz_small_batch as T
    import test_hz_small_decode as TD
    out = _run(_exe(tmp_path_factory), SELF_PARTS)
    assert "ok total: bound %d pixels, window %d, caps %d %d, stride at the bound %d, table bits at the bound %d, pair cap %d, 0 mismatches" % (
        T.MAX_PX, T.WINDOW, T.SPEC_CAP, T.GIVE_UP, T.STRIDE_AT_BOUND, T.TABLE_BITS_AT_BOUND, TD.MAX_PAIRS) in out
    mutants = int(re.search(r"ok decode: \d+ streams, (\d+) mutants", out).group(1))
    assert mutants >= 2000


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path_factory, tmp_path):
    exe = _exe(tmp_path_factory, sanitized=True)
    frames, streams = str(tmp_path / "frames.bin"), str(tmp_path / "streams.bin")
    _write_frames(frames, _gpu_test_frames(1024))
    _run(exe, ENC_PARTS, "enc", frames, streams)
    import test_hz_small_decode as TD
    given = str(tmp_path / "given.bin")
    _write_streams(given, [s for _, s in TD.hostile()])
    _run(exe, ("total",), "dec", given)
    _run(exe, SELF_PARTS)


def test_the_encode_emulation_on_the_gpu_tests_frames_against_zip_dict_ref(tmp_path_factory, tmp_path):
    import test_hz_small_batch as T
    imgs = _gpu_test_frames(T.MAX_PX)
    assert len(imgs) >= 4 * len(T.SIZES) and max(im.shape[0] * im.shape[1] for im in imgs) == T.MAX_PX
    frames, streams = str(tmp_path / "frames.bin"), str(tmp_path / "streams.bin")
    _write_frames(frames, imgs)
    _run(_exe(tmp_path_factory), ENC_PARTS, "enc", frames, streams)
    blob = open(streams, "rb").read()
    at = 0
    for k, im in enumerate(imgs):
        ln, = struct.unpack_from("<I", blob, at)
        at += 4
        assert blob[at:at + ln] == T.restated(im), k
        at += ln
    assert at == len(blob)


def _decode_lines(exe, path, *caps):
    out = _run(exe, ("total",), "dec", path, *[str(c) for c in caps])
    rows = [ln.split() for ln in out.splitlines() if re.match(r"^\d+ -?\d+ ", ln)]
    return [(int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]), int(r[6], 16)) for r in rows]


def _hold_against_the_program(exe, tmp_path, streams, what, **caps):
    """analyse (tests/test_hz_small_decode.py) says of every stream what the program's table decoder and emulation say"""
    import test_hz_small_decode as TD
    path = str(tmp_path / (what + ".bin"))
    _write_streams(path, streams)
    args = (caps.get("max_pairs", TD.MAX_PAIRS), caps.get("hops", TD.HOPS), caps.get("rounds", TD.ROUNDS))
    rows = _decode_lines(exe, path, *args)
    assert len(rows) == len(streams)
    for f, (s, (verdict, a, w, h, cut, fnv)) in enumerate(zip(streams, rows)):
        c = TD.analyse(s, **caps)
        if not c["cand"]:
            assert verdict == -1, (what, f)
            continue
        assert verdict == VERDICTS[c["verdict"]] and a == c["a"] and (w, h) == (c["w"], c["h"]), (what, f, verdict, c["verdict"])
        if c["verdict"] == "ok":
            assert cut == c["cut"] and fnv == _fnv(c["lin"].tobytes()), (what, f)


def test_the_library_and_hostile_streams_are_what_the_gpu_test_claims(tmp_path_factory, tmp_path):
    import test_hz_small_decode as TD
    dec = lambda s, need: Z.decode_c(TD.HB.clib(), s, need)
    names, imgs, streams = zip(*TD.library())
    import oracle_lib as O
    for nm, im, s in zip(names, imgs, streams):
        a = TD.analyse(s)
        if not a["cand"]:
            assert im.shape[0] * im.shape[1] > TD.MAX_PX, nm
            continue
        assert a["verdict"] == "ok" and a["cut"] == im.shape[0] * im.shape[1] and a["needed"] == a["P"], nm     # nobody is handed back, every pair is needed
        assert np.array_equal(a["lin"], O.hilbert_linearize(im)) and np.array_equal(TD.along_the_scan(a["lin"], a["w"], a["h"]), im), nm
        assert a["gen"] < TD.ROUNDS and a["visits"] <= TD.HOPS and a["P"] <= TD.MAX_PAIRS, nm
    _hold_against_the_program(_exe(tmp_path_factory), tmp_path, streams[::3], "library")
    # the hostile streams: the restatement's pixels, or its verdict
    hnames, hstreams = zip(*TD.hostile())
    kinds = dict(zip(hnames, (TD.analyse(s) for s in hstreams)))
    for nm, s in zip(hnames, hstreams):
        a, ref = kinds[nm], Z.hilbert_decode_lin(dec, s)
        if not a["cand"]:
            continue
        assert (ref is None) == (a["verdict"] != "ok"), nm
        if ref is not None:
            assert np.array_equal(ref[2], a["lin"]), nm
    for k in (0, 1, 100):
        for r in range(4):
            a = kinds["cut %d + %d" % (k, r)]
            assert a["verdict"] == ("dangling" if r >= 2 else "ok") and (r >= 2 or a["cut"] < 3700), (k, r)
    for at in (0, 1234, 3699):
        for lenb in (4, 2, 1):
            a = kinds["record %d of length %d" % (at, lenb)]
            assert a["verdict"] == "ok" and a["cut"] == at and not a["lin"][at:].any()
    assert kinds["pair 10 uses its own symbol"]["verdict"] == "symbol" and kinds["pair 10 uses its own symbol"]["a"] == 10
    assert kinds["the last needed pair's second symbol is not handed out"]["verdict"] == "symbol"
    assert kinds["the same symbol behind the last needed pair"]["verdict"] == "ok" and kinds["the same symbol behind the last needed pair"]["cut"] == 3700
    assert all(kinds["garbage %d" % g]["verdict"] == "ok" and kinds["garbage %d" % g]["cut"] == 3700 for g in (1, 2, 3, 4, 5, 255, 768))
    assert kinds["dimensions that claim fewer pixels"]["cut"] == 50 * 37 and kinds["dimensions that claim more"]["cut"] == 3700
    assert not kinds["7 bytes"]["cand"] and kinds["8 bytes"]["verdict"] == "ok" and kinds["8 bytes"]["cut"] == 0
    assert not kinds["2^32 pixels"]["cand"] and not kinds["a width of 0"]["cand"] and not kinds["more than the bound"]["cand"]
    one_short = kinds["an image one byte longer than the stride"]
    assert one_short["cand"] and 3 * one_short["w"] * one_short["h"] - 1 == TD.IMG_STRIDE_HOSTILE >= 3 * 100 * 38
    _hold_against_the_program(_exe(tmp_path_factory), tmp_path, hstreams, "hostile")


def test_the_cap_streams_lie_on_both_sides_of_the_lowered_knobs(tmp_path_factory, tmp_path):
    import test_hz_small_decode as TD
    names, streams = zip(*TD.cap_streams())
    claims = [TD.analyse(s) for s in streams]
    print({nm: (a["needed"], a["visits"], a["gen"]) for nm, a in zip(names, claims)})
    assert all(a["verdict"] == "ok" and a["needed"] >= 2 and a["visits"] >= 2 and a["gen"] >= 1 for a in claims)
    depth = sorted(a["visits"] for a in claims)
    assert depth[2] < depth[4]            # a cap at the median depth hands some back and keeps some
    exe = _exe(tmp_path_factory)
    for key, own in (("max_pairs", lambda a: a["needed"]), ("hops", lambda a: a["visits"]), ("rounds", lambda a: a["gen"] + 1)):
        for f, a in enumerate(claims):
            for value in (own(a) - 1, own(a), own(a) + 1):
                assert TD.back(streams[f], **{key: value}) == (value < own(a)), (names[f], key, value)
                _hold_against_the_program(exe, tmp_path, streams[f:f + 1], "cap", **{key: value})


def test_the_shaped_frames_are_what_the_gpu_test_claims():
    import test_hz_small_batch as T
    names, imgs = zip(*T.shaped())
    by = {nm: T.restated(im, "cpu " + nm) for nm, im in zip(names, imgs)}
    # the small ones through the Python coder too
    import oracle_lib as O
    for nm, im in zip(names, imgs):
        if im.shape[0] * im.shape[1] <= 1024:
            assert Z.hilbert_encode(Z.encode_py, O.hilbert_linearize(im), im.shape[1], im.shape[0]) == by[nm], nm
    assert len(Z.records(Z.photo_like(1, 1))) == 11 and len(by["photo 1x1"]) == T.HEAD + 4 * 5
    assert len(Z.records(np.zeros((23, 3), np.uint8))) == 253 < T.WINDOW < 264 == len(Z.records(np.zeros((24, 3), np.uint8)))
    # exactly which frames are handed back: flat and two-colour ones from 3700 pixels on, no photo-like or noise frame
    back = {nm for nm in names[:-2] if T.handed_back(by[nm])}
    assert back == T.SHAPED_HANDED_BACK and not any(nm.startswith(("photo", "noise", "few")) for nm in back)
    assert max(T.longest_match(by[nm]) for nm in names if nm.startswith(("photo", "noise"))) <= T.SPEC_CAP
    assert any(T.SPEC_CAP < T.longest_match(by[nm]) <= T.GIVE_UP for nm in names[:-2])          # a walk the commit wave finishes
    # both endings
    ends = {nm: T.ends_in_eof(by[nm]) for nm in names}
    assert ends["photo 1x1"] and ends["noise 23x1"] and ends["photo 4x4"] and ends["photo 16384x1"]
    assert not ends["photo 2x1"] and not ends["photo 24x1"] and not ends["noise 64x64"] and not ends["photo 128x128"]
    # the matches of the frames that stay on the route end one before, on and one past a window's end, first and second ones
    first, second = set(), set()
    for nm in names[:-2]:
        if nm not in back:
            a, b = T.windows(by[nm])
            first |= a
            second |= b
    assert first == second == {-1, 0, 1}
    for nm, im in list(zip(names, imgs))[:24]:
        m = T.ZB.matches(T.pairs_of(by[nm]))
        assert m[-1][0] + m[-1][1] == 11 * im.shape[0] * im.shape[1], nm


def test_the_cap_and_machinery_frames_are_what_the_gpu_test_claims():
    import test_hz_small_batch as T
    names, imgs = zip(*T.cap_frames())
    streams = [T.restated(im) for im in imgs]
    longest = dict(zip(names, (T.longest_match(s) for s in streams)))
    print(longest)
    for cap in T.CAPS:
        assert {nm for nm, s in zip(names, streams) if T.handed_back(s, cap)} == T.CAP_HANDED_BACK[cap], cap
        assert 0 < len(T.CAP_HANDED_BACK[cap]) < len(names)
    for cap in T.CAPS[2:]:
        assert any(T.SPEC_CAP < ln <= cap for ln in longest.values()), cap
    mach = T.machinery_frames()
    assert [im.shape[0] * im.shape[1] for im in mach] == [4096, 1600, 1517, 7500, 1, 64, 63, 1024, 12288, 16385, 19200]
    assert [T.handed_back(T.restated(im)) for im in mach[:9]] == T.MACHINERY_HANDED_BACK and sum(T.routed(mach, 1024)) == 4
    assert len({len(T.restated(im)) for im in T.placement_kinds()}) >= 5 and not any(T.handed_back(T.restated(im)) for im in T.placement_kinds())
    many = T.ZB.many()
    assert not any(T.handed_back(T.restated(im)) for im in many[::59]) and not any(T.handed_back(T.restated(im)) for im in T.tiny(6))
    assert T.frame_bytes(T.MAX_PX) == T.STRIDE_AT_BOUND + (8 << T.TABLE_BITS_AT_BOUND) + 32


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_hz_small_batch as T
    import test_hz_small_decode as TD
    hdr = open(os.path.join(CSRC, "hz_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kHzSmallMaxPx = %d;" % T.MAX_PX, hdr) and re.search(r"constexpr uint32_t kHzHead = %d;" % T.HEAD, hdr)
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "return hz_stride(N) + (8ull << zs_table_bits(N)) + sizeof(ZdSmallRow) + sizeof(ZdSmallResult);" in src
    assert 'test_env("%s")' % T.KNOB_CAP in src
    assert 'small_route_max_px("%s", "%s", kHzSmallMaxPx)' % (T.KNOB_OFF, T.KNOB_MAX_PX) in capi and 'test_env("%s")' % T.KNOB_FLOOR_OFF in capi
    assert 'small_route_max_px("%s", "%s", kHzSmallMaxPx)' % (TD.KNOB_OFF, TD.KNOB_MAX_PX) in src and 'test_env("%s")' % TD.KNOB_FLOOR_OFF in src
    for knob, bound in ((TD.KNOB_PAIRS, "kZsdMaxPairs"), (TD.KNOB_HOPS, "kZsdHops"), (TD.KNOB_ROUNDS, "kZsdRounds")):
        assert 'test_lower_cap("%s", %s)' % (knob, bound) in src, knob
    assert "static uint64_t hz_small_floor_px(uint64_t, const CodecDesc &) { return hz_small_floor_off() ? ~0ull : 0; }" in capi       # no class takes the encode route
    assert re.search(r"constexpr uint32_t kHzSmallDecFloorFew = %d, kHzSmallDecFloorMany = %d;" % (TD.FLOOR_FEW, TD.FLOOR_MANY), src)
    assert re.search(r"constexpr uint64_t kHzSmallDecFloorPxFew = %d, kHzSmallDecFloorPxMany = %d;" % (TD.FLOOR_PX_FEW, TD.FLOOR_PX_MANY), src)
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in (T.TIMER, T.PLACE, T.HANDBACK, T.FINISHED, TD.TIMER, TD.HANDBACK):
        assert '"%s"' % name in src and '"%s"' % name in api, name
    for knob in (T.KNOB_OFF, T.KNOB_MAX_PX, T.KNOB_FLOOR_OFF, T.KNOB_CAP, TD.KNOB_OFF, TD.KNOB_MAX_PX, TD.KNOB_FLOOR_OFF, TD.KNOB_PAIRS, TD.KNOB_HOPS, TD.KNOB_ROUNDS):
        assert knob in readme, knob
    for text in TD.MESSAGES.values():
        for piece in re.split(r"%d", text):
            assert piece in src and piece in open(os.path.join(CSRC, "zipdict.cpp")).read(), piece


def test_the_class_the_symbols_and_the_expression_that_stays_rejected():
    import inspect
    import cniic_amd
    from cniic_amd import _lib
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    for name in ("cniic_hilbert_zip_encode_batch_var", "cniic_hilbert_zip_decode_batch", "cniic_hilbert_zip_measure_batch"):
        assert re.search(r"int32_t %s\(cniic_ctx \*ctx," % name, api) and name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["cniic_hilbert_zip_encode_batch_var"][1]) == 10 == len(_lib.PROTOTYPES["cniic_hilbert_zip_decode_batch"][1]) == len(_lib.PROTOTYPES["cniic_hilbert_zip_measure_batch"][1])
    for method in ("hilbert_zip_encode_batch_var", "hilbert_zip_decode_batch", "hilbert_zip_measure_batch"):
        assert callable(getattr(_lib.Context, method)), method
    c = cniic_amd.HilbertZip()
    assert c.name() == "hilbert-zip" and c.is_lossless() and c.expr is None
    assert c.encode_batch([]) == [] and c.decode_batch([]) == [] and c.measure([]) == []
    assert "kw" in inspect.signature(cniic_amd.HilbertZip.encode_batch).parameters and "allow" in inspect.signature(cniic_amd.HilbertZip.encode_batch).parameters
    assert {"seed", "max_iters", "flags"} <= set(inspect.signature(cniic_amd.HilbertZip.measure).parameters)      # what Codec.measure's callers pass
    for method in ("encode_batch", "decode_batch", "measure"):
        body = inspect.getsource(getattr(cniic_amd.HilbertZip, method))
        assert "NotImplementedError" not in body and "self.ctx.hilbert_zip_" in body, method       # one call, not a loop of single calls
    # the library's parser stays as it is
    assert _lib.codec_parse_f64("hilbert(zip)") is None and _lib.codec_parse_f64("zip(dict)") is not None
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    parse = src[src.index("bool parse_codec("):src.index("std::string rust_f64_display(")]
    assert "CODEC_HILBERT_ZIP" not in parse and "CODEC_HILBERT_ZIP = 7" in open(os.path.join(CSRC, "codec.hpp")).read()


def _resources(kern, name):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), kern, name + "E"], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if name in ln]
    assert len(lines) == 1, out
    print(lines[0])
    return lambda field: int(re.search(re.escape(field) + r": (\d+)", lines[0]).group(1))


def test_the_two_kernels_have_no_scratch_no_spills_and_fit_one_cu():
    enc = _resources(os.path.join(CSRC, "k_zd_small.hip"), "k_hz_small")
    assert enc("ScratchSize [bytes/lane]") == 0 and enc("VGPRs Spill") == 0 and enc("SGPRs Spill") == 0 and enc("VGPRs") <= 128
    assert enc("LDS Size [bytes/block]") + 3 * 16384 <= 160 * 1024                     # the dynamic part at the bound: 3 bytes a pixel
    kern = os.path.join(CSRC, "k_zd_small_dec.hip")
    dec = _resources(kern, "k_hz_small_dec")
    assert dec("ScratchSize [bytes/lane]") == 0 and dec("VGPRs Spill") == 0 and dec("SGPRs Spill") == 0
    assert dec("VGPRs") <= 128                                                          # 1024 threads: 16 waves of a block on four SIMDs
    src = open(kern).read()
    assert "constexpr uint32_t kHzdLdsMax = kZsdLdsMax - kHzScanLds;" in src and "constexpr uint32_t kHzScanLds = 2 * 1024 + 16;" in open(os.path.join(CSRC, "hz_small.hpp")).read()
    assert "static_assert(kHzSmallMaxPx == kZdSmallDecMaxPx && zsd_lds_bytes(kZsdMaxPairs, kHzSmallMaxPx) <= kHzdLdsMax" in src
    # the static part from the code object (the 2064 bytes of scan tables and the few words), the dynamic part under the launcher's limit
    assert 2064 <= dec("LDS Size [bytes/block]") <= 2064 + 512 and dec("LDS Size [bytes/block]") + (160 * 1024 - 512 - 2064) <= 160 * 1024
    assert 4 * (24576 + 1) + ((3 * 16384 + 16 + 15) & ~15) == 147476 <= 160 * 1024 - 512 - 2064
