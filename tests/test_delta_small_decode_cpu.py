"""What the small-frame `delta` decode kernel computes per frame (cniic_amd/csrc/delta_small_dec.hpp) and what
tests/test_delta_small_decode.py relies on, without a GPU.  tests/delta_small_dec_check.cpp is compiled against the header as a stand-alone
program: a scalar decoder built from the header's functions walks the payload's 1024 subsequences in the kernel's order, re-decode rounds
included, beside a bit-by-bit walk of the trie, on streams the program builds with a binary heap; the same program runs once more under
-fsanitize=address,undefined.  Then, from the oracle alone: the streams the GPU test cuts, edits or builds by hand parse and fail exactly
where it says, its frames have the leaves and code lengths it relies on, and its mutants stay within their cap."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "delta_small_dec_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
PARTS = ("random", "one", "two", "equal16384", "chain19", "bit_lengths", "truncation", "resync", "fromdiff", "total")


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


def test_header_decoder_against_the_bit_by_bit_walk(tmp_path):
    import test_delta_small_decode as T
    exe = str(tmp_path / "delta_small_dec_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    assert "longest code met %d, bound %d" % (T.MAX_CODE_LEN, T.MAX_CODE_LEN) in out
    assert "1, 31, 32, 33 and %d bits" % (T.MAX_CODE_LEN * T.MAX_PX) in out
    assert "1001 lanes with bits, settled after 1001 rounds" in out
    assert "constants: max px %d, lanes %d, rounds %d," % (T.MAX_PX, T.LANES, T.LANES) in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "delta_small_dec_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_delta_small_decode as T
    import test_delta_small_batch as TE
    hdr = open(os.path.join(CSRC, "delta_small_dec.hpp")).read()
    assert re.search(r"constexpr uint32_t kDeltaSmallDecMaxPx = %d;" % T.MAX_PX, hdr)
    assert re.search(r"constexpr uint32_t kDsdLanes = %d;" % T.LANES, hdr)
    assert T.MAX_PX == TE.MAX_PX and T.MAX_CODE_LEN == TE.MAX_CODE_LEN            # the encode route's bound and longest code
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    for msg in (T.MSG_SHORT, T.MSG_RANGE, T.MSG_DIMS, T.TIMER):
        assert '"%s"' % msg in src, msg
    api = re.sub(r"(\d) (\d)", r"\1\2", open(os.path.join(ROOT, "include", "cniic_hip.h")).read())
    at = api.index("SMALL `delta` frames of a decode")
    para = api[at:api.index("*/", at)]
    assert "%d pixels" % T.MAX_PX in para and "%d bits" % T.MAX_CODE_LEN in para and T.TIMER in para


def _facts(data):
    import test_delta_small_decode as T
    leaves, pay = T.parse_trie(data)
    return len(leaves), max(d for _, d in leaves), pay


def test_route_frames_are_what_the_gpu_test_relies_on():
    import test_delta_small_decode as T
    imgs = T.route_images()
    assert len(imgs) == 3 * len(T.SIZES) + 1 and all(1 <= im.shape[0] * im.shape[1] <= T.MAX_PX for im in imgs)
    assert sorted({w * h for w, h in T.SIZES} & {63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384}) == [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384]
    for f, im in enumerate(imgs):
        rc, data, _ = O.encode("delta", im)
        assert rc == 0
        leaves, longest, pay = _facts(data)
        assert longest <= T.MAX_CODE_LEN and (leaves == 1) == (len(data) == pay), f   # more leaves than one: a payload
        if f == len(imgs) - 1:
            assert (leaves, longest, len(data)) == (1, 0, 15)                          # all black: one leaf, no payload
        if im.shape[:2] == (128, 128) and f % 3 == 1:
            assert leaves >= 16000 and longest <= 15                                   # noise at the bound: nearly every symbol a leaf, codes of nearly one length
        rcd, back = O.decode("delta", data)
        assert rcd == 0 and np.array_equal(back, im)


def test_cut_edited_and_hand_built_streams_fail_where_the_gpu_test_says():
    import test_delta_small_decode as T
    img = T.range_image()
    rc, good, _ = O.encode("delta", img)
    assert rc == 0
    diffs = {tuple(v) for v in O.unpack_signed(O.delta_diff(O.hilbert_linearize(img))).tolist()}
    assert diffs == {(100, 100, 100), (0, 0, 0), (30, 30, 30), (-30, -30, -30)}
    leaves, pay = T.parse_trie(good)
    for name, s, want_rc, msg, routed in T.failure_streams(good):
        rcd, back = O.decode("delta", s)
        assert rcd == want_rc, (name, rcd)
        if name.startswith("good") or name == "one byte more":
            assert np.array_equal(back, img) and routed, name
        elif name == "cut in the dimensions":
            assert len(s) < 8 and not routed
        elif name == "cut in the trie":
            assert 8 < len(s) < pay and not routed
        elif name == "cut at the first payload byte":
            assert len(s) == pay and T.parse_trie(s + b"\0")[1] == pay and not routed  # the decoder is whole, the payload is not there
        elif name in ("cut in the payload", "one byte short"):
            assert pay < len(s) < len(good) and T.parse_trie(s)[1] == pay and routed
            assert O.huf_decode_all(O.SYM_SIGNED, s[8:], 64)[0] != 0                   # the symbols run out
        elif name in ("above 255", "below 0"):
            assert len(s) == len(good) and _facts(s) == _facts(good) and routed
            rcs, syms = O.huf_decode_all(O.SYM_SIGNED, s[8:], 64)
            assert rcs == 0                                                            # it parses and all 64 symbols are there ...
            assert O.delta_undiff(syms)[0] != 0                                        # ... and FromDiff is where it fails
            d = O.unpack_signed(syms).cumsum(axis=0)
            assert (d.max() > 255) == (name == "above 255") and (d.min() < 0) == (name == "below 0")
        else:
            assert name == "a code of 20 bits" and not routed
            assert _facts(s)[:2] == (21, T.MAX_CODE_LEN + 1)
            assert np.array_equal(back, np.tile(np.array([7, 8, 9], np.uint8), (8, 8, 1)))


def test_mutants_stay_within_their_cap():
    """the oracle's decode alone: at most 5 % of the mutants are neither decoded nor refused as undecodable (their dimensions outgrow the room)"""
    import test_delta_small_decode as T
    small, large = T.mutant_sources()
    assert small.shape == (8, 8, 3) and large.shape == (29, 37, 3)
    streams = T.mutant_streams(O.encode("delta", small)[1], O.encode("delta", large)[1])
    assert len(streams) == T.MUTANTS == 200
    other = 0
    for s in streams:
        rc, _ = O.decode("delta", s, max_px=T.MUTANT_STRIDE // 3)
        other += rc not in (O.OK, O.DECODE)
    assert other <= T.MUTANTS // 20, other
