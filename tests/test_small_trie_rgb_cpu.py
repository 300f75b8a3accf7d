"""What the small-decoder parse kernel computes per frame for Rgb leaves (cniic_amd/csrc/small_trie.hpp, S = 11: `hufman` and
`cluster-colors` streams) and what tests/test_small_trie_rgb_gpu.py relies on, without a GPU.  tests/small_trie_rgb_check.cpp is compiled
against the header as a stand-alone program: a scalar parser made of the header's functions, 1024 lanes of up to 7 chunks and 64-bit maps in
the kernel's order, beside a byte-by-byte stack parse, on tries the program builds; the same program runs once more under
-fsanitize=address,undefined.  Then the constants the header, the route and the GPU test share, and, from the oracle alone, what the GPU
test's hand-built streams are."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "small_trie_rgb_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
PARTS = ("words", "small", "chains", "bound", "last", "random", "offsets", "lengths", "mutations", "symbols", "total")


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


def test_header_parser_against_the_stack_parse(tmp_path):
    import test_small_trie_rgb_gpu as G
    exe = str(tmp_path / "small_trie_rgb_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-w", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    window = 13 * G.MAX_LEAVES - 1
    assert window == 212991 and (window + G.CHUNK - 1) // G.CHUNK == 6656 > 4 * G.LANES
    assert "constants: leaves %d, lanes %d, chunk %d, window %d, lane chunks %d, rows %d" % (G.MAX_LEAVES, G.LANES, G.CHUNK, window, G.MAX_LANE_CHUNKS, G.H.MAX_CODE_LEN + 1) in out
    assert "%d leaves parsed, %d not ours" % (G.MAX_LEAVES, G.MAX_LEAVES + 1) in out
    assert "60 tries parsed, up to %d leaves" % G.MAX_LEAVES in out
    assert "%d edits" % (90 * 255) in out and "for k = 1 .. 6" in out
    assert re.search(r"a word each\), [1-9]\d* above \(none\)", out)            # nodes above 2 * 16384 - 2 with a P the table keeps: met, and no word


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "small_trie_rgb_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_small_trie_rgb_gpu as G
    hdr = open(os.path.join(CSRC, "small_trie.hpp")).read()
    assert re.search(r"constexpr uint32_t kSmallTrieMaxLeaves = %d;" % G.MAX_LEAVES, hdr)
    assert re.search(r"constexpr uint32_t kStChunk = %d;" % G.CHUNK, hdr)
    assert re.search(r"constexpr uint32_t kStLanes = %d;" % G.LANES, hdr)
    assert re.search(r"constexpr uint32_t kStMaxKRgb = %d;" % G.MAX_LANE_CHUNKS, hdr)
    assert G.MAX_LANE_CHUNKS * G.LANES * G.CHUNK >= 13 * G.MAX_LEAVES - 1 > (G.MAX_LANE_CHUNKS - 1) * G.LANES * G.CHUNK
    huf = open(os.path.join(CSRC, "huf_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kHufSmallMaxPx = %d;" % G.MAX_PX, huf) and re.search(r"constexpr uint32_t kHufSmallLeafSym = %d;" % (G.LEAF - 1), huf)
    assert (G.LONGEST_SMALL + 15) & ~15 == G.H.T.STRIDE_AT_BOUND                # hs_stride(16384) is that stream's length, rounded up
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    for name in (G.PARSE, G.PARSE_HOST, G.KNOB, G.FLOOR_KNOB, G.H.TIMER):
        assert '"%s"' % name in src, name
    assert re.search(r"constexpr uint32_t kHufSmallDecFloorFrames = %d;" % G.FLOOR, src) and G.FLOOR == G.H.T.DEC_FLOOR_FRAMES
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    assert G.PARSE in api and G.PARSE_HOST in api
    kern = open(os.path.join(CSRC, "k_small_trie.hip")).read()
    assert "void k_small_trieparse_rgb(" in kern and "void k_small_trieparse(" in kern


def _facts(data):
    import test_small_trie_rgb_gpu as G
    leaves, pay = G.H.parse_trie(data)
    return len(leaves), max(d for _, d in leaves), pay


def test_hand_built_decoders_are_what_the_gpu_test_says():
    import test_small_trie_rgb_gpu as G
    for leaves, longest in ((1, 0), (2, 1), (100, 7), (G.MAX_LEAVES, 14)):
        s = G.wide_stream(leaves)
        assert _facts(s) == (leaves, longest, 8 + 13 * leaves - 1)
        rc, back = O.decode("hufman", s)
        assert rc == 0 and np.array_equal(back, G.wide_image()), leaves
    cases = G.switch_streams()
    assert [(k, w) for k, w, _ in cases] == [(k, k * 32768 + more) for k in range(1, 7) for more in (0, 1)]
    for k, window, s in cases:
        leaves, longest, pay = _facts(s)
        assert len(s) == 8 + window and pay + 8 * longest <= 8 + k * 32768 and longest <= G.H.MAX_CODE_LEN and leaves <= G.MAX_LEAVES
        assert G.lane_chunks(window) == k + (window > k * 32768)
    for k, window, s in (cases[0], cases[1], cases[-1]):
        rc, back = O.decode("hufman", s)                                          # (the bytes behind the payload are not the decode's)
        assert rc == 0 and np.array_equal(back, G.wide_image()), (k, window)
    rc, back = O.decode("hufman", G.H.deep_stream())
    assert rc == 0 and _facts(G.H.deep_stream())[:2] == (21, G.H.MAX_CODE_LEN + 1)
    rc, back = O.decode("hufman", G.H.leafy_stream())
    assert rc == 0 and _facts(G.H.leafy_stream())[:2] == (100, 7)


def test_broken_streams_are_no_decoders():
    """the failures the GPU test says are handed back are streams the reference refuses, each with a whole header"""
    import test_small_trie_rgb_gpu as G
    rng = np.random.default_rng(7)
    im = rng.integers(0, 256, (9, 7, 3)).astype(np.uint8)
    rc, good, _ = O.encode("hufman", im)
    assert rc == 0 and O.decode("hufman", good)[0] == 0
    cases = {c[0]: c for c in G.H.failure_streams(good)}
    for name in ("cut in the trie", "a tag of 2", "a symbol of 4 bytes"):
        s = cases[name][1]
        assert len(s) >= 8 and s[:8] == good[:8] and O.decode("hufman", s)[0] == O.DECODE, name
    leaves, pay = G.H.parse_trie(good)
    assert len(cases["cut in the trie"][1]) < pay and len(cases["cut in the dimensions"][1]) < 8
    at = leaves[2][0] + 1
    assert int.from_bytes(good[at:at + 8], "little") == 3 and int.from_bytes(cases["a symbol of 4 bytes"][1][at:at + 8], "little") == 4
