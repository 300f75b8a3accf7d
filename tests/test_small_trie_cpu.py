"""What the small-decoder parse kernel computes per frame (cniic_amd/csrc/small_trie.hpp) and what tests/test_small_trie_gpu.py relies on,
without a GPU.  tests/small_trie_check.cpp is compiled against the header as a stand-alone program: a scalar parser made of the header's
functions, lanes and chunks in the kernel's order, beside a byte-by-byte stack parse, on tries the program builds; the same program runs
once more under -fsanitize=address,undefined.  Then the constants the header, the GPU test and delta_small_dec.hpp share, and, from the
oracle alone, what the GPU test's hand-built streams are."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "small_trie_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
PARTS = ("words", "small", "chains", "bound", "random", "offsets", "lengths", "mutations", "symbols", "total")


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
    import test_small_trie_gpu as G
    exe = str(tmp_path / "small_trie_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    assert "constants: leaves %d, lanes 1024, chunk %d, window %d, rows %d" % (G.MAX_LEAVES, G.CHUNK, 8 * G.MAX_LEAVES - 1, G.T.MAX_CODE_LEN + 1) in out
    assert "%d leaves parsed, %d not ours" % (G.MAX_LEAVES, G.MAX_LEAVES + 1) in out
    assert "60 tries parsed, up to %d leaves" % G.MAX_LEAVES in out
    assert "%d edits" % (55 * 255) in out and "for k = 1, 2, %d" % ((8 * G.MAX_LEAVES - 1) // G.CHUNK) in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "small_trie_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_small_trie_gpu as G
    hdr = open(os.path.join(CSRC, "small_trie.hpp")).read()
    dec = open(os.path.join(CSRC, "delta_small_dec.hpp")).read()
    assert re.search(r"constexpr uint32_t kSmallTrieMaxLeaves = %d;" % G.MAX_LEAVES, hdr)
    assert re.search(r"constexpr uint32_t kStChunk = %d;" % G.CHUNK, hdr)
    assert re.search(r"constexpr uint32_t kStMaxP = kDeltaSmallMaxCodeLen;", hdr)
    assert re.search(r"constexpr uint32_t kDeltaSmallDecMaxPx = %d;" % G.MAX_LEAVES, dec) and G.MAX_LEAVES == G.T.MAX_PX
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    for name in (G.PARSE, G.PARSE_HOST, G.KNOB, G.T.TIMER):
        assert '"%s"' % name in src, name
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    assert G.PARSE in api and G.PARSE_HOST in api


def _facts(data):
    import test_small_trie_gpu as G
    leaves, pay = G.T.parse_trie(data)
    return len(leaves), max(d for _, d in leaves), pay


def test_hand_built_decoders_are_what_the_gpu_test_says():
    import test_small_trie_gpu as G
    for leaves, longest in ((G.MAX_LEAVES + 1, 15), (100, 7)):
        s = G.wide_stream(leaves)
        assert _facts(s) == (leaves, longest, 8 + 8 * leaves - 1) and len(s) > 8 + 8 * leaves - 1      # whole, and a payload behind it
        rc, back = O.decode("delta", s)
        assert rc == 0 and np.array_equal(back, G.wide_image()), leaves
    rc, back = O.decode("delta", G.T.deep_stream())
    assert rc == 0 and np.array_equal(back, G.wide_image()) and _facts(G.T.deep_stream())[:2] == (21, G.T.MAX_CODE_LEN + 1)


def test_broken_streams_are_no_decoders():
    import test_small_trie_gpu as G
    rc, good, _ = O.encode("delta", G.T.range_image())
    assert rc == 0 and O.decode("delta", good)[0] == 0
    leaves, pay = G.T.parse_trie(good)
    for name, s in G.broken_streams(good):
        assert len(s) >= 8 and s[:8] == good[:8], name                                 # a whole header: a candidate of the parse
        assert O.decode("delta", s)[0] == O.DECODE, name
        if name.startswith("cut"):
            assert len(s) < pay
        else:
            assert len(s) == len(good)
    cut = dict(G.broken_streams(good))
    assert good[8] == 1 and len(cut["cut behind a branch"]) == 9
    first = leaves[0][0]
    assert first <= len(cut["cut inside a leaf"]) < first + 6
    assert cut["a tag of 2"][first - 1] == 2 and good[first - 1] == 0
    assert int.from_bytes(cut["a symbol of 256"][first:first + 2], "little", signed=True) == 256


def test_library_frames_stay_below_the_parse_s_bounds():
    """no stream of the frames the GPU test says are parsed there has more leaves than pixels, or a code longer than 19 bits"""
    import test_small_trie_gpu as G
    for f, im in enumerate(G.T.route_images()):
        rc, data, _ = O.encode("delta", im)
        assert rc == 0
        leaves, longest, pay = _facts(data)
        assert leaves <= min(G.MAX_LEAVES, im.shape[0] * im.shape[1]) and longest <= G.T.MAX_CODE_LEN and pay == 8 + 8 * leaves - 1, f
