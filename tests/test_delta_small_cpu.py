"""What the small-frame `delta` kernel computes per frame (cniic_amd/csrc/delta_small.hpp) and what tests/test_delta_small_batch.py relies
on, without a GPU.  tests/delta_small_check.cpp is compiled against the header as a stand-alone program: a scalar encoder built from the
header's functions (the merge in runs of 64 lanes, as one wave takes them) runs beside a plain restatement with a binary heap ordered by
(count, leaf before branch, key) on random symbol lists, 16 384 equal leaves, counts 1, 1, 2, 4, ..., 4096, Fibonacci counts, the strict
chain that meets the 19-bit bound, one and two leaves and runs of 2^k - 1 / 2^k / 2^k + 1 equal counts; the same program runs once more
under -fsanitize=address,undefined.  Then, from the oracle alone: every shaped frame of the GPU test has the distinct symbols, the
longest code and the stream length that test claims, and the further frames are what it says they are."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "delta_small_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "cniic_amd", "csrc")
PARTS = ("random", "all_ones", "powers", "fibonacci", "one", "two", "runs", "total")


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


def test_header_encoder_against_the_plain_restatement(tmp_path):
    import test_delta_small_batch as T
    exe = str(tmp_path / "delta_small_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    assert "longest code met %d, bound %d" % (T.MAX_CODE_LEN, T.MAX_CODE_LEN) in out
    assert "14 leaves, 8192 symbols, longest code 13" in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "delta_small_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_delta_small_batch as T
    hdr = open(os.path.join(CSRC, "delta_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kDeltaSmallMaxPx = %d;" % T.MAX_PX, hdr)
    assert re.search(r"constexpr uint32_t kDeltaSmallMaxCodeLen = %d;" % T.MAX_CODE_LEN, hdr)
    api = re.sub(r"(\d) (\d)", r"\1\2", open(os.path.join(os.path.dirname(HERE), "include", "cniic_hip.h")).read())
    assert "`delta` frames" in api and api.count("%d pixels" % T.MAX_PX) >= 2      # the cluster-colors paragraph and the delta one


def stream_facts(img):
    """(distinct symbols, longest code, bytes of the stream) of the oracle's `delta` stream, read off its pre-order trie"""
    rc, data, st = O.encode("delta", img)
    assert rc == 0
    h, w = img.shape[:2]
    assert int.from_bytes(data[0:4], "little") == w and int.from_bytes(data[4:8], "little") == h
    pos, leaves, longest, pending = 8, 0, 0, [0]       # pending: depths of the subtrees still to read
    while pending:
        depth = pending.pop()
        tag = data[pos]
        if tag == 1:
            pos += 1
            pending += [depth + 1, depth + 1]
        else:
            assert tag == 0
            pos += 7
            leaves += 1
            longest = max(longest, depth)
    return leaves, longest, len(data)


def test_shaped_frames_are_what_the_gpu_test_claims():
    import test_delta_small_batch as T
    imgs = T.shaped_images()
    assert [im.shape[:2] for im in imgs] == [(h, w) for w, h in T.SHAPES] and len(T.CLAIMS) == len(imgs)
    for im, (w, h), claim in zip(imgs, T.SHAPES, T.CLAIMS):
        if w * h <= T.ORACLE_MAX_PX:
            assert stream_facts(im) == claim, ((w, h), stream_facts(im), claim)
            syms = O.delta_diff(O.hilbert_linearize(im))
            assert len(np.unique(syms, axis=0)) == claim[0] and claim[1] <= T.MAX_CODE_LEN
    assert T.routed(imgs) == [True] * 11 + [False] * 2
    assert T.CLAIMS[T.SHAPES.index((128, 128))][0] >= 16000                     # uniform noise at the bound: nearly every symbol is a leaf
    assert T.routed(imgs, 4096) == [w * h <= 4096 for w, h in T.SHAPES]


def test_further_frames_are_what_the_gpu_test_says():
    import test_delta_small_batch as T
    black, flat, checker, flips, powers = T.further_images()
    assert stream_facts(black) == (1, 0, 15)
    assert stream_facts(flat) == (2, 1, 8 + 15 + (599 + 7) // 8)
    assert stream_facts(checker)[0] >= 2
    d = O.unpack_signed(O.delta_diff(O.hilbert_linearize(flips)))
    assert {tuple(v) for v in d.tolist()} == {(255, 255, 255), (-255, -255, -255)}
    assert powers.shape == (64, 128, 3)
    syms = O.delta_diff(O.hilbert_linearize(powers))
    counts = sorted(np.unique(syms, axis=0, return_counts=True)[1].tolist())
    assert counts == [1] + [1 << k for k in range(13)] and sum(counts) == 8192
    assert stream_facts(powers) == (14, 13, 8 + 8 * 14 - 1 + (2 * 8191 + 7) // 8)
    assert all(T.routed(T.further_images()))
