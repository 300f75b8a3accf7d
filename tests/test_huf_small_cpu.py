"""What the small-frame `hufman` kernel computes per frame (cniic_amd/csrc/huf_small.hpp beside delta_small.hpp) and what
tests/test_huf_small_batch.py relies on, without a GPU.  tests/huf_small_check.cpp is compiled against the headers as a stand-alone program:
a scalar encoder built from the headers' functions (the key, the merge in runs of 64 lanes as one wave takes them, the walks, the leaf
bytes, the sizes) runs beside a plain restatement that compares colours as (r, g, b), keeps a binary heap ordered by (count, leaf before
branch, colour) and serialises byte by byte, on random pixel lists, 16 384 equal leaves, counts 1, 1, 2, 4, ..., 4096, the strict chain
that meets the 19-bit bound, one and two leaves, runs of 2^k - 1 / 2^k / 2^k + 1 equal counts and four equally frequent colours whose
order differs between r-major and b-major keys; the same program runs once more under -fsanitize=address,undefined.  Then, from the oracle
alone: every frame of the GPU test has the distinct colours, the longest code and the stream length that test claims."""
import os
import re
import shutil
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "huf_small_check.cpp")
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
PARTS = ("random", "all_ones", "powers", "chain", "one", "two", "runs", "byte_order", "decode", "total")


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
    src.write_text('#include "huf_small.hpp"\nint main() { return cniic::hs_stride(cniic::kHufSmallMaxPx) == 251920 ? 0 : 1; }\n')
    exe = str(tmp_path / "alone")
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.call([exe]) == 0


def test_header_encoder_against_the_plain_restatement(tmp_path):
    import test_huf_small_batch as T
    exe = str(tmp_path / "huf_small_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", exe, SRC])
    out = _run(exe)
    assert "longest code met %d, bound %d, stride at the bound %d" % (T.MAX_CODE_LEN, T.MAX_CODE_LEN, T.STRIDE_AT_BOUND) in out
    assert "ok chain: 20 leaves, 15126 pixels, longest code 19 (the bound: 19), 5215 bytes; a 21st count makes 24475 pixels" in out
    assert "ok powers: 14 leaves, 8192 pixels, longest code 13, 2237 bytes" in out
    assert "ok all_ones: 16384 leaves, every code 14 bits, 241671 bytes" in out
    assert "ok one: 20 bytes, no payload" in out


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "huf_small_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC])
    _run(exe)


def test_the_constants_the_tests_restate_are_the_library_s():
    import test_delta_small_batch as D
    import test_huf_small_batch as T
    hdr = open(os.path.join(CSRC, "huf_small.hpp")).read()
    assert re.search(r"constexpr uint32_t kHufSmallMaxPx = %d;" % T.MAX_PX, hdr)
    assert "CNIIC_DS_HD uint32_t hs_subtree_bytes(uint32_t leaves) { return 13 * leaves - 1; }" in hdr
    assert "CNIIC_DS_HD uint64_t hs_stride(uint64_t n) { return (hs_stream_bytes(n, (uint64_t)kDeltaSmallMaxCodeLen * n) + 15) & ~15ull; }" in hdr
    assert (T.MAX_PX, T.MAX_CODE_LEN) == (D.MAX_PX, D.MAX_CODE_LEN)       # (tests/test_delta_small_cpu.py holds these to delta_small.hpp)
    n = T.MAX_PX
    assert T.STRIDE_AT_BOUND == (8 + 13 * n - 1 + (T.MAX_CODE_LEN * n + 7) // 8 + 15) // 16 * 16 == 251920
    kern = open(os.path.join(CSRC, "k_delta_small.hip")).read()
    assert re.search(r"constexpr int kDsThreads = %d;" % T.THREADS, kern) and "void k_huf_small(" in kern and "void k_delta_small(" in kern
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    assert "return hs_stride(npx) + 12 * delta_small_tmp_px(npx) + sizeof(DeltaSmallRow) + sizeof(DeltaSmallResult); }" in src
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert re.search(r"constexpr uint32_t kHufSmallFloorFew = %d;" % T.FLOOR_FRAMES, capi) and re.search(r"constexpr uint64_t kHufSmallFloorPxFew = %d;" % T.FLOOR_PX, capi)
    assert re.search(r"constexpr uint32_t kHufSmallDecFloorFrames = %d;" % T.DEC_FLOOR_FRAMES, src)
    api = re.sub(r"(\d) (\d)", r"\1\2", open(os.path.join(ROOT, "include", "cniic_hip.h")).read())
    assert "`hufman` frames" in api and "huf_small_batch" in api and "huf_small_place" in api and "huf_small_dec_batch" in api
    assert api.count("%d pixels" % T.MAX_PX) >= 3      # the cluster-colors paragraph, the delta one and this one


def stream_facts(img):
    """(distinct colours, longest code, bytes of the stream) of the oracle's `hufman` stream, read off its pre-order trie"""
    rc, data, st = O.encode("hufman", img)
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
            assert tag == 0 and int.from_bytes(data[pos + 1:pos + 9], "little") == 3
            pos += 12
            leaves += 1
            longest = max(longest, depth)
    assert pos == 8 + 13 * leaves - 1
    return leaves, longest, len(data)


def _colours(img):
    return np.unique(img.reshape(-1, 3), axis=0, return_counts=True)


def test_shaped_frames_are_what_the_gpu_test_claims():
    import test_huf_small_batch as T
    imgs = T.shaped_images()
    assert [im.shape[:2] for im in imgs] == [(h, w) for w, h in T.SHAPES] and len(T.CLAIMS) == len(imgs)
    for im, (w, h), claim in zip(imgs, T.SHAPES, T.CLAIMS):
        assert stream_facts(im) == claim, ((w, h), stream_facts(im), claim)
        assert len(_colours(im)[0]) == claim[0]
        assert claim[1] <= T.MAX_CODE_LEN or w * h > T.MAX_PX
    assert T.routed(imgs) == [True] * 11 + [False] * 2
    assert [w * h for w, h in T.SHAPES[-2:]] == [16385, 19200]
    assert T.routed(imgs, 4096) == [w * h <= 4096 for w, h in T.SHAPES]


def test_further_frames_are_what_the_gpu_test_says():
    import test_huf_small_batch as T
    imgs = dict(zip(T.FURTHER, T.further_images()))
    for name in T.FURTHER:
        assert stream_facts(imgs[name]) == T.FURTHER_CLAIMS[name], (name, stream_facts(imgs[name]))
    assert all(T.routed(list(imgs.values())))
    # the chain: branch k = branch k - 1 + branch k - 2 + 1, leaf k + 2 = branch k - 1 + 1; a 21st count leaves the route
    br, chain = [2, 3], [1, 1, 1]
    while len(chain) < 21:
        chain.append(br[-2] + 1)
        br.append(br[-1] + br[-2] + 1)
    assert chain[:20] == T.CHAIN and sum(T.CHAIN) == 15126 == 6 * 2521 and sum(chain) == 24475 > T.MAX_PX
    assert sorted(_colours(imgs["chain"])[1].tolist()) == T.CHAIN
    assert sorted(_colours(imgs["powers"])[1].tolist()) == [1] + [1 << k for k in range(13)] and imgs["powers"].shape == (64, 128, 3)
    assert len(_colours(imgs["distinct"])[0]) == 16384 and set(_colours(imgs["distinct"])[1].tolist()) == {1}
    assert imgs["one_pixel"].shape == (1, 1, 3) and imgs["flat"].shape == (30, 20, 3)
    assert {tuple(c) for c in _colours(imgs["ends"])[0].tolist()} == {(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255)}
    # four equally frequent colours: the leaves lie in the trie by r, then g, then b -- not by b first
    cols, counts = _colours(imgs["byte_order"])
    assert set(counts.tolist()) == {5}
    data = O.encode("hufman", imgs["byte_order"])[1]
    leaves = [tuple(data[8 + at + 9:8 + at + 12]) for at in (2, 14, 27, 39)]       # pre-order 1 1 L L 1 L L
    assert leaves == [(0, 0, 1), (0, 0, 2), (0, 3, 0), (1, 0, 0)] != sorted(leaves, key=lambda c: c[::-1])


def test_sized_and_many_frames_are_what_the_gpu_test_says():
    import test_huf_small_batch as T
    px = [w * h for w, h in T.SIZES]
    assert px == [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16384, 16384]
    for im in T.sized_images():
        U, longest, nbytes = stream_facts(im)
        assert longest <= T.MAX_CODE_LEN and nbytes <= (8 + 13 * U - 1 + (T.MAX_CODE_LEN * im.shape[0] * im.shape[1] + 7) // 8)
    many = T._many()
    assert len(many) == 3000 and len({im.shape[:2] for im in many}) == 8
    assert max(len(_colours(im)[0]) for im in many[::50]) <= 64
