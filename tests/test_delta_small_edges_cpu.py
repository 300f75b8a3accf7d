"""That every frame of tests/delta_small_edges.py stands at the limit it is named for, without a GPU.  From the oracle alone: the distinct
symbols, the sorted counts, the longest code and the stream length are what CLAIMS states.  From the headers' own scalar encoder
(tests/delta_small_check.cpp --keys, the merge in runs of 64 lanes as one wave takes them, built plain and under
-fsanitize=address,undefined as tests/test_delta_small_cpu.py builds it): fed the oracle's keys it gives the oracle's stream byte for
byte, and its merge statistics are those of MERGE -- the 19-bit code, full and weight-cut runs in both queues, both orders of the
general step, 127 full leaf runs at 16 384 leaves.  That is the proof that tests/test_delta_small_edges.py reaches those branches in
the kernel, which is written from the same header functions."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import delta_small_edges as E
import oracle_lib as O
from test_delta_small_cpu import CSRC, SRC, _compiler, stream_facts


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the check program, plain and sanitized: (paths, a directory for the key files)"""
    d = tmp_path_factory.mktemp("delta_small_edges")
    plain, san = str(d / "delta_small_check"), str(d / "delta_small_check_san")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-I", CSRC, "-o", plain, SRC])
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", san, SRC])
    return (plain, san), d


def keys_mode(exe, d, name):
    """the program's second mode on the oracle's keys of one input -> (the stream it wrote, {line name: {field: value}})"""
    w, h = E.SHAPE[name]
    kf, of = str(d / (name + ".keys")), str(d / (name + ".stream"))
    E.oracle_keys(name).astype("<u4").tofile(kf)
    r = subprocess.run([exe, "--keys", kf, str(w), str(h), of], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, (name, r.stdout[-2000:])
    lines = {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "stream":
            lines["stream"] = dict(bytes=int(f[1]), crc=int(f[2], 16))
        else:
            lines[f[0]] = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
    with open(of, "rb") as fh:
        return fh.read(), lines


def sorted_counts(name):
    return sorted(np.unique(E.oracle_keys(name), return_counts=True)[1].tolist())


def test_every_input_is_what_its_claims_say():
    assert E.MAX_PX == 16384 and len(E.NAMES) == 6 + 2 * len(E.SIZES)
    for name in E.NAMES:
        img = E.image(name)
        w, h = E.SHAPE[name]
        assert img.shape == (h, w, 3) and 1 <= w * h <= E.MAX_PX, name
        facts = stream_facts(img)
        assert facts == E.CLAIMS[name] and facts[2] == len(E.oracle_stream(name)), (name, facts, E.CLAIMS[name])
        keys = E.oracle_keys(name)
        assert keys.size == w * h and np.unique(keys).size == facts[0] and facts[1] <= E.MAX_CODE_LEN, name


def test_the_named_inputs_reach_their_limits():
    # the chain: the header's list of counts, 20 leaves, the longest code the route's bound allows, on the generic scan
    assert sorted_counts("chain19") == sorted(E.CHAIN_COUNTS) and E.CLAIMS["chain19"][:2] == (20, E.MAX_CODE_LEN)
    d = O.unpack_signed(E.oracle_keys("chain19"))
    assert [tuple(v) for v in d.tolist()] == [tuple(v) for v in E.chain_diffs().tolist()]
    w, h = E.SHAPE["chain19"]
    assert w != h and w * h == 15126
    assert E.image("chain19").min() >= 122 and E.image("chain19").max() <= 134
    # every pixel its own symbol at the bound: ranks and head positions up to 2^14 - 1, 8192 leaf pairs
    assert E.SHAPE["all_distinct"] == (128, 128) and E.CLAIMS["all_distinct"][0] == E.MAX_PX and set(sorted_counts("all_distinct")) == {1}
    # the stairs: counts 1, 2, 3, 5, 11 and the heavy zero difference
    want = sorted([c for c, pairs in E.STAIRS for _ in range(2 * pairs)] + [2528])
    assert sorted_counts("stairs") == want and E.CLAIMS["stairs"][0] == 549 and E.SHAPE["stairs"] == (64, 64)
    # two symbols whose branch weighs 16384 = bit 14 of a 16-bit slot; one symbol; sixteen equal ones, all codes 4 bits
    assert sorted_counts("flat128") == [1, E.MAX_PX - 1] and bool((E.image("flat128") == 77).all())
    assert sorted_counts("black128") == [E.MAX_PX] and E.CLAIMS["black128"] == (1, 0, 15)
    assert sorted_counts("equal16") == [1024] * 16 and E.CLAIMS["equal16"][1] == 4
    assert E.CLAIMS["equal16"][2] == 8 + 8 * 16 - 1 + 4 * E.MAX_PX // 8 and (8 * (8 + 8 * 16 - 1)) % 32 == 24      # the payload starts at bit 24 of a word
    for nm in ("flat128", "black128", "equal16"):
        assert E.SHAPE[nm] == (128, 128)


def test_the_sizes_stand_around_the_capacity_and_the_span_switch():
    px = [w * h for w, h in E.SIZES]
    assert px == [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 8192, 16383, 16384, 16384]
    assert {E.MIN_CAP - 1, E.MIN_CAP, E.MIN_CAP + 1, E.THREADS - 1, E.THREADS, E.THREADS + 1, 2 * E.THREADS - 1, 2 * E.THREADS, 2 * E.THREADS + 1} <= set(px)
    squares = [(w, h) for w, h in E.SIZES if w == h and w & (w - 1) == 0]
    assert (8, 8) in squares and (32, 32) in squares                      # the table scan of 2^n squares
    assert {(16384, 1), (2, 8192), (64, 128)} <= set(E.SIZES)
    for w, h in E.SIZES:
        low, dis = "low_%dx%d" % (w, h), "distinct_%dx%d" % (w, h)
        assert E.CLAIMS[dis][0] == w * h and set(sorted_counts(dis)) == {1}, dis
        counts = sorted_counts(low)
        assert 5 <= len(counts) <= 6 and counts[0] == 1, low          # the first difference, against START, occurs once
        if w * h > 4 * E.THREADS:   # runs of one key in the sorted keys cross many threads' spans
            per = max(1, (1 << (w * h - 1).bit_length()) // E.THREADS)
            assert counts[-1] > 100 * per and counts[1] > 10 * per, low


def test_the_chunk_size_comes_from_the_library_s_constants(programs):
    import test_delta_small_batch as T
    assert (E.MAX_PX, E.MAX_CODE_LEN) == (T.MAX_PX, T.MAX_CODE_LEN)       # (tests/test_delta_small_cpu.py holds these to delta_small.hpp)
    hdr = open(os.path.join(CSRC, "delta_small.hpp")).read()
    assert "CNIIC_DS_HD uint32_t ds_subtree_bytes(uint32_t leaves) { return 8 * leaves - 1; }" in hdr
    assert "CNIIC_DS_HD uint64_t ds_header_bytes(uint64_t U) { return 8 + ds_subtree_bytes((uint32_t)U); }" in hdr
    assert "CNIIC_DS_HD uint64_t ds_stride(uint64_t n) { return (ds_stream_bytes(n, (uint64_t)kDeltaSmallMaxCodeLen * n) + 15) & ~15ull; }" in hdr
    out = subprocess.run([programs[0][0]], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "stride at the bound %d" % E.ds_stride(E.MAX_PX) in out
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    assert "static uint64_t delta_small_tmp_px(uint64_t npx) { return (npx + 3) & ~3ull; }" in src
    assert "static uint64_t delta_small_frame_bytes(uint64_t npx) { return ds_stride(npx) + 12 * delta_small_tmp_px(npx); }" in src
    assert "static uint64_t frame_px(const VarFrame &f) { return (uint64_t)f.w * f.h; }" in src
    assert "[](const VarFrame &first) { return (2ull << 30) / delta_small_frame_bytes(frame_px(first)); }" in src
    assert "const uint32_t cnt = (uint32_t)std::min<uint64_t>(n - at, std::max<uint64_t>(1, frames_that_fit(*fr[at])));" in src
    kern = open(os.path.join(CSRC, "k_delta_small.hip")).read()
    assert re.search(r"constexpr int kDsThreads = %d;" % E.THREADS, kern) and re.search(r"constexpr uint32_t kDsMinCap = %d;" % E.MIN_CAP, kern)
    assert E.ds_stride(E.MAX_PX) == 170000 and E.frame_bytes(E.MAX_PX) == 366608 and E.chunk_frames(E.MAX_PX) == 5857


def test_the_short_streams_of_the_chunk_and_placement_tests():
    lens = [len(O.encode("delta", im)[1]) for im in E.chunk_kinds()]
    assert lens[0] == E.CLAIMS["flat128"][2] and lens[-1] == 15 and len(set(lens)) >= 6      # (1 x 1: one symbol)
    assert [im.shape[0] * im.shape[1] for im in E.chunk_kinds()[1:]] == [12, 9, 7, 5, 4, 3, 2, 1]
    assert len(np.unique(O.delta_diff(O.hilbert_linearize(E.chunk_kinds()[4])))) > 1           # the second chunk's first frame has a tree
    # the two-chunk call: one frame at the bound fills the first chunk with chunk_frames(16384) frames; the rest begins among the 5-pixel frames
    rest = 1 + sum(E.TINY_COUNT) - E.chunk_frames(E.MAX_PX)
    assert sum(E.TINY_COUNT) == 5900 and sum(E.TINY_COUNT[4:]) < rest <= sum(E.TINY_COUNT[3:]) and rest < E.chunk_frames(5)
    assert tuple(len(O.encode("delta", im)[1]) for im in E.placement_kinds()) == E.PLACEMENT_LENGTHS
    assert len(E.placement_kinds()) % 2 == 1      # coprime to 16: cycled over 16 x 7 frames under an odd stride, every kind meets every residue


@pytest.mark.parametrize("build", (0, 1), ids=("plain", "sanitized"))
def test_the_headers_encoder_gives_the_oracle_s_stream_and_the_merge_claimed(programs, build):
    exes, d = programs
    for name in E.NAMES:
        data, lines = keys_mode(exes[build], d, name)
        want = E.oracle_stream(name)
        assert data == want and lines["stream"] == dict(bytes=len(want), crc=zlib.crc32(want)), name
        U, longest, nbytes = E.CLAIMS[name]
        assert lines["tree"] == dict(leaves=U, longest=longest), (name, lines["tree"])
        assert lines["general"]["leaf_leaf"] == 0 and lines["general"]["branch_branch"] == 0, name    # a general step is a leaf and a branch
        if name in E.MERGE:
            m = E.MERGE[name]
            for line in ("leaf_runs", "branch_runs", "general", "payload"):
                got = {k: lines[line][k] for k in m[line]}
                assert got == m[line], (name, line, got, m[line])
        if name.startswith("distinct_"):      # all leaves tie: whole waves of pairs, no weight test ever cuts one
            assert lines["leaf_runs"]["full"] == (U - 2) // 128 and lines["leaf_runs"]["cut"] == 0 and lines["branch_runs"]["cut"] == 0, name
    # what each named input is named for
    M = E.MERGE
    assert M["all_distinct"]["leaf_runs"] == dict(full=127, cut=0, queue=1, single=1) and M["all_distinct"]["branch_runs"]["full"] == 127
    s = M["stairs"]
    assert s["leaf_runs"]["full"] >= 1 and s["leaf_runs"]["cut"] >= 1 and s["branch_runs"]["full"] >= 1 and s["branch_runs"]["cut"] >= 1
    assert s["branch_runs"]["queue"] >= 1 and s["general"]["leaf_branch"] >= 1 and s["general"]["branch_leaf"] >= 1
    assert M["chain19"]["general"]["leaf_branch"] == 18                   # one leaf pair, then a leaf and the branch so far, 18 times: depth 19
    assert M["equal16"]["payload"] == dict(threads=E.THREADS, word_ends=0, most_bits=64)   # every thread: 16 codes of 4 bits from bit 24 on
