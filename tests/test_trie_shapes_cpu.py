"""What the hand-built streams of tests/trie_shapes.py are, without a GPU: from the oracle alone (its verdict, its pixels) and from the
plain Python parse (the geometry every case is named for), so that tests/test_trie_shapes.py can say which limit of k_trieparse.hip a
failing case sits on.  Then the host's own readers of a serialised decoder (huff_parse_leaves, huff_parse_trie, huff_decode_host of
cniic_amd/csrc/huff_host.cpp) over the same streams as a stand-alone program, tests/trie_shapes_check.cpp, plain and under
-fsanitize=address,undefined; and the constants these tests restate against the sources.

If an assertion about a case's geometry fails, the case is to be mended, not the assertion: it is what puts the case on its limit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import trie_shapes as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_constants_the_tests_restate_are_the_library_s():
    tp, hh, hc, cc = _src("cniic_amd", "csrc", "k_trieparse.hip"), _src("cniic_amd", "csrc", "huff_host.hpp"), _src("cniic_amd", "csrc", "huff_host.cpp"), _src("cniic_amd", "csrc", "codec.cpp")
    assert "constexpr uint32_t kTpChunk = %d;" % S.CHUNK in tp
    assert "constexpr uint32_t kTpMaxP = %d;" % S.MAX_P in tp
    assert "constexpr uint32_t kTpB = %d;" % S.BATCH in tp
    assert "constexpr uint32_t kLeafMaxLen = %d;" % S.MAX_LEN in hh
    assert "__launch_bounds__(%d) void k_tp_chain_entries" % S.CHAIN in tp and "const uint32_t G = (nchunks + %d) / %d;" % (S.CHAIN - 1, S.CHAIN) in tp
    assert "const uint32_t nblk = ceil_div(nchunks, %du);" % S.CHAIN in tp
    assert "(j & %du)" % (S.GROUP - 1) in tp and "(k & %du)" % (S.GROUP - 1) in tp and "k * %d + lane" % S.GROUP in tp
    assert "case CNIIC_SYM_RGB: return %d;" % (S.R_RGB - 1) in hc and "case CNIIC_SYM_SIGNED: return %d;" % (S.R_SIGNED - 1) in hc
    assert "const int R = 1 + huff_symbol_size(sym_kind);" in tp
    assert "std::min<uint64_t>(std::max<uint64_t>(nbytes / 48, 8192), 4ull << 20)" in cc and S.first_look(10 ** 6) == 20833 and S.first_look(10) == 8192
    assert '"CNIIC_GPU_DECODE_MIN", 1ull << 14)' in cc and S.MIN_SYMS == 1 << 14
    api, readme = _src("include", "cniic_hip.h"), _src("README.md")
    for name in (S.PARSE, S.PARSE_HOST):
        assert '"%s"' % name in cc and '"%s"' % name in api and "`%s`" % name in readme, name
    for knobs in S.KNOBS:
        for k in knobs:
            assert '"%s"' % k in _src("cniic_amd", "csrc", "k_hdecode.hip") or '"%s"' % k in cc, k


def _depths(shape):
    return [d for d, _ in S.walk(shape)[1]]


def test_the_builders_build_what_they_say():
    assert _depths(S.right_comb(6)) == [1, 2, 3, 4, 5, 5] and S.walk(S.right_comb(6))[0] == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0]
    assert _depths(S.left_comb(6)) == [5, 5, 4, 3, 2, 1] and S.walk(S.left_comb(6))[0] == [1] * 5 + [0] * 6
    assert _depths(S.balanced(5)) == [3, 3, 2, 2, 2] and _depths(S.balanced(3, 8)) == _depths(S.balanced(5)) and _depths(S.balanced(1)) == [0]
    assert S.walk(S.over(3, S.balanced(5)))[0] == [1] * 3 + S.walk(S.balanced(5))[0] + [0] * 3
    assert _depths(S.graft(S.right_comb(4), S.balanced(2))) == [1, 2, 3, 4, 4] and _depths(S.graft(S.left_comb(4), S.balanced(2))) == [3, 4, 4, 2, 1]
    assert _depths(S.beside(S.left_comb(3), 2)) == [2, 2, 3, 3, 2]
    for cap in (13, 20, 56):
        d = _depths(S.random_shape(5000, 7, 8, cap=cap))
        assert len(d) == 5000 and max(d) == cap and abs(sum(2.0 ** -x for x in d) - 1) < 1e-9
    assert max(_depths(S.random_shape(64, 1, 8, cap=6))) == 6
    # a stream: the codes of the leaves in pre-order ascend, the payload is theirs
    s = S.Stream("hufman", S.right_comb(3), dims=(2, 2), colours=[0x010203, 0x040506, 0x070809])
    assert s.data == bytes([2, 0, 0, 0, 2, 0, 0, 0, 1, 0, 3, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 1, 0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 5, 6, 0, 3, 0, 0, 0, 0, 0, 0, 0, 7, 8, 9,
                             0b01011000])
    assert s.image.tolist() == [[[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [1, 2, 3]]] and s.keys().tolist() == [0x010203, 0x040506, 0x070809, 0x010203]
    f = S.parse(s.data, s.R)
    assert f.leaves == [(9, 1), (22, 2), (34, 2)] and f.payload == 46 == s.payload_pos and f.right == [2, -1, 4, -1, -1] and f.max_p == 2 and f.entries == [0]
    d = S.Stream("delta", S.balanced(3), dims=(2, 2))
    assert d.syms == [(1, 0, 0), (-1, 0, 0), (0, 0, 0)] and d.data[8:] == b"\1\1\0\1\0\0\0\0\0\0\xff\xff\0\0\0\0\0\0\0\0\0\0\0" + bytes([0b00011000])


def _check_good(name, s):
    """the oracle decodes it to the image built from the payload; every leaf occurs in the payload; the parse finds what was built"""
    rc, px = O.decode(s.codec, s.data)
    assert rc == 0, name
    if s.image is not None:
        assert np.array_equal(px, s.image), name
    assert px.shape == (s.h, s.w, 3) and len(s.seq) == s.w * s.h
    assert np.array_equal(np.unique(s.seq), np.arange(s.leaves)), name
    f = S.parse(s.data, s.R)
    assert (len(f.leaves), f.deepest, f.payload, f.nodes) == (s.leaves, s.deepest, s.payload_pos, 2 * s.leaves - 1), name
    assert s.on_gpu == (f.deepest <= S.MAX_LEN)
    return f


@pytest.fixture(scope="module")
def facts():
    out = {}
    for cases in (S.good_hufman(), S.good_delta()):
        for name, s in cases.items():
            out[name] = _check_good(name, s)
    return out


def _straddles(o, R):
    return (o - S.POS0) // S.CHUNK != (o - S.POS0 + R - 1) // S.CHUNK


def test_entry_offsets(facts):
    g = S.geometry_cases()
    for fam, natural in (("entry over(%d)", False), ("entry over(%d), 700 leaves", True)):
        seen = set()
        for k in range(13):
            s, f = g[fam % k], facts[fam % k]
            assert s.data[8:8 + k + 1] == b"\x01" * (k + 1) and f.leaves[0][0] == facts[fam % 0].leaves[0][0] + k      # every record k bytes later
            assert len(f.entries) >= 6 and S.straddlers(f, s.R) and s.natural == natural
            seen |= set(f.entries[1:])                     # the offsets at which chunks 1 .. are entered
        assert seen == set(range(S.R_RGB)), fam
    d = S.good_delta()
    seen = set()
    for k in range(8):
        f = facts["delta entry over(%d)" % k]
        assert len(f.entries) == 5 and S.straddlers(f, S.R_SIGNED)
        seen |= set(f.entries[1:])
    assert seen == set(range(S.R_SIGNED)) and all(not s.natural for s in d.values())


def test_trie_ends_against_a_chunk_boundary(facts):
    g = S.geometry_cases()
    for r, n in enumerate(S.END_LEAVES):
        s, f = g["end %d leaves" % n], facts["end %d leaves" % n]
        assert s.trie_len == 13 * n - 1 and s.trie_len % S.CHUNK == r
        assert _straddles(f.leaves[-1][0], s.R) == (r > 0), n            # the last record lies across the boundary; at r = 0 it ends on it
        assert s.natural == (s.trie_len + 8 > 8192)
    assert g["end 709 leaves"].payload_pos - S.POS0 == 9216 and len(facts["end 709 leaves"].entries) == 9     # the payload opens chunk 9
    assert [g["end %d leaves" % n].trie_len % S.CHUNK for n in (708, 710)] == [S.CHUNK - 13, 13]
    assert [g["short %d leaves" % n].trie_len for n in (1, 2, 78, 79)] == [12, 25, 1013, 1026]
    # (78 leaves end 11 bytes short of the chunk; the last record of 79 reaches two bytes into chunk 1, which holds no tag)
    assert [_straddles(facts["short %d leaves" % n].leaves[-1][0], S.R_RGB) for n in (1, 2, 78, 79)] == [False, False, False, True]
    assert all(len(facts["short %d leaves" % n].entries) == 1 for n in (1, 2, 78, 79))
    assert g["short 1 leaves"].deepest == 0 and len(g["short 1 leaves"].data) == 8 + 12                        # one leaf: no payload at all


def test_chunk_counts(facts):
    c = S.chunk_count_cases()
    assert len(c) == 9
    spans = sorted(len(s.data) - S.POS0 for s in c.values())
    assert spans == sorted([n * S.CHUNK + m for n in S.CHUNK_COUNTS for m in (0, 1)] + [8193 * S.CHUNK])
    per_thread = {n: -(-n // S.CHAIN) for n in (1024, 1025, 8192, 8193, 8194)}         # G of k_tp_chain_entries; nchunks = ceil(span / 1024)
    assert per_thread == {1024: 1, 1025: 2, 8192: S.BATCH, 8193: S.BATCH + 1, 8194: S.BATCH + 1}
    assert [-(-n // S.CHAIN) for n in (1024, 1025)] == [1, 2]                            # the blocks of k_tp_bases_*
    for name, s in c.items():
        f = facts[name]
        nchunks = -(-(len(s.data) - S.POS0) // S.CHUNK)
        trie_chunks = len(f.entries)
        assert trie_chunks == 102 and s.leaves == 8000
        if nchunks >= 8193:
            assert -(-trie_chunks // per_thread[8193]) >= 10                             # the trie lies across at least ten threads of the chain
        # natural: the 1 MiB spans; at 8 MiB the host's first look (nbytes / 48) holds the whole decoder: the hook's runs only
        assert s.natural == (nchunks <= 1026), name
        assert set(s.data[-5000:]) == {int(name.endswith("with 1"))}, name
    assert sum(name.endswith("with 1") for name in c) == 1


def test_right_children(facts):
    c = S.search_cases()
    for n in S.RIGHT_N:
        f = facts["right child at node %d" % (2 * n)]
        assert f.right[0] == 2 * n and f.right[1] == (2 * ((n + 1) // 2) + 1 if n > 1 else -1)
        assert c["right child at node %d" % (2 * n)].natural == (n >= 2047)
        if n < 2047:
            name = "right child at node %d, 700 leaves behind" % (2 * n)
            assert facts[name].right[0] == 2 * n and c[name].natural
    assert [2 * n for n in S.RIGHT_N[1::3]] == [S.GROUP, S.GROUP ** 2, S.GROUP ** 3]
    assert [facts["delta right child at node %d" % m].right[0] for m in (64, 4096)] == [S.GROUP, S.GROUP ** 2]
    left, right = facts["left comb over 3000"], facts["right comb over 3000"]
    assert left.deepest == right.deepest == S.MAX_LEN and left.nodes == right.nodes == 2 * 3044 - 1 > S.GROUP ** 2
    assert left.right[0] == left.nodes - 1                 # the root's right child is the last node: the search runs through every level to the end
    assert all(left.right[i] == left.nodes - 1 - i for i in range(S.COMB_LEAVES - 2))
    assert all(right.right[2 * i] == 2 * i + 2 for i in range(S.COMB_LEAVES - 2))    # right children at distance 2
    assert c["left comb over 3000"].natural and c["right comb over 3000"].natural
    rnd = S.random_shapes()
    assert len(rnd) >= 4 and any(d == S.MAX_LEN for _, _, _, d in rnd) and all(50 <= d <= S.MAX_LEN for _, _, _, d in rnd)
    assert all(c["random seed %d skew %d" % (seed, skew)].natural for seed, skew, _, _ in rnd)
    twice = c["a colour twice"]
    assert twice.syms == [5, 6, 5, 7] and twice.leaves == 4 and len(np.unique(twice.image.reshape(-1, 3), axis=0)) == 3


def test_depth_limits(facts):
    c = S.depth_cases()
    assert len(c) == 4 * len(S.DEPTHS) and {S.MAX_LEN, S.MAX_LEN + 1, S.MAX_P - 1, S.MAX_P, S.MAX_P + 1} <= set(S.DEPTHS)
    for kind in ("right", "left"):
        for d in S.DEPTHS:
            for name in ("%s comb %d" % (kind, d), "%s comb %d beside 700" % (kind, d)):
                s, f = c[name], facts[name]
                assert f.deepest == d and s.on_gpu == (d <= S.MAX_LEN), name
                deep = s.seq[0]
                assert s.seq[-1] == deep and f.leaves[deep][1] == d          # the payload starts and ends with the deepest leaf
                assert s.natural == name.endswith("700") and (s.w * s.h == 128 * 128) == s.natural, name
                # the parser's stack: a left comb's grows with its depth, a right comb's never (12: the balanced trie of 700 in front)
                # (alone, the root is the comb's: d + 1 subtrees are open in front of its deepest leaf; beside 700 leaves, d)
                assert f.max_p == ((d + 1 if not s.natural else d) if kind == "left" else 2 if not s.natural else 12), name
                if s.natural:
                    # the comb lies behind what the host looks at first: the host cannot find it too deep by itself
                    assert f.leaves[700][0] - 1 > S.first_look(len(s.data)) and max(dd for _, dd in f.leaves[:700]) == 11
    assert facts["left comb 119"].max_p == S.MAX_P and facts["left comb 120"].max_p == S.MAX_P + 1
    assert facts["left comb 120 beside 700"].max_p == S.MAX_P and facts["left comb 121 beside 700"].max_p == S.MAX_P + 1
    # only these push the stack past kTpMaxP
    deep_stack = {n for n, f in facts.items() if f.max_p > S.MAX_P}
    assert deep_stack == {"left comb %d" % d for d in S.DEPTHS if d >= S.MAX_P} | {"left comb %d beside 700" % d for d in S.DEPTHS if d > S.MAX_P}
    k = S.knob_cases()
    assert len(k) == 3 and all(s.deepest == S.MAX_LEN for s in k.values()) and sum(n.startswith("random") for n in k) == 1
    for kind in ("right", "left"):
        assert [facts["delta %s comb %d" % (kind, d)].deepest for d in (56, 57)] == [S.MAX_LEN, S.MAX_LEN + 1]


def test_which_cases_meet_the_natural_gate():
    g = S.good_hufman()
    natural = [n for n, s in g.items() if s.natural]
    assert len(natural) >= 60 and len(g) - len(natural) >= 40
    for n in natural:
        s = g[n]
        assert s.w * s.h >= S.MIN_SYMS and s.payload_pos > max(len(s.data) // 48, 8192) and len(s.data) // 48 < 4 << 20


def test_malformed_streams_and_cuts():
    base = S.malformed_base()
    f = S.parse(base.data, base.R)
    assert len(f.entries) == 6 and S.straddlers(f, base.R) and base.leaves == 403
    cases = S.malformed_hufman()
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names) == 2 * (2 + 2 * 5) + 8 + 12 + 25 * 5 + 4
    for name, data in cases:
        rc, px = O.decode("hufman", data)
        assert (rc == 0) == (name == "one more leaf behind the trie"), name      # bytes behind a complete trie are payload
        if rc == 0:
            assert not np.array_equal(px, base.image)
    # every edit hits what it names
    edits = dict(cases)
    bounds = [S.POS0 + S.CHUNK * c for c in range(1, 6)]
    tags = S.tag_offsets(f, base.R)
    assert len(tags) == f.nodes and all(base.data[t] < 2 for t in tags)
    for b in bounds:
        before, after = edits["tag 2 in the last tag before %d" % b], edits["tag 255 in the first tag from %d" % b]
        at = next(i for i in range(len(base.data)) if before[i] != base.data[i])
        assert at < b and before[at] == 2 and at in tags and not any(at < t < b for t in tags)
        at = next(i for i in range(len(base.data)) if after[i] != base.data[i])
        assert b <= at < b + S.R_RGB and after[at] == 255 and at - b == f.entries[(b - S.POS0) // S.CHUNK]
    assert len(edits["cut behind the trie"]) == f.payload and edits["a trie that never ends"][8:] == b"\x01" * 2000
    d = S.malformed_delta()
    db = S.delta_base()
    assert O.decode("delta", db.data)[0] == 0 and len(d) == 2 * 3 * 2 + S.R_SIGNED
    assert len(S.straddlers(S.parse(db.data, db.R), db.R)) >= 2
    for name, data in d:
        assert O.decode("delta", data)[0] == O.DECODE, name


# ------------------------------------------------------------------ the host's parsers over the same streams, as a program
def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def stream_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("trie_shapes")
    lines = []

    def put(data, kind, nsyms, leaves, deepest, payload, verdict, keys):
        name = "s%04d.bin" % len(lines)
        (d / name).write_bytes(data)
        kname = "-"
        if keys is not None:
            kname = name + ".keys"
            (d / kname).write_bytes(np.ascontiguousarray(keys, "<u4").tobytes())
        lines.append("%s %d %d %d %d %d %d %s" % (name, kind, nsyms, leaves, deepest, payload, verdict, kname))

    for cases in (S.good_hufman(), S.good_delta()):
        for name, s in cases.items():
            put(s.data, O.SYM_RGB if s.codec == "hufman" else O.SYM_SIGNED, s.w * s.h, s.leaves, s.deepest, s.payload_pos, 1, s.keys())
    for codec, cases, base in (("hufman", S.malformed_hufman(), S.malformed_base()), ("delta", S.malformed_delta(), S.delta_base())):
        for name, data in cases:
            put(data, O.SYM_RGB if codec == "hufman" else O.SYM_SIGNED, base.w * base.h, 0, 0, 0, int(O.decode(codec, data)[0] == 0), None)
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    return str(d), len(lines)


def _build_and_run(tmp_path, stream_dir, flags):
    exe = str(tmp_path / "trie_shapes_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17"] + flags + ["-I", CSRC, "-o", exe, os.path.join(HERE, "trie_shapes_check.cpp"), os.path.join(CSRC, "huff_host.cpp")])
    d, n = stream_dir
    r = subprocess.run([exe, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-4000:]
    good = len(S.good_hufman()) + len(S.good_delta()) + 1                       # (and the stream with one more leaf)
    deep = sum(not s.on_gpu for c in (S.good_hufman(), S.good_delta()) for s in c.values())
    assert "constants: kLeafMaxLen %d" % S.MAX_LEN in r.stdout
    assert "%d streams: %d good (%d too deep for the table, the deepest leaf at 300, up to 131173 leaves), %d refused, 0 failures" % (n, good, deep, n - good) in r.stdout, r.stdout[-2000:]


def test_host_parsers_over_the_same_streams(tmp_path, stream_dir):
    _build_and_run(tmp_path, stream_dir, [])


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path, stream_dir):
    _build_and_run(tmp_path, stream_dir, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
