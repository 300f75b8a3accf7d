"""What the batch decode routes work out without a GPU (cniic_amd/csrc/decode_batch_plan.hpp: take_chunk, the staged images' layout, the span
of a route, frame_dims and vor_parse_head), as a stand-alone program, tests/decode_batch_plan_check.cpp, compiled with the host compiler
against that header and huff_host.cpp with -Wall -Werror (and the library's own -Wno-unused-function): once plain, once under -fsanitize=address,undefined.  Nothing is loaded into
Python.

The chunk, layout and span cases are the program's own.  The streams it parses are written here: the `voronoi` streams of
tests/test_vor_small_decode.py (good_streams, handed_back) and hand-made ones around every way a centroid list can end.  Its verdict per
stream must be Ok exactly where that test's takes() says the batch route's parse goes through, a failing verdict must be a stream the
oracle refuses, and the centroids the sink saw must be those of the plain Python parse below.  codec_decode maps the three failing
verdicts to its three messages; tests/test_vor_small_decode.py holds batch and single decode to the same message per stream on the GPU."""
import os
import shutil
import subprocess

import pytest

import oracle_lib as O
import test_vor_small_decode as V

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
IMG_STRIDE = 3 * 40 * 30 + 5          # test_streams_the_route_hands_back_among_good_ones


def u64(v):
    return int(v).to_bytes(8, "little")


def hand_made():
    good = V.stream(6, 5, [(1, 1, (10, 10, 10)), (4, 3, (20, 20, 20)), (5, 0, (30, 31, 32))])
    n = len(good)
    assert n == 16 + 19 * 3
    return [("fewer than 8 bytes", good[:6]),
            ("8 bytes", good[:8]),
            ("fewer than 16 bytes", good[:12]),
            ("nothing", b""),
            ("K = 0", V.stream(4, 4, [])),
            ("K = 0 and bytes behind", V.stream(4, 4, []) + b"\x07" * 40),
            ("K = (n - 16) / 19 + 1", good[:8] + u64((n - 16) // 19 + 1) + good[16:]),
            ("K = (n - 16) / 19", good),
            ("K = (n - 16) / 19 - 1", good[:8] + u64(2) + good[16:]),              # bytes behind the list are not its business
            ("a length word of 2 first", V.stream(6, 5, [(1, 1, (1, 2, 3)), (2, 2, (4, 5, 6))], length_word=2)),
            ("a length word of 3 + 2^32", good[:16 + 8] + u64(3 + 2 ** 32) + good[16 + 16:]),
            ("cut inside the last colour", good[:-1]),
            ("cut behind the last length word", good[:-3]),
            ("cut inside the last y", good[:-13]),
            ("K = 2^32", good[:8] + u64(2 ** 32) + good[16:]),
            ("K = 2^32 + 3", good[:8] + u64(2 ** 32 + 3) + good[16:]),
            ("K = 2^64 - 1", good[:8] + u64(2 ** 64 - 1) + good[16:])]


def all_streams():
    return V.good_streams() + V.handed_back(IMG_STRIDE) + hand_made()


def plain_parse(s):
    """the statement of codec_decode's `voronoi` parse (clusterc.rs:168-189) -> (header read, w, h, verdict, K, the centroids in front of the stop)"""
    if len(s) < 8:
        return False, 0, 0, None, 0, []
    w, h = int.from_bytes(s[0:4], "little"), int.from_bytes(s[4:8], "little")
    if len(s) < 16:
        return True, w, h, "Truncated", 0, []
    K = int.from_bytes(s[8:16], "little")
    if K > (len(s) - 16) // 19:
        return True, w, h, "TruncatedList", K, []
    cents = []
    for k in range(K):
        at = 16 + 19 * k
        if int.from_bytes(s[at + 8:at + 16], "little") != 3:
            return True, w, h, "BadCentroid", K, cents
        cents.append((k, int.from_bytes(s[at:at + 4], "little"), int.from_bytes(s[at + 4:at + 8], "little"), s[at + 16], s[at + 17], s[at + 18]))
    return True, w, h, "Ok", K, cents


def digest(cents):
    d = 0xcbf29ce484222325
    for k, x, y, r, g, b in cents:
        for v, nbytes in ((k, 8), (x, 4), (y, 4), (r, 1), (g, 1), (b, 1)):
            for byte in int(v).to_bytes(nbytes, "little"):
                d = ((d ^ byte) * 0x100000001b3) & (2 ** 64 - 1)
    return d


def test_the_streams_are_what_they_are_named_for():
    facts = {name: plain_parse(s) for name, s in all_streams()}
    assert len(facts) == len(all_streams())                                         # no name twice
    assert all(facts[n][3] == "Ok" for n, _ in V.good_streams())
    assert not facts["7 bytes"][0] and not facts["fewer than 8 bytes"][0] and not facts["nothing"][0]
    for n in ("8 bytes", "15 bytes", "fewer than 16 bytes"):
        assert facts[n][3] == "Truncated", n
    for n in ("K = (n - 16) / 19 + 1", "cut inside the last colour", "cut behind the last length word", "cut inside the last y", "K = 2^32", "K = 2^32 + 3", "K = 2^64 - 1",
              "a list cut by one byte", "K says more than there is"):
        assert facts[n][3] == "TruncatedList", n
    for n, seen in (("a length word of 2", 1), ("a length word of 2 first", 0), ("a length word of 3 + 2^32", 0)):
        assert facts[n][3] == "BadCentroid" and len(facts[n][5]) == seen, n
    for n, K in (("K = 0", 0), ("K = 0 and bytes behind", 0), ("K = (n - 16) / 19", 3), ("K = (n - 16) / 19 - 1", 2), ("K = 257", 257), ("w h = 0", 1)):
        assert facts[n][3] == "Ok" and facts[n][4] == K, n
    # the oracle refuses every stream whose parse fails, and decodes every one that parses and has centroids for its pixels
    for name, s in all_streams():
        seen, w, h, verdict, K, _ = facts[name]
        rc = O.decode("voronoi(1)", s)[0]
        if not seen or verdict != "Ok":
            assert rc == O.DECODE, name
        elif w * h == 0 or (K >= 1 and w * h <= 1 << 20):
            assert rc == 0, name


def test_the_single_decode_gives_each_verdict_its_message():
    src = open(os.path.join(CSRC, "codec.cpp")).read()
    at = [src.index('case VorHead::Truncated: return c->fail(CNIIC_ERR_DECODE, "voronoi: truncated");'),
          src.index('case VorHead::TruncatedList: return c->fail(CNIIC_ERR_DECODE, "voronoi: truncated centroid list");'),
          src.index('case VorHead::BadCentroid: return c->fail(CNIIC_ERR_DECODE, "voronoi: bad centroid");')]
    assert at == sorted(at)
    hdr = open(os.path.join(CSRC, "decode_batch_plan.hpp")).read()
    assert "#include <hip" not in hdr and "hip_runtime" not in hdr and '#include "common.hpp"' not in hdr   # host-only: nothing of the GPU runtime
    assert src.count("vor_parse_head(") == 2 and "l != 3" not in src and hdr.count("l != 3") == 1       # one centroid parser, used by both decodes


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def stream_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_batch_plan")
    names = []
    for i, (_, s) in enumerate(all_streams()):
        names.append("s%03d.bin" % i)
        (d / names[-1]).write_bytes(s)
    (d / "manifest.txt").write_text("\n".join(names) + "\n")
    return str(d), names


def _build_and_run(tmp_path, stream_dir, flags):
    exe = str(tmp_path / "decode_batch_plan_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function"] + flags + ["-I", CSRC, "-o", exe, os.path.join(HERE, "decode_batch_plan_check.cpp"),
                           os.path.join(CSRC, "huff_host.cpp")])
    d, names = stream_dir
    r = subprocess.run([exe, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-4000:]
    assert "plan: 0 failures" in r.stdout and "%d streams, 0 failures" % len(names) in r.stdout, r.stdout[-2000:]
    lines = {ln.split()[1]: ln for ln in r.stdout.splitlines() if ln.startswith("file ")}
    assert len(lines) == len(names)
    for fname, (name, s) in zip(names, all_streams()):
        seen, w, h, verdict, K, cents = plain_parse(s)
        if not seen:
            assert lines[fname] == "file %s dims=0" % fname, name
            assert not V.takes(s)
            continue
        pos = 8 if verdict == "Truncated" else 16 if verdict == "TruncatedList" else 16 + 19 * len(cents) + (16 if verdict == "BadCentroid" else 0)
        want = "file %s dims=1 w=%d h=%d verdict=%s K=%d seen=%d digest=%016x pos=%d" % (fname, w, h, verdict, K, len(cents), digest(cents), pos)
        assert lines[fname] == want, (name, lines[fname], want)
        # Ok exactly where the batch route's parse goes through: takes() is that parse and the route's gates on K and the pixels
        for img_stride in (1 << 40, IMG_STRIDE):
            gates = 1 <= K <= V.MAX_K and 1 <= w * h <= V.MAX_PX and 3 * w * h <= img_stride
            assert (verdict == "Ok" and gates) == V.takes(s, img_stride), name


def test_the_planning_as_a_program(tmp_path, stream_dir):
    _build_and_run(tmp_path, stream_dir, [])


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path, stream_dir):
    _build_and_run(tmp_path, stream_dir, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
