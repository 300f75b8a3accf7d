"""zip(back)'s whole-GPU decode without a GPU: every claim tests/test_zip_back_par.py makes about a stream (its event, p, the text's
length, the depth of its copies, the rounds, routed or handed back) from tests/zip_back_ref.py alone; tests/zb_par_check.cpp -- the
route's phases as a scalar emulation over cniic_amd/csrc/zb_par.hpp against a one-pass decoder -- compiled plain and with ASan + UBSan
and run as a program of its own; the new call's prototype and class surface; the parser's rejection of zip(back); the new kernels'
scratch and spills from the cross-compiled code object."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import test_zip_back_par as G
import zb_par_model as M
import zip_back_edges as E
import zip_back_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_zbp_next", "k_zbp_chain", "k_zbp_ksum", "k_zbp_bscan", "k_zbp_oscan", "k_zbp_result", "k_zbp_fill", "k_zbp_round")


def reference(stream, need=None):
    try:
        return Z.decode_py(stream, need)
    except Z.ZipError:
        return None


@pytest.mark.parametrize("what,stream", G.HOSTILE, ids=[h[0] for h in G.HOSTILE])
def test_the_model_is_the_reference_on_the_hostile_streams(what, stream):
    w = M.walk(stream)
    want = reference(stream)
    assert (want is None) == (w["status"] != M.DONE)
    if want is not None:
        assert w["text"] == want and w["made"] == len(want)
    for cap in (0, 1, 7, max(w["made"] - 1, 0)):
        c = M.walk(stream, cap=cap)
        assert (c["status"], c["p"], c["made"]) == (w["status"], w["p"], w["made"]) and c["text"] == w["text"][:cap] and c["depth"] <= w["depth"]


def test_the_claims_about_events_and_their_order():
    lit, bad = G.LIT, Z.lookback(4, 60000)
    named = dict(G.HOSTILE)
    quiet = M.walk(named["a symbol of no bytes before a bad look-back"])
    assert (quiet["status"], quiet["made"], quiet["p"]) == (M.DONE, 8, len(lit) + 4)
    quiet = M.walk(named["an empty explicit before a bad look-back"])
    assert (quiet["status"], quiet["made"], quiet["p"]) == (M.DONE, 8, len(lit) + 2)
    seen = M.walk(named["a bad look-back before a symbol of no bytes"])
    assert (seen["status"], seen["p"]) == (M.BAD_LOOKBACK, len(lit))
    at = M.walk(named["back == o at 65535"])
    assert at["status"] == M.DONE and at["made"] == 65535 + 100 + 8 and at["depth"] == 1
    past = M.walk(named["back == o + 1 at 65535"])
    assert (past["status"], past["made"], past["p"]) == (M.BAD_LOOKBACK, 65534, 2 * 32769)
    assert M.walk(named["len > back"])["made"] == 8 + 3 + 11
    # need: a bad symbol directly behind the symbol that reaches it is not seen; one symbol earlier it is
    s = lit + Z.lookback(8, 8) + bad
    assert M.walk(s, need=16)["status"] == M.DONE and M.walk(s, need=16)["made"] == 16 and reference(s, 16) is not None
    assert M.walk(s, need=17)["status"] == M.BAD_LOOKBACK and reference(s, 17) is None
    assert M.walk(lit + bad + Z.lookback(8, 8), need=16)["status"] == M.BAD_LOOKBACK
    inside = M.walk(named["long symbols inside a literal"])
    assert inside["status"] == M.DONE and inside["longest"] == 202 and inside["symbols"] == 2
    longest = M.walk(named["an explicit symbol of 32767 bytes"])
    assert longest["longest"] == 32769 and longest["made"] == 32767 * 2 + 1


@pytest.mark.parametrize("n_lookbacks", [1, 2, 31, 32, 33, 1000, 70000])
def test_the_depth_and_the_rounds_of_a_chain(n_lookbacks):
    p = M.plan(M.chain(n_lookbacks))
    assert p["depth"] == n_lookbacks and p["made"] == 8 * (n_lookbacks + 1) and p["rounds"] == int(np.ceil(np.log2(n_lookbacks + 1))) <= 17
    assert p["routed"] and not p["handed"]
    assert M.plan(M.chain(n_lookbacks), round_cap=p["rounds"] - 1)["handed"] and not M.plan(M.chain(n_lookbacks), round_cap=p["rounds"])["handed"]


def test_the_other_streams_of_the_gpu_tests():
    far = M.plan(G.far_chain())
    assert (far["made"], far["depth"], far["rounds"]) == (65535 + 11 * 12500, 3, 2) and far["text"] == Z.decode_py(G.far_chain())
    long_text = M.long_text_stream(E.rnd(512, 3))
    p = M.plan(long_text, cap=1 << 20)
    assert len(long_text) < 4500 and p["made"] == 32768 + 960 * 32767 > 30 << 20 and len(p["text"]) == 1 << 20
    # six doublings, then 31 whole copies of 32767 bytes below the capacity (the 32nd brings 31 bytes, from the shallow front of its source)
    assert p["depth"] == 6 + ((1 << 20) - 32768) // 32767 == 37 and p["rounds"] == 6
    assert not M.plan(b"")["routed"] and M.plan(b"\x07")["routed"] and not M.plan(G.LIT, floor=len(G.LIT) + 1)["routed"]
    for nbytes in (2, 3, M.SCAN_TILE - 1, M.SCAN_TILE, M.SCAN_TILE + 1):
        s = G.explicit_stream(nbytes, 7) if nbytes >= 4 else Z.explicit(b"z" * (nbytes - 2))
        assert len(s) == nbytes and M.walk(s)["text"] == Z.decode_py(s)
    text = E.long_match_mid()
    s = Z.encode_py(text)
    assert M.walk(s)["text"] == text and M.walk(s, cap=len(text) - 1)["made"] == len(text)


def build_check(tmp_path, flags, name):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-g"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "zb_par_check.cpp")])
    return exe


def reference_streams(tmp_path):
    """streams of the reference's coder for the check's mutants: images, and texts with long and far matches"""
    texts = [Z.zip_text(Z.photo_like(24, 16)), Z.zip_text(Z.noise(16, 12)), Z.zip_text(Z.band(40, 3)), E.rnd(500, 1) * 3, b"ab" * 400 + E.rnd(64, 2) + b"ab" * 90]
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        for t in texts:
            s = Z.encode_py(t)
            assert s != Z.PANICS and Z.decode_py(s) == t
            f.write(struct.pack("<I", len(s)) + s)
    return str(path)


@pytest.mark.parametrize("flags,name", [(["-O2"], "plain"), (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "sanitized")])
def test_the_phases_emulated_against_a_one_pass_decoder(tmp_path, flags, name):
    exe = build_check(tmp_path, flags, "zb_par_check_" + name)
    r = subprocess.run([exe, reference_streams(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "zb_par_check ok" in r.stdout, r.stdout + r.stderr


def test_prototype_and_class_surface():
    import inspect
    import cniic_amd
    from cniic_amd import _lib
    assert _lib.PROTOTYPES["cniic_zip_back_image_measure_batch"] == _lib.PROTOTYPES["cniic_hilbert_zip_measure_batch"]
    assert callable(getattr(_lib.Context, "zip_back_measure_batch"))
    src = inspect.getsource(cniic_amd.ZipBack.measure)
    assert "NotImplementedError" not in src and "zip_back_measure_batch" in src
    assert list(inspect.signature(cniic_amd.ZipBack.measure).parameters) == ["self", "imgs", "seed", "max_iters", "flags", "allow"]
    header = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    for mark in ("zb_par_decode", "zb_par_handback", "zb_par_rounds"):
        assert mark in header


def test_zip_back_is_still_no_expression():
    from cniic_amd import _lib
    assert _lib.codec_parse_f64("zip(back)") is None and _lib.codec_parse_f64("zip(dict)") is not None


def test_the_new_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(ROOT, "cniic_amd", "csrc", "k_zipback_par.hip"), "k_zbp_"],
                         capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        lines = [ln for ln in out.splitlines() if re.search(r"\b%s\b" % k, ln) or k + "E" in ln]
        assert len(lines) == 1, (k, out)
        field = lambda name: int(re.search(re.escape(name) + r": (\d+)", lines[0]).group(1))
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, lines[0]
