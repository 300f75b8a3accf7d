"""The hybrid chain of zip(dict)'s frozen parse without a GPU.  tests/zd_chain_check.cpp, a scalar emulation of the route's steps from the
functions of cniic_amd/csrc/zd_chain.hpp that the kernels call, is held against a serial walk -- plain, and once more as a stand-alone
program under -fsanitize=address,undefined.  Then, from the restatement's stream and the text alone (tests/zip_dict_ref, frozen_parse,
symbol_lengths): every claim tests/test_zd_chain_gpu.py makes about a text of tests/zd_chain_cases.py -- fill end, longest entry, the
parse's long steps with origin and landing, the pieces flown over, the break pieces and those the parse enters.  Last, the cross-compiled
kernels' resources and the places where the marks and knobs are documented."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import zd_chain_cases as K
import zip_dict_edges as E
import zip_dict_ref as Z

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cniic_amd", "csrc")
SRC = os.path.join(HERE, "zd_chain_check.cpp")
PARTS = ("sweep", "placed", "corrupt", "total")
KERNELS = ("k_zd_break_flags", "k_zd_maps_wide", "k_zd_break_table", "k_zd_break_walk", "k_zd_break_patch", "k_zd_marks")


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


_EXE = {}


def _exe(tmp_path_factory, sanitized=False):
    if sanitized not in _EXE:
        exe = str(tmp_path_factory.mktemp("zd_chain_check") / ("check_san" if sanitized else "check"))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2", "-Wall", "-Werror"]
        subprocess.check_call([_compiler(), "-std=c++17"] + flags + ["-I", CSRC, "-o", exe, SRC])
        _EXE[sanitized] = exe
    return _EXE[sanitized]


def _run(exe, parts, *args):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln.split()[1].rstrip(":") for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert tuple(ok) == parts and "FAIL" not in r.stdout, r.stdout[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_dict_ref"))
    assert lib is not None, "no C compiler"
    return lib


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "zd_chain.hpp"\nint main() { const cniic::ZcLanding to = cniic::zc_landing(3, 255 + 257); '
                   'return to.piece == 5 && to.entry == 0 && cniic::kZcMaxBreaks == %d && cniic::zc_is_break(256) && !cniic::zc_is_break(255) ? 0 : 1; }\n' % K.MAX_BREAKS)
    exe = str(tmp_path / "alone")
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(src)])
    assert subprocess.call([exe]) == 0
    assert "#include" not in open(os.path.join(CSRC, "zd_chain.hpp")).read().replace("#include <stdint.h>", "")


def test_the_emulation_against_the_serial_walk(tmp_path_factory):
    out = _run(_exe(tmp_path_factory), PARTS)
    assert "ok total: piece 256, group 64, 1542 bytes a break, bound %d, 0 mismatches" % K.MAX_BREAKS in out
    texts, three = re.search(r"ok sweep: (\d+) texts, (\d+) of them with three levels", out).groups()
    assert int(texts) >= 39 and int(three) >= 6
    assert int(re.search(r"ok placed: (\d+) texts", out).group(1)) >= 300 and int(re.search(r"ok corrupt: (\d+) tables", out).group(1)) == 16


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    _run(_exe(tmp_path_factory, sanitized=True), PARTS)


def test_the_base_text_makes_the_entries_it_claims(clib):
    text, stream, info = K.case(clib, "fly 65")
    ln, syms = E.symbol_lengths(stream)
    assert info["longest"] == 32768 == E.MAX_ENTRY                                       # the GPU is given the frozen phase (flat 98303 is the host's)
    assert sorted(set(ln[ln >= K.PIECE].tolist())) == sorted(x for x in K.FLAT_ENTRIES if x >= K.PIECE)   # nothing above 255 bytes but the flat entries
    assert K.STOP not in K.base_text() and K.FLAT not in K.base_text()[sum(K.HEAD_RUNS) + len(K.FRESH):]
    assert K.MAX_BREAKS == (256 << 20) // 1542


@pytest.mark.parametrize("name", K.NAMES)
def test_every_text_stands_where_it_claims(clib, name):
    text0, fill_end = K.base(clib)
    text, stream, info = K.case(clib, name)
    steps, breaks, entered = K.CLAIMS[name]
    assert info["fill_end"] == fill_end and info["longest"] == 32768 and text.size <= 1400000
    assert Z.decode_c(clib, stream) == text.tobytes()
    got, started = K.long_steps(stream)
    assert got == steps
    br = K.break_pieces(text, fill_end)
    assert len(br) == breaks and len(set(br) & started) == entered and breaks <= K.MAX_BREAKS
    assert all(p in br for p, _, _ in steps)
    M = text.size - fill_end
    lands = [((p * K.PIECE + o + n) // K.PIECE, (o + n) % K.PIECE) for p, o, n in steps]
    if name in K.LANDS:
        assert lands[0][1] == K.LANDS[name]
    if name in K.FLIES:
        assert lands[0][0] - steps[0][0] - 1 == K.FLIES[name]
    if name in K.RUNS:                                       # the pieces between the first landing and the next break piece
        assert br[1] - lands[0][0] == K.RUNS[name] and lands[0][0] not in br
        assert (-(-M // K.PIECE) > 4096) == (K.RUNS[name] > 4000)   # three levels of the scan where they are the point
    if name == "at the fill end":
        assert steps[0][:2] == (0, 0)
    if name == "ends on M":
        assert steps[0][0] * K.PIECE + steps[0][1] + steps[0][2] == M
    if name == "ends before M":
        assert steps[0][0] * K.PIECE + steps[0][1] + steps[0][2] == M - 1
    if name == "cut by M":
        assert K.flat_remaining(text)[fill_end + 5 * K.PIECE + 100] == 300 == M - (5 * K.PIECE + 100)
    if name == "adjacent":
        assert steps[1][0] == steps[0][0] + 1
    if name == "long into long":
        assert lands[0] == steps[1][:2]
    if name == "flown break":
        flown = [p for p in br if p not in started]
        assert flown == list(range(3, 10)) + list(range(13, 28)) + [29]
    if name == "no break":
        assert E.frozen_parse(stream)[2].max() == 128          # a stretch of 255 bytes holds no entry above 128


def test_the_program_on_a_case_s_lengths(clib, tmp_path_factory, tmp_path):
    """"flown break" as a length array -- the flat positions' longest entries, the parse's own steps in the noise, 1 elsewhere -- through the
    emulation: its break pieces and entered ones are the claim's"""
    text, stream, info = K.case(clib, "flown break")
    fill_end, starts, lens = E.frozen_parse(stream)
    rem = K.flat_remaining(text)[fill_end:]
    entries = np.array(sorted(K.FLAT_ENTRIES + (1,)))
    ln = np.ones(text.size - fill_end, np.uint32)
    flat = rem > 0
    ln[flat] = entries[np.searchsorted(entries, rem[flat], side="right") - 1]
    on = lens > 0
    assert np.array_equal(ln[(starts - fill_end)[on]][flat[(starts - fill_end)[on]]], lens[on][flat[(starts - fill_end)[on]]])
    ln[(starts - fill_end)[on]] = lens[on]
    path = tmp_path / "len.bin"
    path.write_bytes(struct.pack("<Q", ln.size) + ln.tobytes())
    out = _run(_exe(tmp_path_factory), ("total",), "len", str(path))
    assert out.splitlines()[0].split()[:2] == [str(K.CLAIMS["flown break"][1]), str(K.CLAIMS["flown break"][2])]


def test_band_has_long_steps_behind_its_fill_end(clib):
    ref = Z.encode_c(clib, np.frombuffer(Z.zip_text(Z.band()), np.uint8))
    assert K.band_counts(ref)[0] >= 1


def test_the_new_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), os.path.join(CSRC, "k_zipdict.hip"), "k_zd_"], capture_output=True, text=True,
                         check=True).stdout
    for name in KERNELS:
        lines = [ln for ln in out.splitlines() if re.search(r"\d+%sE" % name, ln)]
        assert len(lines) == 1, (name, out)
        print(lines[0])
        field = lambda f: int(re.search(re.escape(f) + r": (\d+)", lines[0]).group(1))
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0 and field("VGPRs") <= 64, name
        assert field("LDS Size [bytes/block]") == (512 if name == "k_zd_maps_wide" else 0), name


def test_the_marks_and_knobs_are_documented_and_the_constants_agree():
    import test_zd_chain_gpu as T
    src = open(os.path.join(CSRC, "k_zipdict.hip")).read()
    api = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for mark in T.STAGES[3:]:
        assert '"%s"' % mark in src and api.count('"%s"' % mark) >= 2, mark
    for knob in (T.KNOB_CHAIN, T.KNOB_MAX_BREAKS):
        assert 'test_env("%s")' % knob in src and knob in readme, knob
    assert "zd_chain.hpp" in readme and "zd_chain.hpp" in open(os.path.join(CSRC, "Makefile")).read()
    hdr = open(os.path.join(CSRC, "zd_chain.hpp")).read()
    assert "constexpr uint32_t kZcBreakBytes = 512 + 1024 + 4 + 2;" in hdr and "constexpr uint64_t kZcScratchMax = 256ull << 20;" in hdr
    from cniic_amd import _lib
    assert not any("chain" in name for name in _lib.PROTOTYPES)          # no new entry point
