"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/cniic_hip.h declares, mirrors the reference's Codec trait surface (names, lossless flags,
--codec= parsing), and FAILS LOUDLY when no GPU is usable (there is no CPU fallback)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cniic_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from cniic_amd import _lib
    L = _lib.lib()
    decl = declared_symbols()
    assert len(decl) >= 35
    missing = [s for s in decl if not hasattr(L, s)]
    assert not missing, missing
    # the Python loader's own list is the same set
    assert sorted(_lib.SYMBOLS) == decl


def declared_prototypes():
    """include/cniic_hip.h -> {name: (restype, [argtypes])} by the fixed mapping that cniic_amd/_lib.py states above its PROTOTYPES"""
    import ctypes as C

    from cniic_amd import _lib
    text = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    scalar = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    ret = dict(scalar, void=None)

    def param(p):
        if p.startswith("cniic_host_sum_fn "):
            return _lib.HOST_SUM_FN
        if re.match(r"const char ?\*", p):
            return C.c_char_p
        if "*" in p or "[" in p:
            return C.c_void_p
        return scalar[p.split(" ")[0]]   # (KeyError: a parameter kind the mapping does not know)

    protos = {}
    for m in re.finditer(r"\b(void|int32_t|uint32_t|uint64_t|double|const\s+char\s*\*)\s*(cniic_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        r, name, params = m.groups()
        params = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
        protos[name] = (C.c_char_p if "char" in r else ret[r], [] if params == ["void"] else [param(p) for p in params])
    return protos


def test_prototype_table_matches_header():
    """every declaration of the header has exactly its restype and argtypes in _lib.PROTOTYPES, and the table names nothing else"""
    from cniic_amd import _lib
    decl = declared_prototypes()
    assert sorted(decl) == declared_symbols()       # the parser found every function the name check knows
    assert len(decl) >= 111
    for name, (restype, argtypes) in decl.items():
        assert name in _lib.PROTOTYPES, name
        assert _lib.PROTOTYPES[name][0] is restype, name
        assert list(_lib.PROTOTYPES[name][1]) == argtypes, name
    assert not set(_lib.PROTOTYPES) - set(decl)
    assert _lib.SYMBOLS == list(_lib.PROTOTYPES)


def test_loaded_library_is_fully_declared():
    from cniic_amd import _lib
    L = _lib.lib()
    decl = declared_prototypes()
    for name in _lib.SYMBOLS:
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
        assert len(fn.argtypes) == len(decl[name][1]), name
        assert fn.restype is _lib.PROTOTYPES[name][0], name


def test_bare_int_arrives_in_full_width():
    """a uint64_t given as a bare Python int: without a prototype ctypes passes 32 bits of it, and this capacity would arrive as 0"""
    import ctypes as C

    from cniic_amd import _lib
    buf = C.create_string_buffer(64)
    assert _lib.lib().cniic_codec_name(b"hufman", buf, 1 << 32) == _lib.OK      # (host only; writes 7 bytes)
    assert buf.value == b"Hufman"


def test_ptr_of_bytearray_is_its_own_buffer():
    import ctypes as C

    from cniic_amd import _lib
    ba = bytearray(b"0123456789abcdef")
    assert _lib._ptr(ba).value == C.addressof((C.c_char * len(ba)).from_buffer(ba))
    C.memmove(_lib._ptr(ba).value, b"X", 1)
    assert ba[0] == ord("X") and bytes(ba[1:]) == b"123456789abcdef"
    assert isinstance(_lib._ptr(bytearray()), C.c_void_p)    # empty: still a pointer (which may be null), no exception
    b = b"0123456789abcdef"
    assert C.string_at(_lib._ptr(b).value, len(b)) == b      # bytes: the caller's own object, as before


def test_release_library_has_no_test_hooks():
    """CNIIC_TEST_* / CNIIC_DBG_* and the other route-forcing knobs are compiled into the testing build only.
    The release library exports the same symbols, says it is the release build, and none of those names is in its binary."""
    import ctypes as C
    rel = os.path.join(ROOT, "cniic_amd", "libcniic_hip.so")
    tst = os.path.join(ROOT, "cniic_amd", "libcniic_hip_testing.so")
    assert os.path.exists(rel) and os.path.exists(tst), "build both with make -C cniic_amd/csrc"
    R, T = C.CDLL(rel), C.CDLL(tst)
    assert R.cniic_is_testing_build() == 0 and T.cniic_is_testing_build() == 1
    missing = [s for s in declared_symbols() if not hasattr(R, s)]
    assert not missing, missing
    blob_r, blob_t = open(rel, "rb").read(), open(tst, "rb").read()
    hooks = [b"CNIIC_TEST_", b"CNIIC_KM_PS_REQUIRE", b"CNIIC_KM_UNFUSED", b"CNIIC_KM_BATCH", b"CNIIC_HD_PHASES", b"CNIIC_TRACE_HOST", b"CNIIC_XY_UNFUSED"]
    for h in hooks:
        assert h not in blob_r, "release library still carries %s" % h.decode()
        assert h in blob_t, "testing library lost %s" % h.decode()
    # what the release build does read: the documented fallbacks of the context options
    for name in (b"CNIIC_SP_MIN_PIXELS", b"CNIIC_KERNEL_TIMERS", b"CNIIC_COLLECTIVE_TIMEOUT_MS"):
        assert name in blob_r
    from cniic_amd import _lib
    assert _lib.lib().cniic_is_testing_build() == 1     # the suite itself runs on the testing build (conftest.py)


def test_no_oracle_in_product():
    """the product path must not route through oracle/ (tests-only infrastructure)"""
    pkg = os.path.join(ROOT, "cniic_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                src = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in src.lower(), os.path.join(dp, f)


@pytest.mark.parametrize("expr,name,lossless", [
    ("hufman", "Hufman", True), ("HUFMAN", "Hufman", True),                 # hufc.rs:42-59
    ("cluster-colors(256)", "cluster-colors_256", False), ("ccol(16)", "cluster-colors_16", False),
    ("c-colors(3)", "cluster-colors_3", False),                             # clusterc.rs:59-65,116-141
    ("voronoi(2048)", "voronoi_2048", False),                               # clusterc.rs:191-197
    ("delta", "delta", True),                                               # hilbertc.rs:433-439
    ("hilbert(rle)", "hilbert-rle", True), ("Hilbert(rle(0))", "hilbert-rle", True),   # hilbertc.rs:81-97,341-383
    ("hilbert(rle(0.0))", "hilbert-rle", True),
])
def test_codec_names_and_flags(expr, name, lossless):
    from cniic_amd import _lib
    assert _lib.codec_name(expr) == name
    assert _lib.codec_is_lossless(expr) == lossless


@pytest.mark.parametrize("expr", ["", "huffman", "delta2", "Delta", "voronoi()", "cluster-colors(x)", "hilbert-rle", "zip-dict",
                                  "hilbert(zip)", "hilbert(rle(0.5))", "hilbert()", "HILBERT(rle)", "hilbert(rle)x"])
def test_codec_parse_rejects(expr):
    from cniic_amd import _lib
    assert _lib.codec_parse(expr) is None


def test_huf_size_is_host_side_and_matches_oracle():
    import numpy as np

    import oracle_lib as O
    from cniic_amd import _lib
    counts = np.array([5, 1, 1, 2, 9, 30, 2], np.uint64)
    nb = _lib.C.c_uint64(0)
    rc = _lib.lib().cniic_huf_size(_lib.SYM_RGB, counts.ctypes.data_as(_lib.C.c_void_p), _lib.C.c_uint64(counts.size), _lib.C.byref(nb))
    assert rc == 0 and nb.value == O.huf_size(O.SYM_RGB, counts)


def test_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import cniic_amd
    with pytest.raises(cniic_amd.CniicError):
        cniic_amd.Context(0)
