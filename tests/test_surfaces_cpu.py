"""Surfaces without a GPU: the numpy restatement of the import and the export (tests/surface_ref.py) against a loop over Python integers,
cniic_surface_span over a table of good and bad descriptors, the header / SYMBOLS / ctypes layout of cniic_surface, and
tests/surf_index_check.cpp -- the kernels' head / group / tail split and word fetches walked on the host -- plain and under
-fsanitize=address,undefined."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import surface_ref as R
from cniic_amd import _lib
from cniic_amd._lib import PX_BGR8, PX_BGRA8, PX_L8, PX_LA8, PX_NV12, PX_RGB8, PX_RGBA8, Surface

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMATS = (PX_L8, PX_LA8, PX_RGB8, PX_RGBA8, PX_BGR8, PX_BGRA8)
# the header's table once more, written out (C's term, then per channel the factors of C, D, E)
TABLE = {_lib.YUV_601_LIMITED: (16, (298, 0, 409), (298, -100, -208), (298, 516, 0)), _lib.YUV_709_LIMITED: (16, (298, 0, 459), (298, -55, -136), (298, 541, 0)),
         _lib.YUV_601_FULL: (0, (256, 0, 359), (256, -88, -183), (256, 454, 0)), _lib.YUV_709_FULL: (0, (256, 0, 403), (256, -48, -120), (256, 475, 0))}


def py_yuv(y, u, v, matrix):
    ysub, *chans = TABLE[matrix]
    c, d, e = y - ysub, u - 128, v - 128
    raw = [(kc * c + kd * d + ke * e + 128) // 256 for kc, kd, ke in chans]   # (Python's // is a floor)
    return raw, [min(max(x, 0), 255) for x in raw]


def py_import(buf, s):
    """byte by byte, Python integers only"""
    buf, out = [int(b) for b in buf], []
    for y in range(s.h):
        for x in range(s.w):
            if s.format == PX_NV12:
                uv = s.off_uv + (y >> 1) * s.pitch_uv + 2 * (x >> 1)
                out += py_yuv(buf[s.off + y * s.pitch + x], buf[uv], buf[uv + 1], s.matrix)[1]
                continue
            at = s.off + y * s.pitch + x * _lib.PX_BYTES[s.format]
            if s.format in (PX_L8, PX_LA8):
                out += [buf[at]] * 3
            elif s.format in (PX_RGB8, PX_RGBA8):
                out += buf[at:at + 3]
            else:
                out += [buf[at + 2], buf[at + 1], buf[at]]
    return np.array(out, np.uint8).reshape(s.h, s.w, 3)


def py_export(dst, s, rgb, alpha):
    out = [int(b) for b in dst]
    for y in range(s.h):
        for x in range(s.w):
            at = s.off + y * s.pitch + x * _lib.PX_BYTES[s.format]
            r, g, b = (int(c) for c in rgb[y, x])
            out[at:at + 3] = [r, g, b] if s.format in (PX_RGB8, PX_RGBA8) else [b, g, r]
            if s.format in (PX_RGBA8, PX_BGRA8):
                out[at + 3] = alpha
    return np.array(out, np.uint8)


@pytest.mark.parametrize("matrix", R.MATRICES)
def test_nv12_matrices_on_the_cross_product_clip_at_both_ends_in_every_channel(matrix):
    Y, UV = R.nv12_cross_product()
    seen = set()
    for y in R.Y_VALUES:
        for u in R.C_VALUES:
            for v in R.C_VALUES:
                raw, clipped = py_yuv(y, u, v, matrix)
                assert R.yuv_unclipped(y, u, v, matrix).tolist() == raw and R.yuv_to_rgb(y, u, v, matrix).tolist() == clipped
                assert max(abs(x) for x in raw) < 2 ** 10 and abs(298 * (y - 16)) + 516 * 128 + 208 * 128 + 128 < 2 ** 18
                seen.add((y, u, v))
                for ch in range(3):
                    if raw[ch] < 0:
                        seen.add(("low", ch))
                    if raw[ch] > 255:
                        seen.add(("high", ch))
    assert all((end, ch) in seen for end in ("low", "high") for ch in range(3)), "a channel is never clipped at one end"
    # the planes the GPU test feeds hold exactly that cross product
    buf = np.concatenate([Y.ravel(), UV.ravel()])
    s = Surface(off=0, pitch=50, off_uv=300, pitch_uv=50, w=50, h=6, format=PX_NV12, matrix=matrix)
    got = R.import_surface(buf, s)
    assert np.array_equal(got, py_import(buf, s))
    assert {(int(Y[y, x]), int(UV[y >> 1, x & ~1]), int(UV[y >> 1, (x & ~1) + 1])) for y in range(6) for x in range(50)} == {t for t in seen if len(t) == 3}


@pytest.mark.parametrize("w,h", [(2, 2), (3, 2), (3, 3), (4, 3), (5, 3)])
def test_the_restatement_against_a_python_integer_loop_every_format(w, h):
    rng = np.random.default_rng(w * 16 + h)
    for fmt in FORMATS + (PX_NV12,):
        for matrix in (R.MATRICES if fmt == PX_NV12 else (0,)):
            L = R.Layout()
            s = L.add(fmt, w, h, pad=3, src_res=5, rgb_res=9, matrix=matrix, pad_uv=1, uv_res=7)
            src = L.random_source(int(rng.integers(1 << 30)))
            assert np.array_equal(R.import_surface(src, s), py_import(src, s)), (fmt, matrix)
    for fmt in (PX_RGB8, PX_BGR8, PX_RGBA8, PX_BGRA8):
        L = R.Layout()
        s = L.add(fmt, w, h, pad=2, src_res=3)
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        dst = np.full(L.src_bytes, R.POISON, np.uint8)
        want = py_export(dst, s, rgb, 7)
        R.export_surface(dst, s, rgb, 7)
        assert np.array_equal(dst, want)
        assert np.array_equal(R.import_surface(dst, s), rgb)
        untouched = np.ones(dst.size, bool)
        untouched[R.rows(dst, s.off, s.pitch, w * _lib.PX_BYTES[fmt], h).ravel()] = False
        assert (dst[untouched] == R.POISON).all()


GOOD = [
    # descriptor, src_end, rgb_bytes
    (dict(off=0, pitch=1, w=1, h=1, format=PX_L8), 1, 3),
    (dict(off=7, pitch=10, w=5, h=3, format=PX_LA8), 7 + 2 * 10 + 10, 45),
    (dict(off=3, pitch=20, w=5, h=4, format=PX_RGB8), 3 + 3 * 20 + 15, 60),
    (dict(off=0, pitch=1 << 40, w=2, h=2, format=PX_RGBA8), (1 << 40) + 8, 12),
    (dict(off=1, pitch=9, w=3, h=1, format=PX_BGR8), 10, 9),
    (dict(off=16, pitch=16, w=4, h=2, format=PX_BGRA8, matrix=99, off_uv=1 << 60, pitch_uv=0), 48, 24),   # (matrix and the UV fields: ignored)
    # 3 x 3 NV12: three Y rows of 3 bytes, two UV rows of 4 bytes
    (dict(off=0, pitch=3, off_uv=9, pitch_uv=4, w=3, h=3, format=PX_NV12, matrix=_lib.YUV_709_LIMITED), 17, 27),
    (dict(off=100, pitch=8, off_uv=0, pitch_uv=6, w=5, h=5, format=PX_NV12, matrix=_lib.YUV_601_FULL), 100 + 4 * 8 + 5, 75),   # (the UV plane first: 3 rows end at 18)
    (dict(off=0, pitch=1, off_uv=1, pitch_uv=2, w=1, h=1, format=PX_NV12, matrix=_lib.YUV_601_LIMITED), 3, 3),
    (dict(off=0, pitch=7, off_uv=50, pitch_uv=11, w=7, h=4, format=PX_NV12, matrix=_lib.YUV_709_FULL), 50 + 11 + 8, 84),
    (dict(off=0, pitch=65535, w=65535, h=65537, format=PX_L8), 65535 * 65537, 3 * 65535 * 65537),   # (w h = 2^32 - 1)
]
BAD = [
    dict(off=0, pitch=4, w=1, h=1, format=0), dict(off=0, pitch=4, w=1, h=1, format=8), dict(off=0, pitch=4, w=1, h=1, format=-1),
    dict(off=0, pitch=4, w=0, h=1, format=PX_RGB8), dict(off=0, pitch=4, w=1, h=0, format=PX_RGB8),
    dict(off=0, pitch=1 << 20, w=65536, h=65536, format=PX_L8),          # w h = 2^32
    dict(off=0, pitch=14, w=5, h=2, format=PX_RGB8), dict(off=0, pitch=19, w=5, h=2, format=PX_BGRA8), dict(off=0, pitch=4, w=5, h=1, format=PX_L8),
    dict(off=0, pitch=9, w=5, h=1, format=PX_LA8),
    dict(off=0, pitch=3, off_uv=9, pitch_uv=4, w=3, h=3, format=PX_NV12, matrix=0), dict(off=0, pitch=3, off_uv=9, pitch_uv=4, w=3, h=3, format=PX_NV12, matrix=5),
    dict(off=0, pitch=3, off_uv=9, pitch_uv=3, w=3, h=3, format=PX_NV12, matrix=1), dict(off=0, pitch=2, off_uv=9, pitch_uv=4, w=3, h=3, format=PX_NV12, matrix=1),
    dict(off=(1 << 64) - 8, pitch=8, w=2, h=2, format=PX_RGBA8),        # ends behind 2^64
    dict(off=0, pitch=1 << 63, w=1, h=3, format=PX_L8),
]


@pytest.mark.parametrize("desc,src_end,rgb_bytes", GOOD)
def test_surface_span_of_good_descriptors(desc, src_end, rgb_bytes):
    assert _lib.surface_span(Surface(**desc)) == (src_end, rgb_bytes)


@pytest.mark.parametrize("desc", BAD)
def test_surface_span_refuses(desc):
    assert _lib.surface_span(Surface(**desc)) is None


def test_surface_span_refuses_null_arguments():
    L, s, a, b = _lib.lib(), Surface(off=0, pitch=3, w=1, h=1, format=PX_RGB8), C.c_uint64(77), C.c_uint64(77)
    assert L.cniic_surface_span(None, C.byref(a), C.byref(b)) == _lib.BAD_ARG
    assert L.cniic_surface_span(C.byref(s), None, C.byref(b)) == _lib.BAD_ARG and L.cniic_surface_span(C.byref(s), C.byref(a), None) == _lib.BAD_ARG
    assert (a.value, b.value) == (77, 77)
    assert L.cniic_surface_span(C.byref(s), C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (3, 3)


def test_header_symbols_and_the_ctypes_layout_agree():
    text = open(os.path.join(ROOT, "include", "cniic_hip.h")).read()
    for name in ("cniic_surface_span", "cniic_frames_from_surfaces", "cniic_frames_to_surfaces"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)
    px = {n: int(v) for n, v in re.findall(r"#define CNIIC_PX_(\w+)\s+(\d+)", text)}
    assert px == dict(L8=PX_L8, LA8=PX_LA8, RGB8=PX_RGB8, RGBA8=PX_RGBA8, BGR8=PX_BGR8, BGRA8=PX_BGRA8, NV12=PX_NV12) == dict(
        L8=1, LA8=2, RGB8=3, RGBA8=4, BGR8=5, BGRA8=6, NV12=7)
    yuv = {n: int(v) for n, v in re.findall(r"#define CNIIC_YUV_(\w+)\s+(\d+)", text)}
    assert yuv == {"601_LIMITED": _lib.YUV_601_LIMITED, "601_FULL": _lib.YUV_601_FULL, "709_LIMITED": _lib.YUV_709_LIMITED, "709_FULL": _lib.YUV_709_FULL}
    assert (_lib.YUV_601_LIMITED, _lib.YUV_601_FULL, _lib.YUV_709_LIMITED, _lib.YUV_709_FULL) == (1, 2, 3, 4)
    assert C.sizeof(Surface) == 48
    assert [(n, getattr(Surface, n).offset) for n, _ in Surface._fields_] == [("off", 0), ("pitch", 8), ("off_uv", 16), ("pitch_uv", 24), ("w", 32), ("h", 36),
                                                                              ("format", 40), ("matrix", 44)]
    # the struct in the header: the same members in the same order
    body = re.search(r"typedef struct \{([^}]*)\} cniic_surface;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for decl in body.split(";") for m in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",") if decl.strip()]
    assert members == [n for n, _ in Surface._fields_]


# ---- the kernels' index arithmetic, walked on the host
SRC = os.path.join(HERE, "surf_index_check.cpp")
PARTS = ("split", "import", "export", "pieces", "nv12_chroma")


def _compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ok = [ln.split()[1].rstrip(":") for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert tuple(ok) == PARTS and "FAIL" not in r.stdout, r.stdout[-4000:]


def test_the_split_of_every_row_writes_each_byte_once_and_fetches_only_words_of_the_row(tmp_path):
    exe = str(tmp_path / "surf_index_check")
    subprocess.check_call([_compiler(), "-O2", "-std=c++17", "-o", exe, SRC])
    _run(exe)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "surf_index_check_san")
    subprocess.check_call([_compiler(), "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    _run(exe)
