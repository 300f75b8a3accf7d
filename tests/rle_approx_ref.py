"""CPU restatements of Hilbert { compress: RLE(d) }::encode (src/codec/hilbertc.rs:26-45, rle_approx :200-299) for the tests: a
Python one (IEEE doubles, a correctly rounded math.sqrt, no fused operations) and tests/rle_approx_ref.c, compiled on demand for the
large images.  Both take the image in Hilbert order (oracle_lib.hilbert_linearize, or any injected scan's order)."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# the Makefile's settings (d = 1, 2, 4, 8, 16), a half, distances that real colours hit exactly (sqrt 2, sqrt 3), a tiny and a huge
# one, the edges (inf accepts everything, -1 and NaN nothing)
D_VALUES = [1.0, 2.0, 4.0, 8.0, 16.0, 0.5, math.sqrt(2.0), math.sqrt(3.0), 1e-9, 441.7, math.inf, -1.0, math.nan]


def rust_round(v):
    """f64::round for v >= 0: halves away from zero (Python's round() takes halves to even)"""
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


def encode_py(lin, w, h, d):
    """the whole stream for the pixels lin ((n, 3) uint8, Hilbert order) of a w x h image"""
    px = np.asarray(lin, np.uint8).reshape(-1, 3).tolist()
    n = len(px)
    out = bytearray(struct.pack("<II", w, h))
    exact = d == 0.0
    i = 0
    while i < n:
        s = px[i]
        sm = [float(s[0]), float(s[1]), float(s[2])]
        count = 1
        j = i + 1
        while j < n:
            x = px[j]
            if exact:
                accept = x == s
            else:
                a0 = sm[0] / count - x[0]
                a1 = sm[1] / count - x[1]
                a2 = sm[2] / count - x[2]
                accept = math.sqrt(((0.0 + a0 * a0) + a1 * a1) + a2 * a2) <= d
            if not accept:
                break
            sm[0] += x[0]
            sm[1] += x[1]
            sm[2] += x[2]
            count += 1
            j += 1
            if count == 255:
                break
        out += struct.pack("<BQBBB", count, 3, *(rust_round(v / count) for v in sm))
        i = j
    return bytes(out)


def compile_c(dirpath):
    """tests/rle_approx_ref.c as a shared library in dirpath, or None without a C compiler"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        return None
    so = os.path.join(str(dirpath), "rle_approx_ref.so")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "rle_approx_ref.c"), "-lm"])
    lib = C.CDLL(so)
    lib.rla_encode.restype = C.c_uint64
    lib.rla_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p]
    return lib


def encode_c(lib, lin, w, h, d):
    lin = np.ascontiguousarray(np.asarray(lin, np.uint8).reshape(-1, 3))
    n = lin.shape[0]
    out = np.empty(8 + 12 * n, np.uint8)
    ln = lib.rla_encode(lin.ctypes.data, n, w, h, float(d), out.ctypes.data)
    return out[:ln].tobytes()


# ---- test images
def flat(w, h):
    return np.full((h, w, 3), (93, 41, 200), np.uint8)


def ramp(w, h):
    """slow gradients: long runs at every d, so the 255 cap sets the phase"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 3), np.uint8)
    img[..., 0] = (x * 255) // max(w - 1, 1)
    img[..., 1] = (y * 255) // max(h - 1, 1)
    img[..., 2] = ((x + 2 * y) // 5) % 256
    return img


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    a, b = np.array((10, 20, 30), np.uint8), np.array((40, 60, 90), np.uint8)
    return np.where(((x + y) & 1)[..., None] == 0, a, b).astype(np.uint8)


def noise(w, h, seed=7):
    return np.random.default_rng(seed + w * 7919 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


def distinct(w, h):
    """every pixel its own colour (2^24 of them at 4096 x 4096)"""
    k = np.arange(w * h, dtype=np.uint32) * np.uint32(2654435761 % (1 << 24) | 1) % np.uint32(1 << 24)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8).reshape(h, w, 3)
