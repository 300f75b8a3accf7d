"""CPU restatements of the reference's dictionary coder (src/zip/dict.rs) and of the two codecs built on it (Zip::Dict,
src/codec/zipc.rs; Hilbert { compress: Zip }, src/codec/hilbertc.rs) for the tests: a Python one, and tests/zip_dict_ref.c, compiled
on demand for the large inputs.  Written from the reference's behaviour, in this project's own words.

The coder.  Symbols are u16, written little-endian in pairs.  0..255 stand for the single bytes, 0xFFFF for the empty text.  The
encoder reads the longest text that has a symbol, twice, writes the two symbols, and gives the next free symbol (0x100, 0x101, ...)
to the two texts joined -- until 0xFFFE has been handed out; from then on the dictionary stays as it is.  A text that ends after the
first symbol of a pair gets 0xFFFF for the second.  "Longest" is what a trie walk finds: it goes down while the node it stands on has
a child for the next byte and remembers the deepest symbol on the way; the nodes a longer entry created on its way down carry none.

The decoder builds the same table from the pairs it reads.  It fails (the reference panics) on a symbol that has not been handed out
yet and on a first symbol without a second; a single byte behind the last whole pair ends the stream quietly.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

EOF = 0xFFFF
FIRST_NEW = 0x100
MAX_PAIRS = EOF - FIRST_NEW      # 65 279 pairs hand out 0x100 .. 0xFFFE

KNOWN_ANSWERS = [([], []), ([1], [1, EOF]), ([1, 2], [1, 2]), ([1, 2, 1, 3], [1, 2, 1, 3]), ([1, 2, 1, 2, 1, 2], [1, 2, 0x100, 0x100])]


class ZipError(Exception):
    """where the reference's decoder panics or returns None"""


# ---------------------------------------------------------------- Python
def encode_symbols(data, info=None):
    """the symbols of `data` (bytes); info (a dict, optional) receives fill_end (the input position behind the pair that handed out
    0xFFFE, or None if the dictionary never filled) and longest (the longest entry, in bytes)"""
    data = bytes(data)
    n = len(data)
    child, value = {}, {}
    for b in range(256):
        value[b] = b                      # key = node << 8 | byte; the root is node 0
    nodes = 1
    counter = FIRST_NEW
    out = []
    fill_end, longest_entry = None, 1

    def longest(pos):
        node, best, best_end, j = 0, None, pos, pos
        while j < n:
            k = (node << 8) | data[j]
            j += 1
            v = value.get(k)
            if v is not None:
                best, best_end = v, j
            node = child.get(k)
            if node is None:
                break
        return best, best_end

    pos = 0
    while pos < n:
        s1, mid = longest(pos)
        if mid == n:
            out += [s1, EOF]
            break
        s2, end = longest(mid)
        out += [s1, s2]
        if counter != EOF:
            node = 0
            for j in range(pos, end - 1):
                k = (node << 8) | data[j]
                nxt = child.get(k)
                if nxt is None:
                    nxt = child[k] = nodes
                    nodes += 1
                node = nxt
            value[(node << 8) | data[end - 1]] = counter
            counter += 1
            longest_entry = max(longest_entry, end - pos)
            if counter == EOF:
                fill_end = end
        pos = end
    if info is not None:
        info.update(fill_end=fill_end, longest=longest_entry, nodes=nodes)
    return out


def encode_py(data, info=None):
    syms = encode_symbols(data, info)
    return struct.pack("<%dH" % len(syms), *syms)


def decode_py(stream, need=None):
    """the text of `stream`.  need None: all of it (the reference's .collect()).  need = k: as the reference's lazy iterator asked for k
    bytes -- whole pairs are read only while fewer than k bytes are there, nothing behind them is looked at; the text may come out
    shorter than k (the stream ended) or longer (the last pair).  Raises ZipError where the reference panics."""
    stream = bytes(stream)
    table = {b: bytes([b]) for b in range(256)}
    table[EOF] = b""
    counter = FIRST_NEW
    out = bytearray()
    pos = 0
    while need is None or len(out) < need:
        if pos + 2 > len(stream):
            break                                   # no first symbol (or a single byte): the end
        if pos + 4 > len(stream):
            raise ZipError("a first symbol without a second")
        s1, s2 = struct.unpack_from("<HH", stream, pos)
        pos += 4
        if s1 not in table or s2 not in table:
            raise ZipError("symbol not handed out yet")
        text = table[s1] + table[s2]
        if counter != EOF:
            table[counter] = text
            counter += 1
        out += text
    return bytes(out)


# ---------------------------------------------------------------- C
def compile_c(dirpath):
    """tests/zip_dict_ref.c as a shared library in dirpath, or None without a C compiler"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        return None
    so = os.path.join(str(dirpath), "zip_dict_ref.so")
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "zip_dict_ref.c")])
    lib = C.CDLL(so)
    lib.zd_encode.restype = C.c_uint64
    lib.zd_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.zd_decode.restype = C.c_int
    lib.zd_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


NEVER = (1 << 64) - 1


def encode_c(lib, data, info=None):
    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    n = data.size
    out = np.empty(2 * n + 4, np.uint8)
    st = (C.c_uint64 * 3)()
    ln = lib.zd_encode(data.ctypes.data if n else None, n, out.ctypes.data, st)
    if info is not None:
        info.update(fill_end=None if st[0] == NEVER else int(st[0]), longest=int(st[1]), nodes=int(st[2]))
    return out[:ln].tobytes()


def decode_c(lib, stream, need=None, cap=None):
    """as decode_py; cap: the most bytes the text may have (default: room for 64 MiB, or need + the last pair's overshoot)"""
    s = np.frombuffer(bytes(stream), np.uint8)
    if cap is None:
        cap = 64 << 20
    out = np.empty(max(cap, 1), np.uint8)
    ln = C.c_uint64(0)
    rc = lib.zd_decode(s.ctypes.data if s.size else None, s.size, NEVER if need is None else need, out.ctypes.data, cap, C.byref(ln))
    if rc == 1:
        raise ZipError("malformed stream")
    if rc == 2:
        raise MemoryError("text of %d bytes, room for %d" % (ln.value, cap))
    return out[:ln.value].tobytes()


# ---------------------------------------------------------------- the codecs
def records(pixels):
    """Rgb<u8> as the reference serialises it: a u64 length of 3, then the three bytes -- 11 bytes a pixel"""
    px = np.asarray(pixels, np.uint8).reshape(-1, 3)
    rec = np.zeros((px.shape[0], 11), np.uint8)
    rec[:, 0] = 3
    rec[:, 8:11] = px
    return rec.tobytes()


def zip_text(img):
    """what Zip::encode hands the coder: the dimensions, then the pixels' records, row by row"""
    h, w = img.shape[:2]
    return struct.pack("<II", w, h) + records(img)


def codec_encode(enc, img):
    """the zip(dict) stream of img; enc: bytes -> bytes (encode_py, or a lambda around encode_c)"""
    return enc(zip_text(np.ascontiguousarray(img, np.uint8)))


def codec_decode(dec, stream):
    """Zip::decode: the image, or None where the reference returns None or panics.  dec(stream, need) -> text."""
    try:
        head = dec(stream, 8)
        if len(head) < 8:
            return None
        w, h = struct.unpack_from("<II", head)
        need = 8 + 11 * w * h
        text = dec(stream, need)
    except ZipError:
        return None
    if len(text) < need:
        return None
    rec = np.frombuffer(text[8:need], np.uint8).reshape(-1, 11)
    if rec.size and (rec[:, 0] != 3).any() or rec[:, 1:8].any():
        return None
    return rec[:, 8:11].reshape(h, w, 3).copy()


def hilbert_encode(enc, lin, w, h):
    """the hilbert-zip stream: the dimensions as they are, then the coder over the records of the pixels in scan order (lin)"""
    return struct.pack("<II", w, h) + enc(records(lin))


def hilbert_decode_lin(dec, stream):
    """Hilbert { compress: Zip }::decode up to the traversal: (w, h, the w h pixels in scan order), or None where the coder's stream is
    malformed within the text the traversal asks for.  The colours end where the text does, or at the first record whose length is not
    3; the pixels behind them stay zero (the reference's fresh image buffer)."""
    if len(stream) < 8:
        return None
    w, h = struct.unpack_from("<II", stream)
    need = 11 * w * h
    try:
        text = dec(stream[8:], need)
    except ZipError:
        return None
    have = min(len(text), need) // 11
    rec = np.frombuffer(text[:11 * have], np.uint8).reshape(-1, 11)
    bad = np.flatnonzero((rec[:, 0] != 3) | rec[:, 1:8].any(axis=1))
    if bad.size:
        have = int(bad[0])
    lin = np.zeros((w * h, 3), np.uint8)
    lin[:have] = rec[:have, 8:11]
    return w, h, lin


# ---------------------------------------------------------------- test images (numpy.random.default_rng(1) throughout)
def noise(w, h):
    return np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat(w, h):
    return np.full((h, w, 3), (93, 41, 200), np.uint8)


def photo_like(w, h):
    """smooth gradients under a little noise: neighbouring pixels share most of their bits, as a photograph's do"""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 37.0) * np.cos(y / 53.0), 128 + 90 * np.cos(x / 71.0 + y / 29.0), 60 + (x + 2 * y) * 120.0 / (w + 2 * h)], -1)
    return np.clip(base + rng.normal(0.0, 2.0, base.shape), 0, 255).astype(np.uint8)


def band(w=320, h=240):
    """noise with rows 0-15 and 216-239 in one colour: the flat head makes long dictionary entries, the flat tail lies behind the
    point where the dictionary is full"""
    img = noise(w, h)
    img[:16] = (93, 41, 200)
    img[216:] = (93, 41, 200)
    return img
