"""CPU restatements of the reference's look-back coder (src/zip/back.rs) and of the codec built on it (Zip::Back, src/codec/zipc.rs)
for the tests and tools/zip_back_probe.py: a Python one, and tests/zip_back_ref.c, compiled on demand for the large inputs.  Written
from the reference's behaviour, in this project's own words.

The stream.  A sequence of symbols, each headed by a little-endian u16: bit 15 the kind, the low 15 bits `len`.  Kind 0 (explicit):
`len` literal bytes follow.  Kind 1 (look-back): a little-endian u16 `back` follows; the symbol stands for min(len, back) bytes that
start `back` bytes before the end of what has been decoded so far.

The encoder stands at position p with e explicit bytes gathered.  With six or more bytes left it looks, among the positions q with
max(0, p - 65535) <= q <= p - 6 whose six bytes equal those at p, for the longest common run of text[q, p) and text[p, n); among equals
the smallest q.  A candidate found: the gathered explicit symbol is written, then the look-back (length, p - q), and e is 0 again.
None: max(e, 2) more bytes join the explicit run without a look inside them -- or, if fewer are left, those, and the text is done.
A length of 32 768 or more, of either kind, does not fit the header: the reference's assertion fails (back.rs:45), PANICS here.

The decoder ends quietly where no whole header stands (or a look-back header without its `back`), and -- being an iterator that looks
at the next symbol only when it has no byte to hand out, and reports the end when that symbol brings none -- at a symbol that stands
for no byte at all: an explicit one of length 0, a look-back with len 0 or back 0.  It fails (the reference panics) on an explicit
symbol cut short and on a `back` that reaches behind the start of the text.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np

from zip_dict_ref import ZipError, band, flat, noise, photo_like, records, zip_text   # noqa: F401  (the text and the images are zip(dict)'s)

HERE = os.path.dirname(os.path.abspath(__file__))

MIN_REP = 6
WINDOW = 0xFFFF
MAX_LEN = 0x7FFF
PANICS = "reference panics"     # the verdict where compress_len's assertion fails


def explicit(data):
    data = bytes(data)
    return struct.pack("<H", len(data)) + data


def lookback(length, back):
    return struct.pack("<HH", 0x8000 | length, back)


# the reference's own known answers (back.rs:726-825)
KNOWN_ANSWERS = [
    (b"", b""),
    (b"\x01", explicit(b"\x01")),
    (b"\x01\x02", explicit(b"\x01\x02")),
    (b"\x01\x01", explicit(b"\x01\x01")),
    (b"\x01" * 6, explicit(b"\x01" * 6)),
    (b"\x01" * 16, explicit(b"\x01" * 8) + lookback(8, 8)),
    (b"\x01" * 8 + b"\x02" * 8, explicit(b"\x01" * 8 + b"\x02" * 8)),
]


# ---------------------------------------------------------------- Python
def _common(data, q, p, limit):
    """length of the common run of data[q:] and data[p:], at most limit"""
    lo, step = 0, 16
    while lo < limit:
        k = min(step, limit - lo)
        if data[q + lo:q + lo + k] != data[p + lo:p + lo + k]:
            while data[q + lo] == data[p + lo]:
                lo += 1
            return lo
        lo += k
        step *= 2
    return lo


def parse_py(data):
    """the symbols of `data` as a list of ("E", bytes) and ("L", len, back), or PANICS; with them the positions that were probed"""
    data = bytes(data)
    n = len(data)
    index = {}          # six bytes -> ascending positions
    indexed = 0         # keys of the positions below this one are in the index
    syms, probes = [], []
    p, run_start, e = 0, 0, 0
    while True:
        best_len, best_q = 0, -1
        if p + MIN_REP <= n:
            while indexed + MIN_REP <= p:
                index.setdefault(data[indexed:indexed + MIN_REP], []).append(indexed)
                indexed += 1
            probes.append(p)
            for q in index.get(data[p:p + MIN_REP], ()):
                if q < p - WINDOW:
                    continue
                length = _common(data, q, p, min(p - q, n - p))
                if length > best_len:
                    best_len, best_q = length, q
        if best_len:
            if best_len > MAX_LEN:
                return PANICS, probes
            if e:
                syms.append(("E", data[run_start:p]))
            syms.append(("L", best_len, p - best_q))
            p += best_len
            run_start, e = p, 0
            continue
        t = max(e, 2)
        if n - p < t:
            e += n - p
            if e:
                syms.append(("E", data[run_start:n]))
            return syms, probes
        e += t
        p += t
        if e > MAX_LEN:
            return PANICS, probes


def serialize(syms):
    out = bytearray()
    for s in syms:
        out += explicit(s[1]) if s[0] == "E" else lookback(s[1], s[2])
    return bytes(out)


def encode_py(data):
    """the stream of `data`, or PANICS"""
    syms, _ = parse_py(data)
    return PANICS if syms == PANICS else serialize(syms)


def decode_py(stream, need=None):
    """the text of `stream`.  need None: all of it (the reference's .collect()).  need = k: whole symbols are read only while fewer
    than k bytes are there, nothing behind them is looked at.  Raises ZipError where the reference panics."""
    stream = bytes(stream)
    out = bytearray()
    pos = 0
    while need is None or len(out) < need:
        if pos + 2 > len(stream):
            break
        head, = struct.unpack_from("<H", stream, pos)
        pos += 2
        length = head & MAX_LEN
        if head & 0x8000:
            if pos + 2 > len(stream):
                break
            back, = struct.unpack_from("<H", stream, pos)
            pos += 2
            if back > len(out):
                raise ZipError("back reaches behind the start of the text")
            k = min(length, back)
            start = len(out) - back
            out += out[start:start + k]
        else:
            if pos + length > len(stream):
                raise ZipError("an explicit symbol cut short")
            k = length
            out += stream[pos:pos + length]
            pos += length
        if k == 0:
            break                                   # the iterator has nothing to hand out: the end
    return bytes(out)


# ---------------------------------------------------------------- C
def compile_c(dirpath):
    """tests/zip_back_ref.c as a shared library in dirpath, or None without a C compiler"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        return None
    so = os.path.join(str(dirpath), "zip_back_ref.so")
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "zip_back_ref.c")])
    lib = C.CDLL(so)
    lib.zb_encode.restype = C.c_int
    lib.zb_encode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.zb_decode.restype = C.c_int
    lib.zb_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


NEVER = (1 << 64) - 1


def encode_c(lib, data, info=None):
    """the stream of `data`, or PANICS; info (a dict, optional) receives longest (the longest look-back), farthest (the largest back),
    explicit (the longest explicit symbol) and probes"""
    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    n = data.size
    cap = n + n // 4 + 16
    out = np.empty(cap, np.uint8)
    ln = C.c_uint64(0)
    st = (C.c_uint64 * 4)()
    rc = lib.zb_encode(data.ctypes.data if n else None, n, out.ctypes.data, cap, C.byref(ln), st)
    if info is not None:
        info.update(longest=int(st[0]), farthest=int(st[1]), explicit=int(st[2]), probes=int(st[3]))
    if rc == 1:
        return PANICS
    assert rc == 0 and ln.value <= cap
    return out[:ln.value].tobytes()


def decode_c(lib, stream, need=None, cap=None):
    """as decode_py; cap: the most bytes the text may have (default 64 MiB)"""
    s = np.frombuffer(bytes(stream), np.uint8)
    if cap is None:
        cap = 64 << 20
    out = np.empty(max(cap, 1), np.uint8)
    ln = C.c_uint64(0)
    rc = lib.zb_decode(s.ctypes.data if s.size else None, s.size, NEVER if need is None else need, out.ctypes.data, cap, C.byref(ln))
    if rc == 1:
        raise ZipError("malformed stream")
    if rc == 2:
        raise MemoryError("text of %d bytes, room for %d" % (ln.value, cap))
    return out[:ln.value].tobytes()


# ---------------------------------------------------------------- the codec
def codec_encode(enc, img):
    """the zip-back stream of img, or PANICS; enc: bytes -> bytes"""
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
    if rec.size and ((rec[:, 0] != 3).any() or rec[:, 1:8].any()):
        return None
    return rec[:, 8:11].reshape(h, w, 3).copy()
