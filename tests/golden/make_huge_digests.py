#!/usr/bin/env python3
"""Writes tests/golden/huge_digests.json: the ORACLE's results for images of 2^31 pixels and more.

CPU only, one case per process and never two at once (the delta and cluster-colors cases peak near 45 GB of host memory):

    python tests/golden/make_huge_digests.py --only d46k        # then r46k, ra46k, fib, cc46k

tests/test_gpu_huge.py (-m gpu) encodes the same images on the HIP path and compares digests: past 2^31 pixels a 32-bit index,
byte offset or bit offset wraps, and only a comparison with an independent encoder sees the wrong bytes.  Every entry is the
oracle's stream (oracle/*.c, mode L): SHA-256, length, K-means iterations, the longest Huffman code (read back from the stream's
tree), and for lossy codecs the SHA-256 of the image the oracle decodes.  Before a digest is written the oracle is checked
against itself: a lossless stream decodes back to the image, and for `fib` huf_size(counts) + 8 equals the stream length.

Images (tests/huge_gen.py; photo = synth.photo = cniic_synth_image kind 1, numpy rows by make_fullsize_digests.photo_rows):
  d46k   photo 46341 x 46341 (2 147 488 281 px), seed S+5         delta
  r46k   tiles 46341 x 46341                                      hilbert(rle)
  ra46k  tiles + ripple 46341 x 46341                             hilbert(rle(4)), by tests/rle_approx_ref.c on the oracle's scan;
                                                                  decoded by the oracle's hilbert(rle) decoder
  fib    Fibonacci counts F(1..45), 46368 x 64079                 hufman (longest code 44 bits)
  cc46k  tiles with a 55 % background, 46341 x 46341              cluster-colors(256), mode L, threaded kmeans_fast
"""
import argparse
import ctypes as C
import hashlib
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import huge_gen as G  # noqa: E402
import oracle_lib as O  # noqa: E402
import rle_approx_ref as R  # noqa: E402
from cniic_amd import synth  # noqa: E402
from make_fullsize_digests import photo_rows  # noqa: E402

OUT = os.path.join(HERE, "huge_digests.json")
S = synth.SEED0
SIDE = 46341
BAND = 128
CHUNK = 1 << 30


def _band(args):
    kind, w, h, y0, y1 = args
    if kind == "photo":
        return y0, photo_rows(w, h, S + 5, y0, y1)
    if kind == "fib":
        return y0, G.fib_rows(np, y0, y1)
    return y0, G.tiles_rows(np, w, y0, y1, kind)


def image(kind, w, h, procs):
    img = np.empty((h, w, 3), np.uint8)
    jobs = [(kind, w, h, y0, min(h, y0 + BAND)) for y0 in range(0, h, BAND)]
    with mp.Pool(procs) as pool:
        for y0, rows in pool.imap_unordered(_band, jobs):
            img[y0:y0 + rows.shape[0]] = rows
    return img


def sha(a):
    """SHA-256 of a flat uint8 array, fed in 1 GiB pieces"""
    a = a.reshape(-1)
    h = hashlib.sha256()
    for at in range(0, a.size, CHUNK):
        h.update(memoryview(a[at:at + CHUNK]))
    return h.hexdigest()


def same(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    return a.size == b.size and all(np.array_equal(a[at:at + CHUNK], b[at:at + CHUNK]) for at in range(0, a.size, CHUNK))


def encode(expr, img, cap):
    h, w = img.shape[:2]
    out = np.empty(cap, np.uint8)
    ln = C.c_uint64(0)
    st = O.KmStats()
    rc = O.lib().orc_encode(expr.encode(), O.MODE_L, C.c_uint64(O.DEFAULT_SEED), O._p(img), C.c_uint32(w), C.c_uint32(h),
                            O._p(out), C.c_uint64(cap), C.byref(ln), C.byref(st))
    assert rc == 0, (expr, rc)
    return out[:ln.value], st.as_dict()


def decode(expr, data):
    w = int.from_bytes(data[0:4].tobytes(), "little")
    h = int.from_bytes(data[4:8].tobytes(), "little")
    out = np.empty((h, w, 3), np.uint8)
    cw, ch = C.c_uint32(0), C.c_uint32(0)
    rc = O.lib().orc_decode(expr.encode(), O._p(data), C.c_uint64(data.size), O._p(out), C.c_uint64(out.size), C.byref(cw), C.byref(ch))
    assert rc == 0 and (cw.value, ch.value) == (w, h), (expr, rc)
    return out


def longest_code(data, sym_bytes):
    """depth of the deepest leaf of the Huffman tree serialised (pre-order, huf.rs:305-321) after the 8 header bytes"""
    b = data[8:8 + (1 << 26)].tobytes()
    pos, deepest, stack = 0, 0, [0]
    while stack:
        d = stack.pop()
        tag = b[pos]
        pos += 1
        if tag == 0:
            pos += sym_bytes
            deepest = max(deepest, d)
        else:
            assert tag == 1
            stack += [d + 1, d + 1]
    return deepest


def load():
    if os.path.exists(OUT):
        with open(OUT) as f:
            return json.load(f)
    return {"_about": "oracle results past 2^31 pixels; made by tests/golden/make_huge_digests.py (see its docstring)", "cases": {}}


def save(d):
    with open(OUT + ".tmp", "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    os.replace(OUT + ".tmp", OUT)


def case_d46k(a):
    img = image("photo", SIDE, SIDE, a.procs)
    t = time.time()
    data, _ = encode("delta", img, 64 + SIDE * SIDE * 3)
    secs = time.time() - t
    src = sha(img)
    del img
    assert sha(decode("delta", data)) == src, "the oracle's delta stream does not decode to the image"
    return dict(codec="delta", w=SIDE, h=SIDE, image="photo", seed_offset=5, sha256=sha(data), length=int(data.size),
                longest_code=longest_code(data, 6), image_sha256=src, oracle_seconds=round(secs, 1))


def case_r46k(a):
    img = image("tiles", SIDE, SIDE, a.procs)
    t = time.time()
    data, _ = encode("hilbert(rle)", img, 8 + SIDE * SIDE * 12)
    secs = time.time() - t
    assert same(decode("hilbert(rle)", data), img), "the oracle's hilbert(rle) stream does not decode to the image"
    return dict(codec="hilbert(rle)", w=SIDE, h=SIDE, image="tiles", sha256=sha(data), length=int(data.size), image_sha256=sha(img),
                oracle_seconds=round(secs, 1))


def case_ra46k(a):
    img = image("ripple", SIDE, SIDE, a.procs)
    n = SIDE * SIDE
    src = sha(img)
    t = time.time()
    lin = np.empty((n, 3), np.uint8)
    assert O.lib().orc_hilbert_linearize(O._p(img), C.c_uint32(SIDE), C.c_uint32(SIDE), O._p(lin)) == 0
    del img
    with tempfile.TemporaryDirectory() as tmp:
        lib = R.compile_c(tmp)
        assert lib is not None, "no C compiler for tests/rle_approx_ref.c"
        out = np.empty(8 + 12 * n, np.uint8)
        ln = lib.rla_encode(lin.ctypes.data, n, SIDE, SIDE, 4.0, out.ctypes.data)
    del lin
    data = out[:ln]
    secs = time.time() - t
    back = decode("hilbert(rle)", data)
    return dict(codec="hilbert(rle(4))", w=SIDE, h=SIDE, image="ripple", sha256=sha(data), length=int(data.size), image_sha256=src,
                decoded_sha256=sha(back), oracle_seconds=round(secs, 1))


def case_fib(a):
    img = image("fib", G.FIB_W, G.FIB_H, a.procs)
    n = G.FIB_W * G.FIB_H
    t = time.time()
    data, _ = encode("hufman", img, 64 + n * 2)
    secs = time.time() - t
    counts = np.array(sorted(G.fib_counts()), np.uint64)
    assert O.huf_size(O.SYM_RGB, counts) + 8 == data.size, "orc_huf_size + 8 != the oracle's stream length"
    assert same(decode("hufman", data), img), "the oracle's hufman stream does not decode to the image"
    return dict(codec="hufman", w=G.FIB_W, h=G.FIB_H, image="fib", sha256=sha(data), length=int(data.size),
                longest_code=longest_code(data, 11), image_sha256=sha(img), oracle_seconds=round(secs, 1))


def case_cc46k(a):
    img = image("bg", SIDE, SIDE, a.procs)
    src = sha(img)
    O.lib().orc_set_lloyd_threads(a.threads)
    t = time.time()
    data, st = encode("cluster-colors(256)", img, 64 + SIDE * SIDE * 2)
    secs = time.time() - t
    del img
    back = decode("cluster-colors(256)", data)
    return dict(codec="cluster-colors(256)", w=SIDE, h=SIDE, image="bg", mode="L", sha256=sha(data), length=int(data.size),
                iterations=st["iterations"], longest_code=longest_code(data, 11), image_sha256=src, decoded_sha256=sha(back),
                oracle_seconds=round(secs, 1))


CASES = {"d46k": case_d46k, "r46k": case_r46k, "ra46k": case_ra46k, "fib": case_fib, "cc46k": case_cc46k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, help="one case of " + ",".join(CASES))
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--procs", type=int, default=8, help="processes that draw the image's row bands")
    a = ap.parse_args()
    assert a.only in CASES, a.only
    small = synth.photo(200, 130, S + 5)
    assert np.array_equal(np.concatenate([photo_rows(200, 130, S + 5, y0, min(130, y0 + 37)) for y0 in range(0, 130, 37)]), small)
    t = time.time()
    entry = CASES[a.only](a)
    d = load()
    d["cases"][a.only] = entry
    save(d)
    print("%s done in %.0f s: %s" % (a.only, time.time() - t, entry), flush=True)


if __name__ == "__main__":
    main()
