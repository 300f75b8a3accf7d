"""The crafted texts of the zip(back) tests, with what each one claims.  tests/test_zip_back_cpu.py checks every claim on the restatements
(so that a text stands where it says it does), tests/test_zip_back.py runs the same texts through the GPU coder.

A text without repetition cannot be long: the explicit run doubles unprobed until it reaches 32 768 bytes, where the reference panics.
The long texts are therefore built on a GRID of 24-byte chunks -- 16 fresh random bytes, then the first 8 bytes of an earlier chunk.
After a look-back the probes stand at +0, +2, +4, +8, +16: the one at +16 finds the copy (one candidate), the look-back ends on the
chunk's end, and the next chunk goes the same way.  From position 0 the probes 0, 2, 4, 8, 16, 32 find nothing and 64 is +16 of chunk 2.
"""
import numpy as np

CHUNK = 24
RING = 1 << 17
FAR = 2700          # chunks: some copies come from 64 816 bytes back instead of 40


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def grid(k, seed, far=False):
    """k chunks; far: every 7th chunk from the 2700th on copies from 2700 chunks back"""
    fresh = np.random.default_rng(seed).integers(0, 256, (k, 16), dtype=np.uint8)
    out = np.empty((k, CHUNK), np.uint8)
    out[:, :16] = fresh
    src = np.arange(k) - 1
    if far:
        i = np.arange(k)
        sel = (i >= FAR) & (i % 7 == 3)
        src[sel] = i[sel] - FAR
    out[1:, 16:] = fresh[src[1:], :8]
    out[0, 16:] = np.frombuffer(rnd(8, seed + 1000), np.uint8)
    return out.tobytes()


def window_edge(distance):
    """the text's first 16 bytes again at `distance` (65 535 or 65 536), a probe standing exactly there; ten more bytes behind them.
    At 65 535 the look-back is (16, 65 535); at 65 536 position 0 is out of the window and the best left is the copy of its first 8
    bytes in chunk 1: (8, 65 496)."""
    k = 2729
    g = grid(k, 11)
    last = {65535: 23, 65536: 24}[distance]     # the last copy is longer, so that the look-back ends where the marker must stand
    g += rnd(16, 12) + g[(k - 1) * CHUNK:(k - 1) * CHUNK + last]
    assert len(g) == distance
    return g + g[:16] + rnd(10, 13)


def long_match(length):
    """a look-back of `length` bytes (32 767: the longest a header says; 32 768: the reference panics), cut by the end of the text"""
    g = grid(1366, 21)                           # 32 784 bytes, ending on a look-back's end
    return g + g[:length]


def long_match_mid():
    """a look-back of 30 000 bytes from 36 000 to 66 000, across the ring's refills, with more text behind it"""
    g = grid(1500, 31)
    return g + g[100:30100] + grid(200, 32)


SMALL = {
    # name: (text, the symbols it claims: ("E", len) / ("L", len, back))
    "distance_6":      (b"PQ" + b"abcdef" * 2 + b"ghij", [("E", 8), ("L", 6, 6), ("E", 4)]),
    "cut_by_distance": (b"PQ" + b"abcdef" * 3, [("E", 8), ("L", 6, 6), ("L", 6, 12)]),
    "period_3":        (b"PQ" + b"abc" * 4, [("E", 8), ("L", 6, 6)]),
    "period_5":        (b"PQ" + b"abcde" * 5 + b"!", [("E", 16), ("L", 10, 10), ("E", 2)]),
    "equal_lengths":   (b"PQ" + b"abcdef" + b"01234567" + b"abcdef" + b"zz" + b"abcdef" + b"!!", [("E", 16), ("L", 6, 14), ("E", 2), ("L", 6, 22), ("E", 2)]),
    "cut_by_end":      (b"PQ" + b"abcdefgh" + b"ijklmn" + b"abcdefg", [("E", 16), ("L", 7, 14)]),
    "five_left":       (b"PQ" + b"abcdef" + b"ijklmnop" + b"abcde", [("E", 21)]),
    "unprobed_offset": (b"PQ" + b"abcdef" + b"xy" + b"abcdef" + b"0123456789", [("E", 26)]),
}
UNPROBED_PROBES = [0, 2, 4, 8, 16]              # where the coder looks in "unprobed_offset": the repeat at 10 is never seen


def ring_text(rings):
    """a little over `rings` ring lengths of grid, with far copies"""
    return grid(rings * RING // CHUNK + 40, 40 + rings, far=True)


def symbols(stream):
    """the symbols of a well-formed stream, as SMALL spells them"""
    out, pos = [], 0
    while pos < len(stream):
        head = stream[pos] | (stream[pos + 1] << 8)
        if head & 0x8000:
            out.append(("L", head & 0x7FFF, stream[pos + 2] | (stream[pos + 3] << 8)))
            pos += 4
        else:
            out.append(("E", head))
            pos += 2 + head
    return out
