"""Images with a PRESCRIBED sequence of differences along the scan, for tests that must KNOW how many symbols of each 512-symbol chunk of
the `delta` encoder's 16-bit stream (cniic_amd/csrc/k_delta.hip) lie outside the cube [-16, 15]^3 ("cold") before they run the encoder
(tests/test_delta_limits.py on the GPU, tests/test_delta_limits_cpu.py for the table itself).

A chunk keeps up to 64 cold symbols in a side array; with 65 the gather raises its overflow flag and the call starts again on the 32-bit
route.  From 16 cold symbols in a chunk on, their counts are added with equal keys folded together.  The tile gather (2^n squares from
64 x 64: a wave walks 1024 positions = two chunks, a block 4096 = one tile) and the per-position gather (everything else: a wave = a
chunk, a lane = 8 consecutive positions) number a chunk's cold symbols in different ways.  The cases below put known counts at those
numbers and borders; CASES declares for each the route it must take and the cold count of every chunk that has any, and
cold_per_chunk computes both from the oracle, so the crossing is asserted before a GPU runs.

How a plan is built: walk(n, cold) goes through the n positions with the current pixel in hand.  A position in `cold` takes the
difference its rule gives -- every rule returns one that is cold and keeps the pixel in 0..255 whatever the pixel is -- and every other
position takes a step of at most (-16, +15) back towards the base colour, which is hot.  +17 / -17 on one channel are both cold, so
consecutive cold symbols need no room: the pixel toggles between 0 and 17."""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O

CHUNK, COLD_MAX, FOLD_FROM = 512, 64, 16   # kChunk16, kColdPerChunk, the count from which atomic_count folds equal keys

SHAPES = {"s64": (64, 64),      # one tile, 8 chunks: the smallest size the tile gather takes
          "s128": (128, 128),   # four tiles, 32 chunks: predecessors across tile borders, chunk 7 | 8 is a tile border
          "r100": (100, 75),    # the per-position gather: 14 full chunks and one of 332
          "l700": (700, 1),     # one full chunk and one of 188
          "t8": (8, 8)}         # a single chunk of 64
# first, a middle and the last chunk (on the rectangles the last one is the partial one)
PLACES = {"s64": (0, 3, 7), "s128": (0, 13, 31), "r100": (0, 7, 14), "l700": (0, 1), "t8": (0,)}


def nsyms(shape):
    w, h = SHAPES[shape]
    return w * h


def nchunks(shape):
    return -(-nsyms(shape) // CHUNK)


def chunk_len(shape, ch):
    return min(CHUNK, nsyms(shape) - ch * CHUNK)


@functools.lru_cache(maxsize=None)
def _scan(w, h):
    return O.hilbert_iter(w, h).astype(np.int64)


def image_from_diffs(w, h, d):
    """the h x w x 3 image whose differences along the scan are d ((w h, 3) integers; d[0] is against START = (0, 0, 0))"""
    d = np.asarray(d, np.int64)
    assert d.shape == (w * h, 3)
    v = np.cumsum(d, axis=0)
    assert v.min() >= 0 and v.max() <= 255, "the planted differences leave 0..255"
    xy = _scan(w, h)
    img = np.zeros((h, w, 3), np.uint8)
    img[xy[:, 1], xy[:, 0]] = v.astype(np.uint8)
    return img


def is_cold(d):
    d = np.asarray(d)
    return ((d < -16) | (d > 15)).any(axis=-1)


def cold_per_chunk(img):
    """from the oracle's own difference stream: (cold symbols of every 512-symbol chunk, padding not counted; distinct symbols)"""
    syms = O.delta_diff(O.hilbert_linearize(img))
    cold = is_cold(O.unpack_signed(syms))
    pad = np.zeros(-(-cold.size // CHUNK) * CHUNK, np.int64)
    pad[:cold.size] = cold
    return pad.reshape(-1, CHUNK).sum(axis=1), int(np.unique(syms).size)


# ------------------------------------------------------------------ rules: (current pixel, rank of the cold symbol in its chunk) -> difference
def _toggle(c, by=17):
    return -by if c >= by else by


def rule_toggle(cur, k):
    """(17, 0, 0) from a pixel below 17, (-17, 0, 0) otherwise: one key where the walk gets back to the base in between, two where it does not"""
    return (_toggle(cur[0]), 0, 0)


def rule_distinct(cur, k):
    """a key of its own for each rank below 72: |dg| = k % 8 and |db| = k // 8 say which"""
    a, b = k % 8, k // 8
    return (_toggle(cur[0]), -a if cur[1] >= a else a, -b if cur[2] >= b else b)


def fixed(diff):
    return lambda cur, k: diff


def walk(n, cold, base=0):
    """(n, 3) differences: position p in `cold` takes cold[p](pixel, rank in the chunk), every other one a hot step towards `base`"""
    out = []
    cur = (0, 0, 0)
    rank, rank_ch = 0, -1
    for p in range(n):
        if p // CHUNK != rank_ch:
            rank, rank_ch = 0, p // CHUNK
        if p in cold:
            step = tuple(cold[p](cur, rank))
            rank += 1
        else:
            step = tuple(max(-16, min(15, base - c)) for c in cur)
        cur = tuple(c + s for c, s in zip(cur, step))
        assert 0 <= min(cur) and max(cur) <= 255, (p, cur)
        out.append(step)
    d = np.array(out, np.int64)
    assert sorted(cold) == np.nonzero(is_cold(d))[0].tolist(), "a rule gave a hot difference, or a step towards the base a cold one"
    return d


# ------------------------------------------------------------------ positions
def spread(shape, ch, count, first=0):
    """`count` positions of chunk ch, every 8th where the chunk is long enough (7 hot steps in between take the pixel back to the base)"""
    room = chunk_len(shape, ch) - first
    stride = min(8, room // count)
    assert stride >= 1, (shape, ch, count)
    return [ch * CHUNK + first + i * stride for i in range(count)]


def run(start, count):
    return list(range(start, start + count))


# the differences with ONE channel just outside the cube (-17 or 16) and the others on its faces or in its middle (-16, 0, 15): 3 x 2 x 9
def _faces():
    out = []
    for ch in range(3):
        for a in (-17, 16):
            for x in (-16, 0, 15):
                for y in (-16, 0, 15):
                    others = [x, y]
                    out.append(tuple(a if k == ch else others.pop(0) for k in range(3)))
    return out


FACES = _faces()

# all eight (+-255, +-255, +-255) from a pixel that walks between 0 and 255 per channel; three single-channel flips change which channels
# move together (cold as well): 11 consecutive cold symbols that start and end on (0, 0, 0) / (0, 255, 0)
_X = 255
EXTREMES = [(_X, _X, _X), (-_X, -_X, -_X), (_X, 0, 0), (-_X, _X, _X), (_X, -_X, -_X), (0, _X, 0), (-_X, -_X, _X), (_X, _X, -_X), (-_X, 0, 0),
            (_X, -_X, _X), (-_X, _X, -_X)]


# ------------------------------------------------------------------ the cases
# route: 16 or 32; counts: {chunk: cold symbols}, every chunk not named has none
Case = namedtuple("Case", "name shape route counts plan")
CASES = []


def _add(name, shape, route, counts, plan):
    CASES.append(Case(name, shape, route, dict(counts), plan))


def _plan(shape, cold, base=0):
    return lambda: walk(nsyms(shape), cold, base)


def _rules(positions, rule):
    return {p: rule for p in positions}


def _build_cases():
    place_name = ("first", "middle", "last")
    for shape in ("s64", "s128", "r100", "l700", "t8"):
        places = PLACES[shape]
        names = place_name if len(places) == 3 else ("first", "last") if len(places) == 2 else ("only",)
        # counts: exactly 15, 16 (the fold), 63, 64 and 65 (the side array) cold symbols in ONE chunk, spread.  One key in the first and the
        # last chunk (where the walk has the room to get back), distinct keys in the middle one.
        for ch, pn in zip(places, names):
            for count in (15, 16, 63, 64, 65):
                if count > chunk_len(shape, ch):
                    continue   # (8 x 8 has 64 symbols: no image of that size has a chunk of 65)
                rule = rule_distinct if pn == "middle" else rule_toggle
                _add("%s-count%d-%s" % (shape, count, pn), shape, 32 if count == 65 else 16, {ch: count}, _plan(shape, _rules(spread(shape, ch, count), rule)))
        # 64 in every chunk (the partial one included, as far as it has room), and the same with 65 in one of them
        full = {ch: min(64, chunk_len(shape, ch)) for ch in range(nchunks(shape))}
        cold = {}
        for ch, cnt in full.items():
            cold.update(_rules(spread(shape, ch, cnt), rule_distinct))
        _add("%s-all64" % shape, shape, 16, full, _plan(shape, cold))
        if shape != "t8":
            ch = places[-1] if shape in ("s128", "r100") else places[len(places) // 2] if shape == "s64" else 0
            cold = {p: r for p, r in cold.items() if p // CHUNK != ch}
            cold.update(_rules(spread(shape, ch, 65), rule_distinct))
            _add("%s-all64-one65" % shape, shape, 32, {**full, ch: 65}, _plan(shape, cold))
    # layout inside the chunk.  Packed: 64 consecutive from a multiple of 64 (one step of the tile gather, one ballot, all cold), and 65 from 64 j + 32
    for shape, ch, j in (("s64", 3, 2), ("s128", 0, 0), ("r100", 7, 5), ("l700", 1, 1)):
        _add("%s-packed64" % shape, shape, 16, {ch: 64}, _plan(shape, _rules(run(ch * CHUNK + 64 * j, 64), rule_toggle)))
        _add("%s-packed65" % shape, shape, 32, {ch: 65}, _plan(shape, _rules(run(ch * CHUNK + 64 * j + 32, 65), rule_toggle)))
    # one lane's 8 (the per-position gather ranks them inside the lane before its wave scan): lanes 0, 31 and 63 whole; and 9 whole lanes = 72
    for shape, ch in (("s64", 5), ("r100", 3), ("l700", 0)):
        cold = _rules(run(ch * CHUNK, 8) + run(ch * CHUNK + 31 * 8, 8) + run(ch * CHUNK + 63 * 8, 8), rule_distinct)
        _add("%s-lanes3" % shape, shape, 16, {ch: 24}, _plan(shape, cold))
    _add("r100-lanes9", "r100", 32, {9: 72}, _plan("r100", _rules([p for l in range(3, 63, 7) for p in run(9 * CHUNK + 8 * l, 8)], rule_distinct)))
    # straddle: 32 at the end of chunk c and 33 at the start of c + 1 -- 65 consecutive cold symbols and no overflow.  In the tile gather the border
    # after an even chunk is the reset in the middle of a wave's loop, after an odd one a wave border, and 7 | 8 of 128 x 128 a tile border.
    for shape, c in (("s64", 2), ("s64", 3), ("s128", 7), ("s128", 12), ("r100", 6), ("r100", 13), ("l700", 0)):
        _add("%s-straddle%d" % (shape, c), shape, 16, {c: 32, c + 1: 33}, _plan(shape, _rules(run((c + 1) * CHUNK - 32, 65), rule_toggle)))
    # keys.  The 54 differences on the cube's faces, every 8th position from 16 on (the walk climbs to the base 128 first)
    for shape, ch in (("s64", 4), ("s128", 0), ("r100", 7), ("l700", 0)):
        cold = {ch * CHUNK + 16 + 8 * i: fixed(f) for i, f in enumerate(FACES)}
        _add("%s-faces" % shape, shape, 16, {ch: len(FACES)}, _plan(shape, cold, base=128))
    # the extremes: keys 0 and the largest one, the table's first page and the last one a key reaches.  Once (11 cold symbols: one atomicAdd each) and
    # twice in a chunk (22: folded)
    for shape, ch, twice in (("s64", 0, False), ("s64", 7, True), ("s128", 13, True), ("s128", 31, False), ("r100", 0, True), ("r100", 14, False),
                             ("l700", 0, False), ("l700", 1, True), ("t8", 0, False)):
        cold = {ch * CHUNK + i: fixed(f) for i, f in enumerate(EXTREMES)}
        if twice:   # (16 hot steps take (0, 255, 0) back to the base)
            cold.update({ch * CHUNK + 32 + i: fixed(f) for i, f in enumerate(EXTREMES)})
        _add("%s-extremes%d" % (shape, 22 if twice else 11), shape, 16, {ch: 22 if twice else 11}, _plan(shape, cold))


_build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def case_image(name):
    c = BY_NAME[name]
    w, h = SHAPES[c.shape]
    img = image_from_diffs(w, h, c.plan())
    img.setflags(write=False)
    return img


def declared_counts(case):
    out = np.zeros(nchunks(case.shape), np.int64)
    for ch, n in case.counts.items():
        out[ch] = n
    return out


def smooth_image(w, h):
    """no cold symbol at all: each channel a triangle wave along the scan, steps of 7, 11 and 13"""
    t = np.arange(w * h, dtype=np.int64)[:, None] * np.array([7, 11, 13])
    v = 255 - np.abs(t % 510 - 255)
    return image_from_diffs(w, h, np.diff(v, axis=0, prepend=0))
