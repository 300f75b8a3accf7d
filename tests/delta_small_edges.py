"""The frames of tests/test_delta_small_edges.py (GPU) and tests/test_delta_small_edges_cpu.py: every one stands at a limit the small-frame
`delta` route (cniic_amd/csrc/k_delta_small.hip, delta_small.hpp, codec.cpp delta_small_encode) is built around -- the longest code, the
kinds of run its one-wave merge takes, the size that fills the launch's LDS capacity, the sizes at which a thread's span changes, the
extremes of the number of distinct symbols at 16 384 pixels.  The CPU file proves from the oracle and from the headers' own scalar
encoder (tests/delta_small_check.cpp --keys) that each frame is where CLAIMS says it is; the GPU file runs the kernels on them.

Every frame is built from a prescribed sequence of differences along the scan (delta_limits_ref.image_from_diffs).  Everything is
deterministic (numpy.random.default_rng(SEED + k)) and computed once per process.  This module imports no GPU code."""
import functools

import numpy as np

import oracle_lib as O
from delta_limits_ref import image_from_diffs

SEED = 7700
MAX_PX = 16384          # kDeltaSmallMaxPx
MAX_CODE_LEN = 19       # kDeltaSmallMaxCodeLen
THREADS = 1024          # kDsThreads
MIN_CAP = 64            # kDsMinCap

# ------------------------------------------------------------------ 1. the chain that meets the 19-bit bound (delta_small.hpp's comment)
CHAIN_COUNTS = (1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207, 3571, 5778)
# in leaf order, rarest first.  The first one is the difference against START; the others balance: each channel's weighted sum is 0, but +1 in the third
CHAIN_DIFFS = ((128, 128, 128), (0, 0, 1), (0, 0, -3), (0, -3, 1), (0, -3, 0), (-3, 3, 0), (-3, 0, 0), (3, 0, -2), (0, 0, -2), (0, -2, 2), (0, -2, 0),
               (-2, 2, 0), (-2, 0, 0), (2, 0, -1), (0, 0, -1), (0, -1, 1), (0, -1, 0), (-1, 1, 0), (-1, 0, 0), (1, 0, 0))
CHAIN_SHAPE = (6, 2521)   # (w, h): 15 126 pixels, no square: the generic scan


def chain_diffs():
    """(128, 128, 128) first, then symbol i at the times (j + 0.5) / count_i, j = 0 .. count_i - 1, all sorted: evenly interleaved, the pixel
    stays within a few levels of 128"""
    d = np.array(CHAIN_DIFFS, np.int64)
    assert len(CHAIN_COUNTS) == len(CHAIN_DIFFS) == 20 and sum(CHAIN_COUNTS) == CHAIN_SHAPE[0] * CHAIN_SHAPE[1]
    assert ((d[1:] * np.array(CHAIN_COUNTS[1:])[:, None]).sum(axis=0) == (0, 0, 1)).all()
    times = np.concatenate([(np.arange(c) + 0.5) / c for c in CHAIN_COUNTS[1:]])
    which = np.concatenate([np.full(c, i + 1) for i, c in enumerate(CHAIN_COUNTS[1:])])
    order = np.lexsort((which, times))
    return np.concatenate([d[:1], d[which[order]]])


# ------------------------------------------------------------------ 2, 3. out-and-back pairs: a difference and its negative, from and to (0, 0, 0)
def pair_vector(idx):
    """the idx-th out vector, idx = 1 .. 8192: all distinct, none the negative of another"""
    return (idx % 128, idx // 128, 0)


def pairs_diffs(n, mult=None):
    """n differences: pair idx = 1, 2, ... out and back, pair idx repeated mult[idx - 1] times (once without mult); an odd n ends on an out
    step, and with mult the rest up to n are zero differences"""
    out = []
    idx = 1
    while len(out) < n and (mult is None or idx <= len(mult)):
        v = pair_vector(idx)
        out += [v, tuple(-c for c in v)] * (1 if mult is None else mult[idx - 1])
        idx += 1
    out = out[:n] + [(0, 0, 0)] * (n - len(out))
    return np.array(out, np.int64)


STAIRS = ((1, 97), (2, 64), (3, 33), (5, 70), (11, 10))   # (count, pairs): 2 x 274 symbols with these counts beside 2528 zero differences


def stairs_diffs():
    mult = [c for c, pairs in STAIRS for _ in range(pairs)]
    return pairs_diffs(64 * 64, mult)


# ------------------------------------------------------------------ 4. the extremes at 16 384 pixels
def equal16_diffs():
    """16 symbols, 1024 of each: eight pairs, each out and back 1024 times.  All leaves tie, so every code has 4 bits"""
    return pairs_diffs(MAX_PX, [1024] * 8)


# ------------------------------------------------------------------ 5. sizes around the minimum capacity, the span switch, and the bound
SIZES = ((9, 7), (8, 8), (13, 5), (33, 31), (32, 32), (41, 25), (23, 89), (64, 32), (3, 683), (64, 128), (127, 129), (16384, 1), (2, 8192))   # (w, h)
SIZE_PIXELS = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 8192, 16383, 16384, 16384)
LOW_STEPS = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0))


def low_diffs(n, seed):
    """about five symbols: (100, 100, 100) against START, then a walk of LOW_STEPS (half of them zero) that turns round at 0 and 255"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(LOW_STEPS), n, p=(0.5, 0.2, 0.05, 0.15, 0.1))
    cur = [100, 100, 100]
    out = [tuple(cur)]
    for k in pick[1:].tolist():
        s = LOW_STEPS[k]
        if any(not 0 <= c + v <= 255 for c, v in zip(cur, s)):
            s = tuple(-v for v in s)
        cur = [c + v for c, v in zip(cur, s)]
        out.append(s)
    return np.array(out, np.int64)


# ------------------------------------------------------------------ the inputs
def _builders():
    b = [("chain19", CHAIN_SHAPE, chain_diffs),
         ("all_distinct", (128, 128), lambda: pairs_diffs(MAX_PX)),
         ("stairs", (64, 64), stairs_diffs),
         ("flat128", (128, 128), lambda: np.array([(77, 77, 77)] + [(0, 0, 0)] * (MAX_PX - 1), np.int64)),
         ("black128", (128, 128), lambda: np.zeros((MAX_PX, 3), np.int64)),
         ("equal16", (128, 128), equal16_diffs)]
    for k, (w, h) in enumerate(SIZES):
        b.append(("low_%dx%d" % (w, h), (w, h), functools.partial(low_diffs, w * h, SEED + k)))
        b.append(("distinct_%dx%d" % (w, h), (w, h), functools.partial(pairs_diffs, w * h)))
    return b


_BUILDERS = _builders()
NAMES = tuple(name for name, _, _ in _BUILDERS)
SHAPE = {name: shape for name, shape, _ in _BUILDERS}
NAMED = NAMES[:6]
assert [w * h for w, h in SIZES] == list(SIZE_PIXELS) and len(set(NAMES)) == len(NAMES)


@functools.lru_cache(maxsize=None)
def image(name):
    w, h = SHAPE[name]
    diffs = next(fn for nm, _, fn in _BUILDERS if nm == name)()
    img = image_from_diffs(w, h, diffs)
    img.setflags(write=False)
    return img


def images(names=NAMES):
    return [image(nm) for nm in names]


@functools.lru_cache(maxsize=None)
def oracle_stream(name):
    rc, data, st = O.encode("delta", image(name))
    assert rc == 0
    return data


@functools.lru_cache(maxsize=None)
def oracle_keys(name):
    """the oracle's difference stream: a key (three 9-bit fields) per scan position"""
    return O.delta_diff(O.hilbert_linearize(image(name)))


# per input: (distinct symbols U, longest code, bytes of the stream), as the oracle gives them (tests/test_delta_small_edges_cpu.py holds them to it)
CLAIMS = {
    "chain19": (20, 19, 5115), "all_distinct": (16384, 14, 159751), "stairs": (549, 12, 6630), "flat128": (2, 1, 2071), "black128": (1, 0, 15),
    "equal16": (16, 4, 8327),
    "low_9x7": (6, 5, 70), "distinct_9x7": (63, 6, 559), "low_8x8": (6, 5, 70), "distinct_8x8": (64, 6, 567),
    "low_13x5": (6, 4, 72), "distinct_13x5": (65, 7, 576), "low_33x31": (6, 5, 308), "distinct_33x31": (1023, 10, 9470),
    "low_32x32": (6, 5, 316), "distinct_32x32": (1024, 10, 9479), "low_41x25": (6, 5, 307), "distinct_41x25": (1025, 11, 9489),
    "low_23x89": (6, 4, 590), "distinct_23x89": (2047, 11, 19198), "low_64x32": (6, 4, 590), "distinct_64x32": (2048, 11, 19207),
    "low_3x683": (6, 4, 595), "distinct_3x683": (2049, 12, 19217), "low_64x128": (6, 4, 2214), "distinct_64x128": (8192, 13, 78855),
    "low_127x129": (6, 4, 4396), "distinct_127x129": (16383, 14, 159742), "low_16384x1": (6, 4, 4406), "distinct_16384x1": (16384, 14, 159751),
    "low_2x8192": (6, 4, 4412), "distinct_2x8192": (16384, 14, 159751),
}
assert set(CLAIMS) == set(NAMES)

# per named input: what the merge of the headers' scalar encoder does and how the payload falls to the kernel's threads
# (tests/delta_small_check.cpp --keys).  Runs of pairs: full = 64 pairs, cut = ended inside the wave by the weight test, queue = ended
# by the queue's end, single = the one leaf pair taken while no branch exists.  general: the order of a general step's two picks.
MERGE = {
    "chain19": dict(leaf_runs=dict(full=0, cut=0, queue=0, single=1), branch_runs=dict(full=0, cut=0, queue=0),
                    general=dict(leaf_branch=18, branch_leaf=0), payload=dict(threads=1009, word_ends=25, most_bits=94)),
    "all_distinct": dict(leaf_runs=dict(full=127, cut=0, queue=1, single=1), branch_runs=dict(full=127, cut=0, queue=6),
                         general=dict(leaf_branch=0, branch_leaf=0), payload=dict(threads=1024, word_ends=0, most_bits=224)),
    "stairs": dict(leaf_runs=dict(full=3, cut=4, queue=0, single=1), branch_runs=dict(full=1, cut=3, queue=7),
                   general=dict(leaf_branch=3, branch_leaf=4), payload=dict(threads=1024, word_ends=12, most_bits=48)),
    "flat128": dict(leaf_runs=dict(full=0, cut=0, queue=0, single=1), branch_runs=dict(full=0, cut=0, queue=0),
                    general=dict(leaf_branch=0, branch_leaf=0), payload=dict(threads=1024, word_ends=0, most_bits=16)),
    "black128": dict(leaf_runs=dict(full=0, cut=0, queue=0, single=0), branch_runs=dict(full=0, cut=0, queue=0),
                     general=dict(leaf_branch=0, branch_leaf=0), payload=dict(threads=0, word_ends=0, most_bits=0)),
    "equal16": dict(leaf_runs=dict(full=0, cut=0, queue=1, single=1), branch_runs=dict(full=0, cut=0, queue=3),
                    general=dict(leaf_branch=0, branch_leaf=0), payload=dict(threads=1024, word_ends=0, most_bits=64)),
}


# ------------------------------------------------------------------ the short streams of the chunk and placement tests
TINY = ((4, 3), (3, 3), (1, 7), (5, 1), (2, 2), (3, 1), (1, 2), (1, 1))   # (w, h): 12, 9, 7, 5, 4, 3, 2 and 1 pixels
TINY_COUNT = (1500, 1500, 1500, 1360, 10, 10, 10, 10)                      # how many of each follow the one 128 x 128 frame of the two-chunk call


@functools.lru_cache(maxsize=None)
def chunk_kinds():
    """flat128 and one image per TINY size, three levels per channel"""
    rng = np.random.default_rng(SEED + 100)
    return [image("flat128")] + [rng.integers(0, 3, (h, w, 3)).astype(np.uint8) * 40 for w, h in TINY]


PLACEMENT_LENGTHS = (15, 24, 32, 40, 98, 72, 559)


@functools.lru_cache(maxsize=None)
def placement_kinds():
    """seven frames whose streams have PLACEMENT_LENGTHS bytes: 1, 2, 3 and 4 pixels with a difference of their own each, flat 77, and two of the inputs"""
    steps = [(10, 10, 10), (20, 20, 20), (30, 30, 30), (40, 40, 40)]
    tiny = [image_from_diffs(w, h, np.array(steps[:w * h], np.int64)) for w, h in ((1, 1), (2, 1), (3, 1), (2, 2))]
    return tiny + [np.full((20, 30, 3), 77, np.uint8), image("low_13x5"), image("distinct_9x7")]


# ------------------------------------------------------------------ the chunk size of delta_small_encode (codec.cpp), from the constants above
def ds_stride(n):
    """delta_small.hpp ds_stride: header of n leaves, every symbol under the longest code, rounded up to 16"""
    return (8 + 8 * n - 1 + (MAX_CODE_LEN * n + 7) // 8 + 15) & ~15


def frame_bytes(n):
    """codec.cpp delta_small_frame_bytes: the stream's slot and three words per pixel (pixels rounded up to 4)"""
    return ds_stride(n) + 12 * ((n + 3) & ~3)


def chunk_frames(n):
    """how many frames a chunk whose first frame has n pixels takes: 2 GiB of scratch"""
    return (2 << 30) // frame_bytes(n)
