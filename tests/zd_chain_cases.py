"""The texts of tests/test_zd_chain_gpu.py (GPU) and tests/test_zd_chain_cpu.py: every one puts matches of more than 255 bytes at chosen
places of the frozen phase of zip(dict), where the hybrid chain (cniic_amd/csrc/zd_chain.hpp) carries the parse across them.  The CPU file
asserts, from the restatement's stream, that each text stands where it claims to stand; the GPU file holds the library against the
restatement on them and reads the route from the stage timers.

A text is: a head of runs of the flat byte that make the entries 2, 4, ... 32 768, then 16 640, 16 896 and 257 bytes of it (a run is
followed by two bytes that occur nowhere else, as tests/zip_dict_edges.py's run_text); noise without the flat byte, in which the
dictionary fills; and behind the fill end a tail of noise with stretches of the flat byte.  A stretch stands behind a byte that occurs
nowhere else, so a symbol ends in front of it and the stretch's first match starts on its first byte; the match is the longest entry
the stretch holds.  Positions are counted from the fill end in pieces of 256, as the kernels count them.

Everything is deterministic (numpy.random.default_rng(1)) and computed once per process."""
import numpy as np

import zip_dict_edges as E
import zip_dict_ref as Z

PIECE = E.PIECE
FLAT = 7
HEAD_RUNS = (65534, 16640, 16896, 257)             # entries 2 .. 32 768; 16 384 + 256; 16 640 + 256; 256 + 1
FLAT_ENTRIES = tuple(2 ** k for k in range(1, 16)) + (16640, 16896, 257)
FRESH = (1, 2, 3, 4, 5, 6, 8, 9)                   # the separators of the head
STOP = 200                                         # the byte in front of every stretch of the tail: it occurs nowhere else
NOISE_BYTES = 600000
MAX_BREAKS = 174082                                # kZcMaxBreaks


def _noise(n, seed=1):
    alphabet = np.array([b for b in range(256) if b not in (FLAT, STOP) + FRESH], np.uint8)
    return alphabet[np.random.default_rng(seed).integers(0, alphabet.size, n)]


def base_text():
    parts = []
    for k, r in enumerate(HEAD_RUNS):
        parts += [np.full(r, FLAT, np.uint8), np.array(FRESH[2 * k:2 * k + 2], np.uint8)]
    parts.append(_noise(NOISE_BYTES))
    return np.concatenate(parts)


_cache = {}


def base(clib):
    """(the head and the noise, its fill end)"""
    if "base" not in _cache:
        text = base_text()
        info = {}
        Z.encode_c(clib, text, info)
        assert info["fill_end"] is not None and info["fill_end"] < text.size - 4096
        _cache["base"] = (text, info["fill_end"])
    return _cache["base"]


def tail(pieces, stretches, cut=None):
    """`pieces` pieces of noise with a stretch of the flat byte for every (position, length) of `stretches`; the byte in front of a
    stretch is STOP (a stretch at position 0 stands behind the fill end itself).  cut: the tail's length"""
    t = _noise(pieces * PIECE, seed=2)
    t[0] = STOP                                    # (so that the last match of the fill ends where the base text's does)
    for at, n in stretches:
        if at:
            t[at - 1] = STOP
        t[at:at + n] = FLAT
    return t[:cut] if cut is not None else t


def at(piece, offset):
    return piece * PIECE + offset


# name -> (pieces of the tail, stretches, cut).  What each stands for is asserted in tests/test_zd_chain_cpu.py (CLAIMS below).
TAILS = {
    "land 0": (8, [(at(3, 0), 512)], None),
    "land 254": (8, [(at(3, 254), 512)], None),
    "land 255": (8, [(at(3, 255), 512)], None),
    "land 0 from 255": (8, [(at(3, 255), 257)], None),
    "fly 0": (8, [(at(2, 9), 256)], None),
    "fly 1": (8, [(at(2, 9), 512)], None),
    "fly 63": (70, [(at(2, 9), 16384)], None),
    "fly 64": (70, [(at(2, 9), 16640)], None),
    "fly 65": (70, [(at(2, 9), 16896)], None),
    "fly 127": (135, [(at(2, 9), 32768)], None),
    "at the fill end": (8, [(0, 1024)], None),
    "ends on M": (8, [(at(5, 100), 512)], at(7, 100)),
    "ends before M": (8, [(at(5, 100), 512)], at(7, 101)),
    "cut by M": (8, [(at(5, 100), 512)], at(6, 144)),           # 300 of the 512 bytes: a match of 257, then short ones
    "adjacent": (8, [(at(3, 10), 256), (at(4, 11), 256)], None),
    "long into long": (8, [(at(3, 77), 768)], None),            # 512, then 256 from its landing
    "flown break": (40, [(at(2, 5), 2048), (at(12, 0), 4096 + 512)], None),   # pieces 3 .. 9, 13 .. 27 and 29 are breaks that are flown over
    "run 63": (80, [(at(1, 40), 256), (at(2 + 63, 50), 256)], None),
    "run 64": (80, [(at(1, 40), 256), (at(2 + 64, 50), 256)], None),
    "run 65": (80, [(at(1, 40), 256), (at(2 + 65, 50), 256)], None),
    "run 4095": (4110, [(at(1, 40), 256), (at(2 + 4095, 50), 256)], None),
    "run 4096": (4110, [(at(1, 40), 256), (at(2 + 4096, 50), 256)], None),
    "run 4097": (4110, [(at(1, 40), 256), (at(2 + 4097, 50), 256)], None),
    "no break": (300, [(at(3, 0), 255), (at(9, 255), 255)], None),             # entries above 255 bytes exist, none matches behind the fill end
}
# (piece, entry offset) of every long step the parse takes, its length; break pieces; break pieces the parse enters
CLAIMS = {
    "land 0": ([(3, 0, 512)], 2, 1),
    "land 254": ([(3, 254, 512)], 2, 1),
    "land 255": ([(3, 255, 512)], 2, 1),
    "land 0 from 255": ([(3, 255, 257)], 2, 1),
    "fly 0": ([(2, 9, 256)], 1, 1),
    "fly 1": ([(2, 9, 512)], 2, 1),
    "fly 63": ([(2, 9, 16384)], 64, 1),
    "fly 64": ([(2, 9, 16640)], 65, 1),
    "fly 65": ([(2, 9, 16896)], 66, 1),
    "fly 127": ([(2, 9, 32768)], 128, 1),
    "at the fill end": ([(0, 0, 1024)], 4, 1),
    "ends on M": ([(5, 100, 512)], 2, 1),
    "ends before M": ([(5, 100, 512)], 2, 1),
    "cut by M": ([(5, 100, 257)], 1, 1),
    "adjacent": ([(3, 10, 256), (4, 11, 256)], 2, 2),
    "long into long": ([(3, 77, 512), (5, 77, 256)], 3, 2),
    "flown break": ([(2, 5, 2048), (12, 0, 4096), (28, 0, 512)], 8 + 18, 3),
    "run 63": ([(1, 40, 256), (65, 50, 256)], 2, 2),
    "run 64": ([(1, 40, 256), (66, 50, 256)], 2, 2),
    "run 65": ([(1, 40, 256), (67, 50, 256)], 2, 2),
    "run 4095": ([(1, 40, 256), (4097, 50, 256)], 2, 2),
    "run 4096": ([(1, 40, 256), (4098, 50, 256)], 2, 2),
    "run 4097": ([(1, 40, 256), (4099, 50, 256)], 2, 2),
    "no break": ([], 0, 0),
}
# the long step's landing offset, and the whole pieces it flies over
LANDS = {"land 0": 0, "land 254": 254, "land 255": 255, "land 0 from 255": 0}
FLIES = {"fly 0": 0, "fly 1": 1, "fly 63": 63, "fly 64": 64, "fly 65": 65, "fly 127": 127}
RUNS = {"run 63": 63, "run 64": 64, "run 65": 65, "run 4095": 4095, "run 4096": 4096, "run 4097": 4097}
NAMES = list(TAILS)


def case(clib, name):
    """(text, reference stream, {fill_end, longest, ...})"""
    if name not in _cache:
        text0, fill_end = base(clib)
        pieces, stretches, cut = TAILS[name]
        text = np.concatenate([text0[:fill_end], tail(pieces, stretches, cut)])
        text.setflags(write=False)
        info = {}
        stream = Z.encode_c(clib, text, info)
        _cache[name] = (text, stream, info)
    return _cache[name]


def flat_remaining(text):
    """for every position: the bytes of the flat byte's stretch from there on (0 outside one)"""
    flat = (np.asarray(text) == FLAT)
    idx = np.arange(flat.size, dtype=np.int64)
    nxt = np.where(~flat, idx, flat.size)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]      # the next position that is not flat
    return np.where(flat, nxt - idx, 0)


def break_pieces(text, fill_end):
    """the pieces behind fill_end that hold a position whose longest entry has 256 bytes or more: with the flat entries the only ones
    above 255 bytes (asserted by the CPU file from the stream's table), those are the positions with 256 flat bytes or more ahead"""
    rem = flat_remaining(text)[fill_end:]
    return sorted(set((np.flatnonzero(rem >= PIECE) // PIECE).tolist()))


def long_steps(stream):
    """[(piece, offset, length)] of the parse's steps above 255 bytes, from the stream alone; and the pieces that hold a parse start"""
    fill_end, starts, lens = E.frozen_parse(stream)
    rel = starts - fill_end
    big = np.flatnonzero(lens >= PIECE)
    steps = [(int(rel[k] // PIECE), int(rel[k] % PIECE), int(lens[k])) for k in big]
    return steps, set((rel[lens > 0] // PIECE).tolist())


# ---------------------------------------------------------------- images
def band_counts(stream):
    """Z.band()'s text is not made of the flat byte, so only bounds follow from the stream: every piece with a long step of the parse is
    a break piece the parse enters.  (entered at least, breaks at least)"""
    steps, _ = long_steps(stream)
    n = len({p for p, _, _ in steps})
    return n, n
