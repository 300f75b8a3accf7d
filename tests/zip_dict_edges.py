"""The texts of tests/test_zip_dict_edges.py (GPU) and tests/test_zip_dict_edges_cpu.py: every one stands on an edge of the frozen phase
of zip(dict) -- a threshold k_zipdict.hip or zipdict.cpp switches on.  The CPU file asserts, against the restatement, that each text
is where it claims to be; the GPU file holds the library against the restatement on them.

Everything here is deterministic (numpy.random.default_rng(1) throughout) and computed once per process."""
import struct

import numpy as np

import zip_dict_ref as Z

PIECE = 256            # positions per map of the windowed chain (kZdPiece)
WINDOW = 4096          # positions per compaction chunk and per window of the plain chain (kZdChunk)
MAX_ENTRY = 32768      # the longest entry the match kernel is given (kZdMaxEntry)
DEC_CHUNK = 2048       # symbols per chunk of the decoder's sums (kZdDecChunk)

A = 0x41
RUNS_255 = (254, 192, 224, 240, 248, 252, 254, 255)


def _noise(n, exclude=()):
    """n noise bytes, none of them in `exclude`"""
    alphabet = np.array([b for b in range(256) if b not in exclude], np.uint8)
    return alphabet[np.random.default_rng(1).integers(0, alphabet.size, n)]


def run_text(last_run=None):
    """Runs of A, each followed by two bytes that occur nowhere else: a run of 254 makes the entries AA, AAAA, ... A^128 (a pair joins
    two equal halves), and every later run r = (the longest entry so far) + (a shorter one) makes the entry A^r -- 192, 224, 240, 248,
    252, 254, 255 and, with last_run = 256, 256.  Then 400 000 noise bytes without A, in which the dictionary fills; then a tail of
    96 runs of 765 A -- three matches of 255, or two of 256 and one of 253 -- separated by 256 + k noise bytes, so that the matches
    start at many offsets of their 256-position pieces."""
    runs = RUNS_255 + ((last_run,) if last_run else ())
    fresh = list(range(1, 1 + 2 * len(runs)))
    parts = []
    for k, r in enumerate(runs):
        parts += [np.full(r, A, np.uint8), np.array(fresh[2 * k:2 * k + 2], np.uint8)]
    noise = _noise(400000 + sum(256 + k for k in range(96)), exclude=[A] + fresh)
    parts.append(noise[:400000])
    tail_at = sum(p.size for p in parts)
    at = 400000
    for k in range(96):
        parts += [np.full(765, A, np.uint8), noise[at:at + 256 + k]]
        at += 256 + k
    return np.concatenate(parts), tail_at


def flat_then_noise(flat_bytes, noise_bytes=600000):
    """test_zip_dict.py's hand-over text: a stretch of one byte, whose entries double up to the stretch's length, then noise"""
    return np.concatenate([np.full(flat_bytes, 7, np.uint8), np.random.default_rng(1).integers(0, 256, noise_bytes, dtype=np.uint8)])


def noise_text(n=6500000):
    return np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)


M_SWEEP = (0, 1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 1048575, 1048576, 1048577)
SWEEP_LEN = 1400000    # the long texts of the sweep: past fill_end + 1 048 577


def sweep_windowed():
    """noise: no entry longer than a few bytes, the windowed chain"""
    return noise_text(SWEEP_LEN)


def sweep_plain():
    """510 equal bytes -- entries of 2 .. 128 from the first 254, one of 256 from the rest -- then noise: the plain chain"""
    return np.concatenate([np.full(510, 7, np.uint8), noise_text(SWEEP_LEN - 510)])


WINDOW_END_STRETCH = 600


def window_end_text(start):
    """sweep_plain()'s first 300 000 bytes with WINDOW_END_STRETCH bytes of the flat byte at `start`"""
    t = sweep_plain()[:300000].copy()
    t[start:start + WINDOW_END_STRETCH] = 7
    return t


# ---------------------------------------------------------------- reading a reference stream
def symbol_lengths(stream):
    """(the length of every symbol's text as the decoder's table has it once the stream is read, the stream's symbols)"""
    syms = np.frombuffer(stream, "<u2")
    ln = np.zeros(65536, np.int64)
    ln[:256] = 1
    fill = syms[:2 * Z.MAX_PAIRS].tolist()
    for k in range(len(fill) // 2):
        ln[Z.FIRST_NEW + k] = ln[fill[2 * k]] + ln[fill[2 * k + 1]]
    return ln, syms


def frozen_parse(stream):
    """(fill_end, the text position at which every frozen symbol starts, its length) from the stream alone"""
    ln, syms = symbol_lengths(stream)
    fill_end = int(ln[syms[:2 * Z.MAX_PAIRS]].sum())
    lens = ln[syms[2 * Z.MAX_PAIRS:]]
    starts = fill_end + np.concatenate([[0], np.cumsum(lens)[:-1]]) if lens.size else np.zeros(0, np.int64)
    return fill_end, starts, lens


def inside_symbol(starts, lens, at):
    """(the offset of text position `at` inside the frozen symbol that covers it, that symbol's length); None before the frozen phase,
    behind the text, or where `at` is the first byte of a symbol (offset 0 is a cut at a boundary)"""
    k = int(np.searchsorted(starts, at, side="right")) - 1     # the last symbol that starts at or before `at` (empty ones sort first)
    if k < 0 or at >= starts[k] + lens[k] or at == starts[k]:
        return None
    return int(at - starts[k]), int(lens[k])


# ---------------------------------------------------------------- claimed dimensions that end inside a frozen symbol
def clip_image():
    return Z.noise(256, 256)


# hilbert-zip: the dimensions stand outside the coder, so one stream -- the records of clip_image() in scan order, 720 896 bytes of
# text, fill_end 551 924 -- serves every claim.  A noise image's frozen symbols are almost all "b 3 0000000", "g b 3 0000000" and
# "b 3 0000000 r": a record boundary cuts them 1 or 2 bytes in.  237 x 269 = 63 753 pixels is the one claim that cuts 3 bytes into a symbol
# ("r g b 3 0000000"); 163 x 391 cuts a symbol of 3 bytes.  (w', h') -> (offset of 11 w' h' inside its symbol, the symbol's length)
HILBERT_CLIPS = {(251, 241): (2, 10), (255, 255): (1, 9), (256, 255): (1, 9), (253, 256): (1, 10), (237, 269): (3, 11), (269, 237): (3, 11),
                 (210, 263): (1, 11), (160, 353): (2, 11), (163, 391): (2, 3)}
# zip(dict): the dimensions are the text's first 8 bytes, so every claim has a stream of its own
ZIP_CLIPS = {(251, 241): (1, 9), (255, 255): (2, 10), (250, 250): (1, 9), (249, 256): (2, 10), (256, 243): (1, 10)}
# hilbert-zip again: the first symbol of frozen pair 1000 (2 bytes of text at 561 250) gives way to the first symbol of 3 bytes
LONGER_AT_PAIR = 1000


def hilbert_clip_stream(clib, lin):
    """the coder's stream (no dimensions in front) of the records of lin = hilbert_linearize(clip_image())"""
    if "hilbert" not in _cache:
        _cache["hilbert"] = Z.encode_c(clib, Z.records(lin))
    return _cache["hilbert"]


def with_longer_symbol(stream):
    """(stream with the first symbol of frozen pair LONGER_AT_PAIR replaced by one whose text is a byte longer, the text position of
    that symbol, its length)"""
    ln, syms = symbol_lengths(stream)
    fill_end, starts, lens = frozen_parse(stream)
    k = 2 * LONGER_AT_PAIR
    longer = int(np.flatnonzero(ln[:Z.EOF] == lens[k] + 1)[0])
    bad = bytearray(stream)
    struct.pack_into("<H", bad, 4 * Z.MAX_PAIRS + 2 * k, longer)
    return bytes(bad), int(starts[k]), int(lens[k])


def zip_clip_text(w, h):
    """the dimensions w x h in front of the records of clip_image(): more pixels than w h claims"""
    return struct.pack("<II", w, h) + Z.records(clip_image())


# ---------------------------------------------------------------- the texts by name: (text, reference stream, info), computed once
WINDOW_END_START = 174758    # sweep_plain()'s fill_end is 171 174: the stretch's matches are [3584, 3840) and [3840, 4096) behind it

TEXTS = {
    "run 255": lambda: run_text()[0],
    "run 256": lambda: run_text(256)[0],
    "flat 65534": lambda: flat_then_noise(65534),
    "flat 98303": lambda: flat_then_noise(65534 + 32769),
    "windowed": sweep_windowed,
    "plain": sweep_plain,
    "window end": lambda: window_end_text(WINDOW_END_START),
    "many": noise_text,
}
SWEEPS = ("windowed", "plain")
_cache = {}


def case(clib, name):
    """name: a key of TEXTS, or "<sweep> + <m>": the sweep's text cut m bytes behind its fill_end"""
    if name not in _cache:
        if " + " in name:
            base, m = name.split(" + ")
            long_text, _, long_info = case(clib, base)
            text = long_text[:long_info["fill_end"] + int(m)]
        else:
            text = TEXTS[name]()
            text.setflags(write=False)
        info = {}
        stream = Z.encode_c(clib, text, info)
        _cache[name] = (text, stream, info)
    return _cache[name]


SWEEP_NAMES = ["%s + %d" % (s, m) for s in SWEEPS for m in M_SWEEP]
