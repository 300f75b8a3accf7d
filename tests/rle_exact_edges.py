"""Row images for the exact `hilbert(rle)` encoder (cniic_amd/csrc/k_rle.hip: k_rle_last, k_rle_carry_local, k_rle_carry_add, k_rle_flags,
k_rle_offsets / pack_scan, k_rle_records) with colour changes PLACED on its granularities, a vectorised restatement of the codec, and a
model of the kernels' decomposition that can be made wrong on purpose (tests/test_rle_exact_edges.py on the GPU,
tests/test_rle_exact_edges_cpu.py for the table and the model).

The scan of an n x 1 image is the identity (asserted by the CPU test for every n used), so pixel i of a row is scan position i and a row
puts a segment start exactly where the table says.  A thread owns PER = 16 positions, a wave of 64 lanes WAVE = 1024, a block one CHUNK =
4096; the carry scan takes 64 chunks per wave, 1024 chunks (BLOCK positions) per block and then the blocks before; a run holds at most CAP
= 255 elements; up to 1024 chunks the run offsets come from one block, above that from pack_scan.

runs_np / stream_np restate Hilbert { compress: RLE(0.0) }::encode on the linear order: maximal segments of equal colours, ceil(len / 255)
runs each.  model() goes the kernels' way instead -- start masks per thread, last start per chunk, the two-level exclusive max-scan,
per-thread flags from (i - s) % 255, runs per chunk, offsets, records with the 16-thread look-ahead -- and takes named DEFECTS: each one is
a mistake one of the kernels could make at one of its handovers.  The CPU test asserts that the table tells every killable defect from the
right stream, which is how these tests are known to fail for a subtly wrong kernel without running one on a GPU."""
import functools
import struct
from collections import namedtuple

import numpy as np

PER, LANES = 16, 64
WAVE = PER * LANES              # 1024 positions per wave
THREADS = 256
CHUNK = THREADS * PER           # 4096
SCAN = 1024                     # chunks per block of the carry scan, and the largest count k_rle_offsets takes
BLOCK = SCAN * CHUNK            # 4 194 304
CAP = 255
SENTINEL = 0xffffffff           # "no colour has this key"

# three colours that differ pairwise in many bits of the key and are neither black nor white
A, B, C = (200, 30, 60), (17, 220, 90), (90, 90, 250)
PALETTE = (A, B, C)


# ------------------------------------------------------------------ rows
def row(n, starts, palette=PALETTE):
    """the (1, n, 3) image whose segments start at 0 and at every position of `starts` (0 < p < n), with the colours of `palette` in turn:
    two neighbouring segments always differ"""
    starts = sorted(set(int(p) for p in starts if 0 < p < n))
    assert len(palette) >= 2 and all(tuple(palette[i]) != tuple(palette[(i + 1) % len(palette)]) for i in range(len(palette)))
    edges = np.array([0] + starts + [n], np.int64)
    cols = np.array(palette, np.uint8)[np.arange(len(edges) - 1) % len(palette)]
    return np.repeat(cols, np.diff(edges), axis=0).reshape(1, n, 3)


def keys_of(lin):
    lin = np.asarray(lin, np.uint8).reshape(-1, 3).astype(np.uint32)
    return (lin[:, 0] << 16) | (lin[:, 1] << 8) | lin[:, 2]


def segment_starts_np(lin):
    k = keys_of(lin)
    return np.concatenate([np.zeros(1, np.int64), np.flatnonzero(k[1:] != k[:-1]).astype(np.int64) + 1]) if k.size else np.zeros(0, np.int64)


def runs_np(lin):
    """(start, count, colour) of every run: a segment of equal colours of length L gives ceil(L / 255) runs, all but the last of 255"""
    lin = np.asarray(lin, np.uint8).reshape(-1, 3)
    n = lin.shape[0]
    seg = segment_starts_np(lin)
    if n == 0:
        return seg, seg.copy(), lin
    length = np.diff(np.append(seg, n))
    per_seg = (length + CAP - 1) // CAP
    first = np.cumsum(per_seg) - per_seg
    start = np.repeat(seg, per_seg) + CAP * (np.arange(per_seg.sum(), dtype=np.int64) - np.repeat(first, per_seg))
    count = np.minimum(CAP, np.repeat(seg + length, per_seg) - start)
    return start, count, lin[start]


RECORD = np.dtype([("count", "u1"), ("len", "<u8"), ("rgb", "u1", (3,))])   # count.serialize, then the colour as a length and three bytes
assert RECORD.itemsize == 12


def stream_np(lin, w, h):
    start, count, colour = runs_np(lin)
    rec = np.zeros(start.size, RECORD)
    rec["count"], rec["len"], rec["rgb"] = count, 3, colour
    return struct.pack("<II", w, h) + rec.tobytes()


# ------------------------------------------------------------------ the model
# name -> (stage it lives in, can an input below 2^32 positions tell it from the right stream)
DEFECTS = {
    # segment_starts: the colour in front of a thread's 16 positions
    "lane0_uses_lane_below": ("masks", True),             # lane 0 of a wave keeps what the lane shift hands it (0) instead of reading base - 1
    "chunk_first_thread_no_predecessor": ("masks", True),   # thread 0 of a chunk never looks into the chunk before
    "fast_path_sentinel_is_black": ("masks", True),        # position 0 compared with key 0 on the 16-byte path
    "tail_path_sentinel_is_black": ("masks", True),        # ... and on the byte-wise path (an image shorter than a chunk)
    "tail_path_ignores_last_pixel": ("masks", True),       # the byte-wise path tests base + j < n - 1
    # k_rle_carry_local / k_rle_carry_add
    "carry_local_drops_wave_prefix": ("carry", True),      # `pre` left at 0: only the own wave's chunks are seen
    "carry_local_wave_total_from_lane0": ("carry", True),  # wmax written by lane 0 instead of lane 63
    "carry_add_skipped": ("carry", True),
    "carry_add_only_previous_block": ("carry", True),      # block b takes blockmax[b - 1] alone
    # k_rle_flags
    "flags_ignore_carry": ("flags", True),                 # the segment running into a chunk is looked for inside the chunk only
    "phase_in_32_bits": ("flags", False),                  # (uint32_t)(i + 1 - seg) % 255: equal below 2^32 positions, see model()
    # offsets
    "offsets_off_by_one_chunk_at_1025": ("offsets", True),   # above 1024 chunks chunk c writes where chunk c - 1 belongs
    "offsets_block_total_16_bits": ("offsets", True),      # above 1024 chunks the totals of 1024 chunks are carried modulo 2^16
    # k_rle_records
    "lookahead_15_threads": ("records", True),
    "lookahead_stops_at_chunk_end": ("records", True),     # s_f[256..271] stays zero
}
DEFECTS.update({"key_drops_bit_%d" % b: ("masks", True) for b in range(24)})   # load16px_keys / rgb_key lose bit b of every key
STAGES = ("masks", "carry", "flags", "offsets", "records")
KILLABLE = sorted(d for d, (_, k) in DEFECTS.items() if k)


def _excl_cummax(a, axis):
    inc = np.maximum.accumulate(a, axis=axis)
    ex = np.roll(inc, 1, axis=axis)
    idx = [slice(None)] * a.ndim
    idx[axis] = 0
    ex[tuple(idx)] = 0
    return inc, ex


def _bits(positions, nthreads):
    """sorted distinct positions -> a 16-bit word per thread"""
    return np.bincount(positions // PER, weights=(1 << (positions % PER)).astype(np.float64), minlength=nthreads).astype(np.uint32)


def _thread_last(m):
    """31 - clz(m) + base + 1, or 0"""
    hb = np.floor(np.log2(np.maximum(m, 1))).astype(np.int64)
    return np.where(m != 0, np.arange(m.size, dtype=np.int64) * PER + hb + 1, 0)


def model(lin, defects=(), clean=None, want_stages=False):
    """the stream of the n x 1 image lin the way k_rle.hip computes it, with the mistakes named in `defects` built in.  `clean`: the
    stages of the same row without defects (model(lin, want_stages=True)); with it, a run whose defects are all behind it and whose stage
    equals the clean one returns the clean stream at once.  Every array is per thread, per chunk or per run, never per position."""
    defects = tuple(defects)
    assert all(d in DEFECTS for d in defects), defects
    has = lambda d: d in defects   # noqa: E731
    lin = np.asarray(lin, np.uint8).reshape(-1, 3)
    n = lin.shape[0]
    nch = -(-n // CHUNK)
    T = nch * THREADS
    out = {}
    at = [STAGES.index(DEFECTS[d][0]) for d in defects]
    last_stage = max(at, default=-1)
    first_stage = min(at, default=-1) if clean is not None else -1   # the stages before it are the clean run's: taken over, not computed again

    equal = {}
    needs = {"masks": ("masks",), "carry": ("masks", "carry"), "flags": ("flags",), "offsets": ("flags", "offsets")}   # what the stages behind read

    def same(stage, value):
        """record the stage; True when the rest of the run can only repeat the clean one: no mistake is still to come, and everything the
        stages behind this one read came out as in the clean run"""
        out[stage] = value
        if clean is None:
            return False
        equal[stage] = all(np.array_equal(a, b) for a, b in zip(value, clean[stage]))
        return STAGES.index(stage) >= last_stage and all(equal[s] for s in needs[stage])

    # ---- masks: bit j of thread t <=> position 16 t + j differs from its predecessor, or is position 0 (segment_starts)
    untouched = None
    if clean is not None:
        untouched = clean["_st"]
        key, st = clean["_key"], clean["_st"]
    else:
        key = keys_of(lin)
        st = np.concatenate([np.zeros(1, np.int64), np.flatnonzero(key[1:] != key[:-1]).astype(np.int64) + 1])
        out["_key"], out["_st"] = key, st
    keep = 0xffffff   # the bits of a key that the mistaken kernel still compares
    for d in defects:
        if d.startswith("key_drops_bit_"):
            keep &= ~(1 << int(d.rsplit("_", 1)[1]))
    if keep != 0xffffff:   # a start stays one iff its two colours still differ
        inner = st[1:]
        st = np.concatenate([st[:1], inner[((key[inner] ^ key[inner - 1]) & keep) != 0]])
    fast = lambda p: (p // CHUNK + 1) * CHUNK <= n   # noqa: E731  a whole chunk inside the image (the linear image is 16-byte aligned)
    # the other mistakes change the predecessor at a few positions: those are tested again
    redo = {}   # position -> the predecessor's key as the mistaken kernel sees it

    def again(pos, prev):
        for p in np.asarray(pos, np.int64).tolist():
            redo[p] = prev
    if has("lane0_uses_lane_below"):
        pos = np.arange(0, n, WAVE, dtype=np.int64)
        again(pos[fast(pos)], 0)
    if has("chunk_first_thread_no_predecessor"):
        again(np.arange(0, n, CHUNK, dtype=np.int64), SENTINEL)
    if has("fast_path_sentinel_is_black") and fast(0):
        again([0], 0)
    if has("tail_path_sentinel_is_black") and not fast(0):
        again([0], 0)
    if redo:
        pos = np.array(sorted(redo), np.int64)
        is_start = (key[pos].astype(np.int64) & keep) != np.array([redo[p] for p in pos.tolist()], np.int64)
        st = np.union1d(np.setdiff1d(st, pos), pos[is_start])
    if has("tail_path_ignores_last_pixel") and not fast(n - 1):
        st = st[st != n - 1]
    m = clean["masks"][0] if st is untouched else _bits(st, T)
    if same("masks", (m,)):
        return clean["stream"]

    # ---- k_rle_last: the last start of every chunk, + 1 (0: none)
    mine = clean["_mine"] if first_stage > 0 else _thread_last(m)
    out["_mine"] = mine
    chunk_last = mine.reshape(nch, THREADS).max(axis=1)

    # ---- k_rle_carry_local: exclusive max over the chunks before, 64 per wave, 16 waves per block; k_rle_carry_add: the blocks before
    nb = -(-nch // SCAN)
    v = np.zeros(nb * SCAN, np.int64)
    v[:nch] = chunk_last
    v = v.reshape(nb, SCAN // LANES, LANES)
    inc, ex = _excl_cummax(v, 2)
    wmax = inc[:, :, 0] if has("carry_local_wave_total_from_lane0") else inc[:, :, LANES - 1]
    pre = _excl_cummax(wmax, 1)[1]
    if has("carry_local_drops_wave_prefix"):
        pre = np.zeros_like(pre)
    carry = np.maximum(pre[:, :, None], ex)
    blockmax = np.maximum(pre[:, -1], inc[:, -1, -1])
    if nb > 1 and not has("carry_add_skipped"):
        before = _excl_cummax(blockmax, 0)[1]
        if has("carry_add_only_previous_block"):
            before = np.concatenate([np.zeros(1, np.int64), blockmax[:-1]])
        carry = np.maximum(carry, before[:, None, None])
    carry = carry.reshape(-1)[:nch]
    if same("carry", (chunk_last, carry)):
        return clean["stream"]

    # ---- k_rle_flags: seg = the start (+ 1) of the segment running into a thread; position i starts a run iff (i + 1 - seg) % 255 == 0
    # phase_in_32_bits: the difference i + 1 - seg is never negative and, below 2^32 positions, never reaches 2^32, so its low 32 bits
    # are the difference itself: no row of the table (and none the library accepts: n < 2^32) can tell this mistake from the right code
    assert n < 1 << 32
    if first_stage > 2:
        runs, (f, chunk_runs) = clean["_runs"], clean["flags"]
    else:
        seg0 = _excl_cummax(mine.reshape(nch, THREADS), 1)[1]
        if not has("flags_ignore_carry"):
            seg0 = np.maximum(seg0, carry[:, None])
        seg0 = seg0.reshape(-1)
        # stretches of positions with one value of seg: from a thread's first position, and from every start; none is longer than 16
        begin = np.union1d(np.arange(0, n, PER, dtype=np.int64), st)
        at_start = np.zeros(begin.size, bool)
        at_start[np.searchsorted(begin, st)] = True
        seg = np.where(at_start, begin + 1, seg0[begin // PER])
        end = np.append(begin[1:], n)
        first = begin + (seg - 1 - begin) % CAP   # the first i >= begin with (i + 1 - seg) % 255 == 0
        runs = first[first < end]
        f = _bits(runs, T)
        chunk_runs = np.bincount(runs // CHUNK, minlength=nch).astype(np.int64)
    out["_runs"] = runs
    if same("flags", (f, chunk_runs)):
        return clean["stream"]

    # ---- k_rle_offsets (one block, up to 1024 chunks) / pack_scan: runs in the chunks before
    run_off = np.cumsum(chunk_runs) - chunk_runs
    total = int(chunk_runs.sum())
    if nch > SCAN:
        if has("offsets_block_total_16_bits"):
            pad = np.zeros(nb * SCAN, np.int64)
            pad[:nch] = chunk_runs
            inside = np.cumsum(pad.reshape(nb, SCAN), axis=1) - pad.reshape(nb, SCAN)
            totals = pad.reshape(nb, SCAN).sum(axis=1) & 0xffff
            run_off = (inside + (np.cumsum(totals) - totals)[:, None]).reshape(-1)[:nch]
        if has("offsets_off_by_one_chunk_at_1025"):
            run_off = np.concatenate([np.zeros(1, np.int64), run_off[:-1]])
    if same("offsets", (run_off, np.array([total]))):
        return clean["stream"]

    # ---- k_rle_records: a run ends at the next flag -- the thread's own, or the first of the next 1..16 threads (s_f: this chunk's 256
    # threads and the next chunk's first 16) -- else at the image's end.  record = words { count | 3 << 8, 0, r << 8 | g << 16 | b << 24 }
    nxt = np.append(runs[1:], n)
    reach = 15 if has("lookahead_15_threads") else 16
    seen = nxt // PER <= runs // PER + reach
    if has("lookahead_stops_at_chunk_end"):
        seen &= nxt // CHUNK == runs // CHUNK
    e = np.minimum(np.where(seen, nxt, n), n)
    words = np.zeros((total, 3), np.uint32)
    rec = np.empty((runs.size, 3), np.uint32)
    rec[:, 0] = ((e - runs) & 0xffffffff).astype(np.uint32) | np.uint32(3 << 8)
    rec[:, 1] = 0
    px = lin[runs].astype(np.uint32)
    rec[:, 2] = (px[:, 0] << 8) | (px[:, 1] << 16) | (px[:, 2] << 24)
    ch = runs // CHUNK
    where = run_off[ch] + (np.arange(runs.size, dtype=np.int64) - (np.cumsum(chunk_runs) - chunk_runs)[ch])
    ok = where < total
    words[where[ok]] = rec[ok]
    out["records"] = (words,)
    out["stream"] = struct.pack("<II", n, 1) + words.astype("<u4").tobytes()
    return out if want_stages else out["stream"]


# ------------------------------------------------------------------ the cases
# group: the number of the issue's list (1 edges of the start test, 2 single-bit colours, 3 the cap's phase, 4 carry inside a block,
# 5 carry across blocks, 6 offsets at 1024 | 1025 chunks, 7 the records' look-ahead, 8 tiny rows); build() -> the (1, n, 3) image;
# facts: what the CPU test checks from runs_np before a GPU runs
Case = namedtuple("Case", "name group n build facts")
CASES = []
GROUPS = {1: "edges", 2: "bits", 3: "cap", 4: "carry_block", 5: "carry_blocks", 6: "offsets", 7: "lookahead", 8: "tiny"}


def _add(name, group, n, build, **facts):
    CASES.append(Case(name, group, n, build, facts))


def _row_case(name, group, n, starts, palette=PALETTE, **facts):
    starts = [p for p in starts if 0 < p < n]
    _add(name, group, n, lambda: row(n, starts, palette), starts=starts, **facts)


N1 = 2 * CHUNK + 17            # two whole chunks and a partial one of 17 positions: one whole thread and a thread of one position
N1W = 2 * CHUNK + WAVE + 17    # ... of 1041: a wave edge on the byte-wise path
N3 = 3 * CHUNK + 17

# where group 1 puts its single change (name -> (n, p))
EDGES = {
    "per0": (N1, 16 * 37), "per15": (N1, 16 * 37 + 15),
    "wave0": (N1, 2 * WAVE), "wave_last": (N1, 2 * WAVE - 1), "wave0_chunk1": (N1, CHUNK + WAVE),
    "chunk0": (N1, CHUNK), "chunk_last": (N1, CHUNK - 1),
    "tail_chunk0": (N1, 2 * CHUNK), "before_tail": (N1, 2 * CHUNK - 1), "tail_per15": (N1, 2 * CHUNK + 15), "last_pixel": (N1, N1 - 1),
    "tail_per0": (N1W, 2 * CHUNK + 48), "tail_per15_w": (N1W, 2 * CHUNK + 47), "tail_wave0": (N1W, 2 * CHUNK + WAVE),
    "tail_wave_last": (N1W, 2 * CHUNK + WAVE - 1), "last_pixel_w": (N1W, N1W - 1),
}
S_VALUES = {"0": 0, "1": 1, "15": 15, "16": 16, "chunk_m1": CHUNK - 1, "chunk": CHUNK, "chunk_m254": CHUNK - 254, "chunk_m255": CHUNK - 255}
L_VALUES = (254, 255, 256, 509, 510, 511, 4080, 4335)
BITS_BASE = (0x5a, 0xa5, 0x3c)
NOISE_SEED = 20


def _flip(rgb, b):
    k = (rgb[0] << 16 | rgb[1] << 8 | rgb[2]) ^ (1 << b)
    return (k >> 16 & 255, k >> 8 & 255, k & 255)


def noise_row(n, seed=NOISE_SEED):
    """two colours drawn per pixel: about one run per two pixels"""
    pick = np.random.default_rng(seed + n).integers(0, 2, n)
    return np.array([A, B], np.uint8)[pick].reshape(1, n, 3)


def alternating_chunks_row(n):
    """even chunks: A B A B ... (4096 runs); odd chunks: flat C (17 runs)"""
    p = np.arange(n)
    idx = np.where((p // CHUNK) % 2 == 0, p % 2, 2)
    return np.array(PALETTE, np.uint8)[idx].reshape(1, n, 3)


def _build_cases():
    # 1. thread, wave and chunk edges of the segment-start test: one change exactly at p; none at p with changes at p - 1 and p + 1
    for name, (n, p) in EDGES.items():
        _row_case("edge_%s_change" % name, 1, n, [p], at=p)
        _row_case("edge_%s_none" % name, 1, n, [p - 1, p + 1], at=p)
    _row_case("edge_flat", 1, N1, [])
    _row_case("edge_flat_w", 1, N1W, [])
    _row_case("edge_first_black", 1, N1, [3000], palette=((0, 0, 0), A))      # position 0 counts whatever its colour: keys 0 and 2^24 - 1
    _row_case("edge_first_white", 1, N1, [3000], palette=((255, 255, 255), A))
    # 2. one start whose two colours differ in bit b of the key only, in a whole chunk and in the partial last one
    for b in range(24):
        pal = (BITS_BASE, _flip(BITS_BASE, b))
        _row_case("bit%02d_whole" % b, 2, N1, [CHUNK + 777 + 37 * b], palette=pal, bit=b)
        _row_case("bit%02d_tail" % b, 2, N1, [2 * CHUNK + 1 + b % 16], palette=pal, bit=b)
    # 3. the cap's phase: a segment of length L from s
    for sn, s in S_VALUES.items():
        for L in L_VALUES:
            _row_case("cap_L%d_s_%s" % (L, sn), 3, N3, [s, s + L], seg=(s, L))
    for r in (0, 1, 254):   # ... and one that ends with the image
        L = 5 * CAP + r
        _row_case("cap_ends_at_n_r%d" % r, 3, N3, [N3 - L], seg=(N3 - L, L), residue=r)
    # 4. no start for 65 and 66 whole chunks: across a wave of k_rle_carry_local.  From position 5, and from the last position of chunk 3
    for whole in (65, 66):
        for sn, s in (("from5", 5), ("from_chunk3_last", 4 * CHUNK - 1)):
            nxt = (s // CHUNK + 1 + whole) * CHUNK + 9
            _row_case("carry%d_%s" % (whole, sn), 4, nxt - 9 + CHUNK + 17, [s, nxt], seg=(s, nxt - s), whole=whole)
    # 5. across blocks of 1024 chunks
    for sn, s in (("m1", BLOCK - 1), ("0", BLOCK), ("p1", BLOCK + 1)):
        _row_case("block_start_at_%s" % sn, 5, BLOCK + 3 * CHUNK + 1, [s, s + 3 * CHUNK], at=s)
    _row_case("block_without_a_start", 5, 2 * BLOCK + CHUNK + 5, [BLOCK - 3, 2 * BLOCK + 7])
    # (with the next start at 2 BLOCK + 7 no run of the long segment starts inside block 2 -- the first one would, at 2 BLOCK + 188 -- so what block
    # 2 takes in from the blocks before it shows in no byte; with the next start behind that position it does)
    _row_case("block_without_a_start_far", 5, 2 * BLOCK + CHUNK + 5, [BLOCK - 3, 2 * BLOCK + 1000])
    _row_case("blocks_all_flat", 5, 2 * BLOCK + CHUNK + 5, [])
    # 6. the offsets at 1024 | 1025 chunks with many runs per chunk, and at 1 | 2 chunks
    for nn, n in (("1024_chunks", BLOCK), ("1025_chunks", BLOCK + 1), ("1_chunk", CHUNK), ("2_chunks", CHUNK + 1)):
        _add("noise_%s" % nn, 6, n, functools.partial(noise_row, n), nchunks=-(-n // CHUNK))
        _add("alternating_%s" % nn, 6, n, functools.partial(alternating_chunks_row, n), nchunks=-(-n // CHUNK))
    # 7. the look-ahead: a whole run of 255 between two starts, from thread offset j; `where`: in the middle of a chunk, in a chunk's last 16
    # threads (the next flag is among the next chunk's first 16 threads), in the last chunk with nothing behind it
    for j in (0, 1, 15):
        _row_case("look_j%d_mid" % j, 7, N3, [16 * 50 + j, 16 * 50 + j + CAP], run=16 * 50 + j)
        _row_case("look_j%d_chunk_end" % j, 7, N3, [CHUNK - 16 * 3 + j, CHUNK - 16 * 3 + j + CAP], run=CHUNK - 16 * 3 + j)
        s = 3 * CHUNK + 304 + j
        _row_case("look_j%d_image_end" % j, 7, s + CAP, [s], run=s, ends_image=True)
    _add("look_4096_runs_then_flat", 7, 2 * CHUNK, lambda: alternating_chunks_row(2 * CHUNK), nchunks=2)
    # 8. tiny rows
    for n in (1, 2, 15, 16, 17, 255, 256, 257):
        _row_case("tiny_%d_flat" % n, 8, n, [])
        _row_case("tiny_%d_alternating" % n, 8, n, range(1, n), palette=(A, B))
    _row_case("tiny_1_black", 8, 1, [], palette=((0, 0, 0), A))


_build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
LARGE = 1 << 20   # rows from here on are built once and kept by whoever needs them, not cached here


@functools.lru_cache(maxsize=None)
def _small_image(name):
    img = BY_NAME[name].build()
    img.setflags(write=False)
    return img


def case_image(name):
    c = BY_NAME[name]
    if c.n >= LARGE:
        img = c.build()
        img.setflags(write=False)
        return img
    return _small_image(name)


# ------------------------------------------------------------------ where a record starts, for a failure's message
def first_difference(got, want):
    """None, or a line that names the first differing record and the chunk, thread and j its run starts at (from the expected stream)"""
    if got == want:
        return None
    if got[:8] != want[:8]:
        return "the headers differ: %r != %r" % (got[:8], want[:8])
    a, b = np.frombuffer(got[8:len(got) - (len(got) - 8) % 12], np.uint8).reshape(-1, 12), np.frombuffer(want[8:], np.uint8).reshape(-1, 12)
    k = min(len(a), len(b))
    bad = np.flatnonzero((a[:k] != b[:k]).any(axis=1))
    r = int(bad[0]) if bad.size else k
    pos = int(b[:r, 0].astype(np.int64).sum())
    what = "record %d of %d (got %d records, %d bytes)" % (r, len(b), len(a), len(got))
    if r < len(b):
        what += ": expected count %d colour %s" % (b[r, 0], tuple(b[r, 9:]))
    if r < len(a):
        what += ", got count %d len-field %s colour %s" % (a[r, 0], bytes(a[r, 1:9]).hex(), tuple(a[r, 9:]))
    return "%s; its run starts at position %d = chunk %d (block %d, wave-lane %d), thread %d, j %d" % (
        what, pos, pos // CHUNK, pos // BLOCK, pos // CHUNK % LANES, pos % CHUNK // PER, pos % PER)
