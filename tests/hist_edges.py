"""Images and symbol streams for the histogram (cniic_amd/csrc/k_hist.hip: k_hist_rgb, k_hist_rgb_bytes, the partition k_part_pass<false>,
k_part_colscan, k_part_starts, k_part_pass<true>, k_part_hist, and the compaction k_compact_count, k_compact_scan_local, k_compact_scan_add,
k_compact_write) with keys and counts PLACED on its granularities, and a model of the kernels' decomposition that can be made wrong on
purpose (tests/test_hist_edges.py on the GPU, tests/test_hist_edges_cpu.py for the table and the model).  No GPU and no library here.

A key is r << 16 | g << 8 | b.  Its top 12 bits are its BUCKET (one 4096-entry slice of the table), the low 12 its remainder.  The fill has
three routes (route()): below PART_MIN_PX pixels from a 16-byte aligned base 16-pixel groups with the tail (< 16 pixels) done by block 0;
from any other base single pixels; from PART_MIN_PX pixels on an aligned base the partition: PART_BLOCKS blocks own ceil(groups / 512)
groups each and the last one the tail, a bucket of t entries is counted in t // 16384 + (t % 16384 != 0) work items, stored where it is
one item and added where it is several.  The compaction reads the table in chunks of SCAN_CHUNK entries (16 per thread in the write,
quads strided by 256 in the count), scans the chunks' sums in parts of SCAN_PART chunks and leaves rank + 1 in every occupied bin.

The witness everywhere is np.unique(keys, return_counts=True).  model_fill / model_compact go the kernels' way instead -- per block, per
bucket, per work item, per chunk, per part -- and take named defects (FILL_DEFECTS, COMPACT_DEFECTS): each one is a mistake one of the
kernels could make at one of its handovers.  The CPU test asserts that the table tells every one of them from the right histogram."""
import functools
from collections import namedtuple

import numpy as np

PART_BITS = 12
BUCKETS = 4096            # kPartBuckets: one per top 12 key bits
BINS = 4096               # kPartBins: table entries per bucket
PART_BLOCKS = 512
PART_SUB = 16384          # entries per work item of k_part_hist
PART_MIN_PX = 1 << 20
PART_SEGS, PART_ROWS = 8, 64          # k_part_colscan: 8 segments of 64 blocks per column
SCAN_CHUNK = 4096
SCAN_PER_THREAD = 16
SCAN_THREADS = 256
SCAN_PART = 1024
PART_KEYS = SCAN_PART * SCAN_CHUNK    # 2^22 keys per scan part
DIRECT_GRID_CAP = 256 * 8             # blocks of k_hist_rgb
BYTES_GRID_CAP = 256 * 16             # blocks of k_hist_rgb_bytes
N0 = PART_MIN_PX
OFFSETS = (1, 4, 8, 15, 16)           # byte offsets of the device views the GPU test reads every fill case from
KIND_OF_BITS = {24: 1, 27: 2}         # SYM_RGB, SYM_SIGNED


# ------------------------------------------------------------------ builders
def key(bucket, rem):
    return (int(bucket) << PART_BITS) | int(rem)


def keys_of(lin):
    lin = np.asarray(lin, np.uint8).reshape(-1, 3).astype(np.uint32)
    return (lin[:, 0] << 16) | (lin[:, 1] << 8) | lin[:, 2]


def rgb_of(keys):
    k = np.asarray(keys, np.uint32)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=-1).astype(np.uint8)


def pairs(keys, counts):
    """(keys u32, counts i64) of distinct keys, in the order listed"""
    k, c = np.asarray(keys, np.int64).reshape(-1), np.asarray(counts, np.int64).reshape(-1)
    c = np.broadcast_to(c, k.shape).copy()
    assert k.size and (c > 0).all() and np.unique(k).size == k.size and k.min() >= 0
    return k.astype(np.uint32), c


def sorted_pairs(p):
    o = np.argsort(p[0], kind="stable")
    return p[0][o], p[1][o].astype(np.uint64)


def _arrange(k, order, seed):
    """the pixels' keys k (ascending) in one of the four orders"""
    if order == "ascending":
        return k
    if order == "descending":
        return k[::-1].copy()
    if order == "shuffled":
        return k[np.random.default_rng(seed).permutation(k.size)]
    if order == "striped":   # round after round over the buckets that still have pixels: pixel i goes to bucket i mod 4096 where counts allow
        b = (k >> PART_BITS).astype(np.int64)
        first = np.searchsorted(b, b, side="left")
        return k[np.lexsort((b, np.arange(k.size) - first))]
    raise ValueError(order)


def image_of(p, order="shuffled", last=None, seed=1):
    """the (n, 3) uint8 pixels with exactly the (key, count) pairs p -- and those of `last`, one pixel each, behind all of them in the order
    listed ("the listed pixels last")"""
    ks, cs = sorted_pairs(p)
    assert ks.max() < 1 << 24
    k = _arrange(np.repeat(ks, cs.astype(np.int64)), order, seed)
    if last is not None:
        lk = np.asarray(last, np.uint32)
        assert np.unique(lk).size == lk.size and not np.isin(lk, ks).any()
        k = np.concatenate([k, lk])
    lin = rgb_of(k)
    assert lin.shape == (int(cs.sum()) + (0 if last is None else len(last)), 3)
    return lin


def stream_of(p, seed=1):
    """a u32 symbol stream with exactly the pairs p, shuffled"""
    ks, cs = sorted_pairs(p)
    s = np.repeat(ks, cs.astype(np.int64))
    return s[np.random.default_rng(seed).permutation(s.size)] if s.size > 1 else s


def witness(keys):
    k, c = np.unique(np.asarray(keys, np.uint32), return_counts=True)
    return k.astype(np.uint32), c.astype(np.uint64)


# ------------------------------------------------------------------ the kernels' arithmetic
def route(addr, npx):
    """which kernels hist_rgb_dense sends npx pixels at byte address addr to"""
    if npx == 0:
        return "none"
    if addr & 15 == 0 and PART_MIN_PX <= npx < 1 << 32:
        return "partition"
    return "direct" if addr & 15 == 0 else "bytes"


def part_items(t):
    t = np.asarray(t, np.int64)
    return t // PART_SUB + (t % PART_SUB != 0)


def part_split(npx, floor=False):
    """groups, gpb and the groups [g0, g1) of every block of the two passes; the last block also owns pixels 16 groups .. npx - 1"""
    groups = npx // 16
    gpb = groups // PART_BLOCKS if floor else -(-groups // PART_BLOCKS)
    g0 = np.minimum(np.arange(PART_BLOCKS, dtype=np.int64) * gpb, groups)
    g1 = np.minimum(g0 + gpb, groups)
    return groups, gpb, g0, g1


def max_items(npx):
    return BUCKETS + npx // PART_SUB      # the grid of k_part_hist


def nparts(bits):
    return ((1 << bits) // SCAN_CHUNK + SCAN_PART - 1) // SCAN_PART


# ------------------------------------------------------------------ the model of the fill
# name -> the step it lives in
FILL_DEFECTS = {
    "gpb_rounds_down": "pass",                      # gpb = groups / 512: the groups behind 512 gpb belong to nobody
    "tail_dropped": "pass",                         # no block counts or scatters pixels 16 groups .. npx - 1
    "tail_also_by_block0": "pass",                  # ... or block 0 does as well as the last one (k_hist_rgb's habit)
    "total_from_last_segment": "colscan",           # total[k] = the last 64 blocks' sum, without the seven segments before
    "items_round_down": "starts",                   # a bucket of several items forgets the one that is not full: max(1, t / 16384)
    "cursor_without_blocks_before": "scatter",      # cur[k] = start[k]: every block scatters from the bucket's first entry
    "remainder_keeps_11_bits": "scatter",           # key & 2047
    "search_stops_at_first_equal": "hist",          # the first bucket whose item[] equals the one found: an empty bucket in front of it
    "several_items_overwrite": "hist",              # a bucket of several items stores each item's counts instead of adding them
    "last_item_not_clipped": "hist",                # in a bucket of several items ne = 16384 for the last one too: it reads into the next bucket
}
FILL_STEPS = ("pass", "colscan", "starts", "scatter", "hist")
COMPACT_DEFECTS = {
    "count_drops_last_quad_row": "count",           # j < 3: in-chunk positions 3072 .. 4095 are not counted
    "count_max_from_first_of_quad": "count",        # the largest count looks at q.x alone
    "part_total_misses_last_chunk": "scan_local",   # parttot = ex, not ex + v
    "max_from_part0_only": "scan_local",            # total[1] collected by block 0 alone
    "add_only_the_part_before": "scan_add",         # block p adds parttot[p - 1] alone
    "chunk_offset_16_bits": "write",                # blockoff[] read as 16 bits
    "rank_without_inblock_prefix": "write",         # rank = blockoff + the place inside the thread's 16 entries
}
COMPACT_STEPS = ("count", "scan_local", "scan_add", "write")


def _sparse(tk, cnt=None):
    """table keys (with repeats) -> ascending keys and their counts"""
    if cnt is None:
        k, c = np.unique(tk, return_counts=True)
        return k.astype(np.uint32), c.astype(np.uint64)
    k, inv = np.unique(tk, return_inverse=True)
    return k.astype(np.uint32), np.bincount(inv, weights=cnt, minlength=k.size).astype(np.uint64)


def model_direct(k):
    """k_hist_rgb: the 16-pixel groups over the grid's threads (a grid-stride loop: every group once, whatever the grid), the tail by block 0"""
    groups = k.size // 16
    grid = min(max(-(-groups // 256), 1), DIRECT_GRID_CAP)
    assert groups <= grid * 256, "below PART_MIN_PX pixels the loop makes one trip"
    return _sparse(np.concatenate([k[:groups * 16], k[groups * 16:][:256]]))


def model_partition(k, defects=(), memo=None):
    """the table (ascending keys, counts) of the pixels' keys k the way the five partition kernels fill it.  Where the kernels' order is
    free (LDS cursors), pixels of a block go to a bucket in image order; memory that a mistaken kernel reads without having written is 0,
    and what it writes outside an array is dropped.  memo: a dict of the caller's, for runs over the same k: which block works on which
    pixel, and in which order, is the same for every defect behind the passes' split and is kept there"""
    has = lambda d: d in defects   # noqa: E731
    assert all(d in FILL_DEFECTS for d in defects), defects
    n = k.size
    split = tuple(has(d) for d in ("gpb_rounds_down", "tail_dropped", "tail_also_by_block0"))
    if memo is None or split not in memo:
        groups, gpb, g0, g1 = part_split(n, floor=has("gpb_rounds_down"))
        # ---- who owns a pixel (both passes): the entries a block works on
        grp = np.arange(groups * 16, dtype=np.int64) // 16
        owner = np.minimum(grp // max(gpb, 1), PART_BLOCKS)          # PART_BLOCKS: nobody
        assert ((grp >= g0[np.minimum(owner, PART_BLOCKS - 1)]) & (grp < g1[np.minimum(owner, PART_BLOCKS - 1)]) | (owner == PART_BLOCKS)).all()
        ek, eo = [k[:groups * 16]], [owner]
        tail = k[groups * 16:]
        if not has("tail_dropped"):
            ek.append(tail), eo.append(np.full(tail.size, PART_BLOCKS - 1, np.int64))
        if has("tail_also_by_block0"):
            ek.append(tail), eo.append(np.zeros(tail.size, np.int64))
        ek, eo = np.concatenate(ek).astype(np.int64), np.concatenate(eo)
        ek, eo = ek[eo < PART_BLOCKS], eo[eo < PART_BLOCKS]
        cell = eo * BUCKETS + (ek >> PART_BITS)
        # ---- k_part_pass<false>: counts[b][k]
        counts = np.bincount(cell, minlength=PART_BLOCKS * BUCKETS).reshape(PART_SEGS, PART_ROWS, BUCKETS)
        # (for k_part_pass<true>: the entries block by block and bucket by bucket, and each one's place among its block's entries of its bucket)
        order = np.argsort(cell, kind="stable")
        cs = cell[order]
        rank = np.arange(cs.size, dtype=np.int64) - np.searchsorted(cs, cs, side="left")
        kept = (counts, cs, rank, ek[order] & (BINS - 1))
        if memo is not None:
            memo[split] = kept
    counts, cs, rank, rem = kept if memo is None else memo[split]
    # ---- k_part_colscan: per column, 8 segments of 64 rows -> exclusive prefix over the blocks, and the column's total
    inseg = np.cumsum(counts, axis=1) - counts
    part = counts.sum(axis=1)
    run0 = np.cumsum(part, axis=0) - part
    prefix = (inseg + run0[:, None, :]).reshape(PART_BLOCKS, BUCKETS)
    total = part[-1] if has("total_from_last_segment") else run0[-1] + part[-1]
    # ---- k_part_starts: exclusive scans of the entries and of the work items
    items = part_items(total)
    if has("items_round_down"):
        items = np.where(total > 0, np.maximum(1, total // PART_SUB), 0)
    start = np.concatenate([[0], np.cumsum(total)])
    item = np.concatenate([[0], np.cumsum(items)])
    # ---- k_part_pass<true>: payload[cur[bucket]++] = remainder
    cur = start[:BUCKETS][None, :] + (0 if has("cursor_without_blocks_before") else prefix)
    pos = np.broadcast_to(cur, (PART_BLOCKS, BUCKETS)).reshape(-1)[cs] + rank
    payload = np.zeros(n, np.int64)
    ok = pos < n
    payload[pos[ok]] = (rem & 2047 if has("remainder_keeps_11_bits") else rem)[ok]
    # ---- k_part_hist: one block per work item
    its = np.arange(min(int(item[BUCKETS]), max_items(n)), dtype=np.int64)
    kb = np.searchsorted(item[:BUCKETS], its, side="right") - 1       # the last bucket whose first item is <= it
    if has("search_stops_at_first_equal"):
        kb = np.searchsorted(item[:BUCKETS], item[kb], side="left")
    e0 = (start[kb] + (its - item[kb]) * PART_SUB) & 0xffffffff
    ne = np.minimum(PART_SUB, (start[kb + 1] - e0) & 0xffffffff)
    if has("last_item_not_clipped"):
        ne = np.where(item[kb + 1] - item[kb] > 1, PART_SUB, ne)
    rep = np.repeat(its, ne)
    e = e0[rep] + np.arange(rep.size, dtype=np.int64) - (np.cumsum(ne) - ne)[rep]
    rep, e = rep[e < n], e[e < n]
    tk = (kb[rep] << PART_BITS) | payload[e]
    if not has("several_items_overwrite"):
        return _sparse(tk)           # a store into the zeroed slice and an add are the same
    # every item stores the bins it counted: of a bucket's items the last one to write a bin wins (here: the highest item)
    u, c = np.unique(tk * (its.size + 1) + rep, return_counts=True)
    t = u // (its.size + 1)
    lastof = np.append(t[1:] != t[:-1], True)
    return t[lastof].astype(np.uint32), c[lastof].astype(np.uint64)


def model_fill(lin, npx, addr=0, defects=(), memo=None):
    """the dense table after hist_rgb_dense, as (ascending keys, counts).  The defects are the partition's: the other routes ignore them"""
    k = keys_of(np.asarray(lin).reshape(-1, 3)[:npx])
    r = route(addr, npx)
    if r == "partition":
        return model_partition(k, tuple(defects), memo)
    if r == "direct":
        return model_direct(k)
    return _sparse(k)                # k_hist_rgb_bytes: pixel by pixel


# ------------------------------------------------------------------ the model of the compaction
SENT = 0xffffffff


def model_compact(keys, counts, bits, defects=()):
    """hist_compact_count and hist_compact_write over the table that holds counts[i] at keys[i] (ascending) and 0 elsewhere ->
    dict(n_unique, max_count, keys, counts, ranks): the pairs written (SENT where nothing was), and rank + 1 as left in the bins of `keys`"""
    has = lambda d: d in defects   # noqa: E731
    assert all(d in COMPACT_DEFECTS for d in defects), defects
    keys, counts = np.asarray(keys, np.int64), np.asarray(counts, np.int64)
    nchunks = (1 << bits) // SCAN_CHUNK
    P = nparts(bits)
    chunk, pos = keys >> 12, keys & (SCAN_CHUNK - 1)
    # ---- k_compact_count: thread t of a chunk reads quads t, t + 256, t + 512, t + 768
    row = (pos >> 2) // SCAN_THREADS
    seen = row < 3 if has("count_drops_last_quad_row") else np.ones(keys.size, bool)
    nz = np.bincount(chunk[seen], minlength=nchunks)
    blockmax = np.zeros(nchunks, np.int64)
    look = seen & (pos % 4 == 0) if has("count_max_from_first_of_quad") else seen
    lc, lv = chunk[look], counts[look]
    if lc.size:
        firsts = np.flatnonzero(np.append(True, lc[1:] != lc[:-1]))      # (the keys ascend: a chunk's entries lie together)
        blockmax[lc[firsts]] = np.maximum.reduceat(lv, firsts)
    # ---- k_compact_scan_local: a part of 1024 chunks per block
    pad = P * SCAN_PART
    v = np.zeros(pad, np.int64)
    v[:nchunks] = nz
    v = v.reshape(P, SCAN_PART)
    ex = np.cumsum(v, axis=1) - v
    parttot = ex[:, -1] + (0 if has("part_total_misses_last_chunk") else v[:, -1])
    max_count = int(blockmax[:SCAN_PART].max() if has("max_from_part0_only") else blockmax.max())
    # ---- k_compact_scan_add (more than one part)
    if P > 1:
        before = np.concatenate([[0], parttot[:-1]]) if has("add_only_the_part_before") else np.cumsum(parttot) - parttot
        total = int(before[-1] + parttot[-1])
    else:
        before = np.zeros(1, np.int64)
        total = int(ex[0, -1] + v[0, -1])
    blockoff = (ex + before[:, None]).reshape(-1)[:nchunks]
    # ---- k_compact_write: 16 consecutive entries per thread; rank = blockoff + occupied entries of the threads before + those before it in its own
    thread = keys >> 4
    idx = np.arange(keys.size, dtype=np.int64)
    first_of_thread = np.maximum.accumulate(np.where(np.append(True, thread[1:] != thread[:-1]), idx, 0))
    first_of_chunk = np.maximum.accumulate(np.where(np.append(True, chunk[1:] != chunk[:-1]), idx, 0))
    excl = 0 if has("rank_without_inblock_prefix") else first_of_thread - first_of_chunk
    off = blockoff[chunk]
    if has("chunk_offset_16_bits"):
        off = off & 0xffff
    rank = off + excl + (idx - first_of_thread)
    ok = rank < total
    out_k = np.full(total, SENT, np.uint32)
    out_c = np.zeros(total, np.uint64)
    out_k[rank[ok]] = keys[ok]
    out_c[rank[ok]] = counts[ok]
    return dict(n_unique=total, max_count=max_count, keys=out_k, counts=out_c, ranks=rank + 1)


def same_compaction(m, keys, counts):
    """is the model's result the right one for the pairs (ascending keys, counts)"""
    return (m["n_unique"] == keys.size and m["max_count"] == (int(counts.max()) if keys.size else 0) and np.array_equal(m["keys"], keys)
            and np.array_equal(m["counts"], counts) and np.array_equal(m["ranks"], np.arange(1, keys.size + 1)))


# ------------------------------------------------------------------ the fill cases
# build() -> the (n, 3) pixels (n >= npx; the case reads the first npx); image: cases with one name there share the pixels
FillCase = namedtuple("FillCase", "name group npx image build facts")
FILL, FILL_GROUPS = [], {"F1": "threshold", "F2": "block ownership", "F3": "one colour", "F4": "item edges", "F5": "all buckets",
                         "F6": "sparse buckets", "F7": "full slice", "F8": "order", "F9": "direct-route tails"}


def _fill(name, group, npx, build, image=None, **facts):
    FILL.append(FillCase(name, group, npx, image or name, build, facts))


def _walk(i, mul=2531):
    """a fixed multiplicative walk over the 4096 remainders (2531 is odd: i -> i mul mod 4096 is one to one)"""
    return (np.asarray(i, np.int64) * mul) & (BINS - 1)


# F1: 1023 colours x 1025 pixels = 2^20 - 1 in the even buckets 0 .. 2044, then 32 pixels of colours found nowhere else, in odd buckets
# above 2048 that are otherwise empty
F1_NPX = (N0 - 1, N0, N0 + 1, N0 + 15, N0 + 16, N0 + 17, N0 + 31)
F1_BULK = pairs((2 * np.arange(1023) << PART_BITS) | _walk(np.arange(1023), 1237), 1025)
F1_LAST = ((2049 + 64 * np.arange(32)) << PART_BITS) | np.where(np.arange(32) % 8 == 0, 0, np.where(np.arange(32) % 8 == 7, BINS - 1, _walk(np.arange(32) + 5, 331)))


def f1_image():
    return image_of(F1_BULK, "shuffled", last=F1_LAST, seed=11)


# F5: 4096 buckets x 256 pixels: four colours of 61, 63, 65 and 67 pixels whose remainders follow the walk
def f5_pairs():
    b = np.repeat(np.arange(BUCKETS), 4)
    j = np.tile(np.arange(4), BUCKETS)
    return pairs((b << PART_BITS) | _walk(4 * b + j + 5 * (b // 1024)), 61 + 2 * j)     # (+ 5 per 1024 buckets: 4 b alone comes round after 1024)


# F2: F5's pixels, 16 more of five of its colours, and 7 pixels of colours found only in the tail
F2_NPX = N0 + 16 * 5 + 7


def f2_parts():
    k, c = f5_pairs()
    c = c.copy()
    c[[40, 4001, 8002, 12003, 16004]] += 16
    have = set(k.tolist())
    last = []
    for j in range(7):
        b = 300 + 577 * j
        last.append(next(key(b, r) for r in (0, 4095, 2048, 1, 2, 3, 4, 5) if key(b, r) not in have and key(b, r) not in last))
    return (k, c), np.array(last, np.uint32)


def f2_image():
    bulk, last = f2_parts()
    return image_of(bulk, "shuffled", last=last, seed=12)


# F4: buckets of exactly 16383, 16384, 16385, 32768 and 32769 pixels over the remainders 0, 4095 and 1234 (and 77 for two of them), a bucket of
# 16385 pixels of one remainder, and a filler of 64 pixels per colour (the last one 62, to land on 2^20), 3 or 4 colours in each of the
# 4090 other buckets
F4_SPECIAL = {0: 16383, 1: 16384, 2047: 16385, 2048: 32768, 4095: 32769}
F4_SINGLE = (1000, 16385, 2222)          # bucket, pixels, its one remainder


def f4_pairs():
    ks, cs = [], []
    for b, t in F4_SPECIAL.items():
        rems = [0, BINS - 1, 1234] + ([77] if t > PART_SUB + 1 else [])
        share = [t // len(rems)] * len(rems)
        share[-1] += t - sum(share)
        ks += [key(b, r) for r in rems]
        cs += share
    ks.append(key(F4_SINGLE[0], F4_SINGLE[2]))
    cs.append(F4_SINGLE[1])
    rest = N0 - sum(cs)
    others = np.array([b for b in range(BUCKETS) if b not in F4_SPECIAL and b != F4_SINGLE[0]])
    nfill = -(-rest // 64)
    i = np.arange(nfill)
    fk = (others[i % others.size] << PART_BITS) | _walk(i)
    fc = np.full(nfill, 64)
    fc[-1] = rest - 64 * (nfill - 1)
    return pairs(np.concatenate([ks, fk]), np.concatenate([cs, fc]))


def _f6_pairs(which):
    if which == "only_4095":
        return pairs((4095 << PART_BITS) | _walk(np.arange(1024)), 1024)
    if which == "only_0_and_4095":
        return pairs(np.concatenate([_walk(np.arange(512)), (4095 << PART_BITS) | _walk(np.arange(512), 1237)]), 1024)
    if which == "only_odd":
        b = np.repeat(np.arange(1, BUCKETS, 2), 2)
        return pairs((b << PART_BITS) | _walk(b + 2048 * np.tile(np.arange(2), BUCKETS // 2)), 256)
    if which == "only_0_to_7":
        b = np.repeat(np.arange(8), 128)
        return pairs((b << PART_BITS) | _walk(np.arange(1024), 1237), 1024)
    raise ValueError(which)


F6_BUCKETS = {"only_4095": [4095], "only_0_and_4095": [0, 4095], "only_odd": list(range(1, BUCKETS, 2)), "only_0_to_7": list(range(8))}
F7_BUCKET = 0x5A5
F9_NPX = (1, 15, 16, 17, 4096 + 15, 256 * 8 * 256 * 16 + 5)
F9_PALETTE = pairs((np.arange(61) * 274177) & 0xfffffe, 1)[0]     # 61 even keys; the unique last pixels are odd


def f9_image(npx):
    nlast = min(32, npx)
    last = ((np.arange(nlast, dtype=np.int64) * 520021 + 12345) & 0xffffff) | 1
    assert np.unique(last).size == nlast
    nb = npx - nlast
    if nb == 0:
        return rgb_of(last)
    c = np.full(61, nb // 61)
    c[:nb % 61] += 1
    sel = c > 0
    return image_of((F9_PALETTE[sel], c[sel]), "shuffled", last=last, seed=19)


def _build_fill():
    for npx in F1_NPX:
        _fill("F1_npx_N0%+d" % (npx - N0), "F1", npx, f1_image, image="F1", tail=npx % 16, route="direct" if npx < N0 else "partition")
    _fill("F2_block_ownership", "F2", F2_NPX, f2_image, groups=65541, gpb=129, idle=(509, 510, 511), tail=7)
    _fill("F3_one_colour", "F3", N0, lambda: image_of(pairs([0xABCDEF], [N0])), bucket=0xABC, items=64)
    _fill("F4_item_edges", "F4", N0, lambda: image_of(f4_pairs(), "shuffled", seed=14))
    _fill("F5_all_buckets", "F5", N0, lambda: image_of(f5_pairs(), "shuffled", seed=15))
    for which in F6_BUCKETS:
        _fill("F6_" + which, "F6", N0, functools.partial(lambda w: image_of(_f6_pairs(w), "shuffled", seed=16), which), buckets=F6_BUCKETS[which])
    _fill("F7_full_slice", "F7", N0, lambda: image_of(pairs((F7_BUCKET << PART_BITS) | np.arange(BINS), 256), "shuffled", seed=17), bucket=F7_BUCKET)
    for order in ("ascending", "descending", "shuffled", "striped"):
        _fill("F8_" + order, "F8", N0, functools.partial(lambda o: image_of(f4_pairs(), o, seed=18), order), order=order)
    for npx in F9_NPX:
        _fill("F9_npx_%d" % npx, "F9", npx, functools.partial(f9_image, npx), tail=npx % 16, route="direct" if npx < N0 else "partition")


_build_fill()
FILL_BY_NAME = {c.name: c for c in FILL}
FILL_NAMES = [c.name for c in FILL]
assert len(FILL_BY_NAME) == len(FILL)
KILL_MAX_PX = 1 << 21     # the CPU test runs the defects on the cases up to here (the one larger case gets the model without a defect)


@functools.lru_cache(maxsize=2)
def fill_image(image):
    c = next(c for c in FILL if c.image == image)
    lin = c.build()
    lin.setflags(write=False)
    return lin


def fill_pixels(name):
    c = FILL_BY_NAME[name]
    return fill_image(c.image)[:c.npx]


# ------------------------------------------------------------------ the compaction cases
# build(bits) -> the pairs (any order); bits: the table sizes the case runs at
CompCase = namedtuple("CompCase", "name group bits build facts")
COMP, COMP_GROUPS = [], {"C1": "ends", "C2": "chunk edges", "C3": "thread, wave and quad edges", "C4": "full chunk", "C5": "part edges", "C6": "empty parts",
                         "C7": "one key per chunk", "C8": "long run", "C9": "full table", "C10": "counts"}


def _comp(name, group, build, bits=(24, 27), **facts):
    COMP.append(CompCase(name, group, bits, build, facts))


def top(bits):
    return (1 << bits) - 1


def _few(keys):
    """counts 3, 10, 6, 13, 9, 5, ... (3 + 7 i mod 11): no two neighbours alike"""
    keys = np.asarray(keys, np.int64)
    return pairs(keys, 3 + 7 * np.arange(keys.size) % 11)


C3_POS = (3, 4, 15, 16, 1023, 1024)
C10_LIGHT = 100
C10_HEAVY = (1 << 20, 255, 256, 65535, 65536)


def c5_keys(bits):
    ps = (1, 2, 3) + ((16, 31) if bits == 27 else ())
    return np.array([PART_KEYS * p + d for p in ps for d in (-1, 0)], np.int64)


def c6_keys(bits, parts):
    """five keys in each of the parts named (-1: the last one)"""
    P = nparts(bits)
    at = np.array([0, 4095, 123 * SCAN_CHUNK + 77, PART_KEYS // 2 + 9, PART_KEYS - 1], np.int64)
    return np.concatenate([(p % P) * PART_KEYS + at for p in parts])


def c7_keys(bits):
    ch = np.arange((1 << bits) // SCAN_CHUNK, dtype=np.int64)
    return ch * SCAN_CHUNK + (37 * ch) % SCAN_CHUNK


def c10_where(bits):
    return {"chunk0": 2, "part0_last_chunk": (SCAN_PART - 1) * SCAN_CHUNK + 4095, "part2": 2 * PART_KEYS + 5 * SCAN_CHUNK + 1, "top": top(bits)}


def c10_pairs(bits, where, heavy):
    hk = c10_where(bits)[where]
    light = (np.arange(C10_LIGHT, dtype=np.int64) + 1) * ((1 << bits) // (C10_LIGHT + 1)) + 3
    assert hk not in light
    return pairs(np.concatenate([[hk], light]), np.concatenate([[heavy], np.ones(C10_LIGHT, np.int64)]))


def _build_comp():
    _comp("C1_zero", "C1", lambda bits: _few([0]))
    _comp("C1_top", "C1", lambda bits: _few([top(bits)]))
    _comp("C1_zero_and_top", "C1", lambda bits: _few([0, top(bits)]))
    _comp("C2_chunk_edges", "C2", lambda bits: _few([4094, 4095, 4096, 4097]))
    _comp("C3_chunk_start", "C3", lambda bits: _few(C3_POS))
    _comp("C3_chunk_end", "C3", lambda bits: _few([5 * SCAN_CHUNK + 4095 - p for p in C3_POS]))
    _comp("C3_table_end", "C3", lambda bits: _few([top(bits) - p for p in C3_POS]))
    _comp("C4_full_chunk", "C4", lambda bits: _few(np.concatenate([[6 * SCAN_CHUNK + 100], 7 * SCAN_CHUNK + np.arange(SCAN_CHUNK), [8 * SCAN_CHUNK + 200]])))
    _comp("C5_part_edges", "C5", lambda bits: _few(c5_keys(bits)))
    _comp("C6_only_last_part", "C6", lambda bits: _few(c6_keys(bits, (-1,))), parts=(-1,))
    _comp("C6_only_first_part", "C6", lambda bits: _few(c6_keys(bits, (0,))), parts=(0,))
    _comp("C6_only_parts_1_and_3", "C6", lambda bits: _few(c6_keys(bits, (1, 3))), parts=(1, 3))
    _comp("C7_one_key_per_chunk", "C7", lambda bits: _few(c7_keys(bits)))
    _comp("C8_long_run", "C8", lambda bits: pairs(2 * PART_KEYS - (1 << 15) + np.arange(1 << 16), 1))
    _comp("C9_full_table", "C9", lambda bits: pairs(np.arange(1 << 24), 1), bits=(24,))
    for where in ("chunk0", "part0_last_chunk", "part2", "top"):
        for heavy in C10_HEAVY:
            _comp("C10_%s_x%d" % (where, heavy), "C10", functools.partial(lambda w, h, bits: c10_pairs(bits, w, h), where, heavy), where=where, heavy=heavy)


_build_comp()
COMP_BY_NAME = {c.name: c for c in COMP}
assert len(COMP_BY_NAME) == len(COMP)
COMP_IDS = [(c.name, bits) for c in COMP for bits in c.bits]


def comp_pairs(name, bits):
    """the case's pairs, ascending"""
    return sorted_pairs(COMP_BY_NAME[name].build(bits))


def comp_stream(name, bits):
    if name == "C9_full_table":
        return np.arange(1 << 24, dtype=np.uint32)     # (one symbol each: their order is of no interest to an atomic per symbol)
    return stream_of(COMP_BY_NAME[name].build(bits), seed=len(name) + bits)
