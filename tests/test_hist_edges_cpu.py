"""The case table and the model of tests/hist_edges.py, without a GPU: the granularities are the kernels' (read out of k_hist.hip), every case
stands where it claims to (bucket sizes, work items per bucket, which blocks own groups, which chunks and scan parts are occupied -- all
derived from the built data), the model without a defect equals np.unique for every case -- and the part that says what the GPU test is
worth: every defect of the model changes the result of at least one case, and which GROUPS of cases catch which defect.

defect                          step        caught by
gpb_rounds_down                 pass        F1 F2              (a pixel count whose groups are no multiple of 512)
tail_dropped                    pass        F1 F2              (a tail; F9's tails are on the direct route)
tail_also_by_block0             pass        F1 F2
total_from_last_segment         colscan     F1 .. F8
items_round_down                starts      F4 F8              (a bucket of more than one item that is no multiple of 16384)
cursor_without_blocks_before    scatter     F1 .. F8
remainder_keeps_11_bits         scatter     F1 .. F8
search_stops_at_first_equal     hist        F1 F3 F6 F7        (an empty bucket in front of an occupied one)
several_items_overwrite             hist        F3 F4 F6 F7 F8     (a bucket of several items with a colour in two of them)
last_item_not_clipped           hist        F4 F8              (a bucket of several items that ends inside an item, with a bucket behind it)
count_drops_last_quad_row       count       C1 .. C10          (a key at in-chunk position 3072 or above)
count_max_from_first_of_quad    count       C1 C2 C3 C6 C10    (the largest count at a position that is no multiple of 4)
part_total_misses_last_chunk    scan_local  C1 C3 C5 .. C10    (a key in the last chunk of a part)
max_from_part0_only             scan_local  C1 C3 C5 C6 C8 C10 (the largest count outside part 0)
add_only_the_part_before        scan_add    C1 .. C10          (a key more than one part in front of the last part: n_unique itself is wrong)
chunk_offset_16_bits            write       C9                 (65536 occupied bins in front of a chunk)
rank_without_inblock_prefix     write       C3 C4 C6 C8 C9     (two occupied threads in one chunk)

(test_every_defect_is_caught_and_by_which_groups holds the table above to what the model gives.)  The largest count (total[1]) reaches no
output of the histogram calls.  Its one reader is the Huffman code stage's large-alphabet route, whose leaf sort takes its number of radix
passes from it; that route starts at 32768 distinct symbols, so the GPU test forces it (OPT_HUF_GPU_CODES_MIN = 0) for C2, C5, C7 and C10 and
asserts the passes: 1, 2, 2, 3 and 3 for C10's heavy counts 255, 256, 65535, 65536 and 2^20."""
import functools
import os
import re

import numpy as np
import pytest

import hist_edges as E

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cniic_amd", "csrc")
N0 = E.N0

ALL_F = {"F%d" % i for i in range(1, 9)}       # every group on the partition (F9 is the direct route's)
ALL_C = {"C%d" % i for i in range(1, 11)}
CAUGHT_BY = {
    "gpb_rounds_down": {"F1", "F2"},
    "tail_dropped": {"F1", "F2"},
    "tail_also_by_block0": {"F1", "F2"},
    "total_from_last_segment": ALL_F,
    "items_round_down": {"F4", "F8"},
    "cursor_without_blocks_before": ALL_F,
    "remainder_keeps_11_bits": ALL_F,
    "search_stops_at_first_equal": {"F1", "F3", "F6", "F7"},
    "several_items_overwrite": {"F3", "F4", "F6", "F7", "F8"},
    "last_item_not_clipped": {"F4", "F8"},
    "count_drops_last_quad_row": ALL_C,
    "count_max_from_first_of_quad": {"C1", "C2", "C3", "C6", "C10"},
    "part_total_misses_last_chunk": ALL_C - {"C2", "C4"},
    "max_from_part0_only": {"C1", "C3", "C5", "C6", "C8", "C10"},
    "add_only_the_part_before": ALL_C,
    "chunk_offset_16_bits": {"C9"},
    "rank_without_inblock_prefix": {"C3", "C4", "C6", "C8", "C9"},
}


def test_the_granularities_are_the_kernels():
    src = open(os.path.join(CSRC, "k_hist.hip")).read()
    assert re.search(r"constexpr int kPartBits = %d;" % E.PART_BITS, src)
    assert re.search(r"constexpr uint32_t kPartBuckets = 1u << \(24 - kPartBits\);", src) and E.BUCKETS == 1 << (24 - E.PART_BITS) == 4096
    assert re.search(r"constexpr uint32_t kPartBins = 1u << kPartBits;", src) and E.BINS == 1 << E.PART_BITS == 4096
    assert re.search(r"constexpr uint32_t kPartBlocks = %d;" % E.PART_BLOCKS, src)
    assert re.search(r"constexpr uint32_t kPartSub = %d;" % E.PART_SUB, src)
    assert re.search(r"constexpr int kPartCols = 32;", src) and "segs = 256 / kPartCols, rows = kPartBlocks / segs" in src
    assert (E.PART_SEGS, E.PART_ROWS) == (256 // 32, E.PART_BLOCKS // (256 // 32))
    assert re.search(r"constexpr int kScanThreads = %d;" % E.SCAN_THREADS, src)
    assert re.search(r"constexpr int kScanPerThread = %d;" % E.SCAN_PER_THREAD, src)
    assert re.search(r"constexpr int kScanChunk = kScanThreads \* kScanPerThread;", src) and E.SCAN_CHUNK == E.SCAN_THREADS * E.SCAN_PER_THREAD == 4096
    # the route condition of hist_rgb_dense
    assert "(reinterpret_cast<uintptr_t>(rgb_d) & 15) == 0 && npx >= (1u << 20) && npx < (1ull << 32)" in src and E.PART_MIN_PX == 1 << 20
    assert "} else if ((reinterpret_cast<uintptr_t>(rgb_d) & 15) == 0) {" in src
    assert "const uint64_t groups = npx / 16, gpb = ceil_div(groups, kPartBlocks);" in src
    assert "if (blockIdx.x == gridDim.x - 1) {" in src and "if (blockIdx.x == 0) {" in src      # the partition's tail, the direct route's tail
    assert "ceil_div(groups, 256), 1), 256 * 8);" in src and E.DIRECT_GRID_CAP == 256 * 8
    assert "std::min<uint64_t>(ceil_div(npx, 256), 256 * 16);" in src and E.BYTES_GRID_CAP == 256 * 16
    assert "return t / kPartSub + (t % kPartSub != 0);" in src
    assert "const uint32_t max_items = kPartBuckets + (uint32_t)(npx / kPartSub);" in src and E.max_items(N0) == 4096 + 64
    assert "if (nsub == 1) slice[i] = cnt; else atomicAdd(&slice[i], cnt);" in src
    # the scan parts
    assert "const uint32_t nparts = (nblocks + 1023) / 1024;" in src and E.SCAN_PART == 1024
    for kernel in ("k_compact_scan_local", "k_compact_scan_add", "k_part_starts"):
        assert re.search(r"__global__ __launch_bounds__\(1024\) void %s\(" % kernel, src), kernel
    assert "const uint32_t i = blockIdx.x * 1024 + threadIdx.x;" in src
    assert E.nparts(24) == 4 and E.nparts(27) == 32 and E.PART_KEYS == 1 << 22
    assert "const uint32_t quad = j * kScanThreads + threadIdx.x;" in src
    assert "val[i] = rank + 1;" in src
    assert "atomicMax(reinterpret_cast<unsigned long long *>(total + 1), (unsigned long long)m);" in src
    # what the API makes of the symbol kinds
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "const uint32_t bits = sym_kind == CNIIC_SYM_RGB ? 24 : 27;" in capi and E.KIND_OF_BITS == {24: 1, 27: 2}


def test_route():
    assert E.route(0, N0 - 1) == "direct" and E.route(16, N0 - 1) == "direct" and E.route(0, N0) == "partition" and E.route(4096 + 16, N0) == "partition"
    for off in (1, 4, 8, 15):
        assert E.route(off, 5) == E.route(256 + off, N0 + 31) == "bytes"
    assert E.route(0, 0) == "none" and E.route(0, 1 << 32) == "direct"
    assert [E.route(o, N0) for o in E.OFFSETS] == ["bytes"] * 4 + ["partition"]


def test_builders_return_what_they_claim():
    p = E.pairs([5, 1 << 23, 77, (1 << 24) - 1], [3, 1, 40, 2])
    want = E.sorted_pairs(p)
    assert want[0].tolist() == [5, 77, 1 << 23, (1 << 24) - 1] and want[1].tolist() == [3, 40, 1, 2]
    for order in ("ascending", "descending", "shuffled", "striped"):
        lin = E.image_of(p, order)
        assert lin.shape == (46, 3) and lin.dtype == np.uint8
        k, c = E.witness(E.keys_of(lin))
        assert np.array_equal(k, want[0]) and np.array_equal(c, want[1]), order
    assert (np.diff(E.keys_of(E.image_of(p, "ascending")).astype(np.int64)) >= 0).all()
    assert (np.diff(E.keys_of(E.image_of(p, "descending")).astype(np.int64)) <= 0).all()
    assert E.keys_of(E.image_of(p, "striped"))[:4].tolist() == [5, 1 << 23, (1 << 24) - 1, 5]     # round after round over the buckets 0, 2048, 4095
    lin = E.image_of(p, "shuffled", last=[9, 8])
    assert E.keys_of(lin)[-2:].tolist() == [9, 8] and lin.shape == (48, 3)
    assert E.rgb_of([0x123456]).tolist() == [[0x12, 0x34, 0x56]] and E.keys_of(E.rgb_of([0x123456, 7])).tolist() == [0x123456, 7]
    with pytest.raises(AssertionError):
        E.pairs([1, 1], [2, 2])
    with pytest.raises(AssertionError):
        E.image_of(p, last=[5])
    s = E.stream_of(E.pairs([1 << 26, 3], [2, 5]))
    assert s.dtype == np.uint32 and sorted(s.tolist()) == [3] * 5 + [1 << 26] * 2


# ------------------------------------------------------------------ fill
def _buckets(k):
    return np.bincount(k >> E.PART_BITS, minlength=E.BUCKETS)


@functools.lru_cache(maxsize=None)
def _fill_kills(name):
    """the fill defects that change this case's table; with it: the model without a defect, and the compaction behind it, equal np.unique"""
    c = E.FILL_BY_NAME[name]
    lin = E.fill_pixels(name)
    want = E.witness(E.keys_of(lin))
    memo = {}
    got = E.model_fill(lin, c.npx, memo=memo)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    assert E.same_compaction(E.model_compact(got[0], got[1], 24), *want), name
    got = E.model_fill(lin, c.npx, addr=1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, "the byte route")
    if E.route(0, c.npx) != "partition" or c.npx > E.KILL_MAX_PX:
        return frozenset()
    kills = set()
    for d in E.FILL_DEFECTS:
        got = E.model_fill(lin, c.npx, defects=(d,), memo=memo)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            kills.add(d)
    return frozenset(kills)


@pytest.mark.parametrize("name", E.FILL_NAMES)
def test_fill_case_stands_where_it_claims_to(name):
    c = E.FILL_BY_NAME[name]
    F = c.facts
    lin = E.fill_pixels(name)
    assert lin.shape == (c.npx, 3) and lin.dtype == np.uint8
    k = E.keys_of(lin).astype(np.int64)
    sizes = _buckets(k)
    items = E.part_items(sizes)
    groups, gpb, g0, g1 = E.part_split(c.npx)
    assert groups * 16 + c.npx % 16 == c.npx and (g1[-1] == groups or gpb * E.PART_BLOCKS >= groups)
    assert np.union1d(np.concatenate([np.arange(a, b) for a, b in zip(g0, g1)]), []).size == groups      # every group has one owner
    if "route" in F:
        assert E.route(0, c.npx) == F["route"]
    else:
        assert E.route(0, c.npx) == "partition" and c.npx >= N0
    assert [E.route(o, c.npx) for o in E.OFFSETS] == ["bytes"] * 4 + [E.route(0, c.npx)]
    if "tail" in F:
        assert c.npx - 16 * groups == F["tail"]
    if c.group == "F1":
        whole = E.keys_of(E.fill_image("F1")).astype(np.int64)
        assert whole.size == N0 + 31 and c.npx in E.F1_NPX and E.F1_NPX == (N0 - 1, N0, N0 + 1, N0 + 15, N0 + 16, N0 + 17, N0 + 31)
        last = whole[N0 - 1:]
        assert last.size == 32 and np.array_equal(last, E.F1_LAST)
        assert (_buckets(whole)[last >> E.PART_BITS] == 1).all()                       # alone in their buckets: alone in the image
        assert {0, E.BINS - 1} <= set((last & (E.BINS - 1)).tolist())
        inside = c.npx - (N0 - 1)
        assert np.array_equal(np.flatnonzero(sizes == 1), np.sort(last[:inside] >> E.PART_BITS))   # exactly the first `inside` of them are read
        bulk = whole[:N0 - 1]
        assert not (np.sort(bulk) == bulk).all() and np.array_equal(E.witness(bulk)[0], np.sort(E.F1_BULK[0]))
    if c.group == "F2":
        assert (groups, gpb) == (F["groups"], F["gpb"]) == (65541, 129) and c.npx == N0 + 16 * 5 + 7
        owns = g1 > g0
        assert owns[:509].all() and not owns[509:].any() and F["idle"] == (509, 510, 511) and g1[508] - g0[508] == 65541 - 508 * 129 == 9
        tail = k[16 * groups:]
        assert tail.size == 7 and not np.isin(tail, k[:16 * groups]).any() and np.unique(tail).size == 7      # colours found only in the tail
    if c.group == "F3":
        assert np.flatnonzero(sizes).tolist() == [F["bucket"]] == [0xABCDEF >> 12] and items[F["bucket"]] == F["items"] == 64
        assert np.unique(k).tolist() == [0xABCDEF]
    if c.group in ("F4", "F8"):
        assert c.npx == N0
        for b, t in E.F4_SPECIAL.items():
            rems = np.unique(k[k >> E.PART_BITS == b] & (E.BINS - 1))
            assert sizes[b] == t and items[b] == t // 16384 + (t % 16384 != 0) and rems.size >= 3 and {0, 4095} <= set(rems.tolist())
        assert sorted(E.F4_SPECIAL.values()) == [16383, 16384, 16385, 32768, 32769]
        assert [int(items[b]) for b in sorted(E.F4_SPECIAL)] == [1, 1, 2, 2, 3]
        b, t, r = E.F4_SINGLE
        assert sizes[b] == t == 16385 and items[b] == 2 and np.unique(k[k >> E.PART_BITS == b]).tolist() == [E.key(b, r)]
        rest = np.delete(sizes, list(E.F4_SPECIAL) + [b])
        assert rest.size == 4090 and set(rest.tolist()) <= {190, 192, 254, 256} and (np.delete(items, list(E.F4_SPECIAL) + [b]) == 1).all()
        kk, cc = E.witness(k)
        filler = ~np.isin(kk >> E.PART_BITS, list(E.F4_SPECIAL) + [b])
        assert sorted(set(cc[filler].tolist())) == [62, 64]
    if c.group == "F8":
        order = F["order"]
        if order == "ascending":
            assert (np.diff(k) >= 0).all()
        elif order == "descending":
            assert (np.diff(k) <= 0).all()
        elif order == "striped":
            m = E.BUCKETS * 190
            assert np.array_equal(k[:m] >> E.PART_BITS, np.arange(m) % E.BUCKETS)     # pixel i in bucket i mod 4096 while every bucket has pixels
        else:
            assert not (np.diff(k) >= 0).all() and not (np.diff(k) <= 0).all()
    if c.group == "F5":
        assert (sizes == 256).all() and (items == 1).all()
        rems = np.sort((k & (E.BINS - 1)).reshape(-1)[np.argsort(k >> E.PART_BITS, kind="stable")].reshape(E.BUCKETS, 256), axis=1)
        assert all(not np.array_equal(rems[i], rems[i + 1]) for i in range(E.BUCKETS - 1))      # no two neighbouring buckets look alike
        assert len({tuple(np.unique(r).tolist()) for r in rems}) == E.BUCKETS                     # ... nor any two at all
    if c.group == "F6":
        assert np.flatnonzero(sizes).tolist() == F["buckets"] and c.npx == N0
        assert len(set(sizes[F["buckets"]].tolist())) == 1 and (sizes[F["buckets"][0]] % E.PART_SUB == 0 or sizes[F["buckets"][0]] < E.PART_SUB)
    if c.group == "F7":
        assert np.flatnonzero(sizes).tolist() == [F["bucket"]] and items[F["bucket"]] == 64
        kk, cc = E.witness(k)
        assert np.array_equal(kk & (E.BINS - 1), np.arange(E.BINS)) and (cc == 256).all()
    if c.group == "F9":
        nlast = min(32, c.npx)
        kk, cc = E.witness(k)
        assert (cc[np.searchsorted(kk, k[-nlast:])] == 1).all() and np.unique(k[-nlast:]).size == nlast      # the last pixels are unique colours
        if c.npx > E.DIRECT_GRID_CAP * 256 * 16:
            # k_hist_rgb's grid-stride loop would wrap from here on -- but from 2^20 pixels on an aligned base goes to the partition, so the
            # loop never wraps; what does wrap at this size is the byte route's (4096 blocks x 256 pixels), eight times over
            assert c.npx == 256 * 8 * 256 * 16 + 5 and E.route(0, c.npx) == "partition" and c.npx // (E.BYTES_GRID_CAP * 256) == 8
    _fill_kills(name)


def test_the_fill_table_reaches_what_it_is_there_for():
    names = set(E.FILL_NAMES)
    assert {"F1_npx_N0%+d" % d for d in (-1, 0, 1, 15, 16, 17, 31)} <= names
    assert {"F6_" + w for w in ("only_4095", "only_0_and_4095", "only_odd", "only_0_to_7")} <= names
    assert {"F8_" + o for o in ("ascending", "descending", "shuffled", "striped")} <= names
    assert {"F9_npx_%d" % n for n in (1, 15, 16, 17, 4096 + 15, 256 * 8 * 256 * 16 + 5)} <= names
    assert {c.group for c in E.FILL} == set(E.FILL_GROUPS) and E.OFFSETS == (1, 4, 8, 15, 16)
    assert np.array_equal(E.sorted_pairs(E.f4_pairs())[0], E.witness(E.keys_of(E.fill_pixels("F8_striped")))[0])   # F8 is F4's multiset


# ------------------------------------------------------------------ compaction
@functools.lru_cache(maxsize=None)
def _comp_kills(name, bits):
    keys, counts = E.comp_pairs(name, bits)
    stream = E.comp_stream(name, bits)
    if stream.size <= 1 << 21:      # (the full table's stream is its keys)
        w = E.witness(stream)
        assert np.array_equal(w[0], keys) and np.array_equal(w[1], counts), (name, bits)
    else:
        assert np.array_equal(stream, keys) and (counts == 1).all()
    assert E.same_compaction(E.model_compact(keys, counts, bits), keys, counts), (name, bits)
    return frozenset(d for d in E.COMPACT_DEFECTS if not E.same_compaction(E.model_compact(keys, counts, bits, (d,)), keys, counts))


@pytest.mark.parametrize("name,bits", E.COMP_IDS)
def test_compaction_case_stands_where_it_claims_to(name, bits):
    c = E.COMP_BY_NAME[name]
    keys, counts = E.comp_pairs(name, bits)
    k = keys.astype(np.int64)
    top = (1 << bits) - 1
    assert k.max() <= top and (np.diff(k) > 0).all() and counts.dtype == np.uint64
    chunks, parts = np.unique(k >> 12), np.unique(k // E.PART_KEYS)
    pos = k & 4095
    P = E.nparts(bits)
    if name == "C1_zero_and_top":
        assert k.tolist() == [0, top]
    if c.group == "C2":
        assert k.tolist() == [4094, 4095, 4096, 4097] and chunks.tolist() == [0, 1]
    if c.group == "C3":
        assert chunks.size == 1 and chunks[0] == {"C3_chunk_start": 0, "C3_chunk_end": 5, "C3_table_end": (1 << bits) // 4096 - 1}[name]
        p = pos if name == "C3_chunk_start" else 4095 - pos
        assert sorted(p.tolist()) == [3, 4, 15, 16, 1023, 1024]
        assert {0, 3} <= set((pos % 4).tolist()) and {0, 15} <= set((pos % 16).tolist())          # a quad's and a thread's first and last entry
        assert len(set((pos // 1024).tolist())) == 2                                                 # two waves of the write = two quad rows of the count
    if c.group == "C4":
        assert chunks.tolist() == [6, 7, 8] and np.bincount(k >> 12)[6:].tolist() == [1, 4096, 1]
    if c.group == "C5":
        ps = [1, 2, 3] + ([16, 31] if bits == 27 else [])
        assert k.tolist() == sorted(E.PART_KEYS * p + d for p in ps for d in (-1, 0)) and E.PART_KEYS == 1024 * 4096
        assert set(parts.tolist()) == set(ps) | {p - 1 for p in ps}
    if c.group == "C6":
        want = sorted(p % P for p in c.facts["parts"])
        assert parts.tolist() == want and len(want) < P
        assert {0, 4095} <= set(pos.tolist()) and {0, 1023} <= set(((k >> 12) % 1024).tolist())       # a part's first and last chunk
    if c.group == "C7":
        n = (1 << bits) // 4096
        assert k.size == n == {24: 4096, 27: 32768}[bits] and np.array_equal(k >> 12, np.arange(n)) and np.array_equal(pos, 37 * np.arange(n) % 4096)
    if c.group == "C8":
        assert k.size == 1 << 16 and k[-1] - k[0] == k.size - 1 and parts.tolist() == [1, 2] and (np.bincount(k // E.PART_KEYS)[1:] == 1 << 15).all()
    if c.group == "C9":
        assert bits == 24 and c.bits == (24,) and k.size == 1 << 24 and k[-1] == top and (counts == 1).all()
    if c.group == "C10":
        heavy, where = c.facts["heavy"], c.facts["where"]
        i = int(np.argmax(counts))
        assert counts[i] == heavy and (np.delete(counts, i) == 1).all() and k.size == 101 and heavy in (1 << 20, 255, 256, 65535, 65536)
        ch, pt = int(k[i]) >> 12, int(k[i]) // E.PART_KEYS
        assert {"chunk0": ch == 0, "part0_last_chunk": ch == 1023, "part2": pt == 2, "top": k[i] == top}[where]
        assert pos[i] % 4 != 0                          # not a quad's first entry
        assert parts.size == P                          # the light keys reach every part
    _comp_kills(name, bits)


def test_the_compaction_table_reaches_what_it_is_there_for():
    ids = set(E.COMP_IDS)
    for n in ("C1_zero", "C1_top", "C1_zero_and_top", "C2_chunk_edges", "C3_chunk_start", "C3_chunk_end", "C4_full_chunk", "C5_part_edges",
              "C6_only_last_part", "C6_only_first_part", "C6_only_parts_1_and_3", "C7_one_key_per_chunk", "C8_long_run"):
        assert {(n, 24), (n, 27)} <= ids
    assert ("C9_full_table", 24) in ids and ("C9_full_table", 27) not in ids
    assert {("C10_%s_x%d" % (w, h), b) for w in ("chunk0", "part0_last_chunk", "part2", "top") for h in (1 << 20, 255, 256, 65535, 65536) for b in (24, 27)} <= ids
    assert {c.group for c in E.COMP} == set(E.COMP_GROUPS)


# ------------------------------------------------------------------ what the table is worth
def test_every_defect_is_caught_and_by_which_groups():
    caught = {d: set() for d in list(E.FILL_DEFECTS) + list(E.COMPACT_DEFECTS)}
    for c in E.FILL:
        for d in _fill_kills(c.name):
            caught[d].add(c.group)
    for name, bits in E.COMP_IDS:
        for d in _comp_kills(name, bits):
            caught[d].add(E.COMP_BY_NAME[name].group)
    print()
    for d, gs in caught.items():
        print("%-32s %-11s %s" % (d, E.FILL_DEFECTS.get(d) or E.COMPACT_DEFECTS[d], " ".join(sorted(gs, key=lambda g: int(g[1:])))))
    assert all(caught.values()), [d for d, g in caught.items() if not g]
    assert {E.FILL_DEFECTS[d] for d in E.FILL_DEFECTS} == set(E.FILL_STEPS) and {E.COMPACT_DEFECTS[d] for d in E.COMPACT_DEFECTS} == set(E.COMPACT_STEPS)
    assert caught == CAUGHT_BY
    # no partition group is decorative: F9 is on the direct route (its only large case is kept out of the defect runs), every other group
    # catches some defect -- and these are the only ones to catch theirs
    groups = {g for gs in caught.values() for g in gs}
    assert groups == (set(E.FILL_GROUPS) - {"F9"}) | set(E.COMP_GROUPS)
    assert caught["items_round_down"] == {"F4", "F8"} and caught["chunk_offset_16_bits"] == {"C9"}
    # by case: the threshold readings with a tail catch the tail's defects, the one without (npx = N0, N0 + 16) does not
    with_tail = {"F1_npx_N0+1", "F1_npx_N0+15", "F1_npx_N0+17", "F1_npx_N0+31", "F2_block_ownership"}
    assert {n for n in E.FILL_NAMES if "tail_dropped" in _fill_kills(n)} == with_tail
    # a tail counted twice makes npx + tail entries.  The model drops what falls behind the npx entries of the payload, which is the highest bucket's:
    # with a tail of one pixel that is F1's own doubled pixel, and the model's table comes out right (a kernel would write and read past the
    # payload instead); the longer tails show it
    assert {n for n in E.FILL_NAMES if "tail_also_by_block0" in _fill_kills(n)} == with_tail - {"F1_npx_N0+1", "F1_npx_N0+17"}
    assert "gpb_rounds_down" not in _fill_kills("F1_npx_N0+0") and "gpb_rounds_down" in _fill_kills("F1_npx_N0+16")
    # the largest count: from part 0 alone it is wrong wherever the heavy key lies behind part 0
    assert ({n for n, b in E.COMP_IDS if n.startswith("C10_") and "max_from_part0_only" in _comp_kills(n, b)}
            == {c.name for c in E.COMP if c.group == "C10" and c.facts["where"] in ("part2", "top")})
