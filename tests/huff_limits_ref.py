"""Symbol streams with a PRESCRIBED histogram for the large-alphabet Huffman code stage (HuffCodeStage in cniic_amd/csrc/codec.cpp and the
second half of k_huff.hip), for tests that must KNOW which route a call takes before they run it (tests/test_huff_limits.py on the GPU,
tests/test_huff_limits_cpu.py for the table itself).  All routes give the same bytes by design, so a case is worth something only when
it stands on a switch and the route is asserted.  The switches:

  4096 leaves            a block of the stable LSD radix sort by (count, key): U = 4095 | 4096 | 4097
  1024, 8192 counters    256 digit counters per sort block are scanned by one k_pack_scan_local block (<= 1024), by k_pack_scan_small
                         (<= 8192) or by local plus add: U = 16384 | 16385 and 131072 | 131073
  2^8, 2^16, 2^24        the highest count decides the number of 8-bit passes: 255 | 256, 65535 | 65536, 2^24 - 1 | 2^24
  2^16 leaves            from here on the tree is built from runs of equally frequent leaves (when the runs are few): U = 65535 | 65536
  32 bits                the run route's sort by code keys on 32 bits and gives way to the host's merge above: longest code 32 | 33
  26 bits                the (length, code) word holds codes of up to 26 bits, longer ones escape to the per-rank tables: 26 | 27
  34 bits at bit 31      a 34-bit code that starts at bit 31 of an output word is the only one that needs pack_pieces' third piece
  2048 blocks of 256     k_leaf_run_count, k_leaf_run_list, k_tree_leaf_walk and k_fill_code32 stride from 524289 leaves on

A case is a stream (a name in STREAMS), the knobs it runs under, and what it CLAIMS: distinct symbols U, the highest count, radix passes,
runs R of equal count, the longest code and the route of the tree ("small": the host's tree and codes, no mark; "host": the host's merge
and huff_tree_codes; "runs": huff_tree_from_runs).  Sort blocks and scan counters follow from U (sort_blocks, scan_counters, scan_route).
The CPU test asserts every claim from the stream alone, with heap_code_lengths -- a plain binary heap -- for the code lengths.

Keys: symbol number i of a stream is keys_of(kind, i): kind 1 a multiplicative hash over the 24-bit space, kind 2 a valid SignedColor key
(three 9-bit fields 0 .. 510) from a multiplicative walk over 511^3 -- so the compaction's rank order is not the order the counts were
written down in.

Out of reach at a size a test may have, and not faked here: more than 2^16 runs (1 + 2 + ... + 65537 is over 2.1 G symbols); "the runs
exceed a quarter of the leaves" from 2^16 leaves on (16385 runs over 65536 leaves: at least 134 M symbols); codes beyond 64 bits (Fibonacci
counts, the deepest tree there is, need F(67) > 2^32 symbols)."""
import bisect
import functools
import heapq
from collections import namedtuple

import numpy as np

SORT_BLOCK, COUNTERS_PER_BLOCK = 4096, 256          # kSortBlock; the [256][nblocks] digit counters of a pass
SCAN_ONE_BLOCK, SCAN_SMALL_MAX = 1024, 8192         # pack_scan_counts
GPU_CODES_MIN, RUNS_MIN_LEAVES, MAX_RUNS = 32768, 1 << 16, 1 << 16
CODE_SORT_BITS, INLINE_BITS = 32, 26
STRIDE_FROM = 2048 * 256                            # the grid-stride kernels' largest grid

C0 = ("CNIIC_HUF_GPU_CODES_MIN", "0")               # GPU codes for alphabets below 32768 symbols too; the dense table holds the words
R0 = ("CNIIC_HUF_RUNS_MIN", "0")                    # the run route for any number of leaves and runs
NORUNS = ("CNIIC_HUF_RUNS_MIN", "1000000")          # ... for none of these
IMG24 = ("CNIIC_TEST_PACK_IMG_WORDS", "24")         # every chunk of the pack goes straight to memory


# ------------------------------------------------------------------ keys
_P2, _N2 = 1000003, 511 ** 3                        # 1000003 = 4 mod 7 = 49 mod 73: coprime to 511, so i -> i P mod 511^3 is one to one


def keys_of(kind, i):
    i = np.asarray(i, np.uint64)
    if kind == 1:
        return ((i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFF)).astype(np.uint32)
    j = (i * np.uint64(_P2) + np.uint64(7)) % np.uint64(_N2)
    return ((j // np.uint64(511 * 511)) << np.uint64(18) | ((j // np.uint64(511)) % np.uint64(511)) << np.uint64(9) | j % np.uint64(511)).astype(np.uint32)


def valid_keys(kind, keys):
    keys = np.asarray(keys, np.uint32)
    if kind == 1:
        return bool((keys < (1 << 24)).all())
    return bool(((keys >> 27) == 0).all() and ((keys >> 18) <= 510).all() and (((keys >> 9) & 511) <= 510).all() and ((keys & 511) <= 510).all())


# ------------------------------------------------------------------ the yardstick: a binary heap
def heap_code_lengths(counts):
    """counts of the symbols in ascending key order -> (code length of each, number of branches made while a leaf of the same weight was
    still waiting).  The textbook construction (src/huf.rs:58-117) on Python's heapq; among equal weights a leaf goes before a branch, leaves in
    key order, branches in the order they were made -- written as the heap's sort key, (weight, is a branch, number)."""
    counts = [int(c) for c in counts]
    U = len(counts)
    if U == 1:
        return np.zeros(1, np.int64), 0
    waiting = sorted(counts)
    h = [(c, 0, r) for r, c in enumerate(counts)]
    heapq.heapify(h)
    parent = [0] * (2 * U - 1)
    leaves_gone = ties = 0
    for b in range(U - 1):
        x, y = heapq.heappop(h), heapq.heappop(h)
        for z in (x, y):
            parent[z[2] + U * z[1]] = U + b
            leaves_gone += 1 - z[1]
        w = x[0] + y[0]
        k = bisect.bisect_left(waiting, w, leaves_gone)
        ties += k < U and waiting[k] == w
        heapq.heappush(h, (w, 1, b))
    depth = [0] * (2 * U - 1)
    for node in range(2 * U - 3, -1, -1):   # (a parent is made after its children: its number is the larger one)
        depth[node] = depth[parent[node]] + 1
    return np.array(depth[:U], np.int64), ties


def histogram(syms):
    """(keys ascending, counts) of a stream, by sorting"""
    return np.unique(np.asarray(syms), return_counts=True)


def passes_for(max_count):
    p = 0
    while p < 4 and (max_count >> (8 * p)) != 0:
        p += 1
    return p


def sort_blocks(U):
    return -(-U // SORT_BLOCK)


def scan_counters(U):
    return COUNTERS_PER_BLOCK * sort_blocks(U)


def scan_route(U):
    n = scan_counters(U)
    return "local" if n <= SCAN_ONE_BLOCK else "small" if n <= SCAN_SMALL_MAX else "local+add"


def knob(case, name, default):
    return int(dict(case.knobs).get(name, default))


def route_rule(case, U, R, longest):
    """the route as HuffCodeStage::begin and huff_tree_from_runs decide it, restated"""
    if U < 2 or U < knob(case, C0[0], GPU_CODES_MIN):
        return "small"
    forced = R0[0] in dict(case.knobs)
    if U < knob(case, R0[0], RUNS_MIN_LEAVES) or R > MAX_RUNS or (not forced and R > U // 4) or longest > CODE_SORT_BITS:
        return "host"
    return "runs"


def decoder_bits(kind, U):
    return 8 * (U * (1 + (11 if kind == 1 else 6)) + U - 1)   # U leaf records of a tag and the symbol, U - 1 branch tags


# ------------------------------------------------------------------ histograms (counts of symbol number 0, 1, ...)
def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def h_equal(U, c=3):
    return np.full(U, c, np.int64)


def h_skewed(U):
    """1 .. 5 for most, 256 .. 855 for every 61st: two digits, ties in both"""
    i = np.arange(U, dtype=np.uint64)
    h = ((i * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xFFFF)
    return np.where(i % np.uint64(61) == 0, 256 + h % np.uint64(600), 1 + h % np.uint64(5)).astype(np.int64)


def h_passes(top):
    """the heaviest leaf, 40 leaves of 2 .. 41 and 3000 of 1: drop the pass that holds the top digit and the heaviest leaf sorts to the front"""
    return np.array([top] + list(range(2, 42)) + [1] * 3000, np.int64)


def h_gate(U):
    return 1 + np.arange(U, dtype=np.int64) % 12


ODD_RUNS = [2 * ((j * 37) % 50) + 1 for j in range(60)]    # run j: ODD_RUNS[j] leaves of count j + 1
POW2_RUNS = [6, 3, 2, 5, 4, 1, 7, 2, 3, 8, 1, 5]          # run j: leaves of count 2^j -- the branches of runs 0, 1, ... weigh what run j + 1's leaves do


def h_runs(lengths, count_of):
    return np.concatenate([np.full(n, count_of(j), np.int64) for j, n in enumerate(lengths)])


def h_stride(U):
    i = np.arange(U, dtype=np.int64)
    return np.where(i < 16000, 2 + i % 36, 1)


def from_counts(kind, counts, seed):
    """the stream: symbol i counts[i] times, shuffled"""
    counts = np.asarray(counts, np.int64)
    syms = np.repeat(keys_of(kind, np.arange(counts.size)), counts)
    np.random.default_rng(seed).shuffle(syms)
    return syms


def fib34_stream():
    """F(1) .. F(35) of kind 2: the two symbols that occur once have the two 34-bit codes.  One is put where it starts at bit 31 of an output
    word, the other in the middle of the stream at bit 30, by moving some of the most frequent symbol (a 1-bit code) in front of them."""
    kind, L = 2, 34
    counts = np.array(fib(L + 1), np.int64)
    keys = keys_of(kind, np.arange(L + 1))
    order = np.argsort(keys)
    lens = np.empty(L + 1, np.int64)
    lens[order] = heap_code_lengths(counts[order])[0]
    assert lens[0] == lens[1] == L and lens[L] == 1
    base = decoder_bits(kind, L + 1)
    a = (31 - base) % 32
    spare = a + 31
    rest = counts.copy()
    rest[0] -= 1
    rest[1] -= 1
    rest[L] -= spare
    body = np.repeat(keys, rest)
    np.random.default_rng(34).shuffle(body)
    half = body.size // 2
    bits_first = int(lens[order][np.searchsorted(keys[order], body[:half])].sum())
    p = (30 - (base + a + L + bits_first)) % 32
    top = keys[L]
    return np.concatenate([np.full(a, top), keys[:1], body[:half], np.full(p, top), keys[1:2], body[half:], np.full(spare - a - p, top)]).astype(np.uint32)


def capped_fibonacci_stream():
    """what test_huf_encode_all_long_codes and test_huf_long_codes_on_the_gpu used to send: Fibonacci counts capped at 3000 from index 21 on.
    Its longest code is 20 bits, not "up to 39"."""
    f = [min(c, 3000) if i > 20 else c for i, c in enumerate(fib(40))]
    syms = np.concatenate([np.full(c, i * 7 + 1, np.uint32) for i, c in enumerate(f)])
    np.random.default_rng(0).shuffle(syms)
    return syms


FIB_IMAGE_L, FIB_IMAGE_W = 27, 1024


@functools.lru_cache(maxsize=1)
def fib_image():
    """a `hufman` image of 28 colours with Fibonacci counts, what is left of the last row on the largest: a longest code of exactly 27 bits"""
    c = fib(FIB_IMAGE_L + 1)
    h = -(-sum(c) // FIB_IMAGE_W)
    c[-1] += FIB_IMAGE_W * h - sum(c)
    keys = from_counts(1, c, 27)
    img = np.ascontiguousarray(np.stack([keys >> 16, keys >> 8, keys], 1).reshape(h, FIB_IMAGE_W, 3) & 255, np.uint8)
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------ streams and cases
STREAMS = {}   # name -> (kind, builder)
Case = namedtuple("Case", "name stream knobs U max_count passes R longest route")
CASES = []


def _stream(name, kind, builder):
    assert name not in STREAMS
    STREAMS[name] = (kind, builder)


def _add(name, stream, knobs, U, max_count, passes, R, longest, route):
    assert stream in STREAMS
    CASES.append(Case(name, stream, tuple(knobs), U, max_count, passes, R, longest, route))


def _codes(U):
    return (C0,) if U < GPU_CODES_MIN else ()


def _log2_up(U):
    return (U - 1).bit_length()


# the longest code, the runs and the highest count of the skewed histograms, as measured with the heap (test_huff_limits_cpu.py holds them to it)
SKEWED = {4095: (851, 73, 16), 4096: (851, 73, 16), 4097: (851, 73, 16), 16384: (855, 255, 18), 16385: (855, 255, 18),
          131072: (855, 581, 21), 131073: (855, 581, 21)}   # U: (highest count, runs, longest code)
PASSES_LONGEST = {255: 12, 256: 12, 65535: 13, 65536: 13, (1 << 24) - 1: 13, 1 << 24: 13}
STRIDE_LONGEST = {524288: 20, 524289: 20, 600001: 20}
GATE_LONGEST = {65535: 19, 65536: 19}
ODD_LONGEST, SINGLES_LONGEST, POW2_LONGEST = 16, 20, 14


def _build_cases():
    # --- sort blocks and the counter scan: all counts equal (the order is stability's alone) and skewed (two digits)
    for U in (4095, 4096, 4097, 16384, 16385, 131071, 131072, 131073):
        for kind in (1, 2) if U in (4097, 131073) else (1,):
            _stream("eq%d-k%d" % (U, kind), kind, lambda U=U, kind=kind: from_counts(kind, h_equal(U), U + kind))
            if U == 131071:
                continue   # (only the single run below)
            _stream("skew%d-k%d" % (U, kind), kind, lambda U=U, kind=kind: from_counts(kind, h_skewed(U), U + kind + 2))
            tree = "runs" if U >= RUNS_MIN_LEAVES else "host"
            _add("sort-eq%d-k%d" % (U, kind), "eq%d-k%d" % (U, kind), _codes(U), U, 3, 1, 1, _log2_up(U), tree)
            mx, R, longest = SKEWED[U]
            _add("sort-skew%d-k%d" % (U, kind), "skew%d-k%d" % (U, kind), _codes(U), U, mx, 2, R, longest, tree)
    # --- radix passes
    for top, p in ((255, 1), (256, 2), (65535, 2), (65536, 3), ((1 << 24) - 1, 3), (1 << 24, 4)):
        _stream("top%d" % top, 1, lambda top=top: from_counts(1, h_passes(top), top % 1000))
        _add("passes-top%d" % top, "top%d" % top, (C0,), 3041, top, p, 42, PASSES_LONGEST[top], "host")
    # --- the run route's gate under the default knobs (131073 leaves: sort-eq131073, sort-skew131073)
    for U, tree in ((65535, "host"), (65536, "runs")):
        _stream("gate%d" % U, 1, lambda U=U: from_counts(1, h_gate(U), U))
        _add("gate-%d" % U, "gate%d" % U, (), U, 12, 1, 12, GATE_LONGEST[U], tree)
    # --- merge_runs
    for U in (4095, 4096, 4097, 131071, 131072, 131073):   # one run of 2^k - 1 | 2^k | 2^k + 1: 2^k all codes of k bits, 2^k + 1 the carry survives every level
        _add("runs-one%d" % U, "eq%d-k1" % U, _codes(U) + (R0,), U, 3, 1, 1, _log2_up(U), "runs")
    _stream("oddruns", 1, lambda: from_counts(1, h_runs(ODD_RUNS, lambda j: j + 1), 1))
    _stream("singles", 2, lambda: from_counts(2, np.arange(1, 2001), 2))
    _stream("pow2ties", 1, lambda: from_counts(1, h_runs(POW2_RUNS, lambda j: 1 << j), 3))
    _stream("two", 2, lambda: from_counts(2, [3, 5], 4))
    _add("runs-odd", "oddruns", (C0, R0), sum(ODD_RUNS), 60, 1, 60, ODD_LONGEST, "runs")
    _add("runs-singles", "singles", (C0, R0), 2000, 2000, 2, 2000, SINGLES_LONGEST, "runs")
    _add("runs-pow2ties", "pow2ties", (C0, R0), sum(POW2_RUNS), 2048, 2, 12, POW2_LONGEST, "runs")
    _add("runs-two", "two", (C0, R0), 2, 5, 1, 2, 1, "runs")
    # --- grid stride: 2048 blocks of 256 | one leaf more | a partial last block, on both tree routes
    for U in (524288, 524289, 600001):
        _stream("stride%d" % U, 1, lambda U=U: from_counts(1, h_stride(U), U))
        _add("stride%d-runs" % U, "stride%d" % U, (), U, 37, 1, 37, STRIDE_LONGEST[U], "runs")
        _add("stride%d-host" % U, "stride%d" % U, (NORUNS,), U, 37, 1, 37, STRIDE_LONGEST[U], "host")
    # --- code lengths: Fibonacci counts F(1) .. F(L + 1), a longest code of exactly L bits, F(L + 3) - 1 symbols
    for L, kind in ((26, 1), (27, 2), (32, 1), (33, 2)):
        _stream("fib%d" % L, kind, lambda L=L, kind=kind: from_counts(kind, fib(L + 1), L))
    _stream("fib34", 2, fib34_stream)
    for L in (26, 27, 32, 33, 34):
        s, top = "fib%d" % L, fib(L + 1)[-1]
        assert passes_for(top) == 3
        _add("fib%d-rank" % L, s, (), L + 1, top, 0, L, L, "small")          # default threshold: the rank stream and the code table by rank
        _add("fib%d-direct" % L, s, (C0,), L + 1, top, 3, L, L, "host")      # the dense table holds the (length, code) words
        if L in (32, 33):   # the sort by code keys on all 32 bits | the run route gives way
            _add("fib%d-runs" % L, s, (C0, R0), L + 1, top, 3, L, L, "runs" if L == 32 else "host")
        if L in (27, 33, 34):   # the escaped codes straight to memory
            _add("fib%d-rank-img24" % L, s, (IMG24,), L + 1, top, 0, L, L, "small")
            _add("fib%d-direct-img24" % L, s, (C0, IMG24), L + 1, top, 3, L, L, "host")


_build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=3)
def stream(name):
    """(the large ones are 100 MB: only the last few are kept, and the cases of one stream stand together in CASES)"""
    syms = np.ascontiguousarray(STREAMS[name][1](), np.uint32)
    syms.setflags(write=False)
    return syms


def kind_of(name):
    return STREAMS[name][0]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's bytes for a stream, computed once for every test of the session that asks"""
    import oracle_lib as O
    return O.huf_encode_all(O.SYM_RGB if kind_of(name) == 1 else O.SYM_SIGNED, stream(name))
