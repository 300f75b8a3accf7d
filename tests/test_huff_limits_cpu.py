"""The case table of tests/test_huff_limits.py (huff_limits_ref.py), without a GPU: every case's claims -- distinct symbols, highest count,
radix passes, runs, longest code, route -- are computed from its stream alone (np.unique, and a binary heap for the code lengths: not the
oracle, not the library), the constants the table restates are still the library's, and the table stands on both sides of every switch
of the Huffman code stage.  A case that drifts off its switch fails here, not silently on the GPU."""
import functools
import os
import re

import numpy as np
import pytest

import huff_limits_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cniic_amd", "csrc")


@functools.lru_cache(maxsize=None)
def measured(stream):
    """(U, highest count, runs, longest code, ties met, lowest count, symbols) of a stream -- once for all the cases that share it"""
    syms = R.stream(stream)
    keys, counts = R.histogram(syms)
    assert R.valid_keys(R.kind_of(stream), keys), stream
    lens, ties = R.heap_code_lengths(counts)
    return int(keys.size), int(counts.max()), int(np.unique(counts).size), int(lens.max()), int(ties), int(counts.min()), int(syms.size)


def test_the_constants_the_table_restates_are_the_library_s():
    kernel = open(os.path.join(CSRC, "k_huff.hip")).read()
    codec = open(os.path.join(CSRC, "codec.cpp")).read()
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "constexpr int kSortThreads = 256, kSortPer = 16, kSortBlock = kSortThreads * kSortPer;" in kernel and R.SORT_BLOCK == 256 * 16
    assert "blockhist /* [256][nblocks] */" in kernel and R.COUNTERS_PER_BLOCK == 256
    assert "if (n > %d && n <= %d) {" % (R.SCAN_ONE_BLOCK, R.SCAN_SMALL_MAX) in kernel
    assert "for (uint32_t shift = 32; shift < 64 && (max_count >> (shift - 32)) != 0; shift += 8, passes++)" in kernel
    assert "constexpr uint32_t kMaxLeafRuns = 1u << 16;" in kernel and R.MAX_RUNS == 1 << 16
    assert "constexpr uint32_t kRunsMinLeaves = 1u << 16;" in kernel and R.RUNS_MIN_LEAVES == 1 << 16
    assert "if (R == 0 || R > kMaxLeafRuns || (!rm && R > n / 4)) return CNIIC_OK;" in kernel
    assert "if (toolong || longest > %d) return CNIIC_OK;" % R.CODE_SORT_BITS in kernel
    assert kernel.count("len[i] <= %d ?" % R.INLINE_BITS) == 2                      # k_fill_code32, k_fill_code32_hot
    assert kernel.count("std::min<uint32_t>(ceil_div(n, 256u), 2048u)") == 1 and R.STRIDE_FROM == 2048 * 256
    assert kernel.count("std::min<uint64_t>(ceil_div(U, 256), 2048)") == 2          # the grids of k_fill_code32 and k_fill_code32_hot
    assert '{"CNIIC_HUF_GPU_CODES_MIN", %d}' % R.GPU_CODES_MIN in capi
    assert 'c->opt(CNIIC_OPT_HUF_GPU_CODES_MIN, "CNIIC_HUF_GPU_CODES_MIN", %d)' % R.GPU_CODES_MIN in codec
    for mark in ('ktimes["huf_tree_runs"]', 'ktimes["huf_tree_host"]'):
        assert re.search(r"if \(c->timers[^)]*\) c->%s\.launches\+\+;" % re.escape(mark), codec), mark   # nothing with the timers off
    assert 'if (c->timers) c->ktimes["huf_sort_passes"].launches += passes;' in kernel


def test_keys_are_valid_distinct_and_out_of_order():
    i = np.arange(600001)
    for kind in (1, 2):
        k = R.keys_of(kind, i)
        assert R.valid_keys(kind, k) and np.unique(k).size == i.size
        assert not (np.diff(k[:1000].astype(np.int64)) > 0).all()                    # rank order is not insertion order
    assert np.unique(R.keys_of(1, i[:4095]) >> 16).size >= 250                        # kind 1: spread over the 24-bit space
    assert not R.valid_keys(2, [511]) and not R.valid_keys(2, [511 << 9]) and not R.valid_keys(2, [511 << 18]) and not R.valid_keys(1, [1 << 24])
    assert R.valid_keys(2, [510 << 18 | 510 << 9 | 510, 0])


def test_the_heap_on_histograms_whose_lengths_are_known():
    assert R.heap_code_lengths([5, 9])[0].tolist() == [1, 1]
    assert R.heap_code_lengths([1, 1, 1])[0].tolist() == [2, 2, 1]                     # leaves in key order, then a leaf before the branch
    assert R.heap_code_lengths([7] * 1024)[0].tolist() == [10] * 1024
    assert sorted(R.heap_code_lengths(R.fib(20))[0].tolist()) == sorted([19] + list(range(1, 20))[::-1])
    assert R.heap_code_lengths([4, 1, 1, 2])[0].tolist() == [1, 3, 3, 2] and R.heap_code_lengths([4, 1, 1, 2])[1] == 2   # 1 + 1 = the waiting 2, 2 + 2 = the waiting 4
    assert [R.passes_for(c) for c in (1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1)] == [1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_stands_where_it_claims_to(name):
    case = R.BY_NAME[name]
    U, top, runs, longest, _, _, n = measured(case.stream)
    assert (U, top, runs, longest) == (case.U, case.max_count, case.R, case.longest)
    route = R.route_rule(case, U, runs, longest)
    assert route == case.route
    assert case.passes == (0 if route == "small" else R.passes_for(top))
    if U < R.GPU_CODES_MIN and "-rank" not in name:   # (by rank: the default threshold is what sends the codes through the table by rank)
        assert R.C0 in case.knobs
    assert U <= n < 1 << 32


def test_the_two_old_long_code_tests_sent_codes_of_20_bits():
    """tests/test_gpu_parity.py: test_huf_encode_all_long_codes said "> 32 bits" and test_huf_long_codes_on_the_gpu "up to 39 bits" of Fibonacci
    counts capped at 3000 from index 21 on.  Whatever the number of symbols, that histogram's longest code has 20 bits; both now send fib33."""
    keys, counts = R.histogram(R.capped_fibonacci_stream())
    assert keys.size == 40 and counts.sum() == 85656
    assert R.heap_code_lengths(counts)[0].max() == 20
    for n in range(28, 41):
        assert R.heap_code_lengths([min(c, 3000) if i > 20 else c for i, c in enumerate(R.fib(n))])[0].max() == 20, n


def test_fibonacci_streams_have_the_sizes_the_table_is_built_on():
    for L, n in ((26, 514228), (27, 832039), (32, 9227464), (33, 14930351), (34, 24157816)):
        assert sum(R.fib(L + 1)) == R.fib(L + 3)[-1] - 1 == n == measured("fib%d" % L)[6]
    img = R.fib_image()
    assert img.shape == (813, R.FIB_IMAGE_W, 3)
    keys, counts = R.histogram(img.reshape(-1, 3).astype(np.uint32) @ np.array([65536, 256, 1], np.uint32))
    assert keys.size == R.FIB_IMAGE_L + 1 and sorted(counts.tolist())[:-1] == R.fib(R.FIB_IMAGE_L)
    assert R.heap_code_lengths(counts)[0].max() == R.FIB_IMAGE_L


def test_the_34_bit_codes_start_at_bits_31_and_30():
    """a code of L bits that starts at bit b of an output word needs a third word when L + b > 64: 34 bits at b = 31 and nowhere else
    (pack_pieces, device_utils.hpp); at b = 30 the code ends with its second word.  Positions: the serialised decoder, then the running
    sum of the heap's lengths."""
    syms = R.stream("fib34")
    keys, counts = R.histogram(syms)
    assert sorted(counts.tolist()) == sorted(R.fib(35))
    lens = R.heap_code_lengths(counts)[0]
    assert sorted(lens.tolist()) == sorted([34] + list(range(1, 35)))
    per_sym = lens[np.searchsorted(keys, syms)]
    where = np.nonzero(per_sym == 34)[0]
    assert where.size == 2 and counts[np.searchsorted(keys, syms[where])].tolist() == [1, 1]
    start = R.decoder_bits(2, 35) + np.cumsum(per_sym)[where] - 34
    assert (start % 32).tolist() == [31, 30]
    assert [int(34 + b > 64) for b in start % 32] == [1, 0]
    assert where[0] < 16 and 4096 * 1000 < where[1] < syms.size - 4096 * 1000      # the pack's first thread; the middle of the stream
    assert R.decoder_bits(2, 35) == 8 * 279 and R.decoder_bits(1, 28) == 8 * (28 * 12 + 27)


def test_the_table_stands_on_both_sides_of_every_switch():
    cases = R.CASES
    by = lambda pred: [c for c in cases if pred(c)]
    gpu = by(lambda c: c.route != "small")
    # sort blocks: 1 | 1 | 2, all counts equal and skewed, both kinds at 4097 and 131073
    for U in (4095, 4096, 4097, 16384, 16385, 131072, 131073):
        for hist in ("eq", "skew"):
            kinds = {R.kind_of(c.stream) for c in gpu if c.U == U and c.stream.startswith(hist) and c.name.startswith("sort-")}
            assert kinds == ({1, 2} if U in (4097, 131073) else {1}), (U, hist)
    assert [R.sort_blocks(U) for U in (4095, 4096, 4097)] == [1, 1, 2]
    # the counter scan: one local block | small | small | local plus add
    assert [(R.scan_counters(U), R.scan_route(U)) for U in (16384, 16385, 131072, 131073)] == [
        (1024, "local"), (1280, "small"), (8192, "small"), (8448, "local+add")]
    for c in by(lambda c: c.name.startswith("sort-eq")):
        assert (c.max_count, c.R, c.passes) == (3, 1, 1)                             # one digit everywhere: stability alone orders the leaves
    for c in by(lambda c: c.name.startswith("sort-skew")):
        assert measured(c.stream)[5] < 256 <= c.max_count < 65536 and c.passes == 2   # two digits
    # radix passes
    tops = {c.max_count: c.passes for c in by(lambda c: c.name.startswith("passes-"))}
    assert tops == {255: 1, 256: 2, 65535: 2, 65536: 3, (1 << 24) - 1: 3, 1 << 24: 4}
    for c in by(lambda c: c.name.startswith("passes-")):
        counts = R.h_passes(c.max_count)
        assert (counts == 1).sum() == 3000 and np.sort(counts)[-2] == 41              # a few thousand of 1, the rest small
    # the run route's gate, default knobs
    gate = {c.U: c.route for c in cases if not c.knobs and c.route != "small"}
    assert gate[65535] == "host" and gate[65536] == "runs" and gate[131073] == "runs"
    assert all(c.R == 12 for c in by(lambda c: c.name.startswith("gate-")))
    # merge_runs, the run route forced and asserted
    forced = by(lambda c: R.R0 in c.knobs and c.route == "runs")
    assert {c.U for c in forced if c.R == 1} == {4095, 4096, 4097, 131071, 131072, 131073}
    for k in (12, 17):   # 2^k leaves of one count: every code has k bits
        lens = R.heap_code_lengths([3] * (1 << k))[0]
        assert lens.min() == lens.max() == k == R.BY_NAME["runs-one%d" % (1 << k)].longest
    assert all(n % 2 == 1 for n in R.ODD_RUNS) and len(R.ODD_RUNS) == 60 and 1 in R.ODD_RUNS and R.BY_NAME["runs-odd"] in forced
    assert R.BY_NAME["runs-singles"] in forced and R.BY_NAME["runs-singles"].R == R.BY_NAME["runs-singles"].U == 2000
    assert measured("singles")[6] == 2001000
    assert R.BY_NAME["runs-pow2ties"] in forced and measured("pow2ties")[4] >= 8      # branches as heavy as leaves that still wait
    assert {n % 2 for n in R.POW2_RUNS} == {0, 1}
    assert R.BY_NAME["runs-two"] in forced and R.BY_NAME["runs-two"].U == 2
    # grid stride: the largest grid exactly | one leaf more | a partial last block; both tree routes
    stride = {(c.U, c.route) for c in by(lambda c: c.name.startswith("stride"))}
    assert stride == {(U, r) for U in (R.STRIDE_FROM, R.STRIDE_FROM + 1, 600001) for r in ("runs", "host")} and 600001 % 256
    for c in by(lambda c: c.name.startswith("stride")):
        assert R.kind_of(c.stream) == 1 and 24 <= c.R <= 48 and c.U + 250000 < measured(c.stream)[6] < c.U + 350000
    # code lengths: 26 | 27 on both pack routes, 32 | 33 on the run route, 27 and 33 and 34 straight to memory
    for L in (26, 27):
        assert R.BY_NAME["fib%d-rank" % L].route == "small" and R.BY_NAME["fib%d-direct" % L].route == "host"
        assert R.BY_NAME["fib%d-rank" % L].longest == R.BY_NAME["fib%d-direct" % L].longest == L
    assert R.INLINE_BITS == 26 and R.CODE_SORT_BITS == 32
    assert (R.BY_NAME["fib32-runs"].route, R.BY_NAME["fib33-runs"].route) == ("runs", "host")
    assert R.R0 in R.BY_NAME["fib32-runs"].knobs and R.R0 in R.BY_NAME["fib33-runs"].knobs
    for L in (27, 33, 34):
        for how in ("rank", "direct"):
            assert R.IMG24 in R.BY_NAME["fib%d-%s-img24" % (L, how)].knobs
    # the cases of one stream stand together (the large streams are built once)
    seen = []
    for c in cases:
        if not seen or seen[-1] != c.stream:
            seen.append(c.stream)
    assert all(seen.count(s) == 1 for s in seen if s.startswith(("fib", "top", "stride", "singles", "skew", "gate")))
