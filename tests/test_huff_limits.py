"""The large-alphabet Huffman code stage (HuffCodeStage in cniic_amd/csrc/codec.cpp, the second half of k_huff.hip) where it switches routes:
symbol streams with a prescribed histogram (huff_limits_ref.py) on both sides of a sort block (4096 leaves), of the three ways the sort's
digit counters are scanned (1024 and 8192 counters), of every number of radix passes (highest count 2^8, 2^16, 2^24), of the run route's
gate (2^16 leaves) and of its retreat (codes of 32 | 33 bits), through merge_runs with runs of one count, of odd length, of length 1 and
with branches as heavy as waiting leaves, across the grid-stride kernels' largest grid (524288 leaves), and with longest codes of exactly
26 | 27 bits (the inline word's escape, on both pack routes), 32 | 33 and 34 bits (a code in three output words).
tests/test_huff_limits_cpu.py asserts that every case stands where it claims to.  Every stream is the oracle's, byte for byte, and the
ROUTE is asserted too: all routes give the same bytes by design, so only the stage's marks -- huf_tree_runs, huf_tree_host,
huf_sort_passes, recorded with the stage timers on -- can tell a call that went the wrong way."""
import numpy as np
import pytest

import huff_limits_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

MARKS = {"runs": (1, 0), "host": (0, 1), "small": (0, 0)}   # route: launches of (huf_tree_runs, huf_tree_host)


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


def marks(ctx):
    return tuple(ctx.kernel_time(k)[1] for k in ("huf_tree_runs", "huf_tree_host", "huf_sort_passes"))


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_equals_oracle_and_takes_its_route(ctx, monkeypatch, name):
    """a plain call gives the oracle's bytes (computed once per stream); the same call with the stage timers on (the marks are cleared at the
    start of every call) gives the same bytes and went the way the case claims"""
    from cniic_amd import _lib
    case = R.BY_NAME[name]
    syms, kind, want = R.stream(case.stream), R.kind_of(case.stream), R.expected(case.stream)
    for k, v in case.knobs:
        monkeypatch.setenv(k, v)
    assert ctx.huf_encode_all(kind, syms) == want
    assert marks(ctx) == (0, 0, 0)   # (nothing is recorded with the timers off)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        timed = ctx.huf_encode_all(kind, syms)
        got = marks(ctx)
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert timed == want
    assert got == MARKS[case.route] + (case.passes,), (case.route, case.passes, got)


def test_hufman_image_with_a_27_bit_code(ctx, monkeypatch):
    """28 colours with Fibonacci counts through the codec: with the (length, code) words in the dense table the pack's first pass reads
    PIXELS (the RGB source of k_pack_count32) and the 27-bit codes escape; the stream is the oracle's and decodes back"""
    from cniic_amd import _lib
    img = R.fib_image()
    rc, want, _ = O.encode("hufman", img)
    assert rc == 0
    monkeypatch.setenv(*R.C0)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, data, _ = ctx.encode("hufman", img)
        got = marks(ctx)
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert rc == 0 and data == want
    assert got == (0, 1, 3), got
    rc, back = ctx.decode("hufman", data)
    assert rc == 0 and np.array_equal(back, img)
