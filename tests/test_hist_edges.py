"""The histogram (cniic_amd/csrc/k_hist.hip) at its route and scan limits: the three fill routes -- 16-pixel groups with block 0's tail, single
pixels from an unaligned base, the partition from 2^20 pixels on -- and the three-phase compaction, on images and symbol streams whose keys
and counts are placed ON the granularities (tests/hist_edges.py).  Everything is compared for equality with np.unique -- keys (u32), counts
(u64), n_unique -- and, on the cases of at most 2^16 elements, with the oracle's count_freqs as well; there is no tolerance anywhere.
tests/test_hist_edges_cpu.py asserts beforehand that each case stands where it claims to and that the table tells a model of these kernels
with a mistake at any one handover from the right histogram.

Every fill case runs from host memory (the library's own, aligned, upload) and from device views at the byte offsets 1, 4, 8, 15 (the
byte route) and 16 (the aligned one again).  F9's last case (2^23 + 5 pixels) is past the 2048-block grid cap of k_hist_rgb; an aligned base
goes to the partition from 2^20 pixels on, so that kernel's grid-stride loop makes one trip at every size it is launched for.  At this
size the case wraps the byte route's loop (eight times) and runs the partition at eight times its threshold."""
import ctypes as C
import functools

import numpy as np
import pytest

import hist_edges as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

SENT8 = 0xA5
SENT32, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    with Context(0) as c:
        yield c


# ------------------------------------------------------------------ what is expected, computed once
@functools.lru_cache(maxsize=3)
def expected_fill(name):
    """(the pixels, np.unique's keys and counts)"""
    lin = E.fill_pixels(name)
    k = E.keys_of(lin)
    keys, counts = E.witness(k)
    if k.size <= 1 << 16:
        ok, oc = O.count_freqs(k)
        assert np.array_equal(ok, keys) and np.array_equal(oc, counts), name
    return lin, keys, counts


@functools.lru_cache(maxsize=3)
def expected_comp(name, bits):
    """(the stream, the keys and counts): the case's own pairs, which np.unique of the stream returns"""
    stream = E.comp_stream(name, bits)
    keys, counts = E.comp_pairs(name, bits)
    if name == "C9_full_table":   # np.unique of arange(2^24) is itself: a second of sorting that checks nothing of the library
        assert np.array_equal(stream, keys) and (counts == 1).all()
    else:
        wk, wc = E.witness(stream)
        assert np.array_equal(wk, keys) and np.array_equal(wc, counts), (name, bits)
    if stream.size <= 1 << 16:
        ok, oc = O.count_freqs(stream)
        assert np.array_equal(ok, keys) and np.array_equal(oc, counts), (name, bits)
    return stream, keys, counts


def _same(got, keys, counts, what):
    gk, gc = got
    assert gk.dtype == np.uint32 and gc.dtype == np.uint64
    assert gk.size == keys.size, (what, "n_unique", gk.size, keys.size)
    bad = np.flatnonzero((gk != keys) | (gc != counts))
    assert bad.size == 0, (what, "first difference at rank %d: got key %#x count %d, expected key %#x count %d (bucket %d, chunk %d, part %d)" % (
        bad[0], gk[bad[0]], gc[bad[0]], keys[bad[0]], counts[bad[0]], keys[bad[0]] >> 12, keys[bad[0]] >> 12, keys[bad[0]] >> 22))


def placements(lin):
    """("host", the pixels), then ("+off", a device view `off` bytes behind a 16-byte boundary) for every offset"""
    import torch
    yield "host", lin
    src = torch.from_numpy(np.array(lin).reshape(-1)).cuda()      # (a copy: the case's pixels are read-only)
    for off in E.OFFSETS:
        buf = torch.zeros(32 + src.numel(), dtype=torch.uint8, device="cuda")
        view = buf[off:off + src.numel()]
        view.copy_(src)
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off % 16
        assert E.route(view.data_ptr(), lin.shape[0]) == ("bytes" if off % 16 else E.route(0, lin.shape[0]))
        yield "+%d" % off, view


# ------------------------------------------------------------------ fill
@pytest.mark.parametrize("name", E.FILL_NAMES)
def test_fill_case(ctx, name):
    lin, keys, counts = expected_fill(name)
    for where, rgb in placements(lin):
        _same(ctx.hist_rgb24(rgb, lin.shape[0]), keys, counts, (name, where))


@functools.lru_cache(maxsize=2)
def _expected_dense(name):
    _, keys, counts = expected_fill(name)
    table = np.zeros(1 << 24, np.uint32)
    table[keys] = counts
    assert np.array_equal(table, np.bincount(E.keys_of(E.fill_pixels(name)), minlength=1 << 24))
    occ = np.zeros(1 << 21, np.uint32)
    np.add.at(occ, keys >> 3, np.uint32(1) << (4 * (keys & 7)).astype(np.uint32))      # key k in bits 4 (k & 7) of word k >> 3 (the keys are distinct)
    return table, occ


@pytest.mark.parametrize("name", E.FILL_NAMES)
def test_fill_case_into_a_dense_table_and_its_occupancy(ctx, name):
    import torch
    from cniic_amd._lib import _ptr
    lin, _, _ = expected_fill(name)
    want_table, want_occ = _expected_dense(name)
    for where, rgb in placements(lin):
        table = torch.full((4 << 24,), SENT8, dtype=torch.uint8, device="cuda")
        occ = torch.full((4 << 21,), SENT8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx._check(ctx._L.cniic_hist_rgb24_dense(ctx.h, _ptr(rgb), lin.shape[0], table.data_ptr()))
        ctx._check(ctx._L.cniic_occupancy_pack(ctx.h, table.data_ptr(), occ.data_ptr()))
        ctx.sync()
        got = table.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(got != want_table)
        assert bad.size == 0, (name, where, "bin %#x: got %d, expected %d; %d bins differ" % (bad[0], got[bad[0]], want_table[bad[0]], bad.size))
        got = occ.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(got != want_occ)
        assert bad.size == 0, (name, where, "occupancy word %#x: got %#x, expected %#x" % (bad[0], got[bad[0]], want_occ[bad[0]]))


# ------------------------------------------------------------------ compaction
@pytest.mark.parametrize("name,bits", E.COMP_IDS)
def test_compaction_case(ctx, name, bits):
    stream, keys, counts = expected_comp(name, bits)
    _same(ctx.hist_syms(E.KIND_OF_BITS[bits], stream), keys, counts, (name, bits))


# ------------------------------------------------------------------ the raw call
def _call(ctx, which, data, n, keys, counts, cap, allow=()):
    """cniic_hist_rgb24 (which = 0) or cniic_hist_syms of kind `which` -> (rc, n_unique)"""
    from cniic_amd._lib import _ptr
    nu = C.c_uint64(0xdeadbeef)
    if which == 0:
        rc = ctx._L.cniic_hist_rgb24(ctx.h, _ptr(data), n, _ptr(keys), _ptr(counts), cap, C.byref(nu))
    else:
        rc = ctx._L.cniic_hist_syms(ctx.h, which, _ptr(data), n, _ptr(keys), _ptr(counts), cap, C.byref(nu))
    return ctx._check(rc, allow), nu.value


def _raw_inputs():
    """(what, which, data, n, keys, counts): an image on the partition, one on the direct route with a tail, a stream at either kind"""
    for name in ("F2_block_ownership", "F9_npx_4111"):
        lin, keys, counts = expected_fill(name)
        yield name, 0, lin, lin.shape[0], keys, counts
    for name, bits in (("C5_part_edges", 24), ("C5_part_edges", 27), ("C4_full_chunk", 27)):
        stream, keys, counts = expected_comp(name, bits)
        yield (name, bits), E.KIND_OF_BITS[bits], stream, stream.size, keys, counts


def test_raw_call_count_only_capacity_and_sentinels(ctx):
    from cniic_amd import _lib
    for what, which, data, n, keys, counts in _raw_inputs():
        nu = keys.size
        assert _call(ctx, which, data, n, None, None, 0) == (0, nu), what                   # keys = counts = NULL: n_unique alone
        k = np.full(nu + GUARD, SENT32, np.uint32)
        c = np.full(nu + GUARD, SENT64, np.uint64)
        rc, got = _call(ctx, which, data, n, k, c, nu - 1, allow=(_lib.CAPACITY,))         # one short
        assert rc == _lib.CAPACITY and got == nu, what
        assert (k == SENT32).all() and (c == SENT64).all(), (what, "written despite the capacity")
        assert _call(ctx, which, data, n, k, c, nu) == (0, nu), what                        # exactly enough
        _same((k[:nu], c[:nu]), keys, counts, what)
        assert (k[nu:] == SENT32).all() and (c[nu:] == SENT64).all(), (what, "a write behind n_unique entries")
        # one of the two alone
        k[:] = SENT32
        assert _call(ctx, which, data, n, k, None, nu) == (0, nu) and np.array_equal(k[:nu], keys) and (k[nu:] == SENT32).all(), what
        c[:] = SENT64
        assert _call(ctx, which, data, n, None, c, nu) == (0, nu) and np.array_equal(c[:nu], counts) and (c[nu:] == SENT64).all(), what


def test_raw_call_device_outputs_equal_host_outputs(ctx):
    import torch
    from cniic_amd import _lib
    for what, which, data, n, keys, counts in _raw_inputs():
        nu = keys.size
        hk, hc = np.zeros(nu, np.uint32), np.zeros(nu, np.uint64)
        assert _call(ctx, which, data, n, hk, hc, nu) == (0, nu)
        dk = torch.full((4 * (nu + GUARD),), SENT8, dtype=torch.uint8, device="cuda")
        dc = torch.full((8 * (nu + GUARD),), SENT8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, got = _call(ctx, which, data, n, dk, dc, nu - 1, allow=(_lib.CAPACITY,))
        assert rc == _lib.CAPACITY and got == nu and (dk.cpu().numpy() == SENT8).all() and (dc.cpu().numpy() == SENT8).all(), what
        assert _call(ctx, which, data, n, dk, dc, nu) == (0, nu), what
        gk, gc = dk.cpu().numpy().view(np.uint32), dc.cpu().numpy().view(np.uint64)
        assert np.array_equal(gk[:nu], hk) and np.array_equal(gc[:nu], hc), what
        _same((gk[:nu], gc[:nu]), keys, counts, what)
        assert (gk[nu:] == SENT32).all() and (gc[nu:] == SENT64).all(), (what, "a write behind n_unique entries")


def test_raw_call_nothing_gives_nothing(ctx):
    k = np.full(GUARD, SENT32, np.uint32)
    c = np.full(GUARD, SENT64, np.uint64)
    some = np.zeros(48, np.uint8)
    for which, data in ((0, None), (0, some), (1, None), (2, None), (2, some.view(np.uint32))):
        assert _call(ctx, which, data, 0, None, None, 0) == (0, 0), (which, data is None)
        assert _call(ctx, which, data, 0, k, c, GUARD) == (0, 0), (which, data is None)
        assert _call(ctx, which, data, 0, k, c, 0) == (0, 0), (which, data is None)
        assert (k == SENT32).all() and (c == SENT64).all()
    keys, counts = ctx.hist_rgb24(np.zeros((0, 3), np.uint8), 0)
    assert keys.size == 0 and counts.size == 0
    keys, counts = ctx.hist_syms(2, np.zeros(0, np.uint32))
    assert keys.size == 0 and counts.size == 0


# ------------------------------------------------------------------ ranks and the largest count: what the Huffman stage reads
HUF_CASES = [(n, b) for n, b in E.COMP_IDS if n in ("C2_chunk_edges", "C5_part_edges") or n.startswith("C10_")] + [("C7_one_key_per_chunk", 24)]


def passes_of(largest):
    """radix passes of 8 bits that the leaf sort needs for counts up to `largest` (huff_sort_leaves_dev)"""
    return -(-int(largest).bit_length() // 8)


assert [passes_of(h) for h in (255, 256, 65535, 65536, 1 << 20)] == [1, 2, 2, 3, 3]


def gpu_codes_route(ctx, call):
    """call() with the code stage's large-alphabet route forced (OPT_HUF_GPU_CODES_MIN = 0: by default it starts at 32768 distinct symbols,
    more than any case here has) and the stage timers on -> (what call() returned, the leaf sort's radix passes).  That route is the one
    reader of the largest count the compaction collects (plan->max_count -> huff_sort_leaves_dev): with the host's route it is never read"""
    from cniic_amd import _lib
    ctx.set_opt(_lib.OPT_HUF_GPU_CODES_MIN, 0)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        got = call()
        runs, host, passes = (ctx.kernel_time(k)[1] for k in ("huf_tree_runs", "huf_tree_host", "huf_sort_passes"))
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        ctx.set_opt(_lib.OPT_HUF_GPU_CODES_MIN, None)
    assert runs + host == 1, ("the call did not take the GPU's code route", runs, host)
    return got, passes


@pytest.mark.parametrize("name,bits", HUF_CASES)
def test_huffman_of_the_stream_equals_the_oracle(ctx, name, bits):
    """huf_encode_all codes symbol s with entry table[s] - 1 of its code table, the rank the compaction left there: the oracle's bytes on the
    default route (the host builds the codes from the counts).  On the GPU's code route the leaves are sorted by count in as many radix
    passes as the LARGEST COUNT of the compaction needs: the oracle's bytes again, and exactly that many passes -- a largest count that
    came out too small (from part 0 alone, from a quad's first entry alone, never written) makes fewer"""
    stream, _, counts = expected_comp(name, bits)
    kind = E.KIND_OF_BITS[bits]
    want = O.huf_encode_all(kind, stream)
    assert ctx.huf_encode_all(kind, stream) == want, (name, bits)
    got, passes = gpu_codes_route(ctx, lambda: ctx.huf_encode_all(kind, stream))
    assert passes == passes_of(counts.max()), (name, bits, "radix passes", passes, "largest count", int(counts.max()))
    assert got == want, (name, bits, "on the GPU's code route")


def c5_image():
    """64 x 64 pixels of C5's six 24-bit keys"""
    keys = E.c5_keys(24)
    lin = E.image_of(E.pairs(keys, [1000, 700, 900, 600, 500, 396]), "shuffled", seed=5)
    return lin.reshape(64, 64, 3)


def test_hufman_codec_on_item_edges_and_part_edges(ctx):
    """the whole of F4 (1024 x 1024: the partition, buckets of one, two and three work items; the oracle takes 0.2 s for it) and a 64 x 64 image
    of C5's keys, byte for byte the oracle's on the default route and on the GPU's code route, there with the radix passes of the largest
    count (16385 and 1000: two)"""
    for what, img, largest in (("F4", np.ascontiguousarray(E.fill_pixels("F4_item_edges")).reshape(1024, 1024, 3), 16385), ("C5", c5_image(), 1000)):
        assert int(E.witness(E.keys_of(img))[1].max()) == largest
        rc, data, _ = ctx.encode("hufman", img)
        rco, want, _ = O.encode("hufman", img)
        assert rc == 0 and rco == 0 and len(data) == len(want) and data == want, what
        rc, back = ctx.decode("hufman", data)
        assert rc == 0 and np.array_equal(back, img), what
        (rc, data, _), passes = gpu_codes_route(ctx, lambda: ctx.encode("hufman", img))
        assert rc == 0 and passes == passes_of(largest) == 2, (what, passes)
        assert data == want, (what, "on the GPU's code route")


# ------------------------------------------------------------------ one context, many calls
def test_many_calls_on_one_context():
    """the dense table is the context's, grows from 2^24 to 2^27 bins and holds ranks after every call: F3, C7 at 27 bits, F5, a hufman encode, F3
    again, C1 at 24 bits -- each what np.unique says and what the same call gives on a context of its own"""
    from cniic_amd import Context
    img = c5_image()
    steps = [("fill", "F3_one_colour"), ("comp", ("C7_one_key_per_chunk", 27)), ("fill", "F5_all_buckets"), ("hufman", None), ("fill", "F3_one_colour"),
             ("comp", ("C1_zero_and_top", 24))]

    def run(c, kind, arg):
        if kind == "fill":
            lin = expected_fill(arg)[0]
            return ctx_pairs(c.hist_rgb24(lin, lin.shape[0]))
        if kind == "comp":
            return ctx_pairs(c.hist_syms(E.KIND_OF_BITS[arg[1]], expected_comp(*arg)[0]))
        rc, data, _ = c.encode("hufman", img)
        assert rc == 0
        return data

    def ctx_pairs(kc):
        return kc[0].copy(), kc[1].copy()

    with Context(0) as shared:
        got = [run(shared, kind, arg) for kind, arg in steps]
    for (kind, arg), g in zip(steps, got):
        with Context(0) as fresh:
            alone = run(fresh, kind, arg)
        if kind == "hufman":
            assert g == alone == O.encode("hufman", img)[1]
            continue
        keys, counts = (expected_fill(arg) if kind == "fill" else expected_comp(*arg))[1:]
        _same(g, keys, counts, (kind, arg, "shared"))
        _same(alone, keys, counts, (kind, arg, "fresh"))
