"""The decoders of small `hufman` and `cluster-colors` frames parsed on the GPU (k_small_trie.hip k_small_trieparse_rgb: a workgroup per frame
writes the table k_huf_small_dec reads; codec.cpp small_parse_dev) when cniic_codec_decode_batch / cniic_codec_measure_batch are given
streams in device memory.  Every comparison is exact: against the same call with the host's parse (CNIIC_TEST_HUF_SMALL_DEC_PARSE_OFF=1)
-- status, dimensions, pixels, message, the poison around every image and the "huf_small_dec_batch" launch count -- and against
cniic_codec_decode of each stream alone on a fresh context.  Which frames the kernel parsed is read from the stage timers
"huf_small_dec_parse" (launches = frames parsed) and "huf_small_dec_parse_host" (launches = candidates handed back to the host's path:
not a decoder, not ours, a code above 19 bits, or too large a frame); with the knob set, or in a call with fewer candidates than the
floor, neither stage exists.

tests/test_small_trie_rgb_cpu.py establishes from the oracle alone what the hand-built streams below are.  No GPU code is imported at the top."""
import numpy as np
import pytest

import test_huf_small_decode as H
import test_small_trie_gpu as G
from test_delta_small_decode import check_against_singles, singles

pytestmark = pytest.mark.gpu

MAX_LEAVES = 16384    # kSmallTrieMaxLeaves (cniic_amd/csrc/small_trie.hpp)
MAX_PX = H.MAX_PX     # kHufSmallMaxPx
CHUNK = 32            # kStChunk
LANES = 1024          # kStLanes
MAX_LANE_CHUNKS = 7   # kStMaxKRgb
LEAF = 12             # a leaf's record: its tag and S = 11 symbol bytes
FLOOR = 256           # kHufSmallDecFloorFrames (codec.cpp)
PARSE, PARSE_HOST = "huf_small_dec_parse", "huf_small_dec_parse_host"
KNOB = "CNIIC_TEST_HUF_SMALL_DEC_PARSE_OFF"
FLOOR_KNOB = "CNIIC_TEST_HUF_SMALL_FLOOR_OFF"
LONGEST_SMALL = 8 + 13 * MAX_PX - 1 + (19 * MAX_PX + 7) // 8      # hs_stream_bytes(16384, 19 * 16384): the longest candidate


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor; test_the_floor and test_larger_frames_ride_along hold it"""
    monkeypatch.setenv(FLOOR_KNOB, "1")


# ------------------------------------------------------------------ hand-built streams (no GPU)
def wide_image():
    return np.tile(np.array([7, 8, 9], np.uint8), (8, 8, 1))


def wide_stream(leaves, total=None):
    """8 x 8 pixels behind a balanced decoder of `leaves` leaves: leaf 0 is the colour (7, 8, 9), leaf i > 0 one that the payload never
    uses; the payload is leaf 0 64 times.  total: the stream's length, made up with bytes behind the payload that no decode reads"""
    def leaf(i):
        return (3).to_bytes(8, "little") + (bytes((7, 8, 9)) if i == 0 else bytes((i & 255, i >> 8, 200 + i % 50)))
    trie = bytearray()
    G._balanced(0, leaves, trie, leaf)
    data = (8).to_bytes(4, "little") * 2 + bytes(trie)
    found, pay = H.parse_trie(data)
    assert len(found) == leaves and pay == len(data) == 8 + 13 * leaves - 1
    data += G._bits("0" * found[0][1] * 64) if leaves > 1 else b""
    if total is not None:
        assert total >= len(data)
        data += bytes((0x5a + 37 * i) & 255 for i in range(total - len(data)))
    return data


def switch_streams():
    """[(k, window, stream)]: for k = 1 .. 6 a stream whose trie and payload (the window the kernel looks at: everything behind the header, up
    to 212 991 bytes) have exactly k * 32 768 bytes, the most that 1024 lanes of k chunks hold, and one with a byte more"""
    out = []
    for k in range(1, MAX_LANE_CHUNKS):
        edge = k * LANES * CHUNK
        leaves = (edge - 130) // 13                                                  # (the trie and at most 112 bytes of payload end in front of the edge)
        for window in (edge, edge + 1):
            out.append((k, window, wide_stream(leaves, 8 + window)))
    return out


def lane_chunks(window):
    chunks = (min(window, 13 * MAX_LEAVES - 1) + CHUNK - 1) // CHUNK
    return max(1, (chunks + LANES - 1) // LANES)


def cc_images():
    from cniic_amd import synth
    yy, xx = np.mgrid[0:24, 0:31]
    checker = np.where(((xx + yy) & 1)[..., None] == 1, np.array([200, 30, 40], np.uint8), np.array([10, 220, 90], np.uint8)).astype(np.uint8)
    four = np.array([(9, 9, 9), (250, 1, 1), (1, 250, 1), (1, 1, 250)], np.uint8)[(xx // 8 + yy // 8) % 4]
    return [np.full((20, 30, 3), 77, np.uint8), checker, four, synth.photo(32, 32, synth.SEED0 + 9500), synth.photo(100, 75, synth.SEED0 + 9501),
            synth.uniform(128, 128, synth.SEED0 + 9502), synth.photo(1, 1, 5)]


# ------------------------------------------------------------------ GPU helpers
stage = G.stage


def both(ctx, monkeypatch, expr, streams, img_stride, **kw):
    """the batch with the GPU parse and with the host's: equal in everything -> (result, frames parsed, candidates handed back)"""
    on = H.batch(ctx, expr, streams, img_stride, **kw)
    parsed, handed = stage(ctx, PARSE), stage(ctx, PARSE_HOST)
    monkeypatch.setenv(KNOB, "1")
    try:
        off = H.batch(ctx, expr, streams, img_stride, **kw)
        assert stage(ctx, PARSE) is None and stage(ctx, PARSE_HOST) is None          # not merely zero launches: no such stages
    finally:
        monkeypatch.delenv(KNOB)
    assert on[:4] == off[:4] and np.array_equal(on[4], off[4]) and on[5] == off[5] and on[6] == off[6] and (on[7] > 0) == (off[7] > 0)
    return on, parsed, handed


# ------------------------------------------------------------------ the tests
def test_library_hufman_streams_are_all_parsed_on_the_gpu(monkeypatch):
    import cniic_amd
    imgs = H.route_images()                                                          # 1 x 1 .. 128 x 128
    streams = H.encoded("route", "hufman", imgs)
    img_stride = 3 * MAX_PX
    want = singles(("huf", "route"), "hufman", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride)
    assert parsed == len(imgs)                                                       # (no such stage on a build without the parse: None)
    assert handed == 0                                                               # library-made streams never fall back
    assert res[5] == len(imgs) and res[7] == 0
    check_against_singles(res, want, img_stride, "route", sources=imgs)


@pytest.mark.parametrize("K", (2, 16, 256))
def test_library_cluster_colors_streams_are_all_parsed_on_the_gpu(monkeypatch, K):
    import cniic_amd
    expr = "cluster-colors(%d)" % K
    streams = H.encoded(("rgb parse cc", K), expr, cc_images())
    made = sum(1 for s in streams if s)                                              # (fewer colours than K: no stream, an empty one)
    assert made >= 3
    img_stride = 3 * MAX_PX + 3
    want = singles(("rgb parse cc", K), expr, streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, expr, streams, img_stride)
    assert (parsed, handed, res[5], res[7]) == (made, 0, made, 0)
    check_against_singles(res, want, img_stride, expr)


def _limits():
    """[(name, stream, source image or None, parsed on the GPU, routed)]"""
    imgs = H.route_images()
    streams = H.encoded("route", "hufman", imgs)
    assert imgs[0].shape == (1, 1, 3) and len(streams[0]) == 20
    assert imgs[11].shape[0] * imgs[11].shape[1] == 15126 and imgs[13].shape[:2] == (128, 128)
    return [
        ("one leaf: the 20-byte stream", streams[0], imgs[0], True, True),
        ("a 19-bit chain", streams[11], imgs[11], True, True),
        ("16 384 leaves", streams[13], imgs[13], True, True),
        ("a code of 20 bits", H.deep_stream(), None, False, False),
        ("100 leaves, 64 pixels", H.leafy_stream(), None, True, True),
    ]


def test_limit_decoders_alone_and_in_company(monkeypatch):
    import cniic_amd
    cases = _limits()
    streams = [c[1] for c in cases]
    assert [len(H.parse_trie(s)[0]) for s in streams] == [1, 20, MAX_LEAVES, 21, 100]
    assert [max(d for _, d in H.parse_trie(s)[0]) for s in streams] == [0, 19, 14, 20, 7]
    assert H.parse_trie(streams[2])[1] - 8 == 13 * MAX_LEAVES - 1                    # the full window
    img_stride = 3 * MAX_PX + 5
    want = singles(("rgb parse", "limits"), "hufman", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    sources = [c[2] for c in cases]
    with cniic_amd.Context(0) as ctx:
        for f, (name, s, _, on_gpu, routed) in enumerate(cases):
            res, parsed, handed = both(ctx, monkeypatch, "hufman", [s], img_stride)
            assert (parsed, handed, res[5]) == (int(on_gpu), int(not on_gpu), int(routed)), name
            assert (res[7] > 0) == (not routed), name                                # the batched route answers for the 20-bit code
            check_against_singles(res, want[f:f + 1], img_stride, name, sources=sources[f:f + 1])
        res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride)
        assert (parsed, handed, res[5]) == (sum(c[3] for c in cases), sum(not c[3] for c in cases), sum(c[4] for c in cases)) and res[7] > 0
        check_against_singles(res, want, img_stride, "limits together", sources=sources)


def test_failures_among_good_frames(monkeypatch):
    import cniic_amd
    good = H.encoded("route", "hufman", H.route_images())[4]                         # 7 x 9, 63 colours
    cases = H.failure_streams(good)
    streams = [c[1] for c in cases]
    names = [c[0] for c in cases]
    img_stride = 3 * 63 + 7
    want = singles(("rgb parse", "failures"), "hufman", streams, img_stride)
    for (name, s, rc, _), (src, _, _, _, _) in zip(cases, want):
        assert src == rc, name
    # handed back: cut in the trie, a tag of 2, a length word of 4; no candidate: the one without a whole header; the two cut in their
    # payloads are parsed and routed, and fail there
    assert {"cut in the dimensions", "cut in the trie", "a tag of 2", "a symbol of 4 bytes", "cut in half", "one byte short"} <= set(names)
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride)
        assert (parsed, handed, res[5]) == (len(streams) - 4, 3, sum(c[3] for c in cases))
        check_against_singles(res, want, img_stride, "failures")                     # (a failed frame's destination is all poison)
        for first in (2, 4, 7, 8):                                                   # each failure first in a batch: its message
            res, _, _ = both(ctx, monkeypatch, "hufman", streams[first:], img_stride)
            check_against_singles(res, want[first:], img_stride, names[first])


def test_streams_at_every_start_residue(monkeypatch):
    import cniic_amd
    keep = [k for k, im in enumerate(H.route_images()) if im.shape[0] * im.shape[1] <= 2049]
    imgs = ([H.route_images()[k] for k in keep] * 3)[:34]
    streams = ([H.encoded("route", "hufman", H.route_images())[k] for k in keep] * 3)[:34]
    img_stride = 3 * 2049 + 2
    stride = ((max(len(s) for s in streams) + 15) & ~15) + 1                          # no multiple of 4: frame f starts at f modulo 16
    assert {(f * stride) % 16 for f in range(len(imgs))} == set(range(16))
    want = singles(("rgb parse", "align"), "hufman", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        for src_off in (0, 1, 2, 3):
            res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride, stride=stride, src_off=src_off, out_off=5)
            assert (parsed, handed, res[5]) == (len(imgs), 0, len(imgs)), src_off
            check_against_singles(res, want, img_stride, ("start residue", src_off), sources=imgs)


def test_streams_on_both_sides_of_every_lane_chunk_switch(monkeypatch):
    import cniic_amd
    cases = switch_streams()
    assert [lane_chunks(wnd) for _, wnd, _ in cases] == [k + (wnd & 1) for k, wnd, _ in cases] and len(cases) == 12
    streams = [s for _, _, s in cases]
    img_stride = 3 * 64 + 1
    want = singles(("rgb parse", "switches"), "hufman", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        for f in (0, 1, 10, 11):                                                     # alone: the launch's pitch follows the stream
            res, parsed, handed = both(ctx, monkeypatch, "hufman", streams[f:f + 1], img_stride)
            assert (parsed, handed, res[5]) == (1, 0, 1), cases[f][:2]
            check_against_singles(res, want[f:f + 1], img_stride, cases[f][:2], sources=[wide_image()])
        res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride, stride=((max(map(len, streams)) + 15) & ~15) + 3)
    assert (parsed, handed, res[5]) == (12, 0, 12)
    check_against_singles(res, want, img_stride, "switches", sources=[wide_image()] * 12)


def larger_images():
    """16 385 and 19 200 pixels of 16 colours: too large for the small route, with streams short enough to be candidates of the parse"""
    rng = np.random.default_rng(47)
    pal = rng.integers(0, 256, (16, 3)).astype(np.uint8)
    return [pal[rng.integers(0, 16, (1, 16385))], pal[rng.integers(0, 16, (120, 160))]]


def _floor_batch():
    """eight small frames; 8, 9: the larger frames above; 10, 11: the library tests' frames of those sizes, whose streams may be longer"""
    kinds = H.route_images()[:8] + larger_images() + H.T.shaped_images()[11:]
    kstreams = H.encoded("route", "hufman", H.route_images())[:8] + H.encoded("rgb parse above", "hufman", larger_images()) + H.encoded("above", "hufman", H.T.shaped_images()[11:])
    assert [im.shape[0] * im.shape[1] for im in kinds[8:]] == [16385, 19200] * 2 and all(8 <= len(s) <= LONGEST_SMALL for s in kstreams[:10])
    img_stride = 3 * 19200
    kwant = singles(("rgb parse", "floor"), "hufman", kstreams, img_stride)
    return kinds, kstreams, kwant, img_stride


def test_larger_frames_ride_along(monkeypatch):
    """frames of 16 385 and 19 200 pixels among 256 small ones, the floor in force: the kernel skips them on their headers, they are handed
    back, and the batched route (its timer "decode_batch_pass") answers for them"""
    import cniic_amd
    monkeypatch.delenv(FLOOR_KNOB)
    kinds, kstreams, kwant, img_stride = _floor_batch()
    pick = [8, 10] + [f % 8 for f in range(FLOOR)] + [9, 11]
    longer = sum(1 for k in (10, 11) if len(kstreams[k]) > LONGEST_SMALL)                # (no candidates: not even looked at)
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, "hufman", [kstreams[k] for k in pick], img_stride)
    assert (parsed, handed, res[5]) == (FLOOR, 4 - longer, FLOOR) and res[7] > 0
    check_against_singles(res, [kwant[k] for k in pick], img_stride, "larger frames", sources=[kinds[k] for k in pick])


def test_the_floor(monkeypatch):
    """255 candidates: the parse does not run.  255 small frames and two larger ones whose streams are short enough to be candidates: it
    runs, sees 255 small frames on the result rows and routes nothing.  256 small frames: all routed"""
    import cniic_amd
    monkeypatch.delenv(FLOOR_KNOB)
    kinds, kstreams, kwant, img_stride = _floor_batch()
    small = [f % 8 for f in range(FLOOR)]
    with cniic_amd.Context(0) as ctx:
        for pick, stages, routed in ((small[1:], False, 0), (small[1:] + [8, 9], True, 0), (small, True, FLOOR)):
            res, parsed, handed = both(ctx, monkeypatch, "hufman", [kstreams[k] for k in pick], img_stride)
            assert (parsed is not None, handed is not None) == (stages, stages), len(pick)
            assert res[5] == routed and (res[7] > 0) == (routed == 0), len(pick)
            if routed:
                assert (parsed, handed) == (FLOOR, 0)
            check_against_singles(res, [kwant[k] for k in pick], img_stride, ("floor", len(pick)), sources=[kinds[k] for k in pick])


def test_many_frames_in_one_launch(monkeypatch):
    import cniic_amd
    rng = np.random.default_rng(46)
    sizes = [(16, 16), (8, 8), (13, 5), (32, 32), (1, 1), (31, 33), (64, 3), (2, 100)]
    kinds = [(rng.integers(0, 32, (h, w, 3)) * 8).astype(np.uint8) for k in range(40) for w, h in [sizes[k % len(sizes)]]]
    kstreams = H.encoded("rgb parse many", "hufman", kinds)
    streams = [kstreams[(f * 7) % 40] for f in range(3000)]
    img_stride = 3 * 1024 + 3
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride)
    assert (parsed, handed, res[5]) == (3000, 0, 3000) and res[0] == 0 and res[3] == [0] * 3000
    for f in range(3000):
        im = kinds[(f * 7) % 40]
        slot = res[4][f * img_stride:(f + 1) * img_stride]
        assert (res[1][f], res[2][f]) == (im.shape[1], im.shape[0]), f
        assert np.array_equal(slot[:im.size], im.reshape(-1)) and bool((slot[im.size:] == H.POISON).all()), f


def test_two_chunks_of_scratch(monkeypatch):
    """a lowered budget: the parse in two chunks; then, the floor in force, 300 frames in chunks that each end below the floor -- the frames
    of the chunks before the floor was met are parsed once more behind the last one, and every frame is routed"""
    import cniic_amd
    keep = [k for k, im in enumerate(H.route_images()) if im.shape[0] * im.shape[1] <= 2049]
    imgs = [H.route_images()[k] for k in keep]
    streams = [H.encoded("route", "hufman", H.route_images())[k] for k in keep]
    img_stride = 3 * 2049 + 1
    want = singles(("rgb parse", "chunks"), "hufman", streams, img_stride)
    need = [8 * min(MAX_LEAVES, (len(s) - 7) // 13) + 48 for s in streams]              # a leaf's two words as far as the stream has room, the rows
    budget = sum(need) // 2 + max(need)
    assert max(need) < budget < sum(need)
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        try:
            res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride)
            assert (parsed, handed, res[5]) == (len(streams), 0, len(streams))
            check_against_singles(res, want, img_stride, "two chunks of the parse", sources=imgs)
            monkeypatch.delenv(FLOOR_KNOB)
            many = [f % 4 for f in range(300)]
            per_frame = max(need[:4])
            monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(100 * per_frame))      # at least 100 frames a chunk, fewer than 256
            assert 100 * per_frame < FLOOR * min(need[:4])
            res, parsed, handed = both(ctx, monkeypatch, "hufman", [streams[k] for k in many], img_stride)
            assert (parsed, handed, res[5]) == (300, 0, 300)
            check_against_singles(res, [want[k] for k in many], img_stride, "chunks below the floor", sources=[imgs[k] for k in many])
        finally:
            monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")


def test_frames_switched_off_are_not_parsed(monkeypatch):
    import cniic_amd
    imgs = H.route_images()[:11]
    streams = H.encoded("route", "hufman", H.route_images())[:11]
    img_stride = 3 * MAX_PX
    want = singles(("huf", "route"), "hufman", H.encoded("route", "hufman", H.route_images()), img_stride)[:11]
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", "0,3,10")
        try:
            res, parsed, handed = both(ctx, monkeypatch, "hufman", streams, img_stride)
        finally:
            monkeypatch.delenv("CNIIC_TEST_DECODE_BATCH_OFF")
    assert (parsed, handed, res[5]) == (8, 0, 8)
    check_against_singles(res, want, img_stride, "three frames off", sources=imgs)


@pytest.mark.parametrize("expr", ("hufman", "cluster-colors(16)"))
def test_measure_batch_keeps_the_parse_stage(monkeypatch, expr):
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 9600 + i) for i, (w, h) in enumerate(sizes)]
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
    torch.cuda.synchronize()
    allow = (_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE)
    with cniic_amd.Context(0) as ctx:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch(expr, src, offs, [s[0] for s in sizes], [s[1] for s in sizes], allow=allow)
        parsed, handed, routed = stage(ctx, PARSE), stage(ctx, PARSE_HOST), stage(ctx, H.TIMER)
        monkeypatch.setenv(KNOB, "1")
        rc2, rows2, lens2 = ctx.measure_batch(expr, src, offs, [s[0] for s in sizes], [s[1] for s in sizes], allow=allow)
        assert stage(ctx, PARSE) is None and stage(ctx, PARSE_HOST) is None and stage(ctx, H.TIMER) == routed
        monkeypatch.delenv(KNOB)
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    small_ok = sum(1 for f, (w, h) in enumerate(sizes) if w * h <= MAX_PX and rows[f]["rc"] == 0)
    assert parsed == routed == small_ok >= 3 and handed is not None, (parsed, handed, routed, small_ok)   # all but 333 x 200 and 160 x 120
    assert rc == rc2 and lens == lens2
    for f in range(len(imgs)):
        a = {k: v for k, v in rows[f].items() if k != "kmeans"}
        b = {k: v for k, v in rows2[f].items() if k != "kmeans"}
        assert a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (f, a, b)   # every double equal (a failed encode's are NaN)


def test_mutants_with_and_without_the_parse(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    bases = H.encoded("mutants", "hufman", [synth.photo(8, 8, synth.SEED0 + 9400), synth.photo(37, 29, synth.SEED0 + 9401)])
    streams = H.mutant_streams(*bases)
    want_all = singles(("huf", "mutants"), "hufman", streams, H.MUTANT_STRIDE)
    keep = [k for k, s in enumerate(want_all) if s[0] in (H.OK, H.DECODE)]
    assert len(streams) == H.MUTANTS == 200 and all(8 <= len(s) <= LONGEST_SMALL for s in streams)      # every mutant is a candidate
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, "hufman", [streams[k] for k in keep], H.MUTANT_STRIDE)
    print("mutants parsed on the GPU:", parsed, "handed back or skipped:", handed, "routed:", res[5], "held back from the batch:", 200 - len(keep))
    assert parsed + handed + (200 - len(keep)) == 200
    for f, k in enumerate(keep):
        src, sw, sh, spx, _ = want_all[k]
        assert res[3][f] == src, (k, res[3][f], src)
        slot = res[4][f * H.MUTANT_STRIDE:(f + 1) * H.MUTANT_STRIDE]
        if src == 0:
            assert (res[1][f], res[2][f]) == (sw, sh) and np.array_equal(slot[:sw * sh * 3], spx), k
        else:
            assert bool((slot == H.POISON).all()), k
