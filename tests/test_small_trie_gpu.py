"""The decoders of small `delta` frames parsed on the GPU (k_small_trie.hip: a workgroup per frame writes the table k_delta_small_dec reads;
codec.cpp delta_small_parse_dev) when cniic_codec_decode_batch / cniic_codec_measure_batch are given streams in device memory.  Every
comparison is exact: against the same call with the host's parse (CNIIC_TEST_DELTA_SMALL_DEC_PARSE_OFF=1) -- status, dimensions, pixels,
message, the poison around every image and the "delta_small_dec_batch" launch count -- and against cniic_codec_decode of each stream alone
on a fresh context.  Which frames the kernel parsed is read from the stage timers "delta_small_dec_parse" (launches = frames parsed) and
"delta_small_dec_parse_host" (launches = candidates handed back to the host's parse); with the knob set neither stage exists.

tests/test_small_trie_cpu.py establishes from the oracle alone what the hand-built streams below are.  No GPU code is imported at the top."""
import numpy as np
import pytest

import test_delta_small_decode as T

pytestmark = pytest.mark.gpu

MAX_LEAVES = 16384    # kSmallTrieMaxLeaves (cniic_amd/csrc/small_trie.hpp)
CHUNK = 32            # kStChunk
PARSE, PARSE_HOST = "delta_small_dec_parse", "delta_small_dec_parse_host"
KNOB = "CNIIC_TEST_DELTA_SMALL_DEC_PARSE_OFF"


# ------------------------------------------------------------------ hand-built streams (no GPU)
def _balanced(lo, hi, out, leaf):
    """the pre-order trie over leaves lo .. hi - 1, split in halves"""
    if hi - lo == 1:
        out += b"\x00" + leaf(lo)
        return
    mid = lo + (hi - lo + 1) // 2
    out += b"\x01"
    _balanced(lo, mid, out, leaf)
    _balanced(mid, hi, out, leaf)


def _bits(s):
    s += "0" * (-len(s) % 8)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def wide_stream(leaves):
    """8 x 8 pixels behind a balanced decoder of `leaves` leaves: leaf 0 is the difference (7, 8, 9), leaf 1 is (0, 0, 0), leaf i > 1 one
    that the payload never uses; the payload is leaf 0 once, then leaf 1 63 times: every pixel (7, 8, 9)"""
    def leaf(i):
        return T.leaf_bytes((7, 8, 9) if i == 0 else (0, 0, 0) if i == 1 else (i % 255 + 1, i // 255 % 255, -(i // 65025)))
    trie = bytearray()
    _balanced(0, leaves, trie, leaf)
    data = (8).to_bytes(4, "little") * 2 + bytes(trie)
    found, pay = T.parse_trie(data)
    assert len(found) == leaves and pay == len(data) == 8 + 8 * leaves - 1
    code, codes = 0, []
    for _, depth in found[:2]:                                     # leaves in pre-order: ascending left-aligned codes
        codes.append(format(code >> (32 - depth), "0%db" % depth))
        code += 1 << (32 - depth)
    return data + _bits(codes[0] + codes[1] * 63)


def wide_image():
    return np.tile(np.array([7, 8, 9], np.uint8), (8, 8, 1))


def broken_streams(good):
    """good: the stream of T.range_image().  -> [(name, stream)]: four that are no decoders, each a candidate of the parse (a whole header)"""
    leaves, pay = T.parse_trie(good)
    first = leaves[0][0]                                           # the six symbol bytes of the first leaf
    assert good[8] == 1 and len(leaves) == 4
    return [
        ("a tag of 2", good[:first - 1] + b"\x02" + good[first:]),
        ("a symbol of 256", good[:first] + T.leaf_bytes((256, 0, 0)) + good[first + 6:]),
        ("cut inside a leaf", good[:first + 3]),
        ("cut behind a branch", good[:9]),
    ]


# ------------------------------------------------------------------ GPU helpers
def stage(ctx, name):
    """launches of a stage of the last call, None when there is no such stage"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, C.byref(n))
    return int(n.value) if rc == 0 else None


def both(ctx, monkeypatch, streams, img_stride, **kw):
    """the batch with the GPU parse and with the host's: equal in everything -> (result, frames parsed, frames handed back)"""
    on = T.batch(ctx, "delta", streams, img_stride, **kw)
    parsed, handed = stage(ctx, PARSE), stage(ctx, PARSE_HOST)
    monkeypatch.setenv(KNOB, "1")
    try:
        off = T.batch(ctx, "delta", streams, img_stride, **kw)
        assert stage(ctx, PARSE) is None and stage(ctx, PARSE_HOST) is None          # not merely zero launches: no such stages
    finally:
        monkeypatch.delenv(KNOB)
    assert on[:4] == off[:4] and np.array_equal(on[4], off[4]) and on[5] == off[5] and on[6] == off[6]
    return on, parsed, handed


# ------------------------------------------------------------------ the tests
def test_library_streams_are_all_parsed_on_the_gpu(monkeypatch):
    import cniic_amd
    imgs = T.route_images()
    streams = T.encoded("route", imgs)
    img_stride = 3 * T.MAX_PX
    want = T.singles("route", "delta", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
    assert parsed == len(imgs)                                                       # (no such stage on a build without the parse: None)
    assert handed == 0                                                               # library-made streams never fall back
    assert res[5] == len(imgs)
    T.check_against_singles(res, want, img_stride, "route", sources=imgs)


def _limits():
    """[(name, stream, source image or None, parsed on the GPU, routed)]"""
    import delta_small_edges as E
    imgs = T.route_images()
    streams = T.encoded("route", imgs)
    assert imgs[0].shape == (1, 1, 3) and not imgs[-1].any()
    return [
        ("1 x 1", streams[0], imgs[0], True, True),
        ("black: one leaf", streams[-1], imgs[-1], True, True),
        ("a 19-bit chain", E.oracle_stream("chain19"), E.image("chain19"), True, True),
        ("16 384 leaves", E.oracle_stream("all_distinct"), E.image("all_distinct"), True, True),
        ("a code of 20 bits", T.deep_stream(), wide_image(), False, False),
        ("16 385 leaves", wide_stream(MAX_LEAVES + 1), wide_image(), False, True),
        ("100 leaves, 64 pixels", wide_stream(100), wide_image(), True, True),
    ]


def test_limit_decoders_alone_and_in_company(monkeypatch):
    import cniic_amd
    import delta_small_edges as E
    assert E.CLAIMS["chain19"][1] == T.MAX_CODE_LEN and E.CLAIMS["all_distinct"][0] == MAX_LEAVES == T.MAX_PX
    cases = _limits()
    streams = [c[1] for c in cases]
    img_stride = 3 * T.MAX_PX + 5
    want = T.singles("trie limits", "delta", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    sources = [c[2] for c in cases]
    with cniic_amd.Context(0) as ctx:
        for f, (name, s, _, on_gpu, routed) in enumerate(cases):
            res, parsed, handed = both(ctx, monkeypatch, [s], img_stride)
            assert (parsed, handed, res[5]) == (int(on_gpu), int(not on_gpu), int(routed)), name
            T.check_against_singles(res, want[f:f + 1], img_stride, name, sources=sources[f:f + 1])
        res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
        assert (parsed, handed, res[5]) == (sum(c[3] for c in cases), sum(not c[3] for c in cases), sum(c[4] for c in cases))
        T.check_against_singles(res, want, img_stride, "limits together", sources=sources)


def test_failures_among_good_frames(monkeypatch):
    import cniic_amd
    good = T.encoded("range", [T.range_image()])[0]
    cases = T.failure_streams(good)
    broken = broken_streams(good)
    streams = [c[1] for c in cases] + [good] + [s for _, s in broken] + [good]
    img_stride = 3 * 64 + 7
    want = T.singles("trie failures", "delta", streams, img_stride)
    for name, (src, _, _, _, smsg) in zip([n for n, _ in broken], want[len(cases) + 1:]):
        assert src == T.DECODE and smsg, (name, src, smsg)                            # the single decode refuses each of them
    # handed back: the stream cut in its trie, the 20-bit chain, the four broken ones; no candidate: the one without a whole header
    names = [c[0] for c in cases]
    handed_want = 2 + len(broken)
    parsed_want = len(streams) - handed_want - 1
    assert "cut in the dimensions" in names and "cut in the trie" in names and "a code of 20 bits" in names
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
        assert (parsed, handed) == (parsed_want, handed_want)
        assert res[5] == sum(c[4] for c in cases) + 2                                # the routed frames: what they are without the parse
        T.check_against_singles(res, want, img_stride, "failures")                    # (a failed frame's destination is all poison)
        res, parsed, handed = both(ctx, monkeypatch, streams[len(cases):], img_stride)
        assert (parsed, handed, res[5]) == (2, len(broken), 2)
        T.check_against_singles(res, want[len(cases):], img_stride, "broken among good")


def test_streams_at_every_start_residue(monkeypatch):
    import cniic_amd
    imgs = [im for im in T.route_images() if im.shape[0] * im.shape[1] <= 2049][:34]
    streams = T.encoded("route", T.route_images())[:len(imgs)]
    img_stride = 3 * 2049 + 2
    stride = ((max(len(s) for s in streams) + 15) & ~15) + 1                          # no multiple of 4: frame f starts at f modulo 16
    assert {(f * stride) % 16 for f in range(len(imgs))} == set(range(16))
    want = T.singles("align", "delta", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        for src_off in (0, 1, 2, 3):
            res, parsed, handed = both(ctx, monkeypatch, streams, img_stride, stride=stride, src_off=src_off, out_off=5)
            assert (parsed, handed, res[5]) == (len(imgs), 0, len(imgs)), src_off
            T.check_against_singles(res, want, img_stride, ("start residue", src_off), sources=imgs)


def test_many_frames_in_one_launch(monkeypatch):
    import cniic_amd
    rng = np.random.default_rng(45)
    sizes = [(16, 16), (8, 8), (13, 5), (32, 32), (1, 1), (31, 33), (64, 3), (2, 100)]
    kinds = [(rng.integers(0, 32, (h, w, 3)) * 8).astype(np.uint8) for k in range(40) for w, h in [sizes[k % len(sizes)]]]
    kstreams = T.encoded("trie many", kinds)
    streams = [kstreams[(f * 7) % 40] for f in range(3000)]
    img_stride = 3 * 1024 + 3
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
    assert (parsed, handed, res[5]) == (3000, 0, 3000) and res[0] == 0 and res[3] == [0] * 3000
    for f in range(3000):
        im = kinds[(f * 7) % 40]
        slot = res[4][f * img_stride:(f + 1) * img_stride]
        assert (res[1][f], res[2][f]) == (im.shape[1], im.shape[0]), f
        assert np.array_equal(slot[:im.size], im.reshape(-1)) and bool((slot[im.size:] == T.POISON).all()), f


def test_two_chunks_of_scratch(monkeypatch):
    import cniic_amd
    imgs = T.route_images()[9:30]
    streams = T.encoded("route", T.route_images())[9:30]
    img_stride = 3 * 2049 + 1
    want = T.singles("chunks", "delta", streams, img_stride)
    need = [8 * min(MAX_LEAVES, (len(s) - 7) // 8) + 48 for s in streams]              # a leaf's two words as far as the stream has room, the rows
    budget = sum(need) // 2 + max(need)
    assert max(need) < budget < sum(need)
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        try:
            res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
        finally:
            monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert (parsed, handed, res[5]) == (len(streams), 0, len(streams))
    T.check_against_singles(res, want, img_stride, "two chunks of the parse", sources=imgs)


def test_frames_switched_off_are_not_parsed(monkeypatch):
    import cniic_amd
    imgs = [im for im in T.route_images() if im.shape[:2] in ((29, 37), (8, 8))]
    w, h = 37, 29
    p = np.random.default_rng(9).permutation(w * h)
    scan = (w, h, np.stack([p % w, p // w], 1).astype(np.uint32))
    streams = T.encoded("scan", imgs)
    assert len(streams) == 6
    img_stride = 3 * w * h
    want = T.singles("scan", "delta", streams, img_stride, scan=scan)
    builtin = T.singles("scan builtin", "delta", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        ctx.set_scan(*scan)
        res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
        assert (parsed, handed, res[5]) == (3, 0, 3)                                  # the 8 x 8 frames
        T.check_against_singles(res, want, img_stride, "injected scan")
        ctx.set_scan(w, h, None)
        monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", "1,4")
        try:
            res, parsed, handed = both(ctx, monkeypatch, streams, img_stride)
        finally:
            monkeypatch.delenv("CNIIC_TEST_DECODE_BATCH_OFF")
        assert (parsed, handed, res[5]) == (4, 0, 4)
        T.check_against_singles(res, builtin, img_stride, "two frames off", sources=imgs)


def test_measure_batch_keeps_the_parse_stage(monkeypatch):
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 8600 + i) for i, (w, h) in enumerate(sizes)]
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
    torch.cuda.synchronize()
    with cniic_amd.Context(0) as ctx:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch("delta", src, offs, [s[0] for s in sizes], [s[1] for s in sizes])
        parsed, handed, routed = stage(ctx, PARSE), stage(ctx, PARSE_HOST), stage(ctx, T.TIMER)
        monkeypatch.setenv(KNOB, "1")
        rc2, rows2, lens2 = ctx.measure_batch("delta", src, offs, [s[0] for s in sizes], [s[1] for s in sizes])
        assert stage(ctx, PARSE) is None and stage(ctx, PARSE_HOST) is None and stage(ctx, T.TIMER) == routed
        monkeypatch.delenv(KNOB)
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert (parsed, handed, routed) == (5, 0, 5)                                     # all but 333 x 200 and 160 x 120
    assert rc == rc2 == 0 and lens == lens2
    for f in range(len(imgs)):
        a = {k: v for k, v in rows[f].items() if k != "kmeans"}
        b = {k: v for k, v in rows2[f].items() if k != "kmeans"}
        assert a == b and a["error"] == 0.0 and a["rc"] == 0, (f, a, b)              # every double equal


def test_mutants_with_and_without_the_parse(monkeypatch):
    import cniic_amd
    streams = T.mutant_streams(*T.encoded("mutants", list(T.mutant_sources())))
    want_all = T.singles("mutants", "delta", streams, T.MUTANT_STRIDE)
    keep = [k for k, s in enumerate(want_all) if s[0] in (T.OK, T.DECODE)]
    with cniic_amd.Context(0) as ctx:
        res, parsed, handed = both(ctx, monkeypatch, [streams[k] for k in keep], T.MUTANT_STRIDE)
    print("mutants parsed on the GPU:", parsed, "handed back:", handed, "routed:", res[5], "of", len(keep))
    assert parsed >= 1 and parsed + handed <= len(keep)
    for f, k in enumerate(keep):
        src, sw, sh, spx, _ = want_all[k]
        assert res[3][f] == src, (k, res[3][f], src)
        if src == 0:
            assert (res[1][f], res[2][f]) == (sw, sh) and np.array_equal(res[4][f * T.MUTANT_STRIDE:f * T.MUTANT_STRIDE + sw * sh * 3], spx), k
