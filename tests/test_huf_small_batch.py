"""Small `hufman` frames of a batch call on the small-frame route (k_huf_small in k_delta_small.hip: a workgroup per frame from the pixels to
the finished stream; include/cniic_hip.h above cniic_codec_encode_batch_var).  Every comparison is exact: a frame's status, length, bytes
and message are those of cniic_codec_encode_opts for that frame alone on a context that has seen no batch, and the bytes are the oracle's.
Which frames took the route is read from the stage timer "huf_small_batch", whose launch count is the number of routed frames: on a build
without the route that timer does not exist.

The shaped frames alternate uniform and photo-like synthetic images; CLAIMS states each one's distinct colours, longest code and stream
length, which tests/test_huf_small_cpu.py computes from the oracle alone, as it does for the further frames: the strict chain of 20 counts
that meets the 19-bit bound, the counts 1, 1, 2, 4, ..., 4096, 16 384 distinct colours, one colour (1 x 1 and flat), the ends of the
channels, and four equally frequent colours whose order differs between r-major and b-major keys."""
import numpy as np
import pytest

import test_delta_small_batch as D
from test_delta_small_batch import _pack, _round4, check_against_singles

pytestmark = pytest.mark.gpu

MAX_PX = 16384        # kHufSmallMaxPx (cniic_amd/csrc/huf_small.hpp)
MAX_CODE_LEN = 19     # kDeltaSmallMaxCodeLen (delta_small.hpp): an argument about counts, whatever the symbols
THREADS = 1024        # kDsThreads
STRIDE_AT_BOUND = 251920   # hs_stride(16384)
SHAPES = D.SHAPES     # (w, h)
# per shaped frame: (distinct colours, longest code, bytes of the stream)
CLAIMS = [(1, 0, 20), (2, 1, 34), (3, 2, 47), (4, 2, 60), (63, 6, 874), (64, 6, 887), (4096, 12, 59399), (7412, 13, 108442), (16376, 14, 241564),
          (16365, 14, 241420), (16380, 14, 241618), (16319, 14, 240812), (19186, 15, 283726)]
CHAIN = [1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207, 3571, 5778]    # 20 counts, 15 126 pixels
FURTHER = ("chain", "powers", "distinct", "one_pixel", "flat", "ends", "byte_order")
FURTHER_CLAIMS = dict(chain=(20, 19, 5215), powers=(14, 13, 2237), distinct=(16384, 14, 241671), one_pixel=(1, 0, 20), flat=(1, 0, 20),
                      ends=(4, 2, 8 + 13 * 4 - 1 + 16), byte_order=(4, 2, 8 + 13 * 4 - 1 + 5))
# pixel counts around kDsMinCap, the block's threads, twice that, and the bound: (w, h)
SIZES = [(7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (23, 89), (64, 32), (3, 683), (127, 129), (128, 128), (16384, 1), (1, 16384)]
FAILURES = D.FAILURES
CAPACITY = D.CAPACITY
TIMER = "huf_small_batch"
POISON = 0xA5
FLOOR_FRAMES, FLOOR_PX = 4, 4096     # kHufSmallFloorFew, kHufSmallFloorPxFew (capi.cpp): fewer candidate frames than that, and only frames up to so many pixels
DEC_FLOOR_FRAMES = 256               # kHufSmallDecFloorFrames (codec.cpp)


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor (few large frames stay with the workers); test_the_floor holds it"""
    monkeypatch.setenv("CNIIC_TEST_HUF_SMALL_FLOOR_OFF", "1")


def shaped_images():
    from cniic_amd import synth
    return [(synth.photo if i % 2 else synth.uniform)(w, h, synth.SEED0 + 7600 + i) for i, (w, h) in enumerate(SHAPES)]


def image_of_counts(w, h, counts, seed):
    """colour i * 7919 mod 2^24 (distinct: 7919 is odd) counts[i] times, the pixels shuffled"""
    v = np.repeat(np.arange(len(counts), dtype=np.int64) * 7919 % (1 << 24), counts)
    assert len(v) == w * h
    v = np.random.default_rng(seed).permutation(v)
    return np.stack([v >> 16, (v >> 8) & 255, v & 255], 1).astype(np.uint8).reshape(h, w, 3)


def further_images():
    chain = image_of_counts(6, 2521, CHAIN, 11)
    powers = image_of_counts(128, 64, [1] + [1 << k for k in range(13)], 12)
    d = np.arange(128 * 128, dtype=np.int64) * 1021
    distinct = np.stack([d >> 16, (d >> 8) & 255, d & 255], 1).astype(np.uint8).reshape(128, 128, 3)
    one_pixel = np.array([[[255, 0, 1]]], np.uint8)
    flat = np.full((30, 20, 3), 77, np.uint8)
    ends = np.array([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255)], np.uint8)[np.arange(64) % 4].reshape(8, 8, 3)
    byte_order = np.array([(1, 0, 0), (0, 0, 2), (0, 3, 0), (0, 0, 1)], np.uint8)[np.arange(20) % 4].reshape(4, 5, 3)
    return [chain, powers, distinct, one_pixel, flat, ends, byte_order]


def sized_images():
    from cniic_amd import synth
    return [(synth.uniform if i % 2 else synth.photo)(w, h, synth.SEED0 + 7700 + i) for i, (w, h) in enumerate(SIZES)]


def all_images():
    return shaped_images() + further_images()


def routed(imgs, max_px=MAX_PX):
    return [1 <= im.shape[0] * im.shape[1] <= max_px for im in imgs]


def singles(key, imgs):
    return D.singles(("hufman", key), "hufman", imgs)


def batch(ctx, imgs, stride, **kw):
    return D.batch(ctx, "hufman", imgs, stride, timer=TIMER, **kw)


def _stride(want):
    return _round4(max(len(s[1]) for s in want)) + 4


def test_route_and_bytes():
    import cniic_amd
    import oracle_lib as O
    imgs = all_images()
    assert len({o % 16 for o in _pack(imgs)[1]}) >= 6
    want = singles("all", imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, _stride(want))
        assert ctx.kernel_time("huf_small_place")[1] == 1
    assert res[6] == sum(routed(imgs)) == len(imgs) - 2          # all but 5 x 3277 and 160 x 120, which ride along with equal bytes
    check_against_singles(res, want, "hufman")
    for f, im in enumerate(imgs):
        rco, edata, est = O.encode("hufman", im)
        assert rco == 0 and res[4][f] == edata, f
    assert [res[1][f] for f in range(len(SHAPES))] == [c[2] for c in CLAIMS]
    assert [res[1][len(SHAPES) + k] for k in range(len(FURTHER))] == [FURTHER_CLAIMS[name][2] for name in FURTHER]


def test_sizes_alone_and_in_company():
    """cap_px is the launch's largest frame rounded up to a power of two: alone, 63 / 64 / 65 pixels stand around kDsMinCap, 1023 .. 2049 around
    one and two keys a thread, 16 384 fills the LDS arrays exactly; in company every frame runs under the bound's arrays"""
    import cniic_amd
    sized, (chain, powers, distinct) = sized_images(), further_images()[:3]
    assert [im.shape[0] * im.shape[1] for im in sized] == [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16384, 16384]
    imgs = sized + [chain, distinct]
    want = singles("sizes", imgs)
    assert all(s[0] == 0 for s in want)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        for f, im in enumerate(imgs):
            res = batch(ctx, [im], stride, poison=POISON)
            assert res[6] == 1, f
            check_against_singles(res, want[f:f + 1], "alone %d" % f)
            assert bool((res[5][res[1][0]:] == POISON).all()), f
        company = [distinct] + imgs
        res = batch(ctx, company, stride, poison=POISON)
        assert res[6] == len(company)
        check_against_singles(res, [want[-1]] + want, "company")
        for f in range(len(company)):
            assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), f     # nothing behind a stream's end
    assert len(want[-2][1]) == FURTHER_CLAIMS["chain"][2] and len(want[-1][1]) == FURTHER_CLAIMS["distinct"][2]


def test_route_off_and_a_lowered_bound(monkeypatch):
    import cniic_amd
    imgs = all_images()
    want = singles("all", imgs)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, imgs, stride)
        monkeypatch.setenv("CNIIC_TEST_HUF_SMALL_OFF", "1")
        off = batch(ctx, imgs, stride)
        assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0     # not merely zero launches: no such stage
        monkeypatch.delenv("CNIIC_TEST_HUF_SMALL_OFF")
        monkeypatch.setenv("CNIIC_TEST_HUF_SMALL_MAX_PX", "4096")
        low = batch(ctx, imgs, stride)
        monkeypatch.delenv("CNIIC_TEST_HUF_SMALL_MAX_PX")
    assert on[6] == len(imgs) - 2 and off[6] == 0 and low[6] == sum(routed(imgs, 4096)) < on[6]
    for res, what in ((off, "route off"), (low, "bound 4096")):
        assert (on[0], on[1], on[2], on[4]) == (res[0], res[1], res[2], res[4]), what
        check_against_singles(res, want, what)


def test_host_images_are_not_routed_and_host_output_gets_the_same_bytes():
    import cniic_amd
    imgs = all_images()
    want = singles("all", imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs[:9], _stride(want), host_src=True, host_out=True)
        assert res[6] == 0
        check_against_singles(res, want[:9], "host source")
        res = batch(ctx, imgs, _stride(want), host_out=True, poison=POISON)
        assert res[6] == len(imgs) - 2
        check_against_singles(res, want, "host out")
        stride = _stride(want)
        for f in range(len(imgs)):
            if routed(imgs)[f]:
                assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), f


@pytest.mark.parametrize("out_off,host_out", ((1, False), (14, False), (7, True)))
def test_streams_placed_at_every_alignment(out_off, host_out):
    """odd stride, the output pointer off its 16-byte boundary: every destination residue, poison before, between and behind the streams"""
    import cniic_amd
    kinds = [all_images()[k] for k in (0, 1, 2, 3, 4, 5, len(SHAPES) + 6)]       # 20 .. 887 bytes, seven kinds: coprime to 16
    want1 = singles("placement", kinds)
    assert all(s[0] == 0 for s in want1) and len({len(s[1]) for s in want1}) >= 6
    F = 16 * len(kinds)
    imgs, want = [kinds[f % 7] for f in range(F)], [want1[f % 7] for f in range(F)]
    stride = (max(len(s[1]) for s in want1) + 8) | 1
    assert {(out_off + f * stride) % 16 for f in range(F)} == set(range(16))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride, host_out=host_out, poison=POISON, out_off=out_off)
    assert res[6] == F and res[0] == 0
    check_against_singles(res, want, "placement %d" % out_off)
    (whole, at), lens = res[5], res[1]
    assert bool((whole[:at] == POISON).all()) and bool((whole[at + F * stride:] == POISON).all())
    for f in range(F):
        assert bool((whole[at + f * stride + lens[f]:at + (f + 1) * stride] == POISON).all()), f


@pytest.mark.parametrize("host_out", (False, True))
def test_capacity_is_one_frame_s(host_out):
    import cniic_amd
    imgs = all_images()[4:9] + further_images()[:2] + further_images()[3:]     # all on the route; 127 x 129 is the longest by far
    want = singles("capacity", imgs)
    assert all(s[0] == 0 for s in want)
    by_len = sorted(range(len(imgs)), key=lambda f: -len(want[f][1]))
    big, second = by_len[0], by_len[1]
    stride = _round4(len(want[second][1])) + 4
    assert stride < len(want[big][1])
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, imgs, stride, host_out=host_out, poison=POISON)
    assert launches == len(imgs) and rc == CAPACITY
    assert msg == "encode: stream is %d bytes, capacity %d" % (len(want[big][1]), stride)
    for f in range(len(imgs)):
        assert lens[f] == len(want[f][1]), f
        if f == big:
            assert rcs[f] == CAPACITY and bool((host[f * stride:(f + 1) * stride] == POISON).all())
        else:
            assert rcs[f] == 0 and streams[f] == want[f][1], f
            assert bool((host[f * stride + lens[f]:(f + 1) * stride] == POISON).all()), f


def tiny_images():
    """at most 16 x 16"""
    from cniic_amd import synth
    return [synth.uniform(16, 16, synth.SEED0 + 7950), synth.photo(12, 9, synth.SEED0 + 7951), synth.uniform(7, 9, synth.SEED0 + 7952), np.full((4, 5, 3), 77, np.uint8)]


@pytest.mark.parametrize("host_out", (False, True))
def test_a_chunk_whose_frames_all_exceed_their_capacity(host_out):
    """every frame has a stream and none has the room: nothing is placed, no place timer is recorded, no byte is written"""
    import cniic_amd
    imgs = tiny_images()
    want = singles("tiny", imgs)
    assert all(s[0] == 0 and len(s[1]) > 8 for s in want)
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, imgs, 8, host_out=host_out, poison=POISON)
        assert ctx.kernel_time("huf_small_place")[1] == 0
    assert launches == len(imgs) and rc == CAPACITY and rcs == [CAPACITY] * len(imgs)
    assert lens == [len(s[1]) for s in want]
    assert msg == "encode: stream is %d bytes, capacity 8" % len(want[0][1])
    assert bool((host == POISON).all())


@pytest.mark.parametrize("host_out", (False, True))
def test_a_frame_a_chunk(host_out, monkeypatch):
    """CNIIC_TEST_MEASURE_BUDGET=1: every frame is a chunk of its own, placed (device memory) or copied down (host memory) once per chunk"""
    import cniic_amd
    imgs = tiny_images()
    want = singles("tiny", imgs)
    stride = _stride(want)
    monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride, host_out=host_out, poison=POISON)
        assert ctx.kernel_time("huf_small_place")[1] == (0 if host_out else len(imgs))
    monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert res[6] == len(imgs)
    check_against_singles(res, want, "a frame a chunk")
    for f in range(len(imgs)):
        assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), f


def test_the_floor(monkeypatch):
    """in a call with fewer than FLOOR_FRAMES candidate frames only those of at most FLOOR_PX pixels take the route: one CU is slower for
    one large frame than the workers' whole chip (NOTES AF)"""
    import cniic_amd
    from cniic_amd import synth
    monkeypatch.delenv("CNIIC_TEST_HUF_SMALL_FLOOR_OFF")
    big, edge, above = synth.photo(128, 128, synth.SEED0 + 7900), synth.photo(64, 64, synth.SEED0 + 7901), synth.photo(17, 241, synth.SEED0 + 7902)
    tiny = [synth.uniform(5, 3, synth.SEED0 + 7910 + i) for i in range(FLOOR_FRAMES - 1)]
    assert edge.shape[0] * edge.shape[1] == FLOOR_PX and above.shape[0] * above.shape[1] == FLOOR_PX + 1
    imgs = [big, edge, above] + tiny
    want = singles("floor", imgs)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        for which, routed_frames in (([0], 0), ([1], 1), ([2], 0), ([0, 1, 2] + list(range(3, 3 + FLOOR_FRAMES - 4)), FLOOR_FRAMES - 3),
                                     ([0, 1, 2] + list(range(3, 3 + FLOOR_FRAMES - 3)), FLOOR_FRAMES)):
            res = batch(ctx, [imgs[k] for k in which], stride)
            assert res[6] == routed_frames, (which, res[6])
            check_against_singles(res, [want[k] for k in which], "floor %r" % (which,))


def _many():
    rng = np.random.default_rng(47)
    sizes = [(8, 8), (9, 7), (16, 12), (1, 1), (13, 5), (3, 2), (12, 12), (2, 37)]
    imgs = []
    for f in range(3000):
        w, h = sizes[f % 8]
        imgs.append((rng.integers(0, 4, (h, w, 3)) * 85).astype(np.uint8))      # at most 64 colours: short and long codes, ties
    return imgs


def test_many_frames_in_one_launch():
    import cniic_amd
    import oracle_lib as O
    imgs = _many()
    stride = _round4(8 + 13 * 64 - 1 + (MAX_CODE_LEN * 16 * 12 + 7) // 8) + 4
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, imgs, stride)
        assert launches == 3000 and rc == 0 and rcs == [0] * 3000
        with cniic_amd.Context(0) as ref:
            for f in range(0, 3000, 75):
                src, sdata, sst = ref.encode("hufman", imgs[f])
                assert src == 0 and streams[f] == sdata, f
    for f in range(1, 3000, 7):
        assert streams[f] == O.encode("hufman", imgs[f])[1], f


def test_one_call_in_two_chunks(monkeypatch):
    """huf_small_encode sizes a chunk by the slot, scratch and rows of its first (largest) frame under CNIIC_TEST_MEASURE_BUDGET"""
    import cniic_amd
    imgs = all_images()
    want = singles("all", imgs)
    stride = _stride(want)
    frame = STRIDE_AT_BOUND + 12 * MAX_PX + 16 + 8        # huf_small_frame_bytes(16384)
    n_routed = sum(routed(imgs))
    at_bound = sum(im.shape[0] * im.shape[1] == MAX_PX for im in imgs)
    assert at_bound == 3 and n_routed > 4
    with cniic_amd.Context(0) as ctx:
        one = batch(ctx, imgs, stride)
        assert ctx.kernel_time("huf_small_place")[1] == 1
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(2 * frame))      # two of the largest, then the rest under a smaller frame's slot
        two = batch(ctx, imgs, stride)
        chunks = ctx.kernel_time("huf_small_place")[1]
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")                 # a frame a chunk
        many = batch(ctx, imgs, stride)
        assert ctx.kernel_time("huf_small_place")[1] == n_routed
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert 2 <= chunks < n_routed
    for res in (two, many):
        assert res[6] == n_routed and res[:5] == one[:5]
    check_against_singles(two, want, "two chunks")


def test_measure_batch_is_the_loop_of_the_three_single_calls():
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 7800 + i) for i, (w, h) in enumerate(sizes)] + further_images()[:2]
    want = singles("measure", imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        rows_want = []
        for im, (rc, data, st, _) in zip(imgs, want):
            rc2, back = ctx.decode("hufman", data)
            assert rc2 == 0 and np.array_equal(back, im)
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
        buf, offs, ws, hs = _pack(imgs)
        F = len(imgs)
        stride = _stride(want) + 4
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch("hufman", src, offs, ws, hs, out, stride, allow=FAILURES)
        launches, places = ctx.kernel_time(TIMER)[1], ctx.kernel_time("huf_small_place")[1]     # the encode's stages, readable after the decode
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == F - 2 and places == 1 and rc == 0
        host = out.cpu().numpy()
        for f in range(F):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f] and got["error"] == 0.0, (f, got, rows_want[f])
            assert rows[f]["lossless_mismatch"] == 0
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f
