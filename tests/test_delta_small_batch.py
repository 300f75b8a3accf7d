"""Small `delta` frames of a batch call on the small-frame route (k_delta_small.hip: a workgroup per frame from the pixels to the finished
stream; include/cniic_hip.h above cniic_codec_encode_batch_var).  Every comparison is exact: a frame's status, length, bytes and message
are those of cniic_codec_encode_opts for that frame alone on a context that has seen no batch, and -- up to 128 x 128 -- the bytes are the
oracle's.  Which frames took the route is read from the stage timer "delta_small_batch", whose launch count is the number of routed
frames: on a build without the route that timer does not exist.

The shaped frames alternate photo-like and uniform synthetic images; CLAIMS states each one's distinct symbols, longest code and stream
length, which tests/test_delta_small_cpu.py computes from the oracle alone.  The further frames -- all black (one symbol), flat 77 (two),
a checkerboard, white / black alternating along the scan (differences of +-255 on all channels), and the histogram 1, 1, 2, 4, ..., 4096
as a 128 x 64 image (14 leaves, longest code 13) -- ride in the same calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_PX = 16384   # kDeltaSmallMaxPx (cniic_amd/csrc/delta_small.hpp)
MAX_CODE_LEN = 19   # kDeltaSmallMaxCodeLen
SHAPES = [(1, 1), (1, 2), (3, 1), (2, 2), (7, 9), (8, 8), (64, 64), (100, 75), (127, 129), (1, 16384), (128, 128), (5, 3277), (160, 120)]   # (w, h)
# per shaped frame: (distinct symbols, longest code, bytes of the stream)
CLAIMS = [(1, 0, 15), (2, 1, 24), (3, 2, 32), (4, 2, 40), (63, 6, 559), (64, 6, 567), (4095, 12, 38911), (5903, 13, 58888), (16377, 14, 159692),
          (10502, 14, 110995), (16383, 14, 159743), (10512, 14, 111087), (19195, 15, 187870)]
ORACLE_MAX_PX = 128 * 128
FAILURES = (-1, -8)  # BAD_ARG, CAPACITY
CAPACITY = -8
TIMER = "delta_small_batch"


def shaped_images():
    from cniic_amd import synth
    return [(synth.photo if i % 2 else synth.uniform)(w, h, synth.SEED0 + 7400 + i) for i, (w, h) in enumerate(SHAPES)]   # (128 x 128: uniform)


def powers_diffs():
    """8192 differences whose histogram is 1, 1, 2, 4, ..., 4096: a +1 step of count 2c beside a -2 step of count c per channel combination, in
    the order +, +, - so that the pixel stays within 0 .. 2; the two single ones are (1, 1, 1) and (-1, -1, -1)"""
    combos = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
    d = []
    c = 2048
    for m in combos:
        up, down = list(m), [-2 * v for v in m]
        d += [up, up, down] * c
        c //= 4
    d += [[1, 1, 1], [-1, -1, -1]]
    return np.array(d, np.int64)


def further_images():
    from delta_limits_ref import image_from_diffs
    black = np.zeros((20, 30, 3), np.uint8)
    flat = np.full((20, 30, 3), 77, np.uint8)
    yy, xx = np.mgrid[0:24, 0:31]
    checker = np.where(((xx + yy) & 1)[..., None] == 1, np.array([200, 30, 40], np.uint8), np.array([10, 220, 90], np.uint8)).astype(np.uint8)
    flips = np.tile(np.array([[255, 255, 255], [-255, -255, -255]], np.int64), (33 * 17 // 2 + 1, 1))[:33 * 17]
    return [black, flat, checker, image_from_diffs(33, 17, flips), image_from_diffs(128, 64, powers_diffs())]


def all_images():
    return shaped_images() + further_images()


def routed(imgs, max_px=MAX_PX):
    return [1 <= im.shape[0] * im.shape[1] <= max_px for im in imgs]


def _pack(imgs):
    """back to back: 3 w h is rarely a multiple of 16, so the offsets take many residues"""
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    return np.concatenate([im.reshape(-1) for im in imgs]), offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]


def _round4(n):
    return (n + 3) & ~3


def _last_error(ctx):
    return (ctx._L.cniic_last_error(ctx.h) or b"").decode()


_SINGLES = {}


def singles(key, expr, imgs, scan=None):
    """cniic_codec_encode_opts of every image alone, on a context that has seen no batch -> [(rc, bytes, stats, message)]; computed once per key"""
    import cniic_amd
    if key not in _SINGLES:
        res = []
        with cniic_amd.Context(0) as ref:
            if scan is not None:
                ref.set_scan(*scan)
            for im in imgs:
                rc, data, st = ref.encode(expr, im, allow=FAILURES)
                res.append((rc, data, st, _last_error(ref) if rc != 0 else ""))
        _SINGLES[key] = res
    return _SINGLES[key]


def output_buffer(nbytes, out_off, host_out, poison):
    """(buffer, at): a poisoned allocation of 16 + out_off + nbytes + 16 bytes and the index `at` in it whose address is out_off modulo 16
    (at = out_off where the allocation is 16-byte aligned): the output pointer of a call is buffer[at:]"""
    import torch
    total = 16 + out_off + nbytes + 16
    buf = np.full(total, poison, np.uint8) if host_out else torch.full((total,), poison, dtype=torch.uint8, device=torch.device("cuda", 0))
    base = buf.ctypes.data if host_out else buf.data_ptr()
    return buf, (-base) % 16 + out_off


def batch(ctx, expr, imgs, stride, host_out=False, host_src=False, poison=0, out_off=None, timer=TIMER):
    """one cniic_codec_encode_batch_var call with the stage timers on -> (rc, lens, rcs, stats, streams, raw output, routed frames, message).
    With out_off (0 .. 15) the output pointer is out_off modulo 16 inside a larger poisoned allocation, and the raw output is then
    (the whole allocation, the index of the output pointer in it)"""
    import torch
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    buf, offs, ws, hs = _pack(imgs)
    F = len(imgs)
    src = buf if host_src else torch.from_numpy(buf).to(dev)
    if out_off is None:
        whole, at = (np.full(stride * F, poison, np.uint8) if host_out else torch.full((stride * F,), poison, dtype=torch.uint8, device=dev)), 0
    else:
        whole, at = output_buffer(stride * F, out_off, host_out, poison)
    out = whole[at:]
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, lens, rcs, sts = ctx.encode_batch_var(expr, src, offs, ws, hs, out, stride, allow=FAILURES)
        msg = _last_error(ctx) if rc != 0 else ""
        launches = ctx.kernel_time(timer)[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    whole = whole if host_out else whole.cpu().numpy()
    host = whole[at:]
    streams = [host[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == 0 else None for f in range(F)]
    return rc, lens, rcs, sts, streams, host if out_off is None else (whole, at), launches, msg


def check_against_singles(res, want, what):
    rc, lens, rcs, sts, streams = res[:5]
    for f, (src, sdata, sst, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        assert sts[f] == sst and all(v == 0 for v in sts[f].values()), (what, f, sts[f], sst)
        if src == 0:
            assert lens[f] == len(sdata) and streams[f] == sdata, (what, f)
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first])
    if first is not None:
        assert res[7] == want[first][3], (what, res[7], want[first][3])


def _stride(want):
    return _round4(max(len(s[1]) for s in want)) + 4


def test_route_and_bytes():
    import cniic_amd
    import oracle_lib as O
    imgs = all_images()
    assert len({o % 16 for o in _pack(imgs)[1]}) >= 6
    want = singles("all", "delta", imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", imgs, _stride(want))
    assert res[6] == sum(routed(imgs)) == len(imgs) - 2          # all but 5 x 3277 and 160 x 120
    check_against_singles(res, want, "delta")
    for f, im in enumerate(imgs):
        if im.shape[0] * im.shape[1] <= ORACLE_MAX_PX:
            rco, edata, est = O.encode("delta", im)
            assert rco == 0 and res[4][f] == edata, f
    assert [res[1][f] for f in range(len(SHAPES))] == [c[2] for c in CLAIMS]
    n = len(SHAPES)
    assert res[1][n] == 15 and res[1][n + 1] == 8 + 15 + (599 + 7) // 8      # one symbol: no payload; two: a bit per pixel but the first
    assert res[1][n + 4] == 8 + 8 * 14 - 1 + (2 * 8191 + 7) // 8               # counts 2^k: sum of count * length = 2 * 8192 - 2 bits


def test_same_batch_with_the_route_off(monkeypatch):
    import cniic_amd
    imgs = all_images()
    want = singles("all", "delta", imgs)
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, "delta", imgs, _stride(want))
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_OFF", "1")
        off = batch(ctx, "delta", imgs, _stride(want))
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_OFF")
    assert on[6] == len(imgs) - 2 and off[6] == 0
    assert (on[0], on[1], on[2], on[4]) == (off[0], off[1], off[2], off[4])
    check_against_singles(off, want, "route off")


def test_threshold(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    imgs = [synth.photo(128, 128, synth.SEED0 + 7500), synth.photo(5, 3277, synth.SEED0 + 7501), synth.photo(64, 64, synth.SEED0 + 7502),
            synth.photo(17, 241, synth.SEED0 + 7503)]
    assert [im.shape[0] * im.shape[1] for im in imgs] == [16384, 16385, 4096, 4097]
    want = singles("threshold", "delta", imgs)
    assert all(s[0] == 0 for s in want)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", imgs, stride)
        assert res[6] == 3
        check_against_singles(res, want, "16384 | 16385")
        res = batch(ctx, "delta", imgs[:2], stride)
        assert res[6] == 1
        check_against_singles(res, want[:2], "16384 | 16385")
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_MAX_PX", "4096")
        res = batch(ctx, "delta", imgs, stride)
        assert res[6] == 1
        check_against_singles(res, want, "4096 | 4097")
        res = batch(ctx, "delta", imgs[3:], stride)
        assert res[6] == 0
        check_against_singles(res, want[3:], "4097 alone")
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_MAX_PX")


@pytest.mark.parametrize("host_out", (False, True))
def test_capacity_is_one_frame_s(host_out):
    import cniic_amd
    imgs = all_images()[4:9] + further_images()     # 7 x 9 ... 127 x 129 and the further ones: all on the route
    want = singles("capacity", "delta", imgs)
    assert all(s[0] == 0 for s in want)
    by_len = sorted(range(len(imgs)), key=lambda f: -len(want[f][1]))
    big, second = by_len[0], by_len[1]
    stride = _round4(len(want[second][1])) + 4
    assert stride < len(want[big][1])
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, "delta", imgs, stride, host_out=host_out, poison=0xA5)
    assert launches == len(imgs) and rc == CAPACITY
    assert msg == "encode: stream is %d bytes, capacity %d" % (len(want[big][1]), stride)
    for f in range(len(imgs)):
        assert lens[f] == len(want[f][1]), f
        if f == big:
            assert rcs[f] == CAPACITY and bool((host[f * stride:(f + 1) * stride] == 0xA5).all())
        else:
            assert rcs[f] == 0 and streams[f] == want[f][1], f
            assert bool((host[f * stride + lens[f]:(f + 1) * stride] == 0xA5).all()), f     # nothing behind a stream's end


@pytest.mark.parametrize("host_out", (False, True))
def test_a_chunk_whose_frames_all_exceed_their_capacity(host_out):
    """every frame has a stream and none has the room: nothing is placed, no place timer is recorded, no byte is written"""
    import cniic_amd
    from cniic_amd import synth
    imgs = [synth.uniform(16, 16, synth.SEED0 + 7550), synth.photo(12, 9, synth.SEED0 + 7551), synth.uniform(7, 9, synth.SEED0 + 7552), np.full((4, 5, 3), 77, np.uint8)]
    want = singles("tiny", "delta", imgs)
    assert all(s[0] == 0 and len(s[1]) > 8 for s in want)
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, "delta", imgs, 8, host_out=host_out, poison=0xA5)
        assert ctx.kernel_time("delta_small_place")[1] == 0
    assert launches == len(imgs) and rc == CAPACITY and rcs == [CAPACITY] * len(imgs)
    assert lens == [len(s[1]) for s in want]
    assert msg == "encode: stream is %d bytes, capacity 8" % len(want[0][1])
    assert bool((host == 0xA5).all())


def test_many_frames_in_one_launch():
    import cniic_amd
    rng = np.random.default_rng(43)
    imgs = []
    for f in range(3000):
        w, h = int(rng.integers(8, 17)), int(rng.integers(8, 13))
        imgs.append((rng.integers(0, 32, (h, w, 3)) * 8).astype(np.uint8))
    stride = _round4(8 + 8 * 16 * 12 - 1 + (MAX_CODE_LEN * 16 * 12 + 7) // 8) + 4      # ds_stride's terms for 16 x 12
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, "delta", imgs, stride)
        assert launches == 3000 and rc == 0 and rcs == [0] * 3000
        with cniic_amd.Context(0) as ref:
            for f in range(0, 3000, 75):
                src, sdata, sst = ref.encode("delta", imgs[f])
                assert src == 0 and streams[f] == sdata, f


def test_host_output_gets_the_same_bytes():
    import cniic_amd
    imgs = all_images()
    want = singles("all", "delta", imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", imgs, _stride(want), host_out=True)
    assert res[6] == len(imgs) - 2
    check_against_singles(res, want, "host out")


def test_host_images_are_not_routed():
    import cniic_amd
    imgs = all_images()[:9]
    want = singles("all", "delta", all_images())[:9]
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", imgs, _stride(want), host_src=True, host_out=True)
    assert res[6] == 0
    check_against_singles(res, want, "host source")


def test_a_size_with_an_injected_scan_is_not_routed():
    import cniic_amd
    imgs = all_images()[:9]
    w, h = 100, 75
    assert SHAPES[7] == (w, h)
    p = np.random.default_rng(7).permutation(w * h)
    scan = (w, h, np.stack([p % w, p // w], 1).astype(np.uint32))
    want = singles("scan", "delta", imgs, scan=scan)
    builtin = singles("all", "delta", all_images())[:9]
    assert want[7][1] != builtin[7][1] and all(want[f][1] == builtin[f][1] for f in range(9) if f != 7)
    with cniic_amd.Context(0) as ctx:
        ctx.set_scan(*scan)
        res = batch(ctx, "delta", imgs, _stride(want))
        assert res[6] == 8
        check_against_singles(res, want, "injected scan")
        ctx.set_scan(w, h, None)
        res = batch(ctx, "delta", imgs, _stride(want))
        assert res[6] == 9
        check_against_singles(res, builtin, "scan taken back")


def test_the_forced_32_bit_route_is_not_routed():
    import cniic_amd
    from cniic_amd import _lib
    imgs = all_images()[:9]
    want = singles("all", "delta", all_images())[:9]
    with cniic_amd.Context(0) as ctx:
        ctx.set_opt(_lib.OPT_DELTA_ROUTE, 32)
        res = batch(ctx, "delta", imgs, _stride(want))
        assert res[6] == 0
        check_against_singles(res, want, "route 32")
        ctx.set_opt(_lib.OPT_DELTA_ROUTE, None)
        res = batch(ctx, "delta", imgs, _stride(want))
        assert res[6] == 9


@pytest.mark.parametrize("expr", ("hufman", "hilbert(rle)"))
def test_other_codecs_never_report_the_timer(expr):
    import cniic_amd
    imgs = all_images()[4:8]
    want = singles(expr, expr, imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, _stride(want))
        assert res[6] == 0
        from cniic_amd import _lib
        assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0     # not merely zero launches: no such stage
    for f, (src, sdata, sst, smsg) in enumerate(want):
        assert res[2][f] == src == 0 and res[4][f] == sdata, (expr, f)


def test_measure_batch_takes_the_route_for_its_small_frames():
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 7600 + i) for i, (w, h) in enumerate(sizes)]
    want = singles("measure", "delta", imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        rows_want = []
        for im, (rc, data, st, _) in zip(imgs, want):
            rc2, back = ctx.decode("delta", data)
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
        rc, rows, lens = ctx.measure_batch("delta", src, offs, ws, hs, out, stride, allow=FAILURES)
        launches = ctx.kernel_time(TIMER)[1]          # the encode's stage, readable after the decode
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == 5 and rc == 0
        host = out.cpu().numpy()
        for f in range(F):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f] and got["error"] == 0.0, (f, got, rows_want[f])
            assert rows[f]["lossless_mismatch"] == 0
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f
