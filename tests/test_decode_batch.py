"""cniic_codec_decode_batch / cniic_mse_batch: the decode and error halves of the reference's many-image loop (bench.rs:24-59,
measure_all) in one call each.  Every frame of a batch must come out exactly as cniic_codec_decode gives it for that stream alone --
pixels, dimensions and status -- whichever route it took: the batched device decode of `hufman` / `cluster-colors`, or the worker
contexts for the other codecs and for the frames that route leaves alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 160, 96
CODECS = ("hufman", "cluster-colors(16)", "cluster-colors(256)", "delta", "hilbert(rle)", "voronoi(8)")
LOSSLESS = ("hufman", "delta", "hilbert(rle)")


def _frames(w=W, h=H, n=11, seed=0):
    from cniic_amd import synth
    fr = [synth.photo(w, h, synth.SEED0 + 500 + seed + f) for f in range(n)]
    fr.append(np.full((h, w, 3), 77, np.uint8))           # flat: a one-leaf decoder (zero-length codes)
    fr.append(synth.uniform(w, h, synth.SEED0 + 900 + seed))  # noise
    return np.stack(fr)


def _pack(streams, stride):
    buf = np.zeros(stride * len(streams), np.uint8)
    for f, s in enumerate(streams):
        buf[f * stride:f * stride + len(s)] = np.frombuffer(s, np.uint8)
    return buf


def _single(ctx, expr, data, img_stride):
    """cniic_codec_decode of one stream alone -> (rc, w, h, pixels or None)"""
    from cniic_amd import _lib
    out = np.zeros(max(img_stride, 1), np.uint8)
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)   # (a pointer even for an empty stream)
    rc, w, h = ctx.decode_into(expr, raw, len(data), out, allow=(_lib.DECODE, _lib.CAPACITY))
    return rc, w, h, (out[:w * h * 3].copy() if rc == 0 else None)


def _check(ctx, expr, streams, res, out, img_stride, singles, sources=None):
    rc, ws, hs, rcs = res
    host = out.cpu().numpy() if hasattr(out, "cpu") else out
    for f in range(len(streams)):
        src, sw, sh, spx = singles[f]
        assert rcs[f] == src, (expr, f, rcs[f], src)
        if src == 0:
            assert (ws[f], hs[f]) == (sw, sh), (expr, f)
            got = host[f * img_stride:f * img_stride + sw * sh * 3]
            assert np.array_equal(got, spx), (expr, f)
            if sources is not None and sources[f] is not None:
                assert np.array_equal(got, sources[f].reshape(-1)), (expr, f)
    assert rc == next((r for r in rcs if r != 0), 0)


@pytest.mark.parametrize("expr", CODECS)
def test_decode_batch_equals_single_decodes(expr):
    import torch
    import cniic_amd
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    frames = _frames()
    F = len(frames)
    with cniic_amd.Context(0) as ctx:
        stride = W * H * 16 + 4096
        enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        fr_d = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize()
        _, lens, erc, _ = ctx.encode_batch(expr, fr_d, W, H, F, enc, stride, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
        lens = [lens[f] if erc[f] == 0 else 0 for f in range(F)]   # (a frame that did not encode: an empty stream, a decode failure)
        eh = enc.cpu().numpy()
        streams = [eh[f * stride:f * stride + lens[f]].tobytes() for f in range(F)]
        img_stride = W * H * 3
        singles = [_single(ctx, expr, s, img_stride) for s in streams]
        assert sum(s[0] == 0 for s in singles) >= F - 1
        sources = [frames[f] if expr in LOSSLESS and erc[f] == 0 else None for f in range(F)]
        # device buffers, with 1 and 8 worker streams
        for streams_opt in (None, 1, 8):
            ctx.set_opt(_lib.OPT_BATCH_STREAMS, streams_opt)
            out = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            res = ctx.decode_batch(expr, enc, stride, lens, F, out, img_stride, allow=(_lib.DECODE,))
            _check(ctx, expr, streams, res, out, img_stride, singles, sources)
        ctx.set_opt(_lib.OPT_BATCH_STREAMS, None)
        # host buffers
        hout = np.zeros(img_stride * F, np.uint8)
        res = ctx.decode_batch(expr, _pack(streams, stride), stride, lens, F, hout, img_stride, allow=(_lib.DECODE,))
        _check(ctx, expr, streams, res, hout, img_stride, singles, sources)
        # strides that are not multiples of 4, on both sides (device)
        odd, odd_img = max(lens) + 5, img_stride + 1
        enc_odd = torch.from_numpy(_pack(streams, odd)).to(dev)
        out = torch.zeros(odd_img * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        res = ctx.decode_batch(expr, enc_odd, odd, lens, F, out, odd_img, allow=(_lib.DECODE,))
        _check(ctx, expr, streams, res, out, odd_img, singles, sources)
        # ... and from host memory into a host image
        hout = np.zeros(odd_img * F, np.uint8)
        res = ctx.decode_batch(expr, _pack(streams, odd), odd, lens, F, hout, odd_img, allow=(_lib.DECODE,))
        _check(ctx, expr, streams, res, hout, odd_img, singles, sources)
        assert ctx.decode_batch(expr, enc, stride, [], 0, out, img_stride) == (0, [], [], [])


def test_decode_batch_route_launches_do_not_grow_with_frames():
    """the `hufman` frames are decoded by one set of launches: the batched pass kernel runs as often for 64 frames as for 8"""
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    w = h = 256
    counts = []
    with cniic_amd.Context(0) as ctx:
        for F in (8, 64):
            frames = np.stack([synth.photo(w, h, synth.SEED0 + 700 + f) for f in range(F)])
            stride = w * h * 16 + 4096
            enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
            fr_d = torch.from_numpy(frames).to(dev)
            torch.cuda.synchronize()
            rc, lens, _, _ = ctx.encode_batch("hufman", fr_d, w, h, F, enc, stride)
            assert rc == 0
            out = torch.zeros(w * h * 3 * F, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            rc, ws, hs, rcs = ctx.decode_batch("hufman", enc, stride, lens, F, out, w * h * 3)
            counts.append(ctx.kernel_time("decode_batch_pass")[1])
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            assert rc == 0 and ws == [w] * F and hs == [h] * F
            assert np.array_equal(out.cpu().numpy(), frames.reshape(-1))
    assert counts[0] > 0 and counts[0] == counts[1], counts


def test_decode_batch_failures_stay_per_frame():
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    w, h = 64, 48
    with cniic_amd.Context(0) as ctx:
        frames = [synth.photo(w, h, synth.SEED0 + 800 + f) for f in range(7)]
        frames[5] = synth.photo(128, 96, synth.SEED0 + 899)           # larger than img_stride
        streams = [ctx.encode("hufman", im)[1] for im in frames]
        lens = [len(s) for s in streams]
        stride = max(lens) + 16
        buf = _pack(streams, stride)
        lens[1] = lens[1] - 100                                         # the payload cut short
        lens[2] = lens[2] // 2                                          # cut in half
        buf[3 * stride + 20:3 * stride + 60] = 0xA5                     # bytes overwritten inside the decoder
        F, img_stride = len(frames), w * h * 3
        singles = [_single(ctx, "hufman", buf[f * stride:f * stride + lens[f]].tobytes(), img_stride) for f in range(F)]
        assert singles[1][0] == _lib.DECODE and singles[5][0] == _lib.CAPACITY
        sources = [frames[f] if f not in (1, 2, 3, 5) else None for f in range(F)]
        streams_cut = [buf[f * stride:f * stride + lens[f]].tobytes() for f in range(F)]
        for on_dev in (True, False):
            src = torch.from_numpy(buf).to(dev) if on_dev else buf
            out = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev) if on_dev else np.zeros(img_stride * F, np.uint8)
            if on_dev:
                torch.cuda.synchronize()
            res = ctx.decode_batch("hufman", src, stride, lens, F, out, img_stride, allow=(_lib.DECODE, _lib.CAPACITY))
            _check(ctx, "hufman", streams_cut, res, out, img_stride, singles, sources)
            assert res[0] == singles[1][0]
            assert res[3][0] == 0 and res[3][4] == 0 and res[3][6] == 0


def test_decode_batch_fallbacks(monkeypatch):
    """a decoder the host does not parse (the GPU trie parse of a single decode) and a frame sent off the route by the test knob"""
    import torch
    import cniic_amd
    from cniic_amd import synth
    dev = torch.device("cuda", 0)
    imgs = [synth.photo(64, 48, synth.SEED0 + 810), synth.uniform(1024, 1024, synth.SEED0 + 811), synth.photo(200, 120, synth.SEED0 + 812),
            synth.photo(96, 64, synth.SEED0 + 813)]
    monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", "2")
    with cniic_amd.Context(0) as ctx:
        streams = [ctx.encode("hufman", im)[1] for im in imgs]
        lens = [len(s) for s in streams]
        stride = max(lens) + 3
        F, img_stride = len(imgs), 1024 * 1024 * 3
        singles = [_single(ctx, "hufman", s, img_stride) for s in streams]
        for on_dev in (True, False):
            buf = _pack(streams, stride)
            src = torch.from_numpy(buf).to(dev) if on_dev else buf
            out = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev) if on_dev else np.zeros(img_stride * F, np.uint8)
            if on_dev:
                torch.cuda.synchronize()
            res = ctx.decode_batch("hufman", src, stride, lens, F, out, img_stride)
            _check(ctx, "hufman", streams, res, out, img_stride, singles, imgs)


@pytest.mark.parametrize("expr", ("hufman", "cluster-colors(16)", "delta", "hilbert(rle)"))
def test_decode_batch_mixed_sizes(expr):
    import torch
    import cniic_amd
    from cniic_amd import synth
    dev = torch.device("cuda", 0)
    sizes = [(160, 96), (37, 29), (256, 130), (160, 96), (37, 29), (256, 130)]
    imgs = [synth.photo(w, h, synth.SEED0 + 820 + i) for i, (w, h) in enumerate(sizes)]
    with cniic_amd.Context(0) as ctx:
        streams = [ctx.encode(expr, im)[1] for im in imgs]
        lens = [len(s) for s in streams]
        stride = max(lens) + 1
        F, img_stride = len(imgs), 256 * 130 * 3
        singles = [_single(ctx, expr, s, img_stride) for s in streams]
        src = torch.from_numpy(_pack(streams, stride)).to(dev)
        out = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        res = ctx.decode_batch(expr, src, stride, lens, F, out, img_stride)
        _check(ctx, expr, streams, res, out, img_stride, singles, imgs if expr in LOSSLESS else None)


def test_decode_batch_follows_the_injected_scan():
    import cniic_amd
    from cniic_amd import _lib, synth
    w, h, F = 64, 64, 5
    p = np.random.default_rng(11).permutation(w * h)
    s = np.stack([p % w, p // w], 1).astype(np.uint32)
    imgs = [synth.photo(w, h, synth.SEED0 + 840 + f) for f in range(F)]
    with cniic_amd.Context(0) as ctx:
        ctx.set_scan(w, h, s)
        for expr in ("delta", "hilbert(rle)"):
            streams = [ctx.encode(expr, im)[1] for im in imgs]
            lens = [len(x) for x in streams]
            stride = max(lens)
            singles = [_single(ctx, expr, x, w * h * 3) for x in streams]
            out = np.zeros(w * h * 3 * F, np.uint8)
            res = ctx.decode_batch(expr, _pack(streams, stride), stride, lens, F, out, w * h * 3)
            _check(ctx, expr, streams, res, out, w * h * 3, singles, imgs)
        ctx.set_scan(w, h, None)
        # without it the same streams follow the built-in order, in a batch as alone
        singles = [_single(ctx, expr, x, w * h * 3) for x in streams]
        out = np.zeros(w * h * 3 * F, np.uint8)
        res = ctx.decode_batch(expr, _pack(streams, stride), stride, lens, F, out, w * h * 3, allow=(_lib.DECODE,))
        _check(ctx, expr, streams, res, out, w * h * 3, singles)
        assert singles[0][0] != 0 or not np.array_equal(singles[0][3], imgs[0].reshape(-1))


def test_decode_batch_full_size_cluster_colors_256():
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    w, h, F = 1920, 1080, 128
    with cniic_amd.Context(0) as ctx:
        fr_d = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
        for f in range(F):
            ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 1000 + f, w, h, fr_d[f])
        stride = w * h * 2 + (1 << 16)
        enc = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rc, lens, _, _ = ctx.encode_batch("cluster-colors(256)", fr_d, w, h, F, enc, stride)
        assert rc == 0
        img_stride = w * h * 3
        out = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rc, ws, hs, rcs = ctx.decode_batch("cluster-colors(256)", enc, stride, lens, F, out, img_stride)
        assert rc == 0 and ws == [w] * F and hs == [h] * F and rcs == [0] * F
        one = torch.zeros(img_stride, dtype=torch.uint8, device=dev)
        for f in range(F):
            assert ctx.decode_into("cluster-colors(256)", enc[f * stride:], lens[f], one) == (0, w, h)
            ctx.sync()
            assert torch.equal(one, out[f * img_stride:(f + 1) * img_stride]), f
        src = fr_d.reshape(-1)
        mb = ctx.mse_batch(src, out, w * h, F)
        single = [ctx.mse(fr_d[f].cpu().numpy(), out[f * img_stride:(f + 1) * img_stride].cpu().numpy()) for f in range(F)]
        assert mb == single


def test_mse_batch_bit_equal_to_mse():
    import cniic_amd
    rng = np.random.default_rng(5)
    with cniic_amd.Context(0) as ctx:
        for npx, F in ((1, 3), (777, 9), (160 * 96, 4), (1 << 18, 2)):
            a = rng.integers(0, 256, (F, npx * 3), dtype=np.uint8)
            b = rng.integers(0, 256, (F, npx * 3), dtype=np.uint8)
            b[0] = a[0]                                             # an identical pair
            got = ctx.mse_batch(a, b, npx, F)
            assert got == [ctx.mse(a[f], b[f]) for f in range(F)]
            assert got[0] == 0.0
        assert ctx.mse_batch(a, b, 0, F) == [0.0] * F
        assert ctx.mse_batch(a, b, npx, 0) == []


def test_fuzz_decode_batch():
    """a few seconds of tests/fuzz_decode_batch.py: random batches (codecs, sizes, corruptions, strides, host / device buffers, route
    knobs) frame by frame against the oracle and the single decode, with nothing written past a frame (CNIIC_FUZZ_SECONDS for longer)"""
    import os
    import torch
    import cniic_amd
    import fuzz_decode_batch
    torch.cuda.set_stream(torch.cuda.Stream())   # (a context does not share the NULL stream)
    with cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream) as ctx:
        assert fuzz_decode_batch.run(ctx, float(os.environ.get("CNIIC_FUZZ_SECONDS", "6"))) > 0
