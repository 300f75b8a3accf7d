"""cniic_codec_decode_batch and cniic_mse_batch at the limits of their chunking, against the oracle and exact references:
- the batched device decode runs in parts of 4096 frames (codec.cpp, kBatchRouteFrames): batches of 4096, 4097 and 8193 frames, with
  frames off the route, corrupted and flat on either side of each part's edge;
- batch frames have no third tables: codes of 19..32 bits are found by bisection; 33-bit codes and 2^20 leaves leave the route;
- device streams with a stride below a header's 8 bytes;
- a header that claims fewer pixels than the payload holds: nothing is written past w*h*3;
- cniic_mse_batch across its 65535-frame launches (gridDim.y), and per-frame sums above 2^32."""
import heapq

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import torch
    import cniic_amd
    torch.cuda.set_stream(torch.cuda.Stream())   # (a context does not share the NULL stream)
    c = cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _pack(streams, stride):
    buf = np.zeros(stride * len(streams) + 16, np.uint8)
    for f, s in enumerate(streams):
        buf[f * stride:f * stride + len(s)] = np.frombuffer(s, np.uint8)
    return buf


def _single(ctx, expr, data, cap):
    """cniic_codec_decode of one stream alone -> (rc, w, h, pixels or None)"""
    out = np.zeros(max(cap, 1), np.uint8)
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)   # (a pointer even for an empty stream)
    rc, w, h = ctx.decode_into(expr, raw, len(data), out, allow=tuple(range(-1, -10, -1)))
    return rc, w, h, (out[:w * h * 3].copy() if rc == 0 else None)


def _dev(a):
    import torch
    d = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return d


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _decode_and_check(ctx, expr, streams, stride, img_stride, dev_in, dev_out, sources=None, want_ok=None):
    """decode_batch of `streams`, then per frame: status == the single decode's, success exactly when the oracle succeeds, pixels ==
    the oracle's (and == sources[f] where given), the rest of the frame and a guard behind the last one untouched -> per-frame status"""
    import torch
    F = len(streams)
    lens = [len(s) for s in streams]
    buf = _pack(streams, stride)
    src = _dev(buf) if dev_in else buf
    out = torch.full((F * img_stride + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if dev_out else \
        np.full(F * img_stride + 64, SENTINEL, np.uint8)
    if dev_out:
        torch.cuda.synchronize()
    rc, ws, hs, rcs = ctx.decode_batch(expr, src, stride, lens, F, out, img_stride, allow=tuple(range(-1, -10, -1)))
    assert rc == next((r for r in rcs if r != 0), 0), (expr, rc)
    got = _host(out)
    expect = np.full_like(got, SENTINEL)
    cache = {}
    for f, s in enumerate(streams):
        if s not in cache:
            orc, oimg = O.decode(expr, s)
            cache[s] = (orc, oimg, _single(ctx, expr, s, img_stride))
        orc, oimg, (src1, sw, sh, spx) = cache[s]
        assert rcs[f] == src1, (expr, f, rcs[f], src1)
        ok = orc == 0 and oimg.size <= img_stride
        assert (rcs[f] == 0) == ok, (expr, f, rcs[f], orc)
        if want_ok is not None:
            assert ok == want_ok[f], (expr, f, "the test's own frame is not what it should be")
        if ok:
            assert (ws[f], hs[f]) == (oimg.shape[1], oimg.shape[0]) == (sw, sh), (expr, f)
            assert np.array_equal(spx, oimg.reshape(-1)), (expr, f, "single decode")
            expect[f * img_stride:f * img_stride + oimg.size] = oimg.reshape(-1)
            if sources is not None and sources[f] is not None:
                assert np.array_equal(oimg, sources[f]), (expr, f, "the source")
        else:   # (a failed frame may have written anything inside its own img_stride bytes)
            expect[f * img_stride:(f + 1) * img_stride] = got[f * img_stride:(f + 1) * img_stride]
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, (expr, "first difference at frame %d, byte %d" % divmod(int(bad[0]), img_stride))
    return rcs


# ------------------------------------------------------------------ route parts of 4096 frames
@pytest.mark.parametrize("expr", ("hufman", "cluster-colors(4)"))
def test_route_parts(ctx, expr, monkeypatch):
    from cniic_amd import synth
    P, w, h = 37, 12, 9
    imgs = [synth.photo(w, h, synth.SEED0 + 2000 + i) for i in range(P)]
    streams = [ctx.encode(expr, im)[1] for im in imgs]
    flat_img = np.full((h, w, 3), 77, np.uint8)
    flat = ctx.encode("hufman" if expr == "hufman" else "cluster-colors(1)", flat_img)[1]   # a one-leaf decoder
    cut = [s[:-2] for s in streams]                                                         # the payload two bytes short
    lossless = expr == "hufman"
    img_stride = w * h * 3 + 4
    for F, specials, dev in ((4096, (4095,), True), (4097, (4095, 4096), True), (4097, (4095, 4096), False),
                             (8193, (4095, 4096, 8192), True)):
        for rot in range(3):
            kinds = [("off", "corrupt", "flat")[(i + rot) % 3] for i in range(len(specials))]
            frames, srcs, ok, off = [], [], [], []
            for f in range(F):
                kind = dict(zip(specials, kinds)).get(f, "corrupt" if f % 97 == 13 else "off" if f % 89 == 5 else "")
                j = f % P
                if kind == "flat":
                    frames.append(flat); srcs.append(flat_img); ok.append(True)
                elif kind == "corrupt":
                    frames.append(cut[j]); srcs.append(None); ok.append(False)
                else:
                    frames.append(streams[j]); srcs.append(imgs[j] if lossless else None); ok.append(True)
                    if kind == "off":
                        off.append(f)
            monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", ",".join(map(str, off)))
            stride = max(len(s) for s in frames) + 3
            _decode_and_check(ctx, expr, frames, stride, img_stride, dev, dev, srcs, ok)


# ------------------------------------------------------------------ long codes: the bisection, and the route's limits
def heap_max_len(counts):
    """the longest code of a Huffman tree of `counts`, built with a binary heap (ties: the shallower subtree first)"""
    h = [(int(c), 0, i) for i, c in enumerate(counts)]
    heapq.heapify(h)
    i = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, i))
        i += 1
    return h[0][1]


def fib_image(L, rng):
    """L + 1 colours with Fibonacci counts 1, 1, 2, 3, ...: a longest code of exactly L bits, whatever the order ties are merged in
    (the pixels that fill the last row go to the largest count, which keeps that)"""
    c = [1, 1]
    while len(c) < L + 1:
        c.append(c[-1] + c[-2])
    w = 2048
    h = -(-sum(c) // w)
    c[-1] += w * h - sum(c)
    assert heap_max_len(c) == L
    cols = rng.choice(1 << 24, len(c), replace=False)
    keys = rng.permutation(np.repeat(cols, c))
    return np.ascontiguousarray(np.stack([keys >> 16, keys >> 8, keys], 1).reshape(h, w, 3) & 255, np.uint8)


def distinct_image(n, rng):
    """1024 x 1024 pixels of n distinct colours (n = 2^20: every pixel its own leaf; n = 2^20 - 1: one colour twice)"""
    keys = rng.choice(1 << 24, 1 << 20, replace=False)
    keys[n:] = keys[0]
    keys = rng.permutation(keys)
    assert np.unique(keys).size == n
    return np.ascontiguousarray(np.stack([keys >> 16, keys >> 8, keys], 1).reshape(1024, 1024, 3) & 255, np.uint8)


def test_long_codes_in_a_batch(ctx):
    import torch
    from cniic_amd import synth
    rng = np.random.default_rng(20261016)
    imgs = [synth.photo(160, 96, synth.SEED0 + 2100)]
    for L in (20, 25, 32, 33):   # 19..32: bisection on the route; 33: off the route
        imgs += [fib_image(L, rng), synth.photo(96, 64, synth.SEED0 + 2100 + L)]
    imgs += [distinct_image((1 << 20) - 1, rng), distinct_image(1 << 20, rng), np.full((5, 3, 3), 9, np.uint8)]
    streams = []
    for im in imgs:
        rc, s, _ = ctx.encode("hufman", im)
        assert rc == 0
        streams.append(s)
    F = len(imgs)
    img_stride = max(im.size for im in imgs)
    stride = max(len(s) for s in streams) + 5
    for dev_in, dev_out in ((True, True), (False, True), (True, False)):
        src = _dev(_pack(streams, stride)) if dev_in else _pack(streams, stride)
        out = torch.full((F * img_stride,), SENTINEL, dtype=torch.uint8, device="cuda") if dev_out else \
            np.full(F * img_stride, SENTINEL, np.uint8)
        if dev_out:
            torch.cuda.synchronize()
        rc, ws, hs, rcs = ctx.decode_batch("hufman", src, stride, [len(s) for s in streams], F, out, img_stride)
        assert rc == 0 and rcs == [0] * F
        out = out if dev_out else torch.from_numpy(out)
        for f, im in enumerate(imgs):
            assert (ws[f], hs[f]) == (im.shape[1], im.shape[0]), f
            frame = out[f * img_stride:(f + 1) * img_stride]
            want = torch.from_numpy(im.reshape(-1)).to(frame.device)
            assert torch.equal(frame[:im.size], want), (f, im.shape)
            assert bool((frame[im.size:] == SENTINEL).all()), f


# ------------------------------------------------------------------ strides below a header
@pytest.mark.parametrize("dev_out", (True, False))
def test_strides_below_a_header(ctx, dev_out):
    from cniic_amd import _lib, synth
    rng = np.random.default_rng(7)
    whole = ctx.encode("hufman", synth.photo(40, 30, synth.SEED0 + 2200))[1]
    for expr in ("hufman", "cluster-colors(16)"):
        for stride in range(0, 8):
            for dev_in in (True, False):
                F = 11
                lens = [int(x) for x in rng.integers(0, stride + 1, F)]
                lens[0], lens[-1] = stride, stride
                streams = [whole[:n] if f % 2 else rng.integers(0, 256, n, dtype=np.uint8).tobytes() for f, n in enumerate(lens)]
                rcs = _decode_and_check(ctx, expr, streams, stride, 40 * 30 * 3, dev_in, dev_out, want_ok=[False] * F)
                assert rcs == [_lib.DECODE] * F, (expr, stride, dev_in, rcs)


# ------------------------------------------------------------------ a payload with more symbols than the header asks for
@pytest.mark.parametrize("expr", ("hufman", "cluster-colors(64)"))
def test_trailing_symbols_are_not_written(ctx, expr):
    from cniic_amd import synth
    imgs = [synth.photo(64, 48, synth.SEED0 + 2300 + f) for f in range(6)]
    streams = []
    for f, im in enumerate(imgs):
        b = bytearray(ctx.encode(expr, im)[1])
        w, h = 64 - 3 * f if f % 2 == 0 else 64, 48 if f % 2 == 0 else 48 - 5 * f   # the header's w or h made smaller
        b[0:4], b[4:8] = w.to_bytes(4, "little"), h.to_bytes(4, "little")
        streams.append(bytes(b))
    streams.append(ctx.encode(expr, imgs[0])[1])
    for dev_in, dev_out in ((True, True), (False, True), (True, False), (False, False)):
        _decode_and_check(ctx, expr, streams, max(len(s) for s in streams), 64 * 48 * 3, dev_in, dev_out, want_ok=[True] * len(streams))


# ------------------------------------------------------------------ cniic_mse_batch
def sums_of_three_squares(n):
    """n distinct integers, each a^2 + b^2 + c^2 with 0 <= a, b, c <= 255 -> (values, (n, 3) array of a, b, c)"""
    sq = np.arange(256, dtype=np.int64) ** 2
    two = np.full(2 * 255 * 255 + 1, -1, np.int64)
    two[(sq[:, None] + sq[None, :]).ravel()] = np.arange(256 * 256)
    v = np.arange(3 * n + 64, dtype=np.int64)
    rep = np.full(v.size, -1, np.int64)
    for c in range(256):
        r = v - sq[c]
        hit = (rep < 0) & (r >= 0) & (r < two.size)
        hit[hit] = two[r[hit]] >= 0
        rep[hit] = two[r[hit]] * 256 + c
    vals = np.flatnonzero(rep >= 0)[:n]
    assert vals.size == n
    r = rep[vals]
    abc = np.stack([r >> 16, (r >> 8) & 255, r & 255], 1)
    assert np.array_equal((abc ** 2).sum(1), vals)
    return vals, abc.astype(np.uint8)


def exact_mse(a, b, npx, F):
    """sum of the integer squared differences of each pair / npx: Python's int / int is correctly rounded"""
    d = a.reshape(F, npx * 3).astype(np.int64) - b.reshape(F, npx * 3).astype(np.int64)
    return [int(s) / npx for s in (d * d).sum(1)]


@pytest.mark.parametrize("npx", (1, 5))
def test_mse_batch_across_the_grid_split(ctx, npx):
    rng = np.random.default_rng(npx)
    vals, abc = sums_of_three_squares(65537)
    for F in (65535, 65536, 65537):
        a = rng.integers(0, 256, (F, npx, 3), dtype=np.uint8)
        b = a.copy()
        p = np.arange(F) % npx                           # frame f differs in one pixel only, by a sum of squares of its own
        a[np.arange(F), p] = 0
        b[np.arange(F), p] = abc[:F]
        want = exact_mse(a, b, npx, F)
        assert want == [float(v) / npx for v in vals[:F]] and len(set(want)) == F
        got = ctx.mse_batch(a, b, npx, F)
        bad = [f for f in range(F) if got[f] != want[f]]
        assert not bad, (F, npx, bad[:5], [(got[f], want[f]) for f in bad[:5]])
        for f in (0, 1, 65534, 65535, 65536):
            if f < F:
                assert got[f] == pytest.approx(O.mse(a[f], b[f]), rel=1e-12, abs=0)


def test_mse_sums_above_2_to_the_32(ctx):
    npx, F = 1 << 22, 3
    a = np.zeros((F, npx, 3), np.uint8)
    b = np.full((F, npx, 3), 255, np.uint8)
    b[1, 7] = 0                                       # one pixel less in the middle frame
    want = exact_mse(a, b, npx, F)
    assert int(want[0] * npx) == 3 * 255 * 255 * npx > (1 << 32)
    assert want == [195075.0, (195075 * npx - 195075) / npx, 195075.0]
    for a_dev, b_dev in ((False, False), (True, True), (True, False), (False, True)):
        got = ctx.mse_batch(_dev(a.reshape(-1)) if a_dev else a, _dev(b.reshape(-1)) if b_dev else b, npx, F)
        assert got == want, (a_dev, b_dev)
    for f in range(F):
        assert ctx.mse(a[f], b[f]) == want[f]
        assert want[f] == pytest.approx(O.mse(a[f], b[f]), rel=1e-12, abs=0)


@pytest.mark.parametrize("a_dev,b_dev", ((False, False), (True, True), (True, False), (False, True)))
def test_mse_batch_residency(ctx, a_dev, b_dev):
    rng = np.random.default_rng(3)
    for npx, F in ((1, 1), (3, 7), (1000, 5), (160 * 96, 3)):
        a = rng.integers(0, 256, (F, npx * 3), dtype=np.uint8)
        b = rng.integers(0, 256, (F, npx * 3), dtype=np.uint8)
        want = exact_mse(a, b, npx, F)
        got = ctx.mse_batch(_dev(a.reshape(-1)) if a_dev else a, _dev(b.reshape(-1)) if b_dev else b, npx, F)
        assert got == want, (npx, F)
        for f in range(F):
            assert got[f] == pytest.approx(O.mse(a[f], b[f]), rel=1e-12, abs=0)
