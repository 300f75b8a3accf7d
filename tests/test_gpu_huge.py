"""Images of 2^31 pixels and more, up to the C ABI's limit of w h = 2^32 - 1: where a 32-bit pixel index, byte offset, bit offset, count
or frame offset would wrap.  A wrapped offset gives wrong bytes without a fault, so the streams are compared with the oracle's
(tests/golden/huge_digests.json, made by tests/golden/make_huge_digests.py) where the CPU can encode the image, and with exact
properties (round trips, histogram sizes, torch restatements) at 2^32 - 1 pixels, where it cannot.

Everything stays on the device: images are drawn there (cniic_synth_image, tests/huge_gen.py in torch), decoded with decode_into,
and hashed or compared 1 GiB at a time.  Each test first asks the device for the memory it needs and skips, saying so, only when
the device really lacks it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import huge_gen as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x636E696963
GB = 1 << 30
W32, H32 = 65535, 65537                   # 2^32 - 1 pixels
N32 = W32 * H32


def golden(case):
    with open(os.path.join(HERE, "golden", "huge_digests.json")) as f:
        g = json.load(f)["cases"].get(case)
    if g is None:
        pytest.skip("tests/golden/huge_digests.json has no case %r yet" % case)
    return g


@pytest.fixture(scope="module")
def env():
    import torch

    import cniic_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    ctx = cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield ctx, torch, dev
    ctx.close()


@pytest.fixture(autouse=True)
def _release(env):
    yield
    env[1].cuda.synchronize()
    env[1].cuda.empty_cache()


def need(torch, nbytes):
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("needs %.1f GB of device memory, %.1f GB free of %.1f GB" % (nbytes / 1e9, free / 1e9, total / 1e9))


def photo(ctx, torch, dev, seed, w, h):
    img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    ctx.synth_image(1, seed, w, h, out=img)
    return img


def drawn(torch, dev, kind, w, h, band=2048):
    """tests/huge_gen.py's image of this kind, drawn on the device band by band"""
    img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    for y0 in range(0, h, band):
        y1 = min(h, y0 + band)
        img[y0:y1] = G.fib_rows(torch, y0, y1, device=dev) if kind == "fib" else G.tiles_rows(torch, w, y0, y1, kind, device=dev)
    return img


def golden_image(ctx, torch, dev, g):
    if g["image"] == "photo":
        return photo(ctx, torch, dev, SEED + g["seed_offset"], g["w"], g["h"])
    return drawn(torch, dev, g["image"], g["w"], g["h"])


def sha(t, n=None):
    return G.sha256_chunked(t, n)


def encode(ctx, torch, dev, expr, img, w, h, cap):
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n, st = ctx.encode(expr, img, w=w, h=h, out=out)
    assert rc == 0
    return out, n, st


def decode(ctx, torch, dev, expr, stream, n, npx):
    back = torch.empty(npx * 3, dtype=torch.uint8, device=dev)
    rc, w, h = ctx.decode_into(expr, stream, n, back)
    assert rc == 0 and w * h == npx
    return back


# ---------------------------------------------------------------- 1. delta at 46341^2 against the oracle
@pytest.mark.parametrize("route", ["default", "route32", "gather_any"])
def test_delta_46341_equals_the_oracle(env, monkeypatch, route):
    """`delta` on the 46341^2 photo (2^31 + 4697 pixels, about 3.9 GB of stream): the oracle's bytes on the 16-bit route, on the
    32-bit symbol route (a symbol buffer of 8.6 GB) and with the per-position gather; the stream's length is what its histogram
    predicts, and it decodes on the device to the source"""
    ctx, torch, dev = env
    from cniic_amd import _lib
    g = golden("d46k")
    w, h = g["w"], g["h"]
    npx = w * h
    need(torch, npx * (3 + 3 + 3 + 4) + 4 * GB)
    if route == "route32":
        ctx.set_opt(_lib.OPT_DELTA_ROUTE, 32)
    if route == "gather_any":
        monkeypatch.setenv("CNIIC_DELTA_GATHER", "any")
    try:
        img = golden_image(ctx, torch, dev, g)
        out, n, _ = encode(ctx, torch, dev, "delta", img, w, h, npx * 3 + (1 << 24))
    finally:
        ctx.set_opt(_lib.OPT_DELTA_ROUTE, None)
    assert n == g["length"]
    assert sha(out, n) == g["sha256"]
    if route != "default":
        return
    assert sha(img) == g["image_sha256"], "device generator != numpy generator"
    keys, counts, _ = ctx.hilbert_delta_hist(img, w=w, h=h)
    assert int(counts.sum()) == npx and ctx.huf_size(_lib.SYM_SIGNED, counts) + 8 == n
    back = decode(ctx, torch, dev, "delta", out, n, npx)
    assert G.equal_chunked(back, img)


# ---------------------------------------------------------------- 2. delta at 2^32 - 1 pixels, by properties
def test_delta_at_2_to_the_32_minus_1(env):
    """`delta` on a 65535 x 65537 photo, the largest image the C ABI takes: the device round trip, the length the histogram predicts,
    the scan at 10^5 sampled positions and both ends against the oracle's random-access d -> (x, y), and a 65536-symbol window of the
    delta symbols on each side of 2^31 and at the very end against the differences recomputed with torch"""
    import oracle_lib as O
    ctx, torch, dev = env
    from cniic_amd import _lib
    need(torch, N32 * (3 + 3 + 3) + 4 * GB)
    img = photo(ctx, torch, dev, SEED + 7, W32, H32)
    out, n, _ = encode(ctx, torch, dev, "delta", img, W32, H32, N32 * 3 + (1 << 24))
    keys, counts, _ = ctx.hilbert_delta_hist(img, w=W32, h=H32)
    assert int(counts.sum()) == N32 and ctx.huf_size(_lib.SYM_SIGNED, counts) + 8 == n
    back = decode(ctx, torch, dev, "delta", out, n, N32)
    del out
    assert G.equal_chunked(back, img)
    del back
    torch.cuda.empty_cache()

    need(torch, N32 * (3 + 4) + 2 * GB)
    lin = torch.empty(N32 * 3, dtype=torch.uint8, device=dev)
    assert ctx._L.cniic_hilbert_linearize(ctx.h, C.c_void_p(img.data_ptr()), C.c_uint32(W32), C.c_uint32(H32), C.c_void_p(lin.data_ptr())) == 0
    rng = np.random.default_rng(7)
    ds = np.concatenate([[0, 1, (1 << 31) - 1, 1 << 31, N32 - 2, N32 - 1], rng.integers(0, N32, 100000, dtype=np.int64)])
    xy = np.array([O.hilbert_d2xy(W32, H32, int(d)) for d in ds], np.int64)
    at = torch.from_numpy(xy[:, 1] * W32 + xy[:, 0]).to(dev)
    src = img.reshape(-1, 3).index_select(0, at)
    got = lin.reshape(-1, 3).index_select(0, torch.from_numpy(ds).to(dev))
    assert torch.equal(src, got)

    syms = torch.empty(N32, dtype=torch.int32, device=dev)
    nu = C.c_uint64(0)
    k2 = np.empty(keys.size, np.uint32)
    c2 = np.empty(keys.size, np.uint64)
    assert ctx._L.cniic_hilbert_delta_hist(ctx.h, C.c_void_p(img.data_ptr()), C.c_uint32(W32), C.c_uint32(H32), C.c_void_p(k2.ctypes.data),
                                           C.c_void_p(c2.ctypes.data), C.c_uint64(k2.size), C.byref(nu), C.c_void_p(syms.data_ptr())) == 0
    assert np.array_equal(k2[:nu.value], keys) and np.array_equal(c2[:nu.value], counts)
    for d0 in (0, (1 << 31) - 65536, (1 << 31) - 32768, 1 << 31, N32 - 65536):
        cur = lin[3 * d0:3 * (d0 + 65536)].reshape(-1, 3).to(torch.int64)
        prev = torch.cat([torch.zeros((1, 3), dtype=torch.int64, device=dev) if d0 == 0 else lin[3 * (d0 - 1):3 * d0].reshape(1, 3).to(torch.int64),
                          cur[:-1]])
        dd = cur - prev + 255
        want = (dd[:, 0] << 18) | (dd[:, 1] << 9) | dd[:, 2]
        assert torch.equal(syms[d0:d0 + 65536].to(torch.int64), want), d0


# ---------------------------------------------------------------- 3. hilbert(rle) and hilbert(rle(4)) at 46341^2
def test_hilbert_rle_46341_equals_the_oracle(env):
    """the exact run-length codec on 46341^2 tiles: the oracle's stream, and the device decode gives the source back"""
    ctx, torch, dev = env
    g = golden("r46k")
    npx = g["w"] * g["h"]
    need(torch, npx * 6 + g["length"] + 4 * GB)
    img = golden_image(ctx, torch, dev, g)
    assert sha(img) == g["image_sha256"], "device generator != numpy generator"
    out, n, _ = encode(ctx, torch, dev, "hilbert(rle)", img, g["w"], g["h"], g["length"] + (1 << 20))
    assert n == g["length"] and sha(out, n) == g["sha256"]
    assert G.equal_chunked(decode(ctx, torch, dev, "hilbert(rle)", out, n, npx), img)


def test_hilbert_rle_approx_46341_equals_the_oracle(env):
    """hilbert(rle(4)) on 46341^2 tiles with a +-2 ripple: tests/rle_approx_ref.c's stream on the oracle's scan, and the image the
    oracle's decoder makes of it, decoded single and batched"""
    ctx, torch, dev = env
    g = golden("ra46k")
    w, h = g["w"], g["h"]
    npx = w * h
    need(torch, npx * 6 + g["length"] + 4 * GB)
    img = golden_image(ctx, torch, dev, g)
    out = torch.empty(g["length"] + (1 << 20), dtype=torch.uint8, device=dev)
    rc, n = ctx.hilbert_rle_approx_encode(4.0, img, w, h, out=out)
    assert rc == 0 and n == g["length"] and sha(out, n) == g["sha256"]
    del img
    back = decode(ctx, torch, dev, "hilbert(rle)", out, n, npx)
    assert sha(back) == g["decoded_sha256"]
    back.fill_(0)
    rc, ws, hs, rcs = ctx.decode_batch("hilbert(rle)", out, out.numel(), [n], 1, back, npx * 3)
    assert rc == 0 and (ws, hs, rcs) == ([w], [h], [0])
    assert sha(back) == g["decoded_sha256"]


# ---------------------------------------------------------------- 4. Huffman codes of up to 44 bits over 2.97 G symbols
@pytest.mark.parametrize("knobs", [{}, {"CNIIC_GPU_DECODE_MIN": "0", "CNIIC_HD_LUT3": "0"}, {"CNIIC_GPU_DECODE_MIN": "0", "CNIIC_HD_KEEP": "1"}],
                         ids=["default", "no_lut3", "keep"])
def test_hufman_fibonacci_counts(env, monkeypatch, knobs):
    """45 colours with Fibonacci counts F(1..45) over 46368 x 64079 = 2 971 215 072 pixels: codes of up to 44 bits.  The oracle's
    stream, and the device decode gives the source back through the decoder's tables of 34- to 44-bit codes"""
    ctx, torch, dev = env
    from cniic_amd import _lib
    g = golden("fib")
    npx = g["w"] * g["h"]
    assert g["longest_code"] == 44
    need(torch, npx * 6 + g["length"] + 4 * GB)
    img = golden_image(ctx, torch, dev, g)
    out, n, _ = encode(ctx, torch, dev, "hufman", img, g["w"], g["h"], g["length"] + (1 << 24))
    assert n == g["length"] and sha(out, n) == g["sha256"]
    assert ctx.huf_size(_lib.SYM_RGB, np.array(G.fib_counts(), np.uint64)) + 8 == n
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    assert G.equal_chunked(decode(ctx, torch, dev, "hufman", out, n, npx), img)


# ---------------------------------------------------------------- 5. cluster-colors(256) at 46341^2
@pytest.mark.parametrize("route", ["persistent", "launches", "dense"])
def test_cluster_colors_46341_equals_the_oracle(env, route):
    """cluster-colors(256) on 46341^2 tiles, one background colour over 55 % of the pixels (a count of 1.18 G): the oracle's stream and
    iteration count with the persistent K-means loop, with one launch per iteration and with the dense table instead of the
    super-cell partition; the decoded image is the oracle's"""
    ctx, torch, dev = env
    from cniic_amd import _lib
    g = golden("cc46k")
    w, h = g["w"], g["h"]
    npx = w * h
    need(torch, npx * (3 + 2 + 3) + 8 * GB)
    img = golden_image(ctx, torch, dev, g)
    if route == "launches":
        ctx.set_opt(_lib.OPT_KM_LOOP, 1)
    if route == "dense":
        ctx.set_opt(_lib.OPT_SP_MIN_PIXELS, npx + 1)
    try:
        out, n, st = encode(ctx, torch, dev, g["codec"], img, w, h, npx * 2 + (1 << 24))
    finally:
        ctx.set_opt(_lib.OPT_KM_LOOP, None)
        ctx.set_opt(_lib.OPT_SP_MIN_PIXELS, None)
    assert n == g["length"] and st["iterations"] == g["iterations"]
    assert sha(out, n) == g["sha256"]
    if route == "persistent":
        del img
        assert sha(decode(ctx, torch, dev, g["codec"], out, n, npx)) == g["decoded_sha256"]


# ---------------------------------------------------------------- 6. cluster-colors(2) with a colour count above 2^31
def test_cluster_colors_2_at_2_to_the_32_minus_1(env):
    """two colours in a 3:1 split over 2^32 - 1 pixels (3 221 225 472 of one): exact histogram counts, a lossless round trip, and the
    length the histogram predicts"""
    ctx, torch, dev = env
    from cniic_amd import _lib
    need(torch, N32 * 6 + N32 + 4 * GB)
    a, b = (23, 140, 201), (250, 7, 66)
    img = torch.empty((N32, 3), dtype=torch.uint8, device=dev)
    img[:] = torch.tensor(a, dtype=torch.uint8, device=dev)
    img[3::4] = torch.tensor(b, dtype=torch.uint8, device=dev)
    nb = N32 // 4
    keys, counts = ctx.hist_rgb24(img, npx=N32)
    ka, kb = (a[0] << 16) | (a[1] << 8) | a[2], (b[0] << 16) | (b[1] << 8) | b[2]
    assert keys.tolist() == [ka, kb] and counts.tolist() == [N32 - nb, nb] and N32 - nb > (1 << 31)
    out, n, _ = encode(ctx, torch, dev, "cluster-colors(2)", img, W32, H32, N32 + (1 << 24))
    assert n == ctx.huf_size(_lib.SYM_RGB, counts) + 8
    assert G.equal_chunked(decode(ctx, torch, dev, "cluster-colors(2)", out, n, N32), img)


# ---------------------------------------------------------------- 7. hist_rgb24 at 2^32 - 1 pixels
def _bincount(torch, flat, npx, chunk=1 << 28):
    tot = None
    for p0 in range(0, npx, chunk):
        px = flat[3 * p0:3 * min(npx, p0 + chunk)].reshape(-1, 3).to(torch.int64)
        c = torch.bincount((px[:, 0] << 16) | (px[:, 1] << 8) | px[:, 2], minlength=1 << 24)
        tot = c if tot is None else tot + c
    keys = torch.nonzero(tot).reshape(-1)
    return keys.cpu().numpy(), tot[keys].cpu().numpy()


def test_hist_rgb24_at_2_to_the_32_minus_1(env):
    """one colour over 2^32 - 1 pixels: one key with count 4 294 967 295; on the photo, keys and counts equal a chunked int64
    torch.bincount, with the image at an aligned and at an odd device address (the byte-wise route)"""
    ctx, torch, dev = env
    need(torch, N32 * 6 + 4 * GB)
    one = torch.full((N32 * 3,), 77, dtype=torch.uint8, device=dev)
    keys, counts = ctx.hist_rgb24(one, npx=N32)
    assert keys.tolist() == [(77 << 16) | (77 << 8) | 77] and counts.tolist() == [N32]
    del one
    img = photo(ctx, torch, dev, SEED + 7, W32, H32).reshape(-1)
    wk, wc = _bincount(torch, img, N32)
    keys, counts = ctx.hist_rgb24(img, npx=N32)
    assert np.array_equal(keys.astype(np.int64), wk) and np.array_equal(counts.astype(np.int64), wc)
    odd = torch.empty(N32 * 3 + 1, dtype=torch.uint8, device=dev)
    odd[1:].copy_(img)
    del img
    view = odd[1:]
    assert view.data_ptr() % 2 == 1
    keys, counts = ctx.hist_rgb24(view, npx=N32)
    assert np.array_equal(keys.astype(np.int64), wk) and np.array_equal(counts.astype(np.int64), wc)


# ---------------------------------------------------------------- 8. MSE at 2^32 - 1 pixels
def _sq_sum(torch, a, b, chunk=1 << 30):
    s = 0
    for at in range(0, a.numel(), chunk):
        d = a[at:at + chunk].to(torch.int32) - b[at:at + chunk].to(torch.int32)
        s += int((d * d).sum(dtype=torch.int64))
    return s


def test_mse_at_2_to_the_32_minus_1(env):
    """cniic_mse over 2^32 - 1 pixels equals the exact integer sum of squared differences / npx: 0 against 255 everywhere (a sum of
    8.4 10^14), and a photo against a copy with every 97th byte changed"""
    ctx, torch, dev = env
    need(torch, N32 * 6 + 4 * GB)
    a = torch.zeros(N32 * 3, dtype=torch.uint8, device=dev)
    b = torch.full((N32 * 3,), 255, dtype=torch.uint8, device=dev)
    assert ctx.mse(a, b) == 3 * 255 * 255 * N32 / N32
    ctx.synth_image(1, SEED + 7, W32, H32, out=a)
    b.copy_(a)
    b[::97] ^= 0x35
    exact = _sq_sum(torch, a, b)
    assert exact > (1 << 32)
    assert ctx.mse(a, b) == exact / N32


# ---------------------------------------------------------------- 9. batches whose bytes pass 4 GiB
@pytest.mark.parametrize("expr", ["delta", "hufman", "cluster-colors(256)"])
def test_batch_past_4_gib(env, expr):
    """7 frames of 16384^2 photo (frame 6 starts at 4.83 GB, stream 6 at 12.9 GB): encode_batch gives every frame its single encode's
    bytes, decode_batch into one buffer with a 4096-byte gap per frame gives every frame its single decode and leaves the gaps alone,
    and mse_batch over the 7 pairs equals the per-frame cniic_mse and the exact sums"""
    ctx, torch, dev = env
    F, s = 7, 16384
    npx = s * s
    stride = 1 << 31                        # a power of two: a wrapped f stride lands on another frame's stream, whose head parses
    img_stride = npx * 3 + 4096
    need(torch, F * (npx * 3 + stride + img_stride) + stride + npx * 3 + 8 * GB)
    frames = torch.empty((F, s, s, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        ctx.synth_image(1, SEED + 10 + f, s, s, out=frames[f])
    out = torch.empty(F * stride, dtype=torch.uint8, device=dev)
    rc, lens, rcs, _ = ctx.encode_batch(expr, frames, s, s, F, out, stride)
    assert rc == 0 and rcs == [0] * F
    single = torch.empty(stride, dtype=torch.uint8, device=dev)
    for f in range(F):
        rc, n, _ = ctx.encode(expr, frames[f], w=s, h=s, out=single)
        assert rc == 0 and n == lens[f], f
        assert torch.equal(out[f * stride:f * stride + n], single[:n]), f

    dec = torch.full((F * img_stride,), 0xA5, dtype=torch.uint8, device=dev)
    rc, ws, hs, rcs = ctx.decode_batch(expr, out, stride, lens, F, dec, img_stride)
    assert rc == 0 and ws == [s] * F and hs == [s] * F and rcs == [0] * F
    one = torch.empty(npx * 3, dtype=torch.uint8, device=dev)
    for f in range(F):
        rc, w, h = ctx.decode_into(expr, out[f * stride:], lens[f], one)
        assert rc == 0 and (w, h) == (s, s)
        assert torch.equal(dec[f * img_stride:f * img_stride + npx * 3], one), f
        assert bool((dec[f * img_stride + npx * 3:(f + 1) * img_stride] == 0xA5).all()), f
    del out, single, one

    back = dec.reshape(F, img_stride)[:, :npx * 3].contiguous()
    del dec
    got = ctx.mse_batch(frames, back, npx, F)
    flat = frames.reshape(F, -1)
    want = [_sq_sum(torch, flat[f], back[f]) / npx for f in range(F)]
    assert got == want and got == [ctx.mse(flat[f], back[f]) for f in range(F)]
    if expr == "cluster-colors(256)":
        assert all(v > 0 for v in got)
