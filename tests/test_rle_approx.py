"""cniic_hilbert_rle_approx_encode on the GPU: Hilbert { compress: RLE(d) }::encode (src/codec/hilbertc.rs:26-45, rle_approx
:200-299) byte for byte against the CPU restatements (tests/rle_approx_ref.py: Python for the small images, the C file for the large
ones), at the Makefile's d and at the edges; d == 0 against the exact `hilbert(rle)` encode; host and device buffers, an injected scan,
the capacity retry; and the round trip through the `hilbert(rle)` decoder, single and batched, with its MSE (the exact one, and the reference's f64 sum within rounding)."""
import math

import numpy as np
import pytest

import oracle_lib as O
import rle_approx_ref as R

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 300), (300, 1), (37, 29)]
LARGE = [(512, 512), (1024, 1024), (4000, 3000)]
D_LARGE = [1.0, 2.0, 4.0, 8.0, 16.0, 0.5, math.sqrt(2.0), math.sqrt(3.0), math.inf, -1.0, math.nan]


def _image(kind, w, h):
    from cniic_amd import synth
    if kind == "photo":
        return synth.photo(w, h, synth.SEED0 + 41 + w)
    return getattr(R, kind)(w, h)


KINDS = ["photo", "flat", "ramp", "checker", "noise"]


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = R.compile_c(tmp_path_factory.mktemp("rla"))
    if lib is None:
        pytest.skip("no C compiler for the large restatement")
    return lib


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SMALL)
def test_small_images_bit_exact(ctx, w, h, kind):
    img = _image(kind, w, h)
    lin = O.hilbert_linearize(img)
    for d in R.D_VALUES:
        rc, data = ctx.hilbert_rle_approx_encode(d, img)
        assert rc == 0 and data == R.encode_py(lin, w, h, d), (kind, d)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", LARGE)
def test_large_images_bit_exact(ctx, clib, w, h, kind):
    img = _image(kind, w, h)
    lin = O.hilbert_linearize(img)
    for d in D_LARGE:
        rc, data = ctx.hilbert_rle_approx_encode(d, img)
        exp = R.encode_c(clib, lin, w, h, d)
        assert rc == 0 and len(data) == len(exp) and data == exp, (kind, d)


@pytest.mark.parametrize("kind", ["photo", "distinct", "ramp"])
def test_4096_square_against_c(ctx, clib, kind):
    import torch
    w = h = 4096
    img = _image(kind, w, h)
    lin = O.hilbert_linearize(img)
    dev = torch.from_numpy(img).cuda()
    out = torch.empty(8 + 12 * w * h, dtype=torch.uint8, device="cuda")
    for d in (1.0, 4.0, 16.0, 100.0):
        rc, ln = ctx.hilbert_rle_approx_encode(d, dev, w, h, out=out)
        exp = R.encode_c(clib, lin, w, h, d)
        assert rc == 0 and ln == len(exp), (kind, d)
        assert out[:ln].cpu().numpy().tobytes() == exp, (kind, d)


@pytest.mark.parametrize("kind", KINDS + ["distinct"])
@pytest.mark.parametrize("w,h", [(1, 1), (37, 29), (512, 512)])
def test_zero_is_the_exact_codec(ctx, w, h, kind):
    img = _image(kind, w, h)
    rc, exact, _ = ctx.encode("hilbert(rle)", img)
    assert rc == 0
    for d in (0.0, -0.0):
        rc, data = ctx.hilbert_rle_approx_encode(d, img)
        assert rc == 0 and data == exact, (kind, d)


def test_device_buffers_and_capacity(ctx):
    import torch
    from cniic_amd import _lib
    w, h = 333, 211
    img = _image("photo", w, h)
    exp = R.encode_py(O.hilbert_linearize(img), w, h, 4.0)
    dev = torch.from_numpy(img).cuda()
    out = torch.zeros(len(exp) - 1, dtype=torch.uint8, device="cuda")
    rc, need = ctx.hilbert_rle_approx_encode(4.0, dev, w, h, out=out, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(exp)
    out = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc, ln = ctx.hilbert_rle_approx_encode(4.0, dev, w, h, out=out)
    assert rc == 0 and ln == need and out.cpu().numpy().tobytes() == exp
    host = np.zeros(need, np.uint8)   # device image, host stream
    rc, ln = ctx.hilbert_rle_approx_encode(4.0, dev, w, h, out=host)
    assert rc == 0 and host.tobytes() == exp
    small = np.zeros(10, np.uint8)    # host image, host stream, too small
    rc, need2 = ctx.hilbert_rle_approx_encode(4.0, img, out=small, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need2 == need
    rc, data = ctx.hilbert_rle_approx_encode(4.0, np.zeros((0, 5, 3), np.uint8))   # an empty image: the dimensions alone
    assert rc == 0 and data == bytes([5, 0, 0, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("w,h", [(37, 29), (256, 256)])
def test_injected_scan(w, h):
    import cniic_amd
    img = _image("photo", w, h)
    s = np.random.default_rng(w * h).permutation(w * h)
    xy = np.stack([s % w, s // w], 1).astype(np.uint32)
    lin = img[xy[:, 1], xy[:, 0]]
    with cniic_amd.Context(0) as c:
        c.set_scan(w, h, xy)
        for d in (2.0, 16.0, math.inf, -1.0):
            rc, data = c.hilbert_rle_approx_encode(d, img)
            exp = R.encode_py(lin, w, h, d)
            assert rc == 0 and data == exp, d
            rc, back = c.decode("hilbert(rle)", data)
            assert rc == 0
            exp_lin = np.frombuffer(exp[8:], np.uint8).reshape(-1, 12)
            want = np.repeat(exp_lin[:, 9:12], exp_lin[:, 0], axis=0)   # the records expanded, in the injected scan's order
            assert np.array_equal(back[xy[:, 1], xy[:, 0]], want), d


@pytest.mark.parametrize("kind", ["photo", "ramp", "checker", "noise"])
def test_round_trip_and_mse(ctx, kind):
    from cniic_amd import HilbertRleApprox
    w, h = 200, 150
    img = _image(kind, w, h)
    lin = O.hilbert_linearize(img)
    ds = [1.0, 4.0, 16.0, math.sqrt(3.0), math.inf]
    streams = []
    for d in ds:
        codec = HilbertRleApprox(d, ctx=ctx)
        data = codec.encode(img)
        exp = R.encode_py(lin, w, h, d)
        assert data == exp, d
        rco, recon = O.decode("hilbert(rle)", exp)
        assert rco == 0
        back = codec.decode(data)
        assert back is not None and np.array_equal(back, recon), d
        # cniic_mse is the exact integer sum over the pixel count (k_misc.hip); the reference sums sqrt(s)^2 in f64 (bench.rs:95-104)
        sq = int(((img.astype(np.int64) - recon.astype(np.int64)) ** 2).sum())
        m = ctx.mse(img, back)
        assert m == sq / (w * h), d
        assert abs(m - O.mse(img, recon)) <= 1e-9 * max(1.0, O.mse(img, recon)), d
        streams.append((data, recon))
    batch = HilbertRleApprox(8.0, ctx=ctx).decode_batch([s for s, _ in streams])
    for (s, recon), got in zip(streams, batch):
        assert got is not None and np.array_equal(got, recon)
