"""cniic_hilbert_linearize_as (rect / small / large, src/hilbert.rs:10-32) and cniic_channel_diff_hist
(scripts/experiments/hilbert_distribution.py) on the GPU, exactly equal to the numpy restatement in linearize_ref.py, which follows the
oracle's scans.  The sizes are the smallest that stand on each edge: s = 0 (1 x 1, 1 x 2, 1 x 300), S < 64 (the lane-per-pixel
kernel), exactly one tile (64 x 64), a tile clipped on either side (63 x 65, 65 x 64, 64 x 129, 129 x 257), strips whose square is far
larger than they are (1 x 300, 300 x 1, 1 x 65536), power-of-two sides, which halve `small` (4 x 4, 64 x 64, 256 x 256), and two sizes
with many tiles."""
import ctypes as C
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import linearize_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 4), (5, 3), (63, 65), (64, 64), (65, 64), (64, 129), (129, 257), (37, 100), (100, 37), (1, 300),
         (300, 1), (256, 256), (1000, 600), (2048, 1536)]


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _case(w, h):
    """a photo-like image (the device generator writes synth.photo's bytes) and the restatement's three answers, computed once"""
    import cniic_amd
    from cniic_amd import _lib, synth
    with cniic_amd.Context(0) as c:
        img = c.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 700 + w + 3 * h, w, h)
    ref = {m: R.linearize(img, m) for m in R.METHODS}
    for v in (img, *ref.values()):
        v.setflags(write=False)
    return img, ref


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()     # (the context runs on a stream of its own)
    return t


def _pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


def _sorted_pixels(a):
    return np.sort(a.reshape(-1, 3).astype(np.int64) @ np.array([65536, 256, 1]))


@pytest.mark.parametrize("w,h", SIZES)
def test_three_methods_equal_the_restatement(ctx, w, h):
    import torch
    from cniic_amd import _lib
    img, ref = _case(w, h)
    img_d = _dev(img)
    got = {}
    for m in R.METHODS:
        assert _lib.linearize_count(m, w, h) == len(ref[m])
        got[m] = ctx.hilbert_linearize_as(img, m)                                  # host buffers
        assert got[m].shape == ref[m].shape and np.array_equal(got[m], ref[m]), (m, "host")
        out_d = torch.full((max(len(ref[m]), 1) * 3,), 0xA5, dtype=torch.uint8, device=img_d.device)
        torch.cuda.synchronize()
        rc, n = ctx.hilbert_linearize_as(img_d, m, w, h, out_d)                    # device buffers
        assert rc == 0 and n == len(ref[m])
        assert np.array_equal(out_d[:3 * n].cpu().numpy().reshape(-1, 3), ref[m]), (m, "device")
    # rect is cniic_hilbert_linearize byte for byte
    assert np.array_equal(got["rect"], ctx.hilbert_linearize(img))
    # a permutation of the image's pixels
    assert np.array_equal(_sorted_pixels(got["large"]), _sorted_pixels(img))
    if w == h and _pow2(w):
        assert np.array_equal(got["large"], got["rect"])
        if w >= 2:   # small of a 2^n square = cniic_hilbert_linearize of its top-left 2^(n-1) crop
            assert np.array_equal(got["small"], ctx.hilbert_linearize(np.ascontiguousarray(img[:w // 2, :w // 2])))


@pytest.mark.parametrize("w,h", [(129, 257), (256, 256), (5, 3)])
def test_device_output_at_an_odd_byte_offset(ctx, w, h):
    import torch
    img, ref = _case(w, h)
    img_d = _dev(img)
    for m in R.METHODS:
        n = len(ref[m])
        buf = torch.full((3 * n + 16,), 0x5A, dtype=torch.uint8, device=img_d.device)
        torch.cuda.synchronize()
        out = buf[1:1 + 3 * n]
        assert out.data_ptr() % 2 == 1
        rc, got_n = ctx.hilbert_linearize_as(img_d, m, w, h, out)
        host = buf.cpu().numpy()
        assert rc == 0 and got_n == n and np.array_equal(host[1:1 + 3 * n].reshape(-1, 3), ref[m]), m
        assert host[0] == 0x5A and (host[1 + 3 * n:] == 0x5A).all(), m         # nothing outside the answer


def test_strip_whose_square_has_2_to_the_32_positions(ctx):
    """1 x 65536 and 65536 x 1: S = 65536.  The answer is the strip's pixels in the order the square's curve meets them, and it comes at
    once -- which only holds if the S^2 positions are not walked."""
    from cniic_amd import _lib, synth
    for w, h in ((1, 65536), (65536, 1)):
        img = ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 900 + w, w, h)
        exp = R.large_by_position(img)
        ctx.hilbert_linearize_as(img, "large")       # (the first call of a size may allocate)
        t0 = time.perf_counter()
        got = ctx.hilbert_linearize_as(img, "large")
        dt = time.perf_counter() - t0
        assert np.array_equal(got, exp)
        assert dt < 2.0, dt
        assert len(ctx.hilbert_linearize_as(img, "small")) == 0


def snake(w, h):
    xy = np.empty((h, w, 2), np.uint32)
    xs = np.arange(w, dtype=np.uint32)
    for y in range(h):
        xy[y, :, 0] = xs if y % 2 == 0 else xs[::-1]
        xy[y, :, 1] = y
    return xy.reshape(-1, 2)


@pytest.mark.parametrize("w,h", [(100, 37), (65, 64)])
def test_large_along_the_injected_square_scan_equals_the_computed_rank(w, h):
    import cniic_amd
    from cniic_amd import _lib
    img, ref = _case(w, h)
    S = R.large_side(w, h)
    with cniic_amd.Context(0) as c:
        c.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        analytic = c.hilbert_linearize_as(img, "large")
        assert c.kernel_time("lin_large")[1] == 1                 # one launch: the rank is computed
        c.set_scan(S, S, O.hilbert_iter(S, S))                    # the oracle's own scan of the square, now followed position by position
        injected = c.hilbert_linearize_as(img, "large")
        assert c.kernel_time("lin_large")[1] == 3                 # flags, scan, gather: the other route ran
        assert np.array_equal(injected, analytic) and np.array_equal(analytic, ref["large"])
        # an order that is not the curve's: the square walked in rows, back and forth
        s = snake(S, S)
        c.set_scan(S, S, s)
        keep = s[(s[:, 0] < w) & (s[:, 1] < h)]
        assert np.array_equal(c.hilbert_linearize_as(img, "large"), img[keep[:, 1], keep[:, 0]])
        c.set_scan(S, S, None)
        assert np.array_equal(c.hilbert_linearize_as(img, "large"), ref["large"])
        assert c.kernel_time("lin_large")[1] == 1


@pytest.mark.parametrize("w,h", [(100, 37), (129, 257), (5, 3)])
def test_small_follows_an_injected_scan_and_other_dimensions_change_nothing(w, h):
    import cniic_amd
    img, ref = _case(w, h)
    s = R.small_side(w, h)
    with cniic_amd.Context(0) as c:
        sn = snake(s, s)
        c.set_scan(s, s, sn)
        assert np.array_equal(c.hilbert_linearize_as(img, "small"), img[sn[:, 1], sn[:, 0]])
        for m in ("rect", "large"):
            assert np.array_equal(c.hilbert_linearize_as(img, m), ref[m]), m
        c.set_scan(s + 1, s, snake(s + 1, s))                     # dimensions none of the three methods scans
        for m in R.METHODS:
            assert np.array_equal(c.hilbert_linearize_as(img, m), ref[m]), m


def test_capacity_one_short_writes_nothing(ctx):
    import torch
    from cniic_amd import _lib
    w, h = 65, 64
    img, ref = _case(w, h)
    img_d = _dev(img)
    for m in R.METHODS:
        need = len(ref[m])
        host = np.full(3 * need, 0xC3, np.uint8)
        rc, n = ctx.hilbert_linearize_as(img, m, out=host[:3 * (need - 1)], allow=(_lib.CAPACITY,))
        assert rc == _lib.CAPACITY and n == need and (host == 0xC3).all(), m
        dev = torch.full((3 * need,), 0xC3, dtype=torch.uint8, device=img_d.device)
        torch.cuda.synchronize()
        rc, n = ctx.hilbert_linearize_as(img_d, m, w, h, dev[:3 * (need - 1)], allow=(_lib.CAPACITY,))
        assert rc == _lib.CAPACITY and n == need and bool((dev == 0xC3).all()), m
    # an unknown method is refused
    n = C.c_uint64(0)
    assert _lib.lib().cniic_hilbert_linearize_as(ctx.h, C.c_int32(7), img.ctypes.data_as(C.c_void_p), C.c_uint32(w), C.c_uint32(h),
                                                 host.ctypes.data_as(C.c_void_p), C.c_uint64(host.size // 3), C.byref(n)) == _lib.BAD_ARG


def test_module_level_wrappers(ctx):
    import cniic_amd
    img, ref = _case(100, 37)
    for m in R.METHODS:
        assert np.array_equal(cniic_amd.hilbert_linearize(img, m, ctx=ctx), ref[m])
    got = cniic_amd.hilbert_linearize(_dev(img), "large")                          # a device tensor, a context of its own
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref["large"])
    hist = cniic_amd.channel_diff_hist(ref["large"])
    assert hist.dtype == np.int64 and hist.shape == (3, 511) and np.array_equal(hist, R.channel_diff_hist(ref["large"]))
    assert np.array_equal(cniic_amd.channel_diff_hist(got, ctx=ctx), hist)


# ---------------------------------------------------------------- the difference histogram
def _streams():
    from cniic_amd import synth
    rng = np.random.default_rng(11)
    out = {"n%d" % n: rng.integers(0, 256, (n, 3), dtype=np.uint8) for n in (0, 1, 2, 255, 256, 257)}
    n = 1024 * 1024
    out["flat"] = np.full((n, 3), (9, 200, 77), np.uint8)
    out["noise"] = synth.uniform(1024, 1024, synth.SEED0 + 12).reshape(-1, 3)
    board = np.empty((n - 3, 3), np.uint8)                                          # two colours in turn, an odd number of pixels
    board[0::2] = (0, 255, 10)
    board[1::2] = (255, 0, 13)
    out["checkerboard"] = board
    return out


def test_diff_hist_equals_numpy(ctx):
    import torch
    from cniic_amd import _lib, synth
    streams = _streams()
    photo = ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 13, 1024, 1024)
    streams["photo"] = ctx.hilbert_linearize_as(photo, "rect")                    # a 1024^2 photo-like linearisation
    for name, lin in streams.items():
        n = len(lin)
        exp = R.channel_diff_hist(lin)
        assert exp.sum(axis=1).tolist() == [max(n - 1, 0)] * 3
        got = ctx.channel_diff_hist(lin)                                            # host stream, host counts
        assert np.array_equal(got, exp), name
        lin_d = _dev(lin.reshape(-1))
        cnt_d = torch.full((3, 511), -1, dtype=torch.int64, device=lin_d.device)
        torch.cuda.synchronize()
        ctx.channel_diff_hist(lin_d, npx=n, out=cnt_d)                              # device stream, device counts
        assert np.array_equal(cnt_d.cpu().numpy(), exp), name
    flat = ctx.channel_diff_hist(streams["flat"])
    assert (flat[:, 255] == 1024 * 1024 - 1).all() and flat.sum() == 3 * (1024 * 1024 - 1)   # every count in bin 255


@pytest.mark.parametrize("n", [2, 17, 255, 4099, 70001])
def test_diff_hist_input_at_every_offset_from_16_byte_alignment(ctx, n):
    import torch
    lin = np.random.default_rng(n).integers(0, 256, (n, 3), dtype=np.uint8)
    exp = R.channel_diff_hist(lin)
    dev = torch.device("cuda", 0)
    for k in (0, 1, 2, 3, 7, 15):
        buf = torch.zeros(3 * n + 32, dtype=torch.uint8, device=dev)
        buf[k:k + 3 * n] = torch.from_numpy(lin.reshape(-1)).to(dev)
        torch.cuda.synchronize()
        view = buf[k:k + 3 * n]
        assert view.data_ptr() % 16 == k
        assert np.array_equal(ctx.channel_diff_hist(view, npx=n), exp), k


# ---------------------------------------------------------------- the tool
def test_tool_special_hilbert_writes_the_three_csv_files(ctx, tmp_path):
    """cniic_bench --special=hilbert (main.rs:23-55) on a PNG written the way test_boundary.py writes its PNG files: output/<stem>.<method>
    .hilbert.csv (only the last extension replaced), header red,blue,green, one r,g,b row per pixel."""
    from PIL import Image
    from cniic_amd import _lib, synth
    exe = os.path.join(ROOT, "tools", "cniic_bench")
    assert os.path.exists(exe), "tools/cniic_bench is built by `make -C cniic_amd/csrc`"
    img = synth.photo(97, 61, synth.SEED0 + 2)
    Image.fromarray(img, "RGB").save(tmp_path / "photo.v2.png")
    r = subprocess.run([exe, "--special=hilbert", "photo.v2.png"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path / "output")) == ["photo.v2.large.hilbert.csv", "photo.v2.rect.hilbert.csv", "photo.v2.small.hilbert.csv"]
    for m in R.METHODS:
        lines = open(tmp_path / "output" / ("photo.v2.%s.hilbert.csv" % m)).read().split("\n")
        assert lines[0] == "red,blue,green" and lines[-1] == ""
        rows = lines[1:-1]
        assert len(rows) == _lib.linearize_count(m, 97, 61)
        lin = ctx.hilbert_linearize_as(img, m)
        assert rows[0] == "%d,%d,%d" % tuple(lin[0]) and rows[-1] == "%d,%d,%d" % tuple(lin[-1])
        assert np.array_equal(np.array([[int(v) for v in row.split(",")] for row in rows], np.uint8), R.linearize(img, m))
    # every other command line as before
    r = subprocess.run([exe, "--special=nonsense", "photo.v2.png"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "Usage" in r.stderr
