"""cniic_codec_encode_batch_var / cniic_mse_batch_var / cniic_codec_measure_batch: the reference's many-image loop (bench.rs:15-83,
measure_all) over images of DIFFERENT sizes in one call.  Every comparison is exact: a frame of a batch must come out byte for byte,
status for status and double for double as the single calls give it for that image alone, wherever it lies in the caller's buffer and
whichever worker took it."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = ("hufman", "cluster-colors(16)", "cluster-colors(256)", "voronoi(8)", "delta", "hilbert(rle)")
LOSSLESS = ("hufman", "delta", "hilbert(rle)")
# (w, h): the degenerate ones, two equal sizes next to each other (twice), one of more than 2^20 pixels
SIZES = [(1, 1), (1, 37), (37, 1), (64, 64), (100, 75), (333, 517), (160, 96), (160, 96), (97, 131), (256, 130), (256, 130), (200, 300),
         (1200, 900), (50, 50)]
ORACLE_MAX_PX = 333 * 517   # the oracle does these in seconds: all but the largest
FAILURES = (-1, -2, -3, -8)  # BAD_ARG, TOO_FEW_POINTS, FEW_ACTIVE, CAPACITY


def _images(ctx, seed=0):
    from cniic_amd import _lib, synth
    return [ctx.synth_image(_lib.SYNTH_UNIFORM if i % 3 == 1 else _lib.SYNTH_PHOTO, synth.SEED0 + 4000 + seed + i, w, h) for i, (w, h) in enumerate(SIZES)]


def _pack(imgs):
    """back to back: 3 w h is rarely a multiple of 16, so the offsets take many residues"""
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    return np.concatenate([im.reshape(-1) for im in imgs]), offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]


def _singles(expr, imgs):
    """cniic_codec_encode_opts of every image alone, on a context that has seen no batch -> [(rc, bytes, stats)]"""
    import cniic_amd
    with cniic_amd.Context(0) as ref:
        return [ref.encode(expr, im, allow=FAILURES) for im in imgs]


def _round4(n):
    return (n + 3) & ~3


def _batch(ctx, expr, imgs, on_dev, stride, allow=FAILURES):
    import torch
    buf, offs, ws, hs = _pack(imgs)
    F = len(imgs)
    if on_dev:
        dev = torch.device("cuda", 0)
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
    else:
        src, out = buf, np.zeros(stride * F, np.uint8)
    rc, lens, rcs, sts = ctx.encode_batch_var(expr, src, offs, ws, hs, out, stride, allow=allow)
    host = out.cpu().numpy() if on_dev else out
    streams = [host[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == 0 else None for f in range(F)]
    return rc, lens, rcs, sts, streams, out


def _check_against_singles(expr, res, singles):
    rc, lens, rcs, sts, streams, _ = res
    for f, (src, sdata, sst) in enumerate(singles):
        assert rcs[f] == src, (expr, f, rcs[f], src)
        assert sts[f]["iterations"] == sst["iterations"], (expr, f)
        if src == 0:
            assert lens[f] == len(sdata) and streams[f] == sdata, (expr, f, SIZES[f])
    assert rc == next((r for r in rcs if r != 0), 0)


@pytest.mark.parametrize("expr", CODECS)
def test_same_bytes_as_single_encodes(expr):
    import cniic_amd
    import oracle_lib as O
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx)
        assert len(imgs) >= 12 and len({o % 16 for o in _pack(imgs)[1]}) >= 6
        singles = _singles(expr, imgs)
        assert sum(s[0] == 0 for s in singles) >= len(imgs) - 4
        if expr == "voronoi(8)":
            assert singles[0][0] != 0        # 1 x 1: fewer points than clusters; the batch must say so for that frame alone
        stride = _round4(max(len(s[1]) for s in singles)) + 4
        for on_dev in (False, True):
            res = _batch(ctx, expr, imgs, on_dev, stride)
            _check_against_singles(expr, res, singles)
        for f, im in enumerate(imgs):
            if im.shape[0] * im.shape[1] <= ORACLE_MAX_PX and singles[f][0] == 0:
                rco, edata, _ = O.encode(expr, im, mode=O.MODE_L)
                assert rco == 0 and res[4][f] == edata, (expr, f, SIZES[f])
        assert ctx.encode_batch_var(expr, imgs[0], [], [], [], np.zeros(4, np.uint8), 4) == (0, [], [], [])


def test_offsets_do_not_pick_the_route():
    """one image of more than 2^20 pixels at 0, 1, 4 and 15 bytes past a 16-byte boundary: the same bytes four times, and the pixel
    partition of cluster-colors four times (the misaligned three through the workers' aligned scratch)"""
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    w, h = 1200, 900
    shifts = (0, 1, 4, 15)
    with cniic_amd.Context(0) as ctx:
        img = ctx.synth_image(_lib.SYNTH_PHOTO, synth.SEED0 + 4100, w, h)
        want = _singles("cluster-colors(256)", [img])[0]
        assert want[0] == 0
        slot = (img.size + 64) & ~15
        big = torch.zeros(slot * len(shifts), dtype=torch.uint8, device=dev)
        assert big.data_ptr() % 16 == 0
        offs = [k * slot + s for k, s in enumerate(shifts)]
        for o in offs:
            big[o:o + img.size] = torch.from_numpy(img.reshape(-1)).to(dev)
        stride = _round4(len(want[1])) + 16
        out = torch.zeros(stride * len(shifts), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, lens, rcs, sts = ctx.encode_batch_var("cluster-colors(256)", big, offs, [w] * 4, [h] * 4, out, stride)
        routed, staged = ctx.kernel_time("cc_pixel_partition")[1], ctx.kernel_time("batch_stage")[1]
        dense = ctx.kernel_time("hist_rgb")[1]    # (the dense-table route's histogram)
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert rc == 0 and rcs == [0] * 4 and lens == [len(want[1])] * 4
        host = out.cpu().numpy()
        for k in range(4):
            assert host[k * stride:k * stride + lens[k]].tobytes() == want[1], k
            assert sts[k]["iterations"] == want[2]["iterations"]
        assert (routed, staged, dense) == (4, 3, 0)


def test_capacity_stays_per_frame():
    import cniic_amd
    from cniic_amd import _lib
    expr = "hufman"
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx, seed=100)
        singles = _singles(expr, imgs)
        by_len = sorted(range(len(imgs)), key=lambda f: -len(singles[f][1]))
        big2, third = by_len[:2], by_len[2]
        stride = _round4(len(singles[third][1])) + 4
        assert stride < len(singles[big2[1]][1])
        for on_dev in (True, False):
            rc, lens, rcs, sts, streams, _ = _batch(ctx, expr, imgs, on_dev, stride)
            assert rc == _lib.CAPACITY
            for f in range(len(imgs)):
                assert lens[f] == len(singles[f][1]), f
                if f in big2:
                    assert rcs[f] == _lib.CAPACITY
                else:
                    assert rcs[f] == 0 and streams[f] == singles[f][1], f
            res = _batch(ctx, expr, imgs, on_dev, _round4(max(lens)))   # the stride the call asked for
            _check_against_singles(expr, res, singles)
            assert res[0] == 0


@pytest.mark.parametrize("expr", CODECS)
def test_round_trip_through_decode_batch(expr):
    import torch
    import cniic_amd
    dev = torch.device("cuda", 0)
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx, seed=200)
        F = len(imgs)
        stride = _round4(max(im.size for im in imgs) * 6 + (1 << 16))
        rc, lens, rcs, sts, streams, out = _batch(ctx, expr, imgs, True, stride)
        ok = [f for f in range(F) if rcs[f] == 0]
        assert len(ok) >= F - 4
        img_stride = max(im.size for im in imgs)
        back = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        dl = [lens[f] if rcs[f] == 0 else 0 for f in range(F)]
        drc, ws, hs, drcs = ctx.decode_batch(expr, out, stride, dl, F, back, img_stride, allow=(-6,))
        host = back.cpu().numpy()
        for f in ok:
            assert drcs[f] == 0 and (hs[f], ws[f]) == imgs[f].shape[:2], (expr, f)
            got = host[f * img_stride:f * img_stride + imgs[f].size].reshape(imgs[f].shape)
            if expr in LOSSLESS:
                assert np.array_equal(got, imgs[f]), (expr, f)
            else:
                rc1, one = ctx.decode(expr, streams[f])
                assert rc1 == 0 and np.array_equal(got, one), (expr, f)


def _pairs(rng, npx, residues=True):
    """two byte buffers holding len(npx) pairs at random places; the first 16 pairs take every residue mod 16 on the a side and, in
    another order, on the b side"""
    a_off, b_off = [], []
    pa = pb = 0
    for f, n in enumerate(npx):
        ga, gb = (int(rng.integers(0, 16)), int(rng.integers(0, 16)))
        if residues and f < 16:
            ga, gb = (f - pa) % 16, ((5 * f + 3) - pb) % 16
        a_off.append(pa + ga)
        b_off.append(pb + gb)
        pa, pb = a_off[-1] + 3 * n, b_off[-1] + 3 * n
    a = rng.integers(0, 256, pa + 16, dtype=np.uint8)
    b = rng.integers(0, 256, pb + 16, dtype=np.uint8)
    return a, a_off, b, b_off


def _exact(a, ao, b, bo, n):
    if n == 0:
        return 0.0
    d = a[ao:ao + 3 * n].astype(np.int64) - b[bo:bo + 3 * n].astype(np.int64)
    return float(int((d * d).sum())) / float(n)


def test_mse_batch_var_bit_equal_to_mse():
    import torch
    import cniic_amd
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    with cniic_amd.Context(0) as ctx:
        npx = [int(x) for x in rng.integers(0, 5001, 300)]
        npx[20], npx[21], npx[22] = 0, 4999, 1234
        a, a_off, b, b_off = _pairs(rng, npx)
        assert {o % 16 for o in a_off} == set(range(16)) and {o % 16 for o in b_off} == set(range(16))
        b[b_off[21]:b_off[21] + 3 * npx[21]] = a[a_off[21]:a_off[21] + 3 * npx[21]]      # an identical pair
        a[a_off[22]:a_off[22] + 3 * npx[22]] = 0                                           # 0 against 255
        b[b_off[22]:b_off[22] + 3 * npx[22]] = 255
        single = [ctx.mse(a[a_off[f]:a_off[f] + 3 * npx[f]], b[b_off[f]:b_off[f] + 3 * npx[f]]) if npx[f] else 0.0 for f in range(300)]
        assert single == [_exact(a, a_off[f], b, b_off[f], npx[f]) for f in range(300)]
        assert single[21] == 0.0 and single[22] == 195075.0 and single[20] == 0.0
        assert ctx.mse_batch_var(a, a_off, b, b_off, npx) == single                        # host buffers
        a_d, b_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        assert ctx.mse_batch_var(a_d, a_off, b_d, b_off, npx) == single                    # device buffers
        launches = [ctx.kernel_time("sqerr_batch_var")[1]]
        assert ctx.mse_batch_var(a_d, a_off, b, b_off, npx) == single                      # one side each
        assert ctx.mse_batch_var(a_d, [], b_d, [], []) == []
        # more pairs than one grid dimension holds
        many = [int(x) for x in rng.integers(1, 17, 70000)]
        a, a_off, b, b_off = _pairs(rng, many, residues=False)
        a_d, b_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        torch.cuda.synchronize()
        got = ctx.mse_batch_var(a_d, a_off, b_d, b_off, many)
        launches.append(ctx.kernel_time("sqerr_batch_var")[1])
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert got == [_exact(a, a_off[f], b, b_off[f], many[f]) for f in range(70000)]
        for f in range(0, 70000, 139):
            assert got[f] == ctx.mse(a[a_off[f]:a_off[f] + 3 * many[f]], b[b_off[f]:b_off[f] + 3 * many[f]]), f
        assert launches[0] > 0 and launches[0] == launches[1], launches


def test_mse_batch_var_one_pair_past_4_gib():
    import torch
    import cniic_amd
    dev = torch.device("cuda", 0)
    npx = (1 << 32) // 3 + 100003
    nbytes = 3 * npx
    assert nbytes > (1 << 32)
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * nbytes + (6 << 30):
        pytest.skip("two device buffers of %.1f GB each need %.1f GB free, the device has %.1f" % (nbytes / 1e9, (2 * nbytes + (6 << 30)) / 1e9, free / 1e9))
    a_off, b_off, piece = 3, 9, 1 << 28
    a = torch.empty(nbytes + 32, dtype=torch.uint8, device=dev)
    b = torch.empty(nbytes + 32, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    total = 0
    for at in range(0, nbytes + 32, piece):
        n = min(piece, nbytes + 32 - at)
        a[at:at + n] = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)
        b[at:at + n] = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)
    for at in range(0, nbytes, piece):
        n = min(piece, nbytes - at)
        d = a[a_off + at:a_off + at + n].to(torch.int32) - b[b_off + at:b_off + at + n].to(torch.int32)
        total += int((d * d).sum(dtype=torch.int64).item())
        del d
    torch.cuda.synchronize()
    with cniic_amd.Context(0) as ctx:
        got = ctx.mse_batch_var(a, [a_off, a_off], b, [b_off, b_off + 1], [npx, 7])
        assert got[0] == float(total) / float(npx)
        assert got[1] == ctx.mse(a[a_off:a_off + 21].cpu().numpy(), b[b_off + 1:b_off + 22].cpu().numpy())
        assert ctx.mse(a[a_off:a_off + nbytes], b[b_off:b_off + nbytes]) == got[0]


def _rows_of_singles(ctx, expr, imgs, singles):
    rows = []
    for im, (rc, data, st) in zip(imgs, singles):
        if rc != 0:
            rows.append(None)
            continue
        rc2, back = ctx.decode(expr, data)
        assert rc2 == 0
        npx = im.shape[0] * im.shape[1]
        rows.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
    return rows


@pytest.mark.parametrize("expr", ("hufman", "delta", "cluster-colors(64)"))
def test_measure_equals_the_three_single_calls(expr, monkeypatch):
    import math
    import torch
    import cniic_amd
    dev = torch.device("cuda", 0)
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx, seed=300)
        singles = _singles(expr, imgs)
        want = _rows_of_singles(ctx, expr, imgs, singles)
        assert sum(r is not None for r in want) >= len(imgs) - 3   # (cluster-colors(64): the three images of fewer than 64 pixels)
        buf, offs, ws, hs = _pack(imgs)
        F = len(imgs)
        stride = _round4(max(len(s[1]) for s in singles)) + 8

        def check(rc, rows, lens, out):
            assert rc == next((s[0] for s in singles if s[0] != 0), 0)
            for f in range(F):
                if want[f] is None:
                    assert rows[f]["rc"] == singles[f][0] and math.isnan(rows[f]["error"]), (expr, f)
                    continue
                got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
                assert got == want[f], (expr, f, got, want[f])
                assert rows[f]["lossless_mismatch"] == 0 and rows[f]["kmeans"]["iterations"] == singles[f][2]["iterations"]
                if expr in LOSSLESS:
                    assert rows[f]["error"] == 0.0
                if out is not None:
                    host = out.cpu().numpy() if hasattr(out, "cpu") else out
                    assert lens[f] == len(singles[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == singles[f][1], (expr, f)

        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        check(*ctx.measure_batch(expr, src, offs, ws, hs, out, stride, allow=FAILURES), out)     # device buffers, with the streams
        check(*ctx.measure_batch(expr, src, offs, ws, hs, allow=FAILURES), None)                 # ... without them
        hout = np.zeros(stride * F, np.uint8)
        check(*ctx.measure_batch(expr, buf, offs, ws, hs, hout, stride, allow=FAILURES), hout)   # host buffers
        # a scratch budget of 1 MiB: the largest image is a chunk of its own (its stream's room alone is 17 MB), the five images of
        # 25 000 to 172 000 pixels take one each (0.5 to 3.3 MB a frame), the small ones share what is left: seven chunks at least
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(1 << 20))
        check(*ctx.measure_batch(expr, src, offs, ws, hs, out, stride, allow=FAILURES), out)
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
        assert ctx.measure_batch(expr, src, [], [], []) == (0, [], [])


def test_measure_keeps_failures_per_frame():
    """voronoi(8) of a 1 x 1 image has fewer points than clusters: that row carries the encode's status and NaN, the others are measured"""
    import math
    import cniic_amd
    expr = "voronoi(8)"
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx, seed=300)[:8]
        singles = _singles(expr, imgs)
        want = _rows_of_singles(ctx, expr, imgs, singles)
        assert want[0] is None and sum(r is None for r in want) <= 3
        buf, offs, ws, hs = _pack(imgs)
        rc, rows, _ = ctx.measure_batch(expr, buf, offs, ws, hs, allow=FAILURES)
        assert rc == singles[0][0]
        for f in range(len(imgs)):
            if want[f] is None:
                assert rows[f]["rc"] == singles[f][0] and math.isnan(rows[f]["error"]) and rows[f]["compressed_size"] == 0
            else:
                assert {k: rows[f][k] for k in want[f]} == want[f], f


def test_harness_one_call_writes_the_same_csv(tmp_path):
    from cniic_amd import synth
    exe = os.path.join(ROOT, "tools", "cniic_bench")
    assert os.path.exists(exe), "tools/cniic_bench is built by `make -C cniic_amd/csrc`"
    names = []
    for i, (w, h) in enumerate([(96, 64), (333, 200), (40, 33), (640, 480)]):
        img = synth.photo(w, h, synth.SEED0 + 4500 + i) if i != 2 else synth.uniform(w, h, synth.SEED0 + 4500 + i)
        names.append("img%d.ppm" % i)
        with open(tmp_path / names[-1], "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    for expr, csv in (("hufman", "Hufman.csv"), ("cluster-colors(16)", "cluster-colors_16.csv")):
        r = subprocess.run([exe, "--codec=" + expr] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        loop = open(tmp_path / "output" / csv).read().strip().split("\n")
        r = subprocess.run([exe, "--codec=" + expr, "--one-call"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        one = open(tmp_path / "output" / csv).read().strip().split("\n")
        assert one[0] == loop[0] == "name,compressed_size,compression_ratio,error"
        assert [l.split(",")[0] for l in one[1:]] == names                    # rows in argument order
        assert sorted(one[1:]) == sorted(loop[1:])                             # (the loop's rows come in the order its workers finish)
    r = subprocess.run([exe, "--codec=hufman", "--one-call", names[0], "missing.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot read image" in r.stderr
    assert len(open(tmp_path / "output" / "Hufman.csv").read().strip().split("\n")) == 2


def test_dealing_does_not_show():
    """cluster-colors(256) twice each with 1, 3 and 8 worker streams: the same outputs every time"""
    import cniic_amd
    from cniic_amd import _lib
    expr = "cluster-colors(256)"
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx, seed=400)
        stride = _round4(max(im.size for im in imgs) * 2 + (1 << 16))
        runs = []
        for S in (1, 3, 8, 8, 3, 1):
            ctx.set_opt(_lib.OPT_BATCH_STREAMS, S)
            rc, lens, rcs, sts, streams, _ = _batch(ctx, expr, imgs, True, stride)
            runs.append((rc, lens, rcs, [s["iterations"] for s in sts], streams))
        ctx.set_opt(_lib.OPT_BATCH_STREAMS, None)
        assert all(r == runs[0] for r in runs[1:])
        assert sum(r == 0 for r in runs[0][2]) >= len(imgs) - 4


def test_python_mirror_encode_batch_and_measure():
    """Codec.encode_batch sizes the stride itself and repeats the frames that wanted more; Codec.measure gives the CSV's columns"""
    import cniic_amd
    from cniic_amd.codec import AnyCodec
    with cniic_amd.Context(0) as ctx:
        imgs = _images(ctx, seed=500)[:9]
        for expr in ("hufman", "voronoi(8)"):
            codec = AnyCodec.from_str(expr, ctx)
            singles = _singles(expr, imgs)
            data = codec.encode_batch(imgs)
            assert data == [s[1] if s[0] == 0 else None for s in singles]
            assert [s["iterations"] for s in codec.last_stats] == [s[2]["iterations"] for s in singles]
            rows = codec.measure(imgs)
            assert [r["rc"] for r in rows] == [s[0] for s in singles]
            assert [r["compressed_size"] for r in rows] == [len(s[1]) for s in singles]
            assert all(set(("compressed_size", "compression_ratio", "error", "rc")) <= set(r) for r in rows)
