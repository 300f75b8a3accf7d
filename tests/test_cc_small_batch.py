"""Small cluster-colors(K <= 256) frames of a batch call on the small-frame route (k_cc_small.hip: a workgroup per frame, its own palette,
then the frames' tail with a palette per frame; include/cniic_hip.h above cniic_codec_encode_batch_var).  Every comparison is exact:
a frame's status, length, bytes, message and K-means statistics are those of cniic_codec_encode_opts for that frame alone on a
context that has seen no batch, and -- up to 128 x 128 -- the bytes are the oracle's (mode L).  Which frames took the route is read from
the stage timer "cc_small_batch", whose launch count is the number of routed frames.

The shaped frames alternate photo-like and uniform synthetic images.  At K = 16 the three frames of fewer than 16 pixels are refused
(TOO_FEW_POINTS) and every other shaped frame succeeds; at K = 256 the six frames of 64 x 64 and more carry at least 256 distinct
colours and succeed (tests/test_cc_small_cpu.py holds the oracle to both).  The further frames -- flat, checkerboard, 256 distinct
colours, grey ramp -- ride in the same calls, which are also made at K = 255 (U = K + 1 for the 256-colour frame) and K = 2 (the ramp's
ties)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_PX = 16384   # kCcSmallMaxPx (cniic_amd/csrc/cc_small.hpp)
SHAPES = [(1, 1), (1, 2), (3, 1), (7, 9), (64, 64), (100, 75), (127, 129), (128, 128), (5, 3277), (160, 120)]   # (w, h)
ORACLE_MAX_PX = 128 * 128
FAILURES = (-1, -2, -3, -8)  # BAD_ARG, TOO_FEW_POINTS, FEW_ACTIVE, CAPACITY
TOO_FEW_POINTS, FEW_ACTIVE, CAPACITY = -2, -3, -8


def shaped_images():
    from cniic_amd import synth
    return [(synth.uniform if i % 2 else synth.photo)(w, h, synth.SEED0 + 7000 + i) for i, (w, h) in enumerate(SHAPES)]


def further_images():
    flat = np.full((20, 30, 3), 77, np.uint8)
    yy, xx = np.mgrid[0:24, 0:31]
    checker = np.where(((xx + yy) & 1)[..., None] == 1, np.array([200, 30, 40], np.uint8), np.array([10, 220, 90], np.uint8)).astype(np.uint8)
    v = np.arange(256, dtype=np.uint32).reshape(16, 16)
    distinct = np.stack([v, (v * 7) & 255, 255 - v], -1).astype(np.uint8)          # 256 distinct colours
    ramp = np.repeat(np.arange(0, 64, dtype=np.uint8)[None, :, None] * 4, 3, axis=2).repeat(5, axis=0)   # 64 greys, five pixels each
    return [flat, checker, distinct, ramp]


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


def singles(key, expr, imgs, **kw):
    """cniic_codec_encode_opts of every image alone, on a context that has seen no batch -> [(rc, bytes, stats, message)]; computed once per key"""
    import cniic_amd
    if key not in _SINGLES:
        res = []
        with cniic_amd.Context(0) as ref:
            for im in imgs:
                rc, data, st = ref.encode(expr, im, allow=FAILURES, **kw)
                res.append((rc, data, st, _last_error(ref) if rc != 0 else ""))
        _SINGLES[key] = res
    return _SINGLES[key]


def batch(ctx, expr, imgs, stride, host_out=False, poison=0, **kw):
    """one cniic_codec_encode_batch_var call on device images with the stage timers on -> (rc, lens, rcs, stats, streams, raw output, routed frames, message)"""
    import torch
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    buf, offs, ws, hs = _pack(imgs)
    F = len(imgs)
    src = torch.from_numpy(buf).to(dev)
    out = np.full(stride * F, poison, np.uint8) if host_out else torch.full((stride * F,), poison, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, lens, rcs, sts = ctx.encode_batch_var(expr, src, offs, ws, hs, out, stride, allow=FAILURES, **kw)
        msg = _last_error(ctx) if rc != 0 else ""
        launches = ctx.kernel_time("cc_small_batch")[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = out if host_out else out.cpu().numpy()
    streams = [host[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == 0 else None for f in range(F)]
    return rc, lens, rcs, sts, streams, host, launches, msg


def check_against_singles(res, want, what):
    rc, lens, rcs, sts, streams = res[:5]
    for f, (src, sdata, sst, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        for k in ("iterations", "moved_last", "empty_reseeds", "active"):
            assert sts[f][k] == sst[k], (what, f, k, sts[f], sst)
        if src == 0:
            assert lens[f] == len(sdata) and streams[f] == sdata, (what, f)
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first])
    if first is not None:
        assert res[7] == want[first][3], (what, res[7], want[first][3])


@pytest.mark.parametrize("K", (16, 256, 255, 2))
def test_route_and_bytes(K):
    import cniic_amd
    import oracle_lib as O
    expr = "cluster-colors(%d)" % K
    imgs = all_images()
    assert len({o % 16 for o in _pack(imgs)[1]}) >= 6
    want = singles(("all", K), expr, imgs)
    stride = _round4(max(len(s[1]) for s in want)) + 4
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride)
    assert res[6] == sum(routed(imgs)) == len(imgs) - 2          # all but 5 x 3277 and 160 x 120
    check_against_singles(res, want, expr)
    for f, im in enumerate(imgs):
        if im.shape[0] * im.shape[1] <= ORACLE_MAX_PX and res[2][f] == 0:
            rco, edata, est = O.encode(expr, im, mode=O.MODE_L)
            assert rco == 0 and res[4][f] == edata, (expr, f)
            assert res[3][f]["iterations"] == est["iterations"] and res[3][f]["empty_reseeds"] == est["empty_reseeds"], (expr, f)
    shaped_ok = sum(r == 0 for r in res[2][:len(SHAPES)])
    if K == 16:
        assert shaped_ok >= len(SHAPES) - 4
    if K == 256:
        assert shaped_ok >= 6 and all(r == 0 for r in res[2][4:len(SHAPES)])
        assert res[2][len(SHAPES) + 2] == 0                       # 256 distinct colours: U = K
    if K == 255:
        assert res[2][len(SHAPES) + 2] == 0                       # U = K + 1
    if K == 2:
        assert res[2][len(SHAPES) + 3] == 0 and res[2][len(SHAPES) + 1] == 0   # the ramp and the checkerboard


@pytest.mark.parametrize("K", (16, 256))
def test_same_batch_with_the_route_off(K, monkeypatch):
    import cniic_amd
    expr = "cluster-colors(%d)" % K
    imgs = all_images()
    want = singles(("all", K), expr, imgs)
    stride = _round4(max(len(s[1]) for s in want)) + 4
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, expr, imgs, stride)
        monkeypatch.setenv("CNIIC_TEST_CC_SMALL_OFF", "1")
        off = batch(ctx, expr, imgs, stride)
        monkeypatch.delenv("CNIIC_TEST_CC_SMALL_OFF")
    assert on[6] == len(imgs) - 2 and off[6] == 0
    assert (on[0], on[1], on[2], on[4]) == (off[0], off[1], off[2], off[4])
    check_against_singles(off, want, expr)


def test_threshold(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    expr = "cluster-colors(16)"
    imgs = [synth.photo(128, 128, synth.SEED0 + 7100), synth.photo(5, 3277, synth.SEED0 + 7101), synth.photo(64, 64, synth.SEED0 + 7102),
            synth.photo(17, 241, synth.SEED0 + 7103)]
    assert [im.shape[0] * im.shape[1] for im in imgs] == [16384, 16385, 4096, 4097]
    want = singles("threshold", expr, imgs)
    assert all(s[0] == 0 for s in want)
    stride = _round4(max(len(s[1]) for s in want)) + 4
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride)
        assert res[6] == 3
        check_against_singles(res, want, "16384 | 16385")
        res = batch(ctx, expr, imgs[:2], stride)
        assert res[6] == 1
        check_against_singles(res, want[:2], "16384 | 16385")
        monkeypatch.setenv("CNIIC_TEST_CC_SMALL_MAX_PX", "4096")
        res = batch(ctx, expr, imgs, stride)
        assert res[6] == 1
        check_against_singles(res, want, "4096 | 4097")
        res = batch(ctx, expr, imgs[3:], stride)
        assert res[6] == 0
        check_against_singles(res, want[3:], "4097 alone")
        monkeypatch.delenv("CNIIC_TEST_CC_SMALL_MAX_PX")


def test_rare_branches():
    """the empty-cluster reseed, FEW_ACTIVE and TOO_FEW_POINTS, each for its frame alone among good frames"""
    import cniic_amd
    import oracle_lib as O
    from cniic_amd import synth
    from test_cc_small_cpu import G, RGBW, image_of
    good = [synth.photo(40, 30, synth.SEED0 + 7200), synth.uniform(33, 21, synth.SEED0 + 7201), synth.photo(64, 48, synth.SEED0 + 7202)]
    flat = np.full((8, 8, 3), 9, np.uint8)
    by_K = {}
    for name in RGBW:
        by_K.setdefault(int(G[name + "_K"][0]), []).append(name)
    with cniic_amd.Context(0) as ctx:
        for K, names in sorted(by_K.items()):
            expr = "cluster-colors(%d)" % K
            fix = [image_of(G[n + "_keys"], G[n + "_weight"]).copy() for n in names]
            imgs = [good[0]] + fix + [flat, good[1], good[2]]
            want = singles(("rare", K), expr, imgs)
            res = batch(ctx, expr, imgs, _round4(max(len(s[1]) for s in want)) + 4)
            assert res[6] == len(imgs)
            check_against_singles(res, want, expr)
            assert res[0] == TOO_FEW_POINTS and res[2][1 + len(fix)] == TOO_FEW_POINTS and "1 distinct colours for %d clusters" % K in res[7]
            assert res[3][1 + len(fix)] == dict(iterations=0, moved_last=0, empty_reseeds=0, active=0, pair_evals=0) and res[1][1 + len(fix)] == 0
            for j, n in enumerate(names):
                rco, edata, est = O.encode(expr, fix[j], mode=O.MODE_L)
                assert rco == 0 and res[2][1 + j] == 0 and res[4][1 + j] == edata, n
                assert res[3][1 + j]["empty_reseeds"] == est["empty_reseeds"] >= 2, n
        # FEW_ACTIVE: stopped after two iterations, too few clusters have members
        K, mi = int(G["rgbw_few_K"][0]), int(G["rgbw_few_max_iters"][0])
        expr = "cluster-colors(%d)" % K
        imgs = [good[0], image_of(G["rgbw_few_keys"], G["rgbw_few_weight"]).copy(), good[2], flat, good[1]]
        want = singles(("few", K), expr, imgs, max_iters=mi)
        res = batch(ctx, expr, imgs, _round4(max(len(s[1]) for s in want)) + 4, max_iters=mi)
        assert res[6] == len(imgs)
        check_against_singles(res, want, expr)
        assert res[2] == [0, FEW_ACTIVE, 0, TOO_FEW_POINTS, 0] and res[0] == FEW_ACTIVE
        assert res[7] == want[1][3] and res[7].startswith("Not enough active clusters")
        assert res[3][1]["iterations"] == mi and res[3][1]["active"] == int((G["rgbw_few_members"] > 0).sum())
        assert res[3][1] == {**want[1][2], "pair_evals": mi * G["rgbw_few_keys"].size * K}
        # a flat frame at K = 16, with its message
        imgs = [good[0], flat, good[1]]
        want = singles(("flat", 16), "cluster-colors(16)", imgs)
        res = batch(ctx, "cluster-colors(16)", imgs, _round4(max(len(s[1]) for s in want)) + 4)
        check_against_singles(res, want, "flat")
        assert res[2] == [0, TOO_FEW_POINTS, 0] and res[7] == want[1][3] == "kmeans: 1 distinct colours for 16 clusters (src/kmeans.rs:68)"


@pytest.mark.parametrize("host_out", (False, True))
def test_capacity_is_one_frame_s(host_out):
    import cniic_amd
    expr = "cluster-colors(16)"
    imgs = all_images()[3:8] + further_images()[2:]     # 7 x 9 ... 128 x 128, 256 colours, ramp: all on the route, all succeed
    want = singles("capacity", expr, imgs)
    assert all(s[0] == 0 for s in want)
    by_len = sorted(range(len(imgs)), key=lambda f: -len(want[f][1]))
    big, second = by_len[0], by_len[1]
    stride = _round4(len(want[second][1])) + 4
    assert stride < len(want[big][1])
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, expr, imgs, stride, host_out=host_out, poison=0xA5)
    assert launches == len(imgs) and rc == CAPACITY
    assert msg == "encode: stream is %d bytes, capacity %d" % (len(want[big][1]), stride)
    for f in range(len(imgs)):
        assert lens[f] == len(want[f][1]), f
        if f == big:
            assert rcs[f] == CAPACITY and bool((host[f * stride:(f + 1) * stride] == 0xA5).all())
        else:
            assert rcs[f] == 0 and streams[f] == want[f][1], f


def tiny_images():
    """at most 16 x 16: three frames of at least 16 distinct colours, three of fewer"""
    from cniic_amd import synth
    yy, xx = np.mgrid[0:5, 0:6]
    checker = np.where(((xx + yy) & 1)[..., None] == 1, np.array([200, 30, 40], np.uint8), np.array([10, 220, 90], np.uint8)).astype(np.uint8)
    rich = [synth.uniform(16, 16, synth.SEED0 + 7400), synth.uniform(12, 9, synth.SEED0 + 7401), synth.uniform(7, 9, synth.SEED0 + 7402)]
    poor = [np.full((8, 8, 3), 9, np.uint8), checker, synth.photo(3, 1, synth.SEED0 + 7403)]
    return rich, poor


@pytest.mark.parametrize("host_out", (False, True))
def test_a_chunk_whose_frames_all_fail_the_kmeans_check(host_out):
    """no frame goes on to the tail: nothing is placed, no place timer is recorded, no byte is written"""
    import cniic_amd
    expr = "cluster-colors(16)"
    imgs = tiny_images()[1]
    want = singles("all fail", expr, imgs)
    assert [s[0] for s in want] == [TOO_FEW_POINTS] * len(imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, 64, host_out=host_out, poison=0xA5)
        assert ctx.kernel_time("cc_small_place")[1] == 0
    assert res[6] == len(imgs) and res[1] == [0] * len(imgs)
    check_against_singles(res, want, "all fail")
    assert bool((res[5] == 0xA5).all())


@pytest.mark.parametrize("host_out", (False, True))
def test_a_chunk_whose_frames_all_exceed_their_capacity(host_out):
    """every frame has a stream and none has the room: nothing is placed, no place timer is recorded, no byte is written"""
    import cniic_amd
    expr = "cluster-colors(16)"
    imgs = tiny_images()[0]
    want = singles("all short", expr, imgs)
    assert all(s[0] == 0 and len(s[1]) > 8 for s in want)
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, expr, imgs, 8, host_out=host_out, poison=0xA5)
        assert ctx.kernel_time("cc_small_place")[1] == 0
    assert launches == len(imgs) and rc == CAPACITY and rcs == [CAPACITY] * len(imgs)
    assert lens == [len(s[1]) for s in want]
    assert msg == "encode: stream is %d bytes, capacity 8" % len(want[0][1])
    for f, s in enumerate(want):
        for k in ("iterations", "moved_last", "empty_reseeds", "active"):
            assert sts[f][k] == s[2][k], (f, k)
    assert bool((host == 0xA5).all())


def test_many_frames_in_one_launch():
    import cniic_amd
    rng = np.random.default_rng(41)
    expr = "cluster-colors(16)"
    imgs = []
    for f in range(3000):
        w, h = int(rng.integers(8, 25)), int(rng.integers(8, 25))
        imgs.append((rng.integers(0, 32, (h, w, 3)) * 8).astype(np.uint8))
    stride = _round4(8 + 13 * 16 + 24 * 24) + 4            # header bound + a byte per pixel: codes of 16 symbols average under 8 bits
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, expr, imgs, stride)
        assert launches == 3000 and rc == 0 and rcs == [0] * 3000
        with cniic_amd.Context(0) as ref:
            for f in range(0, 3000, 75):
                src, sdata, sst = ref.encode(expr, imgs[f])
                assert src == 0 and streams[f] == sdata and sts[f]["iterations"] == sst["iterations"], f


def test_host_output_gets_the_same_bytes():
    import cniic_amd
    expr = "cluster-colors(256)"
    imgs = all_images()
    want = singles(("all", 256), expr, imgs)
    stride = _round4(max(len(s[1]) for s in want)) + 4
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride, host_out=True)
    assert res[6] == len(imgs) - 2
    check_against_singles(res, want, "host out")


def test_measure_batch_takes_the_route_for_its_small_frames():
    import math
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    expr = "cluster-colors(16)"
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 7300 + i) for i, (w, h) in enumerate(sizes)]
    want = singles("measure", expr, imgs)
    with cniic_amd.Context(0) as ctx:
        rows_want = []
        for im, (rc, data, st, _) in zip(imgs, want):
            if rc != 0:
                rows_want.append(None)
                continue
            rc2, back = ctx.decode(expr, data)
            assert rc2 == 0
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
        assert sum(r is None for r in rows_want) == 1
        buf, offs, ws, hs = _pack(imgs)
        F = len(imgs)
        stride = _round4(max(len(s[1]) for s in want)) + 8
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch(expr, src, offs, ws, hs, out, stride, allow=FAILURES)
        launches = ctx.kernel_time("cc_small_batch")[1]
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == 5
        assert rc == TOO_FEW_POINTS
        host = out.cpu().numpy()
        for f in range(F):
            if rows_want[f] is None:
                assert rows[f]["rc"] == want[f][0] and math.isnan(rows[f]["error"]), f
                continue
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f], (f, got, rows_want[f])
            assert rows[f]["lossless_mismatch"] == 0 and rows[f]["kmeans"]["iterations"] == want[f][2]["iterations"]
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f
