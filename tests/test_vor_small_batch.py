"""Small voronoi(K <= 256) frames of a batch call on the small-frame route (k_vor_small.hip: a workgroup per frame from the pixels through
the whole K-means to the finished stream; include/cniic_hip.h above cniic_codec_encode_batch_var).  Every comparison is exact: a frame's
status, length, bytes, message and K-means statistics are those of cniic_codec_encode_opts for that frame alone on a context that has
seen no batch, and -- up to 128 x 128 (at K = 256 up to 100 x 75) -- the bytes are the oracle's (mode L).  Which frames took the route is
read from the stage timer "vor_small_batch", whose launch count is the number of routed frames.

The shaped frames alternate photo-like and uniform synthetic images.  At K = 16 the three frames of fewer than 16 pixels are refused
(TOO_FEW_POINTS) and every other shaped frame succeeds; at K = 256 the first four are refused (tests/test_vor_small_cpu.py holds the
oracle to both).  The further frames -- flat, checkerboard (reseeds at K = 128; FEW_ACTIVE when stopped after two iterations), 15 x 15
noise (a reseed at K = 100), 256 distinct colours -- ride in the same calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_PX = 16384   # kVorSmallMaxPx (cniic_amd/csrc/vor_small.hpp)
SHAPES = [(1, 1), (1, 2), (3, 1), (7, 9), (64, 64), (100, 75), (127, 129), (128, 128), (5, 3277), (160, 120), (16384, 1), (1, 16384), (129, 127)]   # (w, h)
ORACLE_MAX_PX = 128 * 128
ORACLE_MAX_PX_K256 = 100 * 75
KS = (1, 2, 16, 100, 128, 255, 256)
FAILURES = (-1, -2, -3, -8)  # BAD_ARG, TOO_FEW_POINTS, FEW_ACTIVE, CAPACITY
TOO_FEW_POINTS, FEW_ACTIVE, CAPACITY = -2, -3, -8
STATS = ("iterations", "moved_last", "empty_reseeds", "active")


FLOOR_FEW, FLOOR_MANY, FLOOR_WORK_FEW, FLOOR_WORK_SOME = 8, 128, 131072, 786432    # kVorSmallFloor* (cniic_amd/csrc/capi.cpp)


@pytest.fixture(autouse=True)
def _step_over_the_floor(monkeypatch, request):
    """few heavy frames stay with the workers (the route's floor, capi.cpp vor_small_max_work); every test but the floor's own takes it away"""
    if "floor" not in request.node.name:
        monkeypatch.setenv("CNIIC_TEST_VOR_SMALL_FLOOR_OFF", "1")


def stream_len(K):
    return 16 + 19 * K


def shaped_images():
    from cniic_amd import synth
    return [(synth.uniform if i % 2 else synth.photo)(w, h, synth.SEED0 + 9000 + i) for i, (w, h) in enumerate(SHAPES)]


def further_images():
    from cniic_amd import synth
    flat = np.full((20, 30, 3), 77, np.uint8)
    yy, xx = np.mgrid[0:12, 0:23]
    checker = np.where(((xx + yy) & 1)[..., None] == 1, np.array([200, 30, 40], np.uint8), np.array([10, 220, 90], np.uint8)).astype(np.uint8)
    noise = synth.uniform(15, 15, synth.SEED0 + 31)
    v = np.arange(256, dtype=np.uint32).reshape(16, 16)
    distinct = np.stack([v, (v * 7) & 255, 255 - v], -1).astype(np.uint8)          # 256 distinct colours
    return [flat, checker, noise, distinct]


def all_images():
    return shaped_images() + further_images()


CHECKER = len(SHAPES) + 1


def routed(imgs, max_px=MAX_PX):
    return [1 <= im.shape[0] * im.shape[1] <= max_px for im in imgs]


def _pack(imgs):
    """back to back: 3 w h is rarely a multiple of 16, so the offsets take many residues"""
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    return np.concatenate([im.reshape(-1) for im in imgs]), offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]


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


def batch(ctx, expr, imgs, stride, host_out=False, host_in=False, poison=0, **kw):
    """one cniic_codec_encode_batch_var call with the stage timers on -> (rc, lens, rcs, stats, streams, raw output, routed frames, message)"""
    import torch
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    buf, offs, ws, hs = _pack(imgs)
    F = len(imgs)
    src = buf if host_in else torch.from_numpy(buf).to(dev)
    out = np.full(stride * F, poison, np.uint8) if host_out else torch.full((stride * F,), poison, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, lens, rcs, sts = ctx.encode_batch_var(expr, src, offs, ws, hs, out, stride, allow=FAILURES, **kw)
        msg = _last_error(ctx) if rc != 0 else ""
        launches = ctx.kernel_time("vor_small_batch")[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = out if host_out else out.cpu().numpy()
    streams = [host[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == 0 else None for f in range(F)]
    return rc, lens, rcs, sts, streams, host, launches, msg


def check_against_singles(res, want, what):
    rc, lens, rcs, sts, streams = res[:5]
    for f, (src, sdata, sst, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        for k in STATS:
            assert sts[f][k] == sst[k], (what, f, k, sts[f], sst)
        if src == 0:
            assert lens[f] == len(sdata) and streams[f] == sdata, (what, f)
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first])
    if first is not None:
        assert res[7] == want[first][3], (what, res[7], want[first][3])


def check_poison(res, stride, poison, what, on_route):
    """a frame of the route writes its stream and not a byte more; a frame of the workers may round its stream up to four bytes with zeros in
    device memory, as the single call does (StreamOut, codec.hpp)"""
    lens, rcs, host = res[1], res[2], res[5]
    for f in range(len(rcs)):
        used = lens[f] if rcs[f] == 0 else 0
        if not on_route[f]:
            used = (used + 3) & ~3
        assert bool((host[f * stride + used:(f + 1) * stride] == poison).all()), (what, f)


@pytest.mark.parametrize("K", KS)
def test_route_and_bytes(K):
    import cniic_amd
    import oracle_lib as O
    expr = "voronoi(%d)" % K
    imgs = all_images()
    assert len({o % 16 for o in _pack(imgs)[1]}) >= 6
    want = singles(("all", K), expr, imgs)
    stride = stream_len(K) + 5
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride, poison=0x5A)
    print("voronoi(%d): routed %d of %d, iterations %s" % (K, res[6], len(imgs), [s["iterations"] for s in res[3]]))
    assert res[6] == sum(routed(imgs)) == len(imgs) - 2          # all but 5 x 3277 and 160 x 120
    check_against_singles(res, want, expr)
    check_poison(res, stride, 0x5A, expr, routed(imgs))
    O.lib().orc_set_lloyd_threads(8)
    try:
        for f, im in enumerate(imgs):
            if im.shape[0] * im.shape[1] <= (ORACLE_MAX_PX_K256 if K == 256 else ORACLE_MAX_PX):
                rco, edata, est = O.encode(expr, im, mode=O.MODE_L)
                assert rco == res[2][f], (expr, f, rco, res[2][f])
                if rco == 0:
                    assert res[4][f] == edata, (expr, f)
                    assert res[3][f]["iterations"] == est["iterations"] and res[3][f]["empty_reseeds"] == est["empty_reseeds"], (expr, f)
    finally:
        O.lib().orc_set_lloyd_threads(0)
    shaped = res[2][:len(SHAPES)]
    if K == 16:
        assert shaped == [TOO_FEW_POINTS] * 3 + [0] * (len(SHAPES) - 3)
        assert "1 points for 16 clusters" in res[7]
    if K == 256:
        assert shaped == [TOO_FEW_POINTS] * 4 + [0] * (len(SHAPES) - 4)
        assert res[2][len(SHAPES) + 3] == 0                       # 256 distinct colours on 256 pixels: n = K
    if K == 255:
        assert res[2][len(SHAPES) + 3] == 0                       # n = K + 1
    if K == 128:
        assert res[2][CHECKER] == 0 and res[3][CHECKER]["empty_reseeds"] == 149 and res[3][CHECKER]["iterations"] == 7
    if K == 100:
        assert res[2][CHECKER + 1] == 0 and res[3][CHECKER + 1]["empty_reseeds"] == 1
    for f in range(len(imgs)):
        if res[2][f] == 0 and routed(imgs)[f]:
            n = imgs[f].shape[0] * imgs[f].shape[1]
            assert res[3][f]["iterations"] * n <= res[3][f]["pair_evals"] <= res[3][f]["iterations"] * n * (K + 1), (expr, f)


@pytest.mark.parametrize("K", (16, 128))
def test_same_batch_with_the_route_off_and_without_the_stay_test(K, monkeypatch):
    import cniic_amd
    expr = "voronoi(%d)" % K
    imgs = all_images()
    want = singles(("all", K), expr, imgs)
    stride = stream_len(K) + 5
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, expr, imgs, stride)
        monkeypatch.setenv("CNIIC_TEST_VOR_SMALL_OFF", "1")
        off = batch(ctx, expr, imgs, stride)
        monkeypatch.delenv("CNIIC_TEST_VOR_SMALL_OFF")
        monkeypatch.setenv("CNIIC_TEST_VOR_SMALL_NO_STAY", "1")
        brute = batch(ctx, expr, imgs, stride)
        monkeypatch.delenv("CNIIC_TEST_VOR_SMALL_NO_STAY")
    assert on[6] == len(imgs) - 2 and off[6] == 0 and brute[6] == len(imgs) - 2
    assert (on[0], on[1], on[2], on[4]) == (off[0], off[1], off[2], off[4]) == (brute[0], brute[1], brute[2], brute[4])
    check_against_singles(off, want, expr + " off")
    check_against_singles(brute, want, expr + " no stay")
    saved = 0
    for f, im in enumerate(imgs):
        assert {k: on[3][f][k] for k in STATS} == {k: brute[3][f][k] for k in STATS}, f
        if routed(imgs)[f] and on[2][f] == 0:
            n = im.shape[0] * im.shape[1]
            assert brute[3][f]["pair_evals"] == brute[3][f]["iterations"] * n * (K + 1), f      # every point: its own centroid, then all K
            assert on[3][f]["pair_evals"] <= brute[3][f]["pair_evals"], f
            saved += brute[3][f]["pair_evals"] - on[3][f]["pair_evals"]
    print("voronoi(%d): the stay test saved %d evaluations" % (K, saved))
    assert saved > 0


def test_threshold(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    expr = "voronoi(16)"
    imgs = [synth.photo(128, 128, synth.SEED0 + 9100), synth.photo(5, 3277, synth.SEED0 + 9101), synth.photo(64, 64, synth.SEED0 + 9102),
            synth.photo(17, 241, synth.SEED0 + 9103)]
    assert [im.shape[0] * im.shape[1] for im in imgs] == [16384, 16385, 4096, 4097]
    want = singles("threshold", expr, imgs)
    assert all(s[0] == 0 for s in want)
    stride = stream_len(16)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride)
        assert res[6] == 3
        check_against_singles(res, want, "16384 | 16385")
        res = batch(ctx, expr, imgs[:2], stride)
        assert res[6] == 1
        check_against_singles(res, want[:2], "16384 | 16385")
        monkeypatch.setenv("CNIIC_TEST_VOR_SMALL_MAX_PX", "4096")
        res = batch(ctx, expr, imgs, stride)
        assert res[6] == 1
        check_against_singles(res, want, "4096 | 4097")
        res = batch(ctx, expr, imgs[3:], stride)
        assert res[6] == 0
        check_against_singles(res, want[3:], "4097 alone")
        res = batch(ctx, expr, all_images(), stride)
        assert res[6] == sum(routed(all_images(), 4096))
        check_against_singles(res, singles(("all", 16), expr, all_images()), "all under 4096")
        monkeypatch.delenv("CNIIC_TEST_VOR_SMALL_MAX_PX")


def test_stopped_after_two_iterations():
    """max_iters = 2: the checkerboard answers FEW_ACTIVE for itself alone, the others go on"""
    import cniic_amd
    expr = "voronoi(128)"
    imgs = all_images()
    want = singles(("all", 128, "mi2"), expr, imgs, max_iters=2)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stream_len(128) + 5, max_iters=2)
    assert res[6] == len(imgs) - 2
    check_against_singles(res, want, "max_iters = 2")
    assert res[2][CHECKER] == FEW_ACTIVE and res[3][CHECKER]["iterations"] == 2 and res[3][CHECKER]["active"] == 12 and res[1][CHECKER] == 0
    assert all(s["iterations"] == 2 for f, s in enumerate(res[3]) if res[2][f] in (0, FEW_ACTIVE))
    first = next(f for f, r in enumerate(res[2]) if r != 0)
    assert res[0] == res[2][first] == TOO_FEW_POINTS                  # the 1 x 1 frame comes first
    with cniic_amd.Context(0) as ctx:                                 # ... and with the checkerboard in front, its message is the call's
        sub = [imgs[CHECKER], imgs[4], imgs[CHECKER + 1]]
        res = batch(ctx, expr, sub, stream_len(128), max_iters=2)
    check_against_singles(res, [want[CHECKER], want[4], want[CHECKER + 1]], "checkerboard first")
    assert res[0] == FEW_ACTIVE and res[7].startswith("Not enough active clusters")


def test_a_seed_of_the_caller_s():
    import cniic_amd
    expr = "voronoi(128)"
    imgs = all_images()
    want = singles(("all", 128, "seed"), expr, imgs, seed=12345)
    default = singles(("all", 128), expr, imgs)
    assert want[CHECKER][1] != default[CHECKER][1]                    # the reseeds take other points
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stream_len(128) + 5, seed=12345)
    assert res[6] == len(imgs) - 2
    check_against_singles(res, want, "seed")


def test_a_kmeans_flag_and_host_images_go_to_the_workers():
    import cniic_amd
    from cniic_amd import _lib
    expr = "voronoi(16)"
    imgs = all_images()[3:8] + further_images()
    want = singles("workers", expr, imgs)
    with cniic_amd.Context(0) as ctx:
        for flag in (_lib.KM_BRUTE_FORCE, _lib.KM_NO_SKIP):
            res = batch(ctx, expr, imgs, stream_len(16) + 5, flags=flag)
            assert res[6] == 0
            check_against_singles(res, want, "flag %d" % flag)
        res = batch(ctx, expr, imgs, stream_len(16) + 5, host_in=True)
        assert res[6] == 0
        check_against_singles(res, want, "host images")
        res = batch(ctx, expr, imgs, stream_len(16) + 5)
        assert res[6] == len(imgs)


@pytest.mark.parametrize("K", (16, 256))
def test_host_output_gets_the_same_bytes(K):
    import cniic_amd
    expr = "voronoi(%d)" % K
    imgs = all_images()
    want = singles(("all", K), expr, imgs)
    stride = stream_len(K) + 5
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride, host_out=True, poison=0xC3)
    assert res[6] == len(imgs) - 2
    check_against_singles(res, want, "host out")
    check_poison(res, stride, 0xC3, "host out", routed(imgs))


@pytest.mark.parametrize("host_out", (False, True))
def test_a_stride_one_byte_short(host_out):
    """every frame that has a stream answers CAPACITY with lens[f] = the bytes needed, and nothing is written"""
    import cniic_amd
    K = 16
    expr = "voronoi(%d)" % K
    imgs = all_images()
    want = singles(("all", K), expr, imgs)
    stride = stream_len(K) - 1
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, expr, imgs, stride, host_out=host_out, poison=0xA5)
    assert launches == len(imgs) - 2
    assert bool((host == 0xA5).all())
    for f, (src, sdata, sst, smsg) in enumerate(want):
        if src == 0:
            assert rcs[f] == CAPACITY and lens[f] == stream_len(K), f
            assert {k: sts[f][k] for k in STATS} == {k: sst[k] for k in STATS}, f
        else:
            assert rcs[f] == src and lens[f] == 0, f
    assert rc == TOO_FEW_POINTS and msg == want[0][3]
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs[4:6], stride, host_out=host_out)
        with cniic_amd.Context(0) as ref:
            src, n, st = ref.encode(expr, imgs[4], out=np.zeros(stride, np.uint8), allow=FAILURES)
            assert src == CAPACITY and res[0] == CAPACITY and res[7] == _last_error(ref) == "encode: stream is %d bytes, capacity %d" % (stream_len(K), stride)


def tiny_images():
    """at most 16 x 16, 20 pixels at least"""
    from cniic_amd import synth
    return [synth.uniform(16, 16, synth.SEED0 + 9400), synth.photo(15, 15, synth.SEED0 + 9401), synth.uniform(7, 9, synth.SEED0 + 9402), synth.photo(5, 4, synth.SEED0 + 9403)]


@pytest.mark.parametrize("host_out", (False, True))
def test_a_chunk_whose_frames_all_fail_the_kmeans_check(host_out):
    """no frame has a stream: nothing is placed, no place timer is recorded, no byte is written"""
    import cniic_amd
    expr = "voronoi(256)"
    imgs = tiny_images()[1:]          # fewer than 256 pixels each
    want = singles("all fail", expr, imgs)
    assert [s[0] for s in want] == [TOO_FEW_POINTS] * len(imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stream_len(256) + 1, host_out=host_out, poison=0xA5)
        assert ctx.kernel_time("vor_small_place")[1] == 0
    assert res[6] == len(imgs) and res[1] == [0] * len(imgs)
    check_against_singles(res, want, "all fail")
    assert bool((res[5] == 0xA5).all())


@pytest.mark.parametrize("host_out", (False, True))
def test_a_chunk_whose_frames_all_exceed_their_capacity(host_out):
    """every frame has a stream and none has the room: nothing is placed, no place timer is recorded, no byte is written"""
    import cniic_amd
    K = 16
    expr = "voronoi(%d)" % K
    imgs = tiny_images()
    want = singles("all short", expr, imgs)
    assert all(s[0] == 0 for s in want)
    stride = stream_len(K) - 1
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, expr, imgs, stride, host_out=host_out, poison=0xA5)
        assert ctx.kernel_time("vor_small_place")[1] == 0
    assert launches == len(imgs) and rc == CAPACITY and rcs == [CAPACITY] * len(imgs) and lens == [stream_len(K)] * len(imgs)
    assert msg == "encode: stream is %d bytes, capacity %d" % (stream_len(K), stride)
    for f, s in enumerate(want):
        assert {k: sts[f][k] for k in STATS} == {k: s[2][k] for k in STATS}, f
    assert bool((host == 0xA5).all())


@pytest.mark.parametrize("host_out", (False, True))
def test_a_frame_a_chunk(host_out, monkeypatch):
    """CNIIC_TEST_MEASURE_BUDGET=1: every frame is a chunk of its own, placed (device memory) or copied down (host memory) once per chunk"""
    import cniic_amd
    K = 16
    expr = "voronoi(%d)" % K
    imgs = tiny_images()
    want = singles("all short", expr, imgs)
    stride = stream_len(K) + 5
    monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride, host_out=host_out, poison=0xC3)
        assert ctx.kernel_time("vor_small_place")[1] == (0 if host_out else len(imgs))
    monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert res[6] == len(imgs)
    check_against_singles(res, want, "a frame a chunk")
    check_poison(res, stride, 0xC3, "a frame a chunk", routed(imgs))


def test_many_frames_in_one_launch():
    import cniic_amd
    rng = np.random.default_rng(43)
    expr = "voronoi(16)"
    sizes = [(8, 8), (9, 7), (16, 5), (24, 24), (13, 17), (31, 3), (4, 4), (20, 11)]
    imgs = []
    for f in range(3000):
        w, h = sizes[f % 8]
        imgs.append((rng.integers(0, 32, (h, w, 3)) * 8).astype(np.uint8))
    stride = stream_len(16) + 1
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, expr, imgs, stride, poison=0x11)
        assert launches == 3000 and rc == 0 and rcs == [0] * 3000 and lens == [stream_len(16)] * 3000
        assert bool((host.reshape(3000, stride)[:, -1] == 0x11).all())
        with cniic_amd.Context(0) as ref:
            for f in range(0, 3000, 75):
                src, sdata, sst = ref.encode(expr, imgs[f])
                assert src == 0 and streams[f] == sdata and {k: sts[f][k] for k in STATS} == {k: sst[k] for k in STATS}, f


def test_two_chunks_of_scratch(monkeypatch):
    import cniic_amd
    K = 16
    expr = "voronoi(%d)" % K
    imgs = all_images()
    want = singles(("all", K), expr, imgs)
    stride = stream_len(K) + 5
    with cniic_amd.Context(0) as ctx:
        one = batch(ctx, expr, imgs, stride)
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(8 * (((stream_len(K) + 15) & ~15) + 16 + 32)))   # eight frames a chunk: two chunks
        two = batch(ctx, expr, imgs, stride)
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")                                                 # a frame a chunk
        many = batch(ctx, expr, imgs, stride)
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    for res in (two, many):
        assert res[6] == len(imgs) - 2
        assert res[:5] == one[:5]
        check_against_singles(res, want, "chunks")


def test_a_frame_alone_and_in_company():
    import cniic_amd
    expr = "voronoi(100)"
    imgs = all_images()
    want = singles(("all", 100), expr, imgs)
    with cniic_amd.Context(0) as ctx:
        for f in (5, 10, CHECKER + 1):
            res = batch(ctx, expr, [imgs[f]], stream_len(100))
            assert res[6] == 1
            check_against_singles(res, [want[f]], "alone %d" % f)


def test_measure_batch_takes_the_route_for_its_small_frames():
    import math
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    expr = "voronoi(16)"
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 9300 + i) for i, (w, h) in enumerate(sizes)]
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
        stride = stream_len(16) + 8
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch(expr, src, offs, ws, hs, out, stride, allow=FAILURES)
        launches, dec_launches = ctx.kernel_time("vor_small_batch")[1], ctx.kernel_time("vor_small_dec_batch")[1]
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == 5 and dec_launches == 4      # (the 1 x 1 frame has no stream to decode)
        assert rc == TOO_FEW_POINTS
        host = out.cpu().numpy()
        for f in range(F):
            if rows_want[f] is None:
                assert rows[f]["rc"] == want[f][0] and math.isnan(rows[f]["error"]), f
                continue
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f], (f, got, rows_want[f])
            assert rows[f]["kmeans"]["iterations"] == want[f][2]["iterations"]
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f


def test_the_floor_keeps_few_heavy_frames_with_the_workers():
    """pixels x K of a frame against the number of candidate frames of the call; same bytes either way"""
    import cniic_amd
    from cniic_amd import synth
    K = 64
    expr = "voronoi(%d)" % K
    shapes = [(64, 64), (32, 32), (45, 45), (46, 45), (128, 96), (128, 97), (128, 128)] + [(20, 20)] * 121
    assert [w * h * K <= FLOOR_WORK_FEW for w, h in shapes[:7]] == [False, True, True, False, False, False, False]
    assert [w * h * K <= FLOOR_WORK_SOME for w, h in shapes[:7]] == [True, True, True, True, True, False, False]
    assert 128 * 96 * K == FLOOR_WORK_SOME and 45 * 45 * K < FLOOR_WORK_FEW < 46 * 45 * K and len(shapes) == FLOOR_MANY
    imgs = [(synth.uniform if i % 2 else synth.photo)(w, h, synth.SEED0 + 9400 + i) for i, (w, h) in enumerate(shapes)]
    want = singles("floor", expr, imgs)
    assert all(s[0] == 0 for s in want)
    stride = stream_len(K) + 3
    with cniic_amd.Context(0) as ctx:
        for count, routed_want in ((1, 0), (4, 2), (FLOOR_FEW - 1, 2), (FLOOR_FEW, 6), (FLOOR_MANY - 1, FLOOR_MANY - 3), (FLOOR_MANY, FLOOR_MANY)):
            res = batch(ctx, expr, imgs[:count], stride)
            assert res[6] == routed_want, (count, res[6], routed_want)
            check_against_singles(res, want[:count], "floor, %d frames" % count)
        res = batch(ctx, expr, imgs[1:3], stride)
        assert res[6] == 2
