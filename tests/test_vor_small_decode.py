"""Small `voronoi` frames of cniic_codec_decode_batch / cniic_codec_measure_batch on the small-frame decode route (k_vor_small.hip
k_vor_small_dec: a workgroup per frame, its centroids in LDS, the image in place; include/cniic_hip.h above cniic_codec_decode_batch).
Every comparison is exact: a frame's status, dimensions, pixels and message are those of cniic_codec_decode for that stream alone on a
context that has seen no batch, and the pixels are the oracle's decode.  Which frames took the route is read from the stage timer
"vor_small_dec_batch", whose launch count is the number of frames the route was given: on a build without the route that timer does not
exist.

The streams are those of tests/test_vor_small_batch.py's frames, and ones built by hand with `stream` below: K = 1 and K = 256, two
centroids equidistant from a row of pixels, duplicate centroids, centroids outside the image and with coordinates whose squares wrap in
32 bits; and the ones the route hands back to the single decode -- K = 257, K = 0, w h = 0, a centroid whose length word is 2, a list cut
by one byte, 15 bytes, an image that does not fit img_stride."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_PX = 16384        # kVorSmallMaxPx (cniic_amd/csrc/vor_small.hpp)
MAX_K = 256           # kVorSmallMaxK
OK, DECODE, CAPACITY = 0, -6, -8
TIMER = "vor_small_dec_batch"
POISON = 0xA5
WRAPS = (16384, 65536 + 3, 2 ** 31, 2 ** 32 - 1)


def stream_len(K):
    return 16 + 19 * K


def stream(w, h, cents, K=None, length_word=3):
    """VoronoiCluster's stream by hand: w, h as u32, K as u64, then per centroid x, y as u32, the u64 3 and r g b (clusterc.rs:156-164, 250-257)"""
    out = int(w).to_bytes(4, "little") + int(h).to_bytes(4, "little") + int(len(cents) if K is None else K).to_bytes(8, "little")
    for x, y, (r, g, b) in cents:
        out += int(x).to_bytes(4, "little") + int(y).to_bytes(4, "little") + int(length_word).to_bytes(8, "little") + bytes([r, g, b])
    return out


def colour(k):
    return ((k * 37 + 11) & 255, (k * 101 + 3) & 255, (k * 53 + 200) & 255)


def good_streams():
    """[(name, stream)]: every one decodes and takes the route"""
    rng = np.random.default_rng(77)
    res = [("K = 1", stream(9, 7, [(4, 3, (1, 2, 3))])),
           ("K = 256", stream(40, 30, [(int(rng.integers(0, 40)), int(rng.integers(0, 30)), colour(k)) for k in range(256)])),
           ("K = 256 on 128 x 128", stream(128, 128, [(int(rng.integers(0, 128)), int(rng.integers(0, 128)), colour(k)) for k in range(256)])),
           ("equidistant from a row", stream(11, 5, [(5, 0, (255, 0, 0)), (5, 4, (0, 255, 0))])),           # row y = 2: the first wins
           ("equidistant from a column", stream(11, 5, [(8, 2, (9, 9, 9)), (2, 2, (7, 7, 7)), (5, 9, (1, 1, 1))])),
           ("duplicates", stream(8, 8, [(3, 3, (10, 20, 30)), (3, 3, (40, 50, 60)), (6, 6, (70, 80, 90)), (6, 6, (1, 1, 1))])),
           ("outside the image", stream(16, 4, [(100, 2, (5, 5, 5)), (20, 50, (6, 6, 6)), (17, 0, (7, 7, 7))])),
           ("16384 x 1", stream(16384, 1, [(k * 997 % 16384, 0, colour(k)) for k in range(33)])),
           ("1 x 16384", stream(1, 16384, [(0, k * 613 % 16384, colour(k)) for k in range(200)]))]
    for v in WRAPS:   # the squares wrap: (c.x - x)^2 in u32 arithmetic
        res.append(("x = %d" % v, stream(24, 10, [(v, 5, (200, 0, 0)), (12, 5, (0, 200, 0)), (3, v, (0, 0, 200))])))
        res.append(("y = %d, alone" % v, stream(7, 13, [(2, v, (1, 2, 3)), (v, v, (4, 5, 6))])))
    res.append(("wrapping to a tie", stream(20, 3, [(65536 + 3, 1, (9, 0, 0)), (3, 1, (0, 9, 0)), (2 ** 31 + 10, 2 ** 31, (0, 0, 9)), (10, 0, (8, 8, 8))])))
    return res


def handed_back(img_stride):
    """[(name, stream)]: the route leaves each of these to the single decode"""
    good = stream(6, 5, [(1, 1, (10, 10, 10)), (4, 3, (20, 20, 20))])
    w_big = img_stride // 3 + 1
    return [("K = 257", stream(10, 10, [(k % 10, k // 26, colour(k)) for k in range(257)])),
            ("K = 0 with pixels", stream(4, 4, [])),
            ("w h = 0", stream(0, 9, [(1, 1, (3, 3, 3))])),
            ("w h = 0 and K = 0", stream(5, 0, [])),
            ("a length word of 2", stream(6, 5, [(1, 1, (10, 10, 10))], K=2) + stream(6, 5, [(4, 3, (20, 20, 20))], length_word=2)[16:]),
            ("a list cut by one byte", good[:-1]),
            ("K says more than there is", stream(6, 5, [(1, 1, (10, 10, 10))], K=2)),
            ("15 bytes", good[:15]),
            ("7 bytes", good[:7]),
            ("an image that does not fit", stream(w_big, 1, [(0, 0, (1, 1, 1))]))]


# ------------------------------------------------------------------ GPU helpers
def _last_error(ctx):
    return (ctx._L.cniic_last_error(ctx.h) or b"").decode()


_SINGLES = {}


def singles(key, streams, cap):
    """cniic_codec_decode of every stream alone (capacity cap), on a context that has seen no batch -> [(rc, w, h, pixels or None, message)]"""
    import cniic_amd
    if key not in _SINGLES:
        res = []
        with cniic_amd.Context(0) as ref:
            for s in streams:
                out = np.full(max(cap, 1), POISON, np.uint8)
                raw = np.frombuffer(bytes(s) + b"\0", np.uint8)
                rc, w, h = ref.decode_into("voronoi(1)", raw, len(s), out[:cap], allow=(DECODE, CAPACITY))
                res.append((rc, w, h, out[:w * h * 3].copy() if rc == 0 else None, _last_error(ref) if rc != 0 else ""))
        _SINGLES[key] = res
    return _SINGLES[key]


def aligned(nbytes, off, host, fill):
    """(buffer, at): an allocation of 16 + off + nbytes + 16 bytes of `fill` and the index in it whose address is off modulo 16"""
    import torch
    total = 16 + off + nbytes + 16
    buf = np.full(total, fill, np.uint8) if host else torch.full((total,), fill, dtype=torch.uint8, device=torch.device("cuda", 0))
    base = buf.ctypes.data if host else buf.data_ptr()
    return buf, (-base) % 16 + off


def batch(ctx, streams, img_stride, stride=None, host_src=False, host_out=False, src_off=0, out_off=0):
    """one cniic_codec_decode_batch call with the stage timers on -> (rc, ws, hs, rcs, output as a host array, routed frames, message).  The
    stream of frame f lies at src_off + f * stride modulo 16, its image at out_off + f * img_stride modulo 16, inside poisoned allocations.
    With a stride below a stream's length the streams lie on top of one another: each is written where the next one does not reach."""
    import torch
    from cniic_amd import _lib
    F = len(streams)
    lens = [len(s) for s in streams]
    stride = stride or ((max(lens) + 15) & ~15)
    room = stride * (F - 1) + max(lens)
    src, sat = aligned(room, src_off, True, 0)
    for f, s in enumerate(streams):
        src[sat + f * stride:sat + f * stride + len(s)] = np.frombuffer(s, np.uint8)
    if not host_src:
        dsrc, dat = aligned(room, src_off, False, 0)
        dsrc[dat:dat + room] = torch.from_numpy(src[sat:sat + room].copy()).to(dsrc.device)
        src, sat = dsrc, dat
    whole, at = aligned(img_stride * F, out_off, host_out, POISON)
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, ws, hs, rcs = ctx.decode_batch("voronoi(1)", src[sat:], stride, lens, F, whole[at:], img_stride, allow=(DECODE, CAPACITY))
        msg = _last_error(ctx) if rc != 0 else ""
        launches = ctx.kernel_time(TIMER)[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = whole if host_out else whole.cpu().numpy()
    assert bool((host[:at] == POISON).all()) and bool((host[at + img_stride * F:] == POISON).all())    # nothing before the first image or behind the last
    return rc, ws, hs, rcs, host[at:at + img_stride * F], launches, msg


def check_against_singles(res, want, img_stride, what):
    rc, ws, hs, rcs, host = res[:5]
    for f, (src, sw, sh, spx, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        slot = host[f * img_stride:(f + 1) * img_stride]
        if src == 0:
            assert (ws[f], hs[f]) == (sw, sh), (what, f)
            assert np.array_equal(slot[:sw * sh * 3], spx), (what, f)
            assert bool((slot[sw * sh * 3:] == POISON).all()), (what, f)          # nothing behind an image's end
        else:
            assert bool((slot == POISON).all()), (what, f)                          # a frame that fails leaves its destination alone
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first]), what
    if first is not None:
        assert res[6] == want[first][4], (what, res[6], want[first][4])


def takes(s, img_stride=1 << 40, max_px=MAX_PX):
    """whether the route takes the stream: the header and the whole, well-formed list, 1 <= K <= 256, 1 <= w h <= 16384, the image fits"""
    if len(s) < 16:
        return False
    w, h, K = int.from_bytes(s[0:4], "little"), int.from_bytes(s[4:8], "little"), int.from_bytes(s[8:16], "little")
    if not (1 <= K <= MAX_K and 1 <= w * h <= max_px and 3 * w * h <= img_stride and len(s) >= stream_len(K)):
        return False
    return all(int.from_bytes(s[16 + 19 * k + 8:16 + 19 * k + 16], "little") == 3 for k in range(K))


def check_against_the_oracle(streams, want):
    import oracle_lib as O
    for f, s in enumerate(streams):
        if want[f][0] == 0 and want[f][1] * want[f][2] > 0:
            rcd, back = O.decode("voronoi(1)", s)
            assert rcd == 0 and np.array_equal(back.reshape(-1), want[f][3]), f


_BATCH = {}


def batch_streams():
    """the streams of the frames of tests/test_vor_small_batch.py at K = 16 and K = 100, each encoded alone"""
    import cniic_amd
    import test_vor_small_batch as T
    if "s" not in _BATCH:
        res = []
        with cniic_amd.Context(0) as ref:
            for K in (16, 100):
                for im in T.all_images():
                    rc, data, _ = ref.encode("voronoi(%d)" % K, im, allow=T.FAILURES)
                    if rc == 0:
                        res.append(data)
        _BATCH["s"] = res
    return _BATCH["s"]


# ------------------------------------------------------------------ the tests
def test_the_streams_of_the_batch():
    import cniic_amd
    streams = batch_streams()
    img_stride = 3 * 160 * 120 + 7
    want = singles("batch", streams, img_stride)
    assert all(s[0] == 0 for s in want) and len(streams) >= 24
    check_against_the_oracle(streams, want)
    n_routed = sum(takes(s, img_stride) for s in streams)
    assert n_routed == len(streams) - 4                                # 5 x 3277 and 160 x 120 at either K go to the workers
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, streams, img_stride)
    assert res[5] == n_routed
    check_against_singles(res, want, img_stride, "batch streams")


def test_good_streams_by_hand_and_the_route_off(monkeypatch):
    import cniic_amd
    names, streams = zip(*good_streams())
    img_stride = 3 * MAX_PX
    want = singles("good", streams, img_stride)
    assert all(s[0] == 0 for s in want), [n for n, s in zip(names, want) if s[0] != 0]
    assert all(takes(s, img_stride) for s in streams)
    check_against_the_oracle(streams, want)
    row = want[names.index("equidistant from a row")][3].reshape(5, 11, 3)
    assert (row[2] == (255, 0, 0)).all() and (row[3] == (0, 255, 0)).all()                  # the first of two equal minima
    dup = want[names.index("duplicates")][3].reshape(8, 8, 3)
    assert {tuple(p) for p in dup.reshape(-1, 3)} == {(10, 20, 30), (70, 80, 90)}
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, streams, img_stride)
        monkeypatch.setenv("CNIIC_TEST_VOR_SMALL_DEC_OFF", "1")
        off = batch(ctx, streams, img_stride)
        assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0    # no launches: the stage is not there
        monkeypatch.delenv("CNIIC_TEST_VOR_SMALL_DEC_OFF")
        monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", "1,5,6")
        some = batch(ctx, streams, img_stride)
        monkeypatch.delenv("CNIIC_TEST_DECODE_BATCH_OFF")
    assert on[5] == len(streams) and off[5] == 0 and some[5] == len(streams) - 3
    assert on[:4] == off[:4] == some[:4] and np.array_equal(on[4], off[4]) and np.array_equal(on[4], some[4])
    check_against_singles(on, want, img_stride, "good streams")


@pytest.mark.parametrize("host_src", (False, True))
def test_streams_the_route_hands_back_among_good_ones(host_src):
    import cniic_amd
    img_stride = 3 * 40 * 30 + 5
    good = [s for n, s in good_streams() if takes(s, img_stride)]
    back = handed_back(img_stride)
    assert len(good) >= 8 and not any(takes(s, img_stride) for _, s in back)
    streams = []
    for i, (_, s) in enumerate(back):
        streams += [good[i % len(good)], s]
    streams.append(good[1])
    want = singles("mixed", streams, img_stride)
    by_name = {n: want[2 * i + 1] for i, (n, _) in enumerate(back)}
    assert by_name["K = 257"][0] == OK and by_name["w h = 0"][0] == OK and by_name["w h = 0 and K = 0"][0] == OK
    assert by_name["an image that does not fit"][0] == CAPACITY
    for n in ("K = 0 with pixels", "a length word of 2", "a list cut by one byte", "K says more than there is", "15 bytes", "7 bytes"):
        assert by_name[n][0] == DECODE and by_name[n][4], n
    assert all(want[2 * i][0] == OK for i in range(len(back)))
    check_against_the_oracle(streams, want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, streams, img_stride, host_src=host_src)
    assert res[5] == len(back) + 1                                     # the good ones, and no other
    check_against_singles(res, want, img_stride, "handed back")


@pytest.mark.parametrize("host_src,host_out", ((False, False), (True, False), (False, True), (True, True)))
def test_every_residue_and_both_memories(host_src, host_out):
    import cniic_amd
    streams = [s for _, s in good_streams() if takes(s, 3 * 24 * 10 + 16)] + [stream(5, 1, [(0, 0, (1, 2, 3)), (4, 0, (4, 5, 6))]), stream(1, 1, [(0, 0, (9, 8, 7))])]
    assert len(streams) >= 10
    with cniic_amd.Context(0) as ctx:
        for off in range(16):
            img_stride = 3 * 24 * 10 + 16 + (off * 7) % 16                 # the images' phases differ from frame to frame
            want = singles(("residues", img_stride), streams, img_stride)
            assert all(s[0] == 0 for s in want)
            res = batch(ctx, streams, img_stride, stride=(max(len(s) for s in streams) + off), host_src=host_src, host_out=host_out, src_off=(5 * off) % 16, out_off=off)
            assert res[5] == len(streams)
            check_against_singles(res, want, img_stride, "residue %d" % off)


@pytest.mark.parametrize("host_src", (False, True))
def test_a_stride_below_the_streams_length(host_src):
    """streams on top of one another: in device memory the route sees a head cut at the stride, and the single decode answers; in host
    memory every stream is read where it lies, as the single decode reads it"""
    import cniic_amd
    K = 3     # (a stream's last record is then its successor's first 19 bytes -- w, h, K -- and K = 3 reads as the length word)
    streams = [stream(12, 9, [((f + 3 * k) % 12, (f + k) % 9, colour(f + k)) for k in range(K)]) for f in range(6)]
    stride = stream_len(K) - 19
    lens = [len(s) for s in streams]
    flat = bytearray(stride * 5 + lens[5])
    for f, s in enumerate(streams):
        flat[f * stride:f * stride + len(s)] = s
    seen = [bytes(flat[f * stride:f * stride + lens[f]]) for f in range(6)]     # what a decode of frame f reads: its successor lies over its tail
    img_stride = 3 * 12 * 9
    want = singles("overlap", seen, img_stride)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, streams, img_stride, stride=stride, host_src=host_src)
    assert res[5] == (6 if host_src else 0)                                 # in device memory no head is whole: a look is never wider than the stride
    check_against_singles(res, want, img_stride, "overlap")


def test_many_frames_in_one_launch():
    import cniic_amd
    rng = np.random.default_rng(91)
    sizes = [(8, 8), (9, 7), (16, 5), (24, 24), (13, 17), (31, 3), (4, 4), (20, 11)]
    streams = []
    for f in range(3000):
        w, h = sizes[f % 8]
        K = 1 + f % 19
        streams.append(stream(w, h, [(int(rng.integers(0, w + 3)), int(rng.integers(0, h + 3)), colour(f + k)) for k in range(K)]))
    img_stride = 3 * 24 * 24 + 1
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, streams, img_stride)
    assert res[5] == 3000 and res[0] == 0 and res[3] == [0] * 3000
    picks = list(range(0, 3000, 75))
    want = singles("many", [streams[f] for f in picks], img_stride)
    check_against_the_oracle([streams[f] for f in picks], want)
    host = res[4]
    for f in range(3000):
        w, h = sizes[f % 8]
        assert (res[1][f], res[2][f]) == (w, h) and bool((host[f * img_stride + 3 * w * h:(f + 1) * img_stride] == POISON).all()), f
    for j, f in enumerate(picks):
        assert np.array_equal(host[f * img_stride:f * img_stride + want[j][3].size], want[j][3]), f


def test_two_chunks_of_scratch(monkeypatch):
    import cniic_amd
    names, streams = zip(*good_streams())
    img_stride = 3 * MAX_PX
    want = singles("good", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        for budget in ("20000", "1"):
            monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", budget)
            for host_out in (False, True):
                res = batch(ctx, streams, img_stride, host_out=host_out)
                assert res[5] == len(streams)
                check_against_singles(res, want, img_stride, "budget " + budget)
            monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")


def test_mutants_behave_as_the_single_decode_does():
    import cniic_amd
    rng = np.random.default_rng(20241019)
    bases = [stream(8, 8, [(1, 1, (10, 20, 30)), (6, 2, (40, 50, 60)), (3, 7, (70, 80, 90))]),
             stream(37, 29, [(k * 5 % 37, k * 7 % 29, colour(k)) for k in range(12)])]
    streams = []
    for k in range(200):
        s = bytearray(bases[k % 2])
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, 16)) if rng.integers(0, 6) == 0 else int(rng.integers(0, len(s)))     # a sixth of them in the header
            s[at] = int(rng.integers(0, 256))
        if k % 10 == 9:
            s = s[:int(rng.integers(0, len(s)))]
        streams.append(bytes(s))
    img_stride = 3 * 37 * 29 + 13
    want = singles("mutants", streams, img_stride)
    n_ok, n_bad = sum(s[0] == 0 for s in want), sum(s[0] != 0 for s in want)
    n_routed = sum(takes(s, img_stride) for s in streams)
    print("mutants: %d decode, %d fail, %d on the route" % (n_ok, n_bad, n_routed))
    assert n_ok >= 30 and n_bad >= 20 and 30 <= n_routed < 200
    check_against_the_oracle(streams, want)
    with cniic_amd.Context(0) as ctx:
        for host_src in (False, True):
            res = batch(ctx, streams, img_stride, stride=((len(bases[1]) + 15) & ~15), host_src=host_src)
            assert res[5] == n_routed
            check_against_singles(res, want, img_stride, "mutants")
