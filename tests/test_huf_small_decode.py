"""Small `hufman` and `cluster-colors` frames of cniic_codec_decode_batch / cniic_codec_measure_batch on the small-frame decode route
(k_huf_small_dec in k_delta_small_dec.hip: a workgroup per frame from the payload to the pixels in place; include/cniic_hip.h above
cniic_codec_decode_batch).  Every comparison is exact: a frame's status, dimensions, pixels and message are those of cniic_codec_decode
for that stream alone on a context that has seen no batch; `hufman` frames are also the source image.  Which frames took the route is
read from the stage timer "huf_small_dec_batch", whose launch count is the number of frames given to the kernel (a frame it hands back
included): on a build without the route that timer does not exist.

The streams are the library's own (tests/test_huf_small_batch.py holds them to the oracle's), cut, edited or built by hand where a test
says so.  The mutants are inputs a decoder must refuse or decode identically; no test here is meant to make anything fail but a decode."""
import functools

import numpy as np
import pytest

import test_delta_small_decode as D
import test_huf_small_batch as T
from test_delta_small_decode import aligned, check_against_singles, singles

pytestmark = pytest.mark.gpu

MAX_PX = T.MAX_PX
MAX_CODE_LEN = T.MAX_CODE_LEN
OK, DECODE, CAPACITY = D.OK, D.DECODE, D.CAPACITY
TIMER, ENC_TIMER, OLD_TIMER = "huf_small_dec_batch", "huf_small_batch", "decode_batch_pass"
MSG_SHORT = "Failed to decode symbol"
POISON = D.POISON


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor (a call with few small frames keeps the batched route); test_the_floor holds it"""
    monkeypatch.setenv("CNIIC_TEST_HUF_SMALL_FLOOR_OFF", "1")


# ------------------------------------------------------------------ images and streams
@functools.lru_cache(maxsize=None)
def route_images():
    """the routed frames of the encode tests: shaped (1 .. 16 384 pixels), the chain, the powers, 16 384 leaves, one colour, the channels'
    ends, the four tied colours, and the sizes around the kernel's thresholds"""
    return T.shaped_images()[:11] + T.further_images() + T.sized_images()


def leaf(c):
    return b"\x00" + (3).to_bytes(8, "little") + bytes(c)


def serialise(tree):
    """tree: a colour (r, g, b) or a pair of trees -> the pre-order trie"""
    return leaf(tree) if len(tree) == 3 else b"\x01" + serialise(tree[0]) + serialise(tree[1])


def codes_of(tree, prefix=""):
    return {tuple(tree): prefix} if len(tree) == 3 else {**codes_of(tree[0], prefix + "0"), **codes_of(tree[1], prefix + "1")}


def hand_stream(w, h, tree, pixels):
    codes = codes_of(tree)
    bits = "".join(codes[tuple(p)] for p in pixels)
    bits += "0" * (-len(bits) % 8)
    return w.to_bytes(4, "little") + h.to_bytes(4, "little") + serialise(tree) + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def deep_stream():
    """a trie one level deeper than the route takes: a chain of 21 leaves (depths 1, 2, ..., 19, 20, 20); 8 x 8 pixels, the first the deepest leaf"""
    tree = ((7, 8, 9), (20, 0, 0))
    for k in range(19, 0, -1):
        tree = ((k, 0, 0), tree)
    assert max(len(c) for c in codes_of(tree).values()) == 20 and len(codes_of(tree)) == 21
    return hand_stream(8, 8, tree, [(7, 8, 9)] + [(1, 0, 0)] * 63)


def balanced(cols):
    return cols[0] if len(cols) == 1 else (balanced(cols[:len(cols) // 2]), balanced(cols[len(cols) // 2:]))


def leafy_stream():
    """100 leaves in front of 64 pixels: more leaves than the frame has symbols"""
    cols = [(k, 255 - k, k // 2) for k in range(100)]
    return hand_stream(8, 8, balanced(cols), [cols[(7 * d) % 100] for d in range(64)])


def parse_trie(data):
    """-> (leaves [(offset of the tag, depth)], offset of the payload)"""
    pos, leaves, pending = 8, [], [0]
    while pending:
        depth = pending.pop()
        tag = data[pos]
        if tag == 1:
            pos += 1
            pending += [depth + 1, depth + 1]
        else:
            assert tag == 0
            leaves.append((pos, depth))
            pos += 12
    return leaves, pos


_ENC = {}


def encoded(key, expr, imgs):
    """the library's own streams of imgs, each encoded alone (b"" where the encode fails: too few colours for K); computed once per key"""
    import cniic_amd
    from cniic_amd import _lib
    if key not in _ENC:
        with cniic_amd.Context(0) as ref:
            res = []
            for im in imgs:
                rc, data, _ = ref.encode(expr, im, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
                res.append(data if rc == 0 else b"")
        _ENC[key] = res
    return _ENC[key]


def batch(ctx, expr, streams, img_stride, stride=None, host_src=False, host_out=False, src_off=0, out_off=0):
    """one cniic_codec_decode_batch call with the stage timers on -> (rc, ws, hs, rcs, output as a host array, frames given to the kernel,
    message, launches of the batched route for larger frames); buffers as in tests/test_delta_small_decode.py"""
    import torch
    from cniic_amd import _lib
    F = len(streams)
    lens = [len(s) for s in streams]
    stride = stride or ((max(lens) + 15) & ~15)
    src, sat = aligned(stride * F, src_off, True, 0)
    for f, s in enumerate(streams):
        src[sat + f * stride:sat + f * stride + len(s)] = np.frombuffer(s, np.uint8)
    if not host_src:
        dsrc, dat = aligned(stride * F, src_off, False, 0)
        dsrc[dat:dat + stride * F] = torch.from_numpy(src[sat:sat + stride * F].copy()).to(dsrc.device)
        src, sat = dsrc, dat
    whole, at = aligned(img_stride * F, out_off, host_out, POISON)
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, ws, hs, rcs = ctx.decode_batch(expr, src[sat:], stride, lens, F, whole[at:], img_stride, allow=(DECODE, CAPACITY))
        msg = D._last_error(ctx) if rc != 0 else ""
        launches, old = ctx.kernel_time(TIMER)[1], ctx.kernel_time(OLD_TIMER)[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = whole if host_out else whole.cpu().numpy()
    assert bool((host[:at] == POISON).all()) and bool((host[at + img_stride * F:] == POISON).all())
    return rc, ws, hs, rcs, host[at:at + img_stride * F], launches, msg, old


def small(streams, max_px=MAX_PX):
    return sum(1 for s in streams if len(s) >= 8 and 1 <= int.from_bytes(s[0:4], "little") * int.from_bytes(s[4:8], "little") <= max_px)


# ------------------------------------------------------------------ the tests
def test_route_and_bytes():
    import cniic_amd
    imgs = route_images()
    streams = encoded("route", "hufman", imgs)
    img_stride = 3 * MAX_PX
    want = singles(("huf", "route"), "hufman", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "hufman", streams, img_stride)
        assert res[5] == len(imgs) == small(streams) and res[7] == 0
        check_against_singles(res, want, img_stride, "hufman", sources=imgs)
        both = encoded("above", "hufman", T.shaped_images()[11:])          # 16 385 and 19 200 pixels ride along on the route they had
        res = batch(ctx, "hufman", streams[:6] + both, 3 * 19200)
        assert res[5] == 6 and res[7] > 0
        check_against_singles(res, want[:6] + singles(("huf", "above"), "hufman", both, 3 * 19200), 3 * 19200, "with larger frames", sources=imgs[:6] + T.shaped_images()[11:])


def test_limits_alone_and_in_company():
    """one leaf, two leaves, the 19-bit chain and 16 384 leaves: alone the launch's LDS follows the frame, in company it is the bound's"""
    import cniic_amd
    all_imgs = route_images()
    pick = [0, 1, 11, 13, 14, 15]      # 1 x 1 (one leaf), 1 x 2 (two), chain, distinct, one_pixel, flat
    imgs = [all_imgs[k] for k in pick]
    streams = [encoded("route", "hufman", all_imgs)[k] for k in pick]
    assert [len(parse_trie(s)[0]) for s in streams] == [1, 2, 20, 16384, 1, 1] and max(d for _, d in parse_trie(streams[2])[0]) == MAX_CODE_LEN
    img_stride = 3 * MAX_PX + 5
    want = singles(("huf", "limits"), "hufman", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        for f in range(len(streams)):
            res = batch(ctx, "hufman", streams[f:f + 1], img_stride)
            assert res[5] == 1, f
            check_against_singles(res, want[f:f + 1], img_stride, "alone %d" % f, sources=imgs[f:f + 1])
        res = batch(ctx, "hufman", streams, img_stride)
        assert res[5] == len(streams)
        check_against_singles(res, want, img_stride, "company", sources=imgs)


@pytest.mark.parametrize("K", (2, 16, 256))
def test_cluster_colors_streams(K):
    """a cluster-colors stream is a Hufman stream of palette colours: flat frames (one leaf where the encode succeeds), few colours, photos"""
    import cniic_amd
    from cniic_amd import synth
    yy, xx = np.mgrid[0:24, 0:31]
    checker = np.where(((xx + yy) & 1)[..., None] == 1, np.array([200, 30, 40], np.uint8), np.array([10, 220, 90], np.uint8)).astype(np.uint8)
    four = np.array([(9, 9, 9), (250, 1, 1), (1, 250, 1), (1, 1, 250)], np.uint8)[(xx // 8 + yy // 8) % 4]
    imgs = [np.full((20, 30, 3), 77, np.uint8), checker, four, synth.photo(32, 32, synth.SEED0 + 9000 + K), synth.photo(100, 75, synth.SEED0 + 9001 + K),
            synth.uniform(128, 128, synth.SEED0 + 9002 + K), synth.photo(1, 1, 5)]
    expr = "cluster-colors(%d)" % K
    streams = encoded(("cc", K), expr, imgs)
    assert sum(1 for s in streams if s) >= 3       # (a frame with fewer colours than K has no stream: an empty one, which fails the same either way)
    img_stride = 3 * MAX_PX + 3
    want = singles(("cc", K), expr, streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, streams, img_stride)
        assert res[5] == small(streams) == sum(1 for s in streams if s) and res[7] == 0
        check_against_singles(res, want, img_stride, expr)
        hres = batch(ctx, expr, streams, img_stride, host_src=True, host_out=True)
        assert hres[5] == res[5]
        check_against_singles(hres, want, img_stride, expr + ", host")


def test_hand_serialised_streams():
    """a 20-bit code is outside the route (the batched route for larger frames takes it); 100 leaves for 64 pixels is a decoder like another"""
    import cniic_amd
    good = encoded("route", "hufman", route_images())[5]
    streams = [good, deep_stream(), leafy_stream(), good]
    img_stride = 3 * 64 + 1
    want = singles(("huf", "hand"), "hufman", streams, img_stride)
    assert [s[0] for s in want] == [0, 0, 0, 0]
    assert want[1][3][:3].tolist() == [7, 8, 9] and want[1][3][3:6].tolist() == [1, 0, 0] and want[2][3][:6].tolist() == [0, 255, 0, 7, 248, 3]
    with cniic_amd.Context(0) as ctx:
        for host in (False, True):
            res = batch(ctx, "hufman", streams, img_stride, host_src=host, host_out=host)
            assert res[5] == 3 and res[7] > 0, (res[5], res[7])      # all but the 20-bit one
            check_against_singles(res, want, img_stride, "hand-made")


def failure_streams(good):
    leaves, pay = parse_trie(good)
    assert len(leaves) >= 4 and len(good) - pay >= 8
    tag_at, len_at = leaves[1][0], leaves[2][0] + 1
    return [
        ("good", good, OK, True),
        ("cut in the dimensions", good[:5], DECODE, False),
        ("cut in the trie", good[:8 + 20], DECODE, False),
        ("good again", good, OK, True),
        ("cut in half", good[:pay + (len(good) - pay) // 2], DECODE, True),
        ("one byte short", good[:-1], DECODE, True),
        ("one byte more", good + b"\x5a", OK, True),
        ("a tag of 2", good[:tag_at] + b"\x02" + good[tag_at + 1:], DECODE, False),
        ("a symbol of 4 bytes", good[:len_at] + b"\x04" + good[len_at + 1:], DECODE, False),
        ("good at the end", good, OK, True),
    ]


@pytest.mark.parametrize("host", (False, True))
def test_failures_among_good_frames(host):
    import cniic_amd
    good = encoded("route", "hufman", route_images())[4]      # 7 x 9, 63 colours
    cases = failure_streams(good)
    streams = [c[1] for c in cases]
    img_stride = 3 * 63 + 7
    want = singles(("huf", "failures"), "hufman", streams, img_stride)
    for (name, s, rc, _), (src, sw, sh, spx, smsg) in zip(cases, want):
        assert src == rc, (name, src, smsg)
    assert want[4][4] == want[5][4] == MSG_SHORT
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "hufman", streams, img_stride, host_src=host, host_out=host)
        assert res[5] == sum(c[3] for c in cases)
        check_against_singles(res, want, img_stride, "failures")          # a failing frame's destination untouched, the others complete
        for first in (4, 5, 7, 8):                                        # each failure first in a batch: its message
            res = batch(ctx, "hufman", streams[first:], img_stride, host_src=host, host_out=host)
            check_against_singles(res, want[first:], img_stride, cases[first][0])


@pytest.mark.parametrize("host_src,host_out", ((False, False), (True, True), (False, True), (True, False)))
def test_destinations_and_payloads_at_every_alignment(host_src, host_out):
    import cniic_amd
    keep = [k for k, im in enumerate(route_images()) if im.shape[0] * im.shape[1] <= 2049]
    imgs = [route_images()[k] for k in keep]
    streams = [encoded("route", "hufman", route_images())[k] for k in keep]
    imgs, streams = (imgs * 2)[:32], (streams * 2)[:32]
    img_stride = 3 * 2049 + 2                                             # odd: the images start at every residue modulo 16
    stride = ((max(len(s) for s in streams) + 3) & ~3) + 1                # odd: the streams at every byte shift
    assert {(f * img_stride) % 16 for f in range(32)} == set(range(16))
    pays = [parse_trie(s)[1] for s in streams]
    assert {(f * stride + p) % 4 for f, p in enumerate(pays) if len(streams[f]) > p} == set(range(4))
    want = singles(("huf", "align"), "hufman", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        for src_off, out_off in ((0, 0), (1, 7), (3, 15)):
            res = batch(ctx, "hufman", streams, img_stride, stride=stride, host_src=host_src, host_out=host_out, src_off=src_off, out_off=out_off)
            assert res[5] == 32
            check_against_singles(res, want, img_stride, (host_src, host_out, src_off, out_off), sources=imgs)


def test_device_streams_wider_than_one_group_of_the_second_look():
    """1200 device streams of 128 x 128 frames, up to 241 671 bytes each: the first look (8 KiB a frame) ends inside every decoder, and the
    pinned block holds 1110 rows at the full width, so the second look takes two groups.  Every frame is routed."""
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    kinds = [T.further_images()[2], synth.photo(128, 128, synth.SEED0 + 9100), synth.uniform(128, 128, synth.SEED0 + 9101), synth.photo(128, 128, synth.SEED0 + 9102)]
    ks = encoded("wide", "hufman", kinds)
    F = 1200
    stride = (max(len(s) for s in ks) + 15) & ~15
    assert (256 << 20) // stride < F and min(len(s) for s in ks) > 3 * 8192
    one = np.zeros(4 * stride, np.uint8)
    for k, s in enumerate(ks):
        one[k * stride:k * stride + len(s)] = np.frombuffer(s, np.uint8)
    src = torch.from_numpy(one).to(dev).repeat(F // 4)
    lens = [len(ks[f % 4]) for f in range(F)]
    img_stride = 3 * MAX_PX
    out = torch.full((img_stride * F,), POISON, dtype=torch.uint8, device=dev)
    with cniic_amd.Context(0) as ctx:
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, ws, hs, rcs = ctx.decode_batch("hufman", src, stride, lens, F, out, img_stride)
        launches, old = ctx.kernel_time(TIMER)[1], ctx.kernel_time(OLD_TIMER)[1]
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert rc == 0 and rcs == [0] * F and ws == [128] * F and hs == [128] * F and (launches, old) == (F, 0)
    got = out.reshape(F // 4, 4, img_stride)
    for k, im in enumerate(kinds):
        assert bool((got[:, k, :] == torch.from_numpy(im.reshape(-1)).to(dev)).all()), k


def test_the_floor(monkeypatch):
    """a call with fewer than DEC_FLOOR_FRAMES small frames keeps the batched route for them (NOTES AF); larger frames do not count"""
    import cniic_amd
    monkeypatch.delenv("CNIIC_TEST_HUF_SMALL_FLOOR_OFF")
    N = T.DEC_FLOOR_FRAMES
    pick = [f % 8 for f in range(N)] + [8, 9]                           # the first eight small frames in turn, then 16 385 and 19 200 pixels
    kinds = route_images()[:8] + T.shaped_images()[11:]
    kstreams = encoded("route", "hufman", route_images())[:8] + encoded("above", "hufman", T.shaped_images()[11:])
    img_stride = 3 * 19200
    kwant = singles(("huf", "floor"), "hufman", kstreams, img_stride)
    imgs, streams, want = [kinds[k] for k in pick], [kstreams[k] for k in pick], [kwant[k] for k in pick]
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "hufman", streams[1:], img_stride)             # N - 1 small frames and two larger ones
        assert res[5] == 0 and res[7] > 0
        check_against_singles(res, want[1:], img_stride, "below the floor", sources=imgs[1:])
        res = batch(ctx, "hufman", streams, img_stride)
        assert res[5] == N and res[7] > 0
        check_against_singles(res, want, img_stride, "at the floor", sources=imgs)


def test_frames_named_by_decode_batch_off(monkeypatch):
    import cniic_amd
    imgs = route_images()[:11]
    streams = encoded("route", "hufman", route_images())[:11]
    img_stride = 3 * MAX_PX
    want = singles(("huf", "route"), "hufman", encoded("route", "hufman", route_images()), img_stride)[:11]
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", "0,3,10")
        res = batch(ctx, "hufman", streams, img_stride)
        monkeypatch.delenv("CNIIC_TEST_DECODE_BATCH_OFF")
    assert res[5] == 8
    check_against_singles(res, want, img_stride, "three frames off", sources=imgs)


def test_the_hand_back(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    imgs = [synth.uniform(128, 128, synth.SEED0 + 9200), synth.photo(64, 64, synth.SEED0 + 9201), np.zeros((9, 9, 3), np.uint8)]
    streams = encoded("handback", "hufman", imgs)
    img_stride = 3 * MAX_PX + 1
    want = singles(("huf", "handback"), "hufman", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_DEC_ROUNDS", "1")
        res = batch(ctx, "hufman", streams, img_stride)
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_DEC_ROUNDS")
        assert res[5] == 3                       # the launch took all three; the caller's single decode answered for what it handed back
        check_against_singles(res, want, img_stride, "one round", sources=imgs)
        res = batch(ctx, "hufman", streams, img_stride)
        assert res[5] == 3
        check_against_singles(res, want, img_stride, "all rounds", sources=imgs)


def test_route_off_and_a_lowered_bound(monkeypatch):
    import cniic_amd
    imgs = route_images()
    streams = encoded("route", "hufman", imgs)
    img_stride = 3 * MAX_PX
    want = singles(("huf", "route"), "hufman", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, "hufman", streams, img_stride)
        monkeypatch.setenv("CNIIC_TEST_HUF_SMALL_DEC_OFF", "1")
        off = batch(ctx, "hufman", streams, img_stride)
        assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0    # no launches: the stage is not there
        monkeypatch.delenv("CNIIC_TEST_HUF_SMALL_DEC_OFF")
        monkeypatch.setenv("CNIIC_TEST_HUF_SMALL_DEC_MAX_PX", "4096")
        low = batch(ctx, "hufman", streams, img_stride)
        monkeypatch.delenv("CNIIC_TEST_HUF_SMALL_DEC_MAX_PX")
    assert on[5] == len(imgs) and off[5] == 0 and off[7] > 0 and low[5] == small(streams, 4096) < on[5]
    for res, what in ((off, "route off"), (low, "bound 4096")):
        assert on[:4] == res[:4] and np.array_equal(on[4], res[4]), what
        check_against_singles(res, want, img_stride, what, sources=imgs)


def test_two_chunks_of_scratch(monkeypatch):
    import cniic_amd
    keep = [k for k, im in enumerate(route_images()) if im.shape[0] * im.shape[1] <= 2049]
    imgs = [route_images()[k] for k in keep]
    streams = [encoded("route", "hufman", route_images())[k] for k in keep]
    img_stride = 3 * 2049 + 1
    want = singles(("huf", "chunks"), "hufman", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    tables = [8 * len(parse_trie(s)[0]) + 60 for s in streams]           # a leaf's two words, the row, the status word
    budget = sum(tables) // 2 + max(tables)
    assert max(tables) < budget < sum(tables)
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        res = batch(ctx, "hufman", streams, img_stride)
        hres = batch(ctx, "hufman", streams, img_stride, host_src=True, host_out=True)
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert res[5] == hres[5] == len(streams)
    check_against_singles(res, want, img_stride, "two chunks", sources=imgs)
    check_against_singles(hres, want, img_stride, "two chunks, host", sources=imgs)


def test_measure_batch_takes_both_routes():
    """encode, decode and MSE of a folder in one call: equal to the loop of the three single calls, both halves' timers readable afterwards;
    the small cluster-colors frames get their decode half too"""
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 9300 + i) for i, (w, h) in enumerate(sizes)]
    offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
    for expr, enc_timer, lossless in (("hufman", ENC_TIMER, True), ("cluster-colors(256)", "cc_small_batch", False)):
        with cniic_amd.Context(0) as ctx:
            rows_want, streams = [], []
            for im in imgs:
                rc, data, _ = ctx.encode(expr, im, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
                streams.append(data if rc == 0 else None)
                if rc != 0:
                    rows_want.append(None)
                    continue
                rc2, back = ctx.decode(expr, data)
                assert rc2 == 0 and (not lossless or np.array_equal(back, im))
                npx = im.shape[0] * im.shape[1]
                rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
            ok = [f for f in range(len(imgs)) if streams[f] is not None]
            stride = ((max(len(streams[f]) for f in ok) + 3) & ~3) + 8
            out = torch.zeros(stride * len(imgs), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
            rc, rows, lens = ctx.measure_batch(expr, src, offs, [s[0] for s in sizes], [s[1] for s in sizes], out, stride, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
            enc_launches, dec_launches = ctx.kernel_time(enc_timer)[1], ctx.kernel_time(TIMER)[1]
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
            small_ok = sum(1 for f in ok if sizes[f][0] * sizes[f][1] <= MAX_PX)
            assert enc_launches == 5 and dec_launches == small_ok >= 3, (expr, enc_launches, dec_launches)
            host = out.cpu().numpy()
            for f in ok:
                got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
                assert got == rows_want[f], (expr, f, got, rows_want[f])
                assert lens[f] == len(streams[f]) and host[f * stride:f * stride + lens[f]].tobytes() == streams[f], (expr, f)


MUTANTS = 200
MUTANT_STRIDE = 3 * 37 * 29 + 13


def mutant_streams(base_small, base_large):
    """200 streams: an 8 x 8 and a 37 x 29 stream in turn, one to three random bytes of each replaced; every second pair of edits falls
    behind the decoder, where a stream stays one the route takes"""
    rng = np.random.default_rng(20241020)
    out = []
    for k in range(MUTANTS):
        s = bytearray(base_large if k % 2 else base_small)
        lo = parse_trie(bytes(s))[1] if k % 4 >= 2 else 0
        for _ in range(int(rng.integers(1, 4))):
            s[int(rng.integers(lo, len(s)))] = int(rng.integers(0, 256))
        out.append(bytes(s))
    return out


def test_mutants():
    """a differential check on whatever the edits produce: every status the single decode's, and where that is 0 the pixels too"""
    import cniic_amd
    from cniic_amd import synth
    bases = encoded("mutants", "hufman", [synth.photo(8, 8, synth.SEED0 + 9400), synth.photo(37, 29, synth.SEED0 + 9401)])
    streams = mutant_streams(*bases)
    want_all = singles(("huf", "mutants"), "hufman", streams, MUTANT_STRIDE)
    keep = [k for k, s in enumerate(want_all) if s[0] in (OK, DECODE)]
    held = [(k, want_all[k][0]) for k in range(MUTANTS) if k not in keep]
    print("mutants held back (index, status of the single decode):", held)
    assert len(held) <= MUTANTS // 20
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "hufman", [streams[k] for k in keep], MUTANT_STRIDE)
    want = [want_all[k] for k in keep]
    for f, (src, sw, sh, spx, smsg) in enumerate(want):
        assert res[3][f] == src, (keep[f], res[3][f], src)
        slot = res[4][f * MUTANT_STRIDE:(f + 1) * MUTANT_STRIDE]
        if src == 0:
            assert (res[1][f], res[2][f]) == (sw, sh) and np.array_equal(slot[:sw * sh * 3], spx), keep[f]
        else:
            assert bool((slot == POISON).all()), keep[f]
    print("mutants on the route:", res[5], "of", len(keep))
    assert res[5] >= MUTANTS // 4
