"""Small `hilbert(rle)` and `hilbert(rle(d))` frames of a batch call on the small-frame route (k_rle_small.hip: a workgroup per frame from
the pixels to the finished stream; include/cniic_hip.h above cniic_codec_encode_batch_var).  Every comparison is exact: a frame's status,
length, bytes and message are those of cniic_codec_encode_opts for that frame alone on a context that has seen no batch, and the bytes are
the oracle's (d == 0) or those of rle_approx_ref.encode_py on the oracle's linearisation (d != 0).  Which frames took the route is read
from the stage timer "rle_small_batch", whose launch count is the number of routed frames: on a build without the route that timer does
not exist.

Every case states, from that restatement alone and before any GPU call, the property it is named for (CLAIMS and the asserts beside the
images); tests/test_rle_small_cpu.py recomputes the claimed run counts and stream lengths without a GPU."""
import math

import numpy as np
import pytest

import rle_approx_ref as R
import test_delta_small_batch as D
from test_delta_small_batch import _pack, _round4, check_against_singles

pytestmark = pytest.mark.gpu

MAX_PX = 16384             # kRleSmallMaxPx (cniic_amd/csrc/rle_small.hpp)
MAX_RUN = 255              # kRleSmallMaxRun
PIECE = 256                # kRleSmallPiece: phase c's pieces
THREADS = 1024             # kRsThreads (k_rle_small.hip)
STRIDE_AT_BOUND = 196624   # rs_stride(16384)
TIMER, PLACE = "rle_small_batch", "rle_small_place"
KNOB_OFF, KNOB_MAX_PX, KNOB_FLOOR_OFF = "CNIIC_TEST_RLE_SMALL_OFF", "CNIIC_TEST_RLE_SMALL_MAX_PX", "CNIIC_TEST_RLE_SMALL_FLOOR_OFF"
FAILURES, CAPACITY = D.FAILURES, D.CAPACITY
POISON = 0xA5
# the floor (capi.cpp): in a call with fewer than FLOOR_NONE candidate frames none takes the route, with fewer than FLOOR_FRAMES only those
# of at most FLOOR_PX pixels do
FLOOR_NONE, FLOOR_FRAMES, FLOOR_PX = 4, 32, 4096
D_ALL = [0.0, -0.0] + R.D_VALUES
D_BIG = [0.0, 4.0, 441.7, math.inf, -1.0]       # on the 16 384-pixel frames
ROWS = [254, 255, 256, 257, 510, 511, 1023, 1024, 1025, 16383, 16384]
RECTS = [(128, 128), (64, 64), (100, 75), (128, 96), (37, 41)]   # two table scans, three general rectangles
UNROUTED = [(16385, 1), (160, 120)]
A, B = (16, 16, 16), (240, 240, 240)            # the flat colour and the odd pixel


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor (few large frames stay with the workers); test_the_floor holds it"""
    monkeypatch.setenv(KNOB_FLOOR_OFF, "1")


def expr_of(d):
    return "hilbert(rle)" if d == 0.0 and not math.copysign(1.0, d) < 0 else "hilbert(rle(%r))" % float(d)


# ---- images laid along the scan
_ORDER = {}


def scan_order(w, h):
    """(n, 2) of (x, y): the pixel at every position of the oracle's scan"""
    import oracle_lib as O
    if (w, h) not in _ORDER:
        k = np.arange(w * h, dtype=np.uint32).reshape(h, w)
        lin = O.hilbert_linearize(np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8)).astype(np.uint32)
        idx = (lin[:, 0] << 16) | (lin[:, 1] << 8) | lin[:, 2]
        assert sorted(idx.tolist()) == list(range(w * h))
        _ORDER[(w, h)] = np.stack([idx % w, idx // w], 1)
    return _ORDER[(w, h)]


def along_scan(w, h, lin):
    """the w x h image whose linearisation is lin"""
    xy = scan_order(w, h)
    img = np.zeros((h, w, 3), np.uint8)
    img[xy[:, 1], xy[:, 0]] = np.asarray(lin, np.uint8).reshape(-1, 3)
    return img


def lin_flat(n):
    return np.tile(np.array(A, np.uint8), (n, 1))


def lin_odd(n, at):
    v = lin_flat(n)
    v[at] = B
    return v


def lin_alternating(n):
    return np.array([(10, 20, 30), (40, 60, 90)], np.uint8)[np.arange(n) % 2]


def lin_ramp01(n):
    """0, 1, 0, 1, ...: a run of even length averages to exactly one half, which rounds away from zero"""
    return np.repeat((np.arange(n) % 2).astype(np.uint8), 3).reshape(n, 3)


def lin_ends(n):
    return np.array([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255), (255, 255, 255)], np.uint8)[(np.arange(n) // 3) % 5]


def lin_noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def photo(w, h, k):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + 8100 + k)


# ---- the restatement
_WANT = {}


def restated(img, d, key=None):
    """the stream the reference writes for img under d: the oracle (d == 0) or rle_approx_ref on the oracle's linearisation"""
    import oracle_lib as O
    k = (key, repr(float(d))) if key is not None else None
    if k is None or k not in _WANT:
        h, w = img.shape[:2]
        if d == 0.0:
            rc, data, st = O.encode("hilbert(rle)", img)
            assert rc == 0
        else:
            data = R.encode_py(O.hilbert_linearize(img), w, h, d)
        if k is None:
            return data
        _WANT[k] = data
    return _WANT[k]


def records(stream):
    """[(start, count, (r, g, b))] of a stream"""
    assert (len(stream) - 8) % 12 == 0
    out, at = [], 0
    for r in range((len(stream) - 8) // 12):
        rec = stream[8 + 12 * r:20 + 12 * r]
        assert rec[1:9] == (3).to_bytes(8, "little")
        out.append((at, rec[0], tuple(rec[9:12])))
        at += rec[0]
    return out


def counts(stream):
    return [c for _, c, _ in records(stream)]


# ---- the shaped frames: every size of the issue under the content kinds in turn
def shaped():
    """[(name, image)]: 1 x 1, 2 x 1, the rows n x 1 and 1 x n, the rectangles, then the two frames that ride along unrouted"""
    kinds = [lambda n, k: lin_flat(n), lambda n, k: lin_noise(n, 100 + k), lambda n, k: lin_alternating(n), lambda n, k: lin_ramp01(n), lambda n, k: lin_ends(n),
             lambda n, k: lin_odd(n, n - 1)]
    out = [("1x1", np.array([[[255, 0, 1]]], np.uint8)), ("2x1", np.array([[[0, 0, 0], [255, 255, 255]]], np.uint8))]
    k = 0
    for n in ROWS:
        for w, h in ((n, 1), (1, n)):
            out.append(("%dx%d" % (w, h), along_scan(w, h, kinds[k % len(kinds)](n, k))))
            k += 1
    for j, (w, h) in enumerate(RECTS):
        out.append(("%dx%d photo" % (w, h), photo(w, h, j)))
        out.append(("%dx%d" % (w, h), along_scan(w, h, kinds[(k + j) % len(kinds)](w * h, k + j))))
    for j, (w, h) in enumerate(UNROUTED):
        out.append(("%dx%d unrouted" % (w, h), photo(w, h, 20 + j)))
    return out


def routed(imgs, max_px=MAX_PX):
    return [1 <= im.shape[0] * im.shape[1] <= max_px for im in imgs]


# ---- 16 384-pixel frames by content: (name, image); the odd pixel sits at the run offsets and at the piece borders of phase c
ODD_AT = sorted({0, 1, 253, 254, 255, 256, 257} | {k * PIECE + o for k in (1, 2, 3, 4) for o in (-1, 0, 1)})


def bound_frames():
    n = MAX_PX
    out = [("flat", along_scan(n, 1, lin_flat(n)))]
    for j, at in enumerate(ODD_AT):
        w, h = ((n, 1), (1, n), (128, 128))[j % 3]
        out.append(("odd at %d" % at, along_scan(w, h, lin_odd(n, at))))
    out += [("alternating", along_scan(128, 128, lin_alternating(n))), ("noise", along_scan(n, 1, lin_noise(n, 5))), ("photo", photo(128, 128, 40)),
            ("ramp01", along_scan(1, n, lin_ramp01(n))), ("ends", along_scan(n, 1, lin_ends(n)))]
    return out


def bound_claims(frames, d):
    """asserts each 16 384-pixel frame's property under d from the restatement -> [(runs, stream length)]"""
    n = MAX_PX
    none, lossy_all = not d >= 0.0, d >= 441.7
    claims = []
    for name, im in frames:
        s = restated(im, d, "bound " + name)
        recs = records(s)
        cs = [c for _, c, _ in recs]
        assert sum(cs) == n and max(cs) <= MAX_RUN
        if none or name in ("noise", "alternating") and d == 0.0:
            assert cs == [1] * n, name                                    # every run has length 1
        elif name == "flat" or lossy_all:
            assert cs == [MAX_RUN] * 64 + [64], name                        # the cap's phase: a run of exactly 255 ends at position 16319
            assert recs[63][0] + recs[63][1] - 1 == 16319
        elif name.startswith("odd at"):                                     # d is 0 or 4 here; the odd pixel is 224 * sqrt 3 away
            at = int(name.split()[-1])
            assert (at, 1, B) in recs, name                                 # the odd pixel is a run of its own ...
            assert at + 1 in [r[0] for r in recs] and recs[[r[0] for r in recs].index(at + 1)][1] == MAX_RUN     # ... and restarts the cap's phase
            assert [r[0] for r in recs if r[0] < at] == list(range(0, at, MAX_RUN)), name
        elif name == "ramp01" and d == 4.0:
            assert cs == [MAX_RUN] * 64 + [64] and recs[-1][2] == (1, 1, 1), name           # 32 / 64 is one half: 1, away from zero
            assert recs[0][2] == (0, 0, 0) and recs[1][2] == (1, 1, 1)                      # 127 / 255 and 128 / 255
        if name == "ends":
            assert {0, 255} >= {v for _, _, c in recs for v in c} or d != 0.0
        claims.append((len(recs), len(s)))
    return claims


def singles(key, d, imgs, scan=None):
    return D.singles(("rle_small", key, repr(float(d))), expr_of(d), imgs, scan=scan)


def batch(ctx, d, imgs, stride, **kw):
    return D.batch(ctx, expr_of(d), imgs, stride, timer=TIMER, **kw)


def _stride(want):
    return _round4(max(len(s[1]) for s in want)) + 4


def check(res, want, imgs, d, what, key=None):
    """against the single calls, and those against the restatement"""
    check_against_singles(res, want, what)
    for f, im in enumerate(imgs):
        assert want[f][0] == 0 and want[f][1] == restated(im, d, None if key is None else "%s %d" % (key, f)), (what, f)


@pytest.mark.parametrize("d", D_BIG, ids=repr)
def test_every_shape(d):
    import cniic_amd
    names, imgs = zip(*shaped())
    assert [im.shape[0] * im.shape[1] for im in imgs[-2:]] == [16385, 19200] and sum(routed(imgs)) == len(imgs) - 2 == 2 + 2 * len(ROWS) + 2 * len(RECTS)
    assert len({o % 16 for o in _pack(imgs)[1]}) >= 6
    want = singles("shapes", d, imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, d, imgs, _stride(want), poison=POISON)
        assert ctx.kernel_time(PLACE)[1] == 1
    assert res[6] == len(imgs) - 2
    check(res, want, imgs, d, "shapes d = %r" % d, "shapes")
    stride = _stride(want)
    for f in range(len(imgs)):
        assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), names[f]


def full_d_frames():
    return [photo(64, 64, 50), along_scan(64, 64, lin_noise(4096, 51)), photo(100, 75, 52), along_scan(100, 75, lin_ramp01(7500)), along_scan(511, 1, lin_noise(511, 53)),
            along_scan(511, 1, lin_odd(511, 255)), photo(511, 1, 54)]


@pytest.mark.parametrize("d", D_ALL, ids=repr)
def test_every_d(d):
    import cniic_amd
    imgs = full_d_frames()
    assert [im.shape[:2] for im in imgs] == [(64, 64)] * 2 + [(75, 100)] * 2 + [(1, 511)] * 3
    ramp, odd = restated(imgs[3], d, "every_d 3"), restated(imgs[5], d, "every_d 5")
    if d >= math.sqrt(3.0):       # the first step of the ramp is sqrt 3 away, every later one nearer
        assert counts(ramp) == [MAX_RUN] * 29 + [105]
    else:
        assert counts(ramp) == [1] * 7500
    if d >= 0.0 and d < 100.0:    # 255 flat pixels are a full run, the odd one after them begins the next
        assert counts(odd)[:2] == [MAX_RUN, 1] and records(odd)[1][2] == B
    want = singles("every_d", d, imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, d, imgs, _stride(want))
    assert res[6] == len(imgs)
    check(res, want, imgs, d, "d = %r" % d, "every_d")


@pytest.mark.parametrize("d", D_BIG, ids=repr)
def test_contents_at_the_bound(d):
    import cniic_amd
    frames = bound_frames()
    claims = bound_claims(frames, d)
    imgs = [im for _, im in frames]
    assert all(im.shape[0] * im.shape[1] == MAX_PX for im in imgs)
    want = singles("bound", d, imgs)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, d, imgs, STRIDE_AT_BOUND)
    assert res[6] == len(imgs)
    check(res, want, imgs, d, "bound d = %r" % d)
    assert [(len(records(s)), len(s)) for s in res[4]] == claims


def machinery_frames():
    """a few frames of every kind and many stream lengths, all on the route but the last two"""
    return [photo(64, 64, 60), along_scan(37, 41, lin_noise(37 * 41, 61)), along_scan(1024, 1, lin_flat(1024)), along_scan(1, 1025, lin_odd(1025, 256)), photo(100, 75, 62),
            np.array([[[9, 8, 7]]], np.uint8), along_scan(128, 128, lin_alternating(MAX_PX)), photo(7, 9, 63), photo(128, 96, 64), photo(16385, 1, 65), photo(160, 120, 66)]


def test_route_off_and_a_lowered_bound(monkeypatch):
    import cniic_amd
    imgs = machinery_frames()
    for d in (0.0, 4.0):
        want = singles("machinery", d, imgs)
        stride = _stride(want)
        with cniic_amd.Context(0) as ctx:
            on = batch(ctx, d, imgs, stride)
            monkeypatch.setenv(KNOB_OFF, "1")
            off = batch(ctx, d, imgs, stride)
            assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0     # not merely zero launches: no such stage
            monkeypatch.delenv(KNOB_OFF)
            monkeypatch.setenv(KNOB_MAX_PX, "1024")
            low = batch(ctx, d, imgs, stride)
            monkeypatch.delenv(KNOB_MAX_PX)
        px = [im.shape[0] * im.shape[1] for im in imgs]
        assert 1024 in px and 1025 in px                                                     # frames on both sides of the lowered bound
        assert on[6] == len(imgs) - 2 and off[6] == 0 and low[6] == sum(routed(imgs, 1024)) == 3
        for res, what in ((off, "route off"), (low, "bound 1024")):
            assert (on[0], on[1], on[2], on[4]) == (res[0], res[1], res[2], res[4]), what
        check(on, want, imgs, d, "route on", "machinery")


def test_host_images_are_not_routed_and_host_output_gets_the_same_bytes():
    import cniic_amd
    imgs = machinery_frames()
    d = 4.0
    want = singles("machinery", d, imgs)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, d, imgs[:8], stride, host_src=True, host_out=True)
        assert res[6] == 0
        check_against_singles(res, want[:8], "host source")
        res = batch(ctx, d, imgs, stride, host_out=True, poison=POISON)
        assert res[6] == len(imgs) - 2
        check_against_singles(res, want, "host out")
        for f in range(len(imgs)):
            assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), f


def placement_kinds():
    """seven frames of 1 .. 7 runs: streams of 20 .. 92 bytes"""
    return [along_scan(k + 3, 1, np.array([(30 * min(j, k),) * 3 for j in range(k + 3)], np.uint8)) for k in range(7)]      # k + 1 colours, the last three times


@pytest.mark.parametrize("out_off,host_out", ((1, False), (14, False), (7, True)))
def test_streams_placed_at_every_alignment(out_off, host_out):
    """odd stride, the output pointer off its 16-byte boundary: every destination residue, poison before, between and behind the streams"""
    import cniic_amd
    kinds = placement_kinds()
    want1 = singles("placement", 0.0, kinds)
    assert sorted(len(s[1]) for s in want1) == [8 + 12 * r for r in range(1, 8)]
    F = 16 * len(kinds)
    imgs, want = [kinds[f % 7] for f in range(F)], [want1[f % 7] for f in range(F)]
    stride = (max(len(s[1]) for s in want1) + 8) | 1
    assert {(out_off + f * stride) % 16 for f in range(F)} == set(range(16))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, 0.0, imgs, stride, host_out=host_out, poison=POISON, out_off=out_off)
    assert res[6] == F and res[0] == 0
    check_against_singles(res, want, "placement %d" % out_off)
    (whole, at), lens = res[5], res[1]
    assert bool((whole[:at] == POISON).all()) and bool((whole[at + F * stride:] == POISON).all())
    for f in range(F):
        assert bool((whole[at + f * stride + lens[f]:at + (f + 1) * stride] == POISON).all()), f


@pytest.mark.parametrize("host_out", (False, True))
def test_capacity_is_one_frame_s(host_out):
    """the stride one byte short for exactly one frame: CAPACITY with its true length, nothing written, the neighbours intact"""
    import cniic_amd
    imgs = machinery_frames()[:9]
    d = 4.0
    want = singles("machinery", d, machinery_frames())[:9]
    by_len = sorted(range(len(imgs)), key=lambda f: -len(want[f][1]))
    big, second = by_len[0], by_len[1]
    stride = len(want[big][1]) - 1
    assert len(want[second][1]) <= stride
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, d, imgs, stride, host_out=host_out, poison=POISON)
    assert launches == len(imgs) and rc == CAPACITY
    assert msg == "encode: stream is %d bytes, capacity %d" % (len(want[big][1]), stride)
    for f in range(len(imgs)):
        assert lens[f] == len(want[f][1]), f
        if f == big:
            assert rcs[f] == CAPACITY and bool((host[f * stride:(f + 1) * stride] == POISON).all())
        else:
            assert rcs[f] == 0 and streams[f] == want[f][1], f
            assert bool((host[f * stride + lens[f]:(f + 1) * stride] == POISON).all()), f


def many():
    rng = np.random.default_rng(48)
    sizes = [(8, 8), (9, 7), (16, 12), (1, 1), (13, 5), (3, 2), (12, 12), (2, 37)]
    imgs = []
    for f in range(3000):
        w, h = sizes[f % 8]
        imgs.append((rng.integers(0, 2, (h, w, 3)) * 6 + 100).astype(np.uint8))      # eight colours, 6 apart per channel: runs at d = 0 and longer ones at d = 8
    return imgs


def test_many_frames_in_one_launch():
    import cniic_amd
    imgs = many()
    assert len(imgs) == 3000 and len({im.shape[:2] for im in imgs}) == 8
    stride = 8 + 12 * 16 * 12 + 4
    for d in (0.0, 8.0):
        lens_want = [len(restated(im, d)) for im in imgs[::60]]
        assert len(set(lens_want)) > 8
        with cniic_amd.Context(0) as ctx:
            rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, d, imgs, stride)
            assert launches == 3000 and rc == 0 and rcs == [0] * 3000
            with cniic_amd.Context(0) as ref:
                for f in range(0, 3000, 75):
                    src, sdata, sst = ref.encode(expr_of(d), imgs[f])
                    assert src == 0 and streams[f] == sdata, f
        for k, f in enumerate(range(0, 3000, 60)):
            assert len(streams[f]) == lens_want[k] and streams[f] == restated(imgs[f], d), f


def test_chunks(monkeypatch):
    """rle_small_encode sizes a chunk by the slot and the rows of its first (largest) frame under CNIIC_TEST_MEASURE_BUDGET"""
    import cniic_amd
    imgs = machinery_frames()
    d = 4.0
    want = singles("machinery", d, imgs)
    stride = _stride(want)
    frame = STRIDE_AT_BOUND + 16 + 8        # rle_small_frame_bytes(16384)
    n_routed = sum(routed(imgs))
    px = sorted((im.shape[0] * im.shape[1] for im in imgs if im.shape[0] * im.shape[1] <= MAX_PX), reverse=True)
    assert px[:3] == [16384, 12288, 7500]
    # the first chunk holds 16384 and 12288 (two slots of the bound), the second the next four under 7500's slot, the third the rest
    budget = 2 * frame
    slot = lambda n: ((8 + 12 * n + 15) & ~15) + 16 + 8
    assert budget // slot(7500) == 4 and budget // slot(px[6]) >= len(px) - 6
    with cniic_amd.Context(0) as ctx:
        one = batch(ctx, d, imgs, stride)
        assert ctx.kernel_time(PLACE)[1] == 1
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        three = batch(ctx, d, imgs, stride)
        chunks = ctx.kernel_time(PLACE)[1]
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")                 # a frame a chunk
        each = batch(ctx, d, imgs, stride)
        assert ctx.kernel_time(PLACE)[1] == n_routed
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert chunks == 3
    for res in (three, each):
        assert res[6] == n_routed and res[:5] == one[:5]
    check_against_singles(three, want, "three chunks")


def test_the_floor(monkeypatch):
    """in a call with fewer than FLOOR_NONE candidate frames none takes the route, with fewer than FLOOR_FRAMES only those of at most
    FLOOR_PX pixels do: the call and one CU are slower for few or few heavy frames than the workers' whole chip (NOTES AN)"""
    import cniic_amd
    monkeypatch.delenv(KNOB_FLOOR_OFF)
    big, edge, above = photo(128, 128, 70), photo(64, 64, 71), photo(17, 241, 72)
    tiny = [photo(5, 3, 73 + i) for i in range(FLOOR_FRAMES - 3)]
    assert edge.shape[0] * edge.shape[1] == FLOOR_PX and above.shape[0] * above.shape[1] == FLOOR_PX + 1
    imgs = [big, edge, above] + tiny
    T = list(range(3, len(imgs)))
    assert (FLOOR_NONE, len(T)) == (4, FLOOR_FRAMES - 3)
    # (frames of the call, candidates, frames expected on the route)
    calls = (([0], 1, 0), ([1], 1, 0), ([1] + T[:2], FLOOR_NONE - 1, 0), ([1, 2] + T[:2], FLOOR_NONE, 3), ([0, 1, 2] + T[:-1], FLOOR_FRAMES - 1, FLOOR_FRAMES - 3),
             ([0, 1, 2] + T, FLOOR_FRAMES, FLOOR_FRAMES))
    for d in (0.0, 4.0):
        want = singles("floor", d, imgs)
        stride = _stride(want)
        with cniic_amd.Context(0) as ctx:
            for which, candidates, routed_frames in calls:
                assert len(which) == candidates
                res = batch(ctx, d, [imgs[k] for k in which], stride)
                assert res[6] == routed_frames, (d, which, res[6])
                check_against_singles(res, [want[k] for k in which], "floor %r" % (which,))
            monkeypatch.setenv(KNOB_FLOOR_OFF, "1")
            res = batch(ctx, d, imgs[:1], stride)
            monkeypatch.delenv(KNOB_FLOOR_OFF)
            assert res[6] == 1


def test_a_size_with_an_injected_scan_stays_with_the_workers_and_follows_it():
    import cniic_amd
    imgs = machinery_frames()[:9]
    w, h = 100, 75
    assert imgs[4].shape[:2] == (h, w)
    p = np.random.default_rng(7).permutation(w * h)
    scan = (w, h, np.stack([p % w, p // w], 1).astype(np.uint32))
    for d in (0.0, 4.0):
        want = singles("scan", d, imgs, scan=scan)
        builtin = singles("machinery", d, machinery_frames())[:9]
        assert want[4][1] != builtin[4][1] and all(want[f][1] == builtin[f][1] for f in range(9) if f != 4)
        assert want[4][1] == R.encode_py(imgs[4][scan[2][:, 1], scan[2][:, 0]], w, h, d)          # the single call follows the injected order
        with cniic_amd.Context(0) as ctx:
            ctx.set_scan(*scan)
            res = batch(ctx, d, imgs, _stride(want))
            assert res[6] == 8
            check_against_singles(res, want, "injected scan")
            ctx.set_scan(w, h, None)
            res = batch(ctx, d, imgs, _stride(want))
            assert res[6] == 9
            check_against_singles(res, builtin, "scan taken back")


def test_two_alternating_calls_with_different_d_on_one_context():
    import cniic_amd
    imgs = machinery_frames()[:9]
    ds = (4.0, 0.0, 16.0, math.nan)
    wants = [singles("machinery", d, machinery_frames())[:9] for d in ds]
    assert len({tuple(len(s[1]) for s in w) for w in wants}) == len(ds)
    stride = max(_stride(w) for w in wants)
    with cniic_amd.Context(0) as ctx:
        for turn in range(2):
            for d, want in zip(ds, wants):
                res = batch(ctx, d, imgs, stride)
                assert res[6] == 9
                check_against_singles(res, want, "turn %d, d = %r" % (turn, d))


@pytest.mark.parametrize("d", (0.0, 4.0), ids=repr)
def test_measure_batch_is_the_loop_of_the_three_single_calls(d):
    import torch
    import cniic_amd
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    imgs = machinery_frames() + [photo(333, 200, 80)]
    expr = expr_of(d)
    want = singles("measure", d, imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        rows_want, backs = [], []
        for im, (rc, data, st, _) in zip(imgs, want):
            rc2, back = ctx.decode(expr, data)
            assert rc2 == 0 and (d != 0.0 or np.array_equal(back, im))
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
            backs.append(back)
        assert d == 0.0 or any(r["error"] > 0.0 for r in rows_want)
        buf, offs, ws, hs = _pack(imgs)
        F = len(imgs)
        stride = _stride(want) + 4
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch(expr, src, offs, ws, hs, out, stride, allow=FAILURES)
        launches, places = ctx.kernel_time(TIMER)[1], ctx.kernel_time(PLACE)[1]     # the encode's stages, readable after the decode
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == F - 3 and places == 1 and rc == 0
        host = out.cpu().numpy()
        for f in range(F):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f], (f, got, rows_want[f])
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f
