"""Small `zip(dict)` frames of a batch call on the small-frame route (k_zd_small.hip: a workgroup per frame, the trie in a table of edges
in device memory, windows of speculated walks repaired from the window's own entries; include/cniic_hip.h above
cniic_codec_encode_batch_var).  Every comparison is exact: a frame's status, length, bytes and message are those of
cniic_codec_encode_opts for that frame alone on a context that has seen no batch, and the bytes are those of tests/zip_dict_ref.py through
its C restatement.  Which frames took the route is read from the stage timer "zd_small_batch", whose launch count is the number of frames
given to the kernel; "zd_small_handback" counts those of them the kernel gave up and the workers coded, "zd_small_finished" the walks the
commit wave finished behind the speculation's cap.  On a build without the route none of these marks exists.

What a case claims about a frame -- how its stream ends, its longest match and so which side of a cap it lies on, where its matches
stand against the windows' ends -- is computed from the reference stream alone (longest_match, windows); tests/test_zd_small_cpu.py
asserts the same claims without a GPU."""
import struct
import tempfile

import numpy as np
import pytest

import test_delta_small_batch as D
import zip_dict_ref as Z
from test_delta_small_batch import _pack, _round4, check_against_singles

pytestmark = pytest.mark.gpu

MAX_PX = 16384              # kZdSmallMaxPx (cniic_amd/csrc/zd_small.hpp)
WINDOW = 256                # kZsWindow
SPEC_CAP, GIVE_UP = 32, 1024   # kZsSpecCap, kZsGiveUp
STRIDE_AT_BOUND = 360480    # zs_stride(8 + 11 * 16384)
TABLE_BITS_AT_BOUND = 19    # zs_table_bits(8 + 11 * 16384)
FLOOR_FRAMES, FLOOR_PX = 256, 4096   # kZdSmallFloorFrames, kZdSmallFloorPx (capi.cpp): the frames of at most FLOOR_PX pixels take the route in a call with FLOOR_FRAMES of them
TIMER, PLACE, HANDBACK, FINISHED = "zd_small_batch", "zd_small_place", "zd_small_handback", "zd_small_finished"
KNOB_OFF, KNOB_MAX_PX, KNOB_FLOOR_OFF, KNOB_CAP = "CNIIC_TEST_ZD_SMALL_OFF", "CNIIC_TEST_ZD_SMALL_MAX_PX", "CNIIC_TEST_ZD_SMALL_FLOOR_OFF", "CNIIC_TEST_ZD_SMALL_CAP"
EXPR = "zip(dict)"
FAILURES, CAPACITY = D.FAILURES, D.CAPACITY
POISON = 0xA5
SIZES = [(1, 1), (2, 1), (3, 1), (5, 1), (7, 3), (8, 8), (13, 5), (32, 32), (64, 64), (128, 96), (128, 128), (16384, 1), (1, 16384)]   # (w, h)
UNROUTED = [(16385, 1), (160, 120)]
EDGE_FRAMES = (134, 138)    # of many()
FLAT_LONGEST = {(8, 8): 264, (32, 32): 4224, (64, 64): 16896, (128, 96): 45056, (128, 128): 67584}   # the longest entry of a flat frame


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor; test_the_floor holds it"""
    monkeypatch.setenv(KNOB_FLOOR_OFF, "1")


# ---- contents
def two_colour(w, h):
    """columns alternate (255, 0, 7) and black"""
    img = np.zeros((h, w, 3), np.uint8)
    img[:, ::2] = (255, 0, 7)
    return img


def banded(w, h, at, px):
    """photo-like with `px` pixels in one colour from pixel `at` on: the long entries appear mid-frame"""
    img = Z.photo_like(w, h).reshape(-1, 3).copy()
    img[at:at + px] = (93, 41, 200)
    return img.reshape(h, w, 3)


CONTENTS = (("photo", Z.photo_like), ("noise", Z.noise), ("flat", Z.flat), ("two-colour", two_colour))


def shaped():
    """[(name, image)]: every size under every content, two frames of many(), then the two frames that ride along unrouted"""
    out = [("%s %dx%d" % (nm, w, h), gen(w, h)) for w, h in SIZES for nm, gen in CONTENTS]
    out += [("few colours %d" % k, many()[k]) for k in EDGE_FRAMES]      # (second matches that end one past a window's end are rare)
    return out + [("photo %dx%d unrouted" % (w, h), Z.photo_like(w, h)) for w, h in UNROUTED]


def routed(imgs, max_px=MAX_PX):
    return [1 <= im.shape[0] * im.shape[1] <= max_px for im in imgs]


# ---- the restatement, and what a stream says about the walks that made it
_CLIB, _WANT = [], {}


def restated(img, key=None):
    """the stream of tests/zip_dict_ref.py (the C restatement) for img; cached under key"""
    if key is None or key not in _WANT:
        if not _CLIB:
            _CLIB.append(Z.compile_c(tempfile.mkdtemp(prefix="zd_small_ref")))
        assert _CLIB[0] is not None, "no C compiler"
        data = Z.codec_encode(lambda t: Z.encode_c(_CLIB[0], t), img)
        if key is None:
            return data
        _WANT[key] = data
    return _WANT[key]


def matches(stream):
    """[(start, length, is the pair's second)] of every match of a stream, from the symbols alone"""
    syms = struct.unpack("<%dH" % (len(stream) // 2), stream)
    length = {b: 1 for b in range(256)}
    counter, pos, out = Z.FIRST_NEW, 0, []
    for k in range(0, len(syms), 2):
        s1, s2 = syms[k], syms[k + 1]
        out.append((pos, length[s1], False))
        if s2 != Z.EOF:
            out.append((pos + length[s1], length[s2], True))
            if counter != Z.EOF:
                length[counter] = length[s1] + length[s2]
                counter += 1
            pos += length[s1] + length[s2]
        else:
            pos += length[s1]
    return out


def longest_match(stream):
    return max(ln for _, ln, _ in matches(stream))


def ends_in_eof(stream):
    return stream[-2:] == b"\xff\xff"


def handed_back(stream, cap=GIVE_UP):
    """the kernel gives a frame up when one of its matches is longer than the cap"""
    return longest_match(stream) > cap


def windows(stream, W=WINDOW):
    """how the kernel's windows fall on a stream's matches: a window starts at the first match that begins at or behind the end of the
    one before.  -> (first matches' ends, second matches' ends), each as the set of offsets end - (window start + W) in -1 .. 1"""
    base, first, second = 0, set(), set()
    for start, ln, is_second in matches(stream):
        if start >= base + W:
            base = start
        off = start + ln - (base + W)
        if -1 <= off <= 1:
            (second if is_second else first).add(off)
    return first, second


def singles(key, imgs):
    return D.singles(("zd_small", key), EXPR, imgs)


def batch(ctx, imgs, stride, **kw):
    """D.batch, and behind the routed frames' count the frames handed back and the walks the commit finished"""
    res = D.batch(ctx, EXPR, imgs, stride, timer=TIMER, **kw)
    return res + (ctx.kernel_time(HANDBACK)[1], ctx.kernel_time(FINISHED)[1])


def _stride(want):
    return _round4(max(len(s[1]) for s in want)) + 4


def check(res, want, imgs, what, key=None):
    """against the single calls, and those against the restatement"""
    check_against_singles(res, want, what)
    for f, im in enumerate(imgs):
        assert want[f][0] == 0 and want[f][1] == restated(im, None if key is None else "%s %d" % (key, f)), (what, f)


def test_every_shape_and_content():
    import cniic_amd
    names, imgs = zip(*shaped())
    assert [im.shape[0] * im.shape[1] for im in imgs[-2:]] == [16385, 19200] and sum(routed(imgs)) == len(imgs) - 2 == 4 * len(SIZES) + len(EDGE_FRAMES)
    want = singles("shapes", imgs)
    by = dict(zip(names, (s[1] for s in want)))
    # both endings
    for nm in ("photo 5x1", "photo 13x5", "photo 32x32", "noise 2x1", "noise 8x8", "flat 7x3", "flat 8x8", "flat 32x32"):
        assert ends_in_eof(by[nm]), nm
    for nm in ("photo 1x1", "photo 8x8", "photo 64x64"):
        assert not ends_in_eof(by[nm]), nm
    assert len(by["photo 1x1"]) == 4 * 7
    # every match of a flat or two-colour frame reuses what the pair before it made; the large ones pass the cap and are handed back
    back = [handed_back(s) for s in by.values()][:-2]
    assert not handed_back(by["flat 8x8"]) and longest_match(by["flat 8x8"]) > SPEC_CAP and handed_back(by["flat 32x32"]) and handed_back(by["two-colour 128x128"])
    assert not any(handed_back(by[nm]) for nm in by if nm.startswith(("photo", "noise")))
    # pairs and entries end on, one before and one past a window's end
    first, second = set(), set()
    for nm in by:
        if not handed_back(by[nm]):
            a, b = windows(by[nm])
            first |= a
            second |= b
    assert first == second == {-1, 0, 1}
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride, poison=POISON)
        assert ctx.kernel_time(PLACE)[1] == 1
    assert res[6] == len(imgs) - 2 and res[8] == sum(back) and 0 < sum(back) < len(back) and res[9] > 0
    check(res, want, imgs, "shapes", "shapes")
    for f in range(len(imgs)):
        assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), names[f]


def cap_frames():
    """(name, image): flat, two-colour and banded frames, and three good ones"""
    return [("flat 8x8", Z.flat(8, 8)), ("flat 32x32", Z.flat(32, 32)), ("two-colour 13x5", two_colour(13, 5)), ("two-colour 32x32", two_colour(32, 32)),
            ("band 40", banded(64, 64, 2000, 40)), ("band 300", banded(64, 64, 2000, 300)), ("flat 2x1", Z.flat(2, 1)),
            ("photo 32x32", Z.photo_like(32, 32)), ("noise 13x5", Z.noise(13, 5)), ("photo 64x64", Z.photo_like(64, 64))]


CAPS = (8, 20, 100, 300, GIVE_UP)


@pytest.mark.parametrize("cap", CAPS)
def test_frames_on_both_sides_of_the_caps(cap, monkeypatch):
    """the knob lowers the give-up cap, and the speculation's cap with it where it is lower: every frame alone and all together"""
    import cniic_amd
    names, imgs = zip(*cap_frames())
    want = singles("caps", imgs)
    back = [handed_back(s[1], cap) for s in want]
    longest = dict(zip(names, (longest_match(s[1]) for s in want)))
    assert longest["band 40"] < longest["band 300"] and longest["photo 64x64"] <= SPEC_CAP and longest["flat 2x1"] <= 8
    assert 0 < sum(back) < len(back) or cap == 8
    stride = _stride(want)
    monkeypatch.setenv(KNOB_CAP, str(cap))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride)
        assert res[6] == len(imgs) and res[8] == sum(back), (cap, res[8], back)
        if cap > SPEC_CAP:       # a frame that stays has a match between the two caps: the commit wave finished that walk
            assert any(SPEC_CAP < ln <= cap for ln in longest.values()) and res[9] > 0
        check(res, want, imgs, "cap %d" % cap, "caps")
        for f in range(len(imgs)):
            one = batch(ctx, imgs[f:f + 1], stride)
            assert one[6] == 1 and one[8] == int(back[f]), (cap, names[f])
            check_against_singles(one, want[f:f + 1], "cap %d, %s alone" % (cap, names[f]))


def machinery_frames():
    """frames of many stream lengths, all on the route but the last two; the second is handed back"""
    return [Z.photo_like(64, 64), Z.flat(40, 40), Z.noise(37, 41), Z.photo_like(100, 75), np.array([[[9, 8, 7]]], np.uint8), two_colour(8, 8), Z.photo_like(7, 9),
            Z.noise(32, 32), Z.photo_like(128, 96), Z.photo_like(16385, 1), Z.photo_like(160, 120)]


def test_route_off_and_a_lowered_bound(monkeypatch):
    import cniic_amd
    imgs = machinery_frames()
    want = singles("machinery", imgs)
    assert [handed_back(s[1]) for s in want[:9]] == [False, True] + [False] * 7
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, imgs, stride)
        monkeypatch.setenv(KNOB_OFF, "1")
        off = batch(ctx, imgs, stride)
        for name in (TIMER, PLACE, HANDBACK, FINISHED):
            assert ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, None) != 0     # not merely zero launches: no such stage
        monkeypatch.delenv(KNOB_OFF)
        monkeypatch.setenv(KNOB_MAX_PX, "1024")
        low = batch(ctx, imgs, stride)
        monkeypatch.delenv(KNOB_MAX_PX)
    px = [im.shape[0] * im.shape[1] for im in imgs]
    assert 1024 in px and 1517 in px
    assert on[6] == len(imgs) - 2 and on[8] == 1 and off[6] == 0 and low[6] == sum(routed(imgs, 1024)) == 4 and low[8] == 0
    for res, what in ((off, "route off"), (low, "bound 1024")):
        assert (on[0], on[1], on[2], on[4]) == (res[0], res[1], res[2], res[4]), what
    check(on, want, imgs, "route on", "machinery")


def test_host_images_are_not_routed_and_host_output_gets_the_same_bytes():
    import cniic_amd
    imgs = machinery_frames()
    want = singles("machinery", imgs)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs[:8], stride, host_src=True, host_out=True)
        assert res[6] == 0
        check_against_singles(res, want[:8], "host source")
        res = batch(ctx, imgs, stride, host_out=True, poison=POISON)
        assert res[6] == len(imgs) - 2 and res[8] == 1
        check_against_singles(res, want, "host out")
        for f in range(len(imgs)):
            assert bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), f


def placement_kinds():
    """seven tiny frames whose streams differ in length"""
    return [Z.photo_like(1, 1), Z.photo_like(2, 1), Z.noise(3, 1), Z.flat(5, 1), two_colour(7, 3), Z.noise(4, 2), Z.photo_like(6, 1)]


@pytest.mark.parametrize("out_off,host_out", ((1, False), (14, False), (7, True)))
def test_streams_placed_at_every_alignment(out_off, host_out):
    """odd stride, the output pointer off its 16-byte boundary: every destination residue, poison before, between and behind the streams"""
    import cniic_amd
    kinds = placement_kinds()
    want1 = singles("placement", kinds)
    assert len({len(s[1]) for s in want1}) >= 5
    F = 16 * len(kinds)
    imgs, want = [kinds[f % 7] for f in range(F)], [want1[f % 7] for f in range(F)]
    stride = (max(len(s[1]) for s in want1) + 8) | 1
    assert {(out_off + f * stride) % 16 for f in range(F)} == set(range(16))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride, host_out=host_out, poison=POISON, out_off=out_off)
    assert res[6] == F and res[0] == 0 and res[8] == 0
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
    want = singles("machinery", machinery_frames())[:9]
    by_len = sorted(range(len(imgs)), key=lambda f: -len(want[f][1]))
    big, second = by_len[0], by_len[1]
    stride = len(want[big][1]) - 1
    assert len(want[second][1]) <= stride and not handed_back(want[big][1])
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg, back, fin = batch(ctx, imgs, stride, host_out=host_out, poison=POISON)
    assert launches == len(imgs) and rc == CAPACITY and back == 1
    assert msg == "encode: stream is %d bytes, capacity %d" % (len(want[big][1]), stride)
    for f in range(len(imgs)):
        assert lens[f] == len(want[f][1]), f
        if f == big:
            assert rcs[f] == CAPACITY and bool((host[f * stride:(f + 1) * stride] == POISON).all())
        else:
            assert rcs[f] == 0 and streams[f] == want[f][1], f
            assert bool((host[f * stride + lens[f]:(f + 1) * stride] == POISON).all()), f


_MANY = []


def many():
    if not _MANY:
        _MANY.extend(_many())
    return list(_MANY)


def _many():
    rng = np.random.default_rng(48)
    sizes = [(8, 8), (9, 7), (16, 12), (1, 1), (13, 5), (3, 2), (32, 32), (2, 37)]
    imgs = []
    for f in range(3000):
        w, h = sizes[f % 8]
        imgs.append((rng.integers(0, 4, (h, w, 3)) * 60 + 10).astype(np.uint8))      # 64 colours: entries that repeat, none long
    return imgs


def test_many_frames_in_one_launch():
    import cniic_amd
    imgs = many()
    assert len(imgs) == 3000 and len({im.shape[:2] for im in imgs}) == 8 and max(im.shape[0] * im.shape[1] for im in imgs) == 1024
    sample = range(0, 3000, 59)
    wants = {f: restated(imgs[f]) for f in sample}
    assert len({len(s) for s in wants.values()}) > 8 and not any(handed_back(s) for s in wants.values())
    stride = 2 * (8 + 11 * 1024) + 4
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg, back, fin = batch(ctx, imgs, stride)
        assert launches == 3000 and rc == 0 and rcs == [0] * 3000 and back == 0 and ctx.kernel_time(PLACE)[1] == 1
        with cniic_amd.Context(0) as ref:
            for f in range(0, 3000, 75):
                src, sdata, sst = ref.encode(EXPR, imgs[f])
                assert src == 0 and streams[f] == sdata, f
    for f in sample:
        assert streams[f] == wants[f], f


def frame_bytes(npx):
    """zd_small_frame_bytes (codec.cpp): the slot, the table, the row and the result row"""
    N = 8 + 11 * npx
    bits = 10
    while (1 << bits) < 2 * (N + 256):
        bits += 1
    return ((2 * N + 2 + 15) & ~15) + (8 << bits) + 16 + 16


def tiny(count):
    return [Z.photo_like(5, 3 + k % 6) for k in range(count)]


def test_chunks(monkeypatch):
    """zd_small_encode sizes a chunk by the slot and the table of its first (largest) frame under CNIIC_TEST_MEASURE_BUDGET"""
    import cniic_amd
    imgs = machinery_frames()
    want = singles("machinery", imgs)
    stride = _stride(want)
    n_routed = sum(routed(imgs))
    px = sorted((im.shape[0] * im.shape[1] for im in imgs if im.shape[0] * im.shape[1] <= MAX_PX), reverse=True)
    assert px[:4] == [12288, 7500, 4096, 1600] and frame_bytes(MAX_PX) == STRIDE_AT_BOUND + (8 << TABLE_BITS_AT_BOUND) + 32
    # the first chunk holds 12288 alone, the second 7500 and 4096 under 7500's table, the third the rest under 1600's
    budget = frame_bytes(12288) + frame_bytes(7500)
    assert budget // frame_bytes(12288) == 1 and budget // frame_bytes(7500) == 2 and budget // frame_bytes(1600) >= len(px) - 3
    with cniic_amd.Context(0) as ctx:
        one = batch(ctx, imgs, stride)
        assert ctx.kernel_time(PLACE)[1] == 1
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        three = batch(ctx, imgs, stride)
        chunks = ctx.kernel_time(PLACE)[1]
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")                 # a frame a chunk
        each = batch(ctx, imgs, stride)
        assert ctx.kernel_time(PLACE)[1] == n_routed - 1                     # (the frame handed back places nothing)
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert chunks == 3
    for res in (three, each):
        assert res[6] == n_routed and res[8] == 1 and res[:5] == one[:5]
    check_against_singles(three, want, "three chunks")


def test_chunks_under_the_floor_one_of_which_ends_below_it(monkeypatch):
    """the floor counts the call's frames, not a chunk's: the last chunk holds fewer frames than the floor asks of a call"""
    import cniic_amd
    monkeypatch.delenv(KNOB_FLOOR_OFF)
    imgs = [Z.photo_like(64, 64), Z.noise(64, 64)] + tiny(FLOOR_FRAMES + 40)
    want = singles("chunks floor", imgs)
    stride = _stride(want)
    budget = 2 * frame_bytes(FLOOR_PX)
    per = budget // frame_bytes(5 * 8)
    rest = len(imgs) - 2
    assert 0 < rest % per < FLOOR_FRAMES and rest // per >= 2
    monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride)
        assert ctx.kernel_time(PLACE)[1] == 1 + (rest + per - 1) // per
    assert res[6] == len(imgs) and res[8] == 0
    check_against_singles(res, want, "chunks under the floor")


def test_the_floor(monkeypatch):
    """the frames of at most FLOOR_PX pixels take the route when the call has FLOOR_FRAMES of them or more: one workgroup is slower for
    larger and for fewer frames than the workers' cores (NOTES AO)"""
    import cniic_amd
    monkeypatch.delenv(KNOB_FLOOR_OFF)
    edge, above, big = Z.photo_like(64, 64), Z.photo_like(17, 241), Z.photo_like(128, 128)
    assert edge.shape[0] * edge.shape[1] == FLOOR_PX and above.shape[0] * above.shape[1] == FLOOR_PX + 1
    imgs = [above, big, edge] + tiny(FLOOR_FRAMES - 1)
    want = singles("floor", imgs)
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        for which, routed_frames in ((list(range(len(imgs) - 1)), 0), (list(range(len(imgs))), FLOOR_FRAMES), ([2], 0)):
            res = batch(ctx, [imgs[k] for k in which], stride)
            assert res[6] == routed_frames, (len(which), res[6])       # (frames 0 and 1 are no candidates)
            check_against_singles(res, [want[k] for k in which], "floor %d" % len(which))
        monkeypatch.setenv(KNOB_FLOOR_OFF, "1")
        res = batch(ctx, imgs[:3], stride)
        assert res[6] == 3


def test_alternating_calls_on_one_context(monkeypatch):
    import cniic_amd
    imgs = machinery_frames()[:9]
    want = singles("machinery", machinery_frames())[:9]
    other = [Z.noise(16, 16), Z.flat(8, 8), Z.photo_like(128, 128)]
    want_other = singles("alternating", other)
    stride = max(_stride(want), _stride(want_other))
    with cniic_amd.Context(0) as ctx:
        for turn in range(2):
            res = batch(ctx, imgs, stride)
            assert res[6] == 9 and res[8] == 1
            check_against_singles(res, want, "turn %d" % turn)
            res = batch(ctx, other, stride)
            assert res[6] == 3 and res[8] == 0
            check_against_singles(res, want_other, "turn %d, other" % turn)
            rc, data, st = ctx.encode(EXPR, imgs[0])
            assert rc == 0 and data == want[0][1]


def test_other_codecs_never_report_the_marks():
    import cniic_amd
    imgs = machinery_frames()[:8]
    with cniic_amd.Context(0) as ctx:
        res = D.batch(ctx, "hufman", imgs, 400000, timer="huf_small_batch")
        assert res[0] == 0
        for name in (TIMER, PLACE, HANDBACK, FINISHED):
            assert ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, None) != 0


def test_measure_batch_is_the_loop_of_the_three_single_calls():
    import torch
    import cniic_amd
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    imgs = machinery_frames() + [Z.photo_like(333, 200)]
    want = singles("measure", imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        rows_want = []
        for im, (rc, data, st, _) in zip(imgs, want):
            rc2, back = ctx.decode(EXPR, data)
            assert rc2 == 0 and np.array_equal(back, im)
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
        buf, offs, ws, hs = _pack(imgs)
        F = len(imgs)
        stride = _stride(want) + 4
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch(EXPR, src, offs, ws, hs, out, stride, allow=FAILURES)
        launches, places, back = ctx.kernel_time(TIMER)[1], ctx.kernel_time(PLACE)[1], ctx.kernel_time(HANDBACK)[1]     # the encode's stages, readable after the decode
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == F - 3 and places == 1 and back == 1 and rc == 0
        host = out.cpu().numpy()
        for f in range(F):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f], (f, got, rows_want[f])
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f
