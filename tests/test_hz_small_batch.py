"""Hilbert { compress: Zip } frames of a batch call (cniic_hilbert_zip_encode_batch_var, cniic_hilbert_zip_measure_batch; include/cniic_hip.h)
and the small-frame route under them (k_hz_small in k_zd_small.hip: `zip(dict)`'s workgroup-per-frame coder over the text of
cniic_amd/csrc/hz_small.hpp -- the pixels in scan order, no dimensions in the text, the 8 raw bytes of the dimensions in front of the pairs).
Every comparison is exact: a frame's status, length, bytes and message are those of cniic_hilbert_zip_encode for that frame alone on a
context that has seen no batch, and the bytes are those of tests/zip_dict_ref.py (hilbert_encode over oracle_lib.hilbert_linearize)
through its C restatement.  Which frames took the route is read from the stage timer "hz_small_batch", whose launch count is the number of
frames given to the kernel; "hz_small_handback" counts those of them the kernel gave up and the workers coded, "hz_small_finished" the
walks the commit wave finished behind the speculation's cap.

What a case claims about a frame -- how its stream ends, its longest match and so which side of a cap it lies on, where its matches stand
against the windows' ends -- is computed from the reference stream alone; tests/test_hz_small_cpu.py asserts the same claims, and the exact
sets of frames handed back, without a GPU."""
import tempfile

import numpy as np
import pytest

import test_zd_small_batch as ZB
import zip_dict_ref as Z
from test_delta_small_batch import _last_error, _pack, _round4, output_buffer

pytestmark = pytest.mark.gpu

MAX_PX = 16384              # kHzSmallMaxPx (cniic_amd/csrc/hz_small.hpp)
WINDOW = 256                # kZsWindow (zd_small.hpp)
SPEC_CAP, GIVE_UP = 32, 1024   # kZsSpecCap, kZsGiveUp
HEAD = 8                    # kHzHead: the raw dimensions
STRIDE_AT_BOUND = 360464    # hz_stride(11 * 16384)
TABLE_BITS_AT_BOUND = 19    # zs_table_bits(11 * 16384)
TIMER, PLACE, HANDBACK, FINISHED = "hz_small_batch", "hz_small_place", "hz_small_handback", "hz_small_finished"
KNOB_OFF, KNOB_MAX_PX, KNOB_FLOOR_OFF, KNOB_CAP = "CNIIC_TEST_HZ_SMALL_OFF", "CNIIC_TEST_HZ_SMALL_MAX_PX", "CNIIC_TEST_HZ_SMALL_FLOOR_OFF", "CNIIC_TEST_HZ_SMALL_CAP"
FAILURES, CAPACITY = (-1, -8), -8
POISON = 0xA5
# (w, h): a text of 11 bytes; 23 and 24 pixels, texts of 253 and 264 bytes on either side of one window; 2^n squares (the table scan);
# rectangles (the general scan); the bound both ways
SIZES = [(1, 1), (2, 1), (1, 2), (3, 2), (23, 1), (24, 1), (2, 2), (4, 4), (64, 64), (128, 128), (100, 37), (128, 96), (16384, 1), (1, 16384)]
UNROUTED = [(16385, 1), (160, 120)]
# the frames of shaped() whose longest match passes GIVE_UP: the kernel hands exactly these back (tests/test_hz_small_cpu.py derives the set)
SHAPED_HANDED_BACK = {"flat 64x64", "flat 128x128", "flat 100x37", "flat 128x96", "flat 16384x1", "flat 1x16384",
                      "two-colour 64x64", "two-colour 128x128", "two-colour 100x37", "two-colour 128x96", "two-colour 16384x1", "two-colour 1x16384"}
EDGE_FRAMES = (22, 42)      # of ZB.many(): first and second matches that end one past a window's end (found by search on the CPU)


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor; test_the_floor holds it"""
    monkeypatch.setenv(KNOB_FLOOR_OFF, "1")


two_colour, banded = ZB.two_colour, ZB.banded
CONTENTS = (("photo", Z.photo_like), ("noise", Z.noise), ("flat", Z.flat), ("two-colour", two_colour))


def shaped():
    """[(name, image)]: every size under every content, two frames of few colours, then the two frames that ride along unrouted"""
    out = [("%s %dx%d" % (nm, w, h), gen(w, h)) for w, h in SIZES for nm, gen in CONTENTS]
    out += [("few colours %d" % k, ZB.many()[k]) for k in EDGE_FRAMES]
    return out + [("photo %dx%d unrouted" % (w, h), Z.photo_like(w, h)) for w, h in UNROUTED]


def routed(imgs, max_px=MAX_PX):
    return [1 <= im.shape[0] * im.shape[1] <= max_px for im in imgs]


# ---- the restatement, and what a stream says about the walks that made it
_CLIB, _WANT = [], {}


def clib():
    if not _CLIB:
        _CLIB.append(Z.compile_c(tempfile.mkdtemp(prefix="hz_small_ref")))
    assert _CLIB[0] is not None, "no C compiler"
    return _CLIB[0]


def restated(img, key=None, lin=None):
    """the stream of tests/zip_dict_ref.py (the C restatement) for img along the built-in scan (or along lin); cached under key"""
    import oracle_lib as O
    if key is None or key not in _WANT:
        h, w = img.shape[:2]
        data = Z.hilbert_encode(lambda t: Z.encode_c(clib(), t), O.hilbert_linearize(img) if lin is None else lin, w, h)
        if key is None:
            return data
        _WANT[key] = data
    return _WANT[key]


def pairs_of(stream):
    return stream[HEAD:]


def longest_match(stream):
    return ZB.longest_match(pairs_of(stream))


def ends_in_eof(stream):
    return ZB.ends_in_eof(pairs_of(stream))


def handed_back(stream, cap=GIVE_UP):
    """the kernel gives a frame up when one of its matches is longer than the cap"""
    return longest_match(stream) > cap


def windows(stream):
    return ZB.windows(pairs_of(stream), WINDOW)


# ---- the calls
_SINGLES = {}


def singles(key, imgs, scan=None):
    """cniic_hilbert_zip_encode of every image alone, on a context that has seen no batch -> [(rc, bytes, message)]; computed once per key"""
    import cniic_amd
    if key not in _SINGLES:
        res = []
        with cniic_amd.Context(0) as ref:
            if scan is not None:
                ref.set_scan(*scan)
            for im in imgs:
                rc, data = ref.hilbert_zip_encode(im, allow=FAILURES)
                res.append((rc, data, _last_error(ref) if rc != 0 else ""))
        _SINGLES[key] = res
    return _SINGLES[key]


def batch(ctx, imgs, stride, host_out=False, host_src=False, poison=0, out_off=None):
    """one cniic_hilbert_zip_encode_batch_var call with the stage timers on
    -> (rc, lens, rcs, streams, raw output, message, frames given to the kernel, frames handed back, walks the commit finished, place launches).
    With out_off (0 .. 15) the output pointer is out_off modulo 16 inside a larger poisoned allocation, and the raw output is then (the whole
    allocation, the index of the output pointer in it)"""
    import torch
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    buf, offs, ws, hs = _pack(imgs)
    F = len(imgs)
    src = buf if host_src else torch.from_numpy(buf).to(dev)
    if out_off is None:
        whole, at = (np.full(stride * F, poison, np.uint8) if host_out else torch.full((stride * F,), poison, dtype=torch.uint8, device=dev)), 0
    else:
        whole, at = output_buffer(stride * F, out_off, host_out, poison)
    out = whole[at:]
    torch.cuda.synchronize()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, lens, rcs = ctx.hilbert_zip_encode_batch_var(src, offs, ws, hs, out, stride, allow=FAILURES)
        msg = _last_error(ctx) if rc != 0 else ""
        marks = tuple(ctx.kernel_time(name)[1] for name in (TIMER, HANDBACK, FINISHED, PLACE))
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    whole = whole if host_out else whole.cpu().numpy()
    host = whole[at:]
    streams = [host[f * stride:f * stride + lens[f]].tobytes() if rcs[f] == 0 else None for f in range(F)]
    return (rc, lens, rcs, streams, host if out_off is None else (whole, at), msg) + marks


def check_against_singles(res, want, what):
    rc, lens, rcs, streams, _, msg = res[:6]
    for f, (src, sdata, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        if src == 0:
            assert lens[f] == len(sdata) and streams[f] == sdata, (what, f)
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first]), what
    if first is not None:
        assert msg == want[first][2], (what, msg, want[first][2])


def check(res, want, imgs, what, key=None):
    """against the single calls, and those against the restatement"""
    check_against_singles(res, want, what)
    for f, im in enumerate(imgs):
        assert want[f][0] == 0 and want[f][1] == restated(im, None if key is None else "%s %d" % (key, f)), (what, f)


def _stride(want):
    return _round4(max(len(s[1]) for s in want)) + 4


def no_marks(ctx):
    """not merely zero launches: no such stage"""
    return all(ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, None) != 0 for name in (TIMER, PLACE, HANDBACK, FINISHED))


# ---- the tests
def test_the_three_entry_points_exist():
    import cniic_amd
    from cniic_amd import _lib
    with cniic_amd.Context(0) as ctx:
        for name in ("cniic_hilbert_zip_encode_batch_var", "cniic_hilbert_zip_decode_batch", "cniic_hilbert_zip_measure_batch"):
            assert name in _lib.PROTOTYPES and hasattr(ctx._L, name), name
        # frames == 0: nothing is looked at
        assert ctx.hilbert_zip_encode_batch_var(None, [], [], [], None, 0)[0] == 0
        assert ctx.hilbert_zip_decode_batch(None, 0, [], 0, None, 0)[0] == 0
        assert ctx.hilbert_zip_measure_batch(None, [], [], [])[0] == 0


def test_every_shape_and_content():
    import cniic_amd
    names, imgs = zip(*shaped())
    assert [im.shape[0] * im.shape[1] for im in imgs[-2:]] == [16385, 19200] and sum(routed(imgs)) == len(imgs) - 2 == 4 * len(SIZES) + len(EDGE_FRAMES)
    want = singles("shapes", imgs)
    by = dict(zip(names, (s[1] for s in want)))
    assert len(by["photo 1x1"]) == HEAD + 4 * 5 and {nm for nm in names[:-2] if handed_back(by[nm])} == SHAPED_HANDED_BACK
    assert {ends_in_eof(by[nm]) for nm in names if nm.startswith(("photo", "noise"))} == {False, True}
    first, second = set(), set()
    for nm in names[:-2]:
        if nm not in SHAPED_HANDED_BACK:
            a, b = windows(by[nm])
            first |= a
            second |= b
    assert first == second == {-1, 0, 1}
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride, poison=POISON)
    assert res[6] == len(imgs) - 2 and res[7] == len(SHAPED_HANDED_BACK) and res[8] > 0 and res[9] == 1, res[6:]
    check(res, want, imgs, "shapes", "shapes")
    for f in range(len(imgs)):
        assert bool((res[4][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), names[f]


def cap_frames():
    """(name, image): flat, two-colour and banded frames, and three good ones"""
    return [("flat 8x8", Z.flat(8, 8)), ("flat 32x32", Z.flat(32, 32)), ("two-colour 13x5", two_colour(13, 5)), ("two-colour 32x32", two_colour(32, 32)),
            ("band 40", banded(64, 64, 2000, 40)), ("band 300", banded(64, 64, 2000, 300)), ("flat 2x1", Z.flat(2, 1)),
            ("photo 32x32", Z.photo_like(32, 32)), ("noise 13x5", Z.noise(13, 5)), ("photo 64x64", Z.photo_like(64, 64))]


CAPS = (8, 20, 100, 300, GIVE_UP)
# the frames of cap_frames() handed back under each cap (tests/test_hz_small_cpu.py derives them)
CAP_HANDED_BACK = {
    8: {"flat 8x8", "flat 32x32", "two-colour 13x5", "two-colour 32x32", "band 40", "band 300", "photo 32x32", "noise 13x5", "photo 64x64"},
    20: {"flat 8x8", "flat 32x32", "two-colour 13x5", "two-colour 32x32", "band 40", "band 300"},
    100: {"flat 8x8", "flat 32x32", "two-colour 32x32", "band 300"},
    300: {"flat 32x32", "two-colour 32x32", "band 300"},
    GIVE_UP: {"flat 32x32"},
}


@pytest.mark.parametrize("cap", CAPS)
def test_frames_on_both_sides_of_the_caps(cap, monkeypatch):
    """the knob lowers the give-up cap, and the speculation's cap with it where it is lower: every frame alone and all together"""
    import cniic_amd
    names, imgs = zip(*cap_frames())
    want = singles("caps", imgs)
    back = [handed_back(s[1], cap) for s in want]
    assert {nm for nm, b in zip(names, back) if b} == CAP_HANDED_BACK[cap]
    stride = _stride(want)
    monkeypatch.setenv(KNOB_CAP, str(cap))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride)
        assert res[6] == len(imgs) and res[7] == sum(back), (cap, res[6:])
        if cap > SPEC_CAP:       # a frame that stays has a match between the two caps: the commit wave finished that walk
            assert any(SPEC_CAP < longest_match(s[1]) <= cap for s in want) and res[8] > 0
        check(res, want, imgs, "cap %d" % cap, "caps")
        for f in range(len(imgs)):
            one = batch(ctx, imgs[f:f + 1], stride)
            assert one[6] == 1 and one[7] == int(back[f]), (cap, names[f])
            check_against_singles(one, want[f:f + 1], "cap %d, %s alone" % (cap, names[f]))


def machinery_frames():
    """frames of many stream lengths, all on the route but the last two; the second is handed back"""
    return [Z.photo_like(64, 64), Z.flat(40, 40), Z.noise(37, 41), Z.photo_like(100, 75), np.array([[[9, 8, 7]]], np.uint8), two_colour(8, 8), Z.photo_like(7, 9),
            Z.noise(32, 32), Z.photo_like(128, 96), Z.photo_like(16385, 1), Z.photo_like(160, 120)]


MACHINERY_HANDED_BACK = [False, True] + [False] * 7


def test_route_off_and_a_lowered_bound(monkeypatch):
    import cniic_amd
    imgs = machinery_frames()
    want = singles("machinery", imgs)
    assert [handed_back(s[1]) for s in want[:9]] == MACHINERY_HANDED_BACK
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, imgs, stride)
        monkeypatch.setenv(KNOB_OFF, "1")
        off = batch(ctx, imgs, stride)
        assert no_marks(ctx)
        monkeypatch.delenv(KNOB_OFF)
        monkeypatch.setenv(KNOB_MAX_PX, "1024")
        low = batch(ctx, imgs, stride)
        monkeypatch.delenv(KNOB_MAX_PX)
    assert on[6] == len(imgs) - 2 and on[7] == 1 and off[6] == 0 and low[6] == sum(routed(imgs, 1024)) == 4 and low[7] == 0
    for res, what in ((off, "route off"), (low, "bound 1024")):
        assert on[:4] == res[:4], what
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
        assert res[6] == len(imgs) - 2 and res[7] == 1
        check_against_singles(res, want, "host out")
        for f in range(len(imgs)):
            assert bool((res[4][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), f


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
    assert res[6] == F and res[0] == 0 and res[7] == 0
    check_against_singles(res, want, "placement %d" % out_off)
    (whole, at), lens = res[4], res[1]
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
        rc, lens, rcs, streams, host, msg, launches, back = batch(ctx, imgs, stride, host_out=host_out, poison=POISON)[:8]
        one = ctx.hilbert_zip_encode(imgs[big], out=np.full(stride, POISON, np.uint8), allow=FAILURES)
        assert one == (CAPACITY, len(want[big][1])) and _last_error(ctx) == msg
    assert launches == len(imgs) and rc == CAPACITY and back == 1
    assert msg == "encode: stream is %d bytes, capacity %d" % (len(want[big][1]), stride)
    for f in range(len(imgs)):
        assert lens[f] == len(want[f][1]), f
        if f == big:
            assert rcs[f] == CAPACITY and bool((host[f * stride:(f + 1) * stride] == POISON).all())
        else:
            assert rcs[f] == 0 and streams[f] == want[f][1], f
            assert bool((host[f * stride + lens[f]:(f + 1) * stride] == POISON).all()), f


def test_many_frames_in_one_launch():
    import cniic_amd
    imgs = ZB.many()
    assert len(imgs) == 3000 and len({im.shape[:2] for im in imgs}) == 8 and max(im.shape[0] * im.shape[1] for im in imgs) == 1024
    sample = range(0, 3000, 59)
    wants = {f: restated(imgs[f]) for f in sample}
    assert len({len(s) for s in wants.values()}) > 8 and not any(handed_back(s) for s in wants.values())
    stride = HEAD + 2 * 11 * 1024 + 4
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, streams, host, msg, launches, back, fin, places = batch(ctx, imgs, stride)
        assert launches == 3000 and rc == 0 and rcs == [0] * 3000 and back == 0 and places == 1
        with cniic_amd.Context(0) as ref:
            for f in range(0, 3000, 75):
                src, sdata = ref.hilbert_zip_encode(imgs[f])
                assert src == 0 and streams[f] == sdata, f
    for f in sample:
        assert streams[f] == wants[f], f


def frame_bytes(npx):
    """hz_small_frame_bytes (codec.cpp): the slot, the table, the row and the result row"""
    N = 11 * npx
    bits = 10
    while (1 << bits) < 2 * (N + 256):
        bits += 1
    return ((HEAD + 2 * N + 2 + 15) & ~15) + (8 << bits) + 16 + 16


def tiny(count):
    return [Z.photo_like(5, 3 + k % 6) for k in range(count)]


def test_chunks(monkeypatch):
    """hz_small_encode sizes a chunk by the slot and the table of its first (largest) frame under CNIIC_TEST_MEASURE_BUDGET"""
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
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        three = batch(ctx, imgs, stride)
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", "1")                 # a frame a chunk
        each = batch(ctx, imgs, stride)
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert one[9] == 1 and three[9] == 3 and each[9] == n_routed - 1         # (the frame handed back places nothing)
    for res in (three, each):
        assert res[6] == n_routed and res[7] == 1 and res[:4] == one[:4]
    check_against_singles(three, want, "three chunks")


def test_the_floor_keeps_every_class_with_the_workers(monkeypatch):
    """no class of calls was clear of the workers for photo-like, noise and flat frames alike (NOTES AS), so with the floor on no frame
    takes the route, however many or small they are, and no mark is reported; the knob takes the floor away"""
    import cniic_amd
    monkeypatch.delenv(KNOB_FLOOR_OFF)
    imgs = [Z.photo_like(64, 64), Z.photo_like(128, 128)] + tiny(298)
    want6 = singles("floor", imgs[:8])
    want = want6[:2] + [want6[2 + k % 6] for k in range(298)]
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        for count in (1, 2, 256, 300):
            res = batch(ctx, imgs[:count], stride)
            assert res[6] == 0 and no_marks(ctx), count
            check_against_singles(res, want[:count], "floor on, %d frames" % count)
        monkeypatch.setenv(KNOB_FLOOR_OFF, "1")
        res = batch(ctx, imgs[:3], stride)
        assert res[6] == 3
        check_against_singles(res, want[:3], "floor off")


def chunk_sizes(px, budget):
    """for_chunks (codec.cpp): the frames largest first, a chunk as many as the budget holds at the size of its first frame, one at least"""
    px, at, out = sorted(px, reverse=True), 0, []
    while at < len(px):
        out.append(min(len(px) - at, max(1, budget // frame_bytes(px[at]))))
        at += out[-1]
    return out


def test_chunks_one_of_which_holds_a_single_frame(monkeypatch):
    """many small frames behind two larger ones under a small scratch budget: four chunks, the last of one frame"""
    import cniic_amd
    imgs = [Z.photo_like(64, 64), Z.noise(64, 64)] + tiny(265)
    want8 = singles("chunks small", imgs[:8])
    want = want8[:2] + [want8[2 + k % 6] for k in range(265)]
    stride = _stride(want)
    budget = 2 * frame_bytes(4096)
    sizes = chunk_sizes([im.shape[0] * im.shape[1] for im in imgs], budget)
    assert sizes == [2, 131, 133, 1]          # (a chunk that starts at a smaller frame holds more: its table is smaller)
    monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, imgs, stride)
    assert res[6] == len(imgs) and res[7] == 0 and res[9] == len(sizes)
    check_against_singles(res, want, "chunks")


def test_a_size_with_an_injected_scan_stays_with_the_workers():
    """those frames carry the injected order, the others take the route"""
    import cniic_amd
    imgs = [Z.photo_like(64, 64), Z.noise(37, 41), Z.photo_like(37, 41), Z.photo_like(41, 37), Z.noise(8, 8)]
    w, h = 37, 41
    p = np.random.default_rng(7).permutation(w * h)
    scan = (w, h, np.stack([p % w, p // w], 1).astype(np.uint32))
    want = singles("scan", imgs, scan=scan)
    builtin = singles("scan builtin", imgs)
    for f, im in enumerate(imgs):
        injected = im.shape[:2] == (h, w)
        assert (want[f][1] != builtin[f][1]) == injected and builtin[f][1] == restated(im), f
        if injected:
            assert want[f][1] == restated(im, lin=im.reshape(-1, 3)[p])
    with cniic_amd.Context(0) as ctx:
        ctx.set_scan(*scan)
        res = batch(ctx, imgs, _stride(want))
        assert res[6] == 3
        check_against_singles(res, want, "injected scan")
        ctx.set_scan(w, h, None)
        res = batch(ctx, imgs, _stride(want))
        assert res[6] == 5
        check_against_singles(res, builtin, "scan taken back")


def test_alternating_calls_with_other_codecs_on_one_context():
    import cniic_amd
    import test_delta_small_batch as D
    imgs = machinery_frames()[:9]
    want = singles("machinery", machinery_frames())[:9]
    other = [Z.noise(16, 16), Z.flat(8, 8), Z.photo_like(128, 128)]
    stride = _stride(want)
    with cniic_amd.Context(0) as ctx:
        for turn in range(2):
            res = batch(ctx, imgs, stride)
            assert res[6] == 9 and res[7] == 1
            check_against_singles(res, want, "turn %d" % turn)
            for expr, timer in (("zip(dict)", ZB.TIMER), ("hilbert(rle)", "rle_small_batch")):
                got = D.batch(ctx, expr, other, 400000, timer=timer)
                assert got[0] == 0 and no_marks(ctx), expr                  # the expression calls never report the hz marks
                for f, im in enumerate(other):
                    rc, data, st = ctx.encode(expr, im)
                    assert rc == 0 and got[4][f] == data, (expr, f)
            rc, data = ctx.hilbert_zip_encode(imgs[0])
            assert rc == 0 and data == want[0][1]


def test_the_expression_calls_reject_the_codec_and_never_report_the_marks(monkeypatch):
    import cniic_amd
    import test_delta_small_batch as D
    from cniic_amd import _lib
    monkeypatch.setenv("CNIIC_TEST_ZD_SMALL_FLOOR_OFF", "1")
    imgs = machinery_frames()[:8]
    assert _lib.codec_parse_f64("hilbert(zip)") is None
    with cniic_amd.Context(0) as ctx:
        for expr, timer in (("zip(dict)", ZB.TIMER), ("hufman", "huf_small_batch")):
            res = D.batch(ctx, expr, imgs, 400000, timer=timer)
            assert res[0] == 0 and res[6] == 8 and no_marks(ctx), expr
        rc, lens, rcs, sts = ctx.encode_batch_var("hilbert(zip)", np.zeros(3, np.uint8), [0], [1], [1], np.zeros(64, np.uint8), 64, allow=(-1,))
        assert rc == -1 and _last_error(ctx) == "Malformed codec argument: hilbert(zip)"


def test_measure_batch_is_the_loop_of_the_three_single_calls():
    import torch
    import cniic_amd
    from cniic_amd import _lib
    dev = torch.device("cuda", 0)
    imgs = machinery_frames() + [Z.photo_like(333, 200)]
    want = singles("measure", imgs)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        codec = cniic_amd.HilbertZip(ctx)
        rows_want = []
        for im, (rc, data, _) in zip(imgs, want):
            back = codec.decode(data)
            assert back is not None and np.array_equal(back, im)
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
        buf, offs, ws, hs = _pack(imgs)
        F = len(imgs)
        stride = _stride(want) + 4
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.hilbert_zip_measure_batch(src, offs, ws, hs, out, stride, allow=FAILURES)
        launches, places, back = ctx.kernel_time(TIMER)[1], ctx.kernel_time(PLACE)[1], ctx.kernel_time(HANDBACK)[1]     # the encode's stages, readable after the decode
        dec = ctx.kernel_time("hz_small_dec_batch")[1]
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert launches == sum(routed(imgs)) == F - 3 and places == 1 and back == 1 and rc == 0
        assert dec == sum(1 <= im.shape[0] * im.shape[1] <= 4096 for im in imgs) == 7          # (the decode's own floor: 9 candidates, those of at most 4096 pixels)
        host = out.cpu().numpy()
        for f in range(F):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f] and rows[f]["lossless_mismatch"] == 0, (f, got, rows_want[f])
            assert lens[f] == len(want[f][1]) and host[f * stride:f * stride + lens[f]].tobytes() == want[f][1], f
        # the class: rows with the reference's CSV columns, from host images
        got = codec.measure(imgs[:5])
        for f in range(5):
            assert {k: got[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")} == rows_want[f], f
        assert codec.measure(imgs[:2], seed=7, max_iters=3)[1]["compressed_size"] == rows_want[1]["compressed_size"]      # (Codec.measure's options: taken)
        assert codec.encode_batch(imgs[:5]) == [s[1] for s in want[:5]] == codec.encode_batch(imgs[:5], allow=(CAPACITY,))
        # headers that lie among good streams: no room is taken from a claim of 2^32 pixels; the calls are bounded by DECODE_BATCH_BYTES
        import struct
        hostile = struct.pack("<II", 65536, 65536) + want[0][1][HEAD:]
        got = codec.decode_batch([s[1] for s in want[:5]] + [hostile, want[4][1][:7]])
        assert got[5] is None and got[6] is None
        for im, back in zip(imgs[:5], got):
            assert np.array_equal(im, back)
        codec.DECODE_BATCH_BYTES = 3 * 4096          # (an instance's own bound: several calls, and the frame of 7500 pixels alone)
        for im, back in zip(imgs[:5], codec.decode_batch([s[1] for s in want[:5]])):
            assert np.array_equal(im, back)


def test_the_harness_writes_hilbert_zip_csv_in_a_loop_and_in_one_call(tmp_path):
    """tools/cniic_bench takes the reference's spelling itself (the library's parser rejects it) and writes the Makefile's hilbert-zip.csv"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "cniic_bench")
    assert os.path.exists(exe), "tools/cniic_bench is built by `make -C cniic_amd/csrc`"
    imgs = [Z.photo_like(96, 64), Z.noise(40, 33), Z.photo_like(200, 120)]
    names = []
    for i, im in enumerate(imgs):
        names.append("img%d.ppm" % i)
        with open(tmp_path / names[-1], "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
    r = subprocess.run([exe, "--codec=hilbert(zip)"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    loop = open(tmp_path / "output" / "hilbert-zip.csv").read().strip().split("\n")
    r = subprocess.run([exe, "--codec=hilbert(zip)", "--one-call"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    one = open(tmp_path / "output" / "hilbert-zip.csv").read().strip().split("\n")
    assert one[0] == loop[0] == "name,compressed_size,compression_ratio,error"
    assert [l.split(",")[0] for l in one[1:]] == names and sorted(one[1:]) == sorted(loop[1:])
    for line, im in zip(one[1:], imgs):
        size = len(restated(im))
        assert line.split(",")[1] == str(size) and float(line.split(",")[2]) == size / (im.shape[0] * im.shape[1] * 24.0) * 100.0 and float(line.split(",")[3]) == 0.0
