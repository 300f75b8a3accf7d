"""Small `delta` frames of cniic_codec_decode_batch / cniic_codec_measure_batch on the small-frame decode route (k_delta_small_dec.hip: a
workgroup per frame from the payload to the pixels in place; include/cniic_hip.h above cniic_codec_decode_batch).  Every comparison is
exact: a frame's status, dimensions, pixels and message are those of cniic_codec_decode for that stream alone on a context that has seen
no batch; lossless frames are also the source image and, up to 128 x 128, the oracle's decode.  Which frames took the route is read from the
stage timer "delta_small_dec_batch", whose launch count is the number of routed frames (a frame the kernel hands back included): on a
build without the route that timer does not exist.

The streams are the library's own (byte-equal to the oracle's, asserted once), cut, edited or built by hand where a test says so;
tests/test_delta_small_decode_cpu.py establishes from the oracle alone what each of those is.  This module imports no GPU code at its top."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_PX = 16384        # kDeltaSmallDecMaxPx (cniic_amd/csrc/delta_small_dec.hpp)
MAX_CODE_LEN = 19     # kDeltaSmallMaxCodeLen
LANES = 1024          # kDsdLanes
OK, DECODE, CAPACITY = 0, -6, -8
TIMER, ENC_TIMER = "delta_small_dec_batch", "delta_small_batch"
MSG_SHORT = "delta: cannot decode the difference stream"
MSG_RANGE = "delta: colour out of range (hilbertc.rs:505)"
MSG_DIMS = "decode: truncated dimensions"
POISON = 0xA5
# (w, h): 1, 2, 2, 64 pixels; 63 / 64 / 65; 1023 / 1024 / 1025; 2047 / 2048 / 2049; rectangles, lines, 2^n squares, 16 383 and 16 384
SIZES = [(1, 1), (2, 1), (1, 2), (8, 8), (9, 7), (64, 1), (13, 5), (33, 31), (32, 32), (41, 25), (23, 89), (64, 32), (3, 683), (37, 29), (100, 75),
         (700, 1), (1, 700), (64, 64), (128, 96), (127, 129), (128, 128)]
ORACLE_MAX_PX = 128 * 128


# ------------------------------------------------------------------ images and streams (no GPU)
@functools.lru_cache(maxsize=None)
def route_images():
    """per size a photo-like, a noise and a flat frame; then an all-black one (a single zero difference: a one-leaf decoder)"""
    from cniic_amd import synth
    imgs = []
    for i, (w, h) in enumerate(SIZES):
        imgs += [synth.photo(w, h, synth.SEED0 + 8100 + i), synth.uniform(w, h, synth.SEED0 + 8200 + i), np.full((h, w, 3), 60 + i, np.uint8)]
    imgs.append(np.zeros((20, 30, 3), np.uint8))
    return imgs


def parse_trie(data):
    """the pre-order trie of a `delta` stream -> (leaves [(offset of the six symbol bytes, depth)], offset of the payload)"""
    pos, leaves, pending = 8, [], [0]
    while pending:
        depth = pending.pop()
        tag = data[pos]
        pos += 1
        if tag == 1:
            pending += [depth + 1, depth + 1]
        else:
            assert tag == 0
            leaves.append((pos, depth))
            pos += 6
    return leaves, pos


def leaf_bytes(d):
    return b"".join(int(v).to_bytes(2, "little", signed=True) for v in d)


def rewrite_leaf(data, diff_from, diff_to):
    """the stream with the first leaf that holds diff_from rewritten to diff_to"""
    leaves, _ = parse_trie(data)
    at = next(o for o, _ in leaves if data[o:o + 6] == leaf_bytes(diff_from))
    return data[:at] + leaf_bytes(diff_to) + data[at + 6:]


def range_image():
    """8 x 8, grey 100 everywhere but one pixel of 130 in the middle of the scan: differences (100,100,100), 0, (30,30,30), (-30,-30,-30)"""
    import oracle_lib as O
    img = np.full((8, 8, 3), 100, np.uint8)
    x, y = O.hilbert_iter(8, 8)[30]
    img[y, x] = 130
    return img


def deep_stream():
    """a trie one level deeper than the route takes, by hand: a chain of 21 leaves (depths 1, 2, ..., 19, 20, 20); 8 x 8 pixels, the first symbol
    the deepest leaf (7, 8, 9), then 63 times the first leaf (0, 0, 0): twenty ones, then zeros"""
    out = (8).to_bytes(4, "little") + (8).to_bytes(4, "little")
    for k in range(20):
        out += b"\x01\x00" + leaf_bytes((0, 0, 0) if k == 0 else (k, 0, 0))
    out += b"\x00" + leaf_bytes((7, 8, 9))
    bits = "1" * 20 + "0" * 63
    bits += "0" * (-len(bits) % 8)
    return out + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def failure_streams(good):
    """good: the stream of range_image().  -> [(name, stream, expected rc, expected message or None, routed)] among which the good ones stand"""
    leaves, pay = parse_trie(good)
    assert len(leaves) == 4 and len(good) - pay >= 8
    return [
        ("good", good, OK, None, True),
        ("cut in the dimensions", good[:5], DECODE, MSG_DIMS, False),
        ("cut in the trie", good[:8 + 10], DECODE, MSG_SHORT, False),
        ("cut at the first payload byte", good[:pay], DECODE, MSG_SHORT, False),
        ("good again", good, OK, None, True),
        ("cut in the payload", good[:pay + (len(good) - pay) // 2], DECODE, MSG_SHORT, True),
        ("one byte short", good[:-1], DECODE, MSG_SHORT, True),
        ("one byte more", good + b"\x5a", OK, None, True),
        ("above 255", rewrite_leaf(good, (30, 30, 30), (30, 156, 30)), DECODE, MSG_RANGE, True),
        ("below 0", rewrite_leaf(good, (-30, -30, -30), (-131, -30, -30)), DECODE, MSG_RANGE, True),
        ("a code of 20 bits", deep_stream(), OK, None, False),
        ("good at the end", good, OK, None, True),
    ]


MUTANT_SEED = 20240612
MUTANTS = 200
MUTANT_STRIDE = 3 * 37 * 29 + 13     # bytes between the mutants' images: what a decode of one of them may write


def mutant_streams(base_small, base_large):
    """200 streams: the 8 x 8 and the 37 x 29 stream in turn, one to three random bytes of each replaced"""
    rng = np.random.default_rng(MUTANT_SEED)
    out = []
    for k in range(MUTANTS):
        s = bytearray(base_large if k % 2 else base_small)
        for _ in range(int(rng.integers(1, 4))):
            s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
        out.append(bytes(s))
    return out


def mutant_sources():
    from cniic_amd import synth
    return synth.photo(8, 8, synth.SEED0 + 8300), synth.photo(37, 29, synth.SEED0 + 8301)


# ------------------------------------------------------------------ GPU helpers
def _last_error(ctx):
    return (ctx._L.cniic_last_error(ctx.h) or b"").decode()


_ENC = {}


def encoded(key, imgs):
    """the library's own `delta` streams of imgs, each encoded alone; computed once per key"""
    import cniic_amd
    if key not in _ENC:
        with cniic_amd.Context(0) as ref:
            res = []
            for im in imgs:
                rc, data, _ = ref.encode("delta", im)
                assert rc == 0
                res.append(data)
        _ENC[key] = res
    return _ENC[key]


_SINGLES = {}


def singles(key, expr, streams, cap, scan=None):
    """cniic_codec_decode of every stream alone (capacity cap), on a context that has seen no batch -> [(rc, w, h, pixels or None, message)]"""
    import cniic_amd
    if key not in _SINGLES:
        res = []
        with cniic_amd.Context(0) as ref:
            if scan is not None:
                ref.set_scan(*scan)
            for s in streams:
                out = np.zeros(max(cap, 1), np.uint8)
                raw = np.frombuffer(bytes(s) + b"\0", np.uint8)
                rc, w, h = ref.decode_into(expr, raw, len(s), out[:cap], allow=(DECODE, CAPACITY))
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


def batch(ctx, expr, streams, img_stride, stride=None, host_src=False, host_out=False, src_off=0, out_off=0):
    """one cniic_codec_decode_batch call with the stage timers on -> (rc, ws, hs, rcs, output as a host array, routed frames, message).  The
    stream of frame f lies at src_off + f * stride modulo 16, its image at out_off + f * img_stride modulo 16, inside poisoned allocations."""
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
        msg = _last_error(ctx) if rc != 0 else ""
        launches = ctx.kernel_time(TIMER)[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = whole if host_out else whole.cpu().numpy()
    assert bool((host[:at] == POISON).all()) and bool((host[at + img_stride * F:] == POISON).all())    # nothing before the first image or behind the last
    return rc, ws, hs, rcs, host[at:at + img_stride * F], launches, msg


def check_against_singles(res, want, img_stride, what, sources=None):
    rc, ws, hs, rcs, host = res[:5]
    for f, (src, sw, sh, spx, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        slot = host[f * img_stride:(f + 1) * img_stride]
        if src == 0:
            assert (ws[f], hs[f]) == (sw, sh), (what, f)
            assert np.array_equal(slot[:sw * sh * 3], spx), (what, f)
            assert bool((slot[sw * sh * 3:] == POISON).all()), (what, f)          # nothing behind an image's end
            if sources is not None and sources[f] is not None:
                assert np.array_equal(spx, sources[f].reshape(-1)), (what, f)
        else:
            assert bool((slot == POISON).all()), (what, f)                          # a frame that fails leaves its destination alone
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first]), what
    if first is not None:
        assert res[6] == want[first][4], (what, res[6], want[first][4])


def routed(streams, max_px=MAX_PX):
    return sum(1 for s in streams if 1 <= int.from_bytes(s[0:4], "little") * int.from_bytes(s[4:8], "little") <= max_px)


# ------------------------------------------------------------------ the tests
def test_route_and_bytes():
    import cniic_amd
    import oracle_lib as O
    imgs = route_images()
    streams = encoded("route", imgs)
    img_stride = 3 * MAX_PX
    want = singles("route", "delta", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    for f, im in enumerate(imgs):
        if im.shape[0] * im.shape[1] <= ORACLE_MAX_PX:
            rco, edata, _ = O.encode("delta", im)
            assert rco == 0 and streams[f] == edata, f                                # the oracle's streams are byte-equal
            rcd, back = O.decode("delta", streams[f])
            assert rcd == 0 and np.array_equal(back.reshape(-1), want[f][3]), f
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", streams, img_stride)
    assert res[5] == len(imgs) == routed(streams)
    check_against_singles(res, want, img_stride, "delta", sources=imgs)


def test_same_batch_with_the_route_off(monkeypatch):
    import cniic_amd
    imgs = route_images()
    streams = encoded("route", imgs)
    img_stride = 3 * MAX_PX
    want = singles("route", "delta", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        on = batch(ctx, "delta", streams, img_stride)
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_DEC_OFF", "1")
        off = batch(ctx, "delta", streams, img_stride)
        assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0    # no launches: the stage is not there
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_DEC_OFF")
    assert on[5] == len(imgs) and off[5] == 0
    assert on[:4] == off[:4] and np.array_equal(on[4], off[4])
    check_against_singles(off, want, img_stride, "route off", sources=imgs)


def test_threshold(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    imgs = [synth.photo(128, 128, synth.SEED0 + 8400), synth.photo(5, 3277, synth.SEED0 + 8401), synth.photo(256, 130, synth.SEED0 + 8402),
            synth.photo(64, 64, synth.SEED0 + 8403), synth.photo(17, 241, synth.SEED0 + 8404)]
    assert [im.shape[0] * im.shape[1] for im in imgs] == [16384, 16385, 33280, 4096, 4097]
    streams = encoded("threshold", imgs)
    img_stride = 3 * 33280
    want = singles("threshold", "delta", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", streams, img_stride)
        assert res[5] == 3
        check_against_singles(res, want, img_stride, "16384 | 16385", sources=imgs)
        res = batch(ctx, "delta", streams[1:3], img_stride)
        assert res[5] == 0
        check_against_singles(res, want[1:3], img_stride, "above the bound alone", sources=imgs[1:3])
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_DEC_MAX_PX", "4096")
        res = batch(ctx, "delta", streams, img_stride)
        assert res[5] == 1
        check_against_singles(res, want, img_stride, "4096 | 4097", sources=imgs)
        res = batch(ctx, "delta", streams[4:], img_stride)
        assert res[5] == 0
        check_against_singles(res, want[4:], img_stride, "4097 alone", sources=imgs[4:])
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_DEC_MAX_PX")


EDGE_NAMES = ("chain19", "all_distinct", "stairs", "flat128", "black128", "equal16", "distinct_127x129", "distinct_16384x1", "distinct_2x8192", "low_9x7",
              "distinct_13x5")


def test_the_kernel_s_own_limits(monkeypatch):
    """the prescribed-difference frames of tests/delta_small_edges.py: a 19-bit longest code, 16 384 leaves, 16 384 symbols of one count"""
    import cniic_amd
    import delta_small_edges as E
    assert E.CLAIMS["chain19"][1] == MAX_CODE_LEN and E.CLAIMS["all_distinct"][0] == MAX_PX and E.MAX_PX == MAX_PX
    imgs = [E.image(nm) for nm in EDGE_NAMES]
    streams = [E.oracle_stream(nm) for nm in EDGE_NAMES]
    img_stride = 3 * MAX_PX + 5
    want = singles("edges", "delta", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    small = [f for f, im in enumerate(imgs) if im.shape[0] * im.shape[1] <= 4096]
    assert len(small) >= 3
    with cniic_amd.Context(0) as ctx:
        for f in range(len(streams)):                                                   # alone: the launch's LDS follows the frame
            res = batch(ctx, "delta", streams[f:f + 1], img_stride)
            assert res[5] == 1, EDGE_NAMES[f]
            check_against_singles(res, want[f:f + 1], img_stride, EDGE_NAMES[f], sources=imgs[f:f + 1])
        res = batch(ctx, "delta", streams, img_stride)                                  # in company with 16 384-pixel frames
        assert res[5] == len(streams)
        check_against_singles(res, want, img_stride, "edges together", sources=imgs)
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_DEC_MAX_PX", "4096")                 # the capacity follows the small frames
        res = batch(ctx, "delta", streams, img_stride)
        assert res[5] == len(small)
        check_against_singles(res, want, img_stride, "edges, bound 4096", sources=imgs)
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_DEC_MAX_PX")


@pytest.mark.parametrize("host_src,host_out", ((False, False), (True, True), (False, True), (True, False)))
def test_destinations_and_payloads_at_every_alignment(host_src, host_out):
    import cniic_amd
    imgs = [im for im in route_images() if im.shape[0] * im.shape[1] <= 2049][:34]
    streams = encoded("route", route_images())[:len(imgs)]
    assert len(imgs) == 34
    img_stride = 3 * 2049 + 2                                                           # odd: the images start at every residue modulo 16
    stride = ((max(len(s) for s in streams) + 3) & ~3) + 1                              # odd: the streams at every byte shift
    assert {(f * img_stride) % 16 for f in range(len(imgs))} == set(range(16)) and {(f * stride) % 4 for f in range(len(imgs))} == set(range(4))
    leaves_pay = [parse_trie(s)[1] for s in streams]
    assert {(f * stride + p) % 4 for f, p in enumerate(leaves_pay) if len(streams[f]) > p} == set(range(4))   # and so do the payloads
    want = singles("align", "delta", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    with cniic_amd.Context(0) as ctx:
        for src_off, out_off in ((0, 0), (1, 7), (3, 15)):
            res = batch(ctx, "delta", streams, img_stride, stride=stride, host_src=host_src, host_out=host_out, src_off=src_off, out_off=out_off)
            assert res[5] == len(imgs)
            check_against_singles(res, want, img_stride, (host_src, host_out, src_off, out_off), sources=imgs)


@pytest.mark.parametrize("host", (False, True))
def test_failures_among_good_frames(host):
    import cniic_amd
    good = encoded("range", [range_image()])[0]
    cases = failure_streams(good)
    streams = [c[1] for c in cases]
    img_stride = 3 * 64 + 7
    want = singles("failures", "delta", streams, img_stride)
    for (name, s, rc, msg, _), (src, sw, sh, spx, smsg) in zip(cases, want):
        assert src == rc and (msg is None or smsg == msg), (name, src, smsg)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", streams, img_stride, host_src=host, host_out=host)
        assert res[5] == sum(c[4] for c in cases)
        check_against_singles(res, want, img_stride, "failures")
        assert res[0] == DECODE and res[6] == MSG_DIMS                                  # the first failure's
        for first in (5, 8, 9):                                                         # each routed failure first in a batch: its message
            res = batch(ctx, "delta", streams[first:], img_stride, host_src=host, host_out=host)
            check_against_singles(res, want[first:], img_stride, cases[first][0])
            assert res[6] == cases[first][3]


def test_the_hand_back(monkeypatch):
    import cniic_amd
    from cniic_amd import synth
    imgs = [synth.uniform(128, 128, synth.SEED0 + 8500), synth.photo(64, 64, synth.SEED0 + 8501), np.zeros((9, 9, 3), np.uint8)]
    streams = encoded("handback", imgs)
    img_stride = 3 * MAX_PX + 1
    want = singles("handback", "delta", streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_DEC_ROUNDS", "1")
        res = batch(ctx, "delta", streams, img_stride)
        monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_DEC_ROUNDS")
        assert res[5] == 3                                                              # the launch took all three; the workers decoded what it handed back
        check_against_singles(res, want, img_stride, "one round", sources=imgs)
        res = batch(ctx, "delta", streams, img_stride)
        assert res[5] == 3
        check_against_singles(res, want, img_stride, "all rounds", sources=imgs)


def test_many_frames_in_one_launch():
    import cniic_amd
    rng = np.random.default_rng(44)
    kinds = [(rng.integers(0, 32, (16, 16, 3)) * 8).astype(np.uint8) for _ in range(40)]
    kstreams = encoded("many", kinds)
    streams = [kstreams[f % 40] for f in range(3000)]
    img_stride = 3 * 256 + 3
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", streams, img_stride)
    assert res[5] == 3000 and res[0] == 0 and res[3] == [0] * 3000
    for f in range(3000):
        slot = res[4][f * img_stride:(f + 1) * img_stride]
        assert np.array_equal(slot[:768], kinds[f % 40].reshape(-1)) and bool((slot[768:] == POISON).all()), f


def test_two_chunks_of_scratch(monkeypatch):
    import cniic_amd
    imgs = route_images()[9:30]
    streams = encoded("route", route_images())[9:30]
    img_stride = 3 * 2049 + 1
    want = singles("chunks", "delta", streams, img_stride)
    assert all(s[0] == 0 for s in want)
    tables = [8 * len(parse_trie(s)[0]) + 60 for s in streams]                          # a leaf's two words, the row, the status word
    budget = sum(tables) // 2 + max(tables)
    assert max(tables) < budget < sum(tables)
    with cniic_amd.Context(0) as ctx:
        monkeypatch.setenv("CNIIC_TEST_MEASURE_BUDGET", str(budget))
        res = batch(ctx, "delta", streams, img_stride)
        hres = batch(ctx, "delta", streams, img_stride, host_src=True, host_out=True)
        monkeypatch.delenv("CNIIC_TEST_MEASURE_BUDGET")
    assert res[5] == hres[5] == len(streams)
    check_against_singles(res, want, img_stride, "two chunks", sources=imgs)
    check_against_singles(hres, want, img_stride, "two chunks, host", sources=imgs)


def test_measure_batch_decodes_its_small_frames_on_the_route():
    import torch
    import cniic_amd
    from cniic_amd import _lib, synth
    dev = torch.device("cuda", 0)
    sizes = [(64, 64), (333, 200), (7, 9), (100, 75), (160, 120), (1, 1), (128, 128)]
    imgs = [(synth.uniform if i % 3 == 1 else synth.photo)(w, h, synth.SEED0 + 8600 + i) for i, (w, h) in enumerate(sizes)]
    streams = encoded("measure", imgs)
    with cniic_amd.Context(0) as ctx:
        rows_want = []
        for im, data in zip(imgs, streams):
            rc2, back = ctx.decode("delta", data)
            assert rc2 == 0 and np.array_equal(back, im)
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ctx.mse(im, back), rc=0))
        offs = np.cumsum([0] + [im.size for im in imgs])[:-1].tolist()
        src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
        stride = ((max(len(s) for s in streams) + 3) & ~3) + 8
        out = torch.zeros(stride * len(imgs), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch("delta", src, offs, [s[0] for s in sizes], [s[1] for s in sizes], out, stride)
        enc_launches, dec_launches = ctx.kernel_time(ENC_TIMER)[1], ctx.kernel_time(TIMER)[1]
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert rc == 0 and enc_launches == dec_launches == 5                            # all but 333 x 200 and 160 x 120, both halves
        host = out.cpu().numpy()
        for f in range(len(imgs)):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f] and got["error"] == 0.0, (f, got, rows_want[f])
            assert rows[f]["lossless_mismatch"] == 0
            assert lens[f] == len(streams[f]) and host[f * stride:f * stride + lens[f]].tobytes() == streams[f], f


@pytest.mark.parametrize("expr", ("hufman", "hilbert(rle)", "cluster-colors(8)"))
def test_other_expressions_never_report_the_stage(expr):
    import cniic_amd
    from cniic_amd import _lib
    imgs = route_images()[9:21]
    with cniic_amd.Context(0) as ref:
        streams = []
        for im in imgs:
            rc, data, _ = ref.encode(expr, im, allow=(_lib.TOO_FEW_POINTS, _lib.FEW_ACTIVE))
            streams.append(data if rc == 0 else b"")
    img_stride = 3 * 1025
    want = singles(expr, expr, streams, img_stride)
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, streams, img_stride)
        assert res[5] == 0
        assert ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0     # not merely zero launches: no such stage
    check_against_singles(res, want, img_stride, expr)


def test_a_size_with_an_injected_scan_is_not_routed():
    import cniic_amd
    imgs = [im for im in route_images() if im.shape[:2] in ((29, 37), (8, 8))]
    w, h = 37, 29
    p = np.random.default_rng(9).permutation(w * h)
    scan = (w, h, np.stack([p % w, p // w], 1).astype(np.uint32))
    streams = encoded("scan", imgs)
    img_stride = 3 * w * h
    want = singles("scan", "delta", streams, img_stride, scan=scan)
    builtin = singles("scan builtin", "delta", streams, img_stride)
    assert any(not np.array_equal(a[3], b[3]) for a, b in zip(want, builtin))
    with cniic_amd.Context(0) as ctx:
        ctx.set_scan(*scan)
        res = batch(ctx, "delta", streams, img_stride)
        assert res[5] == 3                                                              # the 8 x 8 frames
        check_against_singles(res, want, img_stride, "injected scan")
        ctx.set_scan(w, h, None)
        res = batch(ctx, "delta", streams, img_stride)
        assert res[5] == 6
        check_against_singles(res, builtin, img_stride, "scan taken back", sources=imgs)


def test_mutants():
    """a differential check on whatever the edits produce: every status the single decode's, and where that is 0 the pixels too"""
    import cniic_amd
    streams = mutant_streams(*encoded("mutants", list(mutant_sources())))
    want_all = singles("mutants", "delta", streams, MUTANT_STRIDE)
    keep = [k for k, s in enumerate(want_all) if s[0] in (OK, DECODE)]
    held = [(k, want_all[k][0]) for k in range(MUTANTS) if k not in keep]
    print("mutants held back (index, status of the single decode):", held)
    assert len(held) <= MUTANTS // 20
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", [streams[k] for k in keep], MUTANT_STRIDE)
    want = [want_all[k] for k in keep]
    for f, (src, sw, sh, spx, smsg) in enumerate(want):
        assert res[3][f] == src, (keep[f], res[3][f], src)
        if src == 0:
            assert (res[1][f], res[2][f]) == (sw, sh) and np.array_equal(res[4][f * MUTANT_STRIDE:f * MUTANT_STRIDE + sw * sh * 3], spx), keep[f]
    print("mutants on the route:", res[5], "of", len(keep))
    assert res[5] >= 1               # (most edits fall into the serialised decoder, which then does not parse: those are the workers')
