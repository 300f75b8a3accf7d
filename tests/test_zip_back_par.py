"""zip(back)'s decode of a stream by the whole GPU (cniic_amd/csrc/k_zipback_par.hip) on the testing library with the route's floor at
zero and the stage timers on.  Every stream is held three ways: against the CPU restatement of the reference's decoder
(tests/zip_back_ref.py), against the same call with the route off (status, length, bytes, message), and against the marks
"zb_par_decode" / "zb_par_handback" / "zb_par_rounds" / "zb_decode", whose values tests/zb_par_model.py computes from the streams
alone.  The route has no pieces: what can go wrong at an edge are the tiles of its prefix sum (2048 stream positions a block, 1024
tiles a pass of the block that sums them), the wave that shares a symbol of more than 8 bytes, and the two ends of every table."""
import struct

import numpy as np
import pytest

import zb_par_model as M
import zip_back_edges as E
import zip_back_ref as Z

pytestmark = pytest.mark.gpu

MIN, OFF, ROUNDS = "CNIIC_TEST_ZB_PAR_MIN", "CNIIC_TEST_ZB_PAR_OFF", "CNIIC_TEST_ZB_PAR_ROUNDS"
MARKS = ("zb_par_decode", "zb_par_handback", "zb_par_rounds", "zb_decode")
LIT = Z.explicit(b"abcdefgh")


def L():
    from cniic_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_back_ref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    _lib = L()
    with cniic_amd.Context(0) as c:
        c.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        yield c


@pytest.fixture(autouse=True)
def floor_at_zero(monkeypatch):
    monkeypatch.setenv(MIN, "0")


def last_error(ctx):
    return (ctx._L.cniic_last_error(ctx.h) or b"").decode()


def marks(ctx):
    return {m: ctx.kernel_time(m)[1] for m in MARKS}


def dev(data, lead=0, tail=0, fill=0xCD):
    import torch
    buf = np.full(lead + len(data) + tail + 1, fill, np.uint8)
    buf[lead:lead + len(data)] = np.frombuffer(bytes(data), np.uint8)
    return torch.from_numpy(buf).cuda()


def decode(ctx, stream, cap, device=False, lead_in=0, lead_out=0):
    """cniic_zip_back_decode with the caller's buffers as they are -> (rc, *len, the bytes below cap, whether the rest is untouched, message, marks)"""
    import torch
    _lib = L()
    ln = _lib.C.c_uint64(0)
    if device:
        src = dev(stream, lead_in, 16)
        out = torch.full((lead_out + cap + 24,), 0xAB, dtype=torch.uint8, device="cuda")
        rc = ctx._L.cniic_zip_back_decode(ctx.h, src.data_ptr() + lead_in, _lib.C.c_uint64(len(stream)), out.data_ptr() + lead_out, _lib.C.c_uint64(cap), _lib.C.byref(ln))
        host = out.cpu().numpy()
    else:
        src = np.frombuffer(bytes(stream), np.uint8)
        host = np.full(lead_out + cap + 24, 0xAB, np.uint8)
        rc = ctx._L.cniic_zip_back_decode(ctx.h, _lib._ptr(src) if len(stream) else None, _lib.C.c_uint64(len(stream)), host.ctypes.data + lead_out, _lib.C.c_uint64(cap), _lib.C.byref(ln))
    untouched = bool((host[:lead_out] == 0xAB).all() and (host[lead_out + cap:] == 0xAB).all())
    return rc, ln.value, host[lead_out:lead_out + cap].tobytes(), untouched, last_error(ctx) if rc else "", marks(ctx)


def hold(ctx, monkeypatch, stream, cap=None, device=False, round_cap=None, **kw):
    """one stream three ways; -> the model's plan"""
    _lib = L()
    if round_cap is not None:
        monkeypatch.setenv(ROUNDS, str(round_cap))
    full = M.walk(stream)
    cap = full["made"] + 3 if cap is None else cap
    plan = M.plan(stream, cap=cap, round_cap=M.MAX_ROUNDS if round_cap is None else round_cap)
    rc, ln, got, untouched, msg, mk = decode(ctx, stream, cap, device, **kw)
    monkeypatch.setenv(OFF, "1")
    rc0, ln0, got0, untouched0, msg0, mk0 = decode(ctx, stream, cap, device, **kw)
    monkeypatch.delenv(OFF)
    if round_cap is not None:
        monkeypatch.delenv(ROUNDS)
    assert untouched and untouched0
    # the reference
    try:
        want = Z.decode_py(stream)
    except Z.ZipError:
        want = None
    assert (want is None) == (plan["status"] != M.DONE) and (want is None or (want == full["text"] and len(want) == plan["made"]))
    if want is None:
        assert rc == _lib.DECODE and "stream byte %d " % plan["p"] in msg
    else:
        assert rc == (_lib.OK if len(want) <= cap else _lib.CAPACITY) and ln == len(want)
        if rc == _lib.OK or device:      # (a text that does not fit a HOST buffer is not copied down: nothing of it arrives, on either route)
            assert got[:min(ln, cap)] == want[:cap]
    # the route off
    assert (rc, ln, msg) == (rc0, ln0, msg0) and (want is None or got == got0)
    # the marks
    routed = bool(len(stream)) and plan["routed"]
    exp = {"zb_par_decode": int(routed and not plan["handed"]), "zb_par_handback": int(routed and plan["handed"]), "zb_par_rounds": plan["rounds"] if routed else 0}
    assert {m: mk[m] for m in exp} == exp, (mk, exp)
    assert (mk["zb_decode"] > 0) == (bool(len(stream)) and (not routed or plan["handed"])) and mk0["zb_par_decode"] == 0 and (mk0["zb_decode"] > 0) == bool(len(stream))
    return plan


# ---------------------------------------------------------------- hostile streams and the order of the events
HOSTILE = [
    ("back > produced", LIT + Z.lookback(4, 9)),
    ("back == produced", LIT + Z.lookback(4, 8)),
    ("back == 0", LIT + Z.lookback(4, 0) + LIT),
    ("len == 0", LIT + Z.lookback(0, 4) + LIT),
    ("empty explicit", LIT + Z.explicit(b"") + LIT),
    ("len > back", LIT + Z.lookback(7, 3) + Z.lookback(32767, 11)),
    ("truncated literal", LIT + b"\x04\x00abc"),
    ("one trailing byte", LIT + b"\x05"),
    ("header without back", LIT + b"\x04\x80\x03"),
    ("first symbol looks back", Z.lookback(1, 1)),
    ("a literal across stages", Z.explicit(E.rnd(20000, 3)) + Z.lookback(30000, 20000) + Z.explicit(E.rnd(17000, 4)) + Z.lookback(9, 57000)),
    ("back beyond the ring", Z.explicit(E.rnd(30000, 3)) * 3 + Z.lookback(5, 65535) + Z.lookback(100, 50)),
    # the order of the events
    ("a symbol of no bytes before a bad look-back", LIT + Z.lookback(0, 4) + Z.lookback(4, 60000)),
    ("an empty explicit before a bad look-back", LIT + Z.explicit(b"") + Z.lookback(4, 60000)),
    ("a bad look-back before a symbol of no bytes", LIT + Z.lookback(4, 60000) + Z.lookback(0, 4)),
    ("back == o at 65535", Z.explicit(E.rnd(32767, 1)) + Z.explicit(E.rnd(32767, 2)) + Z.explicit(b"x") + Z.lookback(100, 65535) + LIT),
    ("back == o + 1 at 65535", Z.explicit(E.rnd(32767, 1)) + Z.explicit(E.rnd(32767, 2)) + Z.lookback(100, 65535) + LIT),
    ("headers cut 1, 2, 3 bytes in", LIT + Z.lookback(5, 5)[:1]),
    ("a look-back header cut 2 bytes in", LIT + Z.lookback(5, 5)[:2]),
    ("a look-back header cut 3 bytes in", LIT + Z.lookback(5, 5)[:3]),
    ("one byte", b"\x07"),
    ("long symbols inside a literal", Z.explicit((Z.lookback(32767, 65535) + Z.explicit(E.rnd(300, 5)))[:200]) + Z.lookback(50, 100)),
    ("an explicit symbol of 32767 bytes", Z.explicit(E.rnd(32767, 6)) + Z.lookback(32767, 32767) + Z.lookback(32767, 1)),
]


@pytest.mark.parametrize("what,stream", HOSTILE, ids=[h[0] for h in HOSTILE])
@pytest.mark.parametrize("device", [False, True])
def test_hostile_streams_and_the_order_of_events(ctx, monkeypatch, what, stream, device):
    hold(ctx, monkeypatch, stream, device=device)


# the IMAGES of tests/test_zip_back.py on which the reference's encoder does not panic (band 320x240 and flat 100x100 are refused)
IMAGES = {
    "noise 64x48": lambda: Z.noise(64, 48), "photo-like 64x48": lambda: Z.photo_like(64, 48), "band 64x48": lambda: Z.band(64, 48),
    "noise 320x240": lambda: Z.noise(320, 240), "photo-like 320x240": lambda: Z.photo_like(320, 240),
    "1x1": lambda: Z.noise(1, 1), "0x5": lambda: np.zeros((5, 0, 3), np.uint8), "5x0": lambda: np.zeros((0, 5, 3), np.uint8),
    "1x300": lambda: Z.photo_like(1, 300), "300x1": lambda: Z.photo_like(300, 1), "flat 16x16": lambda: Z.flat(16, 16),
}


def last_start_below(s, limit):
    """where the last symbol of a well-formed stream starts at which the text is still shorter than `limit`"""
    p = o = last = 0
    while p + 2 <= len(s) and o < limit:
        last = p
        head = s[p] | (s[p + 1] << 8)
        k = head & 0x7FFF
        if head & 0x8000:
            k = min(k, s[p + 2] | (s[p + 3] << 8))
        p += 4 if head & 0x8000 else 2 + (head & 0x7FFF)
        o += k
    return last


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_images_lazy_and_strict(ctx, clib, monkeypatch, name):
    """through cniic_zip_back_image_decode (need = 8 + 11 w h): garbage and a bad symbol directly behind the symbol that completes the
    text are never seen, a bad symbol one symbol earlier is (in a text above 65 535 bytes no `back` is bad that late: there it stands
    before the last symbol that starts below 65 535 bytes of text); a row too few, a record of length 4 and a cut stream fail as they do on
    the serial kernel, with its message; a failing frame leaves a host destination as it was"""
    import cniic_amd
    _lib = L()
    img = IMAGES[name]()
    h, w = img.shape[:2]
    npx = w * h
    s = Z.codec_encode(lambda d: Z.encode_c(clib, d), img)
    assert s != Z.PANICS
    text = Z.zip_text(img)
    codec = cniic_amd.ZipBack(ctx)
    whole = M.walk(s)
    assert whole["made"] == len(text) == 8 + 11 * npx and whole["p"] == len(s)
    at = last_start_below(s, min(len(text), 65535))
    bad = Z.lookback(4, 65535)
    seen = s[:at] + bad + s[at:]
    assert M.walk(seen, need=len(text))["status"] == M.BAD_LOOKBACK and (len(text) > 65535 or M.walk(s[:at])["made"] < len(text) <= M.walk(s)["made"] and M.walk(s[:at])["symbols"] + 1 == whole["symbols"])
    cases = [(s, True), (s + bad + b"\x09\x00ab", True), (seen, False), (s[:len(s) // 2], False), (s[:5], False)]
    if npx:
        cases.append((Z.encode_c(clib, struct.pack("<II", w, h + 1) + text[8:]), False))        # claims a row more than it carries
        rec = bytearray(text)
        rec[8 + 11 * min(100, npx - 1)] = 4                                                       # a record of length 4
        cases.append((Z.encode_c(clib, bytes(rec)), False))
    for i, (stream, good) in enumerate(cases):
        got = codec.decode(stream)
        mk, msg = marks(ctx), last_error(ctx)
        monkeypatch.setenv(OFF, "1")
        got0 = codec.decode(stream)
        msg0 = last_error(ctx)
        monkeypatch.delenv(OFF)
        assert (got is not None) == good == (got0 is not None) and (not good or (got.shape == img.shape and np.array_equal(got, img))) and (good or msg == msg0), (name, i)
        if _lib.zip_back_dims(stream) is not None:      # (without dimensions the binding makes no call: nothing to mark)
            plan = M.plan(stream, need=len(text), cap=len(text))
            assert plan["routed"] and not plan["handed"]
            assert (mk["zb_par_decode"], mk["zb_par_handback"], mk["zb_par_rounds"], mk["zb_decode"]) == (1, 0, plan["rounds"], 0), (name, i, mk)
    if h > 1 and w:
        fewer = Z.encode_c(clib, struct.pack("<II", w, h - 1) + text[8:])                         # a row fewer: the rest is never pulled
        assert np.array_equal(codec.decode(fewer), img[:h - 1]) and marks(ctx)["zb_par_decode"] == 1
    # a failing frame leaves a host destination as it was
    px = np.full(max(img.size, 1), 0x5A, np.uint8)
    half = np.frombuffer(seen, np.uint8)
    assert ctx.zip_back_image_decode_into(half, half.size, px, allow=(_lib.DECODE,))[0] == _lib.DECODE and (px == 0x5A).all()


# ---------------------------------------------------------------- the ends of the tables and the tiles of the prefix sum
def explicit_stream(nbytes, seed):
    """nbytes of stream made of explicit symbols only (the last one takes what is left; 2 bytes at least)"""
    out = b""
    while len(out) < nbytes:
        k = min(32767, nbytes - len(out) - 2)
        out += Z.explicit(E.rnd(k, seed + len(out)))
    return out


@pytest.mark.parametrize("nbytes", [2, 3, M.SCAN_TILE - 2, M.SCAN_TILE - 1, M.SCAN_TILE, M.SCAN_TILE + 1, 2 * M.SCAN_TILE - 1, 2 * M.SCAN_TILE])
def test_streams_around_a_tile(ctx, monkeypatch, nbytes):
    """position n is a node of the chain: it is the last of a tile, the first of the next, alone in one"""
    body = explicit_stream(nbytes - 8, 7) if nbytes >= 12 else b""
    stream = body + (Z.lookback(3, 2) + Z.lookback(600, 5) if nbytes >= 12 else Z.explicit(b"z" * (nbytes - 2)))
    assert len(stream) == nbytes
    hold(ctx, monkeypatch, stream, device=True)
    hold(ctx, monkeypatch, stream[:-1], device=True)


@pytest.mark.parametrize("tiles", [M.SCAN_BLOCK, M.SCAN_BLOCK + 1])
def test_the_last_tile_count_of_one_pass_and_one_more(ctx, monkeypatch, tiles):
    """1024 tiles fill one pass of the block that sums the tiles; with 1025 it takes a second pass, with a carry"""
    n = M.SCAN_TILE * (tiles - 1) + 5
    stream = explicit_stream(n - 4, 11) + Z.lookback(20000, 40000)
    assert len(stream) == n and (n + 1 + M.SCAN_TILE - 1) // M.SCAN_TILE == tiles
    plan = hold(ctx, monkeypatch, stream, device=True)
    assert plan["rounds"] == 1


@pytest.mark.parametrize("k", [1, 8, 9, 63, 64, 65, 129, 32767])
def test_symbols_a_lane_writes_alone_and_symbols_a_wave_shares(ctx, monkeypatch, k):
    """kZbpSmallK = 8 on either side, a wave's 64 lanes on either side, the longest symbol; literal and copy; next to each other"""
    body = E.rnd(max(k, 40000), 9)
    stream = Z.explicit(body[:k]) + Z.explicit(body[:40000 - k]) + Z.lookback(k, 40000) + Z.lookback(k, k) + Z.explicit(body[:k]) * 3 + Z.lookback(k, min(3 * k, 65535))
    hold(ctx, monkeypatch, stream, device=True)
    hold(ctx, monkeypatch, stream, cap=40000 + k // 2, device=True)        # the capacity ends inside a shared symbol


# ---------------------------------------------------------------- depth
@pytest.mark.parametrize("n_lookbacks", [1, 2, 31, 32, 33, 1000, 70000])
def test_rounds_of_a_chain_of_lookbacks(ctx, monkeypatch, n_lookbacks):
    """explicit(8 bytes) + N x lookback(8, 8): the last bytes are N copies away from a literal; the route runs ceil(log2(N + 1)) rounds
    and no further one (a round that leaves no pointer says so itself)"""
    plan = hold(ctx, monkeypatch, M.chain(n_lookbacks), device=True)
    assert plan["depth"] == n_lookbacks and plan["rounds"] == int(np.ceil(np.log2(n_lookbacks + 1))) and not plan["handed"]


def far_chain():
    return Z.explicit(E.rnd(32767, 1)) + Z.explicit(E.rnd(32767, 2)) + Z.explicit(b"x") + Z.lookback(11, 65535) * 12500


def test_far_lookbacks_across_200_kb(ctx, monkeypatch):
    plan = hold(ctx, monkeypatch, far_chain(), device=True)
    assert plan["made"] == 65535 + 11 * 12500 and plan["depth"] == 3 and plan["rounds"] == 2       # ceil(11 * 12500 / 65535) copies deep


def test_the_round_cap_on_either_side_of_a_streams_own_rounds(ctx, monkeypatch):
    stream = M.chain(1000)
    own = M.plan(stream)["rounds"]
    assert own == 10
    below = hold(ctx, monkeypatch, stream, device=True, round_cap=own - 1)
    at = hold(ctx, monkeypatch, stream, device=True, round_cap=own)
    assert below["handed"] and below["rounds"] == own - 1 and not at["handed"] and at["rounds"] == own
    assert hold(ctx, monkeypatch, stream, round_cap=0)["handed"]


# ---------------------------------------------------------------- capacity
@pytest.mark.parametrize("device", [False, True])
def test_capacity_both_sides(ctx, clib, monkeypatch, device):
    text = E.long_match_mid()
    stream = Z.encode_c(clib, text)
    for cap in (0, 1, 7, len(text) - 1, len(text)):
        plan = hold(ctx, monkeypatch, stream, cap=cap, device=device)
        assert plan["made"] == len(text)


def test_a_long_text_from_a_short_stream_against_a_small_capacity(ctx, monkeypatch):
    """4 KB of stream spell 30 MB; the capacity is 1 MB: CAPACITY with the length, the first 1 MB right, tables of 1 MB"""
    import time
    stream = M.long_text_stream(E.rnd(512, 3))
    assert len(stream) < 4500 and M.walk(stream, cap=0)["made"] == 32768 + 960 * 32767 > 30 << 20
    t0 = time.perf_counter()
    plan = hold(ctx, monkeypatch, stream, cap=1 << 20, device=True)
    assert plan["made"] == 32768 + 960 * 32767 and plan["rounds"] == 6 and time.perf_counter() - t0 < 5.0


# ---------------------------------------------------------------- alignment
def test_every_residue_of_stream_and_text(ctx, monkeypatch):
    stream = LIT + Z.lookback(8, 8) * 5 + Z.explicit(E.rnd(100, 1)) + Z.lookback(90, 100) + Z.lookback(3, 1)
    want = Z.decode_py(stream)
    _lib = L()
    for r in range(16):
        rc, ln, got, untouched, msg, mk = decode(ctx, stream, len(want), device=True, lead_in=r, lead_out=(r * 7 + 3) % 16)
        assert (rc, ln, got) == (_lib.OK, len(want), want) and untouched and mk["zb_par_decode"] == 1, r


# ---------------------------------------------------------------- batches
def batch_streams(clib):
    rng = np.random.default_rng(9)
    imgs = []
    for i in range(24):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 70))
        imgs.append([Z.noise, Z.photo_like][i % 2](w, h))
    imgs[3] = Z.noise(1, 1)
    imgs[7] = np.zeros((0, 9, 3), np.uint8)
    imgs[11] = Z.photo_like(1, 300)
    imgs[19] = Z.photo_like(200, 150)
    streams = [Z.codec_encode(lambda d: Z.encode_c(clib, d), im) for im in imgs]
    assert Z.PANICS not in streams
    return imgs, streams


def run_batch(ctx, streams, img_stride, device):
    import torch
    F = len(streams)
    stride = max(len(s) for s in streams) + 3
    blob = np.zeros(stride * F, np.uint8)
    for f, s in enumerate(streams):
        blob[f * stride:f * stride + len(s)] = np.frombuffer(s, np.uint8)
    px = np.full(img_stride * F, 0x5A, np.uint8)
    src, dst = (torch.from_numpy(blob).cuda(), torch.from_numpy(px).cuda()) if device else (blob, px)
    rc, ws, hs, rcs = ctx.zip_back_decode_batch(src, stride, [len(s) for s in streams], F, dst, img_stride, allow=(L().DECODE,))
    return rc, ws, hs, rcs, (dst.cpu().numpy() if device else dst), last_error(ctx) if rc else "", marks(ctx)


@pytest.mark.parametrize("device", [False, True])
def test_batch_of_good_hostile_and_handed_back_streams(ctx, clib, monkeypatch, device):
    _lib = L()
    imgs, streams = batch_streams(clib)
    streams = list(streams)
    streams[5] = LIT + Z.lookback(4, 9)                          # dimensions, then a look-back behind the start
    streams[9] = streams[9][:len(streams[9]) // 2]                # cut
    streams[13] = b"\x01"                                         # no dimensions: the route never sees it
    img_stride = max(im.size for im in imgs) + 1
    monkeypatch.setenv(ROUNDS, "1")                               # streams with copies of copies are handed back
    plans = [M.plan(s, need=8 + 11 * im.shape[0] * im.shape[1], cap=8 + 11 * im.shape[0] * im.shape[1], round_cap=1) for s, im in zip(streams, imgs)]
    rc, ws, hs, rcs, px, msg, mk = run_batch(ctx, streams, img_stride, device)
    monkeypatch.delenv(ROUNDS)
    monkeypatch.setenv(OFF, "1")
    rc0, ws0, hs0, rcs0, px0, msg0, mk0 = run_batch(ctx, streams, img_stride, device)
    monkeypatch.delenv(OFF)
    assert (rc, ws, hs, rcs, msg) == (rc0, ws0, hs0, rcs0, msg0) and rc == _lib.DECODE and [f for f in range(len(imgs)) if rcs[f]] == [5, 9, 13]
    for f, im in enumerate(imgs):
        if rcs[f] == 0:
            assert px[f * img_stride:f * img_stride + im.size].tobytes() == im.tobytes(), f
    assert np.array_equal(px, px0)
    seen = [f for f in range(len(imgs)) if f != 13]              # (frame 5's claim of dimensions is "abcdefgh": too large an image; it is refused before the decode)
    seen = [f for f in seen if not (f == 5)]
    handed = sum(plans[f]["handed"] for f in seen)
    assert handed >= 3 and mk["zb_par_handback"] == handed and mk["zb_par_decode"] == len(seen) - handed
    assert mk["zb_par_rounds"] == sum(plans[f]["rounds"] for f in seen) and mk["zb_decode"] > 0 and mk0["zb_par_decode"] == 0


def test_300_streams_in_one_call(ctx, monkeypatch):
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 4, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 3), dtype=np.uint8) for _ in range(300)]
    streams = [Z.codec_encode(Z.encode_py, im) for im in imgs]
    rc, ws, hs, rcs, px, msg, mk = run_batch(ctx, streams, 8 * 8 * 3, False)
    assert rc == 0 and rcs == [0] * 300 and ws == [im.shape[1] for im in imgs] and hs == [im.shape[0] for im in imgs]
    assert all(px[f * 192:f * 192 + imgs[f].size].tobytes() == imgs[f].tobytes() for f in range(300))
    plans = [M.plan(s, need=8 + 11 * im.shape[0] * im.shape[1], cap=8 + 11 * im.shape[0] * im.shape[1]) for s, im in zip(streams, imgs)]
    assert mk["zb_par_decode"] == 300 and mk["zb_par_handback"] == 0 and mk["zb_decode"] == 0 and mk["zb_par_rounds"] == sum(p["rounds"] for p in plans)


def test_no_frames_and_alternating_calls(ctx, clib, monkeypatch):
    _lib = L()
    assert ctx.zip_back_decode_batch(np.zeros(1, np.uint8), 1, [], 0, np.zeros(1, np.uint8), 1)[0] == _lib.OK
    stream = Z.encode_c(clib, E.long_match_mid())
    want = E.long_match_mid()
    for i in range(6):
        if i % 2:
            monkeypatch.setenv(OFF, "1")
        rc, got = ctx.zip_back_decode(stream, cap=len(want))
        mk = marks(ctx)
        if i % 2:
            monkeypatch.delenv(OFF)
        assert rc == _lib.OK and got == want and (mk["zb_par_decode"], mk["zb_decode"] > 0) == ((0, True) if i % 2 else (1, False))


# ---------------------------------------------------------------- the floor
FLOOR = 512 << 10          # kZbParFloorBytes; kZbParMaxStreams = 1 (NOTES AW)


def test_the_release_floor(ctx, monkeypatch):
    """with the knob unset: a call of ONE stream of 512 KiB or more takes the route, a byte fewer does not, and calls of two such
    streams do not; CNIIC_TEST_ZB_SLICE alone takes the route off, whatever the floor"""
    monkeypatch.delenv(MIN)
    at = explicit_stream(FLOOR - 4, 5) + Z.lookback(20000, 40000)
    below = explicit_stream(FLOOR - 5, 5) + Z.lookback(20000, 40000)
    assert len(at) == FLOOR and len(below) == FLOOR - 1
    for stream, routed in ((at, 1), (below, 0), (LIT + Z.lookback(8, 8), 0)):
        rc, got = ctx.zip_back_decode(stream, cap=1 << 20)
        mk = marks(ctx)
        assert rc == 0 and got == Z.decode_py(stream)
        assert (mk["zb_par_decode"], mk["zb_par_rounds"], mk["zb_decode"] > 0) == (routed, routed, not routed), (len(stream), mk)
    # an image whose stream is above the floor: alone it takes the route, two of them in one call do not
    img = Z.noise(220, 220)
    text = Z.zip_text(img)
    stream = b"".join(Z.explicit(text[i:i + 32767]) for i in range(0, len(text), 32767))
    assert len(stream) >= FLOOR
    rc, ws, hs, rcs, px, msg, mk = run_batch(ctx, [stream], img.size, True)
    assert rc == 0 and px[:img.size].tobytes() == img.tobytes() and (mk["zb_par_decode"], mk["zb_decode"]) == (1, 0)
    rc, ws, hs, rcs, px, msg, mk = run_batch(ctx, [stream, stream], img.size, True)
    assert rc == 0 and px.tobytes() == img.tobytes() * 2 and mk["zb_par_decode"] == 0 and mk["zb_decode"] > 0
    monkeypatch.setenv("CNIIC_TEST_ZB_SLICE", "70000")
    rc, got = ctx.zip_back_decode(at, cap=1 << 20)
    assert rc == 0 and got == Z.decode_py(at) and marks(ctx)["zb_par_decode"] == 0 and marks(ctx)["zb_decode"] > 1
