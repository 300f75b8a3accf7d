"""Small `zip(dict)` frames of cniic_codec_decode_batch / cniic_codec_measure_batch on the small-frame decode route (k_zd_small_dec.hip: a
workgroup per frame from its pairs to its pixels; include/cniic_hip.h above cniic_codec_decode_batch).  Every comparison is exact: a
frame's status, dimensions, pixels and message are those of cniic_codec_decode for that stream alone on a context that has seen no batch,
and for good streams the pixels are those of tests/zip_dict_ref.py and the source image.  Which frames took the route is read from the
stage timer "zd_small_dec_batch", whose launch count is the number of frames the kernel was given; "zd_small_dec_handback" counts those of
them the kernel handed back to the workers.  On a build without the route neither mark exists.

What a case claims about a stream -- whether it is a candidate, its verdict and the numbers of its message, the pairs its text needs, its
generation and the pairs a byte visits, and so which side of a cap it lies on -- is computed from the symbols alone (analyse);
tests/test_zd_small_dec_cpu.py asserts the same claims without a GPU, against tests/zip_dict_ref.py and against
tests/zd_small_dec_check.cpp."""
import struct
import tempfile

import numpy as np
import pytest

import zip_dict_ref as Z

pytestmark = pytest.mark.gpu

MAX_PX = 16384                 # kZdSmallDecMaxPx (cniic_amd/csrc/zd_small_dec.hpp)
MAX_PAIRS = 24576              # kZsdMaxPairs
HOPS, ROUNDS = 64, 64          # kZsdHops, kZsdRounds
HEAD = 64                      # kZdDecHead (codec.cpp): the bytes of a stream the host reads
FLOOR_FEW, FLOOR_MANY = 8, 32                 # kZdSmallDecFloorFew, kZdSmallDecFloorMany (codec.cpp): candidates of a call from which ...
FLOOR_PX_FEW, FLOOR_PX_MANY = 4096, 16384     # kZdSmallDecFloorPxFew, kZdSmallDecFloorPxMany: ... those of at most so many pixels take the route
TIMER, HANDBACK, ENC_TIMER = "zd_small_dec_batch", "zd_small_dec_handback", "zd_small_batch"
KNOB_OFF, KNOB_MAX_PX, KNOB_FLOOR_OFF = "CNIIC_TEST_ZD_SMALL_DEC_OFF", "CNIIC_TEST_ZD_SMALL_DEC_MAX_PX", "CNIIC_TEST_ZD_SMALL_DEC_FLOOR_OFF"
KNOB_PAIRS, KNOB_HOPS, KNOB_ROUNDS = "CNIIC_TEST_ZD_SMALL_DEC_MAX_PAIRS", "CNIIC_TEST_ZD_SMALL_DEC_HOPS", "CNIIC_TEST_ZD_SMALL_DEC_ROUNDS"
KNOB_BUDGET, KNOB_BATCH_OFF = "CNIIC_TEST_MEASURE_BUDGET", "CNIIC_TEST_DECODE_BATCH_OFF"
EXPR = "zip(dict)"
OK, DECODE, CAPACITY = 0, -6, -8
POISON = 0xA5
SIZES = [(1, 1), (2, 1), (3, 1), (5, 1), (7, 3), (8, 8), (13, 5), (32, 32), (64, 64), (128, 96), (128, 128), (16384, 1), (1, 16384)]   # (w, h)
UNROUTED = [(16385, 1), (160, 120)]
EOF, FIRST = Z.EOF, Z.FIRST_NEW
MESSAGES = {"symbol": "zip-dict: pair %d uses a symbol that has not been handed out", "dangling": "zip-dict: a first symbol without a second at the end of the stream",
            "short": "zip-dict: the text ends after %d of %d bytes", "record": "zip-dict: pixel %d is not a record of 3 bytes (ser.rs:216-221)"}


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor; test_the_floor holds it"""
    monkeypatch.setenv(KNOB_FLOOR_OFF, "1")


# ------------------------------------------------------------------ contents and streams
def two_colour(w, h):
    """columns alternate (255, 0, 7) and black"""
    img = np.zeros((h, w, 3), np.uint8)
    img[:, ::2] = (255, 0, 7)
    return img


CONTENTS = (("photo", Z.photo_like), ("noise", Z.noise), ("flat", Z.flat), ("two-colour", two_colour))
_CLIB, _STREAMS = [], {}


def clib():
    if not _CLIB:
        _CLIB.append(Z.compile_c(tempfile.mkdtemp(prefix="zd_small_dec_ref")))
    assert _CLIB[0] is not None, "no C compiler"
    return _CLIB[0]


def encoded(img, key=None):
    """the zip(dict) stream of img as tests/zip_dict_ref.py writes it (its C restatement); cached under key"""
    if key is None or key not in _STREAMS:
        data = Z.codec_encode(lambda t: Z.encode_c(clib(), t), img)
        if key is None:
            return data
        _STREAMS[key] = data
    return _STREAMS[key]


def library():
    """[(name, image, stream)]: every size under every content, then the two frames that ride along unrouted"""
    out = [("%s %dx%d" % (nm, w, h), gen(w, h)) for w, h in SIZES for nm, gen in CONTENTS]
    out += [("photo %dx%d unrouted" % (w, h), Z.photo_like(w, h)) for w, h in UNROUTED]
    return [(nm, im, encoded(im, nm)) for nm, im in out]


def pairs_of(stream):
    n = len(stream) // 4
    s = struct.unpack("<%dH" % (2 * n), stream[:4 * n])
    return list(zip(s[0::2], s[1::2]))


def from_pairs(pairs):
    return b"".join(struct.pack("<HH", a, b) for a, b in pairs)


def analyse(stream, max_pairs=MAX_PAIRS, hops=HOPS, rounds=ROUNDS, max_px=MAX_PX):
    """What the route makes of a stream, from its symbols alone -> dict.  cand: the head (16 pairs) spells the dimensions and the frame has
    1 .. max_px pixels.  For a candidate: w, h, need, P (the pairs looked at), kb (the first of them with a symbol not handed out, or P),
    gen (the deepest generation below kb: a pair of literals or empty texts has 0, any other one more than the deeper of its parts),
    verdict (ok / back / symbol / dangling / short / record), its numbers a and b, message; for a text that is complete: needed (the pairs
    the lazy reader reads) and visits (the most pairs a byte of the records visits on its way to its literal); for ok: pixels."""
    stream = bytes(stream)
    n = len(stream)
    try:
        head = Z.decode_py(stream[:4 * min(n // 4, HEAD // 4)], 8)
    except Z.ZipError:
        return dict(cand=False)
    if len(head) < 8:
        return dict(cand=False)
    w, h = struct.unpack_from("<II", head)
    if not 1 <= w * h <= max_px:
        return dict(cand=False, w=w, h=h)
    need, P = 8 + 11 * w * h, min(n // 4, max_pairs)
    C = need + 1
    pairs = pairs_of(stream)[:P]
    length, gen, kb = [], [], P
    for k, (s1, s2) in enumerate(pairs):
        if any(s != EOF and s >= FIRST + k for s in (s1, s2)):
            kb = k
            break
        length.append(min(sum(1 if s < FIRST else 0 if s == EOF else length[s - FIRST] for s in (s1, s2)), C))
        gen.append(1 + max(-1 if s < FIRST or s == EOF else gen[s - FIRST] for s in (s1, s2)))
    res = dict(cand=True, w=w, h=h, need=need, P=P, kb=kb, gen=max(gen, default=-1), a=0, b=0, message="")

    def verdict(v, a=0, b=0):
        res.update(verdict=v, a=a, b=b)
        if v in MESSAGES:
            res["message"] = MESSAGES[v] % ((a, b) if v == "short" else (a,) if v in ("symbol", "record") else ())
        return res

    if res["gen"] >= rounds:
        return verdict("back")
    total, needed = 0, None
    for k in range(kb):
        total = min(total + length[k], C)
        if total >= need:
            needed = k + 1
            break
    if needed is None:
        if kb < P:
            return verdict("symbol", kb)
        if P < n // 4:
            return verdict("back")
        if n & 3 >= 2:
            return verdict("dangling")
        return verdict("short", total, need)
    # the text of the needed pairs, and per byte the pairs visited from the pair that wrote it
    text, vis = [], []
    lit_v = np.ones(1, np.uint32)
    for s1, s2 in pairs[:needed]:
        t, v = [], []
        for s in (s1, s2):
            if s == EOF:
                continue
            if s < FIRST:
                t.append(np.array([s], np.uint8))
                v.append(lit_v)
            else:
                t.append(text[s - FIRST])
                v.append(vis[s - FIRST] + 1)
        text.append(np.concatenate(t)[:C] if t else np.zeros(0, np.uint8))
        vis.append(np.concatenate(v)[:C] if v else np.zeros(0, np.uint32))
    whole, visits = np.concatenate(text)[:need], np.concatenate(vis)[:need]
    res.update(needed=needed, visits=int(visits[8:].max()))
    if res["visits"] > hops:
        return verdict("back")
    rec = whole[8:].reshape(-1, 11)
    bad = np.flatnonzero((rec[:, 0] != 3) | rec[:, 1:8].any(axis=1))
    if bad.size:
        return verdict("record", int(bad[0]))
    res["pixels"] = rec[:, 8:11].reshape(-1).copy()
    return verdict("ok")


def takes(stream, img_stride, F=1, stride=1 << 40, **caps):
    """whether the route is given the stream: a candidate whose image fits, and which ends before the next one starts"""
    a = analyse(stream, **caps)
    return a["cand"] and 3 * a["w"] * a["h"] <= img_stride and (F == 1 or stride >= len(stream))


def back(stream, **caps):
    return analyse(stream, **caps).get("verdict") == "back"


def chain(D):
    """a black frame of n x 1 whose text has period 11: four literal pairs for the dimensions, seven pairs that spell three records and
    make symbol 0x10A = one record, then (the previous symbol, 0x10A) D times -- entries of 2 .. D + 1 records, chained.  -> (n, stream)"""
    n = 3 + sum(range(2, D + 2))
    dims = struct.pack("<II", n, 1)
    pairs = [(dims[0], dims[1]), (dims[2], dims[3]), (dims[4], dims[5]), (dims[6], dims[7]),
             (3, 0), (0, 0), (0x105, 0x105), (0, 0x105), (0x104, 0x106), (0x107, 0x105), (0x108, 0x109)]
    pairs += [(0x10A + j, 0x10A) for j in range(D)]
    return n, from_pairs(pairs)


def with_empty_texts(stream):
    """the same text from more pairs: (0xFFFF, 0xFFFF) behind the head, and the last pair whose symbol nobody uses, (a, b), as
    (a, 0xFFFF) (0xFFFF, b); every later symbol renumbered, since each pair hands one out"""
    pairs = pairs_of(stream)
    used = {s for p in pairs for s in p if FIRST <= s < EOF}
    split = max(k for k in range(5, len(pairs)) if FIRST + k not in used and pairs[k][1] != EOF)

    def moved(s, k_new):   # symbol s as it is numbered in the new stream
        if s < FIRST or s == EOF:
            return s
        k = s - FIRST
        return FIRST + k + (1 if k >= 4 else 0) + (1 if k > split else 0)

    out = []
    for k, (a, b) in enumerate(pairs):
        if k == 4:
            out.append((EOF, EOF))
        if k == split:
            out += [(moved(a, 0), EOF), (EOF, moved(b, 0))]
        else:
            out.append((moved(a, 0), moved(b, 0)))
    return from_pairs(out)


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
                rc, w, h = ref.decode_into(EXPR, raw, len(s), out[:cap], allow=(DECODE, CAPACITY))
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
    """one cniic_codec_decode_batch call with the stage timers on -> (rc, ws, hs, rcs, output as a host array, frames given to the kernel,
    message, frames handed back).  The stream of frame f lies at src_off + f * stride modulo 16, its image at out_off + f * img_stride
    modulo 16, inside poisoned allocations."""
    import torch
    from cniic_amd import _lib
    F = len(streams)
    lens = [len(s) for s in streams]
    stride = stride or ((max(lens) + 15) & ~15)
    room = stride * (F - 1) + max(max(lens), 1)
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
        rc, ws, hs, rcs = ctx.decode_batch(EXPR, src[sat:], stride, lens, F, whole[at:], img_stride, allow=(DECODE, CAPACITY))
        msg = _last_error(ctx) if rc != 0 else ""
        launches, handed = ctx.kernel_time(TIMER)[1], ctx.kernel_time(HANDBACK)[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = whole if host_out else whole.cpu().numpy()
    assert bool((host[:at] == POISON).all()) and bool((host[at + img_stride * F:] == POISON).all())    # nothing before the first image or behind the last
    return rc, ws, hs, rcs, host[at:at + img_stride * F], launches, msg, handed


def check_against_singles(res, want, img_stride, what, on_route=()):
    """on_route: the frames the kernel settled.  One of them that fails leaves its destination alone; the single decode, which the
    workers run for every other frame, may have written pixels before it met a bad record."""
    rc, ws, hs, rcs, host = res[:5]
    for f, (src, sw, sh, spx, smsg) in enumerate(want):
        assert rcs[f] == src, (what, f, rcs[f], src)
        slot = host[f * img_stride:(f + 1) * img_stride]
        if src == 0:
            assert (ws[f], hs[f]) == (sw, sh), (what, f)
            assert np.array_equal(slot[:sw * sh * 3], spx), (what, f)
            assert bool((slot[sw * sh * 3:] == POISON).all()), (what, f)          # nothing behind an image's end
        elif f in on_route:
            assert bool((slot == POISON).all()), (what, f)                          # a frame that fails on the route leaves its destination alone
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first]), what
    if first is not None:
        assert res[6] == want[first][4], (what, res[6], want[first][4])


def check_against_claims(streams, want, what, **caps):
    """the single decode against what analyse says of the stream (a stream handed back has no claim of its own: its uncapped one)"""
    for f, s in enumerate(streams):
        a = analyse(s)
        if not a["cand"] or a["verdict"] == "back":
            continue
        rc, w, h, px, msg = want[f]
        if a["verdict"] == "ok":
            assert rc == 0 and (w, h) == (a["w"], a["h"]) and np.array_equal(px, a["pixels"]), (what, f)
        else:
            assert rc == DECODE and msg == a["message"], (what, f, msg, a["message"])


def run(ctx, streams, want, img_stride, what, **kw):
    """a batch call; the frames given to the kernel and handed back are those the streams say, the results the single decode's"""
    caps = kw.pop("caps", {})
    F, stride = len(streams), kw.get("stride") or ((max(len(s) for s in streams) + 15) & ~15)
    given = [f for f, s in enumerate(streams) if takes(s, img_stride, F, stride, **caps)]
    res = batch(ctx, streams, img_stride, **kw)
    assert res[5] == len(given), (what, res[5], len(given))
    handed = [f for f in given if back(streams[f], **{k: v for k, v in caps.items() if k != "max_px"})]
    assert res[7] == len(handed), (what, res[7], len(handed))
    check_against_singles(res, want, img_stride, what, on_route=set(given) - set(handed))
    return res


# ------------------------------------------------------------------ the tests
def test_library_streams_alone_together_and_with_the_route_off(monkeypatch):
    import cniic_amd
    names, imgs, streams = zip(*library())
    img_stride = 3 * 19200
    assert [im.shape[0] * im.shape[1] for im in imgs[-2:]] == [16385, 19200]
    want = singles("library", streams, img_stride)
    for f, im in enumerate(imgs):
        back_py = Z.codec_decode(lambda s, need: Z.decode_c(clib(), s, need, cap=need + (1 << 18)), streams[f])
        assert want[f][0] == 0 and np.array_equal(want[f][3], im.reshape(-1)) and np.array_equal(back_py, im), names[f]
    check_against_claims(streams, want, "library")
    assert sum(takes(s, img_stride) for s in streams) == len(streams) - 2 and not any(back(s) for s in streams)
    assert len(pairs_of(streams[names.index("noise 128x128")])) == 23310
    with cniic_amd.Context(0) as ctx:
        for f, s in enumerate(streams):
            run(ctx, [s], want[f:f + 1], img_stride, names[f])
        on = run(ctx, streams, want, img_stride, "together")
        assert on[5] == len(streams) - 2 and on[7] == 0
        monkeypatch.setenv(KNOB_OFF, "1")
        off = batch(ctx, streams, img_stride)
        for name in (TIMER, HANDBACK):
            assert ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, None) != 0    # no launches: the stage is not there
        monkeypatch.delenv(KNOB_OFF)
        monkeypatch.setenv(KNOB_MAX_PX, "4096")
        low = run(ctx, streams, want, img_stride, "4096 pixels", caps=dict(max_px=4096))
        assert low[5] == sum(im.shape[0] * im.shape[1] <= 4096 for im in imgs) == 4 * 9
        monkeypatch.delenv(KNOB_MAX_PX)
    check_against_singles(off, want, img_stride, "route off")
    assert off[5] == 0 and on[:4] == off[:4] == low[:4] and np.array_equal(on[4], off[4]) and np.array_equal(on[4], low[4])


def lazy_streams():
    """[(name, stream)] around the last pair the text of a 13 x 5 photo needs"""
    base = encoded(Z.photo_like(13, 5), "photo 13x5")
    a = analyse(base)
    needed = a["needed"]
    good = base[:4 * needed]
    never = struct.pack("<HH", 0xFFFE, 0x100 + needed + 5)     # two symbols nobody has handed out
    lone = struct.pack("<H", 0x41)                               # a first symbol without a second
    garbage = {4: never, 5: never + b"\x07", 6: never + lone, 7: never + lone + b"\x07"}
    out = [("the last needed pair, then nothing", good)]
    out += [("%d bytes of garbage behind" % k, good + g) for k, g in garbage.items()]
    out += [("%d bytes of garbage in front of the last needed pair" % k, good[:-4] + g + good[-4:]) for k, g in garbage.items()]
    return needed, out


def test_the_lazy_reader():
    import cniic_amd
    needed, cases = lazy_streams()
    names, streams = zip(*cases)
    img_stride = 3 * 13 * 5 + 5
    want = singles("lazy", streams, img_stride)
    assert all(w[0] == 0 for w in want[:5]), [w[4] for w in want[:5]]
    for w in want[5:]:
        assert w[0] == DECODE and w[4] == MESSAGES["symbol"] % (needed - 1), w[4]
    check_against_claims(streams, want, "lazy")
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "lazy")
        assert res[5] == len(streams) and res[7] == 0
        for f, s in enumerate(streams):
            run(ctx, [s], want[f:f + 1], img_stride, names[f])


def verdict_streams():
    base = encoded(Z.photo_like(13, 5), "photo 13x5")
    needed = analyse(base)["needed"]
    good = base[:4 * needed]
    out = [("cut by %d" % k, good[:-k]) for k in (1, 2, 3, 4)]
    for nm, k in (("first", 0), ("a middle", needed // 2), ("the last needed", needed - 1)):
        for half in (0, 2):
            s = bytearray(good)
            s[4 * k + half:4 * k + half + 2] = struct.pack("<H", FIRST + k)      # the symbol this very pair hands out
            out.append(("a bad symbol in %s pair, half %d" % (nm, half // 2), bytes(s)))
    out.append(("a bad symbol one pair behind the last needed", good + struct.pack("<HH", FIRST + needed, 7)))
    return needed, out


def test_every_verdict():
    import cniic_amd
    needed, cases = verdict_streams()
    names, streams = zip(*cases)
    img_stride = 3 * 13 * 5
    want = singles("verdicts", streams, img_stride)
    by = dict(zip(names, want))
    claims = dict(zip(names, (analyse(s) for s in streams)))
    assert [claims["cut by %d" % k]["verdict"] for k in (1, 2, 3, 4)] == ["dangling", "dangling", "short", "short"]
    assert claims["cut by 3"]["a"] == claims["cut by 4"]["a"] < claims["cut by 4"]["b"] == 8 + 11 * 65
    assert by["cut by 1"][4] == by["cut by 2"][4] == MESSAGES["dangling"] and by["cut by 4"][4] == MESSAGES["short"] % (claims["cut by 4"]["a"], 8 + 11 * 65)
    assert not claims["a bad symbol in first pair, half 0"]["cand"] and not claims["a bad symbol in first pair, half 1"]["cand"]     # no dimensions: the workers'
    for nm, k in (("a middle", needed // 2), ("the last needed", needed - 1)):
        for half in (0, 1):
            assert by["a bad symbol in %s pair, half %d" % (nm, half)][4] == MESSAGES["symbol"] % k
    assert by["a bad symbol one pair behind the last needed"][0] == 0
    check_against_claims(streams, want, "verdicts")
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "verdicts")
        assert res[5] == len(streams) - 2 and res[7] == 0
        for f, s in enumerate(streams):
            run(ctx, [s], want[f:f + 1], img_stride, names[f])


def test_empty_texts():
    import cniic_amd
    imgs = [Z.photo_like(13, 5), Z.noise(32, 32), Z.flat(8, 8), two_colour(7, 3)]
    plain = [encoded(im) for im in imgs]
    streams = [with_empty_texts(s) for s in plain]
    for s, p, im in zip(streams, plain, imgs):
        assert len(s) == len(p) + 8 and Z.decode_py(s) == Z.decode_py(p) and np.array_equal(analyse(s)["pixels"], im.reshape(-1))
        assert sum(a == EOF and b == EOF for a, b in pairs_of(s)) == 1 and sum((a == EOF) != (b == EOF) for a, b in pairs_of(s)) >= 2
    img_stride = 3 * 32 * 32 + 1
    want = singles("empty", streams, img_stride)
    assert all(w[0] == 0 and np.array_equal(w[3], im.reshape(-1)) for w, im in zip(want, imgs))
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "empty texts")
        assert res[5] == len(streams) and res[7] == 0


def saturation_streams():
    dims = struct.pack("<II", 5, 1)
    head = [(dims[0], dims[1]), (dims[2], dims[3]), (dims[4], dims[5]), (dims[6], dims[7])]
    doubling = head + [(3, 0)] + [(FIRST + 4 + j, FIRST + 4 + j) for j in range(70)]          # 2^71 bytes claimed, and generation 70: handed back
    forty = head + [(3, 0)] + [(FIRST + 4 + j, FIRST + 4 + j) for j in range(40)]             # 2^41 bytes, generation 40: the route's own
    need = 8 + 11 * 5
    grow = head + [(3, 0)] + [(FIRST + 4 + j, FIRST + 4 + j) for j in range(6)]                # the last entry: 2^7 = 128 >= need
    big = FIRST + len(grow) - 1
    many = grow + [(big, big)] * 200
    assert 2 ** 7 >= need
    return [("2^71 bytes", from_pairs(doubling)), ("2^41 bytes", from_pairs(forty)), ("200 pairs of at least need", from_pairs(many))]


def test_saturation():
    import cniic_amd
    names, streams = zip(*saturation_streams())
    img_stride = 15
    want = singles("saturation", streams, img_stride)
    check_against_claims(streams, want, "saturation")
    assert all(analyse(s)["cand"] for s in streams) and [analyse(s)["verdict"] for s in streams] == ["back", "record", "record"]
    assert [analyse(s)["gen"] for s in streams] == [70, 40, 7] and all(w[0] == DECODE and w[4] == MESSAGES["record"] % 0 for w in want)
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "saturation")
        assert res[5] == 3 and res[7] == 1


def record_streams():
    """streams of texts with a record that is not (3, 0 x 7, r, g, b), coded by tests/zip_dict_ref.py"""
    img = Z.photo_like(13, 5)
    text = bytearray(Z.zip_text(img))
    n = 65
    out = []

    def coded(name, edits):
        t = bytearray(text)
        for px, off, v in edits:
            t[8 + 11 * px + off] = v
        out.append((name, Z.encode_py(bytes(t)), min(px for px, _, _ in edits)))

    for px in (0, n // 2, n - 1):
        coded("a length byte of 4 at pixel %d" % px, [(px, 0, 4)])
    for off in range(1, 8):
        coded("byte %d of a record is 1" % off, [(20 + off, off, 1)])
    coded("two bad pixels", [(40, 3, 9), (17, 0, 0)])
    return out


def test_records():
    import cniic_amd
    names, streams, first_bad = zip(*record_streams())
    img_stride = 3 * 65
    want = singles("records", streams, img_stride)
    for w, px in zip(want, first_bad):
        assert w[0] == DECODE and w[4] == MESSAGES["record"] % px, w[4]
    assert first_bad[-1] == 17
    check_against_claims(streams, want, "records")
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams + (encoded(Z.photo_like(13, 5)),), want + singles("records good", [encoded(Z.photo_like(13, 5))], img_stride), img_stride, "records")
        assert res[5] == len(streams) + 1 and res[7] == 0


DEPTHS = (60, 61, 62, 63, 64, 65)     # generations 63 .. 68: on either side of the caps of 64, and the three that lie behind them


def test_depth(monkeypatch):
    import cniic_amd
    frames = [chain(D) for D in DEPTHS]
    streams = [s for _, s in frames]
    assert [n for n, _ in frames][3:] == [2082, 2147, 2213] and [len(s) // 4 for s in streams][3:] == [74, 75, 76]
    claims = [analyse(s, hops=1 << 20, rounds=1 << 20) for s in streams]
    assert [a["gen"] for a in claims] == [D + 3 for D in DEPTHS] and [a["gen"] for a in claims][3:] == [66, 67, 68]
    assert [a["visits"] for a in claims] == [D + 4 for D in DEPTHS]           # a byte of the deepest pair visits every generation
    for (n, s), a in zip(frames, claims):
        assert a["verdict"] == "ok" and not a["pixels"].any() and a["needed"] == len(s) // 4
        img = Z.codec_decode(Z.decode_py, s)
        assert img.shape == (1, n, 3) and not img.any()
    # at the caps as they are: generation 63 needs 64 rounds and a byte of it visits 64 pairs
    assert [back(s) for s in streams] == [False, True, True, True, True, True]
    img_stride = 3 * 2213 + 3
    want = singles("depth", streams, img_stride)
    assert all(w[0] == 0 and not w[3].any() for w in want)
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "depth")
        assert res[5] == 6 and res[7] == 5
        shallow = [chain(D)[1] for D in (3, 10, 11, 12, 30)]
        want_sh = singles("depth shallow", shallow, img_stride)
        for knob, name in ((KNOB_HOPS, "hops"), (KNOB_ROUNDS, "rounds")):
            for cap in (6, 14, 15, 16, 17, 33, 34, 35):
                monkeypatch.setenv(knob, str(cap))
                caps = {name: cap}
                handed = [back(s, **caps) for s in shallow]
                res = run(ctx, shallow, want_sh, img_stride, "%s %d" % (name, cap), caps=caps)
                assert res[5] == len(shallow) and res[7] == sum(handed)
                if name == "rounds":
                    assert handed == [D + 3 >= cap for D in (3, 10, 11, 12, 30)]     # generation D + 3 needs D + 4 rounds
                else:
                    assert handed == [D + 4 > cap for D in (3, 10, 11, 12, 30)]      # and its deepest byte visits D + 4 pairs
            monkeypatch.delenv(knob)


def test_the_pair_cap(monkeypatch):
    import cniic_amd
    photo = encoded(Z.photo_like(64, 64), "photo 64x64")
    noise = encoded(Z.noise(128, 128), "noise 128x128")
    company = [encoded(Z.photo_like(13, 5), "photo 13x5"), encoded(Z.flat(32, 32), "flat 32x32")]
    needed = analyse(photo)["needed"]
    assert 5000 < needed <= len(photo) // 4 and analyse(noise)["needed"] > 23000 and len(noise) // 4 == 23310
    img_stride = 3 * MAX_PX
    want = singles("pair cap", [photo, noise] + company, img_stride)
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, [photo, noise] + company, want, img_stride, "the cap as it is")
        assert res[5] == 4 and res[7] == 0
        for cap, handed in ((needed - 1, 1), (needed, 0), (needed + 1, 0)):
            monkeypatch.setenv(KNOB_PAIRS, str(cap))
            assert back(photo, max_pairs=cap) == bool(handed)
            res = run(ctx, [photo], want[:1], img_stride, "alone under %d pairs" % cap, caps=dict(max_pairs=cap))
            assert res[5] == 1 and res[7] == handed
            res = run(ctx, company[:1] + [photo] + company[1:], [want[2], want[0], want[3]], img_stride, "in company under %d pairs" % cap, caps=dict(max_pairs=cap))
            assert res[5] == 3 and res[7] == handed
        monkeypatch.delenv(KNOB_PAIRS)


def placement_streams():
    imgs = [Z.photo_like(13, 5), Z.noise(7, 3), Z.flat(8, 8), two_colour(5, 1), Z.photo_like(1, 1), Z.noise(16, 15), Z.photo_like(3, 1), Z.noise(2, 1)]
    streams = [encoded(im) for im in imgs]
    bad = bytearray(streams[0])
    bad[40:42] = struct.pack("<H", 0xFFF0)
    return streams[:3] + [bytes(bad)] + streams[3:]


@pytest.mark.parametrize("host_src,host_out", ((False, False), (True, False), (False, True), (True, True)))
def test_every_residue_and_both_memories(host_src, host_out):
    import cniic_amd
    streams = placement_streams()
    longest = max(len(s) for s in streams)
    with cniic_amd.Context(0) as ctx:
        for off in range(16):
            img_stride = 3 * 16 * 15 + 16 + (off * 7) % 16                 # the images' phases differ from frame to frame
            want = singles(("residues", img_stride), streams, img_stride)
            assert [w[0] for w in want] == [0, 0, 0, DECODE] + [0] * 5
            stride = (longest + off) | 1                                     # odd: the streams lie at all four residues
            res = run(ctx, streams, want, img_stride, "residue %d" % off, stride=stride, host_src=host_src, host_out=host_out, src_off=(5 * off) % 16, out_off=off)
            assert res[5] == len(streams) and res[7] == 0


def test_an_image_one_byte_too_large_for_its_slot():
    import cniic_amd
    streams = placement_streams()[:3]
    img_stride = 3 * 8 * 8 - 1                                              # the third frame's image, less a byte; 13 x 5 does not fit either
    want = singles("short slot", streams, img_stride)
    assert [w[0] for w in want] == [CAPACITY, 0, CAPACITY]
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "short slot")
        assert res[5] == 1


def volume_streams():
    sizes = [(8, 8), (9, 7), (16, 5), (24, 24), (13, 17), (31, 3), (4, 4), (20, 11)]
    rng = np.random.default_rng(91)
    kinds = []
    for w, h in sizes:
        for c in range(3):
            img = Z.photo_like(w, h) if c == 0 else Z.flat(w, h) if c == 1 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            kinds.append((img, encoded(img)))
    return sizes, [kinds[3 * (f % 8) + (f // 8) % 3] for f in range(3000)]


def test_many_frames_chunks_and_calls_in_turn(monkeypatch):
    import cniic_amd
    sizes, frames = volume_streams()
    streams = [s for _, s in frames]
    img_stride = 3 * 24 * 24 + 1
    picks = list(range(24))
    want24 = singles("volume", streams[:24], img_stride)
    assert all(w[0] == 0 for w in want24)

    def check_all(res, what, given):
        assert res[0] == 0 and res[3] == [0] * 3000 and res[5] == given and res[7] == 0, what
        host = res[4]
        for f in range(3000):
            w, h = sizes[f % 8]
            px = frames[f][0].reshape(-1)
            slot = host[f * img_stride:(f + 1) * img_stride]
            assert (res[1][f], res[2][f]) == (w, h) and np.array_equal(slot[:px.size], px) and bool((slot[px.size:] == POISON).all()), (what, f)
        for f in picks:
            assert np.array_equal(host[f * img_stride:f * img_stride + want24[f][3].size], want24[f][3])

    with cniic_amd.Context(0) as ctx:
        check_all(batch(ctx, streams, img_stride), "one call", 3000)
        monkeypatch.setenv(KNOB_BUDGET, "20000")                             # several chunks
        check_all(batch(ctx, streams, img_stride), "chunks", 3000)
        check_all(batch(ctx, streams, img_stride, host_src=True, host_out=True), "chunks, host memory", 3000)
        monkeypatch.setenv(KNOB_BUDGET, "1")                                 # a frame a chunk
        few = run(ctx, streams[:24], want24, img_stride, "a frame a chunk")
        assert few[5] == 24
        monkeypatch.delenv(KNOB_BUDGET)
        other = [encoded(Z.noise(32, 32), "noise 32x32"), encoded(Z.photo_like(64, 64), "photo 64x64")]
        want_o = singles("volume other", other, 3 * 64 * 64)
        for turn in range(3):                                                # alternating calls on one context
            run(ctx, streams[:24], want24, img_stride, "turn %d" % turn)
            run(ctx, other, want_o, 3 * 64 * 64, "turn %d, other" % turn)
        monkeypatch.setenv(KNOB_BATCH_OFF, "1,5,6,23")
        some = batch(ctx, streams[:24], img_stride)
        monkeypatch.delenv(KNOB_BATCH_OFF)
        assert some[5] == 20
        check_against_singles(some, want24, img_stride, "frames switched off")


def test_measure_batch_is_the_loop_of_the_three_single_calls(monkeypatch):
    import torch
    import cniic_amd
    from cniic_amd import _lib
    monkeypatch.setenv("CNIIC_TEST_ZD_SMALL_FLOOR_OFF", "1")                # the encode route's floor as well
    dev = torch.device("cuda", 0)
    imgs = [Z.photo_like(13, 5), Z.noise(32, 32), Z.flat(8, 8), Z.photo_like(64, 64), Z.noise(7, 3), Z.photo_like(333, 200)]
    with cniic_amd.Context(0) as ref, cniic_amd.Context(0) as ctx:
        rows_want, datas = [], []
        for im in imgs:
            rc, data, _ = ref.encode(EXPR, im)
            rc2, img_back = ref.decode(EXPR, data)
            assert rc == 0 and rc2 == 0 and np.array_equal(img_back, im)
            npx = im.shape[0] * im.shape[1]
            rows_want.append(dict(compressed_size=len(data), compression_ratio=len(data) / (npx * 24.0) * 100.0, error=ref.mse(im, img_back), rc=0))
            datas.append(bytes(data))
        buf = np.concatenate([im.reshape(-1) for im in imgs])
        offs = list(np.cumsum([0] + [im.size for im in imgs[:-1]]))
        ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
        F = len(imgs)
        stride = ((max(len(d) for d in datas) + 15) & ~15) + 16
        src = torch.from_numpy(buf).to(dev)
        out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch(EXPR, src, [int(o) for o in offs], ws, hs, out, stride)
        dec, enc = ctx.kernel_time(TIMER)[1], ctx.kernel_time(ENC_TIMER)[1]         # both routes' stages, readable side by side
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert rc == 0 and dec == F - 1 and enc == F - 1
        host = out.cpu().numpy()
        for f in range(F):
            got = {k: rows[f][k] for k in ("compressed_size", "compression_ratio", "error", "rc")}
            assert got == rows_want[f], (f, got, rows_want[f])
            assert lens[f] == len(datas[f]) and host[f * stride:f * stride + lens[f]].tobytes() == datas[f], f


def mutants():
    rng = np.random.default_rng(20251021)
    bases = [encoded(Z.photo_like(13, 5), "photo 13x5"), encoded(Z.noise(32, 32), "noise 32x32"), encoded(Z.flat(32, 32), "flat 32x32"), encoded(two_colour(16, 9))]
    out = []
    for k in range(200):
        s = bytearray(bases[k % 4])
        at = int(rng.integers(16, len(s)))                                    # behind the dimensions: every mutant stays a candidate
        s[at] = (s[at] + int(rng.integers(1, 256))) & 255
        out.append(bytes(s))
    return out


def test_mutants_behave_as_the_single_decode_does():
    import cniic_amd
    streams = mutants()
    img_stride = 3 * 32 * 32 + 13
    want = singles("mutants", streams, img_stride)
    verdicts = [analyse(s)["verdict"] for s in streams]
    print("mutants:", {v: verdicts.count(v) for v in sorted(set(verdicts))})
    assert all(analyse(s)["cand"] for s in streams) and verdicts.count("ok") >= 10 and verdicts.count("symbol") >= 10 and verdicts.count("record") >= 1 and verdicts.count("short") >= 1
    check_against_claims(streams, want, "mutants")
    with cniic_amd.Context(0) as ctx:
        for host_src in (False, True):
            res = run(ctx, streams, want, img_stride, "mutants", host_src=host_src)
            assert res[5] == 200


def test_the_floor(monkeypatch):
    """without the fixture's knob: a call with fewer than FLOOR_FEW candidates goes to the workers whole; from FLOOR_FEW on the candidates
    of at most FLOOR_PX_FEW pixels take the route, from FLOOR_MANY on those of at most FLOOR_PX_MANY; nothing else changes"""
    import cniic_amd
    monkeypatch.delenv(KNOB_FLOOR_OFF)
    small, large = encoded(Z.photo_like(13, 5), "photo 13x5"), encoded(Z.photo_like(128, 96), "photo 128x96")
    assert 13 * 5 <= FLOOR_PX_FEW < 128 * 96 <= FLOOR_PX_MANY == MAX_PX
    img_stride = 3 * 128 * 96
    want_s, want_l = singles("floor small", [small], img_stride), singles("floor large", [large], img_stride)
    with cniic_amd.Context(0) as ctx:
        for n_small, n_large, given in ((1, 0, 0), (FLOOR_FEW - 1, 0, 0), (FLOOR_FEW, 0, FLOOR_FEW), (1, FLOOR_FEW - 1, 1), (0, FLOOR_FEW, 0),
                                        (0, FLOOR_MANY - 1, 0), (0, FLOOR_MANY, FLOOR_MANY), (1, FLOOR_MANY - 2, 1), (1, FLOOR_MANY - 1, FLOOR_MANY)):
            res = batch(ctx, [small] * n_small + [large] * n_large, img_stride)
            assert res[5] == given and res[7] == 0, (n_small, n_large, res[5])
            check_against_singles(res, want_s * n_small + want_l * n_large, img_stride, "floor, %d small and %d large frames" % (n_small, n_large))
        monkeypatch.setenv(KNOB_FLOOR_OFF, "1")
        res = batch(ctx, [large], img_stride)
        assert res[5] == 1
