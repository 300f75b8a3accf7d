"""Hilbert { compress: Zip } streams of cniic_hilbert_zip_decode_batch on the small-frame decode route (k_hz_small_dec in
k_zd_small_dec.hip: `zip(dict)`'s workgroup-per-frame decode under the lenient verdict and the record cut of cniic_amd/csrc/hz_small.hpp;
include/cniic_hip.h above cniic_hilbert_zip_encode_batch_var).  Every comparison is exact: a frame's status, dimensions, pixels and message
are those of cniic_hilbert_zip_decode for that stream alone on a context that has seen no batch -- a failing frame's destination keeps its
poison there as here --, and the pixels are those of tests/zip_dict_ref.py (hilbert_decode_lin) laid along oracle_lib.hilbert_iter.  Which
frames took the route is read from the stage timer "hz_small_dec_batch", whose launch count is the number of frames the kernel was given;
"hz_small_dec_handback" counts those of them the kernel handed back to the workers.

What a case claims about a stream -- whether it is a candidate, its verdict, where its colours end, the pairs its text needs, its generation
and the pairs a byte visits, and so which side of a cap it lies on -- is computed from the symbols alone (analyse);
tests/test_hz_small_cpu.py asserts the same claims without a GPU, against tests/zip_dict_ref.py and tests/hz_small_check.cpp."""
import struct

import numpy as np
import pytest

import test_hz_small_batch as HB
import test_zd_small_decode as ZD
import zip_dict_ref as Z
from test_zd_small_decode import aligned, from_pairs, pairs_of

pytestmark = pytest.mark.gpu

MAX_PX = 16384                 # kHzSmallMaxPx (cniic_amd/csrc/hz_small.hpp)
MAX_PAIRS = 24576              # kZsdMaxPairs (zd_small_dec.hpp)
HOPS, ROUNDS = 64, 64          # kZsdHops, kZsdRounds
HEAD = 8                       # kHzHead: the raw dimensions, all the host reads of a stream
FLOOR_FEW, FLOOR_MANY = 4, 256                 # kHzSmallDecFloorFew, kHzSmallDecFloorMany (codec.cpp): candidates of a call from which ...
FLOOR_PX_FEW, FLOOR_PX_MANY = 4096, 16384      # kHzSmallDecFloorPxFew, kHzSmallDecFloorPxMany: ... those of at most so many pixels take the route
TIMER, HANDBACK = "hz_small_dec_batch", "hz_small_dec_handback"
KNOB_OFF, KNOB_MAX_PX, KNOB_FLOOR_OFF = "CNIIC_TEST_HZ_SMALL_DEC_OFF", "CNIIC_TEST_HZ_SMALL_DEC_MAX_PX", "CNIIC_TEST_HZ_SMALL_DEC_FLOOR_OFF"
KNOB_PAIRS, KNOB_HOPS, KNOB_ROUNDS = "CNIIC_TEST_HZ_SMALL_DEC_MAX_PAIRS", "CNIIC_TEST_HZ_SMALL_DEC_HOPS", "CNIIC_TEST_HZ_SMALL_DEC_ROUNDS"
KNOB_BUDGET = "CNIIC_TEST_MEASURE_BUDGET"
OK, DECODE, CAPACITY = 0, -6, -8
POISON = ZD.POISON
EOF, FIRST = Z.EOF, Z.FIRST_NEW
MESSAGES = {"symbol": "zip-dict: pair %d uses a symbol that has not been handed out", "dangling": "zip-dict: a first symbol without a second at the end of the stream"}
SIZES, UNROUTED, CONTENTS = HB.SIZES, HB.UNROUTED, HB.CONTENTS


@pytest.fixture(autouse=True)
def _no_floor(monkeypatch):
    """the tests of this module step over the route's floor; test_the_floor holds it"""
    monkeypatch.setenv(KNOB_FLOOR_OFF, "1")


# ------------------------------------------------------------------ streams
def encoded(img, key=None):
    return HB.restated(img, key)


def library():
    """[(name, image, stream)]: every size under every content, then the two frames that ride along unrouted"""
    out = [("%s %dx%d" % (nm, w, h), gen(w, h)) for w, h in SIZES for nm, gen in CONTENTS]
    out += [("photo %dx%d unrouted" % (w, h), Z.photo_like(w, h)) for w, h in UNROUTED]
    return [(nm, im, encoded(im, "dec " + nm)) for nm, im in out]


def stream_of_text(text, w, h):
    """the dimensions as given, then the coder over any text"""
    return struct.pack("<II", w, h) + Z.encode_c(HB.clib(), bytes(text))


def along_the_scan(lin, w, h):
    """the image whose pixels in scan order are lin"""
    import oracle_lib as O
    xy = O.hilbert_iter(w, h).astype(np.int64)
    img = np.zeros((h, w, 3), np.uint8)
    img[xy[:, 1], xy[:, 0]] = np.asarray(lin, np.uint8).reshape(-1, 3)
    return img


def analyse(stream, max_pairs=MAX_PAIRS, hops=HOPS, rounds=ROUNDS, max_px=MAX_PX):
    """What the route makes of a stream, from its symbols alone -> dict.  cand: 8 bytes of dimensions and 1 .. max_px pixels.  For a
    candidate: w, h, need, P (the pairs looked at), kb (the first of them with a symbol not handed out, or P), gen (the deepest generation
    below kb), verdict (ok / back / symbol / dangling), a, message; for ok: needed (the pairs the lazy reader reads, None for a short text),
    records (the whole records the text reaches), cut (the scan positions that get colours), visits (the most pairs a byte the kernel reads
    visits) and lin (the w h pixels in scan order, zeros from the cut on)."""
    stream = bytes(stream)
    if len(stream) < HEAD:
        return dict(cand=False)
    w, h = struct.unpack_from("<II", stream)
    if not 1 <= w * h <= max_px:
        return dict(cand=False, w=w, h=h)
    body = stream[HEAD:]
    n = len(body)
    need, P = 11 * w * h, min(n // 4, max_pairs)
    C = need + 1
    pairs = pairs_of(body)[:P]
    length, gen, kb = [], [], P
    for k, (s1, s2) in enumerate(pairs):
        if any(s != EOF and s >= FIRST + k for s in (s1, s2)):
            kb = k
            break
        length.append(min(sum(1 if s < FIRST else 0 if s == EOF else length[s - FIRST] for s in (s1, s2)), C))
        gen.append(1 + max(-1 if s < FIRST or s == EOF else gen[s - FIRST] for s in (s1, s2)))
    res = dict(cand=True, w=w, h=h, need=need, P=P, kb=kb, gen=max(gen, default=-1), a=0, message="")

    def verdict(v, a=0):
        res.update(verdict=v, a=a)
        if v in MESSAGES:
            res["message"] = MESSAGES[v] % ((a,) if v == "symbol" else ())
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
    # the text of the pairs read, and per byte the pairs visited from the pair that wrote it
    text, vis = [], []
    lit_v = np.ones(1, np.uint32)
    for s1, s2 in pairs[:needed if needed is not None else kb]:
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
    whole = np.concatenate(text + [np.zeros(0, np.uint8)])[:need]
    visits = np.concatenate(vis + [np.zeros(0, np.uint32)])[:need]
    records = min(total, need) // 11
    rec, rvis = whole[:11 * records].reshape(-1, 11), visits[:11 * records].reshape(-1, 11)
    bad = np.flatnonzero((rec[:, 0] != 3) | rec[:, 1:8].any(axis=1))
    cut = int(bad[0]) if bad.size else records
    read = np.concatenate([rvis[:, :8].reshape(-1), rvis[:cut, 8:].reshape(-1), np.zeros(1, np.uint32)])
    res.update(needed=needed, records=records, cut=cut, visits=int(read.max()))
    if res["visits"] > hops:
        return verdict("back")
    lin = np.zeros((w * h, 3), np.uint8)
    lin[:cut] = rec[:cut, 8:11]
    res["lin"] = lin
    return verdict("ok")


def takes(stream, img_stride, F=1, stride=1 << 40, scan=None, **caps):
    """whether the route is given the stream: a candidate whose image fits, which ends before the next one starts, of no injected scan's size"""
    a = analyse(stream, **caps)
    return a["cand"] and 3 * a["w"] * a["h"] <= img_stride and (F == 1 or stride >= len(stream)) and (a["w"], a["h"]) != scan


def back(stream, **caps):
    return analyse(stream, **caps).get("verdict") == "back"


# ------------------------------------------------------------------ GPU helpers
_last_error = ZD._last_error
_SINGLES = {}


def singles(key, streams, cap, scan=None):
    """cniic_hilbert_zip_decode of every stream alone (capacity cap), on a context that has seen no batch
    -> [(rc, w, h, pixels or None, message)]; a failing stream leaves its destination's poison alone"""
    import cniic_amd
    if key not in _SINGLES:
        res = []
        with cniic_amd.Context(0) as ref:
            if scan is not None:
                ref.set_scan(*scan)
            for s in streams:
                out = np.full(max(cap, 1), POISON, np.uint8)
                raw = np.frombuffer(bytes(s) + b"\0", np.uint8)
                rc, w, h = ref.hilbert_zip_decode_into(raw, len(s), out[:cap], allow=(DECODE, CAPACITY))
                if rc != 0:
                    assert bool((out == POISON).all())
                res.append((rc, w, h, out[:w * h * 3].copy() if rc == 0 else None, _last_error(ref) if rc != 0 else ""))
        _SINGLES[key] = res
    return _SINGLES[key]


def batch(ctx, streams, img_stride, stride=None, host_src=False, host_out=False, src_off=0, out_off=0):
    """one cniic_hilbert_zip_decode_batch call with the stage timers on -> (rc, ws, hs, rcs, output as a host array, frames given to the
    kernel, message, frames handed back).  The stream of frame f lies at src_off + f * stride modulo 16, its image at out_off + f *
    img_stride modulo 16, inside poisoned allocations."""
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
        rc, ws, hs, rcs = ctx.hilbert_zip_decode_batch(src[sat:], stride, lens, F, whole[at:], img_stride, allow=(DECODE, CAPACITY))
        msg = _last_error(ctx) if rc != 0 else ""
        launches, handed = ctx.kernel_time(TIMER)[1], ctx.kernel_time(HANDBACK)[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    host = whole if host_out else whole.cpu().numpy()
    assert bool((host[:at] == POISON).all()) and bool((host[at + img_stride * F:] == POISON).all())    # nothing before the first image or behind the last
    return rc, ws, hs, rcs, host[at:at + img_stride * F], launches, msg, handed


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
            assert bool((slot == POISON).all()), (what, f)                          # a frame that fails leaves its destination alone, as the single call does
    first = next((f for f, r in enumerate(rcs) if r != 0), None)
    assert rc == (0 if first is None else rcs[first]), what
    if first is not None:
        assert res[6] == want[first][4], (what, res[6], want[first][4])


def check_against_claims(streams, want, img_stride, what, scan=None):
    """the single decode against what analyse says of the stream and against the restatement (a stream handed back has no claim of its
    own: its uncapped one; an image that does not fit its room is CAPACITY, whatever the pairs say)"""
    dec = lambda s, need: Z.decode_c(HB.clib(), s, need)
    for f, s in enumerate(streams):
        a = analyse(s)
        if not a["cand"] or a["verdict"] == "back" or (a["w"], a["h"]) == scan:
            continue
        rc, w, h, px, msg = want[f]
        if 3 * a["w"] * a["h"] > img_stride:
            assert rc == CAPACITY, (what, f)
            continue
        ref = Z.hilbert_decode_lin(dec, s)
        if a["verdict"] == "ok":
            assert ref is not None and np.array_equal(ref[2], a["lin"]), (what, f)
            assert rc == 0 and (w, h) == (a["w"], a["h"]) and np.array_equal(px, along_the_scan(a["lin"], w, h).reshape(-1)), (what, f)
        else:
            assert ref is None and rc == DECODE and msg == a["message"], (what, f, msg, a["message"])


def run(ctx, streams, want, img_stride, what, **kw):
    """a batch call; the frames given to the kernel and handed back are those the streams say, the results the single decode's"""
    caps = kw.pop("caps", {})
    scan = kw.pop("scan", None)
    F, stride = len(streams), kw.get("stride") or ((max(len(s) for s in streams) + 15) & ~15)
    given = [f for f, s in enumerate(streams) if takes(s, img_stride, F, stride, scan, **caps)]
    res = batch(ctx, streams, img_stride, **kw)
    assert res[5] == len(given), (what, res[5], len(given))
    handed = [f for f in given if back(streams[f], **{k: v for k, v in caps.items() if k != "max_px"})]
    assert res[7] == len(handed), (what, res[7], len(handed))
    check_against_singles(res, want, img_stride, what)
    return res


# ------------------------------------------------------------------ the tests
def test_library_streams_alone_together_and_with_the_route_off(monkeypatch):
    import cniic_amd
    names, imgs, streams = zip(*library())
    img_stride = 3 * 19200
    want = singles("library", streams, img_stride)
    for f, im in enumerate(imgs):
        assert want[f][0] == 0 and want[f][1:3] == (im.shape[1], im.shape[0]) and np.array_equal(want[f][3], im.reshape(-1)), names[f]
    check_against_claims(streams, want, img_stride, "library")
    assert not any(back(s) for s in streams)
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "library")
        assert res[5] == len(streams) - 2 and res[7] == 0
        for f in range(0, len(streams), 5):
            run(ctx, streams[f:f + 1], want[f:f + 1], img_stride, names[f] + " alone")
        monkeypatch.setenv(KNOB_OFF, "1")
        off = batch(ctx, streams, img_stride)
        assert off[5] == 0 and ctx._L.cniic_last_kernel_time(ctx.h, TIMER.encode(), None, None) != 0
        check_against_singles(off, want, img_stride, "route off")
        monkeypatch.delenv(KNOB_OFF)
        monkeypatch.setenv(KNOB_MAX_PX, "4096")
        low = run(ctx, streams, want, img_stride, "bound 4096", caps=dict(max_px=4096))
        assert low[5] == sum(1 for im in imgs if im.shape[0] * im.shape[1] <= 4096)


def hostile():
    """[(name, stream)] around one photo-like frame of 100 x 37 and one of 4 x 4: cuts, records of another length, symbols not handed out,
    garbage, dimensions that lie"""
    w, h = 100, 37
    img = Z.photo_like(w, h)
    good = encoded(img, "hostile good")
    import oracle_lib as O
    lin = O.hilbert_linearize(img)
    npairs = (len(good) - HEAD) // 4
    a = analyse(good)
    assert a["verdict"] == "ok" and a["needed"] == npairs and a["cut"] == w * h
    out = [("good", good), ("7 bytes", good[:7]), ("8 bytes", good[:8])]
    for k in (0, 1, 100, npairs - 1):
        out += [("cut %d + %d" % (k, r), good[:HEAD + 4 * k + r]) for r in range(4)]
    for at in (0, 1234, w * h - 1):
        for lenb in (4, 2, 1):
            t = bytearray(Z.records(lin))
            t[11 * at] = lenb
            out.append(("record %d of length %d" % (at, lenb), stream_of_text(t, w, h)))
    t = bytearray(Z.records(lin))
    t[11 * 50 + 3] = 1                                   # a length of 3 + 2^24
    out.append(("record 50 with a high length byte", stream_of_text(t, w, h)))
    bad = bytearray(good)
    struct.pack_into("<H", bad, HEAD + 4 * 10, FIRST + 10)
    out.append(("pair 10 uses its own symbol", bytes(bad)))
    bad = bytearray(good)
    struct.pack_into("<H", bad, HEAD + 4 * (npairs - 1) + 2, FIRST + npairs)
    out.append(("the last needed pair's second symbol is not handed out", bytes(bad)))
    tail = struct.pack("<HH", FIRST + npairs + 5, 7)
    out.append(("the same symbol behind the last needed pair", good + tail))
    rng = np.random.default_rng(5)
    out += [("garbage %d" % g, good + rng.integers(0, 256, g, dtype=np.uint8).tobytes()) for g in (1, 2, 3, 4, 5, 255, 768)]
    body = good[HEAD:]
    out += [("dimensions that claim fewer pixels", struct.pack("<II", 50, 37) + body), ("dimensions that claim more", struct.pack("<II", 100, 38) + body),
            ("a width of 0", struct.pack("<II", 0, 37) + body), ("a height of 0", struct.pack("<II", 100, 0) + body),
            ("2^32 pixels", struct.pack("<II", 65536, 65536) + body), ("more than the bound", struct.pack("<II", 16385, 1) + body),
            ("an image one byte longer than the stride", struct.pack("<II", 3801, 1) + body[:400])]
    small = encoded(Z.noise(4, 4), "hostile 4x4")
    out += [("4x4", small), ("4x4 cut", small[:-4]), ("4x4 dangling", small[:-2])]
    return out


IMG_STRIDE_HOSTILE = 3 * 3801 - 1      # one byte short of the 3801 x 1 frame; 100 x 38 fits


def test_hostile_streams_alone_and_together():
    import cniic_amd
    names, streams = zip(*hostile())
    want = singles("hostile", streams, IMG_STRIDE_HOSTILE)
    check_against_claims(streams, want, IMG_STRIDE_HOSTILE, "hostile")
    by = dict(zip(names, want))
    kinds = {nm: analyse(s) for nm, s in zip(names, streams)}
    # the cuts that leave a first symbol alone are errors, the others zero-fill
    for k in (0, 1, 100):
        for r in range(4):
            a = kinds["cut %d + %d" % (k, r)]
            assert a["verdict"] == ("dangling" if r >= 2 else "ok") and (r >= 2 or a["cut"] < 3700), (k, r)
            assert by["cut %d + %d" % (k, r)][0] == (DECODE if r >= 2 else OK)
    for at in (0, 1234, 3699):
        for lenb in (4, 2, 1):
            a = kinds["record %d of length %d" % (at, lenb)]
            assert a["verdict"] == "ok" and a["cut"] == at and not a["lin"][at:].any()
    assert kinds["record 50 with a high length byte"]["cut"] == 50
    assert kinds["pair 10 uses its own symbol"]["verdict"] == "symbol" and kinds["pair 10 uses its own symbol"]["a"] == 10
    assert kinds["the last needed pair's second symbol is not handed out"]["verdict"] == "symbol"
    assert kinds["the same symbol behind the last needed pair"]["verdict"] == "ok" and np.array_equal(by["the same symbol behind the last needed pair"][3], by["good"][3])
    assert all(np.array_equal(by["garbage %d" % g][3], by["good"][3]) for g in (1, 2, 3, 4, 5, 255, 768))
    assert kinds["dimensions that claim fewer pixels"]["cut"] == 50 * 37 and kinds["dimensions that claim more"]["cut"] == 3700
    assert by["7 bytes"][0] == DECODE and by["7 bytes"][4] == "decode: truncated dimensions" and by["8 bytes"][0] == OK and not by["8 bytes"][3].any()
    assert by["2^32 pixels"][4] == "decode: image too large" and by["an image one byte longer than the stride"][0] == CAPACITY
    assert by["a width of 0"][0] == OK and by["more than the bound"][0] == CAPACITY
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, IMG_STRIDE_HOSTILE, "hostile")
        assert res[5] == sum(1 for a in kinds.values() if a["cand"]) - 1 and res[7] == 0       # (one candidate's image does not fit its slot)
        for f in range(len(streams)):
            run(ctx, streams[f:f + 1], want[f:f + 1], IMG_STRIDE_HOSTILE, names[f] + " alone")
        run(ctx, streams, want, IMG_STRIDE_HOSTILE, "hostile from the host", host_src=True, host_out=True)


@pytest.mark.parametrize("residue", (0, 1, 2, 3))
def test_streams_and_images_at_every_residue(residue):
    """the streams at all four byte residues (an odd stride moves them on), the images at all sixteen"""
    import cniic_amd
    imgs = [Z.photo_like(7, 9), Z.noise(4, 4), Z.flat(8, 8), HB.two_colour(13, 5), Z.photo_like(64, 64), Z.noise(37, 41), Z.photo_like(1, 1), Z.noise(3, 2)] * 2
    streams = [encoded(im) for im in imgs[:8]] * 2
    streams[3] = streams[3][:-2]            # a failing frame among good ones: a first symbol alone
    streams[9] = streams[9][:HEAD + 4 * 6]  # ... and a short one
    img_stride = 3 * 4096 + 1
    want = singles("residues", streams, img_stride)
    assert want[3][0] == DECODE and want[9][0] == OK and sum(w[0] != 0 for w in want) == 1
    stride = (max(len(s) for s in streams) + 3) | 1
    assert {(residue + f * stride) % 4 for f in range(16)} == {0, 1, 2, 3} and {(residue + f * img_stride) % 16 for f in range(16)} == set(range(16))
    with cniic_amd.Context(0) as ctx:
        for host in (False, True):
            res = run(ctx, streams, want, img_stride, "residue %d" % residue, stride=stride, src_off=residue, out_off=residue, host_src=host, host_out=host)
            assert res[5] == 16


def cap_streams():
    """[(name, stream)]: frames whose own pair counts, depths and generations the lowered knobs lie on either side of"""
    return [("photo 64x64", encoded(Z.photo_like(64, 64), "cap photo")), ("flat 32x32", encoded(Z.flat(32, 32), "cap flat")),
            ("two-colour 13x5", encoded(HB.two_colour(13, 5), "cap two")), ("noise 8x8", encoded(Z.noise(8, 8), "cap noise")),
            ("band", encoded(HB.banded(64, 64, 2000, 300), "cap band"))]


def test_the_pair_hop_and_round_caps_on_either_side(monkeypatch):
    import cniic_amd
    names, streams = zip(*cap_streams())
    img_stride = 3 * 4096
    want = singles("caps", streams, img_stride)
    assert all(w[0] == 0 for w in want)
    claims = [analyse(s) for s in streams]
    with cniic_amd.Context(0) as ctx:
        for f, a in enumerate(claims):
            for knob, key, own in ((KNOB_PAIRS, "max_pairs", a["needed"]), (KNOB_HOPS, "hops", a["visits"]), (KNOB_ROUNDS, "rounds", a["gen"] + 1)):
                for value in (own - 1, own, own + 1):
                    if value < 1:
                        continue
                    assert back(streams[f], **{key: value}) == (value < own), (names[f], key, value)
                    monkeypatch.setenv(knob, str(value))
                    res = run(ctx, streams[f:f + 1], want[f:f + 1], img_stride, "%s %s %d" % (names[f], key, value), caps={key: value})
                    assert res[7] == int(value < own)
                monkeypatch.delenv(knob)
        depth = sorted(a["visits"] for a in claims)
        monkeypatch.setenv(KNOB_HOPS, str(depth[2]))
        res = run(ctx, streams, want, img_stride, "hops %d for all" % depth[2], caps=dict(hops=depth[2]))
        assert 0 < res[7] < len(streams)


def test_mutants():
    """200 seeded mutants of four streams: a byte changed, a cut, a symbol moved up, garbage, other dimensions"""
    import cniic_amd
    rng = np.random.default_rng(11)
    bases = [encoded(Z.photo_like(23, 7)), encoded(Z.noise(8, 8)), encoded(Z.flat(5, 5)), encoded(HB.two_colour(16, 16))]
    streams = []
    for m in range(200):
        s = bytearray(bases[m % 4])
        kind = (m // 4) % 5
        if kind == 0:
            s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
        elif kind == 1:
            del s[int(rng.integers(0, len(s) + 1)):]
        elif kind == 2:
            k = int(rng.integers(0, (len(s) - HEAD) // 4))
            struct.pack_into("<H", s, HEAD + 4 * k + 2 * int(rng.integers(0, 2)), FIRST + k + int(rng.integers(-2, 3)))
        elif kind == 3:
            s += rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        else:
            struct.pack_into("<I", s, 4 * int(rng.integers(0, 2)), int(rng.integers(0, 40)))
        streams.append(bytes(s))
    img_stride = 3 * 40 * 40
    want = singles("mutants", streams, img_stride)
    check_against_claims(streams, want, img_stride, "mutants")
    claims = [analyse(s) for s in streams]
    assert {"ok", "symbol", "dangling", "none"} <= {a.get("verdict", "none") for a in claims}
    assert any(a["cut"] < a["w"] * a["h"] for a in claims if a.get("verdict") == "ok")
    with cniic_amd.Context(0) as ctx:
        run(ctx, streams, want, img_stride, "mutants")


def test_many_frames_in_one_launch_and_in_chunks(monkeypatch):
    """3000 streams in one launch; then several chunks of scratch from host memory"""
    import cniic_amd
    import test_zd_small_batch as ZB
    imgs = ZB.many()
    kinds = {}
    streams = []
    for f, im in enumerate(imgs):
        if f < 120:
            kinds[f] = encoded(im)
        streams.append(kinds[f % 120])
    img_stride = 3 * 1024
    want120 = singles("many", streams[:120], img_stride)
    want = [want120[f % 120] for f in range(3000)]
    for f in range(0, 120, 7):
        assert want[f][0] == 0 and np.array_equal(want[f][3], imgs[f].reshape(-1)), f
    with cniic_amd.Context(0) as ctx:
        res = run(ctx, streams, want, img_stride, "many")
        assert res[5] == 3000
        # host streams and host images: a chunk's scratch holds its rows, its streams and its staged images
        per = 32 + 32 + ((img_stride + 15) & ~15) + max(len(s) for s in streams[:40])
        monkeypatch.setenv(KNOB_BUDGET, str(12 * per))
        res = run(ctx, streams[:40], want[:40], img_stride, "chunks", host_src=True, host_out=True)
        assert res[5] == 40


def test_the_floor(monkeypatch):
    """fewer than FLOOR_FEW candidates stay with the workers; from there on those of at most FLOOR_PX_FEW pixels take the route, from
    FLOOR_MANY on all of them: calls of one below and of exactly each count; the floor counts the call's candidates, not a chunk's (NOTES AS)"""
    import cniic_amd
    monkeypatch.delenv(KNOB_FLOOR_OFF)
    big, above, edge = encoded(Z.photo_like(128, 96), "floor big"), encoded(Z.photo_like(17, 241), "floor above"), encoded(Z.photo_like(64, 64), "floor edge")
    kinds = [encoded(im) for im in HB.tiny(6)]
    streams = [big, above, edge] + [kinds[k % 6] for k in range(FLOOR_MANY - 3)]
    img_stride = 3 * 12288
    want9 = singles("floor", streams[:9], img_stride)
    want = want9[:3] + [want9[3 + k % 6] for k in range(FLOOR_MANY - 3)]
    assert (FLOOR_PX_FEW, FLOOR_PX_MANY) == (64 * 64, MAX_PX) and 17 * 241 == FLOOR_PX_FEW + 1
    with cniic_amd.Context(0) as ctx:
        for count, given in ((FLOOR_FEW - 1, 0), (FLOOR_FEW, FLOOR_FEW - 2), (FLOOR_MANY - 1, FLOOR_MANY - 3), (FLOOR_MANY, FLOOR_MANY)):
            res = batch(ctx, streams[:count], img_stride)
            assert res[5] == given, (count, res[5])
            check_against_singles(res, want[:count], img_stride, "floor %d" % count)
        # several chunks of scratch, the last of which holds fewer frames than the floor asks of a call
        monkeypatch.setenv(KNOB_BUDGET, str(4 * 56))          # (a row and a result row a frame: four frames a chunk)
        res = batch(ctx, streams[:11], img_stride)
        assert res[5] == 9
        check_against_singles(res, want[:11], img_stride, "floor on, chunks of four")
        monkeypatch.delenv(KNOB_BUDGET)
        monkeypatch.setenv(KNOB_FLOOR_OFF, "1")
        assert batch(ctx, streams[:1], img_stride)[5] == 1


def test_a_size_with_an_injected_scan_stays_with_the_workers():
    """those streams are laid along the injected order, the others take the route"""
    import cniic_amd
    imgs = [Z.photo_like(64, 64), Z.noise(37, 41), Z.photo_like(37, 41), Z.photo_like(41, 37), Z.noise(8, 8)]
    w, h = 37, 41
    p = np.random.default_rng(7).permutation(w * h)
    scan = (w, h, np.stack([p % w, p // w], 1).astype(np.uint32))
    streams = [encoded(im) for im in imgs]
    img_stride = 3 * 4096
    want = singles("scan", streams, img_stride, scan=scan)
    builtin = singles("scan builtin", streams, img_stride)
    for f, im in enumerate(imgs):
        injected = im.shape[:2] == (h, w)
        assert np.array_equal(builtin[f][3], im.reshape(-1)) and np.array_equal(want[f][3], builtin[f][3]) != injected, f
        if injected:
            lin = Z.hilbert_decode_lin(lambda s, need: Z.decode_c(HB.clib(), s, need), streams[f])[2]
            laid = np.zeros((h, w, 3), np.uint8)
            laid.reshape(-1, 3)[p] = lin
            assert np.array_equal(want[f][3], laid.reshape(-1)), f
    with cniic_amd.Context(0) as ctx:
        ctx.set_scan(*scan)
        res = run(ctx, streams, want, img_stride, "injected scan", scan=(w, h))
        assert res[5] == 3
        ctx.set_scan(w, h, None)
        res = run(ctx, streams, builtin, img_stride, "scan taken back")
        assert res[5] == 5


def test_the_expression_decode_never_reports_the_marks():
    import cniic_amd
    streams = [ZD.encoded(Z.photo_like(8, 8)), ZD.encoded(Z.noise(5, 3))]
    with cniic_amd.Context(0) as ctx:
        res = ZD.batch(ctx, streams, 3 * 64)
        assert res[0] == 0
        for name in (TIMER, HANDBACK):
            assert ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, None) != 0
