"""hilbert(rle(d)) through the entry points that take an expression, and `hilbert(rle)` streams on cniic_codec_decode_batch's batched
route (k_rle.hip, k_rle_decb_*).  References: tests/rle_approx_ref.py (the encoder restated), oracle_lib (decode, hilbert_linearize)
and integer arithmetic for the MSE; nothing is compared with the code under test alone.

The route's granularities -- 1024 records per counts block, 4096 colours per stretch, 16 colours per thread, 4096 frames per set --
are where the frames' edges are put; so is the route's limit of 2^18 pixels per frame (larger frames go to the worker contexts)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rle_approx_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["photo", "flat", "ramp", "checker", "noise"]
DS = R.D_VALUES   # (the Makefile's five, a half, sqrt 2, sqrt 3, 1e-9, 441.7, and the edges inf, -1, NaN)
SIZES = [(1, 1), (300, 1), (37, 29), (333, 211)]
SENTINEL, GUARD = 0xA7, 256
ROUTE_MAX_PX = 1 << 18   # the header's: frames of more pixels are decoded singly
ANY = tuple(range(-1, -10, -1))


def _image(kind, w, h):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + 77 + w) if kind == "photo" else getattr(R, kind)(w, h)


def _expr(d):
    return "hilbert(rle(%r))" % float(d)


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


_EXPECTED = {}


def _expected(kind, w, h):
    """R.encode_py of the image for every d of DS, computed once"""
    key = (kind, w, h)
    if key not in _EXPECTED:
        img = _image(kind, w, h)
        lin = O.hilbert_linearize(img)
        _EXPECTED[key] = (img, [R.encode_py(lin, w, h, d) for d in DS])
    return _EXPECTED[key]


# ---------------------------------------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_expression_encodes_like_the_restatement_and_the_f64_entry_point(ctx, w, h, kind):
    from cniic_amd import _lib
    img, exp = _expected(kind, w, h)
    for d, want in zip(DS, exp):
        rc, data, _ = ctx.encode(_expr(d), img)
        assert rc == 0 and data == want, (kind, d)
        rc, data2 = ctx.hilbert_rle_approx_encode(d, img)
        assert rc == 0 and data2 == want, (kind, d)
    # the capacity retry: one byte short says what is needed, and that much is enough
    want = exp[2]
    out = np.zeros(len(want), np.uint8)
    rc, need, _ = ctx.encode(_expr(DS[2]), img, out=out[:len(want) - 1], allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(want)
    rc, ln, _ = ctx.encode(_expr(DS[2]), img, out=out)
    assert rc == 0 and out[:ln].tobytes() == want


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_encode_batch_var_at_odd_offsets(ctx, w, h, on_dev):
    import torch
    from cniic_amd import _lib
    imgs = [_expected(k, w, h)[0] for k in KINDS]
    nb = w * h * 3
    offs = [1 + f * (nb + 3) + (f & 1) * 2 for f in range(len(imgs))]    # odd byte offsets, frames apart by odd gaps
    buf = np.zeros(offs[-1] + nb + 8, np.uint8)
    for o, im in zip(offs, imgs):
        buf[o:o + nb] = im.reshape(-1)
    src = torch.from_numpy(buf).cuda() if on_dev else buf
    for di, d in enumerate(DS):
        want = [_expected(k, w, h)[1][di] for k in KINDS]
        stride = max(len(s) for s in want) + 5
        out = torch.zeros(stride * len(imgs), dtype=torch.uint8, device="cuda") if on_dev else np.zeros(stride * len(imgs), np.uint8)
        torch.cuda.synchronize()
        rc, lens, rcs, _ = ctx.encode_batch_var(_expr(d), src, offs, [w] * 5, [h] * 5, out, stride)
        got = out.cpu().numpy() if on_dev else out
        assert rc == 0 and rcs == [0] * 5 and lens == [len(s) for s in want], d
        for f, s in enumerate(want):
            assert got[f * stride:f * stride + len(s)].tobytes() == s, (d, f)
    # the capacity retry per frame: a stride that the longest stream does not fit fails that frame alone, with what it needs
    want = [_expected(k, w, h)[1][0] for k in KINDS]
    longest = max(len(s) for s in want)
    if min(len(s) for s in want) + 4 <= longest:
        stride = (longest - 1) & ~3
        out = np.zeros(stride * 5, np.uint8)
        rc, lens, rcs, _ = ctx.encode_batch_var(_expr(DS[0]), src, offs, [w] * 5, [h] * 5, out, stride, allow=(_lib.CAPACITY,))
        for f, s in enumerate(want):
            fits = ((len(s) + 3) & ~3) <= stride
            assert rcs[f] == (0 if fits else _lib.CAPACITY) and lens[f] == len(s), f
            if fits:
                assert out[f * stride:f * stride + len(s)].tobytes() == s
        assert rc == _lib.CAPACITY


def test_encode_batch_of_equal_frames(ctx):
    import torch
    w, h = 37, 29
    imgs = [_expected(k, w, h)[0] for k in KINDS]
    fr = torch.from_numpy(np.stack(imgs)).cuda()
    for di in (2, 4, 10, 12):   # d = 4, 16, inf, NaN
        want = [_expected(k, w, h)[1][di] for k in KINDS]
        stride = (max(len(s) for s in want) + 7) & ~3
        out = torch.zeros(stride * 5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, lens, rcs, _ = ctx.encode_batch(_expr(DS[di]), fr, w, h, 5, out, stride)
        got = out.cpu().numpy()
        assert rc == 0 and rcs == [0] * 5
        for f, s in enumerate(want):
            assert lens[f] == len(s) and got[f * stride:f * stride + len(s)].tobytes() == s, (DS[di], f)


# ---------------------------------------------------------------------------------------------------------------- measure
MEASURE_SIZES = [(96, 64), (37, 29), (1, 1), (300, 1), (1, 77), (64, 64), (130, 50), (33, 97), (128, 16), (17, 17), (80, 45), (5, 3)]


def _measure_images():
    return [_image(KINDS[i % 5], w, h) for i, (w, h) in enumerate(MEASURE_SIZES)]


def _exact_mse(a, b):
    d = a.astype(np.int64).reshape(-1) - b.astype(np.int64).reshape(-1)
    return int((d * d).sum()) / (a.shape[0] * a.shape[1])


@pytest.mark.parametrize("d", [4.0, 16.0])
def test_measure_batch_rows(ctx, d):
    from cniic_amd import Codec, HilbertRleApprox
    imgs = _measure_images()
    buf, offs, ws, hs = Codec._packed(imgs)
    rc, rows, lens = ctx.measure_batch(_expr(d), buf, offs, ws, hs)
    assert rc == 0
    mirror = HilbertRleApprox(d, ctx=ctx).measure(imgs)
    for f, im in enumerate(imgs):
        h, w = im.shape[:2]
        want = R.encode_py(O.hilbert_linearize(im), w, h, d)
        orc, back = O.decode("hilbert(rle)", want)
        assert orc == 0
        rc1, single, _ = ctx.encode(_expr(d), im)
        rc2, sback = ctx.decode(_expr(d), single)
        assert rc1 == 0 and rc2 == 0 and single == want and np.array_equal(sback, back)
        for row in (rows[f], mirror[f]):
            assert row["rc"] == 0 and row["lossless_mismatch"] == 0, f
            assert row["compressed_size"] == len(want) == lens[f], f
            assert row["compression_ratio"] == len(want) / (w * h * 24.0) * 100.0, f     # bench.rs:43,74
            assert row["error"] == _exact_mse(im, back) == ctx.mse(im, sback), f


def test_harness_writes_the_references_csv(tmp_path):
    exe = os.path.join(ROOT, "tools", "cniic_bench")
    assert os.path.exists(exe), "tools/cniic_bench is built by `make -C cniic_amd/csrc`"
    names, imgs = [], []
    for i, (w, h) in enumerate([(96, 64), (333, 200), (40, 33)]):
        imgs.append(_image(KINDS[i], w, h))
        names.append("img%d.ppm" % i)
        with open(tmp_path / names[-1], "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h) + imgs[-1].tobytes())
    r = subprocess.run([exe, "--codec=hilbert(rle(4))"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    loop = open(tmp_path / "output" / "hilbert-rle-approx_4.csv").read().strip().split("\n")
    r = subprocess.run([exe, "--codec=hilbert(rle(4))", "--one-call"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    one = open(tmp_path / "output" / "hilbert-rle-approx_4.csv").read().strip().split("\n")
    assert one[0] == loop[0] == "name,compressed_size,compression_ratio,error"
    assert [l.split(",")[0] for l in one[1:]] == names and sorted(one[1:]) == sorted(loop[1:])
    for line, im in zip(one[1:], imgs):
        h, w = im.shape[:2]
        assert int(line.split(",")[1]) == len(R.encode_py(O.hilbert_linearize(im), w, h, 4.0))


# ---------------------------------------------------------------------------------------------------------------- the batched decode
def _records(runs):
    return b"".join(struct.pack("<BQBBB", c, 3, *rgb) for c, rgb in runs)


def _stream(w, h, runs):
    return struct.pack("<II", w, h) + _records(runs)


def _unit_runs(n, seed):
    """n runs of one pixel, neighbours of different colours"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, 256, (n, 3))
    return [(1, (int(c[0]), int(c[1]), int(i & 255))) for i, c in enumerate(cols)]


def _enc(im, d):
    h, w = im.shape[:2]
    return R.encode_py(O.hilbert_linearize(im), w, h, d)


def _on_route(data, img_stride):
    if len(data) < 8:
        return False
    w, h = struct.unpack("<II", data[:8])
    return 0 < w * h <= ROUTE_MAX_PX and w * h * 3 <= img_stride


class Batch:
    """streams + what the oracle and the single decode say about each of them (computed once, shared by the runs)"""

    def __init__(self, ctx, streams, img_stride, expected=None):
        self.ctx, self.streams, self.img_stride = ctx, streams, img_stride
        self.oracle, self.single = [], []
        for f, s in enumerate(streams):
            orc, oimg = O.decode("hilbert(rle)", s)
            if expected is not None and f in expected:
                oimg = expected[f]
            self.oracle.append((orc, oimg))
            one = np.zeros(max(img_stride, 1), np.uint8)
            raw = np.frombuffer(s + b"\0", np.uint8)
            rc, sw, sh = ctx.decode_into("hilbert(rle)", raw, len(s), one, allow=ANY)
            msg = (ctx._L.cniic_last_error(ctx.h) or b"").decode() if rc != 0 else ""
            self.single.append((rc, sw, sh, one, msg))

    def run(self, stride, dev_in, dev_out, expr="hilbert(rle)", off=(), shift_in=0, shift_out=0):
        import torch
        from cniic_amd import _lib
        F, img_stride = len(self.streams), self.img_stride
        lens = [len(s) for s in self.streams]
        buf = np.zeros(F * stride + max(lens) + 16 + shift_in, np.uint8)
        for f, s in enumerate(self.streams):
            buf[shift_in + f * stride:shift_in + f * stride + len(s)] = np.frombuffer(s, np.uint8)
        out = np.full(shift_out + F * img_stride + GUARD, SENTINEL, np.uint8)
        src = torch.from_numpy(buf).cuda()[shift_in:] if dev_in else buf[shift_in:]
        dst = torch.from_numpy(out).cuda() if dev_out else out
        torch.cuda.synchronize()
        self.ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        try:
            rc, ws, hs, rcs = self.ctx.decode_batch(expr, src, stride, lens, F, dst[shift_out:], img_stride, allow=ANY)
            launches = self.ctx.kernel_time("rle_dec_batch")[1]
            msg = (self.ctx._L.cniic_last_error(self.ctx.h) or b"").decode() if rc != 0 else ""
        finally:
            self.ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        got = (dst.cpu().numpy() if dev_out else out)
        what = (stride, dev_in, dev_out, expr, off)
        assert (got[:shift_out] == SENTINEL).all(), what
        got = got[shift_out:]
        first = None
        for f in range(F):
            orc, oimg = self.oracle[f]
            src_rc, sw, sh, spx, smsg = self.single[f]
            assert rcs[f] == src_rc, what + (f, rcs[f], src_rc)
            ok = orc == 0 and oimg.size <= img_stride
            assert (rcs[f] == 0) == ok, what + (f, rcs[f], orc)
            if rcs[f] != 0 and first is None:
                first = (rcs[f], smsg)
            if not ok:
                continue
            assert (ws[f], hs[f]) == (oimg.shape[1], oimg.shape[0]) == (sw, sh), what + (f,)
            frame = got[f * img_stride:(f + 1) * img_stride]
            assert np.array_equal(frame[:oimg.size], oimg.reshape(-1)), what + (f, "pixels")
            assert np.array_equal(spx[:oimg.size], oimg.reshape(-1)), what + (f, "single pixels")
            assert (frame[oimg.size:] == SENTINEL).all(), what + (f, "a write past w*h*3")
        assert (got[F * img_stride:] == SENTINEL).all(), what + ("a write past the last frame",)
        assert (rc, msg) == (first if first else (0, "")), what     # the first failure's status and message, as the single decode words it
        want = sum(1 for f, s in enumerate(self.streams) if f not in off and _on_route(s, img_stride))
        assert launches == want, what + ("frames on the route", launches, want)


def _edge_streams():
    """exact and approximate streams with their edges at the route's granularities, and frames the route must leave alone"""
    from cniic_amd import synth
    s = []
    for n in (4095, 4096, 4097):                                     # colours: one below, at and one above a stretch
        s.append(_enc(R.noise(n, 1, n), 0.0))
    s.append(_enc(synth.photo(64, 64, synth.SEED0 + 5), 4.0))        # 4096 colours as a 2^n square (the tile scatter), approximate
    s.append(_enc(R.ramp(4111, 1), 16.0))                            # 16 colours per thread: a stretch's last thread straddles n
    for r in (1023, 1024, 1025, 2047, 2048, 2049):                   # complete records: around one and two counts blocks
        s.append(_stream(r, 1, _unit_runs(r, r)))
    s.append(_enc(R.flat(100, 50), 0.0))                             # runs of 255: the 17th crosses colour 4096
    s.append(_enc(R.flat(100, 50), math.inf))
    s.append(_enc(R.noise(1, 1), 2.0))                               # 1 x 1
    s.append(_enc(R.checker(1, 300), 0.0))                           # 1 x N
    s.append(_enc(R.checker(300, 1), 8.0))                           # N x 1
    s.append(_enc(synth.photo(37, 29, synth.SEED0 + 6), 1.0))
    s.append(struct.pack("<II", 0, 5))                               # w * h == 0: not on the route (decodes to nothing)
    s.append(struct.pack("<II", 7, 0) + _records(_unit_runs(3, 1)))
    s.append(b"\x03\x00\x00")                                        # shorter than a header
    s.append(b"")
    s.append(_enc(R.noise(101, 50), 0.0))                            # does not fit img_stride (100 x 50 x 3)
    s.append(struct.pack("<II", 1 << 16, 1 << 16) + _records(_unit_runs(2, 2)))   # w * h == 2^32
    s.append(_enc(synth.photo(40, 30, synth.SEED0 + 7), 0.0))        # a good frame behind them
    return s


@pytest.fixture(scope="module")
def edges(ctx):
    return Batch(ctx, _edge_streams(), 100 * 50 * 3)


@pytest.mark.parametrize("dev_in,dev_out", [(True, True), (True, False), (False, True), (False, False)])
def test_route_edges_against_the_oracle(edges, dev_in, dev_out):
    longest = max(len(s) for s in edges.streams)
    for stride in ((longest + 3) & ~3, longest + (2 if longest % 2 else 1), longest):   # a multiple of 4, odd, tight
        edges.run(stride, dev_in, dev_out)
    edges.run(longest + 5, dev_in, dev_out, expr="hilbert(rle(4))", shift_in=1, shift_out=3)   # decode ignores d; buffers off their words


def test_frames_sent_off_the_route_come_out_the_same(edges, monkeypatch):
    monkeypatch.setenv("CNIIC_TEST_DECODE_BATCH_OFF", "0,3,11,24")
    longest = max(len(s) for s in edges.streams)
    edges.run(longest + 1, True, True, off=(0, 3, 11, 24))
    edges.run(longest, False, False, off=(0, 3, 11, 24))


def _hostile_streams():
    from cniic_amd import synth
    im = synth.photo(40, 30, synth.SEED0 + 9)
    good = _enc(im, 4.0)
    R_ = (len(good) - 8) // 12
    assert R_ > 40
    k = R_ // 2

    def patched(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)
    s = [good,
         patched(8 + 12 * k, 0),                                      # a zero count inside the pixels
         good + _records([(0, (1, 2, 3))]),                           # ... and after them: never read, not an error
         good + _records([(0, (1, 2, 3))] * 5000),                    # (thousands of them: the expansion must not walk over them)
         patched(8 + 12 * k + 1, 4),                                  # a length word != 3
         patched(8 + 12 * k + 8, 1),                                  # ... in its high byte
         patched(8 + 12 * (R_ - 1) + 1, 2),                           # ... in the last record that is read
         good[:8 + 12 * k + 5],                                       # the tail cut mid-record before the last pixel
         good + b"\x07\x03\x00\x00\x00",                              # ... and after it
         good[:8 + 12 * k],                                           # the records stop short: the rest is zero
         good[:8],                                                    # no records at all: a black image
         good[:8 + 3],                                                # ... and a cut first record
         good]
    # a long stream whose first bad record lies in its third counts block, next to one whose bad record lies past the pixels
    runs = _unit_runs(3000, 5)
    bad = list(runs)
    bad[2500] = (0, (9, 9, 9))
    s.append(_stream(3000, 1, bad))
    s.append(_stream(2500, 1, bad))
    s.append(_stream(3000, 1, runs))
    return s


def test_hostile_frames_next_to_good_ones(ctx):
    b = Batch(ctx, _hostile_streams(), 3000 * 3)
    from cniic_amd import _lib
    assert [x[0] for x in b.single[:13]] == [0, _lib.DECODE, 0, 0, _lib.DECODE, _lib.DECODE, _lib.DECODE, _lib.DECODE, 0, 0, 0, _lib.DECODE, 0]
    assert [x[0] for x in b.single[13:]] == [_lib.DECODE, 0, 0]
    longest = max(len(s) for s in b.streams)
    for dev_in, dev_out in ((True, True), (False, False), (True, False)):
        b.run(longest, dev_in, dev_out)
        b.run(longest + 3, dev_in, dev_out)


def test_a_second_set_of_frames(ctx):
    """4097 frames of 2 x 2: one more than a set of launches takes"""
    rng = np.random.default_rng(11)
    streams = []
    for f in range(4097):
        im = rng.integers(0, 4, (2, 2, 3)).astype(np.uint8) * 60
        streams.append(_enc(im, float(f % 3)))       # exact and approximate streams mixed
    streams[4095] = streams[4095][:8 + 5]             # a bad frame at the end of the first set
    b = Batch(ctx, streams, 12)
    b.run(8 + 4 * 12, True, True)
    b.run(8 + 4 * 12 + 1, False, False)


def test_frames_around_the_routes_pixel_limit(ctx):
    """2^18 pixels as a 2^n square and as a row are on the route, one pixel more is not; all three come out as the oracle's"""
    streams = [_enc(R.ramp(512, 512), 16.0), _enc(R.flat(1 << 18, 1), 0.0), _enc(R.checker((1 << 18) + 1, 1), math.inf), _enc(R.noise(9, 7), 0.0)]
    b = Batch(ctx, streams, ((1 << 18) + 1) * 3)
    assert [_on_route(s, b.img_stride) for s in streams] == [True, True, False, True]
    b.run(max(len(s) for s in streams) + 1, True, True)
    b.run(max(len(s) for s in streams), False, False)


def test_injected_scan_applies_to_frames_of_its_size(ctx):
    from cniic_amd import synth
    w, h = 37, 29
    y, x = np.mgrid[0:h, 0:w]
    x = np.where(y & 1, w - 1 - x, x)
    snake = np.stack([x.reshape(-1), y.reshape(-1)], 1).astype(np.uint32)
    imgs = [synth.photo(w, h, synth.SEED0 + 20), R.noise(40, 30), synth.photo(w, h, synth.SEED0 + 21), R.ramp(64, 64)]
    streams = [_enc(imgs[0], 4.0), _enc(imgs[1], 0.0), _enc(imgs[2], 0.0), _enc(imgs[3], 2.0)]
    expected = {}
    for f in (0, 2):   # what the records hold, laid along the injected order
        lin = np.concatenate([np.tile(np.frombuffer(streams[f][8 + 12 * r + 9:8 + 12 * r + 12], np.uint8), (streams[f][8 + 12 * r], 1))
                              for r in range((len(streams[f]) - 8) // 12)])
        img = np.zeros((h, w, 3), np.uint8)
        img[snake[:, 1], snake[:, 0]] = lin
        expected[f] = img
    ctx.set_scan(w, h, snake)
    try:
        b = Batch(ctx, streams, 64 * 64 * 3, expected=expected)
        assert not np.array_equal(expected[2], imgs[2])
        b.run(max(len(s) for s in streams) + 2, True, True)
        b.run(max(len(s) for s in streams), False, True)
    finally:
        ctx.set_scan(w, h, None)


def test_differential_fuzz_with_more_rle(ctx, monkeypatch):
    """tests/fuzz_decode_batch.py with `hilbert(rle)` (exact and running-average streams) as three batches in four
    (CNIIC_FUZZ_SECONDS for longer)"""
    import fuzz_decode_batch as Z
    plain = Z.codec
    monkeypatch.setattr(Z, "codec", lambda: "hilbert(rle)" if Z.rng.random() < 0.75 else plain())
    assert Z.run(ctx, float(os.environ.get("CNIIC_FUZZ_SECONDS", "5"))) > 0
