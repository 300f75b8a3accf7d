"""cniic_zip_back_image_measure_batch (include/cniic_hip.h): a folder of Zip::Back in one call.  Every row is held against
cniic_zip_back_image_encode -> cniic_zip_back_image_decode -> cniic_mse of that image alone, the streams against the CPU restatement of
the reference's coder (tests/zip_back_ref.py / .c): host and device images, `out` on either side and absent, a stride one byte short,
an image the reference panics on among the others, a frame per chunk under CNIIC_TEST_MEASURE_BUDGET, the class, and tools/cniic_bench
--codec='zip(back)' in a loop and in one call.  Every test here fails on a library without the call."""
import math
import os
import subprocess

import numpy as np
import pytest

import zip_back_ref as Z

pytestmark = pytest.mark.gpu

COLUMNS = ("compressed_size", "compression_ratio", "error", "rc")
BUDGET = "CNIIC_TEST_MEASURE_BUDGET"


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
    with cniic_amd.Context(0) as c:
        yield c


def folder():
    """the sizes the single calls are tested at, noise and photo-like, and (index 4) an image on which the reference panics"""
    imgs = [Z.noise(1, 1), np.zeros((5, 0, 3), np.uint8), Z.photo_like(1, 300), Z.noise(64, 48), Z.flat(100, 100), Z.photo_like(64, 48),
            Z.noise(320, 240), Z.photo_like(320, 240), Z.noise(1, 300)]
    for im in imgs:
        im.setflags(write=False)
    return imgs


PANICS_AT = 4
_want = {}


def singles(ctx, clib):
    """per image: (stream, row) of the three single calls, None where the encode is refused -- computed once, never changed"""
    if "rows" not in _want:
        _lib = L()
        rows = []
        for f, im in enumerate(folder()):
            rc, data = ctx.zip_back_image_encode(im, allow=(_lib.UNSUPPORTED,))
            ref = Z.codec_encode(lambda d: Z.encode_c(clib, d), im)
            if rc != _lib.OK:
                assert f == PANICS_AT and rc == _lib.UNSUPPORTED and ref == Z.PANICS
                _want["message"] = last_error(ctx)
                rows.append((None, rc))
                continue
            assert data == ref, f
            rc, back = ctx.zip_back_image_decode(data)
            assert rc == _lib.OK and np.array_equal(back, im), f
            npx = im.shape[0] * im.shape[1]
            ratio = len(data) / (npx * 24.0) * 100.0 if npx else math.inf      # (bench.rs:43 in floating point: x / 0 is infinite)
            rows.append((data, dict(compressed_size=len(data), compression_ratio=ratio, error=ctx.mse(im, back), rc=0)))
        _want["rows"] = rows
    return _want["rows"]


def last_error(ctx):
    return (ctx._L.cniic_last_error(ctx.h) or b"").decode()


def pack(imgs, pad=0):
    offs, at = [], 0
    for i, im in enumerate(imgs):
        at += (i * 5) % 3 if pad else 0     # any alignment
        offs.append(at)
        at += im.size
    buf = np.zeros(at + 1, np.uint8)
    for o, im in zip(offs, imgs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def check_rows(want, rc, rows, lens, out, stride, short=()):
    _lib = L()
    assert rc == _lib.UNSUPPORTED                       # the first failure, lowest f: frames `short` come behind it
    host = None if out is None else out.cpu().numpy() if hasattr(out, "cpu") else out
    for f, (data, row) in enumerate(want):
        if data is None:
            assert rows[f]["rc"] == row == _lib.UNSUPPORTED and rows[f]["compressed_size"] == 0 and lens[f] == 0
            assert math.isnan(rows[f]["compression_ratio"]) and math.isnan(rows[f]["error"])
            continue
        exp = dict(row, rc=_lib.CAPACITY) if f in short else row
        assert all(same(rows[f][k], exp[k]) for k in COLUMNS), (f, rows[f], exp)
        assert rows[f]["lossless_mismatch"] == 0 and rows[f]["error"] == 0.0 and rows[f]["kmeans"]["iterations"] == 0
        if host is None:
            continue
        assert lens[f] == len(data), f
        if f not in short:
            assert host[f * stride:f * stride + lens[f]].tobytes() == data, f


def test_symbol_and_prototype():
    _lib = L()
    assert "cniic_zip_back_image_measure_batch" in _lib.PROTOTYPES
    assert hasattr(_lib.lib(), "cniic_zip_back_image_measure_batch")


@pytest.mark.parametrize("images_on_device", [False, True])
@pytest.mark.parametrize("out_on", ["none", "host", "device"])
def test_rows_are_the_three_single_calls(ctx, clib, images_on_device, out_on):
    import torch
    want = singles(ctx, clib)
    imgs = folder()
    buf, offs, ws, hs = pack(imgs, pad=1)
    src = torch.from_numpy(buf).cuda() if images_on_device else buf
    stride = max(len(d) for d, _ in want if d is not None) + 3
    out = None if out_on == "none" else np.full(stride * len(imgs), 0xA5, np.uint8)
    if out_on == "device":
        out = torch.from_numpy(out).cuda()
    rc, rows, lens = ctx.zip_back_measure_batch(src, offs, ws, hs, out, stride if out is not None else 0, allow=(L().UNSUPPORTED,))
    check_rows(want, rc, rows, lens, out, stride)
    assert last_error(ctx) == _want["message"] and "back.rs:45" in _want["message"]      # the refused frame's own message
    if out is not None:                                 # nothing is written behind a stream, nor into the refused frame's slot
        host = out.cpu().numpy() if out_on == "device" else out
        for f, (d, _) in enumerate(want):
            n = 0 if d is None else len(d)
            assert (host[f * stride + n:(f + 1) * stride] == 0xA5).all(), f


def test_a_stride_one_byte_short(ctx, clib):
    """the largest stream does not fit: its row says CAPACITY with its measurements and lens = the bytes needed; the others are as before"""
    want = singles(ctx, clib)
    imgs = folder()
    largest = max((f for f, (d, _) in enumerate(want) if d is not None), key=lambda f: len(want[f][0]))
    stride = len(want[largest][0]) - 1
    assert sum(len(d) > stride for d, _ in want if d is not None) == 1
    buf, offs, ws, hs = pack(imgs)
    out = np.full(stride * len(imgs), 0xA5, np.uint8)
    rc, rows, lens = ctx.zip_back_measure_batch(buf, offs, ws, hs, out, stride, allow=(L().UNSUPPORTED, L().CAPACITY))
    check_rows(want, rc, rows, lens, out, stride, short=(largest,))
    assert (out[largest * stride:(largest + 1) * stride] == 0xA5).all()


@pytest.mark.parametrize("images_on_device", [False, True])
def test_a_frame_per_chunk(ctx, clib, monkeypatch, images_on_device):
    """CNIIC_TEST_MEASURE_BUDGET=1: every image is a chunk of its own ("zb_encode" counts one launch per chunk of images this small)"""
    import torch
    _lib = L()
    keep = [f for f, im in enumerate(folder()) if im.size < 100000]      # (the two 320 x 240 images are encoded by the tests above)
    want = [singles(ctx, clib)[f] for f in keep]
    imgs = [folder()[f] for f in keep]
    assert len(imgs) == 7 and want[PANICS_AT][0] is None
    buf, offs, ws, hs = pack(imgs, pad=1)
    src = torch.from_numpy(buf).cuda() if images_on_device else buf
    stride = max(len(d) for d, _ in want if d is not None)
    out = np.zeros(stride * len(imgs), np.uint8)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, rows, lens = ctx.zip_back_measure_batch(src, offs, ws, hs, out, stride, allow=(_lib.UNSUPPORTED,))
        together = ctx.kernel_time("zb_encode")[1]
        monkeypatch.setenv(BUDGET, "1")
        rc1, rows1, lens1 = ctx.zip_back_measure_batch(src, offs, ws, hs, out, stride, allow=(_lib.UNSUPPORTED,))
        alone = ctx.kernel_time("zb_encode")[1]
        monkeypatch.delenv(BUDGET)
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    check_rows(want, rc, rows, lens, out, stride)
    check_rows(want, rc1, rows1, lens1, out, stride)
    assert together == 1 and alone == len(imgs)         # every text is below one slice of 256 KiB: a launch a chunk


def test_no_frames_and_null_arguments(ctx):
    _lib = L()
    assert ctx.zip_back_measure_batch(np.zeros(1, np.uint8), [], [], []) == (0, [], [])
    rc, rows, lens = ctx.zip_back_measure_batch(None, [0], [2], [2], allow=(_lib.BAD_ARG,))
    assert rc == _lib.BAD_ARG


def test_the_class_measures_in_one_call(ctx, clib):
    import cniic_amd
    _lib = L()
    want = singles(ctx, clib)
    imgs = folder()
    codec = cniic_amd.ZipBack(ctx)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rows = codec.measure(imgs[:6])
        launches = ctx.kernel_time("zb_encode")[1]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    assert launches == 1                                # six images, one launch: one call
    for f in range(6):
        data, row = want[f]
        if data is None:
            assert rows[f]["rc"] == _lib.UNSUPPORTED and math.isnan(rows[f]["error"]) and rows[f]["compressed_size"] == 0
        else:
            assert all(same(rows[f][k], row[k]) for k in COLUMNS), (f, rows[f], row)
    assert codec.measure([]) == []
    assert codec.measure(imgs[2:4], seed=7, max_iters=3, flags=0)[1]["compressed_size"] == want[3][1]["compressed_size"]   # (Codec.measure's options: taken)
    with pytest.raises(ValueError):
        codec.measure([np.zeros((4, 4), np.uint8)])


def test_the_harness_writes_zip_back_csv_in_a_loop_and_in_one_call(ctx, tmp_path):
    """tools/cniic_bench takes the reference's spelling itself (the library's parser rejects it) and writes the Makefile's zip-back.csv:
    the CSV rows are the rows of the Python call on the same synthetic images"""
    import cniic_amd
    from cniic_amd import synth
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "cniic_bench")
    assert os.path.exists(exe), "tools/cniic_bench is built by `make -C cniic_amd/csrc`"
    specs = [("P", 96, 64, 1), ("U", 40, 33, 2), ("P", 200, 120, 3)]
    names = ["synth:%s:%dx%d:%d" % s for s in specs]
    imgs = [(synth.photo if k == "P" else synth.uniform)(w, h, synth.SEED0 + off) for k, w, h, off in specs]
    rows = cniic_amd.ZipBack(ctx).measure(imgs)
    assert all(r["rc"] == 0 and r["error"] == 0.0 for r in rows)
    want = ["%s,%d,%s,%s" % (n, r["compressed_size"], repr(r["compression_ratio"]), repr(r["error"])) for n, r in zip(names, rows)]
    r = subprocess.run([exe, "--codec=zip(back)"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    loop = open(tmp_path / "output" / "zip-back.csv").read().strip().split("\n")
    r = subprocess.run([exe, "--codec=zip(back)", "--one-call"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    one = open(tmp_path / "output" / "zip-back.csv").read().strip().split("\n")
    assert one[0] == loop[0] == "name,compressed_size,compression_ratio,error"
    assert [l.split(",")[0] for l in one[1:]] == names and sorted(one[1:]) == sorted(loop[1:])

    def parsed(lines):
        return [(l.split(",")[0], int(l.split(",")[1]), float(l.split(",")[2]), float(l.split(",")[3])) for l in lines]
    assert parsed(one[1:]) == parsed(want)
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "zip(back)" in r.stderr
