"""cniic_frames_from_surfaces / cniic_frames_to_surfaces on the GPU, through the C ABI: every comparison is exact, against tests/surface_ref.py.
Sources are random bytes with fixed seeds; every byte around and between the frames, and every padding byte of an export, is 0xA5 before
the call and checked afterwards (the whole written buffer is compared, not the frames alone).  Buffers are sized by cniic_surface_span."""
import ctypes as C

import numpy as np
import pytest

import surface_ref as R
from cniic_amd import _lib
from cniic_amd._lib import PX_BGR8, PX_BGRA8, PX_L8, PX_LA8, PX_NV12, PX_RGB8, PX_RGBA8, Surface

pytestmark = pytest.mark.gpu

FORMATS = (PX_L8, PX_LA8, PX_RGB8, PX_RGBA8, PX_BGR8, PX_BGRA8)
WRITABLE = (PX_RGB8, PX_BGR8, PX_RGBA8, PX_BGRA8)
SHAPES = [(1, 1), (2, 3), (5, 1), (15, 2), (16, 2), (17, 3), (21, 5), (22, 4), (63, 2), (64, 3), (65, 2), (257, 3)]
PADS, RESIDUES = (0, 1, 5, 16), (0, 1, 4, 15)


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


def _dev(a):
    import torch
    t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _host(ctx, t):
    ctx.sync()
    return t.cpu().numpy()


def _import(ctx, L, src, timers=False):
    """-> the whole packed buffer after the call (poison before it)"""
    out = _dev(np.full(L.rgb_bytes, R.POISON, np.uint8))
    if timers:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        assert ctx.frames_from_surfaces(_dev(src), L.surfaces, out, L.img_off) == 0
        if timers:
            assert ctx.kernel_time("surf_import")[1] == 1
    finally:
        if timers:
            ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    return _host(ctx, out)


def _grid(formats):
    L = R.Layout(guard=16)
    for fmt in formats:
        for w, h in SHAPES:
            for pad in PADS:
                for rs in RESIDUES:
                    for rd in RESIDUES:
                        L.add(fmt, w, h, pad=pad, src_res=rs, rgb_res=rd)
    return L


@pytest.fixture(scope="module")
def grid():
    """test 1's 4608 frames, their source and what the import must give: computed once, left unchanged"""
    L = _grid(FORMATS)
    assert len(L.surfaces) == 4608
    src = L.random_source(1)
    want = L.expected_import(src)
    src.setflags(write=False)
    want.setflags(write=False)
    return L, src, want


def test_every_format_at_the_shapes_where_the_split_can_go_wrong_in_one_call(ctx, grid):
    L, src, want = grid
    got = _import(ctx, L, src, timers=True)
    assert np.array_equal(got, want), "first difference at byte %d" % int(np.flatnonzero(got != want)[0])


def test_frames_of_several_chunks_and_rows_longer_than_a_chunk(ctx):
    L = R.Layout()
    L.add(PX_RGBA8, 700, 50, pad=12, src_res=0, rgb_res=3)
    L.add(PX_L8, 3, 9000, pad=0, src_res=7, rgb_res=0)
    L.add(PX_BGR8, 9000, 3, pad=2, src_res=1, rgb_res=15)
    L.add(PX_RGB8, 40000, 1, pad=0, src_res=9, rgb_res=6)
    src = L.random_source(2)
    got, want = _import(ctx, L, src, timers=True), L.expected_import(src)
    assert np.array_equal(got, want), "first difference at byte %d" % int(np.flatnonzero(got != want)[0])


def test_the_pan_eight_windows_on_one_image(ctx):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    L, surfaces, offs, at = R.Layout(), [], [], 16
    for i in range(8):
        x, y = 8 * i, 4 * i
        surfaces.append(Surface(off=(y * 256 + x) * 3, pitch=256 * 3, w=96, h=54, format=PX_RGB8))
        assert R.span(surfaces[-1])[0] <= img.size
        offs.append(at)
        at += 96 * 54 * 3 + 16
    L.surfaces, L.img_off, L.rgb_bytes = surfaces, offs, at
    got = _import(ctx, L, img.reshape(-1), timers=True)
    want = np.full(at, R.POISON, np.uint8)
    for i in range(8):
        want[offs[i]:offs[i] + 96 * 54 * 3] = img[4 * i:4 * i + 54, 8 * i:8 * i + 96].ravel()
    assert np.array_equal(got, want)


NV12_SIZES = [(1, 1), (2, 2), (3, 3), (5, 4), (16, 2), (17, 17), (66, 5), (130, 3)]


def test_nv12_all_matrices_paddings_and_plane_offsets(ctx):
    L = R.Layout()
    for matrix in R.MATRICES:
        for w, h in NV12_SIZES:
            for pad in (0, 3):
                for pad_uv in (0, 3):
                    for res in (0, 1, 15):
                        L.add(PX_NV12, w, h, pad=pad, pad_uv=pad_uv, src_res=res, uv_res=(res * 7 + pad) % 16 if res else 0, rgb_res=(res + 2 * pad) % 16, matrix=matrix)
    # the cross product of the CPU test, once per matrix and plane residue
    Y, UV = R.nv12_cross_product()
    cross = []
    for matrix in R.MATRICES:
        for res in (0, 1, 15):
            cross.append(L.add(PX_NV12, 50, 6, pad=1, pad_uv=2, src_res=res, uv_res=15 - res, rgb_res=res, matrix=matrix))
    src = L.random_source(4)
    for s in cross:
        src[R.rows(src, s.off, s.pitch, 50, 6)] = Y
        src[R.rows(src, s.off_uv, s.pitch_uv, 50, 3)] = UV
    got, want = _import(ctx, L, src, timers=True), L.expected_import(src)
    assert np.array_equal(got, want), "first difference at byte %d" % int(np.flatnonzero(got != want)[0])
    for s, o in zip(L.surfaces, L.img_off):   # both ends of the clip are in what was compared
        if s in cross:
            px = want[o:o + 900]
            assert px.min() == 0 and px.max() == 255


@pytest.fixture(scope="module")
def export_grid():
    L = _grid(WRITABLE)
    assert len(L.surfaces) == 3072
    rgb = L.random_frames(5)
    rgb.setflags(write=False)
    return L, rgb


def _export(ctx, L, rgb, alpha, allow=()):
    dst = _dev(np.full(L.src_bytes, R.POISON, np.uint8))
    rc = ctx.frames_to_surfaces(_dev(rgb), L.img_off, L.surfaces, dst, alpha=alpha, allow=allow)
    return rc, _host(ctx, dst)


@pytest.mark.parametrize("alpha", [0, 7, 255])
def test_export_leaves_padding_and_guards_alone_and_import_brings_it_back(ctx, export_grid, alpha):
    L, rgb = export_grid
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        rc, got = _export(ctx, L, rgb, alpha)
        assert rc == 0 and ctx.kernel_time("surf_export")[1] == 1
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    want = L.expected_export(rgb, alpha)
    assert np.array_equal(got, want), "first difference at byte %d" % int(np.flatnonzero(got != want)[0])
    assert np.array_equal(_import(ctx, L, got), rgb)   # import(export(x)) == x, the guards between the frames included


def test_export_refuses_grey_nv12_and_an_alpha_that_is_no_byte(ctx):
    for fmt, alpha in ((PX_L8, 255), (PX_LA8, 255), (PX_NV12, 255), (PX_RGBA8, 256), (PX_RGB8, 1 << 31)):
        L = R.Layout()
        L.add(PX_RGBA8, 33, 5, pad=4)
        L.add(fmt, 20, 4, pad=1, matrix=_lib.YUV_601_FULL)
        L.add(PX_BGR8, 7, 7)
        rc, got = _export(ctx, L, L.random_frames(6), alpha, allow=(_lib.BAD_ARG,))
        assert rc == _lib.BAD_ARG and (got == R.POISON).all(), (fmt, alpha)


def test_every_refusal_through_the_calls_one_bad_descriptor_among_good_ones(ctx):
    import test_surfaces_cpu as T
    L = R.Layout()
    for fmt, w, h in ((PX_RGBA8, 40, 9), (PX_L8, 17, 3), (PX_BGR8, 5, 5)):
        L.add(fmt, w, h, pad=3, src_res=1, rgb_res=5)
    src = L.random_source(7)
    src_d, rgb_d = _dev(src), _dev(L.random_frames(8))
    for desc in T.BAD:
        surfaces = L.surfaces[:2] + [Surface(**desc)] + L.surfaces[2:]
        offs = L.img_off[:2] + [L.rgb_bytes] + L.img_off[2:]
        out = _dev(np.full(L.rgb_bytes + 64, R.POISON, np.uint8))
        assert ctx.frames_from_surfaces(src_d, surfaces, out, offs, allow=(_lib.BAD_ARG,)) == _lib.BAD_ARG, desc
        assert (_host(ctx, out) == R.POISON).all(), desc
        if desc.get("format") in R.PX_BYTES and desc["format"] not in WRITABLE:
            continue   # (an export of these is refused for the format already: test above)
        writable = [s for s in L.surfaces if s.format in WRITABLE]
        dst = _dev(np.full(L.src_bytes, R.POISON, np.uint8))
        rc = ctx.frames_to_surfaces(rgb_d, offs[:1] + offs[2:3] + offs[3:4], writable[:1] + [Surface(**desc)] + writable[1:], dst, allow=(_lib.BAD_ARG,))
        assert rc == _lib.BAD_ARG and (_host(ctx, dst) == R.POISON).all(), desc
    # a frame that ends behind 2^64, null arguments, and no frames at all
    out = _dev(np.full(L.rgb_bytes, R.POISON, np.uint8))
    assert ctx.frames_from_surfaces(src_d, L.surfaces, out, L.img_off[:2] + [(1 << 64) - 10], allow=(_lib.BAD_ARG,)) == _lib.BAD_ARG
    n = len(L.surfaces)
    arr, off = (Surface * n)(*L.surfaces), (C.c_uint64 * n)(*L.img_off)
    lib, h = _lib.lib(), ctx.h
    for args in ((None, arr, n, out.data_ptr(), off), (src_d.data_ptr(), None, n, out.data_ptr(), off), (src_d.data_ptr(), arr, n, None, off),
                 (src_d.data_ptr(), arr, n, out.data_ptr(), None)):
        assert lib.cniic_frames_from_surfaces(h, *args) == _lib.BAD_ARG
    assert lib.cniic_frames_from_surfaces(None, src_d.data_ptr(), arr, n, out.data_ptr(), off) == _lib.BAD_ARG
    dst = _dev(np.full(L.src_bytes, R.POISON, np.uint8))
    for args in ((None, off, arr, n, dst.data_ptr(), 255), (rgb_d.data_ptr(), None, arr, n, dst.data_ptr(), 255), (rgb_d.data_ptr(), off, None, n, dst.data_ptr(), 255),
                 (rgb_d.data_ptr(), off, arr, n, None, 255)):
        assert lib.cniic_frames_to_surfaces(h, *args) == _lib.BAD_ARG
    assert lib.cniic_frames_from_surfaces(h, None, None, 0, None, None) == 0 and lib.cniic_frames_to_surfaces(h, None, None, None, 0, None, 0) == 0
    assert (_host(ctx, out) == R.POISON).all() and (_host(ctx, dst) == R.POISON).all()


def test_host_memory_on_either_side_gives_the_bytes_of_the_device_call(ctx, grid):
    G, _, _ = grid
    L = R.Layout()
    for i, s in enumerate(G.surfaces[::37]):   # 125 of test 1's frames, every format, shape, padding and residue among them
        L.add(s.format, s.w, s.h, pad=s.pitch - s.w * R.PX_BYTES[s.format], src_res=s.off % 16, rgb_res=G.img_off[37 * i] % 16)
    L.add(PX_NV12, 33, 7, pad=5, pad_uv=1, src_res=3, uv_res=9, rgb_res=2, matrix=_lib.YUV_709_LIMITED)
    src = L.random_source(9)
    want = L.expected_import(src)
    assert np.array_equal(_import(ctx, L, src), want)
    for src_host, rgb_host in ((True, False), (False, True), (True, True)):
        out = np.full(L.rgb_bytes, R.POISON, np.uint8)
        out_arg = out if rgb_host else _dev(out)
        assert ctx.frames_from_surfaces(src if src_host else _dev(src), L.surfaces, out_arg, L.img_off) == 0
        assert np.array_equal(out if rgb_host else _host(ctx, out_arg), want), (src_host, rgb_host)
    E = R.Layout()
    for s in L.surfaces:
        if s.format in WRITABLE:
            E.add(s.format, s.w, s.h, pad=s.pitch - s.w * R.PX_BYTES[s.format], src_res=s.off % 16, rgb_res=s.w % 16)
    rgb = E.random_frames(10)
    want = E.expected_export(rgb, 9)
    assert np.array_equal(_export(ctx, E, rgb, 9)[1], want)
    for rgb_host, dst_host in ((True, False), (False, True), (True, True)):
        dst = np.full(E.src_bytes, R.POISON, np.uint8)
        dst_arg = dst if dst_host else _dev(dst)
        assert ctx.frames_to_surfaces(rgb if rgb_host else _dev(rgb), E.img_off, E.surfaces, dst_arg, alpha=9) == 0
        assert np.array_equal(dst if dst_host else _host(ctx, dst_arg), want), (rgb_host, dst_host)


@pytest.mark.parametrize("expr", ["delta", "cluster-colors(16)"])
def test_imported_frames_feed_encode_batch_var(ctx, expr):
    import torch
    from cniic_amd import synth
    sizes = [(33, 17), (64, 64), (5, 70)]
    L = R.Layout()
    for i, (w, h) in enumerate(sizes):
        L.add(PX_RGBA8, w, h, pad=4 * i, src_res=4 * i, rgb_res=(5 * i) % 16)
    src = L.random_source(11)
    imgs = []
    for i, (s, (w, h)) in enumerate(zip(L.surfaces, sizes)):   # photographs, not noise: the K-means has something to cluster
        im = synth.photo(w, h, synth.SEED0 + 9100 + i)
        imgs.append(im)
        src[R.rows(src, s.off, s.pitch, 4 * w, h)] = np.concatenate([im, np.full((h, w, 1), 200 + i, np.uint8)], axis=2).reshape(h, 4 * w)
    packed = np.full(L.rgb_bytes, R.POISON, np.uint8)
    for im, o in zip(imgs, L.img_off):
        packed[o:o + im.size] = im.ravel()
    assert np.array_equal(L.expected_import(src), packed)
    ws, hs, stride = [w for w, _ in sizes], [h for _, h in sizes], 1 << 16
    rgb = _dev(np.full(L.rgb_bytes, R.POISON, np.uint8))
    src_d = _dev(src)   # (kept alive: the call below returns before its kernel has run)
    assert ctx.frames_from_surfaces(src_d, L.surfaces, rgb, L.img_off) == 0     # (no sync: the encode is ordered behind it)
    streams = []
    for images in (rgb, _dev(packed)):
        out = torch.zeros(stride * 3, dtype=torch.uint8, device=rgb.device)
        rc, lens, rcs, _ = ctx.encode_batch_var(expr, images, L.img_off, ws, hs, out, stride)
        assert rc == 0 and rcs == [0, 0, 0]
        host = _host(ctx, out)
        streams.append([host[f * stride:f * stride + lens[f]].tobytes() for f in range(3)])
    assert streams[0] == streams[1]
