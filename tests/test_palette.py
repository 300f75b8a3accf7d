"""Frozen palettes (cniic_cc_palette, cniic_palette_*): the colour -> label table of k_palette.hip and the streams coded through it.

The yardstick is numpy plus the oracle, never the code under test:
    label(p)        = np.argmin over the int32 squared distances to the K entries (the first minimum = the lowest index among equals)
    expected(frame) = oracle_lib.encode("hufman", remapped), remapped[p] = palette[label(p)] -- ClusterColors::encode ends in Hufman.encode of
                      the reduced image (clusterc.rs:52), so this is the reference's stream for that assignment.

CELL = 16 is kPalCellSide of cniic_amd/csrc/pal_bounds.hpp: one workgroup builds the table entries of one 16^3 cell of the colour cube."""
import ctypes as C_
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_dist import keys_of  # noqa: E402
from test_frames_var import C as CHUNK, RAGGED, flat_bytes, new_ctx, oracle, ragged_frames  # noqa: E402

pytestmark = pytest.mark.gpu

CELL = 16


# ------------------------------------------------------------------ the yardstick
def np_labels(px, pal):
    """px: (n, 3) uint8, pal: (K, 3) uint8 -> (n,) the lowest index of a nearest entry.  The squared distances are int32; the products behind
    them go through a float32 matrix product, which is exact here (every partial sum is an integer below 2^24)."""
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    pf = pal.astype(np.float32)
    pn = (pal.astype(np.int32) ** 2).sum(1)
    out = np.empty(px.shape[0], np.int64)
    step = max(1, (1 << 26) // max(pal.shape[0], 16))
    for a in range(0, px.shape[0], step):
        c = px[a:a + step]
        dot = (c.astype(np.float32) @ pf.T).astype(np.int32)
        d = (c.astype(np.int32) ** 2).sum(1)[:, None] - 2 * dot + pn[None, :]
        out[a:a + step] = np.argmin(d, axis=1)
    return out


def test_the_yardstick_itself_on_a_brute_force_sample():
    rng = np.random.default_rng(5)
    pal = rng.integers(0, 256, size=(37, 3), dtype=np.uint8)
    pal[7] = pal[3]
    px = np.concatenate([rng.integers(0, 256, size=(500, 3), dtype=np.uint8), pal])
    want = [min(range(37), key=lambda k: (sum((int(a) - int(b)) ** 2 for a, b in zip(p, pal[k])), k)) for p in px]
    assert np_labels(px, pal).tolist() == want


def expected(frame, pal):
    import oracle_lib as O
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    remapped = pal[np_labels(frame.reshape(-1, 3), pal)].reshape(frame.shape)
    rc, data, _ = O.encode("hufman", remapped)
    assert rc == 0
    return data, remapped


_cube = {}


def cube():
    """the 4096 x 4096 image that holds every colour once, in key order (host array; its device copy is made per context)"""
    if "px" not in _cube:
        k = np.arange(1 << 24, dtype=np.uint32)
        px = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], 1).astype(np.uint8)
        px.setflags(write=False)
        _cube["px"] = px
    return _cube["px"]


def face_subset():
    """every 97th colour, plus all colours with a coordinate within one step of a cell face (the last of one cell or the first of the next)"""
    if "sub" not in _cube:
        px = cube()
        near = ((px % CELL == 0) | (px % CELL == CELL - 1)).any(1)
        near[::97] = True
        _cube["sub"] = np.nonzero(near)[0]
    return _cube["sub"]


def tie_palettes():
    """(name, (K, 3) palette) for K = 1, 2, 3, 16: random ones and the tie cases"""
    rng = np.random.default_rng(20261018)
    out = [("random-%d" % K, rng.integers(0, 256, size=(K, 3), dtype=np.uint8)) for K in (1, 2, 3, 16)]
    out.append(("tie-0-2", np.array([(0, 0, 0), (2, 0, 0)], np.uint8)))        # colour (1, 0, 0) is equidistant: label 0
    out.append(("tie-2-0", np.array([(2, 0, 0), (0, 0, 0)], np.uint8)))        # ... and label 0 again
    out.append(("equal-3", np.tile(np.array([(90, 200, 17)], np.uint8), (3, 1))))
    mirrored = []
    for i in range(8):   # pairs mirrored about a cell face: 15 | 16, 31 | 32, ... on one axis; the higher side first in every other pair
        face, axis = CELL * (1 + 2 * i), i % 3
        lo = [int(x) for x in rng.integers(0, 256, size=3)]
        hi = list(lo)
        lo[axis], hi[axis] = face - 1, face
        mirrored += [hi, lo] if i & 1 else [lo, hi]
    out.append(("mirrored-16", np.array(mirrored, np.uint8)))
    out.append(("corners-16", (CELL * rng.integers(0, 256 // CELL, size=(16, 3)) + (CELL - 1) * rng.integers(0, 2, size=(16, 3))).astype(np.uint8)))
    out.append(("cluster-16", (np.array([250, 3, 128]) + rng.integers(0, 5, size=(16, 3))).astype(np.uint8)))
    return out


def timed_ctx():
    from cniic_amd import _lib
    ctx, dev = new_ctx()
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    return ctx, dev


def table_of(ctx, dev, pal):
    """-> (labels of the whole cube through cniic_palette_labels as a numpy array, cells that took the plain route)"""
    import torch
    import cniic_amd
    p = cniic_amd.Palette.create(ctx, pal)
    plain = ctx.kernel_time("pal_lut_plain")[1]
    assert ctx.kernel_time("pal_lut")[1] == 1
    try:
        assert p.label_bytes == (1 if len(pal) <= 256 else 2)
        t = torch.from_numpy(cube()).to(dev)
        out = torch.empty(1 << 24, dtype=torch.uint8 if p.label_bytes == 1 else torch.int16, device=dev)
        torch.cuda.synchronize(dev)
        p.labels(t, 1 << 24, out)
        ctx.sync()
        lab = out.cpu().numpy()
    finally:
        p.close()
    return (lab if lab.dtype == np.uint8 else lab.view(np.uint16)), plain


def wide_palettes():
    rng = np.random.default_rng(257)
    return {K: rng.integers(0, 256, size=(K, 3), dtype=np.uint8) for K in (256, 257)}


# ------------------------------------------------------------------ test 1: the whole table
@pytest.mark.parametrize("name,pal", tie_palettes(), ids=[n for n, _ in tie_palettes()])
def test_whole_table_small_palettes(name, pal):
    ctx, dev = timed_ctx()
    got, plain = table_of(ctx, dev, pal)
    ctx.close()
    assert plain == 0
    want = np_labels(cube(), pal)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d colours differ, first %06x: %d, numpy %d" % (name, bad.size, bad[0], got[bad[0]], want[bad[0]])
    if name.startswith("tie-"):
        assert got[0x010000] == 0


@pytest.mark.parametrize("K", [256, 257])
def test_whole_table_large_palettes_on_the_face_subset(K):
    sub = face_subset()
    assert sub.size >= 1 << 18
    pal = wide_palettes()[K]
    ctx, dev = timed_ctx()
    got, plain = table_of(ctx, dev, pal)
    ctx.close()
    assert plain == 0
    assert got.dtype == (np.uint8 if K == 256 else np.uint16)
    want = np_labels(cube()[sub], pal)
    bad = np.nonzero(got[sub] != want)[0]
    assert bad.size == 0, "K = %d: %d colours differ, first %06x" % (K, bad.size, sub[bad[0]])


# ------------------------------------------------------------------ test 2: the plain route
@pytest.mark.parametrize("K", [16, 257])
def test_plain_route_with_a_lowered_budget(monkeypatch, K):
    monkeypatch.setenv("CNIIC_TEST_PAL_LIST_MAX", "4")
    pal = wide_palettes()[257] if K == 257 else tie_palettes()[3][1]
    assert len(pal) == K
    ctx, dev = timed_ctx()
    got, plain = table_of(ctx, dev, pal)
    ctx.close()
    assert plain > 0
    idx = np.arange(1 << 24) if K == 16 else face_subset()
    assert np.array_equal(got[idx], np_labels(cube()[idx], pal))


def test_plain_route_of_many_equal_entries():
    pal = np.tile(np.array([(12, 250, 99)], np.uint8), (5000, 1))
    ctx, dev = timed_ctx()
    got, plain = table_of(ctx, dev, pal)
    ctx.close()
    assert plain > 0 and got.dtype == np.uint16
    assert not got.any()


# ------------------------------------------------------------------ test 3: ragged frames equal the yardstick
def sampled_palette(frames, K, seed):
    px = np.concatenate([f.reshape(-1, 3) for f in frames])
    return px[np.random.default_rng(seed).choice(px.shape[0], K, replace=False)].copy()


def encode_with(ctx, dev, pal, frames, host=False, stride=None):
    """-> (streams, lengths, raw output as a numpy array, stride) through Palette.encode_frames_var"""
    import torch
    import cniic_amd
    ws, hs = [f.shape[1] for f in frames], [f.shape[0] for f in frames]
    if stride is None:
        stride = (max(w * h for w, h in zip(ws, hs)) * 4 + 8192 + 3) & ~3
    flat = flat_bytes(frames)
    own = not isinstance(pal, cniic_amd.Palette)
    p = cniic_amd.Palette.create(ctx, pal) if own else pal
    try:
        if host:
            out = np.zeros(stride * len(frames), np.uint8)
            lens = p.encode_frames_var(flat, ws, hs, out, stride)
            raw = out
        else:
            out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            lens = p.encode_frames_var(torch.from_numpy(flat).to(dev), ws, hs, out, stride)
            ctx.sync()
            raw = out.cpu().numpy()
    finally:
        if own:
            p.close()
    return [bytes(raw[f * stride:f * stride + lens[f]].tobytes()) for f in range(len(frames))], lens, raw, stride


def decode_all(ctx, dev, K, raw, stride, lens, frames):
    """the streams through cniic_codec_decode_batch -> (list of images, the device tensor they lie in, offsets)"""
    import torch
    F = len(frames)
    img_stride = max(f.size for f in frames)
    out = torch.zeros(img_stride * F, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rc, ws, hs, rcs = ctx.decode_batch("cluster-colors(%d)" % K, torch.from_numpy(raw).to(dev), stride, lens, F, out, img_stride)
    ctx.sync()
    assert rc == 0 and not any(rcs)
    host = out.cpu().numpy()
    imgs = [host[f * img_stride:f * img_stride + frames[f].size].reshape(frames[f].shape) for f in range(F)]
    assert [(w, h) for w, h in zip(ws, hs)] == [(f.shape[1], f.shape[0]) for f in frames]
    return imgs, out, [f * img_stride for f in range(F)]


_exp16 = {}


def ragged_expected():
    """K = 16 over the ragged list: (palette, [(stream, remapped frame)]) -- computed once, shared"""
    if not _exp16:
        frames, _ = ragged_frames()
        pal = sampled_palette(frames, 16, 16)
        _exp16["pal"], _exp16["exp"] = pal, [expected(f, pal) for f in frames]
    return _exp16["pal"], _exp16["exp"]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("trees", ["gpu", "host"])
def test_ragged_frames_equal_the_yardstick(monkeypatch, trees, host):
    if trees == "host":
        monkeypatch.setenv("CNIIC_FRAME_TREES_HOST", "1")
    else:
        monkeypatch.delenv("CNIIC_FRAME_TREES_HOST", raising=False)
    frames, _ = ragged_frames()
    pal, exp = ragged_expected()
    ctx, dev = new_ctx()
    got, lens, raw, stride = encode_with(ctx, dev, pal, frames, host=host)
    for f, (w, h) in enumerate(RAGGED):
        assert got[f] == exp[f][0], "frame %d (%d x %d) differs from the yardstick's stream" % (f, w, h)
    imgs, _, _ = decode_all(ctx, dev, 16, raw, stride, lens, frames)
    ctx.close()
    for f in range(len(frames)):
        assert np.array_equal(imgs[f], exp[f][1]), "frame %d does not decode to the remapped frame" % f


def test_ragged_frames_wide_labels():
    K = 300
    frames, _ = ragged_frames()
    pal = sampled_palette(frames, K, 300)
    ctx, dev = new_ctx()
    got, lens, raw, stride = encode_with(ctx, dev, pal, frames)
    ctx.close()
    for f in range(len(frames)):
        assert got[f] == expected(frames[f], pal)[0], "frame %d" % f


# ------------------------------------------------------------------ test 4: degenerate alphabets
def test_degenerate_alphabets():
    from cniic_amd import synth
    rng = np.random.default_rng(4)
    pal = rng.integers(0, 256, size=(16, 3), dtype=np.uint8)
    pal[5], pal[11] = (200, 200, 200), (250, 10, 40)
    pal[0] = (0, 0, 0)
    flat = np.full((7, 9, 3), 200, np.uint8)
    two = np.zeros((11, 23, 3), np.uint8); two[:, 8:] = (250, 10, 40)
    frames = [synth.photo(37, 29, synth.SEED0 + 931), flat, two, synth.photo(CHUNK + 5, 1, synth.SEED0 + 932)]
    ctx, dev = new_ctx()
    got, _, _, _ = encode_with(ctx, dev, pal, frames)
    exp = [expected(f, pal)[0] for f in frames]
    assert len(exp[1]) == 8 + 12                                     # dimensions and one leaf
    assert len(exp[2]) == 8 + 1 + 2 * 12 + (11 * 23 + 7) // 8        # two leaves, one bit per pixel
    assert got == exp
    # duplicated entries: both copies' pixels end up under the lower index, and the stream has ONE leaf for the colour
    dup = pal.copy()
    dup[9] = dup[5]; dup[2] = dup[11]
    import cniic_amd
    p = cniic_amd.Palette.create(ctx, dup)
    lab = p.labels(np.concatenate([flat.reshape(-1, 3), two.reshape(-1, 3)]))
    p.close()
    assert set(lab[:63].tolist()) == {5} and set(lab[63:].tolist()) == {0, 2}
    got, _, _, _ = encode_with(ctx, dev, dup, frames)
    assert got == [expected(f, dup)[0] for f in frames] and len(got[1]) == 8 + 12 and len(got[2]) == len(exp[2])
    # K = 1: every frame is one leaf
    one = np.array([(17, 99, 203)], np.uint8)
    got, _, _, _ = encode_with(ctx, dev, one, frames)
    ctx.close()
    assert got == [expected(f, one)[0] for f in frames] and all(len(g) == 8 + 12 for g in got)


# ------------------------------------------------------------------ tests 5 and 6: out of a session and back; frames the palette never saw
@pytest.fixture(scope="module")
def session_palette():
    """a K = 16 session over the ragged frames, run; its palette taken out; its own streams afterwards; a Palette made of those centroids"""
    import torch
    import cniic_amd
    import oracle_lib as O
    from cniic_amd.dist import ShardedClusterColors
    K = 16
    frames, _ = ragged_frames()
    flat = flat_bytes(frames)
    ws, hs = [w for w, _ in RAGGED], [h for _, h in RAGGED]
    saved = os.environ.get("CNIIC_SP_MIN_PIXELS")
    os.environ["CNIIC_SP_MIN_PIXELS"] = "0"
    try:
        ctx, dev = new_ctx()
        scc = ShardedClusterColors(ctx, K, None, dev)
        t = torch.from_numpy(flat).to(dev)
        handle, _ = scc._cluster(t, flat.size // 3)
        stride = (2 * CHUNK + 3) * 4 + 8192
        out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=dev)
        try:
            cent, pixels = scc.be.palette(handle, K)
            lens, st = scc.be.finish_frames_var(handle, t, ws, hs, out, stride)
        finally:
            scc.be.destroy(handle)
    finally:
        if saved is None:
            del os.environ["CNIIC_SP_MIN_PIXELS"]
        else:
            os.environ["CNIIC_SP_MIN_PIXELS"] = saved
    raw = out.cpu().numpy()
    # the oracle's centroids: test_dist.expected_streams' K-means (mode L over the union histogram)
    keys, counts = O.count_freqs(np.concatenate([keys_of(f) for f in frames]))
    pts = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1).astype(np.int32)
    rc, r = O.kmeans(O.PT_RGBW, O.MODE_L, pts, counts.astype(np.uint32), K)
    assert rc == 0
    pal = cniic_amd.Palette.create(ctx, cent)
    s = dict(ctx=ctx, dev=dev, K=K, frames=frames, cent=cent, pixels=pixels, lens=lens, raw=raw, stride=stride, iterations=st["iterations"],
             oracle_cent=r["centroids"].astype(np.uint8), oracle_labels=r["labels"], oracle_counts=counts, pal=pal)
    yield s
    pal.close()
    ctx.close()


def test_out_of_a_session_and_back(session_palette):
    s = session_palette
    frames, K, ctx, dev = s["frames"], s["K"], s["ctx"], s["dev"]
    assert np.array_equal(s["cent"], s["oracle_cent"].reshape(K, 3))
    assert np.array_equal(s["pixels"], np.bincount(s["oracle_labels"], weights=s["oracle_counts"], minlength=K).astype(np.uint64))
    # the session is still good for its own streams
    exp_sess, iters = oracle(tuple(RAGGED), K)
    sess = [bytes(s["raw"][f * s["stride"]:f * s["stride"] + s["lens"][f]].tobytes()) for f in range(len(frames))]
    assert s["iterations"] == iters and sess == exp_sess
    # the handle made of those centroids: the yardstick's streams
    got, lens, raw, stride = encode_with(ctx, dev, s["pal"], frames)
    for f in range(len(frames)):
        assert got[f] == expected(frames[f], s["cent"])[0], "frame %d" % f
    # ... and an error that is not larger than the session's: summed squared error, exact doubles times the pixel counts
    import torch
    flat = torch.from_numpy(flat_bytes(frames)).to(dev)
    offs = np.concatenate([[0], np.cumsum([f.size for f in frames])])[:-1]
    npx = [f.size // 3 for f in frames]
    _, dec_p, off_p = decode_all(ctx, dev, K, raw, stride, lens, frames)
    _, dec_s, off_s = decode_all(ctx, dev, K, s["raw"], s["stride"], s["lens"], frames)
    torch.cuda.synchronize(dev)
    sse_p = sum(m * n for m, n in zip(ctx.mse_batch_var(flat, offs, dec_p, off_p, npx), npx))
    sse_s = sum(m * n for m, n in zip(ctx.mse_batch_var(flat, offs, dec_s, off_s, npx), npx))
    assert sse_p <= sse_s


def test_frames_the_palette_never_saw(session_palette):
    from cniic_amd import synth
    s = session_palette
    first = [synth.photo(w, h, synth.SEED0 + 950 + i) for i, (w, h) in enumerate([(64, 48), (5, 1639), (17, 1)])]
    second = [synth.photo(w, h, synth.SEED0 + 960 + i) for i, (w, h) in enumerate([(3, 3), (CHUNK + 1, 2), (40, 30)])]
    for frames in (first, second):
        got, _, _, _ = encode_with(s["ctx"], s["dev"], s["pal"], frames)
        assert got == [expected(f, s["cent"])[0] for f in frames]


# ------------------------------------------------------------------ test 7: errors
def test_errors():
    import torch
    import cniic_amd
    from cniic_amd import _lib
    L = _lib.lib()
    ctx, dev = new_ctx()
    h = C_.c_void_p()
    cent = np.zeros((65537, 3), np.uint8)
    for K in (0, 65537):
        assert L.cniic_palette_create(ctx.h, C_.c_void_p(cent.ctypes.data), C_.c_uint32(K), C_.byref(h)) == _lib.BAD_ARG
    assert L.cniic_palette_create(ctx.h, None, C_.c_uint32(16), C_.byref(h)) == _lib.BAD_ARG
    assert L.cniic_palette_create(ctx.h, C_.c_void_p(cent.ctypes.data), C_.c_uint32(16), None) == _lib.BAD_ARG
    assert L.cniic_palette_create(None, C_.c_void_p(cent.ctypes.data), C_.c_uint32(16), C_.byref(h)) == _lib.BAD_ARG

    shapes = ((64, 48), (4, 4), (1, CHUNK + 1), (37, 29))
    frames, _ = ragged_frames(shapes)
    pal = sampled_palette(frames, 16, 7)
    exp = [expected(f, pal)[0] for f in frames]
    flat = flat_bytes(frames)
    ws, hs = [w for w, _ in shapes], [h for _, h in shapes]
    t = torch.from_numpy(flat).to(dev)
    stride = (CHUNK + 1) * 4 + 8192
    out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    p = cniic_amd.Palette.create(ctx, pal)

    def call(rgb, ws_, hs_, F, stride_, out_=out.data_ptr(), lens_=True):
        n = max(len(ws_ if ws_ is not None else hs_), 1)
        lens = (C_.c_uint64 * n)()
        w = (C_.c_uint32 * n)(*ws_) if ws_ is not None else None
        hh = (C_.c_uint32 * n)(*hs_) if hs_ is not None else None
        rc = L.cniic_palette_encode_frames_var(p.h, C_.c_void_p(rgb), w, hh, C_.c_uint32(F), C_.c_void_p(out_), C_.c_uint64(stride_), lens if lens_ else None)
        return rc, [int(x) for x in lens]

    try:
        assert L.cniic_palette_encode_frames_var(None, C_.c_void_p(t.data_ptr()), (C_.c_uint32 * 4)(*ws), (C_.c_uint32 * 4)(*hs), 4, C_.c_void_p(out.data_ptr()), stride,
                                                 (C_.c_uint64 * 4)()) == _lib.BAD_ARG
        assert call(0, ws, hs, 4, stride)[0] == _lib.BAD_ARG
        assert call(t.data_ptr(), None, hs, 4, stride)[0] == _lib.BAD_ARG
        assert call(t.data_ptr(), ws, None, 4, stride)[0] == _lib.BAD_ARG
        assert call(t.data_ptr(), ws, hs, 4, stride, out_=0)[0] == _lib.BAD_ARG
        assert call(t.data_ptr(), ws, hs, 4, stride, lens_=False)[0] == _lib.BAD_ARG
        assert call(t.data_ptr(), ws, hs, 0, stride)[0] == _lib.BAD_ARG
        zero_ws = list(ws); zero_ws[2] = 0
        assert call(t.data_ptr(), zero_ws, hs, 4, stride)[0] == _lib.BAD_ARG
        assert call(t.data_ptr(), ws, hs, 4, 6)[0] == _lib.BAD_ARG
        assert L.cniic_palette_labels(p.h, None, C_.c_uint64(5), C_.c_void_p(out.data_ptr())) == _lib.BAD_ARG
        assert L.cniic_palette_labels(p.h, C_.c_void_p(t.data_ptr()), C_.c_uint64(5), None) == _lib.BAD_ARG
        assert L.cniic_palette_labels(None, C_.c_void_p(t.data_ptr()), C_.c_uint64(5), C_.c_void_p(out.data_ptr())) == _lib.BAD_ARG
        # a stride one word too short for the longest stream: the lengths needed, nothing packed
        longest = max(len(e) for e in exp)
        short = ((longest + 3) & ~3) - 4
        out.fill_(0xA7)
        torch.cuda.synchronize(dev)
        rc, lens = call(t.data_ptr(), ws, hs, 4, short)
        ctx.sync()
        assert rc == _lib.CAPACITY and lens == [len(e) for e in exp]
        assert bool((out == 0xA7).all())
        # ... and every refusal left the handle usable
        got, _, _, _ = encode_with(ctx, dev, p, frames)
        assert got == exp
    finally:
        p.close()
        ctx.close()
