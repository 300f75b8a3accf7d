"""cniic_cc_finish_frames_var: a batch of frames of DIFFERENT sizes coded with one palette, against the oracle's union clustering
(tests/test_dist.py expected_streams: K-means mode L over the union histogram, then each reduced frame coded alone).

C = 4096 is kPackChunk of cniic_amd/csrc/k_huff.hip (kPackThreads 256 x kPackPer 16): the labels one block of the pack, of the label copy
and of the chunk scan's row handle; the ragged list below sits on both sides of it."""
import ctypes as C_
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from test_dist import expected_streams, make_frames  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096   # kPackChunk

# (w, h).  Pixels before each frame: 0, 3072, 7168 (16-byte aligned label runs), then 15363, 15379, 19476, 19477, 19492, 19509, 23604 (not
# aligned).  Multi-block frames are those above C pixels: 4 x 4 -- one block -- sits between the 2C+3 frame and 1 x (C+1).
RAGGED = [(64, 48), (C, 1), (5, 1639), (4, 4), (1, C + 1), (1, 1), (5, 3), (17, 1), (C - 1, 1), (37, 29)]
assert 5 * 1639 == 2 * C + 3

_cache = {}


def ragged_frames(shapes=tuple(RAGGED)):
    """the frames (synth.photo), and the oracle's streams for K = 16: computed once, shared, never written to"""
    from cniic_amd import synth
    if shapes not in _cache:
        frames = [synth.photo(w, h, synth.SEED0 + 900 + i) for i, (w, h) in enumerate(shapes)]
        for f in frames:
            f.setflags(write=False)
        _cache[shapes] = (frames, {})
    return _cache[shapes]


def oracle(shapes, K):
    frames, exp = ragged_frames(shapes)
    if K not in exp:
        exp[K] = expected_streams(frames, K)
    return exp[K]


def flat_bytes(frames):
    return np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in frames])


def new_ctx():
    import torch
    import cniic_amd
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    return cniic_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream), dev


def encode_var(frames, K, stride=None):
    """-> (list of streams, stats, ctx) through ShardedClusterColors.encode_frames_var with device buffers"""
    import torch
    from cniic_amd.dist import ShardedClusterColors
    ctx, dev = new_ctx()
    ws, hs = [f.shape[1] for f in frames], [f.shape[0] for f in frames]
    if stride is None:
        stride = (max(w * h for w, h in zip(ws, hs)) * 4 + 8192 + 3) & ~3
    out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=dev)
    lens, st = ShardedClusterColors(ctx, K, None, dev).encode_frames_var(torch.from_numpy(flat_bytes(frames)).to(dev), ws, hs, out, stride)
    host = out.cpu().numpy()
    return [bytes(host[f * stride:f * stride + lens[f]].tobytes()) for f in range(len(frames))], st, ctx


@pytest.mark.parametrize("trees", ["gpu", "host"])
@pytest.mark.parametrize("route", ["dense", "partition"])
def test_ragged_frames_equal_the_oracle(monkeypatch, route, trees):
    """test 1: the ragged list, both session routes, trees by k_frame_trees and on host threads; every stream decodes to its frame's shape"""
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0" if route == "partition" else str(1 << 40))
    if trees == "host":
        monkeypatch.setenv("CNIIC_FRAME_TREES_HOST", "1")
    else:
        monkeypatch.delenv("CNIIC_FRAME_TREES_HOST", raising=False)
    K = 16
    frames, _ = ragged_frames()
    exp, iters = oracle(tuple(RAGGED), K)
    got, st, ctx = encode_var(frames, K)
    assert st["iterations"] == iters
    for f, (w, h) in enumerate(RAGGED):
        assert got[f] == exp[f], "frame %d (%d x %d) differs from the oracle's stream" % (f, w, h)
        rc, back = ctx.decode("cluster-colors(%d)" % K, got[f])
        assert rc == 0 and back.shape == (h, w, 3)
    ctx.close()


def test_one_flat_frame_among_the_others(monkeypatch):
    """test 2: a frame of one colour (a one-symbol tree, no payload) and one that uses two of the sixteen clusters"""
    from cniic_amd import synth
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    K = 16
    frames = [synth.photo(37, 29, synth.SEED0 + 931), np.full((7, 9, 3), 200, np.uint8)]
    two = np.zeros((11, 23, 3), np.uint8); two[:, 8:] = (250, 10, 40); frames.append(two)
    frames.append(synth.photo(C + 5, 1, synth.SEED0 + 932))
    exp, iters = expected_streams(frames, K)
    got, st, ctx = encode_var(frames, K)
    ctx.close()
    assert st["iterations"] == iters
    assert len(exp[1]) == 8 + 12      # dimensions and one leaf: the yardstick itself has the one-symbol tree
    assert len(exp[2]) == 8 + 1 + 2 * 12 + (11 * 23 + 7) // 8   # two leaves, one bit per pixel
    for f in range(len(frames)):
        assert got[f] == exp[f], "frame %d" % f


def test_wide_labels(monkeypatch):
    """test 3: K = 300 -- two-byte labels through the label copy, the histogram and the var pack; trees on the host"""
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    K = 300
    shapes = ((64, 48), (4, 4), (1, C + 1), (37, 29))
    frames, _ = ragged_frames(shapes)
    keys = np.unique(np.concatenate([f.reshape(-1, 3).astype(np.uint32) @ np.array([65536, 256, 1], np.uint32) for f in frames]))
    assert keys.size >= 300
    exp, iters = oracle(shapes, K)
    got, st, ctx = encode_var(frames, K)
    ctx.close()
    assert st["iterations"] == iters
    for f in range(len(frames)):
        assert got[f] == exp[f], "frame %d" % f


@pytest.mark.parametrize("F,h,w", [(4, 48, 64), (3, 29, 37)])
def test_equal_sizes_change_nothing(monkeypatch, F, h, w):
    """test 4: frames of one size through finish_frames_var and through finish_frames, two sessions over the same pixels: the same bytes"""
    import torch
    from cniic_amd.dist import ShardedClusterColors
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    K = 16
    frames = make_frames(0, F, h, w)
    ctx, dev = new_ctx()
    stride = (w * h * 4 + 4096 + 3) & ~3
    t = torch.from_numpy(frames).to(dev)
    scc = ShardedClusterColors(ctx, K, None, dev)
    out_e = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
    out_v = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
    lens_e, st_e = scc.encode_frames(t, w, h, F, out_e, stride)
    lens_v, st_v = scc.encode_frames_var(t.reshape(-1), [w] * F, [h] * F, out_v, stride)
    ctx.close()
    assert lens_v == list(lens_e) and st_v["iterations"] == st_e["iterations"]
    assert bytes(out_v.cpu().numpy().tobytes()) == bytes(out_e.cpu().numpy().tobytes())


def test_one_frame_is_the_single_encode(monkeypatch):
    """test 5"""
    from cniic_amd import synth
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    img = synth.photo(40, 30, synth.SEED0 + 940)
    got, st, ctx = encode_var([img], 16)
    rc, exp, st1 = ctx.encode("cluster-colors(16)", img)
    ctx.close()
    assert rc == 0 and got[0] == exp and st["iterations"] == st1["iterations"]


# frames 0, 1, 65534, 65535, 65536 and 59 more, drawn once with numpy's default_rng(20261018)
SAMPLE = [0, 1, 154, 1217, 1777, 1812, 1994, 2231, 2532, 4090, 4524, 7720, 7803, 8890, 9364, 10054, 10201, 11407, 11826, 11995, 16119, 16283, 22443,
          25080, 25282, 26516, 26865, 29672, 29975, 30302, 31908, 33022, 33225, 37102, 37607, 38195, 40404, 40896, 43636, 45353, 45434, 45460, 45589,
          46019, 47546, 48070, 49992, 50422, 51117, 53605, 54971, 55098, 55664, 56253, 56708, 56884, 57268, 58855, 60607, 63479, 64140, 65534, 65535,
          65536]


def test_more_frames_than_a_grids_y_extent(monkeypatch):
    """test 6: 65 537 frames of 1-4 pixels.  The oracle codes the 64 sampled frames alone and all the others as ONE image behind them: the
    union histogram -- and so the palette -- is that of all 65 537 frames, and only the sampled frames cost a Python call each"""
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    K, F = 16, 65537
    assert len(SAMPLE) == 64 and len(set(SAMPLE)) == 64
    rng = np.random.default_rng(65537)
    shapes = np.array([(1, 1), (2, 1), (1, 2), (3, 1), (1, 3), (2, 2), (4, 1), (1, 4)])[rng.integers(0, 8, size=F)]   # (w, h)
    palette = rng.integers(0, 256, size=(48, 3), dtype=np.uint8)
    npx = shapes[:, 0] * shapes[:, 1]
    start = np.concatenate([[0], np.cumsum(npx)])
    pixels = palette[rng.integers(0, 48, size=int(start[-1]))]
    assert np.unique(pixels, axis=0).shape[0] >= 16
    frame = lambda f: pixels[start[f]:start[f + 1]].reshape(shapes[f][1], shapes[f][0], 3)
    rest = np.ones(F, bool); rest[SAMPLE] = False
    rest_px = np.concatenate([pixels[start[f]:start[f + 1]] for f in np.nonzero(rest)[0]]).reshape(1, -1, 3)
    exp, iters = expected_streams([frame(f) for f in SAMPLE] + [rest_px], K)

    import torch
    from cniic_amd.dist import ShardedClusterColors
    ctx, dev = new_ctx()
    stride = 64   # at most four leaves: 8 + 4 * 12 + 3 bytes of header, 2 of payload
    out = torch.zeros(stride * F, dtype=torch.uint8, device=dev)
    lens, st = ShardedClusterColors(ctx, K, None, dev).encode_frames_var(torch.from_numpy(pixels.reshape(-1)).to(dev), shapes[:, 0], shapes[:, 1], out, stride)
    ctx.close()
    host = out.cpu().numpy()
    assert st["iterations"] == iters
    assert len(lens) == F and min(lens) > 0
    for i, f in enumerate(SAMPLE):
        assert bytes(host[f * stride:f * stride + lens[f]].tobytes()) == exp[i], "frame %d" % f


def _session(scc, t, npx):
    handle, _ = scc._cluster(t, npx)
    return handle


def test_host_buffers(monkeypatch):
    """test 7: rgb and out in host memory (the session itself was opened on the same pixels in device memory)"""
    import torch
    from cniic_amd.dist import ShardedClusterColors
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    K = 16
    frames, _ = ragged_frames()
    exp, iters = oracle(tuple(RAGGED), K)
    flat = flat_bytes(frames)
    ws, hs = [w for w, _ in RAGGED], [h for _, h in RAGGED]
    ctx, dev = new_ctx()
    scc = ShardedClusterColors(ctx, K, None, dev)
    handle = _session(scc, torch.from_numpy(flat).to(dev), flat.size // 3)
    stride = (2 * C + 3) * 4 + 8192
    out = np.zeros(stride * len(frames), np.uint8)
    try:
        lens, st = scc.be.finish_frames_var(handle, flat, ws, hs, out, stride)
    finally:
        scc.be.destroy(handle)
    ctx.close()
    assert st["iterations"] == iters
    for f in range(len(frames)):
        assert bytes(out[f * stride:f * stride + lens[f]].tobytes()) == exp[f], "frame %d" % f


@pytest.mark.parametrize("route", ["dense", "partition"])
def test_refusals(monkeypatch, route):
    """test 8: every refusal is CNIIC_ERR_BAD_ARG and leaves the session usable: the right call afterwards gives the oracle's streams"""
    import torch
    from cniic_amd import _lib
    from cniic_amd.dist import ShardedClusterColors
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0" if route == "partition" else str(1 << 40))
    K = 16
    shapes = ((64, 48), (4, 4), (1, C + 1), (37, 29))
    frames, _ = ragged_frames(shapes)
    exp, iters = oracle(shapes, K)
    flat = flat_bytes(frames)
    ws, hs = [w for w, _ in shapes], [h for _, h in shapes]
    ctx, dev = new_ctx()
    scc = ShardedClusterColors(ctx, K, None, dev)
    t = torch.from_numpy(flat).to(dev)
    stride = (C + 1) * 4 + 8192
    out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=dev)
    handle = _session(scc, t, flat.size // 3)
    L = _lib.lib()

    def call(ws, hs, F, stride):
        n = max(len(ws), 1)
        lens = (C_.c_uint64 * n)()
        rc = L.cniic_cc_finish_frames_var(handle, C_.c_void_p(t.data_ptr()), (C_.c_uint32 * n)(*ws), (C_.c_uint32 * n)(*hs), C_.c_uint32(F),
                                          C_.c_void_p(out.data_ptr()), C_.c_uint64(stride), lens, None)
        return rc, (L.cniic_last_error(ctx.h) or b"").decode()

    try:
        rc, msg = call(ws[:3] + [36], hs[:3] + [29], 4, stride)      # 29 pixels short ...
        assert rc == _lib.BAD_ARG
        short_hs = list(hs); short_hs[2] = C                           # ... and one pixel short: 1 x C instead of 1 x (C + 1)
        rc, msg = call(ws, short_hs, 4, stride)
        assert rc == _lib.BAD_ARG and str(flat.size // 3) in msg and str(flat.size // 3 - 1) in msg, msg
        zero_ws = list(ws); zero_ws[2] = 0
        assert call(zero_ws, hs, 4, stride)[0] == _lib.BAD_ARG
        assert call(ws, hs, 4, 6)[0] == _lib.BAD_ARG
        assert call(ws, hs, 0, stride)[0] == _lib.BAD_ARG
        lens, st = scc.be.finish_frames_var(handle, t, ws, hs, out, stride)
    finally:
        scc.be.destroy(handle)
    ctx.close()
    host = out.cpu().numpy()
    assert st["iterations"] == iters
    for f in range(len(frames)):
        assert bytes(host[f * stride:f * stride + lens[f]].tobytes()) == exp[f], "frame %d" % f


def test_a_stride_below_the_longest_stream_is_answered_as_for_equal_frames(monkeypatch):
    """test 8, last case: the status of cniic_cc_finish_frames for the same batch, and the lengths needed in lens"""
    import torch
    from cniic_amd import _lib
    from cniic_amd.dist import ShardedClusterColors
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    K, F, h, w = 16, 3, 29, 37
    frames = make_frames(0, F, h, w)
    ctx, dev = new_ctx()
    scc = ShardedClusterColors(ctx, K, None, dev)
    t = torch.from_numpy(frames).to(dev).reshape(-1)
    big = (w * h * 4 + 4096 + 3) & ~3
    out = torch.zeros(big * F, dtype=torch.uint8, device=dev)
    need, _ = scc.encode_frames_var(t, [w] * F, [h] * F, out, big)
    L = _lib.lib()
    small = 64
    assert small < max(need)
    got = {}
    for which in ("equal", "var"):
        handle = _session(scc, t, w * h * F)
        lens = (C_.c_uint64 * F)()
        try:
            if which == "equal":
                rc = L.cniic_cc_finish_frames(handle, C_.c_void_p(t.data_ptr()), C_.c_uint32(w), C_.c_uint32(h), C_.c_uint32(F), C_.c_void_p(out.data_ptr()),
                                              C_.c_uint64(small), lens, None)
            else:
                rc = L.cniic_cc_finish_frames_var(handle, C_.c_void_p(t.data_ptr()), (C_.c_uint32 * F)(*[w] * F), (C_.c_uint32 * F)(*[h] * F), C_.c_uint32(F),
                                                  C_.c_void_p(out.data_ptr()), C_.c_uint64(small), lens, None)
        finally:
            scc.be.destroy(handle)
        got[which] = (rc, [int(x) for x in lens])
    ctx.close()
    assert got["var"][0] == got["equal"][0] == _lib.CAPACITY
    assert got["var"][1] == got["equal"][1] == need
