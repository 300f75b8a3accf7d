"""cniic_palette_fit_frames_var (k_palette_fit, cniic_amd/csrc/k_palette.hip): the summed squared error of every frame and the pixels per
entry of a batch under a frozen palette, against a numpy brute force in int64 (tests/warm_ref.py: the nearest entry in squared integer
distance, the lowest index among equals) -- exactly, for sse and for the counts.

One batch covers the kernel's cuts: a chunk is 4096 pixels (kFrameVarChunk), read 16 pixels at a time from the first 16-byte boundary, with
a head and a tail of fewer than 16 pixels; the frames are packed back to back, so most start at an odd byte.  1 x 1 and 3 x 5 are all head
or tail; 64 x 64 is one chunk exactly; 100 x 41 is 4 pixels past one; 350 x 200 is 70 000 pixels, past 2^16; the flat frame sends every
lane to one entry, the checkerboard to two."""
import numpy as np
import pytest

import warm_ref as R

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (3, 5), (64, 64), (100, 41), (350, 200), (256, 256), (128, 128))   # (w, h); the last two are the flat frame and the checkerboard
_cache = {}


def batch():
    if "frames" not in _cache:
        from cniic_amd import synth
        frames = [synth.photo(w, h, synth.SEED0 + 700 + i) for i, (w, h) in enumerate(SHAPES[:5])]
        frames.append(np.full((256, 256, 3), (201, 17, 64), np.uint8))
        y, x = np.mgrid[0:128, 0:128]
        frames.append(np.where(((x + y) & 1)[..., None] == 1, np.array([250, 250, 5], np.uint8), np.array([3, 40, 200], np.uint8)).astype(np.uint8))
        assert [(f.shape[1], f.shape[0]) for f in frames] == list(SHAPES)
        _cache["frames"] = frames
        starts = np.cumsum([0] + [f.size for f in frames[:-1]])
        assert sum(1 for s in starts if s % 16) >= 4      # packed back to back, most frames start unaligned
    return _cache["frames"]


def palette(name):
    """K = 1, 16, 256, 300 sampled from the batch's pixels, and K = 16 with entries 3 and 9 equal"""
    if ("pal", name) not in _cache:
        dup = name == "16dup"
        px = np.concatenate([f.reshape(-1, 3) for f in batch()[:5 if dup else None]])   # (16dup: from the photographs, so that no other entry is the flat colour)
        K = 16 if dup else int(name)
        pal = px[np.random.default_rng(900 + K).choice(px.shape[0], K, replace=False)].copy()
        if dup:
            pal[3] = (201, 17, 64)    # the flat frame's colour, twice: entry 9 is shadowed
            pal[9] = pal[3]
            assert sum(1 for e in pal if tuple(e) == (201, 17, 64)) == 2
        _cache[("pal", name)] = pal
    return _cache[("pal", name)]


def reference(name):
    if ("ref", name) not in _cache:
        _cache[("ref", name)] = R.fit(palette(name), batch())
    return _cache[("ref", name)]


def new_ctx(timers=False):
    from cniic_amd import _lib
    from test_frames_var import new_ctx as make
    ctx, dev = make()
    if timers:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    return ctx, dev


@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("name", ["1", "16", "256", "300", "16dup"])
def test_fit_equals_the_brute_force(name, memory):
    import torch
    import cniic_amd
    from test_frames_var import flat_bytes
    frames = batch()
    sse_ref, px_ref = reference(name)
    ws, hs = [w for w, _ in SHAPES], [h for _, h in SHAPES]
    flat = flat_bytes(frames)
    ctx, dev = new_ctx(timers=True)
    try:
        with cniic_amd.Palette.create(ctx, palette(name)) as p:
            src = flat
            if memory == "device":
                src = torch.from_numpy(flat).to(dev)
                torch.cuda.synchronize(dev)
            sse, pixels = p.fit_frames_var(src, ws, hs)
            assert ctx.kernel_time("pal_fit")[1] == 1      # one launch whatever the number of frames
            sse_only, none = p.fit_frames_var(src, ws, hs, want_pixels=False)
    finally:
        ctx.close()
    assert sse.tolist() == sse_ref.tolist()
    assert pixels.tolist() == px_ref.tolist()
    assert none is None and sse_only.tolist() == sse_ref.tolist()
    assert int(pixels.sum()) == sum(w * h for w, h in SHAPES)
    if name == "16dup":
        assert pixels[9] == 0 and pixels[3] >= 256 * 256 and sse[5] == 0
    if name == "1":
        assert pixels.tolist() == [sum(w * h for w, h in SHAPES)]


@pytest.mark.parametrize("name", ["16", "300"])
def test_fit_is_the_error_of_the_decoded_streams(name):
    """sse[f] = the summed squared difference between frame f and what its cniic_palette_encode_frames_var stream decodes to"""
    import torch
    import cniic_amd
    from test_frames_var import flat_bytes
    frames = batch()
    K = len(palette(name))
    ws, hs = [w for w, _ in SHAPES], [h for _, h in SHAPES]
    flat = flat_bytes(frames)
    ctx, dev = new_ctx()
    try:
        with cniic_amd.Palette.create(ctx, palette(name)) as p:
            t = torch.from_numpy(flat).to(dev)
            stride = (max(f.size for f in frames) * 2 + 16384 + 3) & ~3
            out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            lens = p.encode_frames_var(t, ws, hs, out, stride)
            sse, _ = p.fit_frames_var(t, ws, hs)
        img_stride = max(f.size for f in frames)
        back = torch.zeros(img_stride * len(frames), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        rc, dw, dh, rcs = ctx.decode_batch("cluster-colors(%d)" % K, out, stride, lens, len(frames), back, img_stride)
        ctx.sync()
        host = back.cpu().numpy()
    finally:
        ctx.close()
    assert rc == 0 and not any(rcs)
    for f, frame in enumerate(frames):
        dec = host[f * img_stride:f * img_stride + frame.size].astype(np.int64)
        assert int(((dec - frame.reshape(-1).astype(np.int64)) ** 2).sum()) == int(sse[f]), "frame %d" % f


def test_fit_arguments():
    import cniic_amd
    from cniic_amd import _lib
    ctx, dev = new_ctx()
    try:
        with cniic_amd.Palette.create(ctx, palette("16")) as p:
            px = np.zeros((4, 3), np.uint8)
            assert p.fit_frames_var(px, [], [], allow=(_lib.BAD_ARG,))[0] == _lib.BAD_ARG          # frames == 0
            assert p.fit_frames_var(px, [2, 0], [2, 5], allow=(_lib.BAD_ARG,))[0] == _lib.BAD_ARG  # an empty frame
            assert p.fit_frames_var(None, [2], [2], allow=(_lib.BAD_ARG,))[0] == _lib.BAD_ARG      # a null image
            rc, sse, pixels = p.fit_frames_var(px, [2], [2], allow=(_lib.BAD_ARG,))
            assert rc == 0 and int(pixels.sum()) == 4
    finally:
        ctx.close()
