"""K-means from given centroids on the GPU (cniic_kmeans_rgbw_from, cniic_kmeans_xyrgb_from, cniic_cc_set_centroids,
cniic_codec_encode_warm; k_rgbw_given_cent, k_xy_init_from, k_xyw_init_from) against tests/warm_ref.py's lloyd_from, bit for bit: return
code, iterations, empty_reseeds, centroids, labels and members.  Every init variant has a precondition, asserted on the reference's run
before the GPU is asked:
    (a)  the converged palette of a DIFFERENT image            at least 3 iterations (where K allows any: not K = 1, not K = U)
    (b)  all K entries the same colour                          exactly 1 iteration, nothing moves: stay-on-tie against the chunk labels
    (c)  one entry at (255,255,255), the image's channels < 128  empty_reseeds >= 1
    (c') xyrgb: a white centroid in the corner (0, 0), where a   empty_reseeds >= 1
         darker one already sits: no pixel can prefer it
    (d)  the reference's own init                                 the ordinary run: equal to cniic_kmeans_rgbw / _xyrgb as well
"""
import ctypes as C_

import numpy as np
import pytest

import oracle_lib as O
import warm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


def photo(w, h, seed):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + seed)


# ------------------------------------------------------------------ rgbw
_cache = {}


def colours(U, which):
    """U distinct colours of a photo-like image with their pixel counts, ascending keys; which: "A" the image under test, "B" a different one,
    "dark" A with every channel halved (below 128)"""
    key = ("colours", U, which)
    if key not in _cache:
        img = photo(240, 180, 77 if which == "B" else 41)
        if which == "dark":
            img = img >> 1
        keys, w = R.colour_points(img)
        assert keys.size >= U, "the image has %d distinct colours" % keys.size
        pick = np.sort(np.random.default_rng(U).choice(keys.size, U, replace=False))
        _cache[key] = (keys[pick].copy(), w[pick].copy())
    return _cache[key]


def rgbw_case(U, K, kind, max_iters=0):
    """-> (keys, weights, init (K, 3), the reference's run), computed once per case"""
    key = ("rgbw", U, K, kind, max_iters)
    if key in _cache:
        return _cache[key]
    keys, w = colours(U, "dark" if kind == "c" else "A")
    pts = R.pts_of_keys(keys)
    if kind == "a":
        kb, wb = colours(U, "B")
        rcb, other = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(kb), wb, K)
        assert rcb == 0
        init = other["centroids"]
    elif kind == "b":
        init = np.tile(np.array([[90, 120, 60]], np.int32), (K, 1))
    elif kind == "c":
        assert pts.max() < 128
        init = R.ref_init_centroids(pts, K)
        init[K // 2] = (255, 255, 255)   # (every other entry is below 128 in every channel: strictly nearer to every point than white)
    else:
        init = R.ref_init_centroids(pts, K)
    rc, ref = R.lloyd_from(O.PT_RGBW, pts, w, K, init, max_iters=max_iters)
    assert rc in (O.OK, O.FEW_ACTIVE)   # (a capped run, or K = U from another image's colours, may end with too few active clusters: the GPU must say the same)
    if not max_iters:
        if kind == "a" and 1 < K < U:
            assert ref["iterations"] >= 3, "init (a) converged in %d iterations" % ref["iterations"]
        if kind == "b":
            assert ref["iterations"] == 1 and ref["moved_last"] == 0 and np.array_equal(ref["labels"], O.init_labels(U, K))
        if kind == "c":
            assert ref["empty_reseeds"] >= 1
    _cache[key] = (keys, w, init, ref)
    return _cache[key]


def same_rgbw(got, rc, ref):
    assert rc == ref["rc"]
    assert got["stats"]["iterations"] == ref["iterations"]
    assert got["stats"]["empty_reseeds"] == ref["empty_reseeds"]
    assert np.array_equal(got["centroids"].astype(np.int32), ref["centroids"])
    assert np.array_equal(got["labels"], ref["labels"])
    assert np.array_equal(got["members"], ref["members"])


ROUTES = {
    # name: (U, K, environment, flags)
    "persist16": (5000, 16, {"CNIIC_KM_PS_REQUIRE": "1"}, 0),
    "loop16": (5000, 16, {"CNIIC_KM_LOOP": "1"}, 0),
    "brute16": (5000, 16, {}, "KM_BRUTE_FORCE"),
    "noskip16": (5000, 16, {}, "KM_NO_SKIP"),
    "k1": (5000, 1, {}, 0),
    "wide300": (5000, 300, {}, 0),
    "big2100": (6000, 2100, {}, 0),
    "k_is_u": (5000, 5000, {}, 0),
}


def run_route(ctx, monkeypatch, route, kind, max_iters=0):
    from cniic_amd import _lib
    U, K, env, flags = ROUTES[route]
    for name in ("CNIIC_KM_PS_REQUIRE", "CNIIC_KM_LOOP"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    keys, w, init, ref = rgbw_case(U, K, kind, max_iters)
    rc, got = ctx.kmeans_rgbw(keys, w, K, max_iters=max_iters, flags=getattr(_lib, flags) if flags else 0, init=init, allow=(_lib.FEW_ACTIVE,))
    same_rgbw(got, rc, ref)
    return keys, w, got


@pytest.mark.parametrize("route", list(ROUTES))
def test_rgbw_from_another_images_palette_on_every_route(ctx, monkeypatch, route):
    run_route(ctx, monkeypatch, route, "a")


# (big2100 with (c) is left out: its reference takes 113 iterations of a 6000 x 2100 step on the CPU, seconds for nothing (a) and (d) do not show)
VARIANTS = [(r, k) for r in ("persist16", "loop16", "brute16", "wide300", "big2100") for k in "bcd" if (r, k) != ("big2100", "c")]


@pytest.mark.parametrize("route,kind", VARIANTS)
def test_rgbw_init_variants(ctx, monkeypatch, route, kind):
    keys, w, got = run_route(ctx, monkeypatch, route, kind)
    if kind == "d":   # the ordinary run, on the GPU as well
        rc, cold = ctx.kmeans_rgbw(keys, w, ROUTES[route][1], flags=0)
        assert rc == 0 and got["stats"]["empty_reseeds"] == cold["stats"]["empty_reseeds"] and cold["stats"]["iterations"] == got["stats"]["iterations"]
        for name in ("centroids", "labels", "members"):
            assert np.array_equal(cold[name], got[name]), name


@pytest.mark.parametrize("max_iters", [1, 2])
@pytest.mark.parametrize("route", ["persist16", "loop16", "wide300"])
def test_rgbw_iteration_cap(ctx, monkeypatch, route, max_iters):
    run_route(ctx, monkeypatch, route, "a", max_iters)


# ------------------------------------------------------------------ xyrgb
def xy_case(w, h, K, kind):
    key = ("xy", w, h, K, kind)
    if key in _cache:
        return _cache[key]
    img = photo(w, h, 5) >> 1 if kind == "c" else photo(w, h, 5)
    pts = R.xy_pts(img)
    if kind == "a":
        rcb, other = O.kmeans(O.PT_XYRGB, O.MODE_L, R.xy_pts(photo(w, h, 6)), None, K)
        assert rcb == 0
        init = other["centroids"]
    elif kind == "c":
        assert img.max() < 128
        init = R.ref_init_centroids(pts, K)
        # the corner (0, 0) is where the last cluster's init centroid already sits (the first pixel heads chunk K - 1) with a colour below 128:
        # at most 3 * 127^2 from any pixel's, while white is at least 3 * 128^2 away -- so centroid K - 1 is STRICTLY nearer to every pixel
        assert K // 2 != K - 1 and tuple(init[K - 1, :2]) == (0, 0)
        init[K // 2] = (0, 0, 255, 255, 255)
    else:
        init = R.ref_init_centroids(pts, K)
    rc, ref = R.lloyd_from(O.PT_XYRGB, pts, None, K, init)
    assert rc in (O.OK, O.FEW_ACTIVE)
    if kind == "c":
        assert ref["empty_reseeds"] >= 1
    _cache[key] = (img, init, ref)
    return _cache[key]


def same_xy(got, rc, ref):
    assert rc == ref["rc"]
    assert got["stats"]["iterations"] == ref["iterations"]
    assert got["stats"]["empty_reseeds"] == ref["empty_reseeds"]
    assert np.array_equal(R.c5_of(got["centroids"]), ref["centroids"])
    assert np.array_equal(got["labels"], ref["labels"])
    assert np.array_equal(got["members"], ref["members"])


@pytest.mark.parametrize("kind", ["a", "c", "d"])
@pytest.mark.parametrize("w,h,K", [(130, 70, 16), (130, 70, 600), (16385, 3, 9)])
def test_xyrgb_from(ctx, monkeypatch, w, h, K, kind):
    monkeypatch.delenv("CNIIC_XY_UNFUSED", raising=False)
    img, init, ref = xy_case(w, h, K, kind)
    from cniic_amd import _lib
    rc, got = ctx.kmeans_xyrgb(img, K, init=R.colorpos(init), allow=(_lib.FEW_ACTIVE,))
    same_xy(got, rc, ref)
    if kind == "d":
        rc, cold = ctx.kmeans_xyrgb(img, K)
        assert rc == 0 and np.array_equal(cold["centroids"], got["centroids"]) and np.array_equal(cold["labels"], got["labels"])


@pytest.mark.parametrize("K", [16, 600])
def test_xyrgb_from_unfused(ctx, monkeypatch, K):
    monkeypatch.setenv("CNIIC_XY_UNFUSED", "1")
    img, init, ref = xy_case(130, 70, K, "a")
    from cniic_amd import _lib
    rc, got = ctx.kmeans_xyrgb(img, K, init=R.colorpos(init), allow=(_lib.FEW_ACTIVE,))
    same_xy(got, rc, ref)


@pytest.mark.parametrize("w,h,K", [(130, 70, 16), (16385, 3, 9)])
def test_xyrgb_from_refuses_centroids_outside_the_image(ctx, w, h, K):
    from cniic_amd import _lib
    img, init, _ = xy_case(w, h, K, "d")
    for col, v in ((0, w), (1, h)):
        bad = init.copy()
        bad[K - 1, col] = v
        rc, _ = ctx.kmeans_xyrgb(img, K, init=R.colorpos(bad), allow=(_lib.BAD_ARG,))
        assert rc == _lib.BAD_ARG
    edge = init.copy()
    edge[0, 0], edge[0, 1] = w - 1, h - 1   # the last pixel is inside
    rc, _ = ctx.kmeans_xyrgb(img, K, init=R.colorpos(edge))
    assert rc == 0


# ------------------------------------------------------------------ sessions
SHAPES = ((64, 64), (100, 41), (7, 9))


def session_case(K):
    key = ("session", K)
    if key in _cache:
        return _cache[key]
    frames = [photo(w, h, 300 + i) for i, (w, h) in enumerate(SHAPES)]
    keys, wts = R.colour_points(frames)
    pts = R.pts_of_keys(keys)
    kb, wb = R.colour_points([photo(w, h, 320 + i) for i, (w, h) in enumerate(SHAPES)])
    rcb, other = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(kb), wb, K)
    assert rcb == 0
    init = other["centroids"].astype(np.uint8)
    rc, ref = R.lloyd_from(O.PT_RGBW, pts, wts, K, init)
    assert rc == 0 and ref["iterations"] >= 3
    rcc, cold = O.kmeans(O.PT_RGBW, O.MODE_L, pts, wts, K)
    assert rcc == 0 and not np.array_equal(cold["centroids"], ref["centroids"])
    warm = [R.cc_stream(f, keys, ref["labels"], ref["centroids"]) for f in frames]
    cold_streams = [R.cc_stream(f, keys, cold["labels"], cold["centroids"]) for f in frames]
    _cache[key] = (frames, init, ref, warm, cold, cold_streams)
    return _cache[key]


def open_session(kind, ctx, dev, flat_d, npx, K):
    """-> (backend, session handle, what must stay alive with it)"""
    import torch
    from cniic_amd import _lib
    from cniic_amd.dist import HipBackend
    be = HipBackend(ctx, dev)
    if kind == "dense":       # cniic_cc_create, one shard, the library's own partials
        table = be.hist_dense(flat_d, npx)
        h = C_.c_void_p()
        o = _lib.KmOpts(0, 0, 0, 0)
        ctx._check(be.L.cniic_cc_create(ctx.h, C_.c_void_p(table.data_ptr()), C_.c_uint32(K), C_.byref(o), C_.c_uint32(0), C_.c_uint32(1), None, C_.byref(h)))
        return be, h, table
    ctx.set_opt(_lib.OPT_SP_MIN_PIXELS, 0)   # the pixel partition, on frames this small
    h = be.image_begin(flat_d, npx)
    assert h is not None
    occ = be.image_occupancy(h)
    partials = be.new_partials(K)
    be.image_create(h, occ, K, partials)
    torch.cuda.synchronize(dev)
    return be, h, (occ, partials)


def finish(be, h, frames, flat_d):
    import torch
    ws, hs = [f.shape[1] for f in frames], [f.shape[0] for f in frames]
    stride = (max(f.size for f in frames) * 2 + 8192 + 3) & ~3
    out = torch.zeros(stride * len(frames), dtype=torch.uint8, device=flat_d.device)
    torch.cuda.synchronize(flat_d.device)
    lens, st = be.finish_frames_var(h, flat_d, ws, hs, out, stride)
    raw = out.cpu().numpy()
    return [raw[f * stride:f * stride + lens[f]].tobytes() for f in range(len(frames))], st


@pytest.mark.parametrize("K", [16, 256])
@pytest.mark.parametrize("kind", ["dense", "image"])
def test_session_set_centroids_run_finish_palette(monkeypatch, kind, K):
    import torch
    from test_frames_var import flat_bytes, new_ctx
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0" if kind == "image" else str(1 << 40))
    frames, init, ref, warm, _, _ = session_case(K)
    ctx, dev = new_ctx()
    flat = flat_bytes(frames)
    flat_d = torch.from_numpy(flat).to(dev)
    torch.cuda.synchronize(dev)
    be, h, keep = open_session(kind, ctx, dev, flat_d, flat.size // 3, K)
    try:
        assert be.set_centroids(h, init) == 0
        st = be.run(h, None)
        assert st["iterations"] == ref["iterations"] and st["empty_reseeds"] == ref["empty_reseeds"]
        got, st2 = finish(be, h, frames, flat_d)
        cent, pixels = be.palette(h, K)
    finally:
        be.destroy(h)
        ctx.close()
    assert np.array_equal(cent.astype(np.int32), ref["centroids"])
    for f in range(len(frames)):
        assert got[f] == warm[f], "frame %d (%d x %d) differs from the reference's stream" % ((f,) + SHAPES[f])


@pytest.mark.parametrize("how", ["run", "assign"])
def test_set_centroids_after_the_first_assign_is_refused_and_changes_nothing(monkeypatch, how):
    import torch
    from cniic_amd import _lib
    from test_frames_var import flat_bytes, new_ctx
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", str(1 << 40))
    K = 16
    frames, init, _, _, cold, cold_streams = session_case(K)
    ctx, dev = new_ctx()
    flat = flat_bytes(frames)
    flat_d = torch.from_numpy(flat).to(dev)
    torch.cuda.synchronize(dev)
    be, h, keep = open_session("dense", ctx, dev, flat_d, flat.size // 3, K)
    try:
        if how == "run":
            st = be.run(h, None)
            assert be.set_centroids(h, init, allow=(_lib.BAD_ARG,)) == _lib.BAD_ARG
            assert st["iterations"] == cold["stats"]["iterations"]
        else:   # the caller's own loop (kmeans.rs:26-32): refused between the first assign and its update
            be.assign(h)
            assert be.set_centroids(h, init, allow=(_lib.BAD_ARG,)) == _lib.BAD_ARG
            changed, iters = C_.c_uint64(1), 0
            while True:
                ctx._check(be.L.cniic_cc_update(h, C_.byref(changed)))
                iters += 1
                if not changed.value:
                    break
                be.assign(h)
            assert iters == cold["stats"]["iterations"]
        got, _ = finish(be, h, frames, flat_d)
        cent, _ = be.palette(h, K)
    finally:
        be.destroy(h)
        ctx.close()
    assert np.array_equal(cent.astype(np.int32), cold["centroids"])
    assert got == cold_streams


# ------------------------------------------------------------------ cniic_codec_encode_warm
def shifted(seed):
    """two frames of 96 x 64 cut from one image, the second 8 pixels to the right and 4 down: consecutive frames of a pan"""
    big = photo(128, 96, seed)
    return big[0:64, 0:96].copy(), big[4:68, 8:104].copy()


def test_encode_warm_cluster_colors_two_frames(ctx):
    K = 16
    f0, f1 = shifted(50)
    kb, wb = R.colour_points(photo(96, 64, 51))
    rcb, other = O.kmeans(O.PT_RGBW, O.MODE_L, R.pts_of_keys(kb), wb, K)
    assert rcb == 0
    init = other["centroids"].astype(np.uint8)
    for frame in (f0, f1):
        keys, w = R.colour_points(frame)
        rc, ref = R.lloyd_from(O.PT_RGBW, R.pts_of_keys(keys), w, K, init)
        assert rc == 0
        rcg, data, st, cent = ctx.encode_warm("cluster-colors(%d)" % K, frame, init)
        assert rcg == 0 and st["iterations"] == ref["iterations"]
        assert np.array_equal(cent.astype(np.int32), ref["centroids"])
        assert data == R.cc_stream(frame, keys, ref["labels"], ref["centroids"])
        rcd, back = ctx.decode("cluster-colors(%d)" % K, data)
        assert rcd == 0 and np.array_equal(back, R.remap(frame, keys, ref["labels"], ref["centroids"]))
        init = cent   # what the caller passes for the next frame


def test_encode_warm_voronoi_two_frames(ctx):
    K = 32
    f0, f1 = shifted(52)
    rcb, other = O.kmeans(O.PT_XYRGB, O.MODE_L, R.xy_pts(photo(96, 64, 53)), None, K)
    assert rcb == 0
    init = R.colorpos(other["centroids"])
    for frame in (f0, f1):
        rc, ref = R.lloyd_from(O.PT_XYRGB, R.xy_pts(frame), None, K, R.c5_of(init))
        assert rc == 0
        rcg, data, st, cent = ctx.encode_warm("voronoi(%d)" % K, frame, init)
        assert rcg == 0 and st["iterations"] == ref["iterations"]
        assert np.array_equal(R.c5_of(cent), ref["centroids"])
        assert len(data) == 16 + 19 * K and data == R.voronoi_stream(96, 64, ref["centroids"])
        init = cent


def test_encode_warm_takes_only_the_kmeans_codecs_and_reports_capacity(ctx):
    from cniic_amd import _lib
    frame = photo(96, 64, 54)
    init = np.zeros((16, 3), np.uint8)
    for expr in ("delta", "hufman"):
        rc, _, _, _ = ctx.encode_warm(expr, frame, init, allow=(_lib.BAD_ARG,))
        assert rc == _lib.BAD_ARG
    keys, w = R.colour_points(frame)
    init = R.ref_init_centroids(R.pts_of_keys(keys), 16).astype(np.uint8)
    rc, data, st = ctx.encode("cluster-colors(16)", frame)
    assert rc == 0
    small = np.zeros(64, np.uint8)
    rcw, need, _, _ = ctx.encode_warm("cluster-colors(16)", frame, init, out=small, allow=(_lib.CAPACITY,))
    rcc, need_cold, _ = ctx.encode("cluster-colors(16)", frame, out=np.zeros(64, np.uint8), allow=(_lib.CAPACITY,))
    assert rcw == rcc == _lib.CAPACITY and need == need_cold == len(data)
    rcw, warm, stw, _ = ctx.encode_warm("cluster-colors(16)", frame, init)   # from the reference's own init: the cold stream
    assert rcw == 0 and warm == data and stw["iterations"] == st["iterations"]
