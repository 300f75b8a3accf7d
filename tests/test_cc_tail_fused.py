"""The back end of a cluster-colors encode through the pixel partition (cniic_amd/csrc/k_points.hip, codec.cpp: cc_finish): for narrow
labels k_sp_pixpack picks every pixel's label and packs it in one kernel, the chunks' first bits from a ticketed look-back, the codes,
lengths and header read from one pinned block of the host's.

Everything runs with CNIIC_SP_MIN_PIXELS = 0.  The witness of every case is the route the library took before -- k_sp_pixlab, then the
label pack's three passes -- which CNIIC_TEST_CC_TAIL=split forces, and the oracle (mode L): bytes, length and statistics equal.
The encodes that are to take the new kernel run under CNIIC_TEST_CC_TAIL=require (the autouse fixture): the library then answers an
error where it would hand over to the split kernels silently (a header that does not fit the pinned block, a look-back given up), so
no case can pass by comparing the split route with itself.
CNIIC_TEST_CC_TAIL_GIVEUP=1 makes every block of k_sp_pixpack that polls a look-back word give up at its first poll, without waiting:
the host must then pack with the split kernels from the labels in partition order."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

CHUNK = 1 << 16   # pixels of a partition chunk, a block of k_sp_pixpack


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def partition_route(monkeypatch):
    monkeypatch.setenv("CNIIC_SP_MIN_PIXELS", "0")
    monkeypatch.setenv("CNIIC_TEST_CC_TAIL", "require")


def photo(w, h, seed=0):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + 50 + seed)


def poster(w, h, ncol, seed):
    """ncol random colours, some common and most rare (codes of many lengths), scattered over the image: few points for the K-means"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (ncol, 3)).astype(np.uint8)
    lab = np.minimum(rng.exponential(ncol / 6.0, w * h).astype(np.int64), ncol - 1)
    return pal[lab].reshape(h, w, 3)


_oracle = {}


def oracle(name, img, K):
    if (name, K) not in _oracle:
        rc, data, st = O.encode("cluster-colors(%d)" % K, img, mode=O.MODE_L)
        assert rc == 0
        _oracle[(name, K)] = (data, st)
    return _oracle[(name, K)]


def split(ctx, monkeypatch, img, K, **kw):
    with monkeypatch.context() as m:
        m.setenv("CNIIC_TEST_CC_TAIL", "split")
        return ctx.encode("cluster-colors(%d)" % K, img, **kw)


def three_ways(ctx, monkeypatch, name, img, K):
    """fused, split and the oracle: the same stream, length and statistics"""
    rc, data, st = ctx.encode("cluster-colors(%d)" % K, img)
    rcs, sdata, sst = split(ctx, monkeypatch, img, K)
    edata, est = oracle(name, img, K)
    assert rc == rcs == 0
    assert len(data) == len(sdata) == len(edata)
    assert data == sdata and data == edata
    assert st == sst
    for f in ("iterations", "moved_last", "empty_reseeds"):
        assert st[f] == est[f], f
    return data


# ---- the edges of a chunk: one full chunk less a pixel, exactly one, a second chunk of one pixel, a ragged last group; no width a multiple of 16
@pytest.mark.parametrize("w,h", [(255, 257), (8, 8192), (65537, 1), (300, 437)])
def test_chunk_edges(ctx, monkeypatch, w, h):
    assert w % 16 and w * h in (CHUNK - 1, CHUNK, CHUNK + 1, 131100)
    three_ways(ctx, monkeypatch, "edge%dx%d" % (w, h), photo(w, h), 16)


def test_forty_chunks_look_back_beyond_one_hop(ctx, monkeypatch):
    three_ways(ctx, monkeypatch, "40chunks", poster(2560, 1024, 3000, 1), 32)


@pytest.mark.parametrize("K", [2, 255, 256])
def test_edges_of_k(ctx, monkeypatch, K):
    three_ways(ctx, monkeypatch, "photo160x128", photo(160, 128, 3), K)


def test_one_cluster_one_symbol_empty_payload(ctx, monkeypatch):
    """K = 1: a tree of one symbol, codes of 0 bits, no payload behind the header"""
    img = photo(160, 128, 3)
    data = three_ways(ctx, monkeypatch, "onecluster", img, 1)
    rc, back = ctx.decode("cluster-colors(1)", data)
    assert rc == 0 and np.unique(back.reshape(-1, 3), axis=0).shape[0] == 1


@pytest.mark.parametrize("words", ["3", "40"])
def test_rounds_that_go_straight_to_memory(ctx, monkeypatch, words):
    """CNIIC_TEST_PACK_IMG_WORDS: the LDS bit image holds next to nothing, every round of every chunk takes the direct route (both packs)"""
    monkeypatch.setenv("CNIIC_TEST_PACK_IMG_WORDS", words)
    three_ways(ctx, monkeypatch, "photo300x260", photo(300, 260, 2), 64)


def fibonacci_blobs(w, h, n):
    """n colours whose pixel counts are 1, 1, 2, 3, 5, ... and the rest: a Huffman tree that is one chain, the longest code n - 1 bits"""
    f = [1, 1]
    while len(f) < n - 1:
        f.append(f[-1] + f[-2])
    counts = f[:n - 1]
    rest = w * h - sum(counts)
    assert rest >= f[n - 2] + f[n - 3] - 1   # (the last colour is merged last)
    counts.append(rest)
    i = np.arange(n)
    pal = np.stack([(i * 7) % 256, (i * 37 + 11) % 256, (i * 101 + 3) % 256], axis=1).astype(np.uint8)
    return pal[np.repeat(i, counts)].reshape(h, w, 3)


def test_codes_longer_than_32_bits(ctx, monkeypatch):
    img = fibonacci_blobs(3900, 3840, 34)
    edata, _ = oracle("fib34", img, 34)
    rcd, back = O.decode("cluster-colors(34)", edata)[:2]
    assert rcd == 0
    p = back.reshape(-1, 3).astype(np.uint32)
    _, cnt = O.count_freqs((p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2])
    lens, _ = O.huf_build(cnt)
    assert int(lens.max()) >= 33   # (what the oracle's decoder was built from: the histogram of the reduced image)
    three_ways(ctx, monkeypatch, "fib34", img, 34)


@pytest.mark.parametrize("dest", ["device", "device+1", "host"])
def test_destinations(ctx, monkeypatch, dest):
    import torch
    img = photo(300, 437)
    edata, _ = oracle("edge300x437", img, 16)
    if dest == "host":
        out = np.full(len(edata) + 64, 0xAB, np.uint8)
    else:
        buf = torch.full((len(edata) + 80,), 0xAB, dtype=torch.uint8, device="cuda:0")
        out = buf if dest == "device" else buf[1:]
        assert out.data_ptr() % 4 == (0 if dest == "device" else 1)
    rc, n, st = ctx.encode("cluster-colors(16)", img, out=out)
    got = (out if dest == "host" else out.cpu().numpy())
    assert rc == 0 and n == len(edata) and got[:n].tobytes() == edata


def test_capacity_one_byte_short_leaves_the_output_alone(ctx, monkeypatch):
    import torch
    from cniic_amd import _lib
    img = photo(300, 437)
    edata, _ = oracle("edge300x437", img, 16)
    out = torch.full((len(edata) - 1,), 0xAB, dtype=torch.uint8, device="cuda:0")
    rc, n, st = ctx.encode("cluster-colors(16)", img, out=out, allow=(_lib.CAPACITY,))
    torch.cuda.synchronize()
    assert rc == _lib.CAPACITY
    assert bool((out == 0xAB).all())


@pytest.mark.parametrize("w,h", [(300, 437), (2560, 1024)])
def test_give_up_hands_over_to_the_split_kernels(ctx, monkeypatch, w, h):
    img = poster(w, h, 3000, 1) if w == 2560 else photo(w, h)
    K = 32 if w == 2560 else 16
    rcs, sdata, sst = split(ctx, monkeypatch, img, K)
    monkeypatch.setenv("CNIIC_TEST_CC_TAIL_GIVEUP", "1")
    from cniic_amd import _lib
    rc, _, _ = ctx.encode("cluster-colors(%d)" % K, img, allow=(_lib.HIP,))
    assert rc == _lib.HIP   # (under `require` the hand-over is an error: the hook does reach the kernel)
    monkeypatch.delenv("CNIIC_TEST_CC_TAIL")
    rc, data, st = ctx.encode("cluster-colors(%d)" % K, img)
    assert rc == rcs == 0 and data == sdata and st == sst


def test_alternating_images_rezero_ticket_and_words(monkeypatch):
    """eight encodes on one context, two images of different chunk counts in turn"""
    from cniic_amd import Context
    a, b = photo(300, 437), poster(700, 600, 1000, 4)
    c = Context(0)
    try:
        want = [split(c, monkeypatch, im, 24) for im in (a, b)]
        assert all(rc == 0 for rc, _, _ in want) and want[0][1] != want[1][1]
        for turn in range(8):
            rc, data, st = c.encode("cluster-colors(24)", (a, b)[turn & 1])
            assert rc == 0 and data == want[turn & 1][1] and st == want[turn & 1][2], turn
    finally:
        c.close()


def test_shared_palette_one_rank(monkeypatch):
    """cniic_cc_image_begin ... cniic_cc_finish: the weights of the clusters from this image's own colour counts"""
    import torch
    from cniic_amd import Context
    from cniic_amd.dist import ShardedClusterColors
    dev = torch.device("cuda", 0)
    img = photo(300, 437)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    c = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        t = torch.from_numpy(img).to(dev)
        sh = ShardedClusterColors(c, 16, None, dev)
        outs = []
        for tail in ("split", "require"):
            with monkeypatch.context() as m:
                m.setenv("CNIIC_TEST_CC_TAIL", tail)
                out = torch.zeros(300 * 437 * 4 + (1 << 16), dtype=torch.uint8, device=dev)
                n, st = sh.encode(t, 300, 437, out)
                torch.cuda.synchronize()
                outs.append((out[:n].cpu().numpy().tobytes(), st))
        sh.close()
        assert outs[0] == outs[1] and len(outs[0][0]) > 8
    finally:
        c.close()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def test_persistent_loop_against_the_launches(ctx, monkeypatch):
    """the K-means as one launch (its verdict read with the result block) and as a launch per iteration, in front of the same tail"""
    from cniic_amd import _lib
    img = photo(300, 260, 2)
    monkeypatch.setenv("CNIIC_KM_PS_REQUIRE", "1")
    rc, data, st = ctx.encode("cluster-colors(64)", img)
    ctx.set_opt(_lib.OPT_KM_LOOP, 1)
    try:
        rcl, ldata, lst = ctx.encode("cluster-colors(64)", img)
    finally:
        ctx.set_opt(_lib.OPT_KM_LOOP, None)
    assert rc == rcl == 0 and data == ldata
    for f in ("iterations", "moved_last", "empty_reseeds", "active"):
        assert st[f] == lst[f], f
    assert data == oracle("photo300x260", img, 64)[0]


def test_abort(ctx, monkeypatch):
    """a persistent launch that gives up at its first barrier: the launches run, the result is fetched again and the labels enqueued again"""
    img = photo(300, 260, 2)
    want = oracle("photo300x260", img, 64)[0]
    monkeypatch.setenv("CNIIC_TEST_PS_ABORT_AT", "1")
    rc, data, st = ctx.encode("cluster-colors(64)", img)
    assert rc == 0 and data == want
    monkeypatch.delenv("CNIIC_TEST_PS_ABORT_AT")
    rc, data, st = ctx.encode("cluster-colors(64)", img)
    assert rc == 0 and data == want
