"""The small-frame `delta` route (k_delta_small.hip, one workgroup per frame) and the copy kernel it shares with the cluster-colors route
(k_cc_small_place) at the limits they are built around.  The frames are those of tests/delta_small_edges.py; that each one reaches the
limit it is named for -- the 19-bit code, full and weight-cut merge runs in both queues, both general orders, 16 384 leaves, the weight
16 384 in a 16-bit slot -- is proved without a GPU in tests/test_delta_small_edges_cpu.py.  Here the kernels run on them:

  * every input alone (the launch's LDS capacity is then its own size rounded up), all in one launch, and with the route off;
  * a round trip through cniic_codec_measure_batch at the code-length bound;
  * one call that delta_small_encode splits into two chunks of scratch;
  * streams placed at every alignment of the destination, from scratch offsets of every residue modulo 4, for both routes.

Every comparison is exact: bytes, lengths, statuses and statistics are those of cniic_codec_encode_opts on a context that has seen no
batch and, for every frame of the first three groups, the oracle's."""
import numpy as np
import pytest

import delta_small_edges as E
import test_delta_small_batch as T
from test_delta_small_batch import _pack, batch, check_against_singles, singles

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _want():
    want = singles("edges", "delta", E.images())
    assert all(s[0] == 0 for s in want)
    return want


def _check_all(res, names, want, launches, what):
    """one call's result against the singles, the oracle and CLAIMS, frame by frame"""
    check_against_singles(res, want, what)
    assert res[0] == 0 and res[6] == launches, (what, res[0], res[6], launches)
    for f, name in enumerate(names):
        assert res[2][f] == 0 and res[4][f] == E.oracle_stream(name), (what, name)
        assert res[1][f] == E.CLAIMS[name][2], (what, name, res[1][f])


_WAYS = {}


def _way(which, monkeypatch):
    """the 32 inputs (a) each as a batch of one, (b) all in one batch, (c) all in one batch with the route off -> per frame (rc, length, bytes, stats)"""
    import cniic_amd
    if which not in _WAYS:
        want = _want()
        stride = T._stride(want)
        rows = []
        with cniic_amd.Context(0) as ctx:
            if which == "alone":
                for f, name in enumerate(E.NAMES):
                    res = batch(ctx, "delta", [E.image(name)], stride, poison=POISON)
                    _check_all(res, [name], want[f:f + 1], 1, "alone: " + name)
                    assert bool((res[5][res[1][0]:] == POISON).all()), name
                    rows.append((res[2][0], res[1][0], res[4][0], res[3][0]))
            else:
                if which == "off":
                    monkeypatch.setenv("CNIIC_TEST_DELTA_SMALL_OFF", "1")
                res = batch(ctx, "delta", E.images(), stride, poison=POISON)
                if which == "off":
                    monkeypatch.delenv("CNIIC_TEST_DELTA_SMALL_OFF")
                _check_all(res, E.NAMES, want, 0 if which == "off" else len(E.NAMES), which)
                for f in range(len(E.NAMES)):
                    # (the single-image encoder the workers run packs whole words inside the frame's room: only the route leaves the rest alone)
                    assert which == "off" or bool((res[5][f * stride + res[1][f]:(f + 1) * stride] == POISON).all()), (which, E.NAMES[f])
                    rows.append((res[2][f], res[1][f], res[4][f], res[3][f]))
        _WAYS[which] = rows
    return _WAYS[which]


def test_every_input_alone_in_its_own_launch(monkeypatch):
    """cap_px is the frame's own size rounded up to a power of two: 16384 pixels fill the LDS arrays exactly, 63 / 64 / 65 stand around kDsMinCap"""
    _way("alone", monkeypatch)


def test_all_inputs_in_one_launch(monkeypatch):
    _way("company", monkeypatch)


def test_all_inputs_with_the_route_off(monkeypatch):
    _way("off", monkeypatch)


def test_the_three_ways_agree(monkeypatch):
    a, b, c = (_way(w, monkeypatch) for w in ("alone", "company", "off"))
    assert a == b == c
    assert [r[1] for r in a] == [E.CLAIMS[name][2] for name in E.NAMES]


def test_round_trip_at_the_code_length_bound():
    """19-bit codes through k_hdecode as well: encode, decode, MSE and the lossless check of cniic_codec_measure_batch"""
    import torch
    import cniic_amd
    from cniic_amd import _lib
    names = ("chain19", "all_distinct", "stairs", "flat128")
    imgs = E.images(names)
    buf, offs, ws, hs = _pack(imgs)
    stride = T._round4(max(E.CLAIMS[nm][2] for nm in names)) + 8
    with cniic_amd.Context(0) as ctx:
        src = torch.from_numpy(buf).to(torch.device("cuda", 0))
        out = torch.full((stride * len(names),), POISON, dtype=torch.uint8, device=src.device)
        torch.cuda.synchronize()
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
        rc, rows, lens = ctx.measure_batch("delta", src, offs, ws, hs, out, stride, allow=T.FAILURES)
        launches = ctx.kernel_time(T.TIMER)[1]
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
        assert rc == 0 and launches == len(names)
        host = out.cpu().numpy()
        for f, name in enumerate(names):
            want = E.oracle_stream(name)
            npx = imgs[f].shape[0] * imgs[f].shape[1]
            assert rows[f]["rc"] == 0 and rows[f]["error"] == 0.0 and rows[f]["lossless_mismatch"] == 0, (name, rows[f])
            assert rows[f]["compressed_size"] == len(want) == lens[f] and rows[f]["compression_ratio"] == len(want) / (npx * 24.0) * 100.0, (name, rows[f])
            assert host[f * stride:f * stride + lens[f]].tobytes() == want, name
            assert bool((host[f * stride + lens[f]:(f + 1) * stride] == POISON).all()), name
            rc2, back = ctx.decode("delta", want)
            assert rc2 == 0 and np.array_equal(back, imgs[f]), name


# ------------------------------------------------------------------ two chunks of scratch in one call
def test_one_call_in_two_chunks():
    """delta_small_encode gives every chunk at most 2 GiB of scratch under the slot of its first (largest) frame.  Behind one 128 x 128 frame
    that is chunk_frames(16384) frames; the call has more, so the smallest ones make a second chunk, sized by a frame of 5 pixels"""
    import cniic_amd
    import oracle_lib as O
    first = E.chunk_frames(E.MAX_PX)
    further = sum(E.TINY_COUNT)
    assert further == 5900 and sum(E.TINY_COUNT[4:]) < 1 + further - first <= sum(E.TINY_COUNT[3:])   # the second chunk begins among the 5-pixel frames
    assert 1 + further - first < E.chunk_frames(E.TINY[3][0] * E.TINY[3][1])                          # ... and is the last one
    kinds = E.chunk_kinds()
    which = np.concatenate([[0], 1 + np.random.default_rng(E.SEED + 101).permutation(np.repeat(np.arange(len(E.TINY)), E.TINY_COUNT))]).tolist()
    imgs = [kinds[k] for k in which]
    want = singles("chunks", "delta", kinds)
    assert all(s[0] == 0 for s in want) and [s[1] for s in want] == [O.encode("delta", im)[1] for im in kinds]
    stride = T._stride(want)
    with cniic_amd.Context(0) as ctx:
        rc, lens, rcs, sts, streams, host, launches, msg = batch(ctx, "delta", imgs, stride, poison=POISON)
        assert ctx.kernel_time("delta_small_place")[1] == 2      # one copy launch per chunk
    assert rc == 0 and launches == 1 + further and rcs == [0] * len(imgs), (rc, launches, msg)
    assert lens == [len(want[k][1]) for k in which]
    rows = host.reshape(len(imgs), stride)
    for k in range(len(kinds)):     # every stream is its single's, and nothing is written behind any stream
        mine = rows[np.array(which) == k]
        n = len(want[k][1])
        assert bool((mine[:, :n] == np.frombuffer(want[k][1], np.uint8)).all()) and bool((mine[:, n:] == POISON).all()), k


# ------------------------------------------------------------------ placement at every alignment
def _placement_plan(lens, stride, out_off):
    """per frame, as k_cc_small_place splits it: (dst % 16, head, 16-byte stores, tail bytes, (scratch slot + head) % 4 -- the slot is 16-byte aligned)"""
    plan = []
    for f, n in enumerate(lens):
        dst = (out_off + f * stride) % 16
        head = min(n, (16 - dst) % 16)
        body = (n - head) // 16
        plan.append((dst, head, body, n - head - 16 * body, head % 4))
    return plan


def _check_placed(res, stride, F):
    (whole, at), lens, rcs = res[5], res[1], res[2]
    assert bool((whole[:at] == POISON).all()) and bool((whole[at + F * stride:] == POISON).all())     # before the first stream, behind the last slot
    for f in range(F):
        n = lens[f] if rcs[f] == 0 else 0
        assert bool((whole[at + f * stride + n:at + (f + 1) * stride] == POISON).all()), f          # between the streams


@pytest.mark.parametrize("out_off,host_out", ((1, False), (14, False), (7, True)))
def test_delta_streams_placed_at_every_alignment(out_off, host_out):
    """odd stride, the output pointer off its 16-byte boundary: every destination residue, every shift of the aligned source words; the stream
    that is all head (15 bytes at residue 1: no stream is shorter), bodies of exactly one store, tails of 1 .. 15 bytes"""
    import cniic_amd
    import oracle_lib as O
    kinds = E.placement_kinds()
    want1 = singles("placement", "delta", kinds)
    assert [s[1] for s in want1] == [O.encode("delta", im)[1] for im in kinds]
    assert len(kinds) == 7 and all(s[0] == 0 for s in want1) and tuple(len(s[1]) for s in want1) == E.PLACEMENT_LENGTHS
    F = 16 * len(kinds)
    imgs, want = [kinds[f % 7] for f in range(F)], [want1[f % 7] for f in range(F)]
    stride = (max(len(s[1]) for s in want1) + 8) | 1
    plan = _placement_plan([len(s[1]) for s in want], stride, out_off)
    assert {p[0] for p in plan} == set(range(16))
    assert {p[4] for p in plan if p[2] >= 1} == {0, 1, 2, 3}                 # the shifted source words: (slot + head) % 4 = 1, 2, 3
    assert any(p[1] == n and p[1] > 0 for p, n in zip(plan, (len(s[1]) for s in want)))      # all head
    assert any(p[2] == 0 and p[3] > 0 for p in plan) and any(p[2] == 1 for p in plan) and {p[3] for p in plan} >= set(range(1, 16))
    assert all(any(p[2] == 1 and p[4] == r for p in plan) for r in (1, 2, 3))   # one store, shifted: its fifth word is the last the stream has
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, "delta", imgs, stride, host_out=host_out, poison=POISON, out_off=out_off)
    assert res[6] == F and res[0] == 0
    check_against_singles(res, want, "placement %d" % out_off)
    _check_placed(res, stride, F)


@pytest.mark.parametrize("K", (2, 16))
def test_cluster_colors_streams_placed_at_every_alignment(K):
    """the same kernel behind the cluster-colors route"""
    import cniic_amd
    import test_cc_small_batch as C
    expr = "cluster-colors(%d)" % K
    cand = C.further_images() + C.shaped_images()[3:6]       # flat, checkerboard, 256 colours, grey ramp, 7 x 9, 64 x 64, 100 x 75
    got = C.singles(("placement", K), expr, cand)
    kinds = [f for f in range(len(cand)) if got[f][0] == 0]
    kinds = kinds[:len(kinds) - (len(kinds) + 1) % 2]       # an odd number: with 16 m frames every kind meets every residue
    assert len(kinds) >= 3
    m = len(kinds)
    F = 16 * m
    imgs, want = [cand[kinds[f % m]] for f in range(F)], [got[kinds[f % m]] for f in range(F)]
    stride = (max(len(s[1]) for s in want) + 8) | 1
    out_off = 5
    plan = _placement_plan([len(s[1]) for s in want], stride, out_off)
    assert {p[0] for p in plan} == set(range(16)) and {p[4] for p in plan if p[2] >= 1} == {0, 1, 2, 3}
    assert {p[3] for p in plan} >= set(range(1, 16))
    with cniic_amd.Context(0) as ctx:
        res = batch(ctx, expr, imgs, stride, poison=POISON, out_off=out_off, timer="cc_small_batch")
    assert res[6] == F and res[0] == 0
    C.check_against_singles(res, want, "placement " + expr)
    _check_placed(res, stride, F)
