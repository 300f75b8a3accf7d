"""A context owns what it creates (csrc/common.hpp: PinnedBuf, Event, DevPool, ~Ctx): closing it gives the device its memory back, and a
batch call whose frame fails reports that frame's own message, whichever worker ran it and whatever that worker did afterwards."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _one_context_round():
    """every kind of resource a context creates lazily, then close"""
    from cniic_amd import Context
    img = _noise(64, 64, 1)
    frames = np.stack([_noise(32, 32, 10 + f) for f in range(3)])
    with Context(0) as ctx:
        # `delta`: the 2^27-entry table and its page flags (512 MiB + 32 KiB, outside the pool), the Hilbert tables, pinned_huf, huf_ev
        rc, data, _ = ctx.encode("delta", img)
        assert rc == 0
        rc, back = ctx.decode("delta", data)
        assert rc == 0 and np.array_equal(back, img)
        # cluster-colors: `dense` through the pool, pinned_res / res_ev, pinned_u
        rc, data, _ = ctx.encode("cluster-colors(16)", img)
        assert rc == 0 and data
        # three frames: three worker contexts
        stride = 32 * 32 * 16 + 4096
        out = np.zeros(3 * stride, np.uint8)
        rc, lens, rcs, _ = ctx.encode_batch("hufman", frames, 32, 32, 3, out, stride)
        assert rc == 0 and rcs == [0, 0, 0] and all(lens)


def test_contexts_give_their_memory_back():
    """One warm-up round, then five rounds of open / use / close.  Free device memory after round 5 is at least what it was after round 1
    minus 256 MiB: one `delta` table that a close left behind costs 512 MiB a round, 2.5 GiB over the five, and 256 MiB is half of one
    table (smaller, transient differences are not this test's business).  The device is shared: when free memory moves by more than
    64 MiB in half a second with nothing of ours running, the reading means nothing and the test is skipped."""
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    _one_context_round()   # warm-up: the runtime's own pools, code objects, torch's context
    a = free()
    time.sleep(0.5)
    b = free()
    if abs(a - b) > 64 * MIB:
        pytest.skip("free device memory moved by %d MiB in 0.5 s with nothing of ours running: somebody else is on the device" % (abs(a - b) // MIB))
    after = []
    for _ in range(5):
        _one_context_round()
        after.append(free())
    print("free MiB after rounds 1..5:", [x // MIB for x in after])
    assert after[4] >= after[0] - 256 * MIB, [x // MIB for x in after]


@pytest.mark.parametrize("streams", [1, 3])
def test_encode_batch_reports_the_first_failing_frame(streams):
    """Frame 0 is one colour: a single point for 16 clusters, TOO_FEW_POINTS.  With one worker that worker goes on to frames 1 and 2, and its
    next call clears its message: the batch call must have kept frame 0's."""
    from cniic_amd import Context, _lib
    w = h = 32
    frames = np.stack([_noise(w, h, 20 + f) for f in range(3)])
    frames[0] = 77
    expr = "cluster-colors(16)"
    with Context(0) as ctx:
        single = []
        for f in range(3):
            rc, data, _ = ctx.encode(expr, frames[f], allow=(_lib.TOO_FEW_POINTS,))
            single.append((rc, data, (ctx._L.cniic_last_error(ctx.h) or b"").decode()))
        assert single[0][0] == _lib.TOO_FEW_POINTS and single[0][2] and single[1][0] == 0 and single[2][0] == 0
        ctx.set_opt(_lib.OPT_BATCH_STREAMS, streams)
        stride = w * h * 16 + 4096
        out = np.zeros(3 * stride, np.uint8)
        rc, lens, rcs, _ = ctx.encode_batch(expr, frames, w, h, 3, out, stride, allow=(_lib.TOO_FEW_POINTS,))
        msg = (ctx._L.cniic_last_error(ctx.h) or b"").decode()
        assert rc == _lib.TOO_FEW_POINTS
        assert rcs == [_lib.TOO_FEW_POINTS, 0, 0]
        assert msg == single[0][2], (msg, single[0][2])
        for f in (1, 2):
            assert out[f * stride:f * stride + lens[f]].tobytes() == single[f][1], f
