"""The exact `hilbert(rle)` encoder (cniic_amd/csrc/k_rle.hip: k_rle_last, k_rle_carry_local, k_rle_carry_add, k_rle_flags, k_rle_offsets /
pack_scan, k_rle_records) at its thread, wave, chunk and scan limits: row images whose colour changes are placed ON the granularities
(tests/rle_exact_edges.py), every stream byte for byte the oracle's.  tests/test_rle_exact_edges_cpu.py asserts beforehand that each case
stands where it claims to and that the table tells a model of these kernels with a mistake at any one handover from the right stream.
A mismatch is reported with the first differing record and the chunk, thread and j its run starts at."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import rle_exact_edges as E

pytestmark = pytest.mark.gpu

CODEC = "hilbert(rle)"
SENTINEL, GUARD = 0xA7, 256


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    with Context(0) as c:
        yield c


def _oracle(img, lin, w, h):
    want = E.stream_np(lin, w, h)   # the length is known before anything is encoded
    rc, data, _ = O.encode(CODEC, img)
    assert rc == 0 and len(data) == len(want) and data == want
    return data


@functools.lru_cache(maxsize=None)
def _expected_small(name):
    img = E.case_image(name)
    return img, _oracle(img, img[0], img.shape[1], 1)


@functools.lru_cache(maxsize=3)
def _expected_large(name):
    img = E.case_image(name)
    return img, _oracle(img, img[0], img.shape[1], 1)


def expected(name):
    """(the row, the oracle's stream), computed once for the small rows and kept for the last three large ones"""
    return (_expected_large if E.BY_NAME[name].n >= E.LARGE else _expected_small)(name)


def _assert_stream(got, want, what):
    assert got == want, (what, E.first_difference(got, want))


@pytest.mark.parametrize("name", E.NAMES)
def test_case_equals_oracle(ctx, name):
    img, want = expected(name)
    rc, data, _ = ctx.encode(CODEC, img)
    assert rc == 0 and len(data) == len(want), (name, len(data), len(want))
    _assert_stream(data, want, name)
    rc, back = ctx.decode(CODEC, data)
    assert rc == 0 and np.array_equal(back, img)


# ------------------------------------------------------------------ buffers
BUFFER_CASES = ["cap_L4335_s_chunk_m255", "block_start_at_m1", "noise_1025_chunks"]   # small, across a block of the carry scan, 1025 chunks


def _device_out(nbytes, shift):
    """nbytes of device memory `shift` bytes behind a 16-byte boundary, a guard behind them, all of it sentinel"""
    import torch
    buf = torch.full((16 + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[shift:shift + nbytes]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("name", BUFFER_CASES)
def test_device_image_and_device_stream_at_every_byte_offset(ctx, name, shift):
    """offset 0 with a capacity that is a multiple of 4 is written in place, the others go through the staging buffer; `slack` bytes of
    capacity beyond the stream must stay as they were, as must everything before and behind the buffer"""
    import torch
    img, want = expected(name)
    n = img.shape[1]
    src = torch.from_numpy(np.array(img)).cuda()
    for slack in (0, 4, 5):
        buf, out = _device_out(len(want) + slack, shift)
        torch.cuda.synchronize()
        rc, ln, _ = ctx.encode(CODEC, src, w=n, h=1, out=out)
        got = buf.cpu().numpy()
        assert rc == 0 and ln == len(want), (name, shift, slack)
        _assert_stream(got[shift:shift + ln].tobytes(), want, (name, shift, slack))
        assert (got[:shift] == SENTINEL).all() and (got[shift + ln:] == SENTINEL).all(), (name, shift, slack, "a write outside the stream")


@pytest.mark.parametrize("name", BUFFER_CASES)
def test_device_image_at_an_odd_address(ctx, name):
    import torch
    img, want = expected(name)
    n = img.shape[1]
    for shift in (1, 3):
        raw = torch.zeros(16 + 3 * n, dtype=torch.uint8, device="cuda")
        assert raw.data_ptr() % 16 == 0
        raw[shift:shift + 3 * n] = torch.from_numpy(np.array(img).reshape(-1)).cuda()
        torch.cuda.synchronize()
        rc, data, _ = ctx.encode(CODEC, raw[shift:shift + 3 * n], w=n, h=1)
        assert rc == 0
        _assert_stream(data, want, (name, shift))


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("name", BUFFER_CASES)
def test_capacity_one_byte_short_then_the_retry(ctx, name, on_dev):
    from cniic_amd import _lib
    img, want = expected(name)
    if on_dev:
        buf, out = _device_out(len(want), 0)
    else:
        buf = np.full(len(want) + GUARD, SENTINEL, np.uint8)
        out = buf[:len(want)]
    rc, need, _ = ctx.encode(CODEC, img, out=out[:len(want) - 1], allow=(_lib.CAPACITY,))
    got = buf.cpu().numpy() if on_dev else buf
    assert rc == _lib.CAPACITY and need == len(want)
    assert (got[len(want) - 1:] == SENTINEL).all(), "a write past the capacity"
    rc, ln, _ = ctx.encode(CODEC, img, out=out[:need])
    got = buf.cpu().numpy() if on_dev else buf
    assert rc == 0 and ln == need
    _assert_stream(got[:ln].tobytes(), want, name)
    assert (got[ln:] == SENTINEL).all()


# ------------------------------------------------------------------ the same run structure through the real scan
@pytest.mark.parametrize("w,h,starts", [(600, 460, (5, 66 * E.CHUNK + 9)),                             # carry65_from5: 65 whole chunks without a start
                                        (2100, 2004, (E.BLOCK - 1, E.BLOCK - 1 + 3 * E.CHUNK))])      # block_start_at_m1: into the next block
def test_carry_cases_as_images_along_the_real_scan(ctx, w, h, starts):
    """a w x h image that is flat along the Hilbert scan apart from the same changes: the linearising kernel in front of the same kernels"""
    n = w * h
    lin = E.row(n, starts)[0]
    assert E.segment_starts_np(lin).tolist() == [0] + list(starts)
    xy = O.hilbert_iter(w, h).astype(np.int64)
    img = np.zeros((h, w, 3), np.uint8)
    img[xy[:, 1], xy[:, 0]] = lin
    want = _oracle(img, lin, w, h)
    rc, data, _ = ctx.encode(CODEC, img)
    assert rc == 0 and len(data) == len(want)
    _assert_stream(data, want, (w, h))
    rc, back = ctx.decode(CODEC, data)
    assert rc == 0 and np.array_equal(back, img)


# ------------------------------------------------------------------ route and state
def test_cases_back_to_back_on_one_context():
    """the plan's scratch (chunk_last, carry, blockmax, flags, run offsets) comes from the context's pool, which hands the same memory to
    the next call: a kernel that reads an entry it did not write this call gets the other case's.  Each pair, then the first again."""
    from cniic_amd import Context
    pairs = [("block_without_a_start_far", "noise_1025_chunks"),     # two blocks of the carry scan and pack_scan, with and without starts in every chunk
             ("blocks_all_flat", "block_start_at_0"),
             ("alternating_2_chunks", "cap_L4335_s_chunk_m255"),      # the single-block offsets
             ("carry66_from_chunk3_last", "tiny_1_flat")]
    with Context(0) as c:
        for a, b in pairs:
            for name in (a, b, a):
                img, want = expected(name)
                rc, data, _ = c.encode(CODEC, img)
                assert rc == 0
                _assert_stream(data, want, (a, b, name))
