"""The GPU parse of a serialised Huffman decoder (cniic_amd/csrc/k_trieparse.hip: chunk maps -> their composition -> node records -> right
children through 64-way minima -> leaf codes) on tries built by hand to sit on its limits (tests/trie_shapes.py), and the codes of up to 56
bits it makes through the parallel payload decoder (k_hdecode.hip).  Every comparison is exact: the return code, every pixel -- known from
the payload alone for `hufman`, the oracle's for `delta` and for edited streams -- and WHICH parse answered, read from the stage marks
"trie_parse" (the GPU's table decoded the payload) and "trie_parse_host" (the stream was handed to the host's node walk): a parser that
hands everything back decodes every image and fails every case here.

Each good stream is decoded from host bytes (decode) and from device bytes (decode_into), under CNIIC_TEST_TRIE_GPU=1 with
OPT_GPU_DECODE_MIN = 0 and, where the stream meets the gate of codec_decode by itself (a decoder longer than max(nbytes / 48, 8192) bytes,
at least 2^14 pixels, `hufman`), once more with no hook at all: there trie_parse == 1 proves the gate as well.

tests/test_trie_shapes_cpu.py establishes without a GPU what every stream is and that it sits where its name says.  No GPU code is imported
at the top."""
import numpy as np
import pytest

import oracle_lib as O
import trie_shapes as S

pytestmark = pytest.mark.gpu

DECODE = -6


@pytest.fixture(scope="module")
def env():
    import torch
    import cniic_amd
    from cniic_amd import _lib
    ctx = cniic_amd.Context(0)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    yield ctx, torch, torch.device("cuda", 0)
    ctx.close()


def stage(ctx, name):
    """launches of a stage of the last call, None when there is no such stage"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = ctx._L.cniic_last_kernel_time(ctx.h, name.encode(), None, C.byref(n))
    return int(n.value) if rc == 0 else None


def upload(env, data):
    ctx, torch, dev = env
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    return t


def decode(env, codec, data, w, h, device=None, nbytes=None):
    """one cniic_codec_decode: of the host bytes `data`, or of the first nbytes of the device tensor `device`
    -> (rc, pixels or None, launches of trie_parse, of trie_parse_host)"""
    ctx, torch, dev = env
    if device is None:
        rc, px = ctx.decode(codec, data, allow=(DECODE,))
    else:
        out = torch.zeros(w * h * 3 + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rc, dw, dh = ctx.decode_into(codec, device, len(data) if nbytes is None else nbytes, out, allow=(DECODE,))
        px = None
        if rc == 0:
            assert (dw, dh) == (w, h) and not out[w * h * 3:].any()                 # nothing behind the image
            px = out[:w * h * 3].cpu().numpy().reshape(h, w, 3)
    return rc, (px if rc == 0 else None), stage(ctx, S.PARSE), stage(ctx, S.PARSE_HOST)


class Hook:
    """CNIIC_TEST_TRIE_GPU=1 and OPT_GPU_DECODE_MIN = 0: every decoder through k_trieparse.hip whatever its size"""

    def __init__(self, env, monkeypatch, on=True, **more):
        self.ctx, self.mp, self.on, self.more = env[0], monkeypatch, on, more

    def __enter__(self):
        from cniic_amd import _lib
        if self.on:
            self.mp.setenv("CNIIC_TEST_TRIE_GPU", "1")
            self.ctx.set_opt(_lib.OPT_GPU_DECODE_MIN, 0)
        for k, v in self.more.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        from cniic_amd import _lib
        self.ctx.set_opt(_lib.OPT_GPU_DECODE_MIN, None)
        self.mp.delenv("CNIIC_TEST_TRIE_GPU", raising=False)
        for k in self.more:
            self.mp.delenv(k, raising=False)


_ORACLE = {}


def expected(name, s):
    if s.image is not None:
        return s.image
    if name not in _ORACLE:
        rc, px = O.decode(s.codec, s.data)
        assert rc == 0, name
        _ORACLE[name] = px
    return _ORACLE[name]


def check_good(env, monkeypatch, name, s, natural=True, **knobs):
    """the four decodes of a good stream (two where it does not meet the natural gate): rc 0, the expected pixels, the parse that answered"""
    want = expected(name, s)
    dev_bytes = upload(env, s.data)
    ran = 0
    for hook in (False, True) if natural and s.natural else (True,):
        with Hook(env, monkeypatch, hook, **knobs):
            for device in (None, dev_bytes):
                rc, px, parsed, handed = decode(env, s.codec, s.data, s.w, s.h, device)
                what = (name, "hook" if hook else "natural gate", "host bytes" if device is None else "device bytes", knobs)
                assert rc == 0, what
                assert np.array_equal(px, want), what
                if s.on_gpu:
                    assert parsed == 1 and not handed, (what, parsed, handed)          # the GPU's table answered
                else:
                    assert not parsed and handed == 1, (what, parsed, handed)          # tried on the GPU, handed to the host's walk
                ran += 1
    return ran


def _group(env, monkeypatch, cases, names, **kw):
    assert names
    return sum(check_good(env, monkeypatch, n, cases[n], **kw) for n in names)


# ------------------------------------------------------------------ `hufman`: chunk geometry
def test_records_across_a_chunk_boundary_at_every_entry_offset(env, monkeypatch):
    g = S.geometry_cases()
    ran = _group(env, monkeypatch, g, [n for n in g if n.startswith("entry")])
    assert ran == 13 * 2 + 13 * 4


def test_tries_that_end_on_and_around_a_chunk_boundary(env, monkeypatch):
    g = S.geometry_cases()
    ran = _group(env, monkeypatch, g, [n for n in g if n.startswith("end")])
    assert ran == 14 * 2 + 2 * sum(13 * n - 1 + 8 > 8192 for n in S.END_LEAVES + (708, 710))


def test_tries_shorter_than_a_chunk(env, monkeypatch):
    g = S.geometry_cases()
    assert _group(env, monkeypatch, g, ["short %d leaves" % n for n in (1, 2, 78, 79)]) == 8


def test_spans_of_1024_1025_8192_and_8193_chunks(env, monkeypatch):
    """one chunk per thread of k_tp_chain_entries, two, eight (one batch of loads) and nine; one block of k_tp_bases_* and two; zeros and
    ones behind the payload are never part of the trie"""
    c = S.chunk_count_cases()
    assert _group(env, monkeypatch, c, list(c)) == 9 * 2 + 4 * 2


# ------------------------------------------------------------------ `hufman`: the right-child search
def test_right_children_at_64_4096_and_262144(env, monkeypatch):
    c = S.search_cases()
    ran = _group(env, monkeypatch, c, [n for n in c if n.startswith("right child")])
    assert ran == (9 + 3) * 2 + (6 + 3) * 2


def test_combs_over_a_balanced_trie_and_random_skewed_tries(env, monkeypatch):
    c = S.search_cases()
    names = [n for n in c if not n.startswith("right child")]
    assert len(names) >= 2 + 4 + 1
    assert _group(env, monkeypatch, c, names) == 4 * (len(names) - 1) + 2


# ------------------------------------------------------------------ `hufman`: depth limits
@pytest.mark.parametrize("kind", ["right", "left"])
def test_combs_on_both_sides_of_the_depth_limits(env, monkeypatch, kind):
    """leaves at 55 and 56: the GPU's table, with codes of 55 and 56 bits at both ends of the payload; from 57 on (a stack deeper than 120
    among them, for the left combs) the stream is handed back, and the pixels are the same"""
    c = S.depth_cases()
    names = [n for n in c if n.startswith(kind)]
    assert _group(env, monkeypatch, c, names) == len(S.DEPTHS) * (2 + 4)
    assert sum(c[n].on_gpu for n in names) == 4


@pytest.mark.parametrize("knobs", S.KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in sorted(k.items())))
def test_codes_of_56_bits_through_every_route_of_the_payload_decoder(env, monkeypatch, knobs):
    """the second table, the third tables, the kept symbols and the phase maps with a GPU-parsed table of 56-bit codes (the knobs of
    test_decoder_routes_round_5 in tests/test_decode_device.py)"""
    c = S.knob_cases()
    assert _group(env, monkeypatch, c, list(c), natural=False, **knobs) == 6


# ------------------------------------------------------------------ malformed and cut streams
def _check_verdicts(env, monkeypatch, codec, base, cases, **knobs):
    """every stream: refused or decoded as the oracle does, and to the oracle's pixels; from host and from device bytes.  A cut stream is
    given as the first bytes of the whole one, which lies behind them in device memory"""
    whole = upload(env, base.data)
    ok = 0
    with Hook(env, monkeypatch, True, **knobs):
        for name, data in cases:
            orc, opx = O.decode(codec, data)
            cut = len(data) < len(base.data) and base.data.startswith(data)
            dev_bytes = whole if cut else upload(env, data)
            for device in (None, dev_bytes):
                rc, px, parsed, handed = decode(env, codec, data, base.w, base.h, device, nbytes=len(data))
                assert (rc == 0) == (orc == 0), (name, rc, orc, device is None)
                if rc == 0:
                    assert np.array_equal(px, opx), name
                    assert parsed == 1 and not handed, name
                    ok += 1
    return ok


def test_malformed_and_cut_streams(env, monkeypatch):
    assert _check_verdicts(env, monkeypatch, "hufman", S.malformed_base(), S.malformed_hufman()) == 2      # (the one with a leaf more)


# ------------------------------------------------------------------ `delta`: records of 7 bytes
def test_delta_tries(env, monkeypatch):
    c = S.good_delta()
    ran = _group(env, monkeypatch, c, list(c), CNIIC_TRIE_HOST_SECOND="0")
    assert ran == 2 * len(c) and sum(s.on_gpu for s in c.values()) == len(c) - 2


def test_delta_symbols_out_of_range_and_cuts(env, monkeypatch):
    assert _check_verdicts(env, monkeypatch, "delta", S.delta_base(), S.malformed_delta(), CNIIC_TRIE_HOST_SECOND="0") == 0
