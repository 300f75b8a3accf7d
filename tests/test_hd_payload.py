"""The parallel payload decoder (cniic_amd/csrc/k_hdecode.hip: pass 0 and the checks, the kept symbols and their copy, the phase maps, the
write, FromDiff's chunk sums on the way) on payloads built by hand to sit on its limits (tests/payload_shapes.py).  Every comparison is
exact: the return code, every pixel -- known from the symbol sequence alone for `hufman`, the prefix sums of the differences along the
oracle's traversal for `delta` -- and WHICH route answered, read from the stage marks: "hd_phases" (calls of the phase maps), "hd_recheck"
(checks with a look past the two blind ones), "hd_compact" (1: the final write copied kept rows) and "hd_host_walk" (the host's node walk
decoded the payload).  "hd_host_walk" and "trie_parse_host" must be 0 wherever a case does not name them: a decoder that hands
everything back to the host decodes every image and fails every case here.

Each stream is decoded from host bytes, which the decoder copies to an aligned buffer (bit0 = 0), and from device bytes placed at the
residue modulo 4 that gives the case's bit0, into an image with 16 bytes of poison behind it that must stay; with OPT_GPU_DECODE_MIN = 0.

tests/test_hd_payload_cpu.py establishes without a GPU what every stream is and that it sits where its name says.  No GPU code is imported
at the top."""
import numpy as np
import pytest

import oracle_lib as O
import payload_shapes as P
import trie_shapes as S
from test_trie_shapes import DECODE, stage

pytestmark = pytest.mark.gpu

POISON = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    import cniic_amd
    from cniic_amd import _lib
    ctx = cniic_amd.Context(0)
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    yield ctx, torch, torch.device("cuda", 0)
    ctx.close()


class Knobs:
    """OPT_GPU_DECODE_MIN = 0 and the knobs of a case in the environment"""

    def __init__(self, env, monkeypatch, knobs):
        self.ctx, self.mp, self.knobs = env[0], monkeypatch, knobs

    def __enter__(self):
        from cniic_amd import _lib
        self.ctx.set_opt(_lib.OPT_GPU_DECODE_MIN, 0)
        for k, v in self.knobs.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        from cniic_amd import _lib
        self.ctx.set_opt(_lib.OPT_GPU_DECODE_MIN, None)
        for k in self.knobs:
            self.mp.delenv(k, raising=False)


_XY = {}


def expected(p):
    """the image of a good stream: the builder's (`hufman`), or its colours along the traversal put in their places (`delta`)"""
    if p.codec == "hufman":
        return p.image
    if (p.w, p.h) not in _XY:
        _XY[(p.w, p.h)] = O.hilbert_iter(p.w, p.h).astype(np.int64)
    xy = _XY[(p.w, p.h)]
    img = np.zeros((p.h, p.w, 3), np.uint8)
    img[xy[:, 1], xy[:, 0]] = p.lin.astype(np.uint8)
    return img


def upload_at(env, data, payload_pos, bit0):
    """the stream in device memory with its payload's first byte at bit0 / 8 modulo 4"""
    ctx, torch, dev = env
    lead = (bit0 // 8 - payload_pos) % 4
    t = torch.frombuffer(bytearray(b"\xff" * lead + data + b"\xff" * 8), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    assert t.data_ptr() % 4 == 0
    return t[lead:]


def decode(env, codec, data, w, h, device=None):
    """one cniic_codec_decode of host bytes or of the device tensor -> (rc, pixels or None, {mark: launches})"""
    ctx, torch, dev = env
    if device is None:
        rc, px = ctx.decode(codec, data, allow=(DECODE,))
    else:
        out = torch.full((w * h * 3 + 16,), POISON, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rc, dw, dh = ctx.decode_into(codec, device, len(data), out, allow=(DECODE,))
        px = None
        got = out.cpu().numpy()
        assert (got[w * h * 3:] == POISON).all()                                   # nothing behind the image, decoded or refused
        if rc == 0:
            assert (dw, dh) == (w, h)
            px = got[:w * h * 3].reshape(h, w, 3)
    marks = {m: stage(ctx, m) or 0 for m in P.MARKS + (S.PARSE, S.PARSE_HOST)}
    return rc, (px if rc == 0 else None), marks


def _holds(got, want):
    return got >= want[1] if isinstance(want, tuple) else got == want


def check(env, monkeypatch, name, case, knobs=None, marks=True):
    """host bytes and device bytes: the verdict, the pixels, the marks"""
    p = case.p
    want = expected(p) if p.ok else None
    dev_bytes = upload_at(env, p.data, p.payload_pos, p.bit0)
    assert (dev_bytes.data_ptr() + p.payload_pos) % 4 == p.bit0 // 8
    with Knobs(env, monkeypatch, case.knobs if knobs is None else knobs):
        for device, named in ((None, case.host_marks), (dev_bytes, case.marks)):
            rc, px, got = decode(env, p.codec, p.data, p.w, p.h, device)
            what = (name, "host bytes" if device is None else "device bytes at bit %d" % p.bit0, knobs or case.knobs, got)
            assert rc == (0 if p.ok else DECODE), what
            if p.ok:
                assert np.array_equal(px, want), what
                for m in ("hd_host_walk", S.PARSE_HOST):
                    assert got[m] == named.get(m, 0), (m, what)
                if marks:
                    for m, v in named.items():
                        assert _holds(got[m], v), (m, v, what)


def _group(env, monkeypatch, cases, **kw):
    """(how many cases each group holds is asserted in tests/test_hd_payload_cpu.py)"""
    assert cases
    for n, c in cases.items():
        check(env, monkeypatch, n, c, **kw)


# ------------------------------------------------------------------ kept symbols
@pytest.mark.parametrize("codec", ["hufman", "delta"])
def test_kept_symbols_at_63_64_65_and_512_a_subsequence(env, monkeypatch, codec):
    """subsequences of 59 .. 65 and 512 symbols beside ones of 32, kept | long borders at every residue of the output index, a subsequence
    decoded twice with fewer symbols the second time, and the two sides of the natural keep gate: CNIIC_HD_KEEP unset, 1 and 0"""
    c = {n: v for n, v in P.kept_cases().items() if n.startswith(codec)}
    _group(env, monkeypatch, c)


# ------------------------------------------------------------------ boundaries and ends
def test_payloads_of_exactly_1_255_256_257_512_and_513_subsequences(env, monkeypatch):
    c = {n: v for n, v in P.ends_cases().items() if n.startswith("nsub")}
    _group(env, monkeypatch, c)


def test_padding_that_decodes_to_symbols(env, monkeypatch):
    """1 .. 7 bits of padding where the all-zero code has 1 bit and where it has 7: the image ends with the listed symbols, with what the
    padding decodes to, and is refused when it wants one symbol more; nsyms = 4 k + 1 .. 3 among them"""
    c = {n: v for n, v in P.ends_cases().items() if "padding" in n}
    _group(env, monkeypatch, c)


def test_trailing_bytes_behind_the_payload(env, monkeypatch):
    """1, 64, 65 and 16385 bytes of 00 and of ff: a whole subsequence and a whole block of symbols past nsyms"""
    c = {n: v for n, v in P.ends_cases().items() if "trailing" in n}
    _group(env, monkeypatch, c)


def test_codes_of_32_and_56_bits_over_the_staged_tail(env, monkeypatch):
    c = {n: v for n, v in P.ends_cases().items() if n.startswith("a code of")}
    _group(env, monkeypatch, c)


# ------------------------------------------------------------------ FromDiff on the way
def test_chunk_sums_at_the_borders_of_fromdiff_s_chunks(env, monkeypatch):
    """+v on the last symbol of a chunk and -v on the first of the next, inside a kept subsequence, between two and inside a long one:
    summed by k_hd_compact and k_hd_write(only_long) on their way, and by k_ud_sums after them (CNIIC_HD_KEEP=0)"""
    c = {n: v for n, v in P.fromdiff_cases().items() if n.startswith("borders")}
    _group(env, monkeypatch, c)


def test_colours_on_and_past_the_edge_of_their_range(env, monkeypatch):
    c = {n: v for n, v in P.fromdiff_cases().items() if not n.startswith("borders")}
    _group(env, monkeypatch, c)


def test_an_image_of_1025_chunks(env, monkeypatch):
    check(env, monkeypatch, "2049 x 2048", P.big_delta_case())


# ------------------------------------------------------------------ streams that never fall into step
def test_locked_streams_take_the_phase_maps_once(env, monkeypatch):
    """SEVEN with phases 16 and 17 at bit0 0, 8, 16, 24, the entry offset at which a map saturates, ragged groups of k_hd_phase_chain"""
    _group(env, monkeypatch, P.locked_cases())


def test_the_verdict_of_one_block_in_four(env, monkeypatch):
    """no locked payload and 30 subsequences of it: no phase maps, no looked check; one whole block of four: the maps"""
    _group(env, monkeypatch, P.verdict_cases())


def test_locked_streams_of_65536_and_65537_subsequences(env, monkeypatch):
    """the two sides of kHdPhasesMaxSub: SEVEN reaches the maps by the verdict on both; SIXTEEN at bit 8 by the unsettled blind checks on
    the one and by 46 looked checks (46 synchronisations, a block of 256 rounds each) that still leave it unsettled on the other"""
    _group(env, monkeypatch, P.long_locked_cases())


def test_a_stream_on_which_no_guess_is_ever_right(env, monkeypatch):
    """SIXTEEN at bit0 = 8: one block falls into step per check.  40 blocks settle by looked checks, 60 do not within kHdMaxPasses and
    go to the host's walk (without the phase maps: CNIIC_HD_PHASES=0, or a code wider than 32 bits).  These are up to 48 stream
    synchronisations of a check each, and a check is one block of up to 320 rounds: tens of milliseconds, not a hang"""
    _group(env, monkeypatch, P.sixteen_cases())


# ------------------------------------------------------------------ tables
def test_tables_at_their_limits(env, monkeypatch):
    """no second table | one, its cap of 18 bits, a third table | the bisection, 96 | 97 leaves and one code length under a prefix, the
    second table built from the leaves' side (CNIIC_HD_LUT2_BITS=21: leaves that own 64, 128 and 2^20 prefixes)"""
    ran = 0
    for name, (s, knobs) in P.table_cases().items():
        dev_bytes = upload_at(env, s.data, s.payload_pos, 0)
        with Knobs(env, monkeypatch, knobs):
            for device in (None, dev_bytes):
                rc, px, got = decode(env, "hufman", s.data, s.w, s.h, device)
                assert rc == 0 and np.array_equal(px, s.image), (name, got)
                assert not got["hd_host_walk"] and not got[S.PARSE_HOST], (name, got)
                ran += 1
    assert ran == 20


def test_the_two_sides_of_the_first_table_s_gate(env, monkeypatch):
    _group(env, monkeypatch, P.first_table_cases())


@pytest.mark.parametrize("knobs", S.KNOBS, ids=lambda k: ",".join("%s=%s" % kv for kv in sorted(k.items())))
def test_the_small_streams_through_every_knob(env, monkeypatch, knobs):
    """(the pixels and no hand-back; which route a knob forces is not asserted here)"""
    _group(env, monkeypatch, P.small_cases(), knobs=knobs, marks=False)
