"""zip(dict)'s frozen-phase kernels on either side of every threshold they switch on, byte for byte against the restatement
(tests/zip_dict_ref.py / .c).  tests/zip_dict_edges.py makes the texts and says which edge each stands on;
tests/test_zip_dict_edges_cpu.py asserts that they stand there.  Which route a call took is read from the stage timers' launch counts.

encode   the windowed chain against the plain one (longest entry 255 | 256), the GPU against the host (32 768 | 32 769), and M -- the
         positions handed to the GPU -- at 0, 1, 2, 3, one piece (256 +- 1), one compaction chunk and one window of the plain chain
         (4096 +- 1), 64 | 65 pieces (16 384 +- 1) and 4096 | 4097 pieces (1 048 576 +- 1) of the scan of the maps
decode   the frozen symbols at 0, 2, a wave's 64 +- 2, a chunk's 2048 +- 2, 1024 chunks' 2 097 152 +- 2 and 4 219 364 (2061 chunks:
         k_zd_dec_scan's threads take three each); a first symbol without a second behind each; claimed dimensions that end inside
         a frozen symbol's text (k_zd_dec_copy's clip), through hilbert-zip and through zip(dict)"""
import struct

import numpy as np
import pytest

import zip_dict_edges as E
import zip_dict_ref as Z

pytestmark = pytest.mark.gpu

FILL_BYTES = 4 * Z.MAX_PAIRS


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_dict_ref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


@pytest.fixture(scope="module")
def ctx():
    import cniic_amd
    with cniic_amd.Context(0) as c:
        yield c


# ---------------------------------------------------------------- encode: the stream, the text back, the route
STAGES = ("zd_match", "zd_chain", "zd_chain_plain")
WINDOWED, PLAIN, HOST = (1, 1, 0), (1, 0, 1), (0, 0, 0)      # launches of STAGES in one encode

ROUTES = {"run 255": WINDOWED, "run 256": PLAIN, "flat 65534": PLAIN, "flat 98303": HOST, "window end": PLAIN, "many": WINDOWED}
for _m in E.M_SWEEP:
    ROUTES["windowed + %d" % _m] = WINDOWED if _m else HOST
    ROUTES["plain + %d" % _m] = PLAIN if _m else HOST


def launches(ctx):
    return tuple(ctx.kernel_time(s)[1] for s in STAGES)


def encode_with_route(ctx, data):
    """(rc, stream, launches of STAGES during the call)"""
    from cniic_amd import _lib
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        ctx.zip_dict_encode(b"")               # (the timers of a call are those since the call began)
        before = launches(ctx)
        rc, stream = ctx.zip_dict_encode(data)
        after = launches(ctx)
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    return rc, stream, tuple(a - b for a, b in zip(after, before))


@pytest.mark.parametrize("name", list(ROUTES))
def test_host_bytes_and_route(ctx, clib, name):
    text, ref, info = E.case(clib, name)
    rc, stream, ran = encode_with_route(ctx, text)
    first = next((i for i in range(min(len(stream), len(ref))) if stream[i] != ref[i]), None) if stream != ref else None
    assert rc == 0 and stream == ref, "%s: %d bytes against %d, first difference at %s" % (name, len(stream), len(ref), first)
    assert ran == ROUTES[name], "%s: launches of %s" % (name, STAGES)
    back = np.empty(text.size + 1, np.uint8)
    rc, ln = ctx.zip_dict_decode(ref, out=back)
    assert rc == 0 and ln == text.size and np.array_equal(back[:ln], text)


def test_band_takes_the_plain_route(ctx, clib):
    text = Z.zip_text(Z.band())
    rc, stream, ran = encode_with_route(ctx, text)
    assert rc == 0 and stream == Z.encode_c(clib, text) and ran == PLAIN


@pytest.mark.parametrize("name", list(ROUTES))
def test_device_buffers(ctx, clib, name):
    """test_zip_dict.py's test_raw_frozen_phase_device_buffers on every text"""
    import torch
    from cniic_amd import _lib
    text, ref, info = E.case(clib, name)
    t = torch.from_numpy(text.copy()).cuda()
    out = torch.empty(2 * text.size + 4, dtype=torch.uint8, device="cuda")
    rc, ln = ctx.zip_dict_encode(t, out=out)
    assert rc == 0 and out[:ln].cpu().numpy().tobytes() == ref
    back = torch.empty(text.size, dtype=torch.uint8, device="cuda")
    rc, ln2 = ctx.zip_dict_decode(out, n=ln, out=back)
    assert rc == 0 and ln2 == text.size and np.array_equal(back.cpu().numpy(), text)
    # a text that exceeds cap: CAPACITY, with the bytes needed
    small = torch.empty(text.size - 1, dtype=torch.uint8, device="cuda")
    rc, need = ctx.zip_dict_decode(out, n=ln, out=small, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == text.size
    rc, need = ctx.zip_dict_encode(t, out=small[:100], allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(ref)


# ---------------------------------------------------------------- decode: the count of frozen symbols
DECODE_CUTS = (0, 1, 31, 32, 33, 1023, 1024, 1025, 1048575, 1048576, 1048577, None)     # frozen pairs kept; None: the whole stream


@pytest.mark.parametrize("k", DECODE_CUTS)
def test_decode_sweep(ctx, clib, k):
    """every whole-pair prefix of a stream is a stream; 2 or 3 bytes more are a first symbol without a second"""
    from cniic_amd import _lib
    text, ref, info = E.case(clib, "many")
    n = len(ref) if k is None else 4 * (Z.MAX_PAIRS + k)
    assert n <= len(ref)
    out = np.empty(text.size + 16, np.uint8)
    for extra in (0, 1, 2, 3):
        if n + extra > len(ref):
            continue
        cut = ref[:n + extra]
        try:
            want = Z.decode_c(clib, cut, cap=out.size)
        except Z.ZipError:
            want = None
        assert (want is None) == (extra >= 2)
        rc, ln = ctx.zip_dict_decode(cut, out=out, allow=(_lib.DECODE,))
        if want is None:
            assert rc == _lib.DECODE, (k, extra)
        else:
            assert rc == 0 and ln == len(want) and out[:ln].tobytes() == want, (k, extra, ln, len(want))
    if k is None:
        rc, need = ctx.zip_dict_decode(ref, out=out[:text.size - 1], allow=(_lib.CAPACITY,))
        assert rc == _lib.CAPACITY and need == text.size


# ---------------------------------------------------------------- decode: the text ends inside a frozen symbol
@pytest.fixture(scope="module")
def hilbert_case(clib):
    """(the scan-order pixels of the clip image, the coder's stream of their records)"""
    import oracle_lib as O
    lin = O.hilbert_linearize(E.clip_image())
    return lin, E.hilbert_clip_stream(clib, lin)


def check_hilbert(ctx, clib, stream):
    """HilbertZip.decode against hilbert_decode_lin: the restatement's pixels, or its verdict"""
    import cniic_amd
    import oracle_lib as O
    want = Z.hilbert_decode_lin(lambda s, need: Z.decode_c(clib, s, need), stream)
    got = cniic_amd.HilbertZip(ctx).decode(stream)
    if want is None:
        assert got is None
        return None
    w, h, lin = want
    assert got is not None and got.shape == (h, w, 3)
    assert np.array_equal(O.hilbert_linearize(got).reshape(-1, 3), lin)
    return lin


@pytest.mark.parametrize("w,h", list(E.HILBERT_CLIPS))
def test_hilbert_zip_claims_fewer_pixels(ctx, clib, hilbert_case, w, h):
    lin, stream = hilbert_case
    got = check_hilbert(ctx, clib, struct.pack("<II", w, h) + stream)
    assert got is not None and np.array_equal(got, lin.reshape(-1, 3)[:w * h])      # (every claimed pixel is there)


def test_hilbert_zip_whole_and_shifted(ctx, clib, hilbert_case):
    lin, stream = hilbert_case
    whole = check_hilbert(ctx, clib, struct.pack("<II", 256, 256) + stream)
    assert whole is not None and np.array_equal(whole, lin.reshape(-1, 3))
    bad, at, length = E.with_longer_symbol(stream)
    shifted = check_hilbert(ctx, clib, struct.pack("<II", 256, 256) + bad)
    assert shifted is not None and shifted[at // 11 - 1].any() and not shifted[at // 11 + 1:].any()   # the colours end at the first bad record


@pytest.mark.parametrize("w,h", list(E.ZIP_CLIPS))
def test_zip_dict_claims_fewer_pixels(ctx, clib, w, h):
    from cniic_amd import _lib
    stream = Z.encode_c(clib, E.zip_clip_text(w, h))
    want = Z.codec_decode(lambda s, need: Z.decode_c(clib, s, need), stream)
    assert want is not None and want.shape == (h, w, 3)
    rc, got = ctx.decode("zip(dict)", stream, allow=(_lib.DECODE,))
    assert rc == 0 and np.array_equal(got, want)
