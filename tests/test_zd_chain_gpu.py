"""zip(dict)'s frozen parse where an entry exceeds 255 bytes: the hybrid chain of k_zipdict.hip (cniic_amd/csrc/zd_chain.hpp) on the texts
of tests/zd_chain_cases.py, byte for byte against the restatement (tests/zip_dict_ref.py / .c).  tests/test_zd_chain_cpu.py asserts that
every text stands where it claims to stand and derives, from the restatement's stream and the text alone, how many break pieces it has
and how many of them the parse enters; here the library's route marks must say the same.

The route is read from the stage timers' launch counts: "zd_chain_plain" stays 1 and "zd_chain" 0 for every text with a long entry;
"zd_chain_hybrid" = 1, "zd_chain_breaks" = B and "zd_chain_entered" are there when the new route ran, and only then."""
import numpy as np
import pytest

import zd_chain_cases as K
import zip_dict_edges as E
import zip_dict_ref as Z

pytestmark = pytest.mark.gpu

STAGES = ("zd_match", "zd_chain", "zd_chain_plain", "zd_chain_hybrid", "zd_chain_breaks", "zd_chain_entered")
KNOB_CHAIN, KNOB_MAX_BREAKS = "CNIIC_TEST_ZD_CHAIN", "CNIIC_TEST_ZD_CHAIN_MAX_BREAKS"


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


def routed(ctx, call):
    """(what call() returns, {stage: launches during the call})"""
    from cniic_amd import _lib
    ctx.set_opt(_lib.OPT_STAGE_TIMERS, 1)
    try:
        ctx.zip_dict_encode(b"")               # (the timers of a call are those since the call began)
        before = [ctx.kernel_time(s)[1] for s in STAGES]
        got = call()
        after = [ctx.kernel_time(s)[1] for s in STAGES]
    finally:
        ctx.set_opt(_lib.OPT_STAGE_TIMERS, None)
    return got, {s: a - b for s, a, b in zip(STAGES, after, before)}


def hybrid(breaks, entered):
    return {"zd_match": 1, "zd_chain": 0, "zd_chain_plain": 1, "zd_chain_hybrid": 1, "zd_chain_breaks": breaks, "zd_chain_entered": entered}


WALK = {"zd_match": 1, "zd_chain": 0, "zd_chain_plain": 1, "zd_chain_hybrid": 0, "zd_chain_breaks": 0, "zd_chain_entered": 0}
WINDOWED = dict(WALK, zd_chain=1, zd_chain_plain=0)
HOST = dict(WALK, zd_match=0, zd_chain_plain=0)


def check_text(ctx, text, ref, want):
    (rc, stream), ran = routed(ctx, lambda: ctx.zip_dict_encode(text))
    first = next((i for i in range(min(len(stream), len(ref))) if stream[i] != ref[i]), None) if stream != ref else None
    assert rc == 0 and stream == ref, "%d bytes against %d, first difference at %s" % (len(stream), len(ref), first)
    assert ran == want
    back = np.empty(text.size + 1, np.uint8)
    rc, ln = ctx.zip_dict_decode(stream, out=back)
    assert rc == 0 and ln == text.size and np.array_equal(back[:ln], text)


@pytest.mark.parametrize("name", K.NAMES)
def test_bytes_and_route(ctx, clib, name):
    text, ref, info = K.case(clib, name)
    steps, breaks, entered = K.CLAIMS[name]
    check_text(ctx, text, ref, hybrid(breaks, entered))


@pytest.mark.parametrize("name", K.NAMES)
def test_the_walk_gives_the_same_bytes(ctx, clib, name, monkeypatch):
    text, ref, info = K.case(clib, name)
    monkeypatch.setenv(KNOB_CHAIN, "walk")
    check_text(ctx, text, ref, WALK)


@pytest.mark.parametrize("name", [n for n in K.NAMES if K.CLAIMS[n][1]])
def test_the_bound_on_the_break_pieces(ctx, clib, name, monkeypatch):
    """one below the text's break pieces: the one-block walk; exactly at them: the route"""
    text, ref, info = K.case(clib, name)
    steps, breaks, entered = K.CLAIMS[name]
    monkeypatch.setenv(KNOB_MAX_BREAKS, str(breaks - 1))
    check_text(ctx, text, ref, WALK)
    monkeypatch.setenv(KNOB_MAX_BREAKS, str(breaks))
    check_text(ctx, text, ref, hybrid(breaks, entered))
    monkeypatch.setenv(KNOB_MAX_BREAKS, str(1 << 40))          # (the knob lowers the bound, it never raises it)
    check_text(ctx, text, ref, hybrid(breaks, entered))


def test_band_through_both_codecs(ctx, clib):
    """an image's text is not made of one byte: from the stream only bounds follow (zd_chain_cases.band_counts)"""
    import oracle_lib as O
    img = Z.band()
    text = np.frombuffer(Z.zip_text(img), np.uint8)
    ref = Z.encode_c(clib, text)
    (rc, stream), ran = routed(ctx, lambda: ctx.zip_dict_encode(text))
    assert rc == 0 and stream == ref
    entered_min, breaks_min = K.band_counts(ref)
    assert entered_min >= 1 and ran["zd_chain_hybrid"] == 1 and ran["zd_chain_plain"] == 1 and ran["zd_chain"] == 0
    assert ran["zd_chain_entered"] >= entered_min and ran["zd_chain_breaks"] >= max(breaks_min, ran["zd_chain_entered"])
    (rc, stream, st), ran = routed(ctx, lambda: ctx.encode("zip(dict)", img))
    assert rc == 0 and stream == ref and ran["zd_chain_hybrid"] == 1
    rc, back = ctx.decode("zip(dict)", stream)
    assert rc == 0 and np.array_equal(back, img)
    lin = O.hilbert_linearize(img)
    href = Z.hilbert_encode(lambda t: Z.encode_c(clib, t), lin, img.shape[1], img.shape[0])
    (rc, stream), ran = routed(ctx, lambda: ctx.hilbert_zip_encode(img))
    assert rc == 0 and stream == href
    entered_min, breaks_min = K.band_counts(href[8:])
    assert entered_min >= 1 and ran["zd_chain_hybrid"] == 1 and ran["zd_chain_plain"] == 1
    assert ran["zd_chain_entered"] >= entered_min and ran["zd_chain_breaks"] >= max(breaks_min, ran["zd_chain_entered"])
    rc, back = ctx.hilbert_zip_decode(stream)
    assert rc == 0 and np.array_equal(back, img)


@pytest.mark.parametrize("name", ["land 255", "fly 65", "flown break", "cut by M", "no break"])
def test_device_buffers_and_capacity(ctx, clib, name):
    import torch
    from cniic_amd import _lib
    text, ref, info = K.case(clib, name)
    t = torch.from_numpy(text.copy()).cuda()
    out = torch.empty(2 * text.size + 4, dtype=torch.uint8, device="cuda")
    rc, ln = ctx.zip_dict_encode(t, out=out)
    assert rc == 0 and out[:ln].cpu().numpy().tobytes() == ref
    back = torch.empty(text.size, dtype=torch.uint8, device="cuda")
    rc, ln2 = ctx.zip_dict_decode(out, n=ln, out=back)
    assert rc == 0 and ln2 == text.size and np.array_equal(back.cpu().numpy(), text)
    small = torch.empty(len(ref) - 1, dtype=torch.uint8, device="cuda")
    rc, need = ctx.zip_dict_encode(t, out=small, allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(ref)
    rc, need = ctx.zip_dict_encode(text, out=np.empty(100, np.uint8), allow=(_lib.CAPACITY,))
    assert rc == _lib.CAPACITY and need == len(ref)


def test_alternating_routes_on_one_context(ctx, clib):
    """a windowed text, a hybrid text and a host-route text in turn: nothing of one call's scratch reaches the next"""
    windowed = np.random.default_rng(1).integers(0, 256, 700000, dtype=np.uint8)
    texts = [(windowed, Z.encode_c(clib, windowed), WINDOWED),
             K.case(clib, "flown break")[:2] + (hybrid(*K.CLAIMS["flown break"][1:]),),
             E.case(clib, "flat 98303")[:2] + (HOST,)]
    for k in range(8):
        text, ref, want = texts[k % 3]
        (rc, stream), ran = routed(ctx, lambda: ctx.zip_dict_encode(text))
        assert rc == 0 and stream == ref and ran == want, k


def test_a_batch_of_band_and_noise_frames(ctx, clib):
    """cniic_codec_encode_batch_var's workers run the same code per image: every stream is the single call's"""
    flat_tail = Z.noise(320, 240)
    flat_tail[:2] = (9, 9, 9)
    flat_tail[230:] = (9, 9, 9)
    imgs = [Z.band(), Z.noise(320, 240), flat_tail, Z.noise(300, 260)]
    singles = []
    for im in imgs:
        rc, s, st = ctx.encode("zip(dict)", im)
        assert rc == 0 and s == Z.encode_c(clib, np.frombuffer(Z.zip_text(im), np.uint8))
        singles.append(s)
    sizes = [im.size for im in imgs]
    offs = [int(x) for x in np.concatenate([[0], np.cumsum([(n + 15) & ~15 for n in sizes])[:-1]])]
    buf = np.zeros(offs[-1] + sizes[-1], np.uint8)
    for o, im in zip(offs, imgs):
        buf[o:o + im.size] = im.reshape(-1)
    stride = (max(len(s) for s in singles) + 15) & ~15
    out = np.zeros(stride * len(imgs), np.uint8)
    rc, lens, rcs, sts = ctx.encode_batch_var("zip(dict)", buf, offs, [im.shape[1] for im in imgs], [im.shape[0] for im in imgs], out, stride)
    assert rc == 0 and rcs == [0] * len(imgs)
    for f, s in enumerate(singles):
        assert out[f * stride:f * stride + lens[f]].tobytes() == s, f
