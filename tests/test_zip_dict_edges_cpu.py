"""The texts of tests/test_zip_dict_edges.py are what they claim to be (no GPU): every property the GPU tests rely on -- which side of a
threshold of k_zipdict.hip / zipdict.cpp a text stands on -- is asserted here against the restatement, with the values measured when the
texts were made, so that a change to a generator cannot move a case off its edge unnoticed."""
import numpy as np
import pytest

import zip_dict_edges as E
import zip_dict_ref as Z


@pytest.fixture(scope="module")
def clib(tmp_path_factory):
    lib = Z.compile_c(tmp_path_factory.mktemp("zip_dict_ref"))
    if lib is None:
        pytest.skip("no C compiler")
    return lib


def test_python_and_c_agree_on_the_run_text(clib):
    """the C restatement, which everything below and the GPU tests lean on, against the Python one on the text with the longest entries"""
    text, stream, info = E.case(clib, "run 256")
    ip = {}
    assert Z.encode_py(text.tobytes(), ip) == stream and ip == info
    assert Z.decode_c(clib, stream) == text.tobytes()


@pytest.mark.parametrize("name,longest,fill_end,matches,residues,low,high",
                         [("run 255", 255, 175820, 288, 100, 5, 250), ("run 256", 256, 176852, 192, 50, 10, 245)])
def test_longest_entry_on_either_side_of_the_windowed_route(clib, name, longest, fill_end, matches, residues, low, high):
    """max_entry < 256 takes the windowed chain, whose maps hold nx - 256 <= 254 in a byte.  Measured: 190 residues from 4 to 252 for the
    288 matches of 255 bytes, 92 from 0 to 246 for the 192 matches of 256."""
    text, stream, info = E.case(clib, name)
    tail_at = E.run_text(longest if longest == 256 else None)[1]
    assert info["longest"] == longest
    assert info["fill_end"] == fill_end and fill_end < tail_at - 100000, (info, tail_at)
    fe, starts, lens = E.frozen_parse(stream)
    assert fe == fill_end and int(lens.max()) == longest
    full = starts[lens == longest]
    assert full.size == matches and (full >= tail_at).all(), full.size
    res = np.unique((full - fe) % E.PIECE)
    assert res.size >= residues and res.min() <= low and res.max() >= high, (res.size, res.min(), res.max())
    if longest == 255:      # a full match that starts late in its piece: the map's target lies up to 254 into the next piece
        assert ((full - fe) % E.PIECE + 255 - E.PIECE).max() >= 250


def test_hand_over_bound(clib):
    """max_entry <= 32 768 goes to the GPU: a flat stretch of 65 534 bytes makes an entry of exactly 32 768 (2 + 4 + ... + 32 768 = 65 534);
    32 769 bytes more make one of 32 769"""
    text, stream, info = E.case(clib, "flat 65534")
    assert info["longest"] == E.MAX_ENTRY and info["fill_end"] == 236176 and info["fill_end"] < text.size - 400000, info
    text, stream, info = E.case(clib, "flat 98303")
    assert info["longest"] == E.MAX_ENTRY + 1 and info["fill_end"] == 268943 and info["fill_end"] < text.size - 400000, info


@pytest.mark.parametrize("sweep,P0,longest", [("windowed", 170708, 5), ("plain", 171174, 256)])
def test_m_sweep(clib, sweep, P0, longest):
    """every cut of the sweep hands exactly m positions to the GPU: the restatement's fill_end stays where the long text's is (for
    m = 0 too: the last fill pair's walks end inside the cut), and the longest entry with it"""
    text, stream, info = E.case(clib, sweep)
    assert info["fill_end"] == P0 and info["longest"] == longest and text.size > P0 + max(E.M_SWEEP), info
    for m in E.M_SWEEP:
        cut, cut_stream, cut_info = E.case(clib, "%s + %d" % (sweep, m))
        assert cut.size == P0 + m and cut_info["fill_end"] == P0 and cut_info["longest"] == longest, (m, cut_info)
        assert cut_stream[:4 * Z.MAX_PAIRS] == stream[:4 * Z.MAX_PAIRS]
        assert (len(cut_stream) == 4 * Z.MAX_PAIRS) == (m == 0)
    # the shortest: one symbol and 0xFFFF behind it, then two symbols (noise: single bytes or a short entry each)
    assert len(E.case(clib, sweep + " + 1")[1]) == 4 * Z.MAX_PAIRS + 4 and E.case(clib, sweep + " + 1")[1][-2:] == b"\xff\xff"
    # both parities of the symbol count occur among the cuts
    odd = {E.case(clib, "%s + %d" % (sweep, m))[1][-2:] == b"\xff\xff" for m in E.M_SWEEP if m}
    assert odd == {True, False}


def test_match_ends_at_a_window_end(clib):
    """the plain chain walks windows of 4096 positions; here a match of 256 bytes ends exactly where the first window does, so the second
    window starts at fill_end + 4096 (and the stretch's remaining 88 bytes lie at its head)"""
    text, stream, info = E.case(clib, "window end")
    assert info["fill_end"] == 171174 and info["longest"] == 256, info
    fe, starts, lens = E.frozen_parse(stream)
    k = int(np.flatnonzero(starts + lens == fe + E.WINDOW)[0])
    assert lens[k] == 256 and starts[k] - fe == E.WINDOW - 256 and lens[k - 1] == 256, (lens[k - 1], lens[k], starts[k] - fe)
    assert text[fe + E.WINDOW] == 7                       # the stretch goes on behind the window's end


def test_many_symbols(clib):
    """k_zd_dec_scan gives each of its 1024 threads more than one chunk of 2048 symbols only above 2 097 152 symbols"""
    text, stream, info = E.case(clib, "many")
    frozen = (len(stream) - 4 * Z.MAX_PAIRS) // 2 - (stream[-2:] == b"\xff\xff")
    assert info["fill_end"] == 170708 and frozen == 4219363 and frozen > 2 * 1024 * E.DEC_CHUNK, (info, frozen)
    assert -(-frozen // E.DEC_CHUNK) == 2061
    assert (len(stream) - 4 * Z.MAX_PAIRS) // 4 > 1048577   # the decode sweep's cuts all lie inside the stream


def test_hilbert_clips(clib):
    """11 w' h' lies behind fill_end and inside a frozen symbol, for nine claims and three cut offsets"""
    import oracle_lib as O
    lin = O.hilbert_linearize(E.clip_image())
    stream = E.hilbert_clip_stream(clib, lin)
    fe, starts, lens = E.frozen_parse(stream)
    assert fe == 551924 and int(starts[-1] + lens[-1]) == 11 * 256 * 256 == 720896
    for (w, h), want in E.HILBERT_CLIPS.items():
        assert fe < 11 * w * h < 720896 and w * h < 256 * 256
        got = E.inside_symbol(starts, lens, 11 * w * h)
        assert got == want and got[0] >= 1 and got[1] >= 2, ((w, h), got)
    assert len(E.HILBERT_CLIPS) >= 8 and len({off for off, _ in E.HILBERT_CLIPS.values()}) >= 3
    # the replaced symbol: one byte more of text at 561 250, in the middle of record 51 022 -- the records behind it are shifted
    bad, at, length = E.with_longer_symbol(stream)
    assert (at, length) == (561250, 2) and at > fe and bad != stream and len(bad) == len(stream)
    dec = lambda s, need: Z.decode_c(clib, s, need)
    lin_bad = Z.hilbert_decode_lin(dec, b"\0\1\0\0\0\1\0\0" + bad)
    want = lin.reshape(-1, 3)
    first_zero = at // 11 + 1
    assert lin_bad is not None and np.array_equal(lin_bad[2][:at // 11], want[:at // 11])
    assert not lin_bad[2][first_zero:].any() and at // 11 == 51022


def test_zip_clips(clib):
    """8 + 11 w' h' lies behind fill_end and inside a frozen symbol of the claim's own stream; the restatement decodes every one"""
    for (w, h), want in E.ZIP_CLIPS.items():
        stream = Z.encode_c(clib, E.zip_clip_text(w, h))
        fe, starts, lens = E.frozen_parse(stream)
        at = 8 + 11 * w * h
        got = E.inside_symbol(starts, lens, at)
        assert at > fe and got == want and got[0] >= 1 and got[1] >= 2, ((w, h), fe, got)
        img = Z.codec_decode(lambda s, need: Z.decode_c(clib, s, need), stream)
        assert img is not None and np.array_equal(img.reshape(-1), E.clip_image().reshape(-1)[:3 * w * h])
    assert len(E.ZIP_CLIPS) >= 4
