"""CPU side of cniic_cc_finish_frames_var: the symbol is where the loader and the header say it is, and the yardstick of
tests/test_frames_var.py -- test_dist.expected_streams on frames of any shapes -- is itself pinned to the oracle's single encode."""
import ctypes as C
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

NAME = "cniic_cc_finish_frames_var"


def test_both_libraries_export_the_call_and_the_header_declares_it():
    from cniic_amd import _lib
    # appended to the loader's list right behind the last call of the release before it
    assert _lib.SYMBOLS.count(NAME) == 1 and _lib.SYMBOLS.index(NAME) == _lib.SYMBOLS.index("cniic_channel_diff_hist") + 1
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cniic_hip.h")).read(), flags=re.S)
    decl = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert decl, "include/cniic_hip.h does not declare %s" % NAME
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["cniic_cc *cc", "const uint8_t *rgb", "const uint32_t *w", "const uint32_t *h", "uint32_t frames", "uint8_t *out", "uint64_t stride",
                    "uint64_t *lens", "cniic_kmeans_stats *stats"]
    assert text.index("cniic_cc_finish_frames(") < decl.start() < text.index("cniic_cc_destroy(")   # beside its equal-size neighbour
    for lib in ("libcniic_hip.so", "libcniic_hip_testing.so"):
        assert hasattr(C.CDLL(os.path.join(ROOT, "cniic_amd", lib)), NAME), lib
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 9


def test_expected_streams_of_one_ragged_frame_is_the_single_encode():
    import oracle_lib as O
    from cniic_amd import synth
    from test_dist import expected_streams
    for w, h in ((40, 30), (17, 1), (1, 4097)):
        img = synth.photo(w, h, synth.SEED0 + 940)
        exp, iters = expected_streams([img], 16)
        rc, data, st = O.encode("cluster-colors(16)", img, mode=O.MODE_L)
        assert rc == 0 and exp == [data] and iters == st["iterations"], (w, h)
