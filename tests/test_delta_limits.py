"""The `delta` encoder (cniic_amd/csrc/k_delta.hip, encode_delta in codec.cpp) where its 16-bit symbol stream switches routes: images whose
differences along the scan are prescribed (delta_limits_ref.py), so that each 512-symbol chunk holds a KNOWN number of symbols outside the
cube -- 15 | 16 where the counting folds equal keys, 63 | 64 | 65 where the side array is full and the call restarts on the 32-bit route --
in a first, a middle and the last chunk of the tile gather's squares and the per-position gather's rectangles, packed into one ballot, into
single lanes, across chunk, wave and tile borders, with the keys on the cube's faces and at the table's two ends.  tests/test_delta_limits_cpu.py
asserts that every case stands where it claims to.  Every stream is the oracle's, and the ROUTE is asserted too: both routes give the same
bytes by design, so only the stage timers can tell an encoder that overflows too early, too late or never."""
import numpy as np
import pytest

import delta_limits_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cniic_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """the oracle's stream of a case, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            rc, data, _ = O.encode("delta", R.case_image(name))
            assert rc == 0
            cache[name] = data
        return cache[name]
    return get


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_equals_oracle_and_takes_its_route(ctx, expected, name):
    """a plain call gives the oracle's bytes and decodes to the image; the same call with the stage timers on (they are cleared at the start of
    every call) gives the same bytes, ran the gather once and ran hilbert_delta -- the 32-bit route's first kernel -- exactly when the case
    has a chunk of 65"""
    from cniic_amd import _lib
    case, img, want = R.BY_NAME[name], R.case_image(name), expected(name)
    rc, data, _ = ctx.encode("delta", img)
    assert rc == 0 and data == want
    rc, back = ctx.decode("delta", data)
    assert rc == 0 and np.array_equal(back, img)
    rc, timed, _ = ctx.encode("delta", img, flags=_lib.KM_PROFILE)
    assert rc == 0 and timed == want
    gathers, restarts = ctx.kernel_time("delta_gather")[1], ctx.kernel_time("hilbert_delta")[1]
    assert gathers == 1
    assert restarts == 0 if case.route == 16 else restarts >= 1, (case.route, restarts)


KNOBS = ["CNIIC_DELTA_GATHER=any", "CNIIC_TEST_INLINE_CODE_BITS=5", "CNIIC_TEST_PACK_IMG_WORDS=24", "OPT_DELTA_ROUTE=32"]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_under_the_route_knobs(ctx, monkeypatch, expected, name, knob):
    """the squares through the per-position gather; cold and hot codes out of the inline word (the escape read of k_delta_count16 / k_delta_write16);
    chunks that outgrow the bit image; the 32-bit route asked for.  The full product: a call on these images takes a millisecond or two."""
    from cniic_amd import _lib
    k, v = knob.split("=")
    img = R.case_image(name)
    if k.startswith("OPT_"):
        ctx.set_opt(getattr(_lib, k), int(v))
    else:
        monkeypatch.setenv(k, v)
    try:
        rc, data, _ = ctx.encode("delta", img)
    finally:
        if k.startswith("OPT_"):
            ctx.set_opt(getattr(_lib, k), None)
    assert rc == 0 and data == expected(name)


# ------------------------------------------------------------------ the 2^27-bin table is all zero again after every call
def _hygiene_images():
    a = R.case_image("s64-extremes22")                     # keys 0 and the largest: the table's first page and the last one a key reaches
    b = R.case_image("r100-all64-one65")                   # overflow: the 16-bit gather's counts are swept and the call starts again
    z = np.zeros((64, 64, 3), np.uint8)                    # one symbol, no payload
    s = R.smooth_image(100, 75)
    return {"A": a, "B": b, "Z": z, "S": s}


ORDER = "ASBSZAZBBS"


@pytest.mark.parametrize("mode", ["plain", "failed-calls", "timers-on-alternate-calls"])
def test_table_is_clean_after_every_call(mode):
    """one context; a count left behind by a call adds a leaf to the next call's tree and so changes its header: equality with the oracle is
    the whole assertion.  `failed-calls`: after every A and every B the same image once more into an output too small for it -- the call
    fails half-way (CAPACITY), after the gather has filled the table."""
    from cniic_amd import Context, _lib
    imgs = _hygiene_images()
    want = {k: O.encode("delta", v)[1] for k, v in imgs.items()}
    small = np.empty(16, np.uint8)
    with Context(0) as ctx:
        for i, k in enumerate(ORDER):
            flags = _lib.KM_PROFILE if mode == "timers-on-alternate-calls" and i % 2 else 0
            rc, data, _ = ctx.encode("delta", imgs[k], flags=flags)
            assert rc == 0 and data == want[k], (mode, i, k)
            if mode == "failed-calls" and k in "AB":
                rc, _, _ = ctx.encode("delta", imgs[k], out=small, allow=(_lib.CAPACITY,))
                assert rc == _lib.CAPACITY, (i, k, rc)
