"""The case table and the model of tests/rle_exact_edges.py, without a GPU: the granularities are the kernels' (read out of k_rle.hip), every
case has the property it is named for (computed from runs_np), the restatement, the model without defects and the oracle give one stream
for every case and the oracle decodes it back to the row, the oracle's scan of every n x 1 used is the identity -- and the part that says
what the GPU test is worth: every killable defect of the model changes the stream of at least one case, and which GROUPS of cases catch
which defect.

Six of the eight groups are the only ones to catch some defect (ONLY_KILLER).  The cap's-phase group (3) and the look-ahead group (7) are
not, and cannot be with rows like these: a flat row of 65 chunks or more (groups 4 and 5) walks through every phase of the 255-cap at
every thread offset and every look-ahead distance, so it catches whatever those two catch.  What they add is stated as properties instead
(test_case_stands_where_it_claims_to, test_the_table_reaches_what_it_is_there_for): the 255th and 256th element and the runs behind them
ON j = 0, j = 15, a wave's lane 0 and a chunk's first position, in rows of three chunks, so that a failure there names the handover
without a four-million-pixel row."""
import functools
import os
import re
import struct

import numpy as np
import pytest

import oracle_lib as O
import rle_approx_ref as RA
import rle_exact_edges as E

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cniic_amd", "csrc")

# group -> a defect that no other group's cases tell from the right stream
ONLY_KILLER = {1: "fast_path_sentinel_is_black", 2: "key_drops_bit_%d", 4: "carry_local_wave_total_from_lane0", 5: "carry_add_only_previous_block",
               6: "offsets_block_total_16_bits", 8: "tail_path_sentinel_is_black"}


def test_the_granularities_are_the_kernels():
    src = open(os.path.join(CSRC, "k_rle.hip")).read()
    assert re.search(r"constexpr int kRleThreads = %d;" % E.THREADS, src)
    assert re.search(r"constexpr int kRlePer = %d;" % E.PER, src)
    assert re.search(r"constexpr uint32_t kRleChunk = kRleThreads \* kRlePer;", src) and E.CHUNK == E.THREADS * E.PER == 4096
    assert re.search(r"constexpr uint32_t kRleMaxRun = %d;" % E.CAP, src)
    # the carry kernels and the single-block offsets: 1024 chunks per block, 64 per wave
    for kernel in ("k_rle_carry_local", "k_rle_carry_add", "k_rle_offsets"):
        assert re.search(r"__global__ __launch_bounds__\(%d\) void %s\(" % (E.SCAN, kernel), src), kernel
    assert "blockIdx.x * %d + threadIdx.x" % E.SCAN in src and "if (nchunks > %d)" % E.SCAN in src and "(nchunks + 1023) / 1024" in src
    assert E.BLOCK == E.SCAN * E.CHUNK == 4194304 and E.WAVE == 64 * E.PER == 1024 and E.LANES == 64
    # the look-ahead: 16 threads, 16 more flag words
    assert "s_f[kRleThreads + 16]" in src and "for (uint32_t k = 1; k <= 16; k++)" in src and "s_rec[3 * kRleChunk]" in src
    assert "0xffffffffu;  // no colour has this key" in src and E.SENTINEL == 0xffffffff


def test_row_builder_and_restatement_against_the_python_encoder():
    """row() puts the starts where it is told; runs_np / stream_np equal the per-pixel Python restatement of the codec at d = 0"""
    img = E.row(1000, [1, 17, 300, 999])
    assert img.shape == (1, 1000, 3) and E.segment_starts_np(img[0]).tolist() == [0, 1, 17, 300, 999]
    assert E.row(5, [0, 5, 7, 2, 2]).reshape(-1, 3).tolist() == [list(E.A)] * 2 + [list(E.B)] * 3
    with pytest.raises(AssertionError):
        E.row(4, [2], palette=(E.A, E.A))
    rng = np.random.default_rng(3)
    for n in (1, 2, 254, 255, 256, 700, 5000):
        for lin in (E.row(n, rng.integers(1, max(n, 2), 5))[0], E.noise_row(n)[0], E.row(n, [])[0]):
            want = RA.encode_py(lin, n, 1, 0.0)
            assert E.stream_np(lin, n, 1) == want == E.model(lin)
    start, count, colour = E.runs_np(E.row(600, [100])[0])
    assert start.tolist() == [0, 100, 355] and count.tolist() == [100, 255, 245] and colour.tolist() == [list(E.A), list(E.B), list(E.B)]


@functools.lru_cache(maxsize=None)
def _scan_is_identity(n):
    xy = O.hilbert_iter(n, 1)
    return bool((xy[:, 0] == np.arange(n, dtype=np.uint32)).all() and not xy[:, 1].any())


@functools.lru_cache(maxsize=2)
def _image(name):
    return E.case_image(name)


@functools.lru_cache(maxsize=None)
def _kills(name):
    """the killable defects that change this case's stream; with it the checks that need the row built: the three streams and the round trip"""
    c = E.BY_NAME[name]
    img = _image(name)
    lin = img.reshape(-1, 3)
    clean = E.model(lin, want_stages=True)
    want = E.stream_np(lin, c.n, 1)
    rc, data, _ = O.encode("hilbert(rle)", img)
    assert rc == 0 and len(want) == len(data) == len(clean["stream"]), name
    assert want == data, (name, E.first_difference(want, data))
    assert clean["stream"] == data, (name, E.first_difference(clean["stream"], data))
    rc, back = O.decode("hilbert(rle)", data)
    assert rc == 0 and np.array_equal(back, img), name
    assert len(data) <= 8 + 12 * 2110000, "the largest stream stays at about 25 MB"
    assert E.model(lin, ("phase_in_32_bits",), clean=clean) == data   # (not killable: see model())
    return frozenset(d for d in E.KILLABLE if E.model(lin, (d,), clean=clean) != data)


def _segments(lin):
    st = E.segment_starts_np(lin)
    return st, np.diff(np.append(st, lin.shape[0]))


@pytest.mark.parametrize("name", E.NAMES)
def test_case_stands_where_it_claims_to(name):
    c = E.BY_NAME[name]
    img = _image(name)
    assert img.shape == (1, c.n, 3) and c.n <= 2 * E.BLOCK + E.CHUNK + 5
    assert _scan_is_identity(c.n)
    lin = img.reshape(-1, 3)
    st, ln = _segments(lin)
    start, count, _ = E.runs_np(lin)
    F = c.facts
    if "starts" in F:
        assert st.tolist() == [0] + sorted(F["starts"])
    if c.group == 1 and "at" in F:
        p = F["at"]
        inner = set(st.tolist())
        assert (p in inner and len(inner) == 2) if name.endswith("_change") else (p not in inner and p - 1 in inner and (p + 1 in inner or p + 1 == c.n))
    if c.group == 2:
        p, = F["starts"]
        k = E.keys_of(lin)
        assert int(k[p]) ^ int(k[p - 1]) == 1 << F["bit"]
        assert (p // E.CHUNK + 1) * E.CHUNK <= c.n if name.endswith("_whole") else p // E.CHUNK == c.n // E.CHUNK and c.n % E.CHUNK
    if c.group == 3:
        s, L = F["seg"]
        i = st.tolist().index(s)
        assert ln[i] == L
        mine = start[(start >= s) & (start < s + L)]
        assert mine.tolist() == list(range(s, s + L, E.CAP))
        if "residue" in F:
            assert s + L == c.n and L % E.CAP == F["residue"] and count[-1] == (F["residue"] or E.CAP)
    if c.group == 4:
        s, L = F["seg"]
        i = st.tolist().index(s)
        first_whole = s // E.CHUNK + 1
        assert ln[i] == L and (s + L) // E.CHUNK == first_whole + F["whole"]   # chunks first_whole .. first_whole + whole - 1 hold no start
        assert first_whole <= 64 < first_whole + F["whole"] < E.SCAN          # chunk 64: lane 0 of the carry scan's second wave
        assert name.endswith("from5") == (s // E.CHUNK % E.LANES == 0)          # ... found from lane 0 (chunk 0) and from another lane (chunk 3)
    if name.startswith("block_start_at"):
        s = F["at"]
        assert s in st and (s + 3 * E.CHUNK in st or s + 3 * E.CHUNK == c.n) and c.n == E.BLOCK + 3 * E.CHUNK + 1 and len(st) <= 3
    if name.startswith("block_without_a_start"):
        assert not ((st >= E.BLOCK) & (st < 2 * E.BLOCK)).any()
        i = np.searchsorted(st, E.BLOCK, side="right") - 1
        assert st[i] == E.BLOCK - 3 and st[i] + ln[i] > 2 * E.BLOCK       # the segment covering block 1 starts in block 0 and ends in block 2
        inside = start[(start >= 2 * E.BLOCK) & (start < st[i] + ln[i])]   # its runs that start inside block 2: they need block 0's start
        assert (inside.size > 0) == name.endswith("_far")
    if name == "blocks_all_flat":
        assert st.tolist() == [0] and c.n == 2 * E.BLOCK + E.CHUNK + 5
    if c.group == 6 or name == "look_4096_runs_then_flat":
        per_chunk = np.bincount(start // E.CHUNK, minlength=F["nchunks"])
        assert per_chunk.size == F["nchunks"] == -(-c.n // E.CHUNK)
        if "noise" in name:
            assert 0.45 * c.n <= start.size <= 0.55 * c.n and (per_chunk[:c.n // E.CHUNK] > 1500).all()
        else:
            full = per_chunk[:c.n // E.CHUNK]
            assert (full[0::2] == E.CHUNK).all() and (full[1::2] == 17).all() and per_chunk.max() == E.CHUNK   # the staging buffer exactly full
    if c.group == 7 and "run" in F:
        s = F["run"]
        i = start.tolist().index(s)
        j = s % E.PER
        assert count[i] == E.CAP and s in st                              # a whole run of 255 from a start ...
        assert (start[start // E.PER == s // E.PER] <= s).all()           # ... that is its thread's last flag
        if F.get("ends_image"):
            assert i == start.size - 1 and s + E.CAP == c.n and s // E.CHUNK == (c.n - 1) // E.CHUNK
        else:
            nxt = int(start[i + 1])
            assert 240 < nxt - s <= E.CAP and nxt in st and nxt // E.PER - s // E.PER == (16 if j else 15)
            if name.endswith("chunk_end"):
                assert nxt // E.CHUNK == s // E.CHUNK + 1 and nxt % E.CHUNK // E.PER < 16 and s % E.CHUNK // E.PER >= E.THREADS - 16
    if c.group == 8:
        assert start.size == (c.n if "alternating" in name else -(-c.n // E.CAP)) and c.n < E.CHUNK
    _kills(name)   # the streams: restatement == model == oracle, and the round trip


def test_the_table_reaches_what_it_is_there_for():
    names = set(E.NAMES)
    # 1. every edge, with a change and without, on the 16-byte path and on the byte-wise one
    for e, (n, p) in E.EDGES.items():
        assert {"edge_%s_change" % e, "edge_%s_none" % e} <= names
    at = lambda e: E.EDGES[e][1]   # noqa: E731
    n1, n1w = E.N1, E.N1W
    assert n1 == 2 * E.CHUNK + 17 and n1w // E.CHUNK == 2 and n1w % E.CHUNK > E.WAVE
    assert at("per0") % E.PER == 0 and at("per0") % E.WAVE and at("per15") % E.PER == 15
    assert at("wave0") % E.WAVE == 0 and at("wave0") % E.CHUNK and at("wave_last") % E.WAVE == E.WAVE - 1 and at("wave0_chunk1") // E.CHUNK == 1
    assert at("chunk0") == E.CHUNK and at("chunk_last") == E.CHUNK - 1
    tail = [e for e in E.EDGES if at(e) >= 2 * E.CHUNK]
    assert {at(e) % E.PER for e in tail} >= {0, 15} and at("tail_chunk0") % E.CHUNK == 0 and at("before_tail") == 2 * E.CHUNK - 1
    assert at("tail_wave0") % E.WAVE == 0 and at("tail_wave0") % E.CHUNK and at("tail_wave_last") % E.WAVE == E.WAVE - 1
    assert at("last_pixel") == n1 - 1 and at("last_pixel_w") == n1w - 1
    # 2. every bit of the key, both paths
    assert {"bit%02d_%s" % (b, w) for b in range(24) for w in ("whole", "tail")} <= names
    # 3. L x s complete; element k of a segment (0-based 254: the 255th, the last of a run; 255 and 510: the first of the next run) falls on
    # j = 0, on j = 15, on a wave's lane 0 and on a chunk's first position
    assert {"cap_L%d_s_%s" % (L, s) for L in E.L_VALUES for s in E.S_VALUES} <= names and set(E.L_VALUES) == {254, 255, 256, 509, 510, 511, 4080, 4335}
    assert sorted(E.S_VALUES.values()) == sorted([0, 1, 15, 16, E.CHUNK - 1, E.CHUNK, E.CHUNK - 254, E.CHUNK - 255])
    for k in (254, 255):
        hit = {s + k for s in E.S_VALUES.values()}
        assert {p % E.PER for p in hit} >= {0, 15} and any(p % E.WAVE == 0 for p in hit) and any(p % E.CHUNK == 0 for p in hit), k
    # (with these s the 510th element and the third run's first reach j = 15, and the latter j = 0; no wave or chunk edge)
    assert 15 in {(s + 509) % E.PER for s in E.S_VALUES.values()} and {(s + 510) % E.PER for s in E.S_VALUES.values()} >= {0, 15}
    assert {"cap_ends_at_n_r%d" % r for r in (0, 1, 254)} <= names
    # 5. | 6.
    assert {E.BY_NAME["block_start_at_%s" % s].facts["at"] - E.BLOCK for s in ("m1", "0", "p1")} == {-1, 0, 1}
    assert {E.BY_NAME[k + "_" + s].n for k in ("noise", "alternating") for s in ("1024_chunks", "1025_chunks", "1_chunk", "2_chunks")} == {E.BLOCK, E.BLOCK + 1, E.CHUNK, E.CHUNK + 1}
    # 7. | 8.
    assert {"look_j%d_%s" % (j, w) for j in (0, 1, 15) for w in ("mid", "chunk_end", "image_end")} <= names
    assert {"tiny_%d_%s" % (n, k) for n in (1, 2, 15, 16, 17, 255, 256, 257) for k in ("flat", "alternating")} <= names
    assert {c.group for c in E.CASES} == set(E.GROUPS)


def test_colours_of_every_other_group_differ_in_many_bits():
    """a kernel that mixes up or loses a channel bit must be caught by group 2 and may not be caught by accident elsewhere: everywhere else two
    neighbouring colours differ in at least two bits of the key"""
    pop = lambda x: bin(x).count("1")   # noqa: E731
    for c in E.CASES:
        if c.group == 2 or c.n >= E.LARGE:
            continue
        k = E.keys_of(E.case_image(c.name)[0])
        x = np.unique(k[1:] ^ k[:-1])
        assert all(pop(int(v)) >= 2 for v in x if v), c.name
    pairs = [(E.A, E.B), (E.B, E.C), (E.C, E.A)]
    assert all(pop(int(E.keys_of(np.array([a]))[0]) ^ int(E.keys_of(np.array([b]))[0])) >= 2 for a, b in pairs)


def test_every_killable_defect_is_caught_and_by_which_group():
    killers = {d: set() for d in E.KILLABLE}   # defect -> the groups with a case whose stream it changes
    for c in E.CASES:
        for d in _kills(c.name):
            killers[d].add(c.group)
    assert all(killers.values()), [d for d, g in killers.items() if not g]
    assert not E.DEFECTS["phase_in_32_bits"][1] and "phase_in_32_bits" not in killers
    # no group is decorative: every one catches some defect ...
    caught_by = {g: {d for d, gs in killers.items() if g in gs} for g in E.GROUPS}
    assert all(caught_by.values()), caught_by
    # ... and these are the only ones to catch theirs
    for g, d in ONLY_KILLER.items():
        for name in ([d % b for b in range(24)] if "%d" in d else [d]):
            assert killers[name] == {g}, (name, killers[name])
    # the two groups that own no defect catch what the handovers they are named for can get wrong, in rows of three chunks
    assert {"lookahead_15_threads", "lookahead_stops_at_chunk_end", "flags_ignore_carry", "chunk_first_thread_no_predecessor",
            "lane0_uses_lane_below"} <= caught_by[3] & caught_by[7]
    assert set(E.GROUPS) - set(ONLY_KILLER) == {3, 7}
    # the handovers of the carry scan, by case: the second level only by rows over more than one block
    assert {g for d in ("carry_add_skipped", "carry_add_only_previous_block") for g in killers[d]} == {5}
    assert killers["carry_local_drops_wave_prefix"] == {4, 5}
    assert "carry_add_only_previous_block" in _kills("block_without_a_start_far") and "carry_add_only_previous_block" not in _kills("block_without_a_start")
    assert killers["offsets_off_by_one_chunk_at_1025"] == {5, 6} and killers["tail_path_ignores_last_pixel"] >= {1, 8}


def test_first_difference_names_the_handover():
    lin = E.case_image("cap_L255_s_chunk_m1")[0]
    want = E.stream_np(lin, lin.shape[0], 1)
    got = E.model(lin, ("lookahead_stops_at_chunk_end",))
    msg = E.first_difference(got, want)
    assert "chunk 0 (block 0, wave-lane 0), thread 255, j 15" in msg and "expected count 255" in msg, msg
    assert E.first_difference(want, want) is None
    assert "headers differ" in E.first_difference(struct.pack("<II", 1, 2) + want[8:], want)
