"""Without a GPU: the cases of tests/test_persist_trips.py sit on the boundaries they are there for, from the oracle's trajectory
(tests/rgbw_lists_ref.py) and the host model of the block ranges (cniic_amd/ps_layout.py), and tests/persist_trips_ref.py's model of the
row test's group width is the kernel's ps_row_group (cniic_amd/csrc/k_kmeans_persist.hip): its constants are read from the source."""
import os
import re

import persist_trips_ref as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cniic_amd", "csrc")


def test_the_cost_constants_are_the_kernels():
    text = " ".join(open(os.path.join(CSRC, "k_kmeans_persist.hip")).read().split())
    m = re.search(r"constexpr uint32_t kPsRowFixed = (\d+), kPsRowTrip = (\d+), kPsRowChunk = (\d+);", text)
    assert m and tuple(int(x) for x in m.groups()) == (P.ROW_FIXED, P.ROW_TRIP, P.ROW_CHUNK)
    assert "const uint32_t simd_waves = ((C << lg) + 255u) >> 8, trips = (nS + (1u << lg) - 1u) >> lg;" in text
    assert "const uint32_t cost = simd_waves * (kPsRowFixed + kPsRowTrip * trips + kPsRowChunk * ((trips + 3u) >> 2));" in text
    assert "if (cost < best_cost) { best_cost = cost; best_lg = lg; }" in text   # (ascending lg: the narrower group on a tie)
    hdr = " ".join(open(os.path.join(CSRC, "kmeans_rgbw.hpp")).read().split())
    assert "constexpr uint32_t kMaxMovedSkip = %d;" % P.MAX_MOVED_SKIP in hdr


def test_the_width_model_where_it_switches():
    """a block of the headline encode (119 .. 132 cells) takes 4 lanes per cell whatever moved: two (three) waves a SIMD instead of
    four (five) and eight (nine); a block whose cells fit one wave a SIMD at every width takes the widest group that saves trips"""
    assert all(P.row_group(n, C) == 4 for n in range(1, 65) for C in (119, 126, 128, 129, 132, 256, 257))
    assert [P.row_group(n, 16) for n in (1, 4, 5, 8, 9, 16, 17, 64)] == [4, 4, 8, 8, 16, 16, 16, 16]
    assert [P.row_group(n, 32) for n in (1, 4, 5, 8, 9, 64)] == [4, 4, 8, 8, 8, 8]       # (16 lanes a cell: 32 cells are two waves a SIMD)
    assert [P.row_group(n, 3) for n in (1, 5, 17)] == [4, 8, 16]


def test_the_threshold_cases_reach_every_threshold():
    """CNIIC_KM_MAXSKIP = m runs the skip schedule exactly where at most m centroids moved: the input's run has an update that moves
    exactly m, so m admits an iteration that m - 1 does not"""
    name, K = P.THRESHOLD_INPUT
    nS, run = P.moved_per_update(name, K)
    before_a_step = set(nS[:run["iterations"] - 1])
    assert set(P.THRESHOLDS) - {64} <= before_a_step
    for m in P.THRESHOLDS:
        steps = P.skip_steps(name, K, m)
        assert steps and max(steps) <= m and (m == 64 or max(steps) == m)
        assert len(steps) > len(P.skip_steps(name, K, m - 1)) or m == 64
    name, K = P.FULL_INPUT
    assert P.skip_steps(name, K, 64)[0] == 64 and len(P.skip_steps(name, K, 63)) == len(P.skip_steps(name, K, 64)) - 1


def test_every_forced_width_meets_one_its_width_one_more_and_64_moved_centroids():
    seen = set(P.skip_steps(*P.THRESHOLD_INPUT)) | set(P.skip_steps(*P.FULL_INPUT))
    for Lw in P.WIDTHS:
        assert {1, Lw, Lw + 1, 64} <= seen, Lw


def test_the_block_cases_own_the_cells_they_name():
    for M in P.BLOCK_CELLS:
        name = "cells%d" % M
        assert P.block_cell_counts(name) == [M]
        steps = P.skip_steps(name, P.case_K(name))
        assert len(steps) >= 3 and min(steps) >= 1
    for Lw, M in P.FEW_CELLS.items():
        name = "few%d" % M
        assert P.block_cell_counts(name) == [M] and M < Lw
        assert len(P.skip_steps(name, P.case_K(name))) >= 1
    # 128 | 129: one pass of the block's lanes at 8 lanes a cell against two; 256 | 257: the same at 4 lanes a cell
    assert (128 * 8 + 1023) // 1024 == 1 and (129 * 8 + 1023) // 1024 == 2 and (256 * 4 + 1023) // 1024 == 1 and (257 * 4 + 1023) // 1024 == 2


def test_the_photo_cases_have_blocks_on_both_sides_of_the_default_choice():
    """the marks count block 0's iterations: the photo inputs' block 0 takes 4 lanes a cell in most iterations and 8 in some
    (64 x 64, K = 64: 90 cells, two waves a SIMD at both widths while more than 16 centroids move)"""
    name, K = P.FULL_INPUT
    marks = P.expected_marks(name, K)
    assert marks[4] >= 1 and marks[8] >= 1 and sum(marks.values()) == len(P.skip_steps(name, K))
    marks = P.expected_marks("rgbw1268", P.case_K("rgbw1268"))
    assert marks[4] >= 1 and marks[8] >= 1 and marks[16] >= 1
