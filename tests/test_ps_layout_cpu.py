"""cniic_amd/ps_layout.py (the host model of the persistent K-means' LDS layout that tools/ps_resident.py and
tests/test_persistent_kmeans_state.py use) against the header it mirrors and against the suite's own model of the same kernels
(tests/rgbw_lists_ref.py, whose constants tests/test_rgbw_lists_cpu.py holds to the header's text): a constant that moves in
csrc/kmeans_rgbw.hpp and not here fails on the CPU."""
import os

import numpy as np

import rgbw_lists_ref as R
from cniic_amd import ps_layout as L, synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cniic_amd", "csrc")


def test_constants_are_the_headers():
    text = " ".join(open(os.path.join(CSRC, "kmeans_rgbw.hpp")).read().split())
    assert "constexpr uint32_t kPsRunWords = 5 * 256;" in text and L.PS_RUN_BYTES == 5 * 256 * 8
    assert "constexpr uint32_t kPsBudget = kPsDynBytes - kPsRunWords * 8;" in text and L.PS_BUDGET == R.kPsDynBytes - L.PS_RUN_BYTES == 150528
    assert (L.PS_CHUNKS, L.PS_SLOTS_MAX, L.PS_SCAP, L.PS_REC_WORDS, L.PS_MAX_CELLS) == (R.kPsChunks, R.kPsSlotsMax, R.kPsScap, R.kPsRecWords, R.kPsMaxCells)
    assert (L.PS_OFF_CELL, L.CELL_FIXED_COST, L.CELL_SWEEP_COST) == (R.kPsOffCell, R.kCellFixedCost, R.kCellSweepCost)
    assert all(L.ps_cell_bytes(C) == R.ps_cell_bytes(C) for C in (0, 1, 3, 4, 5, 528, 2047, 2048))
    assert L.ps_cell_bytes(8) - L.ps_cell_bytes(4) == 4 * L.PS_CELL_DESC_BYTES
    assert L.PS_OFF_CELL + L.ps_cell_bytes(L.PS_MAX_CELLS) <= L.PS_BUDGET   # (the header's static_assert)


def test_dealing_is_the_suites_model():
    img = synth.photo(300, 260, synth.SEED0 + 5).reshape(-1, 3).astype(np.uint32)
    keys = np.unique((img[:, 0] << 16) | (img[:, 1] << 8) | img[:, 2])
    assert np.array_equal(L.cell_of(keys), R.cell_of(keys))
    cells, n = np.unique(R.cell_of(keys), return_counts=True)
    for G in (1, 16, 37):
        ref = R.ps_ranges(cells, n, G)
        mine = L.block_cells(keys, G)
        assert [len(c) for c in mine] == ref["ncells"]
        assert all(np.array_equal(c, n[b]) for c, b in zip(mine, ref["blocks"]))
    smallest = L.smallest_budget(keys, 16)
    assert smallest == L.PS_OFF_CELL + L.ps_cell_bytes(max(R.ps_ranges(cells, n, 16)["ncells"]))
    assert L.resident_points(keys, 16, smallest)[2] == 0 and L.resident_points(keys, 16, smallest - 1)[2] >= 1
    res, tot, refused = L.resident_points(keys, 16)
    assert (res, tot, refused) == (keys.size, keys.size, 0)
