"""What tests/test_persist_trips.py (GPU) and tests/test_persist_trips_cpu.py share: the inputs on which the skip schedule's row test of the
persistent colour K-means (cniic_amd/csrc/k_kmeans_persist.hip, `// SKIP schedule`) changes its group width L or its trip count, a host
model of the width it picks (ps_row_group), and -- from the oracle's trajectory -- the iterations that run the skip schedule and with how
many moved centroids, which is what the `kmeans_rgbw_persist_g4 / _g8 / _g16` marks of a KM_PROFILE run must count.

The inputs are the existing builders': the 64 x 64, 128 x 128 and 300 x 260 photos and the re-seed inputs of
tests/test_persistent_kmeans_state.py (same seeds, same pinned grids, so tests/golden/persist_pair_evals.json has their figures), and
tests/rgbw_lists_ref.py's one-colour-per-cell blocks (`_case_g`), whose single block owns exactly as many cells as the case names."""
import os
from collections import Counter

import numpy as np

import oracle_lib as O
import rgbw_lists_ref as R
from cniic_amd import ps_layout as L, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reseed_golden.npz"))
RGBW = ("rgbw38", "rgbw621", "rgbw1268", "rgbw2355")
MAX_MOVED_SKIP = 64          # kMaxMovedSkip: the default (and largest) CNIIC_KM_MAXSKIP
ROW_FIXED, ROW_TRIP, ROW_CHUNK = 8, 1, 4   # kPsRowFixed, kPsRowTrip, kPsRowChunk
WIDTHS = (4, 8, 16)
THRESHOLDS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)   # CNIIC_KM_MAXSKIP of the threshold cases


def row_group(nS, C):
    """ps_row_group: lanes per cell of the row test in a block of C cells when nS centroids moved"""
    best, best_cost = None, None
    for lg in (2, 3, 4):
        simd_waves = ((C << lg) + 255) >> 8
        trips = (nS + (1 << lg) - 1) >> lg
        cost = simd_waves * (ROW_FIXED + ROW_TRIP * trips + ROW_CHUNK * ((trips + 3) >> 2))
        if best_cost is None or cost < best_cost:
            best, best_cost = 1 << lg, cost
    return best


def photo(h, w, seed):
    return synth.photo(w, h, synth.SEED0 + seed)


def colours_of(img):
    p = img.reshape(-1, 3).astype(np.uint32)
    keys, counts = O.count_freqs((p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2])
    return keys, counts.astype(np.uint32)


def few_cells(M):
    """eight colours in each of M cells (a shuffled choice of the 32768), random pixel counts -> (keys, counts)"""
    rng = np.random.default_rng(100 + M)
    cells = np.sort(rng.permutation(32768)[:M])
    keys = []
    for c in cells:
        off = rng.choice(512, 8, replace=False)
        keys.append(R.key_of(R.cell_box(int(c)) + np.stack([off >> 6, (off >> 3) & 7, off & 7], axis=1)))
    keys = np.sort(np.concatenate(keys).astype(np.uint32))
    return keys, rng.integers(1, 50, len(keys)).astype(np.uint32)


_INPUT = {}


def input_of(name):
    """-> (keys, counts, blocks): the colours of a named input and the grid its cases pin (CNIIC_KM_PS_BLOCKS)"""
    if name not in _INPUT:
        if name.startswith("photo"):
            h, w = (int(x) for x in name[5:].split("x"))
            keys, cnt = colours_of(photo(h, w, seed=5 if (h, w) == (300, 260) else 40 + h))
            _INPUT[name] = (keys, cnt, {64: 8, 128: 32, 300: 16}[h])
        elif name.startswith("rgbw"):
            _INPUT[name] = (GOLD[name + "_keys"], GOLD[name + "_weight"], 4)
        elif name.startswith("cells"):
            c = R._case_g(int(name[5:]))
            _INPUT[name] = (c["keys"], c["w"], 1)
        elif name.startswith("few"):
            _INPUT[name] = few_cells(int(name[3:])) + (1,)
        else:
            c = R.case(name)
            _INPUT[name] = (c["keys"], c["w"], c["blocks"] or 1)
    return _INPUT[name]


def case_K(name, K=None):
    if K is not None:
        return K
    if name.startswith("rgbw"):
        return int(GOLD[name + "_K"][0])
    if name.startswith("cells"):
        return 16
    if name.startswith("few"):
        return 6
    return R.case(name)["K"]


_TRAJ = {}


def moved_per_update(name, K):
    """nS of the oracle's run: centroids moved by the update that closes assign step j (rgbw_lists_ref.moved), and the run"""
    if (name, K) not in _TRAJ:
        keys, w, _ = input_of(name)
        tabs, _, run = R.trajectory(R.pts_of_keys(keys), w, K)
        _TRAJ[(name, K)] = (R.moved(tabs), run)
    return _TRAJ[(name, K)]


def skip_steps(name, K, max_skip=MAX_MOVED_SKIP):
    """the nS in front of every assign step that runs the skip schedule (step j >= 1 with nS <= max_skip, max_skip != 0), in order"""
    nS, run = moved_per_update(name, K)
    return [nS[j - 1] for j in range(1, run["iterations"]) if max_skip and nS[j - 1] <= max_skip]


def grid_of(name):
    keys, _, blocks = input_of(name)
    return R.ps_grid(len(keys), blocks)


def block_cell_counts(name):
    """cells per block at the case's grid (cniic_amd/ps_layout.py: k_cell_scan's cost prefix and k_ps_ranges' boundaries)"""
    keys, _, _ = input_of(name)
    return [len(c) for c in L.block_cells(keys, grid_of(name))]


def expected_marks(name, K, max_skip=MAX_MOVED_SKIP, forced=None, fixed=False):
    """{4: n, 8: n, 16: n}: iterations of block 0 per group width -- what the g4 / g8 / g16 marks of a KM_PROFILE run count"""
    C0 = block_cell_counts(name)[0]
    got = Counter(forced if forced else 16 if fixed else row_group(n, C0) for n in skip_steps(name, K, max_skip))
    return {Lw: got.get(Lw, 0) for Lw in WIDTHS}


# ---- the cases: (id, input, K, environment beyond the pinned grid, flags name or None)
THRESHOLD_INPUT = ("photo300x260", 255)      # its run has an update that moves exactly 1, 4, 5, 8, 9, 16, 17, 32 and 33 centroids ...
FULL_INPUT = ("photo64x64", 64)              # ... and this one's first update moves 64 = kMaxMovedSkip (and 1, 4, 5 later)
BLOCK_CELLS = (128, 129, 256, 257)           # one block that owns exactly this many cells
FEW_CELLS = {4: 3, 8: 7, 16: 15}             # ... and one that owns fewer cells than a group has lanes
