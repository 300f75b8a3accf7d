"""Host model of how the persistent colour K-means (csrc/k_kmeans_persist.hip) deals an image's cells to its blocks and how much of a
block's LDS its points get: the constants of csrc/kmeans_rgbw.hpp, k_cell_scan's cost prefix, k_ps_ranges' chunk boundaries and
the kernel's own count of resident cells, in numpy.  For the tests (the LDS budgets at which a launch is still accepted) and for
tools/ps_resident.py (how many points of an image stay in LDS); nothing on a hot path."""
import numpy as np

# ---- csrc/kmeans_rgbw.hpp
PS_CHUNKS = 24            # kPsChunks
PS_SLOTS_MAX = 32         # kPsSlotsMax
PS_SCAP = 96              # kPsScap
PS_REC_WORDS = 11         # kPsRecWords
PS_MAX_CELLS = 2048       # kPsMaxCells
PS_OFF_CELL = 5 * 256 * 8 + 256 * 8 + PS_SLOTS_MAX * PS_SCAP * 4   # kPsOffCell: accumulators, table and shared lists in front of the cells
PS_RUN_BYTES = 5 * 256 * 8                 # kPsRunWords x 8: the running sums, the top of the launch's dynamic LDS (kPsDynBytes)
PS_BUDGET = 160 * 1024 - 3072 - PS_RUN_BYTES   # kPsBudget: what is left for a block's cells and points, the full budget
CELL_FIXED_COST = 512     # kCellFixedCost
CELL_SWEEP_COST = 256     # kCellSweepCost
PS_CELL_DESC_BYTES = 4 + 4 + PS_REC_WORDS * 4 + 2 + 2 + 1   # one cell's descriptor (ps_cell_bytes grows by four of them at a time)


def ps_cell_bytes(C):
    """ps_cell_bytes: the descriptors of a block that owns C cells"""
    return 16 + ((C + 3) & ~3) * PS_CELL_DESC_BYTES


def cell_of(keys):
    """device_utils.hpp cell_of: the 8^3 cell of a 0xRRGGBB key, numbered super-cell (32^3) major"""
    keys = np.asarray(keys, np.uint32)
    rc, gc, bc = (keys >> 16 & 255) >> 3, (keys >> 8 & 255) >> 3, (keys & 255) >> 3
    sup = ((rc >> 2) * 8 + (gc >> 2)) * 8 + (bc >> 2)
    return (sup << 6) | ((rc & 3) << 4) | ((gc & 3) << 2) | (bc & 3)


def block_cells(keys, G):
    """The distinct colours `keys` dealt to G blocks: a list, per block, of the point counts of its cells in the block's own order
    (chunks b, G + b, 2 G + b, ... of the compacted cell list, cut at equal estimated cost: k_cell_scan + k_ps_ranges)."""
    counts = np.bincount(cell_of(np.unique(keys)), minlength=32768).astype(np.int64)
    n = counts[counts > 0]                                   # points of the non-empty cells, ascending cell id
    M = n.size
    sweeps = (n + 255) // 256
    cost = np.zeros(M + 1, np.int64)                          # ne_cost[m]: sweeps before cell m x sweep cost + m x fixed cost
    cost[1:] = np.cumsum(sweeps) * CELL_SWEEP_COST + np.arange(1, M + 1) * CELL_FIXED_COST
    NC = G * PS_CHUNKS
    target = [int(cost[M]) * g // NC for g in range(NC + 1)]
    cb = np.searchsorted(cost[:M], target, side="left")      # first cell whose cost prefix is >= the target
    cb[NC] = M
    return [np.concatenate([n[cb[r * G + b]:cb[r * G + b + 1]] for r in range(PS_CHUNKS)]) for b in range(G)]


def smallest_budget(keys, G, off_cell=PS_OFF_CELL):
    """the smallest dynamic-LDS budget k_ps_ranges accepts for these colours on G blocks: the descriptors of the block with most cells"""
    return off_cell + ps_cell_bytes(max(len(c) for c in block_cells(keys, G)))


def resident_points(keys, G, budget=PS_BUDGET, off_cell=PS_OFF_CELL):
    """(points whose packed word stays in LDS, all points, blocks that would be refused) for budget bytes of dynamic LDS a block"""
    res = tot = refused = 0
    for n in block_cells(keys, G):
        tot += int(n.sum())
        if len(n) > PS_MAX_CELLS or off_cell + ps_cell_bytes(len(n)) > budget:
            refused += 1
            continue
        cap = (budget - off_cell - ps_cell_bytes(len(n))) // 4
        ends = np.cumsum(n)
        fit = int(np.searchsorted(ends, cap, side="right"))  # the leading cells whose points end at or below cap
        res += int(ends[fit - 1]) if fit else 0
    return res, tot, refused
