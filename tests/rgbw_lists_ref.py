"""A numpy restatement (int64: nothing here can wrap) of the lists the two colour K-means kernels are built around -- the persistent launch
(cniic_amd/csrc/k_kmeans_persist.hip) and the launch-per-iteration loop (k_rgbw_assign_cells, k_kmeans_rgbw.hip) -- for tests that must KNOW,
from the oracle's trajectory and before anything runs on a GPU, that a case sits on the switch it is there for (tests/test_rgbw_lists_cpu.py
asserts it without a GPU, tests/test_rgbw_limits.py runs the cases).

Colour space is cut into 8^3 cells, 4 x 4 x 4 of them a 32^3 super-cell.  Per full-schedule iteration a super-cell's LIST is what its pivot (the
centroid nearest the cube's centre, lowest id among equals) does not dominate over the whole cube; a cell's CANDIDATES are what the cell's
pivot -- chosen among the list's members -- does not dominate over the cell's cube, taken from the list or, where the list is not kept, from
the whole table.  Both kernels are exact only through their fall-backs:
    persistent   a list of more than kPsScap members is not kept; a block keeps kPsSlotsMax lists, one per (chunk, super-cell) run of its cells;
                 a cell of more than four candidates walks its mask; a block of more than kPsMaxCells cells is refused
    launches     a list of more than km_scap(K) members is not kept; a candidate strip of more than km_ccap(K) entries sweeps the table
    both         more than max_skip moved centroids: the full schedule instead of the skip schedule
"""
import numpy as np

import oracle_lib as O
import warm_ref as W

# ---- constants, with the line that defines them (tests/test_rgbw_lists_cpu.py reads the headers as text and compares)
CONSTANTS = {
    # name: (value, header, the text the definition must contain)
    "kCellShift": (3, "common.hpp", "constexpr int kCellShift = 3;"),
    "kSuperShift": (6, "device_utils.hpp", "constexpr int kSuperShift = 6;"),
    "kPsScap": (96, "kmeans_rgbw.hpp", "constexpr uint32_t kPsScap = 96;"),
    "kPsSlotsMax": (32, "kmeans_rgbw.hpp", "constexpr uint32_t kPsSlotsMax = 32;"),
    "kPsMaxCells": (2048, "kmeans_rgbw.hpp", "constexpr uint32_t kPsMaxCells = 2048;"),
    "kPsChunks": (24, "kmeans_rgbw.hpp", "constexpr uint32_t kPsChunks = 24;"),
    "kPsRecWords": (11, "kmeans_rgbw.hpp", "constexpr uint32_t kPsRecWords = 11;"),
    "kPsDynBytes": (160 * 1024 - 3072, "kmeans_rgbw.hpp", "constexpr uint32_t kPsDynBytes = 160 * 1024 - 3072;"),
    "kPsOffCell": (5 * 256 * 8 + 256 * 8 + 32 * 96 * 4, "kmeans_rgbw.hpp", "constexpr uint32_t kPsOffCell = 5 * 256 * 8 + 256 * 8 + kPsSlotsMax * kPsScap * 4;"),
    "ps_cell_bytes": (None, "kmeans_rgbw.hpp", "ps_cell_bytes(uint32_t C) { return 16u + ((C + 3u) & ~3u) * (4u + 4u + kPsRecWords * 4u + 2u + 2u + 1u); }"),
    "km_scap": (None, "kmeans_rgbw.hpp", "km_scap(uint32_t K) { return K <= 256 ? (K + 1) / 2 : (K + 1) / 2 < 512u ? (K + 1) / 2 : 512u; }"),
    "km_ccap": (None, "kmeans_rgbw.hpp", "km_ccap(uint32_t K) { return K <= 256 ? K : 256u; }"),
    "kMaxMovedSkip": (64, "kmeans_rgbw.hpp", "constexpr uint32_t kMaxMovedSkip = 64;"),
    "kAggMin": (16, "kmeans_rgbw.hpp", "constexpr uint32_t kAggMin = 16;"),
    "kAggLaunches": (3, "kmeans_rgbw.hpp", "constexpr uint32_t kAggLaunches = 3;"),
    "kCellFixedCost": (512, "kmeans_rgbw.hpp", "constexpr uint32_t kCellFixedCost = 512;"),
    "kCellSweepCost": (256, "kmeans_rgbw.hpp", "constexpr uint32_t kCellSweepCost = 256;"),
    "kSweep": (4, "kmeans_rgbw.hpp", "constexpr int kSweep = 4;"),
}
kCellShift, kSuperShift = 3, 6
kPsScap, kPsSlotsMax, kPsMaxCells, kPsChunks, kPsRecWords = 96, 32, 2048, 24, 11
kPsDynBytes, kPsOffCell = 160 * 1024 - 3072, 5 * 256 * 8 + 256 * 8 + 32 * 96 * 4
kMaxMovedSkip, kAggMin, kAggLaunches, kCellFixedCost, kCellSweepCost, kSweep = 64, 16, 3, 512, 256, 4
SUPERS_PER_DIM = (256 >> kCellShift) // 4   # kSupersPerDim, device_utils.hpp
CELL_EXT, SUPER_EXT = (1 << kCellShift) - 1, (1 << (kCellShift + 2)) - 1   # a cube is [lo, lo + ext]^3


def ps_cell_bytes(C):
    return 16 + ((C + 3) & ~3) * (4 + 4 + kPsRecWords * 4 + 2 + 2 + 1)


def km_scap(K):
    return (K + 1) // 2 if K <= 256 else min((K + 1) // 2, 512)


def km_ccap(K):
    return K if K <= 256 else 256


# ---- cells and cubes (device_utils.hpp: cell_of; kmeans_rgbw.hpp: super_box, cell_box)
def cell_of(key):
    key = np.asarray(key, np.int64)
    rc, gc, bc = ((key >> 16) & 255) >> kCellShift, ((key >> 8) & 255) >> kCellShift, (key & 255) >> kCellShift
    sup = ((rc >> 2) * SUPERS_PER_DIM + (gc >> 2)) * SUPERS_PER_DIM + (bc >> 2)
    return (sup << kSuperShift) | ((rc & 3) << 4) | ((gc & 3) << 2) | (bc & 3)


def super_box(sup):
    """low corner (..., 3) of super-cell sup"""
    sup = np.asarray(sup, np.int64)
    return np.stack([(sup // (SUPERS_PER_DIM * SUPERS_PER_DIM)) << (kCellShift + 2), ((sup // SUPERS_PER_DIM) % SUPERS_PER_DIM) << (kCellShift + 2),
                     (sup % SUPERS_PER_DIM) << (kCellShift + 2)], axis=-1)


def cell_box(c):
    c = np.asarray(c, np.int64)
    return super_box(c >> kSuperShift) + np.stack([((c >> 4) & 3) << kCellShift, ((c >> 2) & 3) << kCellShift, (c & 3) << kCellShift], axis=-1)


def key_of(rgb):
    rgb = np.asarray(rgb, np.int64)
    return ((rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]).astype(np.uint32)


# ---- the pruning test (kmeans_rgbw.hpp: Dominance)
def worst(pivot, lo, ext, v):
    """Dominance::worst: the maximum over the cube [lo, lo + ext]^3 of d(x, pivot) - d(x, v); v can be nearest (or tie) somewhere in the cube only
    if it is >= 0.  p.p - 2 p.lo - ext sum(p) - v.v + v.lo + v.hi + ext sad(p, v); the last axis holds r, g, b and the others broadcast"""
    p, lo, v = np.asarray(pivot, np.int64), np.asarray(lo, np.int64), np.asarray(v, np.int64)
    hi = lo + ext
    return ((p * p).sum(-1) - 2 * (p * lo).sum(-1) - ext * p.sum(-1) - (v * v).sum(-1) + (v * lo).sum(-1) + (v * hi).sum(-1)
            + ext * np.abs(p - v).sum(-1))


def pivot(cent, members, lo, ext):
    """the member nearest the cube's centre lo + (ext + 1) / 2, the lowest id among equals (members ascending)"""
    members = np.asarray(members, np.int64)
    centre = np.asarray(lo, np.int64) + (ext + 1) // 2
    d = ((np.asarray(cent, np.int64)[members] - centre) ** 2).sum(-1)
    return int(members[np.argmin(d)])   # (argmin: the first minimum)


def _kept(cent, members, los, ext):
    """for every cube of los (C, 3): -> (pivot ids (C,), kept (C, n) bool over the members)"""
    cent = np.asarray(cent, np.int64)
    members = np.asarray(members, np.int64)
    los = np.asarray(los, np.int64).reshape(-1, 3)
    mc = cent[members]
    d = ((mc[None, :, :] - (los + (ext + 1) // 2)[:, None, :]) ** 2).sum(-1)
    piv = members[np.argmin(d, axis=1)]
    return piv, worst(cent[piv][:, None, :], los[:, None, :], ext, mc[None, :, :]) >= 0


def super_list(cent, sup):
    """the ids ps_build_lists / build_super keep for super-cell sup (ascending)"""
    K = len(cent)
    _, keep = _kept(cent, np.arange(K), super_box(sup), SUPER_EXT)
    return np.nonzero(keep[0])[0]


def cell_candidates(cent, cell, members=None):
    """the ids ps_row_build_list / build_candidates keep for the cell out of `members` (a super-cell's list), or ps_row_build_table /
    build_candidates on the table (members None) out of all K"""
    members = np.arange(len(cent)) if members is None else np.asarray(members, np.int64)
    _, keep = _kept(cent, members, cell_box(cell), CELL_EXT)
    return members[keep[0]]


def iteration_lists(cent, cells, slotless=()):
    """One full-schedule build over the occupied cells (ascending ids) -> (sizes {sup: members of its list}, candidates per cell as the
    persistent launch builds them, ... as the launches build them): lists of id arrays.  slotless: cells of the persistent launch without a
    shared list (they build from the table)."""
    cent = np.asarray(cent, np.int64)
    cells = np.asarray(cells, np.int64)
    K = len(cent)
    sizes, ps, cl = {}, [None] * len(cells), [None] * len(cells)
    slotless = set(int(c) for c in slotless)
    table = np.arange(K)
    sups = cells >> kSuperShift
    for sup in np.unique(sups):
        idx = np.nonzero(sups == sup)[0]
        S = super_list(cent, sup)
        sizes[int(sup)] = len(S)
        los = cell_box(cells[idx])
        _, from_list = _kept(cent, S, los, CELL_EXT)
        _, from_table = _kept(cent, table, los, CELL_EXT)
        for n, i in enumerate(idx):
            a, b = S[from_list[n]], table[from_table[n]]
            ps[i] = a if len(S) <= kPsScap and int(cells[i]) not in slotless else b
            cl[i] = a if len(S) <= km_scap(K) else b
    return sizes, ps, cl


# ---- the oracle's run, step by step
def trajectory(pts, w, K, init=None):
    """-> (tabs, labs, run): tabs[j] the centroid table assign step j uses and tabs[N] the final one, labs[j] the labels step j starts from and
    labs[N] the final ones (N = run["iterations"]); run is warm_ref.lloyd_from's result (with init None: from the reference's own init, the
    ordinary run)"""
    pts = np.ascontiguousarray(pts, np.int32).reshape(-1, 3)
    trace = []
    start = W.ref_init_centroids(pts, K) if init is None else init
    rc, run = W.lloyd_from(O.PT_RGBW, pts, w, K, start, trace=trace)
    assert rc in (O.OK, O.FEW_ACTIVE), rc
    tabs = [t for t, _ in trace] + [run["centroids"]]
    labs = [l for _, l in trace] + [run["labels"]]
    return tabs, labs, run


def moved(tabs):
    """centroids changed by each update: the kernels' nS in front of assign step j + 1"""
    return [int((tabs[j + 1] != tabs[j]).any(axis=1).sum()) for j in range(len(tabs) - 1)]


def movers_by_pair(before, after, cells):
    """points per (cell, old label, new label) among those that change label -> {(cell, old, new): points}"""
    mv = np.nonzero(np.asarray(before) != np.asarray(after))[0]
    out = {}
    for c, o, n in zip(np.asarray(cells)[mv], np.asarray(before)[mv], np.asarray(after)[mv]):
        out[(int(c), int(o), int(n))] = out.get((int(c), int(o), int(n)), 0) + 1
    return out


# ---- who owns what in the persistent launch (k_cell_scan's ne_cost, k_ps_ranges, the set-up of k_rgbw_persist)
def ps_grid(U, blocks=None, cus=256):
    """ps_grid_for: one block per CU, CNIIC_KM_PS_BLOCKS instead, never more than one block per 512 colours"""
    return min(blocks if blocks else cus, max(1, -(-U // 512)), 1024)


def ps_ranges(cells, points_per_cell, G):
    """cells: the occupied cells' ids ascending, with their populations -> dict(cb chunk boundaries, blocks: per block the cell INDICES it owns in
    its own order, ncells, runs: per block its (chunk, super-cell) runs -- each claims one of the kPsSlotsMax shared lists -- slotless: the cell ids
    beyond the last slot, split: super-cells whose cells lie in more than one chunk, refused: what k_ps_ranges' fail word says)"""
    cells = np.asarray(cells, np.int64)
    n = np.asarray(points_per_cell, np.int64)
    M, NC = len(cells), G * kPsChunks
    sweeps = -(-n // (64 * kSweep))
    ne_cost = np.concatenate([[0], np.cumsum(sweeps)]) * kCellSweepCost + np.arange(M + 1) * kCellFixedCost   # ne_cost[m]: the cost in front of cell m
    total = int(ne_cost[M])
    cb = np.array([int(np.searchsorted(ne_cost[:M], total * g // NC, "left")) for g in range(NC)] + [M], np.int64)
    blocks, runs, slotless = [], [], []
    chunk_of = np.zeros(M, np.int64)
    for i in range(NC):
        chunk_of[cb[i]:cb[i + 1]] = i
    for b in range(G):
        own, nrun = [], 0
        for r in range(kPsChunks):
            lo, hi = cb[r * G + b], cb[r * G + b + 1]
            for m in range(lo, hi):
                if m == lo or (cells[m - 1] >> kSuperShift) != (cells[m] >> kSuperShift):
                    nrun += 1
                if nrun > kPsSlotsMax:
                    slotless.append(int(cells[m]))
                own.append(m)
        blocks.append(np.array(own, np.int64))
        runs.append(nrun)
    sups = cells >> kSuperShift
    split = [int(s) for s in np.unique(sups) if len(np.unique(chunk_of[sups == s])) > 1]
    ncells = [len(b) for b in blocks]
    refused = any(c > kPsMaxCells or kPsOffCell + ps_cell_bytes(c) > kPsDynBytes for c in ncells)
    return dict(cb=cb, blocks=blocks, ncells=ncells, runs=runs, slotless=slotless, split=split, refused=refused)


# ---- the cases of tests/test_rgbw_limits.py
def pts_of_keys(keys):
    return W.pts_of_keys(keys)


def cube_colours(lo, side, n, seed):
    """n distinct colours of the cube [lo, lo + side)^3 -> ascending keys"""
    pick = np.sort(np.random.default_rng(seed).choice(side ** 3, n, replace=False))
    rgb = np.stack([pick // (side * side), (pick // side) % side, pick % side], axis=1) + np.asarray(lo, np.int64)
    return np.sort(key_of(rgb))


def _ones(keys):
    return np.ones(len(keys), np.uint32)


A_CUBE = (96, 64, 160)
A_KS = (1, 2, 63, 64, 65, 96, 97, 255, 256)
H_MAXSKIP = (0, 1, 8, 9, 20, 21)   # CNIIC_KM_MAXSKIP on the K = 256 run of case a: 0, 1, and v - 1, v for v = 9 and 21
E_POPULATIONS = (1, 255, 256, 257, 511, 512)
E_WEIGHTS = (1, 254, 255, 256, 1 << 31, (1 << 32) - 1)


def _case_a(K):
    keys = cube_colours(A_CUBE, 32, 6000, 8)
    return dict(keys=keys, w=_ones(keys), K=K)


def _case_b(first):
    """two far super-cells; `first` centroids placed on colours of the first blob, 256 - first on colours of the second"""
    ka, kb = cube_colours((0, 0, 0), 32, 3000, 2), cube_colours((224, 224, 224), 32, 3000, 3)
    keys = np.concatenate([ka, kb])
    rng = np.random.default_rng(first)
    init = np.concatenate([pts_of_keys(np.sort(rng.choice(ka, first, replace=False))), pts_of_keys(np.sort(rng.choice(kb, 256 - first, replace=False)))])
    return dict(keys=keys, w=_ones(keys), K=256, init=init)


C_CELL, C_FAR = (40, 80, 120), (200, 16, 240)


def _case_c(K, near=None):
    """the 512 colours of one cell, random weights; near: that many of K centroids placed in the cell, the others on a far cell of 64 colours
    (near = K: all of them on colours of the cell, and no far cell)"""
    keys = cube_colours(C_CELL, 8, 512, 4)
    init = None
    if near == K:
        init = pts_of_keys(np.sort(np.random.default_rng(near).choice(keys, near, replace=False)))
    elif near is not None:
        far = cube_colours(C_FAR, 8, 64, 5)
        rng = np.random.default_rng(near)
        init = np.concatenate([pts_of_keys(np.sort(rng.choice(keys, near, replace=False))), pts_of_keys(np.sort(rng.choice(far, K - near, replace=False)))])
        keys = np.sort(np.concatenate([keys, far]))
    w = np.random.default_rng(6).integers(1, 1000, len(keys)).astype(np.uint32)
    return dict(keys=keys, w=w, K=K, init=init)


def _case_e():
    """cells of 1, 255, 256, 257, 511 and 512 colours side by side in one super-cell, every weight of E_WEIGHTS on every sixth colour"""
    parts = [cube_colours((64 + 8 * (i // 2), 96 + 8 * (i % 2), 128), 8, n, 10 + i) for i, n in enumerate(E_POPULATIONS)]
    keys = np.sort(np.concatenate(parts))
    w = np.array([E_WEIGHTS[i % 6] for i in range(len(keys))], np.uint32)
    return dict(keys=keys, w=w, K=12)


def _case_f(nsup, per=1, K=8, blocks=1):
    """`per` colours, each in a cell of its own, in each of the first nsup super-cells of a shuffled order"""
    rng = np.random.default_rng(nsup + per)
    sups = np.sort(rng.permutation(512)[:nsup])
    keys = []
    for s in sups:
        for c in rng.permutation(64)[:per]:
            keys.append(key_of(cell_box((int(s) << kSuperShift) | int(c)) + rng.integers(0, 8, 3)))
    keys = np.sort(np.array(keys, np.uint32))
    return dict(keys=keys, w=rng.integers(1, 50, len(keys)).astype(np.uint32), K=K, blocks=blocks)


def _case_g(ncells, blocks=1):
    """one colour in each of ncells cells (a shuffled choice of the 32768)"""
    rng = np.random.default_rng(7)
    cells = np.sort(rng.permutation(32768)[:ncells])
    keys = np.sort(key_of(cell_box(cells) + rng.integers(0, 8, (ncells, 3))))
    return dict(keys=keys, w=rng.integers(1, 50, ncells).astype(np.uint32), K=16, blocks=blocks)


def g_two_cells():
    """the cell count at which, with two blocks, k_ps_ranges gives the larger block exactly kPsMaxCells cells (every cell costs the same)"""
    for M in range(2 * kPsMaxCells - 48, 2 * kPsMaxCells + 1):
        if max(ps_ranges(np.arange(M), np.ones(M), 2)["ncells"]) == kPsMaxCells:
            return M
    raise AssertionError("no cell count gives a block of exactly kPsMaxCells cells")


def _case_j():
    keys = cube_colours((16, 200, 100), 32, 200, 8)
    return dict(keys=keys, w=np.random.default_rng(8).integers(1, 300, 200).astype(np.uint32), K=200)


CASES = {}
for _K in A_KS:
    CASES["a%d" % _K] = (_case_a, (_K,))
CASES.update({
    "b128": (_case_b, (128,)), "b129": (_case_b, (129,)),
    "c256": (_case_c, (256,)), "c256p": (_case_c, (256, 256)), "c300": (_case_c, (300,)), "c300_256": (_case_c, (300, 256)), "c300_257": (_case_c, (300, 257)),
    "d18": (_case_a, (18,)),
    "e": (_case_e, ()),
    "f32": (_case_f, (32,)), "f33": (_case_f, (33,)), "f512": (_case_f, (512, 1, 32)), "f_split": (_case_f, (512, 2, 8, 2)),
    "g2047": (_case_g, (2047,)), "g2048": (_case_g, (2048,)), "g2049": (_case_g, (2049,)), "g_two": (lambda: _case_g(g_two_cells(), 2), ()),
    "j": (_case_j, ()),
})
_CASE, _REPORT = {}, {}


def case(name):
    if name not in _CASE:
        f, args = CASES[name]
        c = dict(init=None, blocks=None)
        c.update(f(*args))
        assert len(np.unique(c["keys"])) == len(c["keys"]) and np.all(np.diff(c["keys"].astype(np.int64)) > 0)
        _CASE[name] = c
    return _CASE[name]


def report(name, lists=True):
    """everything a test asserts about a case before it runs, from the oracle's trajectory (computed once):
    run, iterations, tabs, labs, nS, cells (of every colour), occ (occupied cells), pop (their populations), ranges (K <= 256: ps_ranges at the
    grid the launch takes), and per assign step j (lists=True): sizes[j] {sup: list members}, ncand_ps[j] / ncand_cl[j] candidates per occupied
    cell as the persistent launch / the launches build them, cand_ps[j] the ids"""
    key = (name, lists)
    if key in _REPORT:
        return _REPORT[key]
    c = case(name)
    keys, K = c["keys"], c["K"]
    tabs, labs, run = trajectory(pts_of_keys(keys), c["w"], K, c["init"])
    cells = cell_of(keys)
    occ, pop = np.unique(cells, return_counts=True)
    r = dict(run=run, iterations=run["iterations"], tabs=tabs, labs=labs, nS=moved(tabs), cells=cells, occ=occ, pop=pop, ranges=None)
    if K <= 256:
        r["G"] = ps_grid(len(keys), c["blocks"])
        r["ranges"] = ps_ranges(occ, pop, r["G"])
    if lists:
        slotless = r["ranges"]["slotless"] if r["ranges"] else ()
        r["sizes"], r["cand_ps"], r["ncand_ps"], r["ncand_cl"] = [], [], [], []
        for j in range(run["iterations"]):
            sizes, ps, cl = iteration_lists(tabs[j], occ, slotless)
            r["sizes"].append(sizes)
            r["cand_ps"].append(ps)
            r["ncand_ps"].append(np.array([len(x) for x in ps]))
            r["ncand_cl"].append(np.array([len(x) for x in cl]))
    _REPORT[key] = r
    return r


def summary(name):
    """one line of figures for a case (NOTES.md quotes them)"""
    r = report(name)
    big = [max(s.values()) for s in r["sizes"]]
    return "%-9s U %5d K %3d iterations %3d  largest list %3d..%3d  candidates per cell %d..%d (persistent) %d..%d (launches)  nS %s" % (
        name, len(case(name)["keys"]), case(name)["K"], r["iterations"], min(big), max(big), min(x.min() for x in r["ncand_ps"]),
        max(x.max() for x in r["ncand_ps"]), min(x.min() for x in r["ncand_cl"]), max(x.max() for x in r["ncand_cl"]), r["nS"])


if __name__ == "__main__":
    import sys
    for nm in sys.argv[1:] or list(CASES):
        print(summary(nm), flush=True)
        rg = report(nm)["ranges"]
        if rg:
            print("          G %d cells per block %s runs %s slotless %d split %d refused %s" % (report(nm)["G"], rg["ncells"][:4], rg["runs"][:4], len(rg["slotless"]), len(rg["split"]), rg["refused"]))
