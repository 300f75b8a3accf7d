"""A numpy model of the voronoi repaint (cniic_amd/csrc/vor_paint.hpp, k_voronoi_paint_tiles and voronoi_paint in k_misc.hip), a numpy
brute force of VoronoiCluster::decode (clusterc.rs:180-186) that knows nothing of either, and the cases tests/test_vor_paint.py runs on the
GPU.  tests/test_vor_paint_cpu.py checks, without a GPU, that the model paints what the brute force paints and that every case has the
property it is named for, so a GPU test cannot pass because its case missed the target.

A case is a dict: name, w, h, xs, ys (uint64 arrays: centroid k at (xs[k], ys[k]), its colour colour(k)), and what it is built for:
route ("tiles" / "brute"), and optionally kept (the kept count of every tile), overflow (tiles whose kept list is longer than the cap),
tie = (x, y, winner id, loser id), pivot = (tile, id)."""
import numpy as np

TW, TH = 64, 32          # kVorPaintTileW, kVorPaintTileH
CAP = 256                # kVorPaintCap
MAX_K = 4096             # kVorPaintMaxK
BOUND = 1 << 14          # kVorPaintCoordBound
MARKS = ("vor_paint_tiles", "vor_paint_brute", "vor_paint_overflow")


# ------------------------------------------------------------------ the stream
def colour(k):
    """a colour per id, distinct for k < 65536: a painted pixel names the centroid that won it"""
    return (k & 255, (k >> 8) & 255, (k * 53 + 200) & 255)


def colours(K):
    k = np.arange(K)
    return np.stack([k & 255, (k >> 8) & 255, (k * 53 + 200) & 255], axis=1).astype(np.uint8)


def stream(w, h, xs, ys):
    """VoronoiCluster's stream: w, h as u32, K as u64, then per centroid x, y as u32, the u64 3 and r g b (clusterc.rs:156-164, 250-257)"""
    K = len(xs)
    rec = np.zeros((K, 19), np.uint8)
    rec[:, 0:4] = np.asarray(xs, np.uint64).astype("<u4").view(np.uint8).reshape(K, 4)
    rec[:, 4:8] = np.asarray(ys, np.uint64).astype("<u4").view(np.uint8).reshape(K, 4)
    rec[:, 8] = 3
    rec[:, 16:19] = colours(K)
    return int(w).to_bytes(4, "little") + int(h).to_bytes(4, "little") + K.to_bytes(8, "little") + rec.tobytes()


def case_stream(c):
    return stream(c["w"], c["h"], c["xs"], c["ys"])


def image_of(labels):
    return colours(int(labels.max()) + 1)[labels]


# ------------------------------------------------------------------ brute force: the first minimum of the wrapping u32 key
def brute_labels(w, h, xs, ys):
    """(h, w) ids: for each pixel the FIRST centroid with the smallest (c.x - x)^2 + (c.y - y)^2 in u32 arithmetic that wraps"""
    xs, ys = np.asarray(xs, np.uint64), np.asarray(ys, np.uint64)
    px = np.arange(w, dtype=np.uint64)[None, None, :]
    py = np.arange(h, dtype=np.uint64)[None, :, None]
    M = np.uint64(0xffffffff)
    best = best_k = None
    step = max(1, (1 << 22) // max(w * h, 1))
    for lo in range(0, len(xs), step):
        cx, cy = xs[lo:lo + step, None, None], ys[lo:lo + step, None, None]
        dx, dy = (cx - px) & M, (cy - py) & M                       # (u64 arithmetic wraps at 2^64, a multiple of 2^32)
        d = ((dx * dx & M) + (dy * dy & M)) & M
        k = d.argmin(axis=0)                                        # the first of equal minima
        dk = np.take_along_axis(d, k[None], axis=0)[0]
        if best is None:
            best, best_k = dk, k + lo
        else:
            take = dk < best                                        # a later centroid wins on `<` alone
            best, best_k = np.where(take, dk, best), np.where(take, k + lo, best_k)
    return best_k.astype(np.int64)


# ------------------------------------------------------------------ the model of the tiled kernel
def route(w, h, xs, ys):
    """the kernel voronoi_paint launches: the gate of codec.cpp (vp_sides_small, vp_coord_small) and vp_tiled_k"""
    small = w <= BOUND and h <= BOUND and bool((np.asarray(xs, np.uint64) < BOUND).all() and (np.asarray(ys, np.uint64) < BOUND).all())
    return "tiles" if small and 1 <= len(xs) <= MAX_K else "brute"


def tiles_of(w, h):
    """[(x0, x1, y0, y1)]: vp_tile_rect for every tile, in launch order"""
    return [(tx, min(w, tx + TW) - 1, ty, min(h, ty + TH) - 1) for ty in range(0, h, TH) for tx in range(0, w, TW)]


def prune(rect, xs, ys, strict=False):
    """vp_pivot_key / vp_pivot_word / vp_keep for one tile -> (pivot id, keep mask, f per centroid); the int64 values are checked against
    the bounds the header claims.  strict: the mutant that keeps on f > 0 (and the pivot's own site, whose f is 0: a bare `f > 0` drops the
    pivot itself and paints nothing right)"""
    x0, x1, y0, y1 = rect
    cx, cy = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    dx, dy = 2 * cx - (x0 + x1), 2 * cy - (y0 + y1)
    key = dx * dx + dy * dy
    assert int(key.max()) < 1 << 31
    pivot = int(((key << 12) | np.arange(len(cx))).argmin())
    px, py = int(cx[pivot]), int(cy[pivot])
    ex, ey = px - cx, py - cy
    t = [ex * (cx + px - 2 * x0), ex * (cx + px - 2 * x1), ey * (cy + py - 2 * y0), ey * (cy + py - 2 * y1)]
    assert max(int(np.abs(v).max()) for v in t) < 1 << 30
    f = np.maximum(t[0], t[1]) + np.maximum(t[2], t[3])
    return pivot, ((f > 0) | ((ex == 0) & (ey == 0)) if strict else f >= 0), f


def model(w, h, xs, ys, strict=False, cap_lt=False):
    """the tiled kernel's steps on the CPU -> (labels (h, w), [pivot per tile], [kept count per tile]).  A tile whose list fits paints the
    first minimum over its kept centroids in ascending id, true arithmetic; any other the wrapping brute force.  strict / cap_lt: the
    mutants `f > 0` and `n < cap`"""
    assert route(w, h, xs, ys) == "tiles"
    cx, cy = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    labels = np.zeros((h, w), np.int64)
    pivots, kept, brute = [], [], None
    for rect in tiles_of(w, h):
        x0, x1, y0, y1 = rect
        pivot, keep, _ = prune(rect, xs, ys, strict)
        ids = np.flatnonzero(keep)
        pivots.append(pivot)
        kept.append(len(ids))
        if (len(ids) < CAP) if cap_lt else (len(ids) <= CAP):
            px, py = np.arange(x0, x1 + 1)[None, None, :], np.arange(y0, y1 + 1)[None, :, None]
            d = (cx[ids, None, None] - px) ** 2 + (cy[ids, None, None] - py) ** 2
            labels[y0:y1 + 1, x0:x1 + 1] = ids[d.argmin(axis=0)]
        else:
            brute = brute_labels(w, h, xs, ys) if brute is None else brute
            labels[y0:y1 + 1, x0:x1 + 1] = brute[y0:y1 + 1, x0:x1 + 1]
    return labels, pivots, kept


def overflow_of(kept, cap_lt=False):
    return sum((n >= CAP) if cap_lt else (n > CAP) for n in kept)


def expected_marks(c):
    """what the stage marks of the decode must read: (tiles, brute, overflow)"""
    if route(c["w"], c["h"], c["xs"], c["ys"]) == "brute":
        return (0, 1, 0)
    return (1, 0, overflow_of(model(c["w"], c["h"], c["xs"], c["ys"])[2]))


# ------------------------------------------------------------------ the cases
def _case(name, w, h, pts, **kw):
    pts = np.asarray(pts, np.uint64).reshape(-1, 2)
    return dict(name=name, w=int(w), h=int(h), xs=pts[:, 0].copy(), ys=pts[:, 1].copy(), **kw)


# image, tie pixel, C, P: d(tie, C) = d(tie, P) = 25, P is the pivot of the tie pixel's tile, and the pivot is strictly nearer than C at every
# other pixel of that tile: f(C) = 0, reached at the tile's corner alone
CORNER_ROWS = (((128, 32), (63, 0), (68, 0), (60, 4)),
               ((128, 32), (64, 0), (59, 0), (67, 4)),
               ((128, 32), (63, 31), (68, 31), (60, 27)),
               ((128, 32), (64, 31), (59, 31), (67, 27)),
               ((100, 32), (99, 0), (104, 0), (96, 4)))


def corner_ties():
    """the table's rows, their transposes, and each with the ids swapped.  tie = (x, y, winner, loser); pivot_id: the id of P"""
    res = []
    for i, ((w, h), t, c, p) in enumerate(CORNER_ROWS):
        for tr in (False, True):
            if tr:
                (w_, h_), t_, c_, p_ = (h, w), t[::-1], c[::-1], p[::-1]
            else:
                (w_, h_), t_, c_, p_ = (w, h), t, c, p
            name = "row %d%s" % (i, " transposed" if tr else "")
            res.append(_case(name + ", C first", w_, h_, [c_, p_], route="tiles", tie=(t_[0], t_[1], 0, 1), pivot_id=1, c_id=0))
            res.append(_case(name + ", P first", w_, h_, [p_, c_], route="tiles", tie=(t_[0], t_[1], 0, 1), pivot_id=0, c_id=1))
    return res


def _tile_sites(rng, n, x0=0, y0=0):
    """n distinct pixels of the tile at (x0, y0), in shuffled order"""
    at = rng.permutation(TW * TH)[:n]
    return [(x0 + int(a) % TW, y0 + int(a) // TW) for a in at]


def list_cap():
    rng = np.random.default_rng(256)
    res = []
    for n in (255, 256, 257):
        res.append(_case("one tile, %d sites" % n, TW, TH, _tile_sites(rng, n), route="tiles", kept=[n], overflow=int(n > CAP)))
    for n in (256, 257):
        pts = _tile_sites(rng, n) + [(5000 + j, 6000) for j in range(44)]
        pts = [pts[i] for i in rng.permutation(len(pts))]
        res.append(_case("one tile, %d sites and 44 far ones" % n, TW, TH, pts, route="tiles", kept=[n], overflow=int(n > CAP)))
    # four tiles: 257 distinct sites in the corner 19 x 14 of tile 0 (all kept there) and one site in each other tile, near enough to each
    # pixel of its tile to be strictly nearer than any site of the corner: those tiles keep their pivot and little else
    at = rng.permutation(19 * 14)[:257]
    pts = [(int(a) % 19, int(a) // 19) for a in at] + [(80, 16), (16, 40), (80, 40)]
    pts = [pts[i] for i in rng.permutation(len(pts))]
    res.append(_case("four tiles, one overflows", 2 * TW, 2 * TH, pts, route="tiles", overflow=1))
    return res


def k_limits():
    rng = np.random.default_rng(4096)
    w, h = 130, 70
    res = [_case("K = 1", w, h, [(17, 60)], route="tiles", overflow=0)]
    for K in (255, 256, 257):
        pts = np.stack([rng.integers(0, w, K), rng.integers(0, h, K)], axis=1)
        pts[K // 2:K // 2 + 20] = pts[:20]                                  # duplicated sites: the lower id wins
        res.append(_case("K = %d scattered" % K, w, h, pts, route="tiles"))
    for K in (4096, 4097):
        r = "tiles" if K <= MAX_K else "brute"
        # dense: drawn from the image's 9100 pixels, so most sites exist more than once and every tile overflows
        pts = np.stack([rng.integers(0, w, K), rng.integers(0, h, K)], axis=1)
        centre = [(31, 15), (32, 15), (31, 16), (32, 16)]                   # the four pixels about tile 0's centre, key 2 each
        for k in range(K - 1):
            while tuple(pts[k]) in centre:
                pts[k] = (rng.integers(0, w), rng.integers(0, h))
        pts[K - 1] = centre[0]                                              # the last id alone is nearest tile 0's centre
        res.append(_case("K = %d dense" % K, w, h, pts, route=r, **({"pivot": (0, K - 1)} if r == "tiles" else {})))
        # sparse: drawn from ten times the image each way, so a tile's list stays short; every site of the first half twice
        pts = np.stack([rng.integers(0, 10 * w, K), rng.integers(0, 10 * h, K)], axis=1)
        pts[K // 2:2 * (K // 2)] = pts[:K // 2]
        keep = [k for k in range(K - 1) if tuple(pts[k]) in centre]
        for k in keep:
            pts[k] = (10 * w - 1, 10 * h - 1)
        pts[K - 1] = centre[0]
        res.append(_case("K = %d sparse" % K, w, h, pts, route=r, **({"pivot": (0, K - 1), "overflow": 0} if r == "tiles" else {})))
    return res


def coordinate_switch():
    rng = np.random.default_rng(16383)
    res = []
    inside = [(int(rng.integers(0, 70)), int(rng.integers(0, 40))) for _ in range(6)]
    for name, far in (("x", lambda v: (v, 20)), ("y", lambda v: (35, v)), ("x and y", lambda v: (v, v))):
        for v in (BOUND - 1, BOUND):
            r = "tiles" if v < BOUND else "brute"
            res.append(_case("%s = %d beside sites inside" % (name, v), 70, 40, inside[:3] + [far(v)] + inside[3:], route=r))
            # every centroid out there: the distances, the pivot key and the products of the prune are as large as they get.  The first
            # two split the image between them (at v = 16383: d0 - d1 = 4 - 2 x + 362 y, and 166 (y - x) for "x and y") with ties on the line
            near = {"x": [(v, 0), (v - 1, 181), (v, 0), (v - 40, 1200)], "y": [(0, v), (181, v - 1), (0, v), (1200, v - 40)],
                    "x and y": [(v, v - 83), (v - 83, v), (v, v), (v, v - 83)]}[name]
            res.append(_case("%s = %d, all centroids far" % (name, v), 70, 40, near, route=r))
    for n in (BOUND, BOUND + 1):
        r = "tiles" if n <= BOUND else "brute"
        ends = [0, n - 1, 1, n - 2, n - 1, 0] + [int(v) for v in rng.integers(0, n, 27)]
        res.append(_case("%d x 1" % n, n, 1, [(v, 0) for v in ends], route=r))
        res.append(_case("1 x %d" % n, 1, n, [(0, v) for v in ends], route=r))
        res.append(_case("%d x 1, centroids off the row" % n, n, 1, [(v, (7 * i) % 11) for i, v in enumerate(ends)], route=r))
    # (65536 + a)^2 = 131072 a + a^2 modulo 2^32: a tie with (3, 1) at x = 3; (2^31 + a)^2 = a^2: (2^31 + 10, 2^31) is (10, 0) everywhere
    res.append(_case("wrapping to a tie", 70, 40, [(65536 + 3, 1), (3, 1), (2 ** 31 + 10, 2 ** 31), (10, 0)], route="brute"))
    res.append(_case("wrapping to a tie, the small ones first", 70, 40, [(3, 1), (65536 + 3, 1), (10, 0), (2 ** 31 + 10, 2 ** 31)], route="brute"))
    return res


CLIPPED_SIZES = ((1, 1), (1, 300), (300, 1), (63, 31), (64, 32), (65, 33), (5, 200), (200, 5))


def clipped_tiles():
    rng = np.random.default_rng(6432)
    res = []
    for w, h in CLIPPED_SIZES:
        pts = [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(4)]
        pts += [(int(rng.integers(0, 3 * w + 1)), int(rng.integers(0, 3 * h + 1))) for _ in range(4)]
        mirrored = []
        for x0, x1, y0, y1 in (tiles_of(w, h)[0], tiles_of(w, h)[-1]):      # a pair mirrored about the tile's centre: equal pivot keys
            a, b = int(rng.integers(0, x1 - x0 + 1)), int(rng.integers(0, y1 - y0 + 1))
            mirrored += [(x0 + a, y0 + b), (x1 - a, y1 - b)]
        pts = mirrored[:2] + pts + mirrored[2:]
        res.append(_case("%d x %d" % (w, h), w, h, pts, route="tiles", overflow=0, mirrored=(0, 1)))
        res.append(_case("%d x %d, the pair alone" % (w, h), w, h, mirrored[:2], route="tiles", overflow=0, mirrored=(0, 1)))
    return res


def lattice_ties():
    rng = np.random.default_rng(9648)
    res = []
    for step in (2, 4):
        pts = np.array([(x, y) for y in range(0, 48, step) for x in range(0, 96, step)])
        pts = pts[rng.permutation(len(pts))]
        res.append(_case("lattice of spacing %d" % step, 96, 48, pts, route="tiles"))
        res.append(_case("lattice of spacing %d, every site twice" % step, 96, 48, np.concatenate([pts, pts[rng.permutation(len(pts))]]), route="tiles"))
    return res


SWEEP_SEED, SWEEP_CASES = 20261021, 200


def sweep():
    """200 cases from one seed: sides 1 .. 200 (drawn again while the image has 20 000 pixels or more), K 1 .. 600, coordinates from a mix
    of distributions"""
    rng = np.random.default_rng(SWEEP_SEED)
    res = []
    for i in range(SWEEP_CASES):
        while True:
            w, h = int(rng.integers(1, 201)), int(rng.integers(1, 201))
            if w * h < 20000:
                break
        K = int(rng.integers(1, 601))
        kind = rng.integers(0, 4, K) if i % 3 else np.full(K, i // 3 % 4)     # mixed within a case, or one kind for the whole case
        xs, ys = np.zeros(K, np.uint64), np.zeros(K, np.uint64)
        step = int(rng.integers(2, 6))
        for k in range(K):
            if kind[k] == 0:
                x, y = rng.integers(0, w), rng.integers(0, h)
            elif kind[k] == 1:
                x, y = rng.integers(0, 3 * w + 1), rng.integers(0, 3 * h + 1)
            elif kind[k] == 2:
                x, y = BOUND - 1 + rng.integers(-2, 3), BOUND - 1 + rng.integers(-2, 3)
                if rng.integers(0, 2):
                    x = rng.integers(0, w)
            else:
                x, y = step * rng.integers(0, w // step + 1), step * rng.integers(0, h // step + 1)
            xs[k], ys[k] = x, y
        if i % 2 == 1:                                                        # keep the far coordinates inside the bound: the tiled kernel at its edge
            xs, ys = np.minimum(xs, BOUND - 1), np.minimum(ys, BOUND - 1)
        res.append(dict(name="sweep %d" % i, w=w, h=h, xs=xs, ys=ys, route=route(w, h, xs, ys)))
    return res


def destinations():
    return [corner_ties()[0], list_cap()[1], list_cap()[4]]


GROUPS = (("corner", corner_ties), ("cap", list_cap), ("k", k_limits), ("coords", coordinate_switch), ("clipped", clipped_tiles), ("lattice", lattice_ties))
