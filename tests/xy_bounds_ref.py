"""A numpy restatement of the box bound of the tiled 5-D K-means (cniic_amd/csrc/k_kmeans_xyrgb.hip, xy_bounds.hpp), for tests that must
KNOW a case crosses a list capacity before they run it (tests/test_xyrgb_limits.py, tests/test_xyrgb_arith_cpu.py).

The image is cut into 64 x 16 tiles, grouped 4 x 4 into super-tiles.  A box = pixel extents and the min / max of each colour channel over its
pixels.  Pivot = the centroid nearest the box centre ((lo + hi) >> 1 per dimension), lowest id first.  Centroid v is kept against pivot p when
    sum_d max((p_d - v_d) (v_d + p_d - 2 lo_d), (p_d - v_d) (v_d + p_d - 2 hi_d)) >= 0,
i.e. when the pivot is not strictly nearer than v at every point of the box.  The super-tile's list is what is kept of all K centroids
against the super-tile's box; a tile's list is what is kept of THAT list against the tile's box, with the pivot chosen from it.  The centroids
are the initial ones (kmeans.rs:101-108: the first pixel of chunk k of the pixel list cut from its end), so the counts are those of iteration 0.
All in int64: nothing here can wrap."""
import numpy as np

TW, TH, STX, STY = 64, 16, 4, 4
KSCAP, MOVED_SKIP = 1024, 512   # kSCap, kXMaxMovedSkip

# (w, h, K, max_iters, least largest super-tile list, most largest super-tile list, least largest tile list): what a case is there to cross it
# crosses by a quarter of the cap at least, so that a pivot tie resolved differently cannot change the verdict
CAPACITY_CASES = [(256, 64, 2048, 6, KSCAP + KSCAP // 4, None, 128 + 128 // 4),     # kSCap and wcap = 128
                  (520, 130, 1100, 8, None, KSCAP, 256 + 256 // 4),                  # wcap = 256 only: the super-tile lists fit
                  (128, 96, 4096, 0, KSCAP + KSCAP // 4, None, 64 + 64 // 4)]        # both, with the table in memory


def case_image(w, h, K):
    from cniic_amd import synth
    return synth.photo(w, h, synth.SEED0 + w + K)


def init_centroids(img, K):
    """(K, 5) int64: x, y, r, g, b of the first pixel of chunk k; the chunks are cut from the END of the list and chunk K - 1 starts at 0"""
    h, w = img.shape[:2]
    N = h * w
    ppc = N // K
    first = np.array([N - (k + 1) * ppc if k < K - 1 else 0 for k in range(K)], np.int64)
    flat = img.reshape(-1, 3).astype(np.int64)
    return np.concatenate([(first % w)[:, None], (first // w)[:, None], flat[first]], axis=1)


def box_of(img, x0, x1, y0, y1):
    """lo, hi (5,) int64 of the pixels [x0, x1) x [y0, y1), clipped to the image"""
    h, w = img.shape[:2]
    x1, y1 = min(x1, w), min(y1, h)
    px = img[y0:y1, x0:x1].reshape(-1, 3).astype(np.int64)
    return (np.concatenate([[x0, y0], px.min(axis=0)]).astype(np.int64), np.concatenate([[x1 - 1, y1 - 1], px.max(axis=0)]).astype(np.int64))


def pivot_of(lo, hi, cent):
    """index into cent of the centroid nearest the box centre, lowest index first"""
    mid = (lo + hi) >> 1
    return int(np.argmin(((cent - mid) ** 2).sum(axis=1)))


def worst(lo, hi, piv, cent):
    """(len(cent),) int64: the maximum over the box of d(point, piv) - d(point, cent[k])"""
    d = piv[None, :] - cent
    s = cent + piv[None, :]
    return np.maximum(d * (s - 2 * lo[None, :]), d * (s - 2 * hi[None, :])).sum(axis=1)


def kept(lo, hi, cent):
    return worst(lo, hi, cent[pivot_of(lo, hi, cent)], cent) >= 0


def list_sizes(img, K):
    """-> (largest super-tile list, largest tile list) at iteration 0"""
    h, w = img.shape[:2]
    cent = init_centroids(img, K)
    big_s = big_t = 0
    for sy in range(0, h, TH * STY):
        for sx in range(0, w, TW * STX):
            lo, hi = box_of(img, sx, sx + TW * STX, sy, sy + TH * STY)
            S = cent[kept(lo, hi, cent)]
            big_s = max(big_s, len(S))
            for ty in range(sy, min(sy + TH * STY, h), TH):
                for tx in range(sx, min(sx + TW * STX, w), TW):
                    lo, hi = box_of(img, tx, tx + TW, ty, ty + TH)
                    big_t = max(big_t, int(kept(lo, hi, S).sum()))
    return big_s, big_t


# xy_create's LDS budget: the table is kept in LDS while fixed + 16 K + 16 * 64 * 18 <= 153 KiB
def lds_plan(K, lds_max=153 * 1024, scap=1024, moved_skip=512, waves=16):
    """-> (use_tab, wcap, dynamic LDS bytes) as xy_create works them out"""
    mw = (K + 63) // 64
    fixed = ((6 * K + 3) & ~3) * 4 + scap * 18 + moved_skip * 16 + waves * mw * 8
    use_tab = fixed + 16 * K + waves * 64 * 18 <= lds_max
    if use_tab:
        fixed += 16 * K
    wcap = min(256, (lds_max - fixed) // (waves * 18) // 32 * 32)
    return use_tab, wcap, fixed + waves * wcap * 18


def capacity_precondition(img, K, s_least, s_most, t_least):
    """assert that the image crosses, at iteration 0, what its case says -> (largest super-tile list, largest tile list)"""
    big_s, big_t = list_sizes(img, K)
    wcap = lds_plan(K)[1]
    assert t_least == wcap + wcap // 4, (t_least, wcap)
    assert s_least is None or big_s >= s_least, (big_s, s_least)
    assert s_most is None or big_s <= s_most, (big_s, s_most)
    assert big_t >= t_least, (big_t, t_least)
    return big_s, big_t
