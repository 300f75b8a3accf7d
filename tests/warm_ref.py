"""The reference for K-means from given centroids and for a palette's fit (include/cniic_hip.h: "K-means from given centroids",
cniic_palette_fit_frames_var), restated from the oracle's public pieces only.

lloyd_from is oracle/kmeans.c:281-306 (mode L) with lines 282-288 -- init_centroids -- replaced by a copy of the given centroids and
nothing else: init_labels, then kmeans_step / kmeans_finalize until a step moves nobody, the iteration number handed to finalize
being the count BEFORE the increment.  The streams are the reference's own serialisations of such a run's result.
"""
import struct

import numpy as np

import oracle_lib as O

DIM = {O.PT_RGBW: 3, O.PT_XYRGB: 5}


def lloyd_from(kind, pts, weight, K, init, seed=O.DEFAULT_SEED, max_iters=0, trace=None):
    """-> (rc, dict(rc, centroids int32 (K, D), labels, members, iterations, empty_reseeds, moved_last, active)); rc is OK or FEW_ACTIVE (the
    results are there in both cases, as from the library), or TOO_FEW_POINTS with no results.
    trace: a list that receives, per assign step, (the centroid table the step used, the labels it started from)"""
    D = DIM[kind]
    pts = np.ascontiguousarray(pts, np.int32).reshape(-1, D)
    n = pts.shape[0]
    if n // K == 0:
        return O.TOO_FEW_POINTS, None                       # kmeans.c:271
    labels = O.init_labels(n, K)                            # kmeans.c:281
    cent = np.array(init, np.int32).reshape(K, D).copy()    # (282-288 replaced)
    iterations = reseeds = 0
    members = np.zeros(K, np.uint64)
    changed = 1
    while changed:                                          # kmeans.c:292
        if trace is not None:
            trace.append((cent.copy(), labels.copy()))
        r = O.kmeans_step(kind, pts, weight, K, cent, labels)                                        # :298
        labels, members, changed = r["labels"], r["members"], r["changed"]
        cent, res = O.kmeans_finalize(kind, pts, K, seed, iterations, r["sums"], r["wsum"], members)   # :302, the count before the increment
        reseeds += res                                      # :303
        iterations += 1                                     # :305
        if max_iters and iterations >= max_iters:           # :306
            break
    # check_enough_active_clusters (kmeans.rs:41-57, kmeans.c:428-434) on the members of the last step; the run's results stand either way
    active = int((members > 0).sum())
    rc = O.FEW_ACTIVE if active < min(int(0.99 * float(K)), n) else O.OK
    return rc, dict(rc=rc, centroids=cent, labels=labels, members=members, iterations=iterations, empty_reseeds=reseeds, moved_last=changed, active=active)


def ref_init_centroids(pts, K):
    """init_centroids (kmeans.rs:101-108, kmeans.c:282-288): the first element of each chunk"""
    pts = np.asarray(pts)
    n = pts.shape[0]
    ppc = n // K
    return np.stack([pts[n - (c + 1) * ppc if c < K - 1 else 0] for c in range(K)]).astype(np.int32)


def keys_of(img):
    p = np.asarray(img).reshape(-1, 3).astype(np.uint32)
    return (p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2]


def pts_of_keys(keys):
    keys = np.asarray(keys, np.uint32)
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=1).astype(np.int32)


def colour_points(imgs):
    """count_freqs over the pixels of one image or of several (clusterc.rs:21): ascending keys = the point list, pixel counts = the weights"""
    if isinstance(imgs, np.ndarray):
        imgs = [imgs]
    keys, counts = O.count_freqs(np.concatenate([keys_of(im) for im in imgs]))
    return keys, counts.astype(np.uint32)


def xy_pts(img):
    h, w = img.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    return np.concatenate([x.reshape(-1, 1), y.reshape(-1, 1), img.reshape(-1, 3)], axis=1).astype(np.int32)


def colorpos(c5):
    """(K, 5) x, y, r, g, b -> K cniic_colorpos entries"""
    from cniic_amd import _lib
    c5 = np.asarray(c5).reshape(-1, 5)
    out = np.zeros(c5.shape[0], _lib.COLORPOS)
    out["x"], out["y"], out["rgb"] = c5[:, 0], c5[:, 1], c5[:, 2:5]
    return out


def c5_of(cp):
    return np.concatenate([cp["x"].reshape(-1, 1), cp["y"].reshape(-1, 1), cp["rgb"].reshape(-1, 3)], axis=1).astype(np.int32)


def remap(img, keys, labels, cent):
    """reduced_colors.get(original colour) for every pixel (clusterc.rs:43-47)"""
    idx = np.searchsorted(keys, keys_of(img))
    return np.asarray(cent, np.int32)[labels[idx]].astype(np.uint8).reshape(img.shape)


def cc_stream(img, keys, labels, cent):
    """ClusterColors::encode's stream (clusterc.rs:31-52): Hufman.encode of the remapped image"""
    rc, data, _ = O.encode("hufman", remap(img, keys, labels, cent))
    assert rc == 0
    return data


def voronoi_stream(w, h, c5):
    """VoronoiCluster::encode's stream (clusterc.rs:156-164): w, h, K as usize, then x, y and a 3-byte colour vector per centroid: 16 + 19 K bytes"""
    b = struct.pack("<IIQ", w, h, len(c5))
    for c in c5:
        b += struct.pack("<IIQ", int(c[0]), int(c[1]), 3) + bytes([int(c[2]), int(c[3]), int(c[4])])
    return b


def palette_labels(cent, px):
    """THE RULE: the entry nearest in squared integer distance, the lowest index among equals -> (labels, squared distances), int64"""
    cent = np.asarray(cent, np.int64).reshape(-1, 3)
    px = np.asarray(px, np.int64).reshape(-1, 3)
    lab = np.empty(px.shape[0], np.int64)
    dist = np.empty(px.shape[0], np.int64)
    for a in range(0, px.shape[0], 1 << 14):
        d = ((px[a:a + (1 << 14), None, :] - cent[None, :, :]) ** 2).sum(axis=2)
        lab[a:a + (1 << 14)] = d.argmin(axis=1)   # (argmin: the first minimum)
        dist[a:a + (1 << 14)] = d.min(axis=1)
    return lab, dist


def fit(cent, frames):
    """-> (sse per frame, pixels per entry over all frames), numpy brute force in int64"""
    K = np.asarray(cent).reshape(-1, 3).shape[0]
    sse, pixels = [], np.zeros(K, np.int64)
    for f in frames:
        lab, dist = palette_labels(cent, f)
        sse.append(int(dist.sum()))
        pixels += np.bincount(lab, minlength=K)
    return np.array(sse, np.uint64), pixels.astype(np.uint64)
